// Forward-only Linear with int8 operands, dynamically quantized (ABI v18): the arithmetic of
// torch.quantization.quantize_dynamic(model, {nn.Linear}, torch.qint8) on the fbgemm engine,
// bit for bit (include/dlrm_hip.h has the rule, tests/exact_mlp8.py its numpy form).
//
//   dlrm_linear8_pack    : W [N][K] fp32 -> Wq [N][ldwq] int8 (per tensor, symmetric, zero
//                          point 0, rows zero-padded) + one device float s_w.  A min/max pass
//                          into kRangeParts partials, then a quantize pass whose workgroups each
//                          fold the partials (min and max are exact: any order, same bits).
//   dlrm_linear8_range   : min/max of X[:M][:K] into kRangeParts partials (the same pass).
//   dlrm_linear8_forward : every workgroup folds the partials and derives (s_x, inv, zp) itself
//                          in fp64 - the same sequence everywhere, so the same bits, with no
//                          one-thread launch and no host read - then runs the tile:
//     X fp32 (registers) -> d = clamp(rint(fma(x, inv, zp)), 0, 255) - zp -> packed int8 in
//     LDS (two buffers, K in steps of 64, one barrier per step) -> one 16-byte LDS read per
//     lane and fragment; Wq straight from global memory with one 16-byte load per lane and
//     fragment (prefetched one step ahead) -> v_mfma_i32_16x16x64_i8 -> int32 accumulators ->
//     y = fma(float(acc), fl(s_x * s_w), bias), ReLU.
// LDS rows are 64 B (4 chunks of 16 B); chunk c of row r sits at chunk c ^ ((r >> 2) & 3), so
// the 16 rows a 16-lane group reads land in 16 different 16-byte bank groups.  Both operands
// give lane l the 16 bytes at k = 16 (l >> 4) .. + 15 of row l & 15: whatever order the
// instruction takes those 16 in, it is the same for A and B, so every k meets its partner.
// Elements with k >= K are selected to d = 0 (and Wq's padding is 0); rows past M / N are
// clamped to the last row when read and never written.  No split-K, no atomics.
#include <cfloat>

#include "linear16_stage.hpp"

namespace dlrm {
namespace {

using l16::kBK;
using l16::kThreads;
using l16::Stage;
using l16::Tile;

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kRangeParts = 1024;  // min partials, then max partials: one workgroup each, so
                                   // a 2048-row input is two rows (two loads in flight) per thread
static_assert(2 * kRangeParts == DLRM_LINEAR8_RANGE_FLOATS && kRangeParts % 256 == 0, "partials");
constexpr int64_t kMaxK = 131072;  // 127 * 128 * K < 2^31

// ------------------------------------------------------------------ min / max --
// Every workgroup reduces a strided set of rows to one (min, max) pair; NaN is skipped
// (fminf / fmaxf), and both start at 0 because every consumer folds 0 in anyway.
// tw (a power of two <= 256) threads share a row.  VEC: 16-byte loads over the K / 4 whole
// float4 of a row (rows start on 16-byte boundaries), the K % 4 tail as element loads.
template <bool VEC>
__global__ __launch_bounds__(256) void range_kernel(int64_t M, int64_t K,
                                                    const float* __restrict__ X, int64_t ldx,
                                                    int tw, float* __restrict__ parts) {
  __shared__ float smn[4], smx[4];
  const int tid = threadIdx.x;
  const int c = tid % tw, rr = tid / tw, rpb = 256 / tw;
  float mn = 0.f, mx = 0.f;
  const int64_t K4 = VEC ? K / 4 : 0;
  for (int64_t r = int64_t(blockIdx.x) * rpb + rr; r < M; r += int64_t(gridDim.x) * rpb) {
    const float* p = X + r * ldx;
    if (VEC) {
      const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll 4
      for (int64_t k = c; k < K4; k += tw) {
        const float4 v = p4[k];
        mn = fminf(fminf(mn, v.x), fminf(fminf(v.y, v.z), v.w));
        mx = fmaxf(fmaxf(mx, v.x), fmaxf(fmaxf(v.y, v.z), v.w));
      }
    }
#pragma unroll 4
    for (int64_t k = K4 * 4 + c; k < K; k += tw) {
      const float v = p[k];
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o));
    mx = fmaxf(mx, __shfl_xor(mx, o));
  }
  if ((tid & 63) == 0) smn[tid >> 6] = mn, smx[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) {
    parts[blockIdx.x] = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
    parts[kRangeParts + blockIdx.x] = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  }
}

void launch_range(int64_t M, int64_t K, const float* X, int64_t ldx, float* parts,
                  hipStream_t s) {
  const bool vec = reinterpret_cast<uintptr_t>(X) % 16 == 0 && ldx % 4 == 0 && K >= 4;
  const int64_t cols = vec ? K / 4 : K;  // at least K % 4 < 4 <= cols threads for the tail
  int tw = 4;
  while (tw < 256 && tw < cols) tw *= 2;
  if (vec)
    hipLaunchKernelGGL(range_kernel<true>, dim3(kRangeParts), dim3(256), 0, s, M, K, X, ldx, tw,
                       parts);
  else
    hipLaunchKernelGGL(range_kernel<false>, dim3(kRangeParts), dim3(256), 0, s, M, K, X, ldx, tw,
                       parts);
}

// The fold of the partials by a 256-thread workgroup: (min(.., 0), max(.., 0)) in every thread.
__device__ __forceinline__ void fold_range(const float* __restrict__ parts, float* sh,
                                           float& mn, float& mx) {
  const int tid = threadIdx.x;
  mn = 0.f, mx = 0.f;
#pragma unroll
  for (int i = 0; i < kRangeParts / 256; ++i) {
    mn = fminf(mn, parts[tid + 256 * i]);
    mx = fmaxf(mx, parts[kRangeParts + tid + 256 * i]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o));
    mx = fmaxf(mx, __shfl_xor(mx, o));
  }
  if ((tid & 63) == 0) sh[tid >> 6] = mn, sh[4 + (tid >> 6)] = mx;
  __syncthreads();
  mn = fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
  mx = fmaxf(fmaxf(sh[4], sh[5]), fmaxf(sh[6], sh[7]));
}

// ----------------------------------------------------------------- weights --
__device__ __forceinline__ float weight_scale(float lo, float hi) {
  return fmaxf(__fdiv_rn(fmaxf(-lo, hi), 127.5f), FLT_EPSILON);
}

// One dword (4 levels) per thread and iteration; columns >= K are 0.
__global__ __launch_bounds__(256) void pack_kernel(int64_t N, int64_t K,
                                                   const float* __restrict__ W, int64_t ldw,
                                                   int32_t* __restrict__ Wq, int64_t ldq4,
                                                   const float* __restrict__ parts,
                                                   float* __restrict__ s_w_out) {
  __shared__ float sh[8];
  float lo, hi;
  fold_range(parts, sh, lo, hi);
  const float s_w = weight_scale(lo, hi);
  const float inv = __fdiv_rn(1.0f, s_w);
  if (blockIdx.x == 0 && threadIdx.x == 0) *s_w_out = s_w;
  const int64_t total = N * ldq4;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total;
       e += int64_t(gridDim.x) * 256) {
    const int64_t n = e / ldq4, k = (e % ldq4) * 4;
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int q = 0;
      if (k + j < K) {
        float t = rintf(__fmul_rn(W[n * ldw + k + j], inv));
        t = fminf(fmaxf(t, -128.f), 127.f);  // NaN -> -128, no undefined conversion
        q = int(t);
      }
      word |= uint32_t(q & 0xff) << (8 * j);
    }
    Wq[e] = int32_t(word);
  }
}

// -------------------------------------------------------------- activations --
struct QParams {
  float s_x, inv, zpf;
  int zp;
};

// torch's ChooseQuantizationParams(min, max, qmin = 0, qmax = 127) (reduce_range), in fp64
// where it is; mn <= 0 <= mx already.  The double -> float conversions are single IEEE
// roundings.  1 / fl(scale) rounds to fp32 infinity when it is >= 2^128 - 2^103, i.e. when
// fl(scale) <= 2^-128 (1 + 2^-25 + ..): 2^-128 is an fp32 subnormal and the next one above it,
// 2^-128 + 2^-149, is already past that bound, so the test is fl(scale) <= 2^-128.
__device__ __forceinline__ QParams choose_qparams(float mn, float mx) {
  const double small = double(6.1e-5f);
  double scale = (double(mx) - double(mn)) / 127.0;
  const float fs = float(scale);
  if (double(fs) <= 0x1p-128) scale = 0.1;  // 0 included
  double mnd = mn, mxd = mx;
  if (scale < small) {
    if (mn == 0.0f) {
      mxd = double(__fmul_rn(6.1e-5f, 127.0f));
    } else if (mx == 0.0f) {
      mnd = -double(__fmul_rn(6.1e-5f, 127.0f));
    } else {
      const double amp = small / scale;
      mnd *= amp;
      mxd *= amp;
    }
    scale = small;
  }
  const double qn = mnd / scale, qx = mxd / scale;
  const double z = fabs(qn) < 127.0 + fabs(qx) ? 0.0 - qn : 127.0 - qx;
  QParams q;
  q.zp = z < 0.0 ? 0 : z > 127.0 ? 127 : int(rint(z));
  if (!(z == z)) q.zp = 0;  // NaN / Inf inputs are unspecified; keep the operand a byte
  q.zpf = float(q.zp);
  q.s_x = float(scale);
  q.inv = __fdiv_rn(1.0f, q.s_x);
  return q;
}

// chunk index (16 B) of (row, chunk) in a [rows][4 chunks] int8 LDS tile
__device__ __forceinline__ int lds8_chunk(int row, int c) {
  return row * 4 + (c ^ ((row >> 2) & 3));
}

// Stage's 8 fp32 of row (tid >> 3) + 32 i at k = kbase + 8 (tid & 7) .. + 7 -> 8 levels d, as
// one 8-byte LDS store (half h = tid & 1 of chunk (tid & 7) >> 1).
template <int ROWS>
__device__ __forceinline__ void store_codes(const Stage<ROWS>& st, uint2* lds, int tid,
                                            const QParams& q, int64_t kvalid) {
#pragma unroll
  for (int i = 0; i < Stage<ROWS>::kIter; ++i) {
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float t = rintf(__fmaf_rn(st.v[i][j], q.inv, q.zpf));
      t = fminf(fmaxf(t, 0.f), 255.f);  // NaN -> 0
      int d = int(t) - q.zp;            // in [-127, 127] for finite inputs
      d = (j < kvalid) ? d : 0;         // k >= K: selected, never computed from memory
      w[j >> 2] |= uint32_t(d & 0xff) << (8 * (j & 3));
    }
    const int row = (tid >> 3) + 32 * i;
    lds[lds8_chunk(row, (tid & 7) >> 1) * 2 + (tid & 1)] = uint2{w[0], w[1]};
  }
}

template <int BM, int BN, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void linear8_kernel(
    int64_t M, int64_t N, int64_t K, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ parts, const int8_t* __restrict__ Wq, int64_t ldwq,
    const float* __restrict__ s_w_dev, const float* __restrict__ bias, int64_t bias_stride,
    int relu, float* __restrict__ Y, int64_t ldy, float* __restrict__ qparams_out, int tiles_n,
    int tiles) {
  constexpr int WTM = BM / 2, WTN = BN / 2;  // a wave's part of the tile
  constexpr int FM = WTM / 16, FN = WTN / 16;
  static_assert(BM % 32 == 0 && BN % 32 == 0, "tile");
  __shared__ i32x4 lds[2][BM * 4];
  __shared__ float sh[8];

  // consecutive tiles (n fastest: they share X rows) go to one XCD; bijective for any count
  const int orig = blockIdx.x;
  const int q8 = tiles / 8, rem = tiles % 8, xcd = orig % 8;
  const int tile = (xcd < rem ? xcd * (q8 + 1) : rem * (q8 + 1) + (xcd - rem) * q8) + orig / 8;
  const int64_t m0 = int64_t(tile / tiles_n) * BM;
  const int64_t n0 = int64_t(tile % tiles_n) * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * WTM, wn = (wave & 1) * WTN;
  const int fr = lane & 15, fc = lane >> 4;

  i32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = i32x4{0, 0, 0, 0};

  Stage<BM> sa;
  const int64_t nk = (K + kBK - 1) / kBK;
  auto fetch = [&](int64_t kt) {
    const int64_t k0 = kt * kBK;
    if (k0 + kBK <= K)
      sa.template load<ALIGNED, true>(X, ldx, m0, M, k0, K, tid);
    else
      sa.template load<ALIGNED, false>(X, ldx, m0, M, k0, K, tid);
  };
  // this lane's 16 bytes of the FN weight rows it multiplies: k0 + 16 fc < ldwq always
  const i32x4* wrow[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    int64_t n = n0 + wn + j * 16 + fr;
    n = n < N ? n : N - 1;
    wrow[j] = reinterpret_cast<const i32x4*>(Wq + n * ldwq + 16 * fc);
  }
  auto fetch_b = [&](int64_t kt, i32x4 (&b)[FN]) {
#pragma unroll
    for (int j = 0; j < FN; ++j) b[j] = wrow[j][kt * (kBK / 16)];
  };

  i32x4 bcur[FN], bnext[FN];
  if (nk > 0) {
    fetch(0);
    fetch_b(0, bcur);
  }
  float mn, mx;
  fold_range(parts, sh, mn, mx);
  const QParams qp = choose_qparams(mn, mx);
  if (orig == 0 && tid == 0 && qparams_out) {
    qparams_out[0] = qp.s_x;
    qparams_out[1] = qp.zpf;
  }
  auto commit = [&](int buf, int64_t kt) {
    store_codes<BM>(sa, reinterpret_cast<uint2*>(lds[buf]), tid, qp,
                    K - (kt * kBK + (tid & 7) * 8));
  };
  if (nk > 0) commit(0, 0);
  __syncthreads();
  for (int64_t kt = 0; kt < nk; ++kt) {
    const int buf = int(kt & 1);
    if (kt + 1 < nk) {
      fetch(kt + 1);
      fetch_b(kt + 1, bnext);
    }
    const i32x4* A = lds[buf];
    i32x4 a[FM];
#pragma unroll
    for (int i = 0; i < FM; ++i) a[i] = A[lds8_chunk(wm + i * 16 + fr, fc)];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], bcur[j], acc[i][j], 0, 0, 0);
    // the other buffer was last read in step kt - 1, which every wave left at its barrier
    if (kt + 1 < nk) {
      commit(buf ^ 1, kt + 1);
#pragma unroll
      for (int j = 0; j < FN; ++j) bcur[j] = bnext[j];
    }
    __syncthreads();
  }

  // C/D map of 16x16: col = lane & 15, row = (lane >> 4) * 4 + reg
  const float sxw = __fmul_rn(qp.s_x, *s_w_dev);
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int64_t n = n0 + wn + j * 16 + fr;
    if (n >= N) continue;
    const float bv = bias ? bias[n * bias_stride] : 0.0f;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + wm + i * 16 + fc * 4 + r;
        if (m >= M) continue;
        const float af = float(acc[i][j][r]);  // nearest even above 2^24
        float y = bias ? __fmaf_rn(af, sxw, bv) : __fmul_rn(af, sxw);
        if (relu) y = (y > 0.0f || y != y) ? y : 0.0f;  // NaN propagates, -0 -> +0
        Y[m * ldy + n] = y;
      }
    }
  }
}

// linear16's rule: the largest tile that still gives every CU two workgroups, else the smallest
Tile plan_tile(int64_t M, int64_t N, int cus) {
  for (const Tile& t : l16::kTiles)
    if (ceil_div(M, t.bm) * ceil_div(N, t.bn) >= 2 * int64_t(cus)) return t;
  return l16::kTiles[l16::kNumTiles - 1];
}

struct Fwd8Args {
  int64_t M, N, K;
  const float* X;
  int64_t ldx;
  const float* parts;
  const int8_t* Wq;
  int64_t ldwq;
  const float* s_w;
  const float* bias;
  int64_t bias_stride;
  int relu;
  float* Y;
  int64_t ldy;
  float* qparams_out;
};

template <int BM, int BN>
void launch(bool aligned, const Fwd8Args& a, hipStream_t s) {
  const int tiles_n = int(ceil_div(a.N, BN));
  const int tiles = int(ceil_div(a.M, BM)) * tiles_n;
  if (aligned)
    hipLaunchKernelGGL((linear8_kernel<BM, BN, true>), dim3(tiles), dim3(kThreads), 0, s, a.M,
                       a.N, a.K, a.X, a.ldx, a.parts, a.Wq, a.ldwq, a.s_w, a.bias, a.bias_stride,
                       a.relu, a.Y, a.ldy, a.qparams_out, tiles_n, tiles);
  else
    hipLaunchKernelGGL((linear8_kernel<BM, BN, false>), dim3(tiles), dim3(kThreads), 0, s, a.M,
                       a.N, a.K, a.X, a.ldx, a.parts, a.Wq, a.ldwq, a.s_w, a.bias, a.bias_stride,
                       a.relu, a.Y, a.ldy, a.qparams_out, tiles_n, tiles);
}

bool dispatch(Tile t, bool aligned, const Fwd8Args& a, hipStream_t s) {
#define DLRM_L8_CASE(BM, BN)          \
  if (t.bm == BM && t.bn == BN) {     \
    launch<BM, BN>(aligned, a, s);    \
    return true;                      \
  }
  DLRM_L8_CASE(128, 128)
  DLRM_L8_CASE(128, 64)
  DLRM_L8_CASE(64, 64)
  DLRM_L8_CASE(32, 64)
#undef DLRM_L8_CASE
  return false;
}

}  // namespace
}  // namespace dlrm

extern "C" size_t dlrm_linear8_pack_workspace_size(int64_t N, int64_t K) {
  (void)N, (void)K;
  return 2 * dlrm::kRangeParts * sizeof(float);
}

extern "C" int dlrm_linear8_pack(int64_t N, int64_t K, const float* W, int64_t ldw, int8_t* Wq,
                                 int64_t ldwq, float* s_w, void* workspace,
                                 size_t workspace_bytes, dlrm_stream_t stream) {
  using namespace dlrm;
  DLRM_ARG(N >= 0 && K >= 0, "dlrm_linear8_pack: negative size");
  DLRM_ARG(s_w, "dlrm_linear8_pack: null s_w");
  DLRM_ARG(N == 0 || (Wq && (K == 0 || W)), "dlrm_linear8_pack: null pointer");
  DLRM_REQUIRE(ldw >= K, DLRM_ERR_SHAPE, "dlrm_linear8_pack: ldw %lld < K %lld", (long long)ldw,
               (long long)K);
  DLRM_REQUIRE(ldwq % 64 == 0 && ldwq >= K && (N == 0 || ldwq >= 64) &&
                   reinterpret_cast<uintptr_t>(Wq) % 16 == 0,
               DLRM_ERR_SHAPE,
               "dlrm_linear8_pack: ldwq %lld must be a multiple of 64, at least K %lld, and Wq "
               "16-byte aligned",
               (long long)ldwq, (long long)K);
  DLRM_REQUIRE(workspace && workspace_bytes >= dlrm_linear8_pack_workspace_size(N, K),
               DLRM_ERR_WORKSPACE, "dlrm_linear8_pack: workspace of %zu bytes, %zu needed",
               workspace_bytes, dlrm_linear8_pack_workspace_size(N, K));
  float* parts = static_cast<float*>(workspace);
  launch_range(N, K, W, ldw, parts, as_stream(stream));
  const int64_t total = N * (ldwq / 4);
  const int grid = int(total > 0 ? (ceil_div(total, 256) < 2048 ? ceil_div(total, 256) : 2048) : 1);
  hipLaunchKernelGGL(pack_kernel, dim3(grid), dim3(256), 0, as_stream(stream), N, K, W, ldw,
                     reinterpret_cast<int32_t*>(Wq), ldwq / 4, parts, s_w);
  DLRM_LAUNCH_CHECK("dlrm_linear8_pack");
  return DLRM_OK;
}

extern "C" int dlrm_linear8_range(int64_t M, int64_t K, const float* X, int64_t ldx,
                                  float* partials, dlrm_stream_t stream) {
  using namespace dlrm;
  DLRM_ARG(M >= 0 && K >= 0, "dlrm_linear8_range: negative size");
  DLRM_ARG(partials && (M == 0 || K == 0 || X), "dlrm_linear8_range: null pointer");
  DLRM_REQUIRE(ldx >= K, DLRM_ERR_SHAPE, "dlrm_linear8_range: ldx %lld < K %lld", (long long)ldx,
               (long long)K);
  launch_range(M, K, X, ldx, partials, as_stream(stream));
  DLRM_LAUNCH_CHECK("dlrm_linear8_range");
  return DLRM_OK;
}

extern "C" int dlrm_linear8_forward(int64_t M, int64_t N, int64_t K, const float* X, int64_t ldx,
                                    const float* partials, const int8_t* Wq, int64_t ldwq,
                                    const float* s_w, const float* bias, int64_t bias_stride,
                                    int32_t relu, float* Y, int64_t ldy, float* qparams_out,
                                    dlrm_stream_t stream) {
  using namespace dlrm;
  DLRM_ARG(M >= 0 && N >= 0 && K >= 0, "dlrm_linear8_forward: negative size");
  if (M == 0 || N == 0) return DLRM_OK;
  DLRM_ARG(Y && partials && Wq && s_w && (K == 0 || X), "dlrm_linear8_forward: null pointer");
  DLRM_REQUIRE(K <= kMaxK, DLRM_ERR_UNSUPPORTED,
               "dlrm_linear8_forward: K %lld > %lld (the int32 accumulator could overflow)",
               (long long)K, (long long)kMaxK);
  DLRM_REQUIRE(ldx >= K && ldy >= N, DLRM_ERR_SHAPE,
               "dlrm_linear8_forward: ldx %lld < K %lld or ldy %lld < N %lld", (long long)ldx,
               (long long)K, (long long)ldy, (long long)N);
  DLRM_REQUIRE(ldwq % 64 == 0 && ldwq >= K && ldwq >= 64 &&
                   reinterpret_cast<uintptr_t>(Wq) % 16 == 0,
               DLRM_ERR_SHAPE,
               "dlrm_linear8_forward: ldwq %lld must be a multiple of 64, at least K %lld, and "
               "Wq 16-byte aligned",
               (long long)ldwq, (long long)K);
  const int64_t forced = tuning(DLRM_TUNE_LINEAR8_TILE);
  Tile t{int(forced / 1000), int(forced % 1000)};
  if (forced != 0) {
    DLRM_ARG(l16::known_tile(t), "dlrm_linear8_forward: DLRM_TUNE_LINEAR8_TILE %lld is not a tile",
             (long long)forced);
  }
  DLRM_REQUIRE(ceil_div(M, 32) * ceil_div(N, 64) <= INT32_MAX, DLRM_ERR_UNSUPPORTED,
               "dlrm_linear8_forward: more than 2^31 - 1 tiles");
  if (forced == 0) t = plan_tile(M, N, l16::device_cus());
  // 16-byte loads of X where every row starts on a 16-byte boundary; elements at k >= K are
  // not read on either path
  const bool aligned = reinterpret_cast<uintptr_t>(X) % 16 == 0 && ldx % 4 == 0;
  const Fwd8Args a{M, N, K, X, ldx, partials, Wq, ldwq, s_w, bias, bias_stride, relu, Y, ldy,
                   qparams_out};
  DLRM_REQUIRE(dispatch(t, aligned, a, as_stream(stream)), DLRM_ERR_UNSUPPORTED,
               "dlrm_linear8_forward: no kernel for the tile");
  DLRM_LAUNCH_CHECK("dlrm_linear8_forward");
  return DLRM_OK;
}
