// Forward-only Linear on the 16-bit MFMA with 16-bit operands IN MEMORY (added to ABI v23):
//   dlrm_linear16_pack           : W [N][K] fp32 -> Wp [N][ldwp] bf16 / fp16, r16 of every
//                                  element (the plain cast of Stage::store), columns >= K zero.
//   dlrm_linear16_forward_packed : Y = act(r16(X) Wp^T + bias); X fp32 (rounded in flight, as
//                                  dlrm_linear16_forward does) or already 16-bit; Y fp32 or
//                                  r16(y).
//   dlrm_linear16_forward_fmt    : the same kernel on the fp32 W itself (rounded in flight by
//                                  Stage<>, as dlrm_linear16_forward does) with a 16-bit X
//                                  and / or Y: the training step's forward (store16).
// The MFMA sees exactly the operand bits dlrm_linear16_forward feeds it - r16(W) was stored by
// the packer, a 16-bit X is what the layer before stored as r16(y) - in the same tile, the
// same k order (steps of 64, two 32-k slices each) and the same lane map, so the accumulators
// are bit for bit that kernel's.  What differs is how the bits get there and how they leave:
//
//   staging   a 16-bit tile moves as whole 16-byte chunks (8 elements): one global load and
//             one ds_write_b128 per chunk, ROWS / 32 chunks per thread, no conversion - half
//             the load instructions and a quarter of the staging registers of the fp32 tile.
//             The chunk lands at the swizzled slot lds_chunk(row, c) the fragment reads expect.
//             Wp's zero pad is readable, so the W tile has no tail logic at all; a 16-bit X
//             (K % 8 == 0) selects chunks with k >= K to zero without reading them.  An fp32 X
//             keeps the convert-in-flight Stage<> for the X tile only (16-byte or element loads).
//   epilogue  fp32 Y: the C/D map's element stores, as in linear16.hip.  16-bit Y: the tile
//             passes through LDS once (the operand buffers are free after the last barrier) -
//             each lane writes its r16(y) at [m][n] of a [BM][BN + 8] image, then the workgroup
//             stores whole rows as 16-byte chunks (8 consecutive n), narrower only in the chunk
//             that crosses N.  The accumulators are untouched by this, which is why it was
//             taken over issuing the MFMA with swapped operands.
// Rows >= M / >= N are clamped when read and never written.  No split-K, no atomics, no
// workspace: two calls give the same bits.
#include "linear16_stage.hpp"

namespace dlrm {
namespace {

using namespace l16;

// ------------------------------------------------------------------ packer --
// One 16-byte chunk (8 elements of one row) per thread and iteration.
template <typename T>
__global__ __launch_bounds__(256) void pack16_kernel(int64_t N, int64_t K,
                                                     const float* __restrict__ W, int64_t ldw,
                                                     typename Op16<T>::vec* __restrict__ Wp,
                                                     int64_t ldc, int vec4) {
  const int64_t total = N * ldc;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total;
       e += int64_t(gridDim.x) * 256) {
    const int64_t n = e / ldc, k = (e % ldc) * 8;
    const float* p = W + n * ldw + k;
    float v[8];
    if (vec4 && k + 8 <= K) {
      const float4 a = *reinterpret_cast<const float4*>(p);
      const float4 b = *reinterpret_cast<const float4*>(p + 4);
      v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
      v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (k + j < K) ? p[j] : 0.0f;  // columns >= K: not read
    }
    typename Op16<T>::vec h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = static_cast<T>(v[j]);  // RNE, as Stage::store
    Wp[e] = h;
  }
}

// ----------------------------------------------------------------- staging --
// (Stage16, the whole-chunk stager of a 16-bit tile, is linear16_stage.hpp's)
// kPacked: dlrm_linear16_pack's image (every row readable and zero up to the k-step's end)
enum XKind { kXF32Vec = 0, kXF32Elem = 1, kX16 = 2, kPacked = 3 };

// The stager of an operand tile (X, or W as the second operand): fp32 in memory -> Stage<>
// (rounded while it is written to LDS) ...
template <typename T, int ROWS, int XK>
struct XTile {
  Stage<ROWS> s;
  __device__ __forceinline__ void load(const void* X, int64_t ld, int64_t m0, int64_t M,
                                       int64_t k0, int64_t K, int tid) {
    const float* p = static_cast<const float*>(X);
    if (k0 + kBK <= K)
      s.template load<XK == kXF32Vec, true>(p, ld, m0, M, k0, K, tid);
    else
      s.template load<XK == kXF32Vec, false>(p, ld, m0, M, k0, K, tid);
  }
  __device__ __forceinline__ void store(typename Op16<T>::vec* lds, int tid) const {
    s.template store<T>(lds, tid);
  }
};
// ... 16-bit in memory -> whole chunks
template <typename T, int ROWS>
struct XTile<T, ROWS, kX16> {
  Stage16<T, ROWS> s;
  __device__ __forceinline__ void load(const void* X, int64_t ld, int64_t m0, int64_t M,
                                       int64_t k0, int64_t K, int tid) {
    s.template load<false>(static_cast<const T*>(X), ld, m0, M, k0, K, tid);
  }
  __device__ __forceinline__ void store(typename Op16<T>::vec* lds, int tid) const {
    s.store(lds, tid);
  }
};
// ... and the packer's image, which has no tail logic at all
template <typename T, int ROWS>
struct XTile<T, ROWS, kPacked> {
  Stage16<T, ROWS> s;
  __device__ __forceinline__ void load(const void* W, int64_t ld, int64_t n0, int64_t N,
                                       int64_t k0, int64_t K, int tid) {
    s.template load<true>(static_cast<const T*>(W), ld, n0, N, k0, K, tid);
  }
  __device__ __forceinline__ void store(typename Op16<T>::vec* lds, int tid) const {
    s.store(lds, tid);
  }
};

struct PackedArgs {
  int64_t M, N, K;
  const void* X;
  int64_t ldx;
  const void* Wp;  // WK == kPacked: the 16-bit image; else the fp32 W of dlrm_linear16_forward_fmt
  int64_t ldwp;
  const float* bias;
  int64_t bias_stride;
  int relu;
  void* Y;
  int64_t ldy;
};

template <typename T, int BM, int BN, int XK, int WK, bool Y16>
__global__ __launch_bounds__(kThreads) void linear16_packed_kernel(PackedArgs a, int tiles_n,
                                                                   int tiles) {
  using vec = typename Op16<T>::vec;
  constexpr int WTM = BM / 2, WTN = BN / 2;  // a wave's part of the tile
  constexpr int FM = WTM / 16, FN = WTN / 16;
  constexpr int YP = BN + 8;  // row pitch (elements) of the 16-bit output image in LDS
  static_assert(BM % 32 == 0 && BN % 32 == 0, "tile");
  static_assert(BM * YP * 2 <= 2 * (BM + BN) * 8 * 16, "the output image fits the operand LDS");
  __shared__ vec lds[2][(BM + BN) * 8];
  const int64_t M = a.M, N = a.N, K = a.K;

  // consecutive tiles (n fastest: they share X rows) go to one XCD; bijective for any count
  const int orig = blockIdx.x;
  const int q = tiles / 8, rem = tiles % 8, xcd = orig % 8;
  const int tile = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + orig / 8;
  const int64_t m0 = int64_t(tile / tiles_n) * BM;
  const int64_t n0 = int64_t(tile % tiles_n) * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * WTM, wn = (wave & 1) * WTN;
  const int fr = lane & 15, fc = lane >> 4;

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  XTile<T, BM, XK> sa;
  XTile<T, BN, WK> sb;
  const int64_t nk = (K + kBK - 1) / kBK;
  auto fetch = [&](int64_t kt) {
    sa.load(a.X, a.ldx, m0, M, kt * kBK, K, tid);
    sb.load(a.Wp, a.ldwp, n0, N, kt * kBK, K, tid);
  };
  auto commit = [&](int buf) {
    sa.store(lds[buf], tid);
    sb.store(lds[buf] + BM * 8, tid);
  };

  if (nk > 0) {
    fetch(0);
    commit(0);
  }
  __syncthreads();
  for (int64_t kt = 0; kt < nk; ++kt) {
    const int buf = int(kt & 1);
    if (kt + 1 < nk) fetch(kt + 1);
    const vec* A = lds[buf];
    const vec* B = lds[buf] + BM * 8;
#pragma unroll
    for (int ks = 0; ks < kBK / 32; ++ks) {
      vec fa[FM], fb[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) fa[i] = A[lds_chunk(wm + i * 16 + fr, ks * 4 + fc)];
#pragma unroll
      for (int j = 0; j < FN; ++j) fb[j] = B[lds_chunk(wn + j * 16 + fr, ks * 4 + fc)];
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = Op16<T>::mfma(fa[i], fb[j], acc[i][j]);
    }
    // the other buffer was last read in step kt - 1, which every wave left at its barrier
    if (kt + 1 < nk) commit(buf ^ 1);
    __syncthreads();
  }

  // C/D map of 16x16: col = lane & 15, row = (lane >> 4) * 4 + reg
  if constexpr (!Y16) {
    float* Y = static_cast<float*>(a.Y);
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int64_t n = n0 + wn + j * 16 + fr;
      if (n >= N) continue;
      const float bv = a.bias ? a.bias[n * a.bias_stride] : 0.0f;
#pragma unroll
      for (int i = 0; i < FM; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t m = m0 + wm + i * 16 + fc * 4 + r;
          if (m >= M) continue;
          float y = acc[i][j][r] + bv;
          if (a.relu) y = (y != y) ? y : fmaxf(y, 0.0f);  // NaN propagates
          Y[m * a.ldy + n] = y;
        }
      }
    }
  } else {
    // Every wave has left the loop's last barrier: no operand tile is read any more, and the
    // [BM][YP] image of r16(y) takes their place.  The pitch of BN + 8 elements keeps every
    // chunk 16-byte aligned and puts the four row groups of a wave 16 banks apart.
    T* img = reinterpret_cast<T*>(&lds[0][0]);
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int nl = wn + j * 16 + fr;
      const int64_t n = n0 + nl;
      const float bv = (a.bias && n < N) ? a.bias[n * a.bias_stride] : 0.0f;
#pragma unroll
      for (int i = 0; i < FM; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float y = acc[i][j][r] + bv;
          if (a.relu) y = (y != y) ? y : fmaxf(y, 0.0f);  // NaN propagates
          img[(wm + i * 16 + fc * 4 + r) * YP + nl] = static_cast<T>(y);  // RNE
        }
      }
    }
    __syncthreads();
    T* Y = static_cast<T*>(a.Y);
    constexpr int CPR = BN / 8;  // 16-byte chunks per row of the tile
    for (int e = tid; e < BM * CPR; e += kThreads) {
      const int ml = e / CPR, c = e % CPR;
      const int64_t m = m0 + ml, n = n0 + c * 8;
      if (m >= M || n >= N) continue;
      const T* src = img + ml * YP + c * 8;
      T* dst = Y + m * a.ldy + n;  // 16-byte aligned: Y is, ldy and n are multiples of 8
      if (n + 8 <= N) {
        *reinterpret_cast<vec*>(dst) = *reinterpret_cast<const vec*>(src);
      } else {
        for (int j = 0; j < int(N - n); ++j) dst[j] = src[j];  // the chunk that crosses N
      }
    }
  }
}

// linear16's rule: the largest tile that still gives every CU two workgroups, else the smallest
Tile plan_tile(int64_t M, int64_t N, int cus) {
  for (const Tile& t : kTiles)
    if (ceil_div(M, t.bm) * ceil_div(N, t.bn) >= 2 * int64_t(cus)) return t;
  return kTiles[kNumTiles - 1];
}

template <typename T, int BM, int BN, int XK, int WK, bool Y16>
void launch_one(const PackedArgs& a, hipStream_t s) {
  const int tiles_n = int(ceil_div(a.N, BN));
  const int tiles = int(ceil_div(a.M, BM)) * tiles_n;
  hipLaunchKernelGGL((linear16_packed_kernel<T, BM, BN, XK, WK, Y16>), dim3(tiles),
                     dim3(kThreads), 0, s, a, tiles_n, tiles);
}

template <typename T, int BM, int BN, int XK, int WK>
void launch_y(bool y16, const PackedArgs& a, hipStream_t s) {
  if (y16)
    launch_one<T, BM, BN, XK, WK, true>(a, s);
  else
    launch_one<T, BM, BN, XK, WK, false>(a, s);
}

// wk == kPacked: dlrm_linear16_forward_packed's kernels.  Else dlrm_linear16_forward_fmt's: W
// fp32 (wk says how it loads; an fp32 X loads the same way), and an fp32 X only beside a
// 16-bit Y - fp32 X to fp32 Y is dlrm_linear16_forward's kernel and is not built here.
template <typename T, int BM, int BN>
void launch(int xk, int wk, bool y16, const PackedArgs& a, hipStream_t s) {
  if (wk == kPacked) {
    if (xk == kX16)
      launch_y<T, BM, BN, kX16, kPacked>(y16, a, s);
    else if (xk == kXF32Vec)
      launch_y<T, BM, BN, kXF32Vec, kPacked>(y16, a, s);
    else
      launch_y<T, BM, BN, kXF32Elem, kPacked>(y16, a, s);
  } else if (xk == kX16) {
    if (wk == kXF32Vec)
      launch_y<T, BM, BN, kX16, kXF32Vec>(y16, a, s);
    else
      launch_y<T, BM, BN, kX16, kXF32Elem>(y16, a, s);
  } else if (wk == kXF32Vec) {
    launch_one<T, BM, BN, kXF32Vec, kXF32Vec, true>(a, s);
  } else {
    launch_one<T, BM, BN, kXF32Elem, kXF32Elem, true>(a, s);
  }
}

template <typename T>
bool dispatch(Tile t, int xk, int wk, bool y16, const PackedArgs& a, hipStream_t s) {
#define DLRM_L16P_CASE(BM, BN)             \
  if (t.bm == BM && t.bn == BN) {          \
    launch<T, BM, BN>(xk, wk, y16, a, s);  \
    return true;                           \
  }
  DLRM_L16P_CASE(128, 128)
  DLRM_L16P_CASE(128, 64)
  DLRM_L16P_CASE(64, 64)
  DLRM_L16P_CASE(32, 64)
#undef DLRM_L16P_CASE
  return false;
}

}  // namespace
}  // namespace dlrm

extern "C" int dlrm_linear16_pack(int32_t type, int64_t N, int64_t K, const float* W,
                                  int64_t ldw, void* Wp, int64_t ldwp, dlrm_stream_t stream) {
  using namespace dlrm;
  DLRM_ARG(type == DLRM_MLP16_BF16 || type == DLRM_MLP16_F16,
           "dlrm_linear16_pack: unknown type %d", (int)type);
  DLRM_ARG(N >= 0 && K >= 0, "dlrm_linear16_pack: negative size");
  DLRM_ARG(N == 0 || (Wp && (K == 0 || W)), "dlrm_linear16_pack: null pointer");
  DLRM_REQUIRE(ldw >= K, DLRM_ERR_SHAPE, "dlrm_linear16_pack: ldw %lld < K %lld",
               (long long)ldw, (long long)K);
  DLRM_REQUIRE(ldwp % 64 == 0 && ldwp >= K && (N == 0 || ldwp >= 64) && aligned16(Wp),
               DLRM_ERR_SHAPE,
               "dlrm_linear16_pack: ldwp %lld must be a multiple of 64, at least K %lld, and Wp "
               "16-byte aligned",
               (long long)ldwp, (long long)K);
  if (N == 0) return DLRM_OK;
  const int64_t ldc = ldwp / 8, total = N * ldc;
  const int grid = int(ceil_div(total, 256) < 2048 ? ceil_div(total, 256) : 2048);
  const int vec4 = aligned16(W) && ldw % 4 == 0;
  if (type == DLRM_MLP16_BF16)
    hipLaunchKernelGGL(pack16_kernel<__bf16>, dim3(grid), dim3(256), 0, as_stream(stream), N, K,
                       W, ldw, static_cast<bf16x8*>(Wp), ldc, vec4);
  else
    hipLaunchKernelGGL(pack16_kernel<_Float16>, dim3(grid), dim3(256), 0, as_stream(stream), N,
                       K, W, ldw, static_cast<f16x8*>(Wp), ldc, vec4);
  DLRM_LAUNCH_CHECK("dlrm_linear16_pack");
  return DLRM_OK;
}

extern "C" int dlrm_linear16_forward_packed(int32_t type, int64_t M, int64_t N, int64_t K,
                                            const void* X, int32_t x_kind, int64_t ldx,
                                            const void* Wp, int64_t ldwp, const float* bias,
                                            int64_t bias_stride, int32_t relu, void* Y,
                                            int32_t y_kind, int64_t ldy, dlrm_stream_t stream) {
  using namespace dlrm;
  const char* fn = "dlrm_linear16_forward_packed";
  DLRM_ARG(type == DLRM_MLP16_BF16 || type == DLRM_MLP16_F16, "%s: unknown type %d", fn,
           (int)type);
  DLRM_ARG(x_kind == DLRM_L16_FP32 || x_kind == DLRM_L16_HALF, "%s: unknown x_kind %d", fn,
           (int)x_kind);
  DLRM_ARG(y_kind == DLRM_L16_FP32 || y_kind == DLRM_L16_HALF, "%s: unknown y_kind %d", fn,
           (int)y_kind);
  DLRM_ARG(M >= 0 && N >= 0 && K >= 0, "%s: negative size", fn);
  if (M == 0 || N == 0) return DLRM_OK;
  DLRM_ARG(Y && Wp && (K == 0 || X), "%s: null pointer", fn);
  DLRM_REQUIRE(ldx >= K && ldy >= N, DLRM_ERR_SHAPE, "%s: ldx %lld < K %lld or ldy %lld < N %lld",
               fn, (long long)ldx, (long long)K, (long long)ldy, (long long)N);
  DLRM_REQUIRE(ldwp % 64 == 0 && ldwp >= K && ldwp >= 64 && aligned16(Wp), DLRM_ERR_SHAPE,
               "%s: ldwp %lld must be a multiple of 64, at least K %lld, and Wp 16-byte aligned",
               fn, (long long)ldwp, (long long)K);
  if (x_kind == DLRM_L16_HALF) {
    DLRM_REQUIRE(K % 8 == 0 && ldx % 8 == 0 && aligned16(X), DLRM_ERR_SHAPE,
                 "%s: a 16-bit X needs K %lld and ldx %lld multiples of 8 and X 16-byte aligned",
                 fn, (long long)K, (long long)ldx);
  }
  if (y_kind == DLRM_L16_HALF) {
    DLRM_REQUIRE(ldy % 8 == 0 && aligned16(Y), DLRM_ERR_SHAPE,
                 "%s: a 16-bit Y needs ldy %lld a multiple of 8 and Y 16-byte aligned", fn,
                 (long long)ldy);
  }
  const int64_t forced = tuning(DLRM_TUNE_LINEAR16_TILE);
  Tile t{int(forced / 1000), int(forced % 1000)};
  if (forced != 0) {
    DLRM_ARG(known_tile(t), "%s: DLRM_TUNE_LINEAR16_TILE %lld is not a tile", fn,
             (long long)forced);
  }
  DLRM_REQUIRE(ceil_div(M, 32) * ceil_div(N, 64) <= INT32_MAX, DLRM_ERR_UNSUPPORTED,
               "%s: more than 2^31 - 1 tiles", fn);
  if (forced == 0) t = plan_tile(M, N, device_cus());
  // an fp32 X takes 16-byte loads where every row starts on a 16-byte boundary; elements at
  // k >= K are not read on any path
  const int xk = x_kind == DLRM_L16_HALF ? kX16
                 : (aligned16(X) && ldx % 4 == 0) ? kXF32Vec
                                                  : kXF32Elem;
  const PackedArgs a{M, N, K, X, ldx, Wp, ldwp, bias, bias_stride, relu, Y, ldy};
  const bool y16 = y_kind == DLRM_L16_HALF;
  const bool ok = type == DLRM_MLP16_BF16
                      ? dispatch<__bf16>(t, xk, kPacked, y16, a, as_stream(stream))
                      : dispatch<_Float16>(t, xk, kPacked, y16, a, as_stream(stream));
  DLRM_REQUIRE(ok, DLRM_ERR_UNSUPPORTED, "%s: no kernel for the tile", fn);
  DLRM_LAUNCH_CHECK(fn);
  return DLRM_OK;
}

extern "C" int dlrm_linear16_forward_fmt(int32_t type, int64_t M, int64_t N, int64_t K,
                                         const void* X, int32_t x_kind, int64_t ldx,
                                         const float* W, int64_t ldw, const float* bias,
                                         int64_t bias_stride, int32_t relu, void* Y,
                                         int32_t y_kind, int64_t ldy, dlrm_stream_t stream) {
  using namespace dlrm;
  const char* fn = "dlrm_linear16_forward_fmt";
  DLRM_ARG(type == DLRM_MLP16_BF16 || type == DLRM_MLP16_F16, "%s: unknown type %d", fn,
           (int)type);
  DLRM_ARG(x_kind == DLRM_L16_FP32 || x_kind == DLRM_L16_HALF, "%s: unknown x_kind %d", fn,
           (int)x_kind);
  DLRM_ARG(y_kind == DLRM_L16_FP32 || y_kind == DLRM_L16_HALF, "%s: unknown y_kind %d", fn,
           (int)y_kind);
  DLRM_ARG(M >= 0 && N >= 0 && K >= 0, "%s: negative size", fn);
  DLRM_REQUIRE(x_kind == DLRM_L16_HALF || y_kind == DLRM_L16_HALF, DLRM_ERR_UNSUPPORTED,
               "%s: fp32 X to fp32 Y is dlrm_linear16_forward", fn);
  if (M == 0 || N == 0) return DLRM_OK;
  DLRM_ARG(Y && (K == 0 || (X && W)), "%s: null pointer", fn);
  DLRM_REQUIRE(ldx >= K && ldw >= K && ldy >= N, DLRM_ERR_SHAPE,
               "%s: ldx %lld / ldw %lld < K %lld or ldy %lld < N %lld", fn, (long long)ldx,
               (long long)ldw, (long long)K, (long long)ldy, (long long)N);
  if (x_kind == DLRM_L16_HALF) {
    DLRM_REQUIRE(K % 8 == 0 && ldx % 8 == 0 && aligned16(X), DLRM_ERR_SHAPE,
                 "%s: a 16-bit X needs K %lld and ldx %lld multiples of 8 and X 16-byte aligned",
                 fn, (long long)K, (long long)ldx);
  }
  if (y_kind == DLRM_L16_HALF) {
    DLRM_REQUIRE(N % 8 == 0 && ldy % 8 == 0 && aligned16(Y), DLRM_ERR_SHAPE,
                 "%s: a 16-bit Y needs N %lld and ldy %lld multiples of 8 and Y 16-byte aligned",
                 fn, (long long)N, (long long)ldy);
  }
  const int64_t forced = tuning(DLRM_TUNE_LINEAR16_TILE);
  Tile t{int(forced / 1000), int(forced % 1000)};
  if (forced != 0) {
    DLRM_ARG(known_tile(t), "%s: DLRM_TUNE_LINEAR16_TILE %lld is not a tile", fn,
             (long long)forced);
  }
  DLRM_REQUIRE(ceil_div(M, 32) * ceil_div(N, 64) <= INT32_MAX, DLRM_ERR_UNSUPPORTED,
               "%s: more than 2^31 - 1 tiles", fn);
  if (forced == 0) t = plan_tile(M, N, device_cus());
  // the fp32 operands (W, and X where it is fp32) take 16-byte loads where each of them starts
  // every row on a 16-byte boundary; elements at k >= K are not read on any path
  const bool vec = aligned16(W) && ldw % 4 == 0 &&
                   (x_kind == DLRM_L16_HALF || (aligned16(X) && ldx % 4 == 0));
  const int wk = vec ? kXF32Vec : kXF32Elem;
  const int xk = x_kind == DLRM_L16_HALF ? kX16 : wk;
  const PackedArgs a{M, N, K, X, ldx, W, ldw, bias, bias_stride, relu, Y, ldy};
  const bool y16 = y_kind == DLRM_L16_HALF;
  const bool ok = type == DLRM_MLP16_BF16
                      ? dispatch<__bf16>(t, xk, wk, y16, a, as_stream(stream))
                      : dispatch<_Float16>(t, xk, wk, y16, a, as_stream(stream));
  DLRM_REQUIRE(ok, DLRM_ERR_UNSUPPORTED, "%s: no kernel for the tile", fn);
  DLRM_LAUNCH_CHECK(fn);
  return DLRM_OK;
}
