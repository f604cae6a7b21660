// Backward of a Linear with 16-bit MFMA operands (dlrm_linear16_dgrad / dlrm_linear16_wgrad,
// ABI v13):
//   dgrad  dX[m][k] = (mask == NULL || mask[m][k] > 0) ? sum_n r16(dY[m][n]) r16(W[n][k]) : 0
//   wgrad  acc[n][k] = sum_m r16(dY[m][n]) r16(X[m][k]);  C = acc  or  C = C - fl(lr acc)
// Every matrix is fp32 in memory; r16 (RNE to bf16 / fp16) happens while a tile is staged to
// LDS, the products accumulate in fp32 on v_mfma_f32_16x16x32_{bf16,f16}.
//
// Both are one kernel, Out[i][j] = sum_r A(i, r) B(j, r), over the forward's structure (one
// workgroup of 2 x 2 waves per BM x BN tile, reduction in steps of 64, two LDS buffers, one
// barrier per step, the same swizzled [row][64 x 16-bit] LDS image and ds_read_b128 fragment
// reads).  What is new is the staging of an operand whose REDUCTION index is the row index in
// memory (W in dgrad, dY and X in wgrad): StageT loads it coalesced along the contiguous
// (output) dimension - a thread takes RG consecutive reduction rows of 4 consecutive
// columns, 16-byte loads - converts, and writes each of its 4 columns' RG reduction elements
// as one packed LDS store into that column's row of the image.  The transpose is done in
// registers; the MFMA side is unchanged.
//
// Neither path reads an element outside the extents: reduction rows >= R and columns past
// the extent are selected to zero without a load (never multiplied); results of rows /
// columns past the output's extent are not written.
//
// wgrad's reduction depth is the batch while its output can be small, so the planner may
// split the reduction over `splits` workgroups per tile.  The partial tiles then go to the
// workspace ([split][N][K] fp32) and a second launch sums them in split order and applies
// STORE / SGD: no atomics, the same bits on every call.
#include <type_traits>

#include "linear16_stage.hpp"

namespace dlrm {
namespace {

using namespace l16;

constexpr int kMaxSplits = 32;

// One thread's share of a [64 reduction rows][OUT columns] fp32 tile whose rows are
// contiguous along the columns: RG reduction rows x 4 columns.
template <int OUT>
struct StageT {
  static constexpr int kCG = OUT / 4;                  // groups of 4 columns
  static constexpr int kRG = kBK / (kThreads / kCG);   // reduction rows per thread
  static_assert(OUT == 32 || OUT == 64 || OUT == 128, "tile");
  float v[kRG][4];

  template <bool ALIGNED>
  __device__ __forceinline__ void load(const float* __restrict__ P, int64_t ld, int64_t r0,
                                       int64_t R, int64_t c0, int64_t C, int tid) {
    const int64_t c = c0 + (tid % kCG) * 4;
    const int64_t rb = r0 + (tid / kCG) * kRG;
#pragma unroll
    for (int i = 0; i < kRG; ++i) {
      const int64_t r = rb + i;
      if (r < R && c + 4 <= C) {
        const float* p = P + r * ld + c;
        if (ALIGNED) {
          const float4 a = *reinterpret_cast<const float4*>(p);
          v[i][0] = a.x, v[i][1] = a.y, v[i][2] = a.z, v[i][3] = a.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[i][j] = p[j];
        }
      } else if (r < R) {
        const float* p = P + r * ld + c;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = (c + j < C) ? p[j] : 0.0f;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = 0.0f;  // a reduction tail: zero, nothing read
      }
    }
  }

  template <typename T>
  __device__ __forceinline__ void store(typename Op16<T>::vec* lds, int tid) const {
    typedef T packed __attribute__((ext_vector_type(kRG)));
    T* base = reinterpret_cast<T*>(lds);
    const int e = (tid / kCG) * kRG;  // first reduction element of this thread
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      packed h;
#pragma unroll
      for (int i = 0; i < kRG; ++i) h[i] = static_cast<T>(v[i][j]);  // RNE
      const int row = (tid % kCG) * 4 + j;
      *reinterpret_cast<packed*>(base + lds_chunk(row, e >> 3) * 8 + (e & 7)) = h;
    }
  }
};

enum Epi { kEpiDgrad = 0, kEpiStore = 1, kEpiSgd = 2, kEpiPartial = 3 };

struct BwdArgs {
  int64_t I, J, R;           // Out [I][J], reduction depth R
  const float* A;            // TRANS_A ? [R][I] : [I][R]
  int64_t lda;
  const float* B;            // [R][J]
  int64_t ldb;
  const float* mask;         // kEpiDgrad: [I][J] or NULL
  int64_t ldmask;
  float* Out;                // kEpiPartial: the workspace, [split][I][J]
  int64_t ldo;
  int epi;
  float lr;
  const float* lr_dev;       // ABI v14: NULL, or the device fp32 that replaces lr (kEpiSgd)
  int tiles_j, tiles;
  int64_t steps_per_split;   // reduction steps of 64 per blockIdx.y
};

template <typename T, int BM, int BN, bool TRANS_A, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void linear16_bwd_kernel(const BwdArgs p) {
  using vec = typename Op16<T>::vec;
  constexpr int WTM = BM / 2, WTN = BN / 2;  // a wave's part of the tile
  constexpr int FM = WTM / 16, FN = WTN / 16;
  static_assert(BM % 32 == 0 && BN % 32 == 0, "tile");
  __shared__ vec lds[2][(BM + BN) * 8];
  const float lr = dlrm_resolve_lr(p.lr_dev, p.lr);

  // consecutive tiles (j fastest: they share A) go to one XCD; bijective for any count
  const int orig = blockIdx.x;
  const int q = p.tiles / 8, rem = p.tiles % 8, xcd = orig % 8;
  const int tile = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + orig / 8;
  const int64_t i0 = int64_t(tile / p.tiles_j) * BM;
  const int64_t j0 = int64_t(tile % p.tiles_j) * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * WTM, wn = (wave & 1) * WTN;
  const int fr = lane & 15, fc = lane >> 4;

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  typename std::conditional<TRANS_A, StageT<BM>, Stage<BM>>::type sa;
  StageT<BN> sb;
  const int64_t nk_all = (p.R + kBK - 1) / kBK;
  const int64_t kt0 = int64_t(blockIdx.y) * p.steps_per_split;
  const int64_t kt1 = kt0 + p.steps_per_split < nk_all ? kt0 + p.steps_per_split : nk_all;
  auto fetch = [&](int64_t kt) {
    const int64_t r0 = kt * kBK;
    if constexpr (TRANS_A) {
      sa.template load<ALIGNED>(p.A, p.lda, r0, p.R, i0, p.I, tid);
    } else {
      if (r0 + kBK <= p.R)
        sa.template load<ALIGNED, true>(p.A, p.lda, i0, p.I, r0, p.R, tid);
      else
        sa.template load<ALIGNED, false>(p.A, p.lda, i0, p.I, r0, p.R, tid);
    }
    sb.template load<ALIGNED>(p.B, p.ldb, r0, p.R, j0, p.J, tid);
  };
  auto commit = [&](int buf) {
    sa.template store<T>(lds[buf], tid);
    sb.template store<T>(lds[buf] + BM * 8, tid);
  };

  if (kt0 < kt1) {
    fetch(kt0);
    commit(0);
  }
  __syncthreads();
  for (int64_t kt = kt0; kt < kt1; ++kt) {
    const int buf = int((kt - kt0) & 1);
    if (kt + 1 < kt1) fetch(kt + 1);
    const vec* A = lds[buf];
    const vec* B = lds[buf] + BM * 8;
#pragma unroll
    for (int ks = 0; ks < kBK / 32; ++ks) {
      vec a[FM], b[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) a[i] = A[lds_chunk(wm + i * 16 + fr, ks * 4 + fc)];
#pragma unroll
      for (int j = 0; j < FN; ++j) b[j] = B[lds_chunk(wn + j * 16 + fr, ks * 4 + fc)];
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = Op16<T>::mfma(a[i], b[j], acc[i][j]);
    }
    // the other buffer was last read in step kt - 1, which every wave left at its barrier
    if (kt + 1 < kt1) commit(buf ^ 1);
    __syncthreads();
  }

  // C/D map of 16x16: col = lane & 15, row = (lane >> 4) * 4 + reg
  float* out = p.Out;
  int64_t ldo = p.ldo;
  if (p.epi == kEpiPartial) {
    out += int64_t(blockIdx.y) * p.I * p.J;
    ldo = p.J;
  }
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int64_t cj = j0 + wn + j * 16 + fr;
    if (cj >= p.J) continue;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t ci = i0 + wm + i * 16 + fc * 4 + r;
        if (ci >= p.I) continue;
        float v = acc[i][j][r];
        float* o = out + ci * ldo + cj;
        if (p.epi == kEpiDgrad) {
          if (p.mask) v = p.mask[ci * p.ldmask + cj] > 0.f ? v : 0.f;  // selects, NaN -> 0
        } else if (p.epi == kEpiSgd) {
          // ONE rounding, unlike DLRM_EPI_SGD: the __fsub_rn(*o, __fmul_rn(lr, v)) that stood
          // here always compiled to this fma (common.hpp, dlrm_scale), and the bf16 step
          // traces pin its bits.  Two roundings are dlrm_sgd_step(*o, dlrm_scale(lr, v)).
          v = fmaf(-lr, v, *o);
        }
        *o = v;
      }
    }
  }
}

// C[n][k] (op)= sum over the splits, in split order
__global__ __launch_bounds__(kThreads) void wgrad16_reduce_kernel(
    int64_t N, int64_t K, const float* __restrict__ partial, int splits, int sgd, float lr_host,
    float* __restrict__ C, int64_t ldc, const float* __restrict__ lr_dev) {
  const float lr = dlrm_resolve_lr(lr_dev, lr_host);
  const int64_t idx = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= N * K) return;
  float acc = partial[idx];
  for (int s = 1; s < splits; ++s) acc += partial[int64_t(s) * N * K + idx];
  float* o = C + (idx / K) * ldc + idx % K;
  *o = sgd ? fmaf(-lr, acc, *o) : acc;  // one rounding, as the unsplit epilogue above
}

template <typename T, int BM, int BN, bool TRANS_A>
void launch(bool aligned, const BwdArgs& a, int splits, hipStream_t s) {
  const dim3 grid(a.tiles, splits);
  if (aligned)
    hipLaunchKernelGGL((linear16_bwd_kernel<T, BM, BN, TRANS_A, true>), grid, dim3(kThreads), 0,
                       s, a);
  else
    hipLaunchKernelGGL((linear16_bwd_kernel<T, BM, BN, TRANS_A, false>), grid, dim3(kThreads),
                       0, s, a);
}

template <typename T, bool TRANS_A>
bool dispatch(Tile t, bool aligned, const BwdArgs& a, int splits, hipStream_t s) {
#define DLRM_L16B_CASE(BM, BN)                               \
  if (t.bm == BM && t.bn == BN) {                            \
    launch<T, BM, BN, TRANS_A>(aligned, a, splits, s);       \
    return true;                                             \
  }
  DLRM_L16B_CASE(128, 128)
  DLRM_L16B_CASE(128, 64)
  DLRM_L16B_CASE(64, 64)
  DLRM_L16B_CASE(32, 64)
#undef DLRM_L16B_CASE
  return false;
}

inline int64_t tiles_of(Tile t, int64_t I, int64_t J) {
  return ceil_div(I, t.bm) * ceil_div(J, t.bn);
}

// dgrad: the forward's rule on the [M][K] output - the largest tile that still gives every CU
// two workgroups, else the smallest.
Tile plan_dgrad(int64_t I, int64_t J, int cus) {
  for (const Tile& t : kTiles)
    if (tiles_of(t, I, J) >= 2 * int64_t(cus)) return t;
  return kTiles[kNumTiles - 1];
}

struct WgradPlan {
  Tile tile;
  int splits;
  int64_t steps;  // reduction steps per split
};

// wgrad: 128 x 128 and no split where that tile alone gives every CU two workgroups.
// Otherwise the tile by the number of 64 x 64 tiles of the [N][K] output (more than cus / 2:
// 128 x 64; at least cus / 8: 64 x 64; else 32 x 64) and the batch split into runs of four
// 64-row steps - more splits while the launch has fewer than cus / 2 workgroups, at most
// kMaxSplits, at least one step each.  Measured at the C3 layers, B = 2048
// (profiles/train16_wgrad_plan_sweep.json): 8 splits win at every layer, 128 x 64 at
// 1024 x 1024 and 512 x 1024, 64 x 64 at 1024 x 479 and 256 x 512, 32 x 64 at 512 x 13
// and 128 x 256.
WgradPlan plan_wgrad(int64_t R, int64_t I, int64_t J, int cus, int64_t forced_tile,
                     int64_t forced_split) {
  const int64_t nk = ceil_div(R, kBK);
  WgradPlan w{{int(forced_tile / 1000), int(forced_tile % 1000)}, 0, 0};
  bool whole = false;
  if (forced_tile == 0) {
    const int64_t t64 = tiles_of(kTiles[2], I, J);
    whole = tiles_of(kTiles[0], I, J) >= 2 * int64_t(cus);
    w.tile = whole ? kTiles[0] : t64 > cus / 2 ? kTiles[1] : t64 >= cus / 8 ? kTiles[2] : kTiles[3];
  }
  const int64_t tiles = tiles_of(w.tile, I, J);
  int64_t s = forced_split;
  if (s == 0 && !whole) {
    const int64_t fill = ceil_div(int64_t(cus) / 2, tiles > 0 ? tiles : 1);
    s = ceil_div(nk, 4) > fill ? ceil_div(nk, 4) : fill;
  }
  s = s < kMaxSplits ? s : kMaxSplits;
  s = s < nk ? s : nk;
  s = s > 1 ? s : 1;
  w.steps = nk > 0 ? ceil_div(nk, s) : 0;
  w.splits = nk > 0 ? int(ceil_div(nk, w.steps)) : 1;  // every split has at least one step
  return w;
}

bool aligned16(const void* a, int64_t lda, const void* b, int64_t ldb) {
  return reinterpret_cast<uintptr_t>(a) % 16 == 0 && reinterpret_cast<uintptr_t>(b) % 16 == 0 &&
         lda % 4 == 0 && ldb % 4 == 0;
}

}  // namespace
}  // namespace dlrm

extern "C" int dlrm_linear16_dgrad(int32_t type, int64_t M, int64_t N, int64_t K,
                                   const float* dY, int64_t lddy, const float* W, int64_t ldw,
                                   const float* mask, int64_t ldmask, float* dX, int64_t lddx,
                                   dlrm_stream_t stream) {
  using namespace dlrm;
  DLRM_ARG(type == DLRM_MLP16_BF16 || type == DLRM_MLP16_F16,
           "dlrm_linear16_dgrad: unknown type %d", (int)type);
  DLRM_ARG(M >= 0 && N >= 0 && K >= 0, "dlrm_linear16_dgrad: negative size");
  if (M == 0 || K == 0) return DLRM_OK;
  DLRM_ARG(dX && (N == 0 || (dY && W)), "dlrm_linear16_dgrad: null pointer");
  DLRM_REQUIRE(lddy >= N && ldw >= K && lddx >= K && (!mask || ldmask >= K), DLRM_ERR_SHAPE,
               "dlrm_linear16_dgrad: lddy %lld < N %lld or ldw %lld / lddx %lld / ldmask %lld "
               "< K %lld",
               (long long)lddy, (long long)N, (long long)ldw, (long long)lddx,
               (long long)ldmask, (long long)K);
  const int64_t forced = tuning(DLRM_TUNE_LINEAR16_DGRAD_TILE);
  Tile t{int(forced / 1000), int(forced % 1000)};
  DLRM_ARG(forced == 0 || known_tile(t),
           "dlrm_linear16_dgrad: DLRM_TUNE_LINEAR16_DGRAD_TILE %lld is not a tile",
           (long long)forced);
  DLRM_REQUIRE(ceil_div(M, 32) * ceil_div(K, 64) <= INT32_MAX, DLRM_ERR_UNSUPPORTED,
               "dlrm_linear16_dgrad: more than 2^31 - 1 tiles");
  if (forced == 0) t = plan_dgrad(M, K, device_cus());
  BwdArgs a{};
  a.I = M, a.J = K, a.R = N;
  a.A = dY, a.lda = lddy, a.B = W, a.ldb = ldw;
  a.mask = mask, a.ldmask = ldmask, a.Out = dX, a.ldo = lddx;
  a.epi = kEpiDgrad, a.lr = 0.f;
  a.tiles_j = int(ceil_div(K, t.bn));
  a.tiles = int(ceil_div(M, t.bm)) * a.tiles_j;
  a.steps_per_split = ceil_div(N, kBK);
  const bool aligned = aligned16(dY, lddy, W, ldw);
  const bool ok = type == DLRM_MLP16_BF16
                      ? dispatch<__bf16, false>(t, aligned, a, 1, as_stream(stream))
                      : dispatch<_Float16, false>(t, aligned, a, 1, as_stream(stream));
  DLRM_REQUIRE(ok, DLRM_ERR_UNSUPPORTED, "dlrm_linear16_dgrad: no kernel for the tile");
  DLRM_LAUNCH_CHECK("dlrm_linear16_dgrad");
  return DLRM_OK;
}

namespace dlrm {
namespace {
// the plan of a wgrad call under the calling thread's tuning; false: a forced value is bad
bool wgrad_plan_checked(int64_t M, int64_t N, int64_t K, WgradPlan* w) {
  const int64_t ft = tuning(DLRM_TUNE_LINEAR16_WGRAD_TILE);
  const int64_t fs = tuning(DLRM_TUNE_LINEAR16_WGRAD_SPLIT);
  if (ft != 0 && !known_tile(Tile{int(ft / 1000), int(ft % 1000)})) return false;
  *w = plan_wgrad(M, N, K, device_cus(), ft, fs);
  return true;
}
}  // namespace
}  // namespace dlrm

extern "C" size_t dlrm_linear16_wgrad_workspace_size(int32_t type, int64_t M, int64_t N,
                                                     int64_t K) {
  using namespace dlrm;
  (void)type;
  WgradPlan w;
  if (M <= 0 || N <= 0 || K <= 0 || !wgrad_plan_checked(M, N, K, &w) || w.splits <= 1) return 0;
  return size_t(w.splits) * size_t(N) * size_t(K) * sizeof(float);
}

namespace {
int linear16_wgrad(int32_t type, int64_t M, int64_t N, int64_t K, const float* dY, int64_t lddy,
                   const float* X, int64_t ldx, int32_t mode, float lr, const float* lr_dev,
                   float* C, int64_t ldc, void* workspace, size_t workspace_bytes,
                   dlrm_stream_t stream) {
  using namespace dlrm;
  DLRM_ARG(type == DLRM_MLP16_BF16 || type == DLRM_MLP16_F16,
           "dlrm_linear16_wgrad: unknown type %d", (int)type);
  DLRM_ARG(mode == DLRM_WGRAD16_STORE || mode == DLRM_WGRAD16_SGD,
           "dlrm_linear16_wgrad: unknown mode %d", (int)mode);
  DLRM_ARG(M >= 0 && N >= 0 && K >= 0, "dlrm_linear16_wgrad: negative size");
  if (N == 0 || K == 0) return DLRM_OK;
  if (M == 0 && mode == DLRM_WGRAD16_SGD) return DLRM_OK;  // C - fl(lr * 0): C stays
  DLRM_ARG(C && (M == 0 || (dY && X)), "dlrm_linear16_wgrad: null pointer");
  DLRM_REQUIRE(lddy >= N && ldx >= K && ldc >= K, DLRM_ERR_SHAPE,
               "dlrm_linear16_wgrad: lddy %lld < N %lld or ldx %lld / ldc %lld < K %lld",
               (long long)lddy, (long long)N, (long long)ldx, (long long)ldc, (long long)K);
  DLRM_REQUIRE(ceil_div(N, 32) * ceil_div(K, 64) <= INT32_MAX &&
                   ceil_div(N * K, kThreads) <= INT32_MAX,
               DLRM_ERR_UNSUPPORTED, "dlrm_linear16_wgrad: more than 2^31 - 1 tiles");
  WgradPlan w;
  DLRM_ARG(wgrad_plan_checked(M, N, K, &w),
           "dlrm_linear16_wgrad: DLRM_TUNE_LINEAR16_WGRAD_TILE %lld is not a tile",
           (long long)tuning(DLRM_TUNE_LINEAR16_WGRAD_TILE));
  const size_t need = w.splits > 1 ? size_t(w.splits) * size_t(N) * size_t(K) * sizeof(float) : 0;
  DLRM_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), DLRM_ERR_WORKSPACE,
               "dlrm_linear16_wgrad: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  BwdArgs a{};
  a.I = N, a.J = K, a.R = M;
  a.A = dY, a.lda = lddy, a.B = X, a.ldb = ldx;
  a.mask = nullptr, a.ldmask = 0;
  const bool split = w.splits > 1;
  a.Out = split ? static_cast<float*>(workspace) : C;
  a.ldo = split ? K : ldc;
  a.epi = split ? kEpiPartial : (mode == DLRM_WGRAD16_SGD ? kEpiSgd : kEpiStore);
  a.lr = lr, a.lr_dev = lr_dev;
  a.tiles_j = int(ceil_div(K, w.tile.bn));
  a.tiles = int(ceil_div(N, w.tile.bm)) * a.tiles_j;
  a.steps_per_split = w.steps;
  const bool aligned = aligned16(dY, lddy, X, ldx);
  hipStream_t s = as_stream(stream);
  const bool ok = type == DLRM_MLP16_BF16
                      ? dispatch<__bf16, true>(w.tile, aligned, a, w.splits, s)
                      : dispatch<_Float16, true>(w.tile, aligned, a, w.splits, s);
  DLRM_REQUIRE(ok, DLRM_ERR_UNSUPPORTED, "dlrm_linear16_wgrad: no kernel for the tile");
  DLRM_LAUNCH_CHECK("dlrm_linear16_wgrad");
  if (split) {
    hipLaunchKernelGGL(wgrad16_reduce_kernel, dim3(unsigned(ceil_div(N * K, kThreads))),
                       dim3(kThreads), 0, s, N, K, static_cast<const float*>(workspace),
                       w.splits, int(mode == DLRM_WGRAD16_SGD), lr, C, ldc, lr_dev);
    DLRM_LAUNCH_CHECK("dlrm_linear16_wgrad (reduce)");
  }
  return DLRM_OK;
}
}  // namespace

extern "C" int dlrm_linear16_wgrad(int32_t type, int64_t M, int64_t N, int64_t K,
                                   const float* dY, int64_t lddy, const float* X, int64_t ldx,
                                   int32_t mode, float lr, float* C, int64_t ldc,
                                   void* workspace, size_t workspace_bytes,
                                   dlrm_stream_t stream) {
  return linear16_wgrad(type, M, N, K, dY, lddy, X, ldx, mode, lr, nullptr, C, ldc, workspace,
                        workspace_bytes, stream);
}

extern "C" int dlrm_linear16_wgrad_dev(int32_t type, int64_t M, int64_t N, int64_t K,
                                       const float* dY, int64_t lddy, const float* X,
                                       int64_t ldx, int32_t mode, const float* lr_dev, float* C,
                                       int64_t ldc, void* workspace, size_t workspace_bytes,
                                       dlrm_stream_t stream) {
  DLRM_ARG(lr_dev && mode == DLRM_WGRAD16_SGD,
           "dlrm_linear16_wgrad_dev: null lr_dev, or a mode other than DLRM_WGRAD16_SGD");
  return linear16_wgrad(type, M, N, K, dY, lddy, X, ldx, mode, 0.f, lr_dev, C, ldc, workspace,
                        workspace_bytes, stream);
}
