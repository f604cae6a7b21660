// Forward-only Linear with 16-bit MFMA operands (dlrm_linear16_forward, ABI v12):
//   Y[m][n] = act( sum_{k<K} r16(X[m][k]) * r16(W[n][k]) + bias[n*bias_stride] )
// X [M][K] and W [N][K] stay fp32 in memory (both K-contiguous, so nothing is transposed);
// r16 is the round-to-nearest-even conversion to bf16 or IEEE fp16 (a plain cast:
// v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32), done while a tile is staged to LDS.  The products
// accumulate in fp32 on v_mfma_f32_16x16x32_{bf16,f16}; bias and ReLU are fp32.
//
// One workgroup (4 waves, 2 x 2) per BM x BN tile of Y, K in steps of 64:
//   global (fp32, registers) -> convert -> LDS (16-bit, two buffers, one barrier per step)
//   -> one 16-byte LDS read per lane and fragment -> MFMA.
// LDS rows are 128 B (64 elements = 8 chunks of 16 B); chunk c of row r sits at chunk
// c ^ ((r >> 1) & 7), which makes the 16-lane groups of ds_read_b128 conflict-free.
// Neither load path ever reads an element with k >= K or a row >= M / >= N: tail elements
// are selected to zero (never multiplied), rows past the end are clamped to the last row
// and their results are not written.  No split-K, no atomics, no workspace.
#include "linear16_stage.hpp"

namespace dlrm {
namespace {

using namespace l16;

template <typename T, int BM, int BN, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void linear16_kernel(
    int64_t M, int64_t N, int64_t K, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ W, int64_t ldw, const float* __restrict__ bias,
    int64_t bias_stride, int relu, float* __restrict__ Y, int64_t ldy, int tiles_n,
    int tiles) {
  using vec = typename Op16<T>::vec;
  constexpr int WTM = BM / 2, WTN = BN / 2;  // a wave's part of the tile
  constexpr int FM = WTM / 16, FN = WTN / 16;
  static_assert(BM % 32 == 0 && BN % 32 == 0, "tile");
  __shared__ vec lds[2][(BM + BN) * 8];

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

  Stage<BM> sa;
  Stage<BN> sb;
  const int64_t nk = (K + kBK - 1) / kBK;
  auto fetch = [&](int64_t kt) {
    const int64_t k0 = kt * kBK;
    if (k0 + kBK <= K) {
      sa.template load<ALIGNED, true>(X, ldx, m0, M, k0, K, tid);
      sb.template load<ALIGNED, true>(W, ldw, n0, N, k0, K, tid);
    } else {
      sa.template load<ALIGNED, false>(X, ldx, m0, M, k0, K, tid);
      sb.template load<ALIGNED, false>(W, ldw, n0, N, k0, K, tid);
    }
  };
  auto commit = [&](int buf) {
    sa.template store<T>(lds[buf], tid);
    sb.template store<T>(lds[buf] + BM * 8, tid);
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
    if (kt + 1 < nk) commit(buf ^ 1);
    __syncthreads();
  }

  // C/D map of 16x16: col = lane & 15, row = (lane >> 4) * 4 + reg
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
        float y = acc[i][j][r] + bv;
        if (relu) y = (y != y) ? y : fmaxf(y, 0.0f);  // NaN propagates
        Y[m * ldy + n] = y;
      }
    }
  }
}

// The largest tile that still gives every CU two workgroups (a workgroup waits on its global
// loads once per k-step; a second one on the CU fills that time), else the smallest.  At
// M = 2048: N = 1024 -> 64x64 (512 workgroups), N = 512 -> 32x64 (512), N <= 256 -> 32x64.
Tile plan_tile(int64_t M, int64_t N, int cus) {
  for (const Tile& t : kTiles)
    if (ceil_div(M, t.bm) * ceil_div(N, t.bn) >= 2 * int64_t(cus)) return t;
  return kTiles[kNumTiles - 1];
}

template <typename T, int BM, int BN>
void launch(bool aligned, int64_t M, int64_t N, int64_t K, const float* X, int64_t ldx,
            const float* W, int64_t ldw, const float* bias, int64_t bias_stride, int relu,
            float* Y, int64_t ldy, hipStream_t s) {
  const int tiles_n = int(ceil_div(N, BN));
  const int tiles = int(ceil_div(M, BM)) * tiles_n;
  if (aligned)
    hipLaunchKernelGGL((linear16_kernel<T, BM, BN, true>), dim3(tiles), dim3(kThreads), 0, s, M,
                       N, K, X, ldx, W, ldw, bias, bias_stride, relu, Y, ldy, tiles_n, tiles);
  else
    hipLaunchKernelGGL((linear16_kernel<T, BM, BN, false>), dim3(tiles), dim3(kThreads), 0, s, M,
                       N, K, X, ldx, W, ldw, bias, bias_stride, relu, Y, ldy, tiles_n, tiles);
}

template <typename T>
bool dispatch(Tile t, bool aligned, int64_t M, int64_t N, int64_t K, const float* X,
              int64_t ldx, const float* W, int64_t ldw, const float* bias, int64_t bias_stride,
              int relu, float* Y, int64_t ldy, hipStream_t s) {
#define DLRM_L16_CASE(BM, BN)                                                              \
  if (t.bm == BM && t.bn == BN) {                                                          \
    launch<T, BM, BN>(aligned, M, N, K, X, ldx, W, ldw, bias, bias_stride, relu, Y, ldy, s); \
    return true;                                                                           \
  }
  DLRM_L16_CASE(128, 128)
  DLRM_L16_CASE(128, 64)
  DLRM_L16_CASE(64, 64)
  DLRM_L16_CASE(32, 64)
#undef DLRM_L16_CASE
  return false;
}

}  // namespace
}  // namespace dlrm

extern "C" int dlrm_linear16_forward(int32_t type, int64_t M, int64_t N, int64_t K,
                                     const float* X, int64_t ldx, const float* W, int64_t ldw,
                                     const float* bias, int64_t bias_stride, int32_t relu,
                                     float* Y, int64_t ldy, dlrm_stream_t stream) {
  using namespace dlrm;
  DLRM_ARG(type == DLRM_MLP16_BF16 || type == DLRM_MLP16_F16,
           "dlrm_linear16_forward: unknown type %d", (int)type);
  DLRM_ARG(M >= 0 && N >= 0 && K >= 0, "dlrm_linear16_forward: negative size");
  if (M == 0 || N == 0) return DLRM_OK;
  DLRM_ARG(Y && (K == 0 || (X && W)), "dlrm_linear16_forward: null pointer");
  DLRM_REQUIRE(ldx >= K && ldw >= K && ldy >= N, DLRM_ERR_SHAPE,
               "dlrm_linear16_forward: ldx %lld / ldw %lld < K %lld or ldy %lld < N %lld",
               (long long)ldx, (long long)ldw, (long long)K, (long long)ldy, (long long)N);
  const int64_t forced = tuning(DLRM_TUNE_LINEAR16_TILE);
  Tile t{int(forced / 1000), int(forced % 1000)};
  if (forced != 0) {
    DLRM_ARG(known_tile(t), "dlrm_linear16_forward: DLRM_TUNE_LINEAR16_TILE %lld is not a tile",
             (long long)forced);
  }
  DLRM_REQUIRE(ceil_div(M, 32) * ceil_div(N, 64) <= INT32_MAX, DLRM_ERR_UNSUPPORTED,
               "dlrm_linear16_forward: more than 2^31 - 1 tiles");
  if (forced == 0) t = plan_tile(M, N, device_cus());
  // 16-byte loads where every row starts on a 16-byte boundary; elements at k >= K are
  // not read on either path, so the rows need not be readable past K
  const bool aligned = (reinterpret_cast<uintptr_t>(X) % 16 == 0) &&
                       (reinterpret_cast<uintptr_t>(W) % 16 == 0) && ldx % 4 == 0 && ldw % 4 == 0;
  const bool ok = type == DLRM_MLP16_BF16
                      ? dispatch<__bf16>(t, aligned, M, N, K, X, ldx, W, ldw, bias, bias_stride,
                                         relu, Y, ldy, as_stream(stream))
                      : dispatch<_Float16>(t, aligned, M, N, K, X, ldx, W, ldw, bias,
                                           bias_stride, relu, Y, ldy, as_stream(stream));
  DLRM_REQUIRE(ok, DLRM_ERR_UNSUPPORTED, "dlrm_linear16_forward: no kernel for the tile");
  DLRM_LAUNCH_CHECK("dlrm_linear16_forward");
  return DLRM_OK;
}
