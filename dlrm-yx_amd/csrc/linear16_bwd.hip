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
#include "linear16_bwd_tile.hpp"

namespace dlrm {
namespace {

using namespace l16;

// the per-tile body (staging, LDS image, MFMA loop, epilogue) is linear16_bwd_tile.hpp's
template <typename T, int BM, int BN, bool TRANS_A, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void linear16_bwd_kernel(const BwdArgs p) {
  using vec = typename Op16<T>::vec;
  __shared__ vec lds[2 * (BM + BN) * 8];
  const float lr = dlrm_resolve_lr(p.lr_dev, p.lr);
  f32x4 acc[BM / 32][BN / 32];
  int64_t i0, j0;
  bwd_tile_acc<T, BM, BN, TRANS_A, ALIGNED>(p, lds, blockIdx.x, blockIdx.y, acc, i0, j0);
  float* out = p.Out;
  int64_t ldo = p.ldo;
  if (p.epi == kEpiPartial) {
    out += int64_t(blockIdx.y) * p.I * p.J;
    ldo = p.J;
  }
  bwd_tile_store<BM, BN>(p, p.epi, lr, acc, i0, j0, out, ldo);
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
