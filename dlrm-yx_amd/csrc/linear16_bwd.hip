// Backward of a Linear with 16-bit MFMA operands (dlrm_linear16_dgrad / dlrm_linear16_wgrad,
// ABI v13):
//   dgrad  dX[m][k] = (mask == NULL || mask[m][k] > 0) ? sum_n r16(dY[m][n]) r16(W[n][k]) : 0
//   wgrad  acc[n][k] = sum_m r16(dY[m][n]) r16(X[m][k]);  C = acc  or  C = C - fl(lr acc)
// Every matrix is fp32 in memory; r16 (RNE to bf16 / fp16) happens while a tile is staged to
// LDS, the products accumulate in fp32 on v_mfma_f32_16x16x32_{bf16,f16}.
// dlrm_linear16_dgrad_fmt / _wgrad_fmt (added to ABI v23) are the same kernels with dY, X, the
// mask and dX each fp32 or already 16-bit in memory: a 16-bit operand is staged as 16-byte
// chunks with no conversion (Stage16 / StageT16), a 16-bit dX leaves through LDS
// (bwd_tile_store16); the operand bits, and so the accumulators, are the fp32 call's.
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
// A16 / B16 / O16: that operand is 16-bit (T) in memory (the _fmt entry points below); ALIGNED
// then speaks of the fp32 operands only.
template <typename T, int BM, int BN, bool TRANS_A, bool ALIGNED, bool A16 = false,
          bool B16 = false, bool O16 = false>
__global__ __launch_bounds__(kThreads) void linear16_bwd_kernel(const BwdArgs p) {
  using vec = typename Op16<T>::vec;
  __shared__ vec lds[2 * (BM + BN) * 8];
  const float lr = dlrm_resolve_lr(p.lr_dev, p.lr);
  f32x4 acc[BM / 32][BN / 32];
  int64_t i0, j0;
  bwd_tile_acc<T, BM, BN, TRANS_A, ALIGNED, A16, B16>(p, lds, blockIdx.x, blockIdx.y, acc, i0,
                                                      j0);
  if constexpr (O16) {  // dgrad only
    bwd_tile_store16<T, BM, BN>(p, lds, acc, i0, j0);
    return;
  }
  float* out = static_cast<float*>(p.Out);
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

template <typename T, int BM, int BN, bool TRANS_A, bool A16, bool B16, bool O16>
void launch_fmt(bool aligned, const BwdArgs& a, int splits, hipStream_t s) {
  const dim3 grid(a.tiles, splits);
  if (aligned)
    hipLaunchKernelGGL((linear16_bwd_kernel<T, BM, BN, TRANS_A, true, A16, B16, O16>), grid,
                       dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL((linear16_bwd_kernel<T, BM, BN, TRANS_A, false, A16, B16, O16>), grid,
                       dim3(kThreads), 0, s, a);
}

// The operand formats a launch was built for: all fp32 (dlrm_linear16_dgrad / _wgrad), and
// what the store16 step uses - dgrad (dY, dX) 16/fp32, 16/16, fp32/16 with W fp32; wgrad
// (dY, X) 16/16, 16/fp32, fp32/16 with C fp32.  false: no kernel for this combination.
template <typename T, int BM, int BN, bool TRANS_A>
bool launch(int a16, int b16, int o16, bool aligned, const BwdArgs& a, int splits,
            hipStream_t s) {
  if (!a16 && !b16 && !o16) {
    launch_fmt<T, BM, BN, TRANS_A, false, false, false>(aligned, a, splits, s);
    return true;
  }
  if constexpr (TRANS_A) {
    if (o16) return false;
    if (a16 && b16)
      launch_fmt<T, BM, BN, true, true, true, false>(aligned, a, splits, s);
    else if (a16)
      launch_fmt<T, BM, BN, true, true, false, false>(aligned, a, splits, s);
    else
      launch_fmt<T, BM, BN, true, false, true, false>(aligned, a, splits, s);
  } else {
    if (b16) return false;
    if (a16 && o16)
      launch_fmt<T, BM, BN, false, true, false, true>(aligned, a, splits, s);
    else if (a16)
      launch_fmt<T, BM, BN, false, true, false, false>(aligned, a, splits, s);
    else
      launch_fmt<T, BM, BN, false, false, false, true>(aligned, a, splits, s);
  }
  return true;
}

template <typename T, bool TRANS_A>
bool dispatch(Tile t, int a16, int b16, int o16, bool aligned, const BwdArgs& a, int splits,
              hipStream_t s) {
#define DLRM_L16B_CASE(BM, BN)                                                  \
  if (t.bm == BM && t.bn == BN)                                                 \
    return launch<T, BM, BN, TRANS_A>(a16, b16, o16, aligned, a, splits, s);
  DLRM_L16B_CASE(128, 128)
  DLRM_L16B_CASE(128, 64)
  DLRM_L16B_CASE(64, 64)
  DLRM_L16B_CASE(32, 64)
#undef DLRM_L16B_CASE
  return false;
}


}  // namespace
}  // namespace dlrm

namespace {
using dlrm::l16::aligned16;

// a 16-bit operand moves as 16-byte chunks: its base and its rows must start on one
bool chunked(const void* p, int64_t ld) { return aligned16(p) && ld % 8 == 0; }
// an fp32 operand takes 16-byte loads where every row starts on a 16-byte boundary
bool vec32(const void* p, int64_t ld) { return aligned16(p) && ld % 4 == 0; }
bool known_kind(int32_t k) { return k == DLRM_L16_FP32 || k == DLRM_L16_HALF; }

int linear16_dgrad(const char* fn, int32_t type, int64_t M, int64_t N, int64_t K, const void* dY,
                   int32_t dy_kind, int64_t lddy, const float* W, int64_t ldw, const void* mask,
                   int32_t mask_kind, int64_t ldmask, void* dX, int32_t dx_kind, int64_t lddx,
                   dlrm_stream_t stream) {
  using namespace dlrm;
  DLRM_ARG(type == DLRM_MLP16_BF16 || type == DLRM_MLP16_F16, "%s: unknown type %d", fn,
           (int)type);
  DLRM_ARG(known_kind(dy_kind) && known_kind(mask_kind) && known_kind(dx_kind),
           "%s: unknown operand kind", fn);
  DLRM_ARG(M >= 0 && N >= 0 && K >= 0, "%s: negative size", fn);
  if (M == 0 || K == 0) return DLRM_OK;
  DLRM_ARG(dX && (N == 0 || (dY && W)), "%s: null pointer", fn);
  DLRM_REQUIRE(lddy >= N && ldw >= K && lddx >= K && (!mask || ldmask >= K), DLRM_ERR_SHAPE,
               "%s: lddy %lld < N %lld or ldw %lld / lddx %lld / ldmask %lld "
               "< K %lld",
               fn, (long long)lddy, (long long)N, (long long)ldw, (long long)lddx,
               (long long)ldmask, (long long)K);
  const int a16 = dy_kind == DLRM_L16_HALF, o16 = dx_kind == DLRM_L16_HALF;
  // the mask is the activation whose gradient dX is: one boundary, one format
  DLRM_REQUIRE(!mask || mask_kind == dx_kind, DLRM_ERR_UNSUPPORTED,
               "%s: no kernel for a mask and a dX of different formats", fn);
  DLRM_REQUIRE(!a16 || (N % 8 == 0 && chunked(dY, lddy)), DLRM_ERR_SHAPE,
               "%s: a 16-bit dY needs N %lld and lddy %lld multiples of 8 and dY 16-byte aligned",
               fn, (long long)N, (long long)lddy);
  DLRM_REQUIRE(!o16 || (K % 8 == 0 && chunked(dX, lddx) && (!mask || chunked(mask, ldmask))),
               DLRM_ERR_SHAPE,
               "%s: a 16-bit dX (and its mask) needs K %lld and lddx %lld / ldmask %lld multiples "
               "of 8 and 16-byte aligned bases",
               fn, (long long)K, (long long)lddx, (long long)ldmask);
  const int64_t forced = tuning(DLRM_TUNE_LINEAR16_DGRAD_TILE);
  Tile t{int(forced / 1000), int(forced % 1000)};
  DLRM_ARG(forced == 0 || known_tile(t), "%s: DLRM_TUNE_LINEAR16_DGRAD_TILE %lld is not a tile",
           fn, (long long)forced);
  DLRM_REQUIRE(ceil_div(M, 32) * ceil_div(K, 64) <= INT32_MAX, DLRM_ERR_UNSUPPORTED,
               "%s: more than 2^31 - 1 tiles", fn);
  if (forced == 0) t = plan_dgrad(M, K, device_cus());
  BwdArgs a{};
  a.I = M, a.J = K, a.R = N;
  a.A = dY, a.lda = lddy, a.B = W, a.ldb = ldw;
  a.mask = mask, a.ldmask = ldmask, a.Out = dX, a.ldo = lddx;
  a.epi = kEpiDgrad, a.lr = 0.f;
  a.tiles_j = int(ceil_div(K, t.bn));
  a.tiles = int(ceil_div(M, t.bm)) * a.tiles_j;
  a.steps_per_split = ceil_div(N, kBK);
  const bool aligned = (a16 || vec32(dY, lddy)) && vec32(W, ldw);
  const bool ok = type == DLRM_MLP16_BF16
                      ? dispatch<__bf16, false>(t, a16, 0, o16, aligned, a, 1, as_stream(stream))
                      : dispatch<_Float16, false>(t, a16, 0, o16, aligned, a, 1, as_stream(stream));
  DLRM_REQUIRE(ok, DLRM_ERR_UNSUPPORTED, "%s: no kernel for the tile", fn);
  DLRM_LAUNCH_CHECK(fn);
  return DLRM_OK;
}
}  // namespace

extern "C" int dlrm_linear16_dgrad(int32_t type, int64_t M, int64_t N, int64_t K,
                                   const float* dY, int64_t lddy, const float* W, int64_t ldw,
                                   const float* mask, int64_t ldmask, float* dX, int64_t lddx,
                                   dlrm_stream_t stream) {
  return linear16_dgrad("dlrm_linear16_dgrad", type, M, N, K, dY, DLRM_L16_FP32, lddy, W, ldw,
                        mask, DLRM_L16_FP32, ldmask, dX, DLRM_L16_FP32, lddx, stream);
}

extern "C" int dlrm_linear16_dgrad_fmt(int32_t type, int64_t M, int64_t N, int64_t K,
                                       const void* dY, int32_t dy_kind, int64_t lddy,
                                       const float* W, int64_t ldw, const void* mask,
                                       int32_t mask_kind, int64_t ldmask, void* dX,
                                       int32_t dx_kind, int64_t lddx, dlrm_stream_t stream) {
  const char* fn = "dlrm_linear16_dgrad_fmt";
  DLRM_REQUIRE(dy_kind != DLRM_L16_FP32 || dx_kind != DLRM_L16_FP32, DLRM_ERR_UNSUPPORTED,
               "%s: fp32 dY to fp32 dX is dlrm_linear16_dgrad", fn);
  return linear16_dgrad(fn, type, M, N, K, dY, dy_kind, lddy, W, ldw, mask, mask_kind, ldmask,
                        dX, dx_kind, lddx, stream);
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
int linear16_wgrad(const char* fn, int32_t type, int64_t M, int64_t N, int64_t K, const void* dY,
                   int32_t dy_kind, int64_t lddy, const void* X, int32_t x_kind, int64_t ldx,
                   int32_t mode, float lr, const float* lr_dev, float* C, int64_t ldc,
                   void* workspace, size_t workspace_bytes, dlrm_stream_t stream) {
  using namespace dlrm;
  DLRM_ARG(known_kind(dy_kind) && known_kind(x_kind), "%s: unknown operand kind", fn);
  DLRM_ARG(type == DLRM_MLP16_BF16 || type == DLRM_MLP16_F16,
           "%s: unknown type %d", fn, (int)type);
  DLRM_ARG(mode == DLRM_WGRAD16_STORE || mode == DLRM_WGRAD16_SGD,
           "%s: unknown mode %d", fn, (int)mode);
  DLRM_ARG(M >= 0 && N >= 0 && K >= 0, "%s: negative size", fn);
  if (N == 0 || K == 0) return DLRM_OK;
  if (M == 0 && mode == DLRM_WGRAD16_SGD) return DLRM_OK;  // C - fl(lr * 0): C stays
  DLRM_ARG(C && (M == 0 || (dY && X)), "%s: null pointer", fn);
  DLRM_REQUIRE(lddy >= N && ldx >= K && ldc >= K, DLRM_ERR_SHAPE,
               "%s: lddy %lld < N %lld or ldx %lld / ldc %lld < K %lld", fn,
               (long long)lddy, (long long)N, (long long)ldx, (long long)ldc, (long long)K);
  DLRM_REQUIRE(ceil_div(N, 32) * ceil_div(K, 64) <= INT32_MAX &&
                   ceil_div(N * K, kThreads) <= INT32_MAX,
               DLRM_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 tiles", fn);
  // a 16-bit operand: whole chunks along its columns; its extent may end inside the last one
  // ([inp | 1]: K = width + 1), which is then read by element
  const int a16 = dy_kind == DLRM_L16_HALF, b16 = x_kind == DLRM_L16_HALF;
  DLRM_REQUIRE(M == 0 || ((!a16 || chunked(dY, lddy)) && (!b16 || chunked(X, ldx))),
               DLRM_ERR_SHAPE,
               "%s: a 16-bit operand needs a leading dimension (lddy %lld, ldx "
               "%lld) that is a multiple of 8 and a 16-byte aligned base", fn,
               (long long)lddy, (long long)ldx);
  WgradPlan w;
  DLRM_ARG(wgrad_plan_checked(M, N, K, &w),
           "%s: DLRM_TUNE_LINEAR16_WGRAD_TILE %lld is not a tile", fn,
           (long long)tuning(DLRM_TUNE_LINEAR16_WGRAD_TILE));
  const size_t need = w.splits > 1 ? size_t(w.splits) * size_t(N) * size_t(K) * sizeof(float) : 0;
  DLRM_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), DLRM_ERR_WORKSPACE,
               "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
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
  const bool aligned = (a16 || vec32(dY, lddy)) && (b16 || vec32(X, ldx));
  hipStream_t s = as_stream(stream);
  const bool ok = type == DLRM_MLP16_BF16
                      ? dispatch<__bf16, true>(w.tile, a16, b16, 0, aligned, a, w.splits, s)
                      : dispatch<_Float16, true>(w.tile, a16, b16, 0, aligned, a, w.splits, s);
  DLRM_REQUIRE(ok, DLRM_ERR_UNSUPPORTED, "%s: no kernel for the tile", fn);
  DLRM_LAUNCH_CHECK(fn);
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
  return linear16_wgrad("dlrm_linear16_wgrad", type, M, N, K, dY, DLRM_L16_FP32, lddy, X,
                        DLRM_L16_FP32, ldx, mode, lr,
                        nullptr, C, ldc, workspace, workspace_bytes, stream);
}

extern "C" int dlrm_linear16_wgrad_dev(int32_t type, int64_t M, int64_t N, int64_t K,
                                       const float* dY, int64_t lddy, const float* X,
                                       int64_t ldx, int32_t mode, const float* lr_dev, float* C,
                                       int64_t ldc, void* workspace, size_t workspace_bytes,
                                       dlrm_stream_t stream) {
  DLRM_ARG(lr_dev && mode == DLRM_WGRAD16_SGD,
           "dlrm_linear16_wgrad_dev: null lr_dev, or a mode other than DLRM_WGRAD16_SGD");
  return linear16_wgrad("dlrm_linear16_wgrad", type, M, N, K, dY, DLRM_L16_FP32, lddy, X,
                        DLRM_L16_FP32, ldx, mode, 0.f,
                        lr_dev, C, ldc, workspace, workspace_bytes, stream);
}

extern "C" int dlrm_linear16_wgrad_fmt(int32_t type, int64_t M, int64_t N, int64_t K,
                                       const void* dY, int32_t dy_kind, int64_t lddy,
                                       const void* X, int32_t x_kind, int64_t ldx, int32_t mode,
                                       float lr, float* C, int64_t ldc, void* workspace,
                                       size_t workspace_bytes, dlrm_stream_t stream) {
  DLRM_REQUIRE(dy_kind != DLRM_L16_FP32 || x_kind != DLRM_L16_FP32, DLRM_ERR_UNSUPPORTED,
               "dlrm_linear16_wgrad_fmt: fp32 dY and fp32 X is dlrm_linear16_wgrad");
  return linear16_wgrad("dlrm_linear16_wgrad_fmt", type, M, N, K, dY, dy_kind, lddy, X, x_kind,
                        ldx, mode, lr, nullptr, C,
                        ldc, workspace, workspace_bytes, stream);
}

extern "C" int dlrm_linear16_wgrad_fmt_dev(int32_t type, int64_t M, int64_t N, int64_t K,
                                           const void* dY, int32_t dy_kind, int64_t lddy,
                                           const void* X, int32_t x_kind, int64_t ldx,
                                           int32_t mode, const float* lr_dev, float* C,
                                           int64_t ldc, void* workspace, size_t workspace_bytes,
                                           dlrm_stream_t stream) {
  DLRM_ARG(lr_dev && mode == DLRM_WGRAD16_SGD,
           "dlrm_linear16_wgrad_fmt_dev: null lr_dev, or a mode other than DLRM_WGRAD16_SGD");
  DLRM_REQUIRE(dy_kind != DLRM_L16_FP32 || x_kind != DLRM_L16_FP32, DLRM_ERR_UNSUPPORTED,
               "dlrm_linear16_wgrad_fmt_dev: fp32 dY and fp32 X is dlrm_linear16_wgrad_dev");
  return linear16_wgrad("dlrm_linear16_wgrad_fmt_dev", type, M, N, K, dY, dy_kind, lddy, X,
                        x_kind, ldx, mode, 0.f, lr_dev, C,
                        ldc, workspace, workspace_bytes, stream);
}
