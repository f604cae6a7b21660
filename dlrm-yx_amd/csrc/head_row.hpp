// The DLRM head's per-row math, shared by the training head (misc.hip:
// head_fused_rows_kernel) and the forward-only head (metrics.hip: head_predict_kernel), so
// both write the same prob bits for the same X, w and clamp: one wave per row, lane l holds
// columns l + 64 c, one fmaf per column in c order, then the wave's xor-tree sum.
#pragma once
#include "head_roles.hpp"

namespace {

constexpr int kHeadRows = 4;  // rows per workgroup (one per wave)
constexpr int kHeadMaxK = 2048;

// This lane's weights w[lane + 64 c] (0 past K).
template <int NC>
__device__ __forceinline__ void head_load_w(const float* __restrict__ w, int64_t K, int lane,
                                            float (&wr)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int64_t k = lane + 64 * c;
    wr[c] = k < K ? w[k] : 0.f;
  }
}

// z = xr . w over the wave (every lane returns the sum); xv keeps this lane's inputs.
template <int NC>
__device__ __forceinline__ float head_row_dot(const float* __restrict__ xr, int64_t K, int lane,
                                              const float (&wr)[NC], float (&xv)[NC]) {
  float sacc = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int64_t k = lane + 64 * c;
    xv[c] = k < K ? xr[k] : 0.f;
    sacc = fmaf(xv[c], wr[c], sacc);
  }
  return wave_sum(sacc);
}

// sigmoid and the loss_threshold clamp: p, the clamped pc (the prob output), and whether p
// lay inside [lo, 1 - lo] (the clamp passes no gradient outside).
__device__ __forceinline__ void head_row_prob(float z, float lo, float& p, float& pc,
                                              bool& pass) {
  p = 1.f / (1.f + expf(-z));
  pc = p;
  pass = true;
  if (lo > 0.f && lo < 0.5f) {
    const float hi = 1.f - lo;
    pass = (p >= lo) && (p <= hi);
    pc = fminf(fmaxf(p, lo), hi);
  }
}

// Per-row loss math shared by the head kernels: returns (prob, dz, row loss).
__device__ __forceinline__ void head_row_math(float z, float t, int loss_kind, float lo,
                                              float gscale, float invM, float& pc, float& dzv,
                                              float& l) {
  float p;
  bool pass;
  head_row_prob(z, lo, p, pc, pass);
  float dp;
  if (loss_kind == DLRM_LOSS_BCE) {
    const float lp = fmaxf(logf(pc), -100.f);
    const float l1p = fmaxf(logf(1.f - pc), -100.f);
    l = -(t * lp + (1.f - t) * l1p);
    dp = (pc - t) / fmaxf((1.f - pc) * pc, 1e-12f) * invM;
  } else {
    const float d = pc - t;
    l = d * d;
    dp = 2.f * d * invM;
  }
  dp *= gscale;
  if (!pass) dp = 0.f;
  dzv = dp * (1.f - p) * p;
}

// The NC (64-column chunks per lane) the head kernels are instantiated for.
#define DLRM_HEAD_NC_DISPATCH(nc, HR)                                                         \
  do {                                                                                        \
    if ((nc) <= 2) HR(2); else if ((nc) <= 4) HR(4); else if ((nc) <= 5) HR(5);               \
    else if ((nc) <= 8) HR(8); else if ((nc) <= 12) HR(12); else if ((nc) <= 17) HR(17);      \
    else if ((nc) <= 24) HR(24); else HR(32);                                                 \
  } while (0)

}  // namespace
