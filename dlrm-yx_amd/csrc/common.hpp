// Shared helpers for the gfx950 DLRM kernels (error plumbing, wave helpers).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "dlrm_hip.h"

namespace dlrm {

// Thread-local last-error message (dlrm_last_error()).
void set_error(const char* fmt, ...);

// Thread-local plan overrides of dlrm_set_tuning (autotuning sweeps and coverage tests of
// the alternative tiles / block lengths / sort paths); 0 = the planner's choice.  The
// library reads no environment variables.
int64_t tuning(int key);

inline hipStream_t as_stream(dlrm_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

constexpr int kWave = 64;  // CDNA wavefront width (never 32)

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace dlrm

// A learning rate that is either a host float baked into the kernel arguments or (ABI v14,
// the `_dev` entry points) one fp32 in device memory: resolved once at kernel entry, a
// wave-uniform load.  The pointer comes from the kernel arguments and no kernel that reads a
// rate writes it (its writer is an earlier kernel or copy, published by the kernel boundary),
// so the load goes through the constant address space: a scalar load into an SGPR, where the
// host float already lives - no vector register is spent on it.
#if defined(__HIPCC__)
__device__ __forceinline__ float dlrm_resolve_lr(const float* lr_dev, float lr) {
  typedef const float __attribute__((address_space(4))) * const_f32;
  return lr_dev ? *(const_f32)lr_dev : lr;
}

// The arithmetic of every scaled epilogue and fused SGD update: alpha * acc is rounded alone
// (dlrm_scale), then one rounded add or subtract - fl(old - fl(alpha * acc)), two roundings.
// Written as plain operators under contract(off), not as __fmul_rn / __fsub_rn / __fadd_rn:
// the HIP headers define those as `x * y`, `x - y`, `x + y` compiled under the translation
// unit's -ffp-contract=fast, and once inlined the pair does fuse into one v_fma_f32.  A
// product or sum without the contract flag fuses with nothing, whatever it is inlined into.
__device__ __forceinline__ float dlrm_scale(float alpha, float acc) {
#pragma clang fp contract(off)
  return alpha * acc;
}
__device__ __forceinline__ float dlrm_sgd_step(float old, float scaled) {
#pragma clang fp contract(off)
  return old - scaled;
}
__device__ __forceinline__ float dlrm_add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
#endif

#define DLRM_REQUIRE(cond, code, ...)   \
  do {                                  \
    if (!(cond)) {                      \
      dlrm::set_error(__VA_ARGS__);     \
      return (code);                    \
    }                                   \
  } while (0)

#define DLRM_ARG(cond, ...) DLRM_REQUIRE(cond, DLRM_ERR_INVALID_ARG, __VA_ARGS__)

#define DLRM_LAUNCH_CHECK(name)                                                        \
  do {                                                                                 \
    hipError_t e_ = hipGetLastError();                                                 \
    if (e_ != hipSuccess) {                                                            \
      dlrm::set_error("%s: HIP launch failed: %s", (name), hipGetErrorString(e_));     \
      return DLRM_ERR_HIP;                                                             \
    }                                                                                  \
  } while (0)

#define DLRM_HIP_CALL(expr, name)                                                      \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) {                                                            \
      dlrm::set_error("%s: %s failed: %s", (name), #expr, hipGetErrorString(e_));      \
      return DLRM_ERR_HIP;                                                             \
    }                                                                                  \
  } while (0)

// Workspace carving: 256-B aligned sub-buffers of one caller-provided block.
struct WsCarver {
  char* base;
  size_t used = 0;
  explicit WsCarver(void* p) : base(static_cast<char*>(p)) {}
  template <typename T>
  T* take(size_t count) {
    used = (used + 255) & ~size_t(255);
    T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
    used += count * sizeof(T);
    return p;
  }
};
