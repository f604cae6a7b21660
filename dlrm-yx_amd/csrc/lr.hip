// Device-resident learning rates (ABI v14): the dlrm_lr_state block and the one-thread
// kernel that advances the reference's LRPolicyScheduler (dlrm_s_pytorch.py:188-222) on the
// device, so a replayed hipGraph walks the schedule with no host work.  Every update kernel
// reads its rate from the block's lr[] slots (the `_dev` entry points).  The fp16 tables'
// stochastic-rounding state (ABI v16) and its one-thread tick live here too.
//
// The arithmetic is fp64 in the reference's operation order with IEEE division (this file
// is built without any fast-math flag): lr[k] has the bits the host gets from
// (float)(policy(step_count, base[k]) * mult[k]).
#include <cstddef>
#include <cstring>

#include "common.hpp"

namespace {

struct LrState {
  int64_t step_count;
  int64_t W, S, D;
  int32_t n, pad;
  double base[DLRM_LR_MAX_SLOTS];
  double mult[DLRM_LR_MAX_SLOTS];
  float lr[DLRM_LR_MAX_SLOTS];
};
static_assert(sizeof(LrState) == DLRM_LR_STATE_BYTES, "dlrm_lr_state layout");
static_assert(offsetof(LrState, step_count) == DLRM_LR_OFF_STEP &&
                  offsetof(LrState, W) == DLRM_LR_OFF_POLICY &&
                  offsetof(LrState, n) == DLRM_LR_OFF_N &&
                  offsetof(LrState, base) == DLRM_LR_OFF_BASE &&
                  offsetof(LrState, mult) == DLRM_LR_OFF_MULT &&
                  offsetof(LrState, lr) == DLRM_LR_OFF_LR,
              "dlrm_lr_state layout");

// LRPolicyScheduler.get_lr for one base rate (x * x for the reference's x ** 2: equal for
// every decay fraction, tests/golden/lr_schedule.json).
__device__ __forceinline__ double lr_policy(int64_t sc, double base, int64_t W, int64_t S,
                                            int64_t D) {
#pragma clang fp contract(off)  // every product and difference rounded on its own, as on the host
  if (sc < W) return base * (1.0 - (double)(W - sc) / (double)W);
  if (D > 0) {
    if (sc < S) return base * (1.0 - 1.0 / (double)W);  // frozen at the value of sc = W - 1
    const int64_t last = S + D - 1;                     // frozen at the decay's last value
    const int64_t ds = (sc < last ? sc : last) - S;
    const double x = (double)(D - ds) / (double)D;
    const double v = base * (x * x);
    return v > 0.0000001 ? v : 0.0000001;
  }
  return base;
}

__global__ __launch_bounds__(64) void lr_tick_kernel(LrState* __restrict__ s) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t sc = s->step_count;
  const int64_t W = s->W, S = s->S, D = s->D;
  int n = s->n;
  if (n > DLRM_LR_MAX_SLOTS) n = DLRM_LR_MAX_SLOTS;
  for (int k = 0; k < n; ++k) s->lr[k] = (float)(lr_policy(sc, s->base[k], W, S, D) * s->mult[k]);
  s->step_count = sc + 1;
}

// dlrm_sr_state (ABI v16): uint64 seed, uint64 step; the update kernels only read it, so a
// replayed graph of {update, tick} draws a fresh stream every step with no host work.
static_assert(DLRM_SR_STATE_BYTES == 2 * sizeof(uint64_t), "dlrm_sr_state layout");
__global__ __launch_bounds__(64) void sr_tick_kernel(uint64_t* __restrict__ s) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  s[1] = s[1] + 1;
}

}  // namespace

extern "C" int dlrm_sr_tick(uint64_t* sr_state, dlrm_stream_t stream) {
  DLRM_ARG(sr_state && (reinterpret_cast<uintptr_t>(sr_state) & 7) == 0,
           "dlrm_sr_tick: sr_state must be an 8-byte aligned device pointer");
  hipLaunchKernelGGL(sr_tick_kernel, dim3(1), dim3(1), 0, dlrm::as_stream(stream), sr_state);
  DLRM_LAUNCH_CHECK("dlrm_sr_tick");
  return DLRM_OK;
}

extern "C" size_t dlrm_lr_state_bytes(void) { return sizeof(LrState); }

extern "C" int dlrm_lr_state_init(void* state_host, int64_t step_count, int64_t num_warmup_steps,
                                  int64_t decay_start_step, int64_t num_decay_steps, int32_t n,
                                  const double* base, const double* mult) {
  const char* name = "dlrm_lr_state_init";
  const int64_t W = num_warmup_steps, S = decay_start_step, D = num_decay_steps;
  DLRM_ARG(state_host && n >= 1 && n <= DLRM_LR_MAX_SLOTS && base && mult,
           "%s: null pointer or n outside 1..%d", name, DLRM_LR_MAX_SLOTS);
  DLRM_ARG(step_count >= 0 && W >= 0 && S >= 0 && D >= 0, "%s: negative step count", name);
  DLRM_ARG(S >= W, "%s: the warm-up (%lld steps) must finish before the decay starts (%lld)",
           name, (long long)W, (long long)S);
  DLRM_ARG(!(D > 0 && W < 2 && S > (W > 1 ? W : 1)),
           "%s: a plateau before the decay needs at least two warm-up steps", name);
  LrState s{};
  s.step_count = step_count, s.W = W, s.S = S, s.D = D, s.n = n;
  for (int k = 0; k < n; ++k) {
    s.base[k] = base[k], s.mult[k] = mult[k];
    s.lr[k] = (float)(base[k] * mult[k]);
  }
  std::memcpy(state_host, &s, sizeof(s));
  return DLRM_OK;
}

extern "C" int dlrm_lr_schedule_tick(void* state, dlrm_stream_t stream) {
  DLRM_ARG(state && (reinterpret_cast<uintptr_t>(state) & 7) == 0,
           "dlrm_lr_schedule_tick: state must be an 8-byte aligned device pointer");
  hipLaunchKernelGGL(lr_tick_kernel, dim3(1), dim3(1), 0, dlrm::as_stream(stream),
                     static_cast<LrState*>(state));
  DLRM_LAUNCH_CHECK("dlrm_lr_schedule_tick");
  return DLRM_OK;
}
