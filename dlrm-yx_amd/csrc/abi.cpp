// Library-level entry points: version and thread-local error message.
#include <cstdarg>
#include <cstdio>

#include "common.hpp"

namespace dlrm {
namespace {
thread_local char g_last_error[1024] = {0};
constexpr int kTuneKeys = 13;
thread_local int64_t g_tuning[kTuneKeys] = {0};
}

int64_t tuning(int key) { return key > 0 && key < kTuneKeys ? g_tuning[key] : 0; }

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
  va_end(ap);
}
}  // namespace dlrm

// ABI v17 - v23: the version is only reported by a library that links the entry points it names
// (taking their addresses with the header's types fails the build if one is missing).
static_assert(DLRM_ABI_VERSION >= 23, "abi.cpp checks the v17 - v23 entry points");
namespace {
[[maybe_unused]] int (*const kLinear8Pack)(int64_t, int64_t, const float*, int64_t, int8_t*,
                                           int64_t, float*, void*, size_t,
                                           dlrm_stream_t) = &dlrm_linear8_pack;
[[maybe_unused]] int (*const kLinear8Range)(int64_t, int64_t, const float*, int64_t, float*,
                                            dlrm_stream_t) = &dlrm_linear8_range;
[[maybe_unused]] int (*const kLinear8Forward)(int64_t, int64_t, int64_t, const float*, int64_t,
                                              const float*, const int8_t*, int64_t, const float*,
                                              const float*, int64_t, int32_t, float*, int64_t,
                                              float*, dlrm_stream_t) = &dlrm_linear8_forward;
[[maybe_unused]] int (*const kRowsQuantize)(const void*, int32_t, int64_t, int64_t, int32_t, void*,
                                            int64_t, dlrm_stream_t) = &dlrm_rows_quantize;
[[maybe_unused]] int (*const kGatherRows)(int32_t, int32_t, int32_t, const float*, int64_t,
                                          const void*, int32_t, int64_t, const int64_t*,
                                          const int32_t*, int32_t, float*, int64_t, int32_t*,
                                          dlrm_stream_t) = &dlrm_interact_dot_forward_gather_rows;
[[maybe_unused]] int (*const kTbeAdagrad)(float*, float*, int64_t, const int64_t*, int32_t,
                                          int32_t, const void*, int32_t, const void*, int32_t,
                                          int64_t, int64_t, const float*, const float*, int64_t,
                                          float, const float*, float, int64_t, void*, size_t,
                                          int32_t*, int32_t,
                                          dlrm_stream_t) = &dlrm_tbe_backward_adagrad;
[[maybe_unused]] int (*const kForwardPool)(int32_t, int32_t, int32_t, const float*, int64_t,
                                           const void*, int32_t, int64_t, const int64_t*,
                                           const int32_t*, const int32_t*, int32_t, float*,
                                           int64_t, float*, int64_t, int32_t*,
                                           dlrm_stream_t) = &dlrm_interact_dot_forward_pool;
[[maybe_unused]] int (*const kChain16Supported)(const dlrm_mlp_chain16*) =
    &dlrm_mlp_chain16_supported;
[[maybe_unused]] int (*const kChain16Forward)(const dlrm_mlp_chain16*,
                                              dlrm_stream_t) = &dlrm_mlp_chain16_forward;
[[maybe_unused]] size_t (*const kBwd16GroupWs)(int32_t, int32_t, const dlrm_linear16_bwd_problem*) =
    &dlrm_linear16_bwd_group_workspace_size;
[[maybe_unused]] int (*const kBwd16Group)(int32_t, int32_t, const dlrm_linear16_bwd_problem*, void*,
                                          size_t, dlrm_stream_t) = &dlrm_linear16_bwd_group;
[[maybe_unused]] int (*const kTbeAdagradF16)(void*, float*, int64_t, const int64_t*, int32_t,
                                             int32_t, const void*, int32_t, const void*, int32_t,
                                             int64_t, int64_t, const float*, const float*,
                                             int64_t, float, const float*, float,
                                             const uint64_t*, int64_t, void*, size_t, int32_t*,
                                             int32_t,
                                             dlrm_stream_t) = &dlrm_tbe_backward_rowwise_adagrad_f16;
[[maybe_unused]] int (*const kLinear16Pack)(int32_t, int64_t, int64_t, const float*, int64_t, void*,
                                            int64_t, dlrm_stream_t) = &dlrm_linear16_pack;
[[maybe_unused]] int (*const kLinear16Packed)(int32_t, int64_t, int64_t, int64_t, const void*,
                                              int32_t, int64_t, const void*, int64_t,
                                              const float*, int64_t, int32_t, void*, int32_t,
                                              int64_t, dlrm_stream_t) = &dlrm_linear16_forward_packed;
[[maybe_unused]] int (*const kLinear16FwdFmt)(int32_t, int64_t, int64_t, int64_t, const void*,
                                              int32_t, int64_t, const float*, int64_t,
                                              const float*, int64_t, int32_t, void*, int32_t,
                                              int64_t, dlrm_stream_t) = &dlrm_linear16_forward_fmt;
[[maybe_unused]] int (*const kLinear16DgradFmt)(int32_t, int64_t, int64_t, int64_t, const void*,
                                                int32_t, int64_t, const float*, int64_t,
                                                const void*, int32_t, int64_t, void*, int32_t,
                                                int64_t, dlrm_stream_t) = &dlrm_linear16_dgrad_fmt;
[[maybe_unused]] int (*const kLinear16WgradFmt)(int32_t, int64_t, int64_t, int64_t, const void*,
                                                int32_t, int64_t, const void*, int32_t, int64_t,
                                                int32_t, float, float*, int64_t, void*, size_t,
                                                dlrm_stream_t) = &dlrm_linear16_wgrad_fmt;
[[maybe_unused]] int (*const kLinear16WgradFmtDev)(int32_t, int64_t, int64_t, int64_t,
                                                   const void*, int32_t, int64_t, const void*,
                                                   int32_t, int64_t, int32_t, const float*,
                                                   float*, int64_t, void*, size_t,
                                                   dlrm_stream_t) = &dlrm_linear16_wgrad_fmt_dev;
}  // namespace

extern "C" int dlrm_abi_version(void) { return DLRM_ABI_VERSION; }

extern "C" const char* dlrm_last_error(void) { return dlrm::g_last_error; }

extern "C" int dlrm_set_tuning(int32_t key, int64_t value) {
  DLRM_ARG(key >= DLRM_TUNE_GEMM_TILE && key <= DLRM_TUNE_LINEAR8_TILE,
           "dlrm_set_tuning: unknown key %d", (int)key);
  DLRM_ARG(value >= 0, "dlrm_set_tuning: negative value");
  dlrm::g_tuning[key] = value;
  return DLRM_OK;
}

extern "C" int64_t dlrm_get_tuning(int32_t key) { return dlrm::tuning(key); }
