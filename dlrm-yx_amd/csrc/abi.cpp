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

// ABI v17 - v19: the version is only reported by a library that links the entry points it names
// (taking their addresses with the header's types fails the build if one is missing).
static_assert(DLRM_ABI_VERSION >= 19, "abi.cpp checks the v17 - v19 entry points");
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
