// Evaluation: the forward-only head, the device log of scored samples, and ROC-AUC /
// average precision from the sorted log (replaces the reference's inference() tail:
// Z_test to the host, numpy concatenate, sklearn on every sample; dlrm_s_pytorch.py:
// 1018-1162).
//
//  * dlrm_head_predict: last layer + sigmoid + clamp, prob only (head_row.hpp: the training
//    head's row math), optionally appending each row to a dlrm_eval_state.
//  * dlrm_eval_update: the same append for probabilities that already exist.
//  * dlrm_eval_metrics: global LSD radix sort of the packed keys (8-bit digits, four
//    passes: per-workgroup digit histogram, its scan, stable scatter), then one pass over
//    the tie groups of the sorted keys.  Integer results are exact; the average precision
//    is a double sum reduced in a fixed order (no floating-point atomics).
#include "common.hpp"
#include "head_row.hpp"

namespace {

// ---------------------------------------------------------------- the log ----
// One scored sample -> its key at keys[base + m] and its confusion class (0 TP, 1 FP, 2 TN,
// 3 FN; -1: the row was refused and an error bit raised).  Shared by the head and
// dlrm_eval_update.  The caller has checked base + m < capacity.
__device__ __forceinline__ int eval_log_row(const dlrm_eval_state& st, uint64_t base, int64_t m,
                                            float p, float t) {
  if (!(p >= 0.f && p <= 1.f)) {
    atomicOr(st.error, (uint32_t)DLRM_EVAL_ERR_SCORE);
    return -1;
  }
  if (!(t == 0.f || t == 1.f)) {
    atomicOr(st.error, (uint32_t)DLRM_EVAL_ERR_LABEL);
    return -1;
  }
  const uint32_t lab = t == 1.f ? 1u : 0u;
  st.keys[base + (uint64_t)m] = (__float_as_uint(p) << 1) | lab;  // (-0.f logs as +0.f)
  const bool pred = p > 0.5f;
  return pred ? (lab ? 0 : 1) : (lab ? 3 : 2);
}

// Where this launch appends: the cursor as every workgroup reads it (the follow-up launch
// advances it), or refuse the whole launch when its M rows do not fit.
__device__ __forceinline__ bool eval_launch_base(const dlrm_eval_state& st, int64_t M,
                                                 uint64_t& base) {
  base = *st.cursor;
  const bool fits = base <= (uint64_t)st.capacity && (uint64_t)M <= (uint64_t)st.capacity - base;
  if (!fits && blockIdx.x == 0 && threadIdx.x == 0)
    atomicOr(st.error, (uint32_t)DLRM_EVAL_ERR_OVERFLOW);
  return fits;
}

// The workgroup's confusion counts (cls[c][wave]: per-wave counts in LDS, written before the
// barrier the caller has passed) -> one integer atomic per non-zero counter.
__device__ __forceinline__ void eval_add_counts(const dlrm_eval_state& st,
                                                const uint32_t (&cls)[4][4]) {
  if (threadIdx.x < 4) {
    const int c = threadIdx.x;
    const uint32_t v = cls[c][0] + cls[c][1] + cls[c][2] + cls[c][3];
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(st.counts) + c, (unsigned long long)v);
  }
}

__global__ void eval_advance_kernel(dlrm_eval_state st, int64_t M) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const uint64_t base = *st.cursor;
    if (base <= (uint64_t)st.capacity && (uint64_t)M <= (uint64_t)st.capacity - base)
      *st.cursor = base + (uint64_t)M;
  }
}

// One wave per row (kHeadRows = 4 rows per workgroup), as head_fused_rows_kernel.
template <int NC>
__global__ __launch_bounds__(256) void head_predict_kernel(int64_t M, int64_t K,
                                                           const float* __restrict__ X,
                                                           int64_t ldx,
                                                           const float* __restrict__ w, float lo,
                                                           float* __restrict__ prob,
                                                           const float* __restrict__ target,
                                                           dlrm_eval_state st, int log) {
  __shared__ uint32_t cls[4][4];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  float wr[NC];
  head_load_w<NC>(w, K, lane, wr);
  uint64_t base = 0;
  const bool fits = log ? eval_launch_base(st, M, base) : false;
  if (log && threadIdx.x < 16) cls[threadIdx.x >> 2][threadIdx.x & 3] = 0;
  __syncthreads();
  const int64_t m = (int64_t)blockIdx.x * kHeadRows + wave;
  if (m < M) {
    float xv[NC];
    const float z = head_row_dot<NC>(X + m * ldx, K, lane, wr, xv);
    if (lane == 0) {
      float p, pc;
      bool pass;
      head_row_prob(z, lo, p, pc, pass);
      if (prob) prob[m] = pc;
      if (fits) {
        const int c = eval_log_row(st, base, m, pc, target[m]);
        if (c >= 0) cls[c][wave] = 1;
      }
    }
  }
  if (fits) {  // (uniform over the workgroup)
    __syncthreads();
    eval_add_counts(st, cls);
  }
}

constexpr int kUpdRows = 4;  // rows per thread of eval_update_kernel

__global__ __launch_bounds__(256) void eval_update_kernel(int64_t n,
                                                          const float* __restrict__ prob,
                                                          const float* __restrict__ target,
                                                          dlrm_eval_state st) {
  __shared__ uint32_t cls[4][4];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  uint64_t base = 0;
  if (!eval_launch_base(st, n, base)) return;  // (uniform over the launch)
  uint32_t cnt[4] = {0, 0, 0, 0};
  const int64_t r0 = (int64_t)blockIdx.x * (256 * kUpdRows);
#pragma unroll
  for (int u = 0; u < kUpdRows; ++u) {
    const int64_t m = r0 + u * 256 + threadIdx.x;
    const int c = m < n ? eval_log_row(st, base, m, prob[m], target[m]) : -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt[k] += (uint32_t)__popcll(__ballot(c == k));
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) cls[k][wave] = cnt[k];
  }
  __syncthreads();
  eval_add_counts(st, cls);
}

// ------------------------------------------------------------- radix sort ----
constexpr int kDigitBits = 8;
constexpr int kNB = 1 << kDigitBits;
constexpr int kTH = 256, kIT = 16, kW = kTH / 64;
constexpr int kTile = kTH * kIT;  // keys per tile
static_assert(kTile == DLRM_EVAL_SORT_TILE, "the header publishes the tile");
constexpr int kMaxSortWgs = 1024;  // workgroups of a pass (each owns a run of tiles)
constexpr int kCS = kW + 1;        // counter row stride (tbe_sort.hpp: distinct LDS banks)
constexpr uint32_t kPadKey = 0xffffffffu;  // past n: digit 255 in every pass, last in its tile

struct SortPlan {
  int64_t ntiles, tiles_per_wg;
  int wgs;
};

SortPlan sort_plan(int64_t n) {
  SortPlan p;
  p.ntiles = dlrm::ceil_div(n > 0 ? n : 1, kTile);
  p.tiles_per_wg = dlrm::ceil_div(p.ntiles, kMaxSortWgs);
  p.wgs = (int)dlrm::ceil_div(p.ntiles, p.tiles_per_wg);
  return p;
}

// Workgroup g's digit counts over its run of tiles -> hist[d * wgs + g] (digit-major: the
// exclusive scan of the flat array gives every (digit, workgroup) its first destination,
// workgroups of a digit in key order: stable).
__global__ __launch_bounds__(kTH) void sort_hist_kernel(const uint32_t* __restrict__ keys,
                                                        int64_t n, int shift,
                                                        int64_t tiles_per_wg, int64_t ntiles,
                                                        uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[kW][kNB];
  const int tid = threadIdx.x, w = tid >> 6;
  for (int i = tid; i < kW * kNB; i += kTH) (&h[0][0])[i] = 0;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * tiles_per_wg;
  const int64_t t1 = t0 + tiles_per_wg < ntiles ? t0 + tiles_per_wg : ntiles;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t e0 = t * kTile;
#pragma unroll
    for (int u = 0; u < kIT; ++u) {
      const int64_t e = e0 + u * kTH + tid;
      if (e < n) atomicAdd(&h[w][(keys[e] >> shift) & (kNB - 1)], 1u);
    }
  }
  __syncthreads();
  hist[(int64_t)tid * gridDim.x + blockIdx.x] = ((h[0][tid] + h[1][tid]) + h[2][tid]) + h[3][tid];
}

// Workgroup d: in-place exclusive scan of digit d's row of the histogram (one entry per
// sort workgroup, <= 1024) and the row's total.  The digits' own bases (the scan of the 256
// totals) are formed by every scatter workgroup itself.
static_assert(kMaxSortWgs <= 1024 && kNB == kTH, "one thread per workgroup entry / per digit");
__global__ __launch_bounds__(1024) void hist_row_scan_kernel(uint32_t* __restrict__ hist, int wgs,
                                                             uint32_t* __restrict__ totals) {
  __shared__ uint32_t wsum[16];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  uint32_t* row = hist + (int64_t)blockIdx.x * wgs;
  const uint32_t v = tid < wgs ? row[tid] : 0u;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(inc, o, 64);
    if (l >= o) inc += y;
  }
  if (l == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t run = inc - v;
#pragma unroll
  for (int k = 0; k < 16; ++k) run += k < w ? wsum[k] : 0u;
  if (tid < wgs) row[tid] = run;
  if (tid == 1023) totals[blockIdx.x] = run + v;
}

// In-place exclusive scan of count uint32 entries by ONE workgroup (thread t owns a
// contiguous chunk); *total = the sum (may be NULL).
__global__ __launch_bounds__(1024) void scan_u32_kernel(uint32_t* __restrict__ data,
                                                        int64_t count,
                                                        uint64_t* __restrict__ total) {
  __shared__ uint32_t wsum[16];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int64_t chunk = (count + 1023) / 1024;
  const int64_t a = (int64_t)tid * chunk < count ? (int64_t)tid * chunk : count;
  const int64_t b = a + chunk < count ? a + chunk : count;
  uint32_t s = 0;
  for (int64_t i = a; i < b; ++i) s += data[i];
  uint32_t inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(inc, o, 64);
    if (l >= o) inc += y;
  }
  if (l == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t run = inc - s;
  uint32_t all = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    run += k < w ? wsum[k] : 0u;
    all += wsum[k];
  }
  for (int64_t i = a; i < b; ++i) {
    const uint32_t v = data[i];
    data[i] = run;
    run += v;
  }
  if (total && tid == 0) *total = all;
}

struct SortLds {
  uint32_t key[kTile];
  uint32_t cnt[kNB * kCS];  // per (digit, wave): count, then tile-local first position
  uint32_t wsum[kW];
  uint32_t delta[kNB];      // digit -> (global destination - tile-local position)
};

// One stable pass: workgroup g walks its tiles in order.  Inside a tile the keys are ranked
// by the ballot idiom of tbe_sort.hpp (peers of a digit in the wave, the wave's running
// count in LDS, one scan over (digit, wave)), gathered digit-sorted in LDS, and written
// out in that order: a digit's keys of the tile go to consecutive addresses.  Thread d
// keeps digit d's next global destination across the tiles.
__global__ __launch_bounds__(kTH) void sort_scatter_kernel(const uint32_t* __restrict__ in,
                                                           uint32_t* __restrict__ out, int64_t n,
                                                           int shift, int64_t tiles_per_wg,
                                                           int64_t ntiles,
                                                           const uint32_t* __restrict__ hist,
                                                           const uint32_t* __restrict__ totals) {
  __shared__ SortLds sm;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const uint64_t below = (1ull << l) - 1;
  // digit tid's first destination: the keys of all smaller digits, then this digit's keys
  // of the workgroups before this one
  uint32_t goff;
  {
    const uint32_t tot = totals[tid];
    uint32_t inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(inc, o, 64);
      if (l >= o) inc += y;
    }
    if (l == 63) sm.wsum[w] = inc;
    __syncthreads();
    goff = inc - tot + hist[(int64_t)tid * gridDim.x + blockIdx.x];
#pragma unroll
    for (int k = 0; k < kW; ++k) goff += k < w ? sm.wsum[k] : 0u;
    __syncthreads();
  }
  const int64_t t0 = (int64_t)blockIdx.x * tiles_per_wg;
  const int64_t t1 = t0 + tiles_per_wg < ntiles ? t0 + tiles_per_wg : ntiles;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t e0 = t * kTile;
    const int nvalid = (int)(n - e0 < kTile ? n - e0 : kTile);
    uint32_t key[kIT];
#pragma unroll
    for (int u = 0; u < kIT; ++u) {  // wave-striped element order (tbe_sort.hpp)
      const int e = w * (kIT * 64) + u * 64 + l;
      key[u] = e < nvalid ? in[e0 + e] : kPadKey;
    }
    for (int i = tid; i < kNB * kCS; i += kTH) sm.cnt[i] = 0;
    __syncthreads();
    uint32_t rank[kIT];
#pragma unroll
    for (int u = 0; u < kIT; ++u) {
      const uint32_t d = (key[u] >> shift) & (kNB - 1);
      uint64_t peers = ~0ull;
#pragma unroll
      for (int b = 0; b < kDigitBits; ++b) {
        const uint64_t bal = __ballot((d >> b) & 1);
        peers &= ((d >> b) & 1) ? bal : ~bal;
      }
      const uint32_t r = __popcll(peers & below);
      const uint32_t c = __popcll(peers);
      const uint32_t base = sm.cnt[d * kCS + w];
      rank[u] = base + r;
      if (r == c - 1) sm.cnt[d * kCS + w] = base + c;  // last peer publishes
    }
    __syncthreads();
    // exclusive scan in (digit, wave) order: thread tid owns digit tid's kW counters
    uint32_t v[kW];
    uint32_t tsum = 0;
#pragma unroll
    for (int k = 0; k < kW; ++k) {
      v[k] = sm.cnt[tid * kCS + k];
      tsum += v[k];
    }
    uint32_t inc = tsum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(inc, o, 64);
      if (l >= o) inc += y;
    }
    if (l == 63) sm.wsum[w] = inc;
    __syncthreads();
    uint32_t run = inc - tsum;
#pragma unroll
    for (int k = 0; k < kW; ++k) run += k < w ? sm.wsum[k] : 0u;
    // digit tid: tile-local first position run, tsum keys (the pads sit in digit 255)
    const uint32_t valid = tid == kNB - 1 ? tsum - (uint32_t)(kTile - nvalid) : tsum;
    sm.delta[tid] = goff - run;
    goff += valid;
#pragma unroll
    for (int k = 0; k < kW; ++k) {
      sm.cnt[tid * kCS + k] = run;
      run += v[k];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kIT; ++u) {
      const uint32_t d = (key[u] >> shift) & (kNB - 1);
      sm.key[sm.cnt[d * kCS + w] + rank[u]] = key[u];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kIT; ++u) {
      const int e = u * kTH + tid;  // digit-sorted position; the pads are the last ones
      if (e < nvalid) {
        const uint32_t k = sm.key[e];
        const uint32_t dst = sm.delta[(k >> shift) & (kNB - 1)] + (uint32_t)e;
        if ((int64_t)dst < n) out[dst] = k;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------- tie groups ----
// Negatives (label bit 0) per tile of the sorted keys.
__global__ __launch_bounds__(kTH) void tile_neg_kernel(const uint32_t* __restrict__ keys,
                                                       int64_t n, uint32_t* __restrict__ tneg) {
  __shared__ uint32_t red[kW];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int64_t e0 = (int64_t)blockIdx.x * kTile;
  uint32_t c = 0;
#pragma unroll
  for (int u = 0; u < kIT; ++u) {
    const int64_t e = e0 + u * kTH + tid;
    c += (e < n && !(keys[e] & 1u)) ? 1u : 0u;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
  if (l == 0) red[w] = c;
  __syncthreads();
  if (tid == 0) tneg[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// First index in [a, n) whose key is >= target, given that every key before a is smaller:
// a doubling probe from a, then a binary search (the keys are sorted), so a group costs
// O(log of its length) loads wherever it ends - in this tile or many tiles on.
__device__ __forceinline__ int64_t gallop_lower_bound(const uint32_t* __restrict__ keys,
                                                      int64_t a, int64_t n, uint32_t target) {
  int64_t step = 1, b;
  for (;;) {
    b = a + step - 1;
    if (b >= n) {
      b = n;
      break;
    }
    if (keys[b] >= target) break;
    a = b + 1;
    step <<= 1;
  }
  while (a < b) {
    const int64_t mid = a + (b - a) / 2;
    if (keys[mid] < target) a = mid + 1; else b = mid;
  }
  return a;
}

struct GroupPartial {
  uint64_t a2, groups;
  double ap;
};

// The element that starts a tie group (its predecessor has another score) owns the group
// [s, e): m = its first positive (negatives sort first), neg_below = the negatives before s
// (the tile's scanned base + the in-tile ballot prefix).  Per tile: one partial, summed in a
// fixed order (thread-serial over its items, then a fixed LDS tree).
__global__ __launch_bounds__(kTH) void group_kernel(const uint32_t* __restrict__ keys, int64_t n,
                                                    const uint32_t* __restrict__ tneg_base,
                                                    const uint64_t* __restrict__ n_neg,
                                                    GroupPartial* __restrict__ part) {
  __shared__ uint32_t wtot[kW];
  __shared__ uint64_t ra[kTH], rg[kTH];
  __shared__ double rp[kTH];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const uint64_t below = (1ull << l) - 1;
  const int64_t e0 = (int64_t)blockIdx.x * kTile;
  const uint64_t N = *n_neg, P = (uint64_t)n - N;
  uint32_t key[kIT], pre[kIT];
  uint32_t wrun = 0;
#pragma unroll
  for (int u = 0; u < kIT; ++u) {
    const int64_t e = e0 + w * (kIT * 64) + u * 64 + l;
    key[u] = e < n ? keys[e] : kPadKey;
    const uint64_t nb = __ballot(e < n && !(key[u] & 1u));
    pre[u] = wrun + (uint32_t)__popcll(nb & below);
    wrun += (uint32_t)__popcll(nb);
  }
  if (l == 0) wtot[w] = wrun;
  __syncthreads();
  uint64_t nbase = tneg_base[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kW; ++k) nbase += k < w ? wtot[k] : 0u;
  uint64_t a2 = 0, groups = 0;
  double ap = 0.0;
#pragma unroll
  for (int u = 0; u < kIT; ++u) {
    const int64_t s = e0 + w * (kIT * 64) + u * 64 + l;
    if (s >= n) continue;
    const uint32_t score = key[u] >> 1;
    if (s > 0 && (keys[s - 1] >> 1) == score) continue;  // inside a group
    const int64_t e = gallop_lower_bound(keys, s + 1, n, (score + 1u) << 1);
    const int64_t m = (key[u] & 1u) ? s : gallop_lower_bound(keys, s + 1, e, key[u] | 1u);
    const uint64_t neg_g = (uint64_t)(m - s), pos_g = (uint64_t)(e - m);
    const uint64_t neg_below = nbase + pre[u];
    groups += 1;
    a2 += pos_g * (2 * neg_below + neg_g);
    if (pos_g && P) {
      const uint64_t tp = P - ((uint64_t)s - neg_below);  // positives scored >= this group
      ap += ((double)pos_g / (double)P) * ((double)tp / (double)((uint64_t)n - (uint64_t)s));
    }
  }
  ra[tid] = a2, rg[tid] = groups, rp[tid] = ap;
  __syncthreads();
  for (int o = kTH / 2; o >= 1; o >>= 1) {
    if (tid < o) ra[tid] += ra[tid + o], rg[tid] += rg[tid + o], rp[tid] += rp[tid + o];
    __syncthreads();
  }
  if (tid == 0) part[blockIdx.x] = GroupPartial{ra[0], rg[0], rp[0]};
}

// The tile partials in fixed order (thread t: tiles t, t + 256, ...; then a fixed tree).
__global__ __launch_bounds__(kTH) void group_final_kernel(int64_t n, int64_t ntiles,
                                                          const GroupPartial* __restrict__ part,
                                                          const uint64_t* __restrict__ n_neg,
                                                          uint64_t* __restrict__ out) {
  __shared__ uint64_t ra[kTH], rg[kTH];
  __shared__ double rp[kTH];
  const int tid = threadIdx.x;
  uint64_t a2 = 0, groups = 0;
  double ap = 0.0;
  for (int64_t t = tid; t < ntiles; t += kTH) {
    a2 += part[t].a2, groups += part[t].groups, ap += part[t].ap;
  }
  ra[tid] = a2, rg[tid] = groups, rp[tid] = ap;
  __syncthreads();
  for (int o = kTH / 2; o >= 1; o >>= 1) {
    if (tid < o) ra[tid] += ra[tid + o], rg[tid] += rg[tid + o], rp[tid] += rp[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const uint64_t N = *n_neg;
    out[0] = ra[0];
    out[1] = (uint64_t)n - N;
    out[2] = N;
    out[3] = rg[0];
    out[4] = (uint64_t)__double_as_longlong(rp[0]);
  }
}

struct MetricsWs {
  uint32_t* tmp;
  uint32_t* hist;
  uint32_t* totals;
  uint32_t* tneg;
  uint64_t* n_neg;
  GroupPartial* part;
  size_t bytes;
};

MetricsWs carve_metrics(void* ws, int64_t n) {
  const SortPlan p = sort_plan(n);
  WsCarver wc(ws);
  MetricsWs m;
  m.tmp = wc.take<uint32_t>((size_t)(n > 0 ? n : 1));
  m.hist = wc.take<uint32_t>((size_t)kNB * p.wgs);
  m.totals = wc.take<uint32_t>(kNB);
  m.tneg = wc.take<uint32_t>((size_t)p.ntiles);
  m.n_neg = wc.take<uint64_t>(1);
  m.part = wc.take<GroupPartial>((size_t)p.ntiles);
  m.bytes = wc.used + 256;
  return m;
}

int check_state(const dlrm_eval_state* s, const char* name) {
  DLRM_ARG(s->keys && s->cursor && s->counts && s->error && s->capacity > 0,
           "%s: incomplete dlrm_eval_state", name);
  return DLRM_OK;
}

}  // namespace

extern "C" int dlrm_head_predict(int64_t M, int64_t K, const float* X, int64_t ldx,
                                 const float* w, float clamp_lo, float* prob_out,
                                 const float* target, const dlrm_eval_state* state,
                                 dlrm_stream_t stream) {
  const char* name = "dlrm_head_predict";
  DLRM_ARG(M > 0 && K > 0, "%s: bad sizes", name);
  DLRM_ARG(X && w && ldx >= K, "%s: null X/w", name);
  DLRM_REQUIRE(K <= kHeadMaxK, DLRM_ERR_UNSUPPORTED, "%s: K > %d", name, kHeadMaxK);
  const int log = target && state;
  DLRM_ARG(prob_out || log, "%s: nothing to write (no prob_out, no state)", name);
  dlrm_eval_state st{};
  if (log) {
    if (int rc = check_state(state, name)) return rc;
    st = *state;
  }
  hipStream_t s = dlrm::as_stream(stream);
  const int64_t nblk = dlrm::ceil_div(M, kHeadRows);
  const int nc = (int)dlrm::ceil_div(K, 64);
#define HR(NC_)                                                                              \
  hipLaunchKernelGGL(head_predict_kernel<NC_>, dim3(nblk), dim3(256), 0, s, M, K, X, ldx, w, \
                     clamp_lo, prob_out, target, st, log)
  DLRM_HEAD_NC_DISPATCH(nc, HR);
#undef HR
  DLRM_LAUNCH_CHECK(name);
  if (log) {
    hipLaunchKernelGGL(eval_advance_kernel, dim3(1), dim3(64), 0, s, st, M);
    DLRM_LAUNCH_CHECK(name);
  }
  return DLRM_OK;
}

extern "C" int dlrm_eval_update(int64_t n, const float* prob, const float* target,
                                const dlrm_eval_state* state, dlrm_stream_t stream) {
  const char* name = "dlrm_eval_update";
  DLRM_ARG(n >= 0, "%s: bad n", name);
  if (n == 0) return DLRM_OK;
  DLRM_ARG(prob && target && state, "%s: null prob/target/state", name);
  if (int rc = check_state(state, name)) return rc;
  hipStream_t s = dlrm::as_stream(stream);
  const int64_t nblk = dlrm::ceil_div(n, 256 * kUpdRows);
  DLRM_ARG(nblk < (int64_t)1 << 31, "%s: n too large", name);
  hipLaunchKernelGGL(eval_update_kernel, dim3(nblk), dim3(256), 0, s, n, prob, target, *state);
  DLRM_LAUNCH_CHECK(name);
  hipLaunchKernelGGL(eval_advance_kernel, dim3(1), dim3(64), 0, s, *state, n);
  DLRM_LAUNCH_CHECK(name);
  return DLRM_OK;
}

extern "C" size_t dlrm_eval_metrics_workspace_size(int64_t n) {
  return carve_metrics(nullptr, n).bytes;
}

extern "C" int dlrm_eval_metrics(uint32_t* keys, int64_t n, void* workspace,
                                 size_t workspace_bytes, uint64_t* out, dlrm_stream_t stream) {
  const char* name = "dlrm_eval_metrics";
  DLRM_ARG(n >= 0 && n < ((int64_t)1 << 31), "%s: n outside [0, 2^31)", name);
  DLRM_ARG(out, "%s: null out", name);
  hipStream_t s = dlrm::as_stream(stream);
  if (n == 0) {
    DLRM_HIP_CALL(hipMemsetAsync(out, 0, 5 * sizeof(uint64_t), s), name);
    return DLRM_OK;
  }
  DLRM_ARG(keys && workspace, "%s: null keys/workspace", name);
  DLRM_REQUIRE(workspace_bytes >= dlrm_eval_metrics_workspace_size(n), DLRM_ERR_WORKSPACE,
               "%s: workspace too small", name);
  const SortPlan p = sort_plan(n);
  const MetricsWs m = carve_metrics(workspace, n);
  uint32_t* src = keys;
  uint32_t* dst = m.tmp;
  for (int shift = 0; shift < 32; shift += kDigitBits) {  // four passes: back in keys
    hipLaunchKernelGGL(sort_hist_kernel, dim3(p.wgs), dim3(kTH), 0, s, src, n, shift,
                       p.tiles_per_wg, p.ntiles, m.hist);
    hipLaunchKernelGGL(hist_row_scan_kernel, dim3(kNB), dim3(1024), 0, s, m.hist, p.wgs,
                       m.totals);
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(p.wgs), dim3(kTH), 0, s, src, dst, n, shift,
                       p.tiles_per_wg, p.ntiles, m.hist, m.totals);
    DLRM_LAUNCH_CHECK(name);
    uint32_t* t = src;
    src = dst;
    dst = t;
  }
  hipLaunchKernelGGL(tile_neg_kernel, dim3(p.ntiles), dim3(kTH), 0, s, keys, n, m.tneg);
  hipLaunchKernelGGL(scan_u32_kernel, dim3(1), dim3(1024), 0, s, m.tneg, p.ntiles, m.n_neg);
  hipLaunchKernelGGL(group_kernel, dim3(p.ntiles), dim3(kTH), 0, s, keys, n, m.tneg, m.n_neg,
                     m.part);
  hipLaunchKernelGGL(group_final_kernel, dim3(1), dim3(kTH), 0, s, n, p.ntiles, m.part, m.n_neg,
                     out);
  DLRM_LAUNCH_CHECK(name);
  return DLRM_OK;
}
