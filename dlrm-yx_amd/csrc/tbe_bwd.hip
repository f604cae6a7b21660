// Table-batched EmbeddingBag backward with the optimizer fused in — deterministic.
//
// Replaces the EmbeddingBag sparse backward + torch.optim.SGD sparse add_ of the
// reference step (dlrm_s_pytorch.py:1923-1934; exact-SGD TBE of create_emb_batched
// :321-334), the sparse branch of RWSAdagrad.step (optim/rwsadagrad.py:92-115) and
// torch.optim.Adagrad's sparse step (the reference's --optimizer adagrad, :1642; element-wise
// mode, one accumulator per weight).
//
// Pipeline (all on the caller's stream, no host sync, graph-capturable):
//  1. keys:    per lookup l, global row row_base[t] + idx[l] (or a sentinel) and its bag;
//  2. sort:    stable LSD radix sort of (row, l) pairs on ceil(log2 rows) bits (hand-written:
//              per-table LDS sort, tiled per-table passes, or device-wide passes; below);
//  3. blocks:  the sorted lookups are cut into fixed blocks (16 lookups; 64 from 2^18
//              lookups per call, tbe_bwd_roles.hpp CH / kLongCH).  One lane-group per
//              block walks them in order (row ids / grad-row offsets loaded coalesced and
//              broadcast by wave shuffles, four gradient rows in flight), summing the
//              gradient of each run of equal rows.  A run that starts and ends inside
//              the block is applied at once (one read + one write of the weight row);
//              a run crossing a block edge leaves its partial sum in slot
//              2*block + (segment starts at the block edge ? 0 : 1) — unique because a
//              block holds at most one continuing and one starting multi-block run;
//  4. combine: the block where a multi-block run starts sums its partials in block
//              order and applies the update.
// Skewed rows (the 3- and 4-row Terabyte tables receive ~700 lookups per row per
// batch) are thus split over many lane-groups instead of serialising one of them, and
// the summation order is fixed by the sort: bitwise reproducible run to run.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mlp_rows.hpp"
#include "tbe_bwd_roles.hpp"
#include "tbe_sort.hpp"
#include "tbe_common.hpp"
#include "tbe_dispatch.hpp"

namespace {


// ---------------------------------------------------------------- backward --
// Per-lookup key: global row (row_base[t] + idx) or sentinel (out of range / outside bags),
// its position and its bag.  One wave per bag (the lanes stride over the bag's lookups:
// coalesced, no search); the workgroups past the bags cover the lookups outside every bag
// (before off[0] / from off[T*B]).  KEYS = 0 (the tiled sort takes its keys from the
// indices itself): only bag_of, plus sentinel keys / positions of the outside lookups
// written straight into the sorted arrays (keys / pos then point at keys_out / pos_out).
constexpr int kBagWaves = 4;     // bags per 256-thread workgroup
constexpr int kOutsideBlocks = 16;
// (as a device function over 256-thread virtual blocks: the tiled sort's first launch runs
// it beside its pass-0 digit counts, tbe_keys_hist_kernel)
template <typename IdxT, typename OffT, typename KeyT, bool KEYS>
__device__ __forceinline__ void keys_body(
    int64_t blk, int tid, const IdxT* __restrict__ idx, const OffT* __restrict__ off,
    const int64_t* __restrict__ row_base, int T, int B, int64_t N, KeyT sentinel,
    KeyT* __restrict__ keys, int32_t* __restrict__ pos, int32_t* __restrict__ bag_of,
    int32_t* __restrict__ err) {
  constexpr int kDim = 256;
  const int64_t nb = (int64_t)T * B;
  const int64_t bag_blocks = (nb + kBagWaves - 1) / kBagWaves;
  const int lane = tid & 63;
  if (blk >= bag_blocks) {  // lookups outside every bag
    const int64_t a = (int64_t)off[0], e = (int64_t)off[nb];
    const int64_t stride = (int64_t)kOutsideBlocks * kDim;
    const int64_t g = (blk - bag_blocks) * kDim + tid;
    auto mark = [&](int64_t p) {  // (the tiled sort keeps these: -1 reads as "no bag" too
      keys[p] = sentinel;          //  when the sorted values are bags)
      pos[p] = KEYS ? (int32_t)p : -1;
      bag_of[p] = -1;
    };
    for (int64_t p = g; p < a && p < N; p += stride) mark(p);
    for (int64_t p = e + g; p < N; p += stride) mark(p);
    return;
  }
  const int64_t bag = blk * kBagWaves + (tid >> 6);
  if (bag >= nb) return;
  const int t = (int)(bag / B);
  const int64_t a = (int64_t)off[bag], e = (int64_t)off[bag + 1];
  const int64_t rb = row_base[t], nrows = row_base[t + 1] - rb;
  for (int64_t p = a + lane; p < e; p += 64) {
    const int64_t r = (int64_t)idx[p];
    const bool ok = r >= 0 && r < nrows;
    if (!ok && err) atomicOr(err, DLRM_TBE_ERR_INDEX);
    if constexpr (KEYS) {
      keys[p] = ok ? (KeyT)(rb + r) : sentinel;
      pos[p] = (int32_t)p;
    }
    bag_of[p] = ok ? (int32_t)bag : -1;
  }
}

template <typename IdxT, typename OffT, typename KeyT, bool KEYS>
__global__ __launch_bounds__(256) void tbe_bwd_keys_kernel(
    const IdxT* __restrict__ idx, const OffT* __restrict__ off, const int64_t* __restrict__ row_base,
    int T, int B, int64_t N, KeyT sentinel, KeyT* __restrict__ keys, int32_t* __restrict__ pos,
    int32_t* __restrict__ bag_of, int32_t* __restrict__ err) {
  keys_body<IdxT, OffT, KeyT, KEYS>(blockIdx.x, threadIdx.x, idx, off, row_base, T, B, N, sentinel,
                                    keys, pos, bag_of, err);
}

inline int64_t keys_grid(int T, int B) {
  return ((int64_t)T * B + kBagWaves - 1) / kBagWaves + kOutsideBlocks;
}

// Per-table sort (replaces keys + device radix sort when every table's lookups fit in
// one workgroup): workgroup t builds table t's local row keys (out-of-range rows ->
// rows_t) and sorts (key, position) with a stable LDS radix sort over only
// bit_width(rows_t) bits, then writes global rows / positions into the table's own range
// of the output.  Stable on positions, so the order equals the device-wide stable sort.
// Tables own disjoint row ranges and consecutive lookup ranges, so the concatenation is
// a valid grouping for the block kernel.  Workgroup T marks the lookups outside all bags
// (before off[0] / after off[T*B]) as sentinels.  A table with more than kSegCap lookups
// (the caller's max_lookups_per_table was an underestimate) is not sorted: all its lookups
// become sentinels (no update, no stale keys, no out-of-bounds row) and bit
// DLRM_TBE_ERR_TABLE_CAP is raised in *err.
constexpr int kSegThreads = 1024, kSegItems = 4;
constexpr int kSegCap = kSegThreads * kSegItems;  // lookups per table
using SegSortLds = SegLds<kSegThreads, kSegItems, false>;

template <typename IdxT, typename OffT>
__global__ __launch_bounds__(kSegThreads) void tbe_bwd_segsort_kernel(
    const IdxT* __restrict__ idx, const OffT* __restrict__ off, const int64_t* __restrict__ row_base,
    int T, int B, int64_t N, uint32_t sentinel, uint32_t* __restrict__ keys_out,
    int32_t* __restrict__ pos_out, int32_t* __restrict__ bag_of, int32_t* __restrict__ err) {
  __shared__ SegSortLds sm;
  segsort_body<kSegThreads, kSegItems, false, IdxT, OffT>(idx, off, row_base, T, B, N, sentinel,
                                                          keys_out, pos_out, bag_of, err,
                                                          blockIdx.x, sm);
}

// The forward gather and the backward's per-table sort in ONE launch: the sort depends only
// on the indices, and its T+1 latency-bound workgroups (LDS radix passes on T CUs) run beside
// the bandwidth-bound gather instead of as a separate launch in the backward.  Blocks
// [0, T] sort (started first), the rest gather.  512 threads per workgroup.
// With mlp_blocks > 0 a third role, the bottom MLP forward (mlp_rows.hpp), takes blocks
// [nsort, nsort+mlp_blocks): it reads only X and the bottom weights, independent of the rest.
// nsort = T + 1 with the sort, 0 without it (tables too large for the per-table LDS sort,
// e.g. C1's L = 100: the lookup and the bottom MLP still share one launch - the gather is
// HBM-bound, the MLP rides on MFMA and LDS).
constexpr int kPreThreads = kSegThreads;
static_assert(kPreThreads == kMlpWaves * 64, "one workgroup size for every role");
union PresortLds {
  SegSortLds sort;
  float mlp[kMlpLdsFloats];
};
template <int LPB, int VW, int MAXV, typename IdxT, typename OffT>
__global__ __launch_bounds__(kPreThreads) void tbe_fwd_presort_kernel(
    const float* __restrict__ W, int64_t D, const int64_t* __restrict__ row_base, int T, int B,
    const IdxT* __restrict__ idx, const OffT* __restrict__ off, const float* __restrict__ psw,
    float* __restrict__ out, int64_t out_bs, int32_t* __restrict__ err, int64_t N,
    uint32_t sentinel, uint32_t* __restrict__ keys_out, int32_t* __restrict__ pos_out,
    int32_t* __restrict__ bag_of, const MlpChain mc, int mlp_blocks, int nsort) {
  __shared__ __attribute__((aligned(16))) PresortLds sm;
  const int b = blockIdx.x;
  if (b < nsort) {
    segsort_body<kSegThreads, kSegItems, false, IdxT, OffT>(idx, off, row_base, T, B, N,
                                                            sentinel, keys_out, pos_out, bag_of,
                                                            err, b, sm.sort);
    return;
  }
  if (b < nsort + mlp_blocks) {
    mlp_rows_body(mc, b - nsort, sm.mlp);
    return;
  }
  const int g0 = nsort + mlp_blocks;
  tbe_fwd_body<LPB, VW, MAXV, IdxT, OffT>(W, D, row_base, T, B, idx, off, psw, out, out_bs, err,
                                          (int64_t)b - g0, (int64_t)gridDim.x - g0);
}

__global__ __launch_bounds__(kMlpWaves * 64) void mlp_chain_kernel(const MlpChain mc) {
  __shared__ __attribute__((aligned(16))) float lds[kMlpLdsFloats];
  mlp_rows_body(mc, blockIdx.x, lds);
}



// The per-table LDS sort applies (and dlrm_tbe_forward_presort can run it early).
inline bool presort_applies(int64_t max_seg, int64_t N) {
  return max_seg > 0 && max_seg <= kSegCap && N < (int64_t)0x7fffffff;
}

inline int bit_width_u64(uint64_t v) {
  int b = 0;
  while (v) {
    ++b;
    v >>= 1;
  }
  return b < 1 ? 1 : b;
}

// ------------------------------------------------ tiled per-table radix sort --
// Tables with more lookups than one workgroup sorts (kSegCap: e.g. L = 100 pooling) and
// 32-bit keys: a stable LSD radix sort of each table's (local row, position) pairs in its
// own lookup range, DB-bit digits, tiles of kTile lookups.  Per pass, three launches:
//   hist:    tile (t, j) counts its digits (LDS atomics) -> hist[t][d][j];
//   scan:    per table, exclusive scan of hist in (digit, tile) order;
//   scatter: tile (t, j) ranks its lookups by digit (wave ballots + per-(digit, wave)
//            running counts in LDS: element order kept, so stable) and writes each to
//            table start + hist[t][d][j] + its rank among the tile's digit-d lookups.
// Same (row, position) order as the device-wide sort and the per-table LDS sort; no
// memsets, no decoupled look-back.  The keys kernel has written bag_of (by lookup
// position) and the sentinels of the lookups outside every bag.  A table with more
// lookups than its J tiles cover (max_lookups_per_table underestimated) is not sorted: its
// range becomes sentinels (no update) and DLRM_TBE_ERR_TABLE_CAP is raised.
constexpr int kTileThreads = 1024, kTileItems = 4, kTile = kTileThreads * kTileItems;
constexpr int kTileWaves = kTileThreads / 64;
// the scatter pass: the same 4096-lookup tiles on 512 threads x 8 items - half the per-
// (digit, wave) counters, so two workgroups share a CU (C1 scatter 23.3 -> 18.5 us); the
// stable rank is by element index in either arrangement
constexpr int kScatThreads = 512, kScatItems = kTile / kScatThreads;
constexpr int kScatWaves = kScatThreads / 64;

struct TiledPass {
  const int64_t* row_base;
  int T, B, J;          // tables, bags per table, tiles per table
  int shift;            // digit shift of this pass
  int first, last;      // pass 0 reads the indices; the last pass writes global keys
  const uint32_t* kin;  // pass input (pass > 0)
  const int32_t* pin;
  uint32_t* kout;       // pass output
  int32_t* pout;
  uint32_t* hist;       // [T][2^DB][J]
  uint32_t sentinel;    // global sentinel key (last pass)
  int32_t* err;
  int global;           // one segment [0, n_all) of global keys read from kin/pin in pass 0
  int64_t n_all;
  const int32_t* bag_of;  // non-null: the sorted values are BAGS (bag_of[position], read
                          // coalesced in pass 0) instead of positions, so the block kernel
                          // reads each lookup's bag in sorted order (no dependent gather)
  // per-table passes (not global): a table of nrows rows needs ceil(bit_width(nrows) / DB)
  // passes, at most npass; pass ps of such a table reads / writes the (ka, pa) or the
  // final (ko, po) pair so that its own last pass lands in (ko, po), and passes past its
  // own count skip it (e.g. 1 M-row tables in an 8 M-row call: 2 passes of 10 bits, not 3)
  uint32_t* ka;
  int32_t* pa;
  uint32_t* ko;
  int32_t* po;
  int ps, npass;
  // the scan in chunks of JC tiles, C per table: csum[t][c][digit] = the chunk's counts
  uint32_t* csum;
  int C, JC;
  // wide scan (tiles per table <= kWideScanMaxJ): hist[t][j][d] becomes the count of digit
  // d in the table's tiles before j, csum[t][0][d] the digit's total; the scatter adds the
  // digit's start (the exclusive scan of the totals) itself
  int wide;
};

// The pass as table t sees it (global mode: the host's ping-pong as given).
struct PassView {
  bool skip, first, last;
  const uint32_t* kin;
  const int32_t* pin;
  uint32_t* kout;
  int32_t* pout;
  int shift;      // this pass's digit: (key >> shift) & mask
  uint32_t mask;
};

template <int DB>
__device__ __forceinline__ PassView pass_view(const TiledPass& a, int64_t nrows) {
  PassView v{};
  if (a.global) {
    v.first = a.first, v.last = a.last, v.kin = a.kin, v.pin = a.pin;
    v.kout = a.kout, v.pout = a.pout;
    v.shift = a.shift, v.mask = (1u << DB) - 1;
    return v;
  }
  int bits = 1;
  while (bits < 32 && ((int64_t)1 << bits) <= nrows) ++bits;  // keys in [0, nrows]
  int passes = (bits + DB - 1) / DB;
  if (passes > a.npass) passes = a.npass;
  // the table's bits split evenly over its passes (17 bits: 9 + 8, not 10 + 7): fewer
  // digits in the first pass, so each tile's runs per digit - the scatter's store segments -
  // are longer (a stable LSD sort by any digit split gives the same order)
  const int width = (bits + passes - 1) / passes < DB ? (bits + passes - 1) / passes : DB;
  v.shift = a.ps * width;
  v.mask = (1u << width) - 1;
  v.skip = a.ps >= passes;
  v.first = a.ps == 0;
  v.last = a.ps == passes - 1;
  const bool out_final = ((passes - 1 - a.ps) & 1) == 0;
  const bool in_final = ((passes - a.ps) & 1) == 0;
  v.kout = out_final ? a.ko : a.ka;
  v.pout = out_final ? a.po : a.pa;
  v.kin = a.ps == 0 ? nullptr : (in_final ? a.ko : a.ka);
  v.pin = a.ps == 0 ? nullptr : (in_final ? a.po : a.pa);
  return v;
}

template <int DB>
struct TiledLds {
  uint32_t cnt[(1 << DB) * (kScatWaves + 1)];  // per (digit, wave)
  uint32_t dstart[1 << DB];                     // tile-local start of each digit
  uint32_t wsum[kScatWaves];
  uint32_t dbase[1 << DB];                      // wide scan: the digit's start in the table
  uint32_t key[kTile];                          // the tile in digit order
  int32_t pos[kTile];
};

// Element e of tile j of table t: wave-striped (e = w*64*IT + u*64 + l), position
// s + j*kTile + e.  Loads this thread's IT (key, pos, valid).
template <int IT, typename IdxT, bool WITH_POS = true>
__device__ __forceinline__ void tiled_load(const TiledPass& a, const PassView& v,
                                           const IdxT* __restrict__ idx, int64_t s, int64_t n,
                                           int j, int64_t nrows, uint32_t (&key)[IT],
                                           int32_t (&pos)[IT], bool (&ok)[IT]) {
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
#pragma unroll
  for (int u = 0; u < IT; ++u) {
    const int64_t e = (int64_t)j * kTile + w * (IT * 64) + u * 64 + l;
    ok[u] = e < n;
    const int64_t p = s + (ok[u] ? e : 0);
    if (v.first && !a.global) {
      const int64_t r = (int64_t)idx[p];
      key[u] = (r >= 0 && r < nrows) ? (uint32_t)r : (uint32_t)nrows;
      if (WITH_POS) pos[u] = a.bag_of ? a.bag_of[p] : (int32_t)p;
    } else {
      key[u] = v.kin[p];
      if (WITH_POS)  // (global pass 0: pin[p] = p)
        pos[u] = (v.first && a.bag_of) ? a.bag_of[p] : v.pin[p];
    }
  }
}

template <typename OffT>
__device__ __forceinline__ bool tiled_range(const TiledPass& a, const OffT* __restrict__ off, int t,
                                            int64_t& s, int64_t& n) {
  if (a.global) {
    s = 0;
    n = a.n_all;
    return n <= (int64_t)a.J * kTile;
  }
  s = (int64_t)off[(int64_t)t * a.B];
  n = (int64_t)off[(int64_t)(t + 1) * a.B] - s;
  return n <= (int64_t)a.J * kTile;  // false: the table overflows its tiles
}

template <typename IdxT, typename OffT, int DB>
__device__ __forceinline__ void hist_body(const IdxT* __restrict__ idx,
                                          const OffT* __restrict__ off, const TiledPass& a,
                                          int blk, uint32_t* cnt) {
  constexpr int NB = 1 << DB;
  const int t = blk / a.J, j = blk - (blk / a.J) * a.J;
  int64_t s, n;
  const int64_t nrows = a.row_base[t + 1] - a.row_base[t];
  const PassView v = pass_view<DB>(a, nrows);
  if (v.skip) return;
  if (!tiled_range(a, off, t, s, n)) {
    if (v.first && j == 0 && threadIdx.x == 0 && a.err) atomicOr(a.err, DLRM_TBE_ERR_TABLE_CAP);
    return;
  }
  for (int d = threadIdx.x; d < NB; d += kTileThreads) cnt[d] = 0;
  uint32_t key[kTileItems];
  int32_t pos[kTileItems];
  bool ok[kTileItems];
  tiled_load<kTileItems, IdxT, false>(a, v, idx, s, n, j, nrows, key, pos, ok);
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kTileItems; ++u)
    if (ok[u]) atomicAdd(&cnt[(key[u] >> v.shift) & v.mask], 1u);
  __syncthreads();
  uint32_t* h = a.hist + ((int64_t)t * a.J + j) * NB;
  for (int d = threadIdx.x; d < NB; d += kTileThreads) h[d] = cnt[d];
}

template <typename IdxT, typename OffT, int DB>
__global__ __launch_bounds__(kTileThreads) void tbe_tiled_hist_kernel(
    const IdxT* __restrict__ idx, const OffT* __restrict__ off, const TiledPass a) {
  __shared__ uint32_t cnt[1 << DB];
  hist_body<IdxT, OffT, DB>(idx, off, a, blockIdx.x, cnt);
}

// The tiled sort's first launch: pass 0's digit counts (workgroups [0, T J): they read only
// the indices) beside the bag-parallel keys pass (the rest, four 256-thread keys blocks per
// workgroup: bag_of and the outside-bag sentinels, read first by pass 0's scatter).
struct KeysArgs {
  const int64_t* row_base;
  int T, B;
  int64_t N;
  uint32_t sentinel;
  uint32_t* keys;
  int32_t* pos;
  int32_t* bag_of;
  int32_t* err;
  int64_t blocks;  // 256-thread keys blocks (keys_grid)
};

template <typename IdxT, typename OffT, int DB>
__global__ __launch_bounds__(kTileThreads) void tbe_keys_hist_kernel(
    const IdxT* __restrict__ idx, const OffT* __restrict__ off, const TiledPass a,
    const KeysArgs k) {
  __shared__ uint32_t cnt[1 << DB];
  const int nh = a.T * a.J;
  if ((int)blockIdx.x < nh) {
    hist_body<IdxT, OffT, DB>(idx, off, a, blockIdx.x, cnt);
    return;
  }
  const int64_t vb = ((int64_t)blockIdx.x - nh) * (kTileThreads / 256) + (threadIdx.x >> 8);
  if (vb < k.blocks)
    keys_body<IdxT, OffT, uint32_t, false>(vb, threadIdx.x & 255, idx, off, k.row_base, k.T, k.B,
                                           k.N, k.sentinel, k.keys, k.pos, k.bag_of, k.err);
}

// The exclusive scan of a table's NB * J counts in (digit, tile) order, in two launches
// over chunks of JC tiles (a table of C chunks gets C workgroups in each: the device-wide
// sort's one segment of J = N / 4096 tiles no longer walks in one workgroup - C1 shape
// 2 x 51 -> ~2 x 5 us).  hist is [t][j][d]; a thread owns DPT digits.
//   csum: workgroup (t, c) sums each digit over its chunk's tiles -> csum[t][c][d];
//   scan: workgroup (t, c) adds up the chunk sums (all chunks: the digit totals, scanned
//         across the workgroup; chunks < c: this chunk's start) and rewrites its tiles'
//         counts as base + running count.
constexpr int kScanChunk = 16, kMaxScanChunks = 64;
// One chunk (the scan walks the tiles itself, no csum launch) up to kScanOneChunk tiles
// per table: the per-table sort's tables (C1: 50 tiles) keep one launch of T workgroups.
constexpr int kScanOneChunk = 64;
inline void plan_scan_chunks(TiledPass& a) {
  a.JC = (a.J + kMaxScanChunks - 1) / kMaxScanChunks;
  if (a.JC < kScanChunk) a.JC = kScanChunk;
  if (a.J <= kScanOneChunk) a.JC = a.J > 0 ? a.J : 1;
  a.C = (a.J + a.JC - 1) / a.JC;
}

template <int DB>
__global__ __launch_bounds__(kTileThreads) void tbe_tiled_csum_kernel(const TiledPass a,
                                                                      const void* off_v,
                                                                      int off_bits) {
  constexpr int NB = 1 << DB;
  constexpr int DPT = NB / kTileThreads > 0 ? NB / kTileThreads : 1;  // digits per thread
  const int t = blockIdx.x / a.C, c = blockIdx.x - (blockIdx.x / a.C) * a.C;
  const int tid = threadIdx.x;
  int64_t s, n;
  const PassView v = pass_view<DB>(a, a.row_base[t + 1] - a.row_base[t]);
  if (v.skip) return;
  const bool fits = off_bits == 32
                        ? tiled_range(a, static_cast<const int32_t*>(off_v), t, s, n)
                        : tiled_range(a, static_cast<const int64_t*>(off_v), t, s, n);
  const int d0 = tid * DPT;
  if (!fits || d0 >= NB) return;
  const uint32_t* h = a.hist + (int64_t)t * a.J * NB;
  const int j0 = c * a.JC, j1 = j0 + a.JC < a.J ? j0 + a.JC : a.J;
  constexpr int U = 32 / DPT;
  uint32_t tot[DPT];
#pragma unroll
  for (int q = 0; q < DPT; ++q) tot[q] = 0;
  for (int jj = j0; jj < j1; jj += U) {
    uint32_t x[U][DPT];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int q = 0; q < DPT; ++q)
        x[u][q] = (jj + u < j1) ? h[(int64_t)(jj + u) * NB + d0 + q] : 0u;
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int q = 0; q < DPT; ++q) tot[q] += x[u][q];
  }
#pragma unroll
  for (int q = 0; q < DPT; ++q) a.csum[((int64_t)t * a.C + c) * NB + d0 + q] = tot[q];
}

template <int DB>
__global__ __launch_bounds__(kTileThreads) void tbe_tiled_scan_kernel(const TiledPass a,
                                                                      const void* off_v,
                                                                      int off_bits) {
  constexpr int NB = 1 << DB;
  constexpr int DPT = NB / kTileThreads > 0 ? NB / kTileThreads : 1;  // digits per thread
  static_assert(NB % kTileThreads == 0 || kTileThreads % NB == 0, "digit map");
  __shared__ uint32_t wsum[kTileWaves];
  const int t = blockIdx.x / a.C, c = blockIdx.x - (blockIdx.x / a.C) * a.C;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  int64_t s, n;
  const PassView v = pass_view<DB>(a, a.row_base[t + 1] - a.row_base[t]);
  if (v.skip) return;
  const bool fits = off_bits == 32
                        ? tiled_range(a, static_cast<const int32_t*>(off_v), t, s, n)
                        : tiled_range(a, static_cast<const int64_t*>(off_v), t, s, n);
  if (!fits) {
    if (v.last && c == 0)  // the table's range holds sentinels (no update)
      for (int64_t i = tid; i < n; i += kTileThreads) {
        v.kout[s + i] = a.sentinel;
        v.pout[s + i] = (int32_t)(s + i);
      }
    return;
  }
  uint32_t* h = a.hist + (int64_t)t * a.J * NB;
  const int j0 = c * a.JC, j1 = j0 + a.JC < a.J ? j0 + a.JC : a.J;
  constexpr int U = 32 / DPT;
  // digits d0 .. d0+DPT-1 of this thread (NB < threads: the first NB threads only)
  const int d0 = tid * DPT;
  const bool active = d0 < NB;
  uint32_t tot[DPT], pre[DPT];
#pragma unroll
  for (int q = 0; q < DPT; ++q) tot[q] = pre[q] = 0;
  if (active && a.C == 1) {  // one chunk: the digit totals straight from the tiles
    for (int jj = j0; jj < j1; jj += U) {
      uint32_t x[U][DPT];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int q = 0; q < DPT; ++q)
          x[u][q] = (jj + u < j1) ? h[(int64_t)(jj + u) * NB + d0 + q] : 0u;
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int q = 0; q < DPT; ++q) tot[q] += x[u][q];
    }
  } else if (active) {
    const uint32_t* cs = a.csum + (int64_t)t * a.C * NB;
    for (int c0 = 0; c0 < a.C; c0 += U) {
      uint32_t x[U][DPT];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int q = 0; q < DPT; ++q)
          x[u][q] = (c0 + u < a.C) ? cs[(int64_t)(c0 + u) * NB + d0 + q] : 0u;
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int q = 0; q < DPT; ++q) {
          tot[q] += x[u][q];
          if (c0 + u < c) pre[q] += x[u][q];
        }
    }
  }
  uint32_t tsum = 0;
#pragma unroll
  for (int q = 0; q < DPT; ++q) tsum += tot[q];
  uint32_t inc = tsum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(inc, o, 64);
    if (l >= o) inc += y;
  }
  if (l == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t base = inc - tsum;
#pragma unroll
  for (int k = 0; k < kTileWaves; ++k) base += k < w ? wsum[k] : 0u;
  if (!active) return;
  uint32_t run[DPT];
#pragma unroll
  for (int q = 0; q < DPT; ++q) {
    run[q] = base + pre[q];
    base += tot[q];
  }
  for (int jj = j0; jj < j1; jj += U) {
    uint32_t x[U][DPT];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int q = 0; q < DPT; ++q)
        x[u][q] = (jj + u < j1) ? h[(int64_t)(jj + u) * NB + d0 + q] : 0u;
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int q = 0; q < DPT; ++q)
        if (jj + u < j1) {
          h[(int64_t)(jj + u) * NB + d0 + q] = run[q];
          run[q] += x[u][q];
        }
  }
}

// Wide scan: workgroup (t, g) takes digits [64 g, 64 g + 64) of table t - a lane per digit,
// wave w the tiles [w JW, (w + 1) JW) - and rewrites each (tile, digit) count as the digit's
// count over the earlier tiles; the digit totals go to csum[t][0][d].  T * 2^DB / 64
// workgroups, each one round of loads (the one-chunk scan: T workgroups walking all J
// tiles of all digits, C1 11.3 us).
constexpr int kWideScanMaxJ = 2048;
template <int DB>
__global__ __launch_bounds__(kTileThreads) void tbe_tiled_wide_scan_kernel(const TiledPass a,
                                                                           const void* off_v,
                                                                           int off_bits) {
  constexpr int NB = 1 << DB, G = NB / 64;
  __shared__ uint32_t ws[kTileWaves][64];
  const int t = blockIdx.x / G, g = blockIdx.x - (blockIdx.x / G) * G;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  int64_t s, n;
  const PassView v = pass_view<DB>(a, a.row_base[t + 1] - a.row_base[t]);
  if (v.skip) return;
  const bool fits = off_bits == 32
                        ? tiled_range(a, static_cast<const int32_t*>(off_v), t, s, n)
                        : tiled_range(a, static_cast<const int64_t*>(off_v), t, s, n);
  if (!fits) {
    if (v.last && g == 0)  // the table's range holds sentinels (no update)
      for (int64_t i = tid; i < n; i += kTileThreads) {
        v.kout[s + i] = a.sentinel;
        v.pout[s + i] = (int32_t)(s + i);
      }
    return;
  }
  const int d = g * 64 + l;
  uint32_t* h = a.hist + (int64_t)t * a.J * NB + d;
  const int JW = (a.J + kTileWaves - 1) / kTileWaves;
  const int j0 = w * JW, j1 = j0 + JW < a.J ? j0 + JW : a.J;
  constexpr int U = 8;
  uint32_t sum = 0;
  for (int jj = j0; jj < j1; jj += U) {
    uint32_t x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = jj + u < j1 ? h[(int64_t)(jj + u) * NB] : 0u;
#pragma unroll
    for (int u = 0; u < U; ++u) sum += x[u];
  }
  ws[w][l] = sum;
  __syncthreads();
  uint32_t run = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kTileWaves; ++k) {
    const uint32_t y = ws[k][l];
    run += k < w ? y : 0u;
    tot += y;
  }
  for (int jj = j0; jj < j1; jj += U) {
    uint32_t x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = jj + u < j1 ? h[(int64_t)(jj + u) * NB] : 0u;
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (jj + u < j1) {
        h[(int64_t)(jj + u) * NB] = run;
        run += x[u];
      }
  }
  if (w == 0) a.csum[(int64_t)t * NB + d] = tot;
}

template <typename IdxT, typename OffT, int DB>
__global__ __launch_bounds__(kScatThreads) void tbe_tiled_scatter_kernel(
    const IdxT* __restrict__ idx, const OffT* __restrict__ off, const TiledPass a) {
  constexpr int NB = 1 << DB;
  constexpr int CS = kScatWaves + 1;  // counter row stride
  __shared__ TiledLds<DB> sm;
  const int t = blockIdx.x / a.J, j = blockIdx.x - (blockIdx.x / a.J) * a.J;
  int64_t s, n;
  const int64_t rb = a.row_base[t];
  const int64_t nrows = a.row_base[t + 1] - rb;
  const PassView v = pass_view<DB>(a, nrows);
  if (v.skip) return;
  if (!tiled_range(a, off, t, s, n)) return;
  if ((int64_t)j * kTile >= n) return;  // empty tile (uniform)
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  uint32_t key[kScatItems];
  int32_t pos[kScatItems];
  bool ok[kScatItems];
  tiled_load<kScatItems>(a, v, idx, s, n, j, nrows, key, pos, ok);
  for (int i = tid; i < NB * CS; i += kScatThreads) sm.cnt[i] = 0;
  __syncthreads();
  const uint64_t below = (1ull << l) - 1;
  uint32_t rank[kScatItems], dig[kScatItems];
#pragma unroll
  for (int u = 0; u < kScatItems; ++u) {
    const uint32_t d = (key[u] >> v.shift) & v.mask;
    uint64_t peers = __ballot(ok[u]);
#pragma unroll
    for (int b = 0; b < DB; ++b) {
      const uint64_t bal = __ballot((d >> b) & 1);
      peers &= ((d >> b) & 1) ? bal : ~bal;
    }
    const uint32_t r = __popcll(peers & below);
    const uint32_t c = __popcll(peers);
    const uint32_t base = sm.cnt[d * CS + w];
    rank[u] = base + r;
    dig[u] = d;
    if (ok[u] && r == c - 1) sm.cnt[d * CS + w] = base + c;  // last peer publishes
  }
  __syncthreads();
  // per digit: exclusive prefix over the waves, and the digit's tile total
  constexpr int DPT = NB / kScatThreads > 0 ? NB / kScatThreads : 1;
  const int d0 = tid * DPT;
  uint32_t tot[DPT];
#pragma unroll
  for (int q = 0; q < DPT; ++q) {
    tot[q] = 0;
    if (d0 + q < NB) {
      uint32_t v[kScatWaves];
#pragma unroll
      for (int k = 0; k < kScatWaves; ++k) v[k] = sm.cnt[(d0 + q) * CS + k];
#pragma unroll
      for (int k = 0; k < kScatWaves; ++k) {
        sm.cnt[(d0 + q) * CS + k] = tot[q];
        tot[q] += v[k];
      }
    }
  }
  // tile-local digit starts: exclusive scan of the totals over the workgroup
  uint32_t tsum = 0;
#pragma unroll
  for (int q = 0; q < DPT; ++q) tsum += tot[q];
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
  for (int k = 0; k < kScatWaves; ++k) run += k < w ? sm.wsum[k] : 0u;
#pragma unroll
  for (int q = 0; q < DPT; ++q)
    if (d0 + q < NB) {
      sm.dstart[d0 + q] = run;
      run += tot[q];
    }
  __syncthreads();
  if (a.wide) {  // the digits' starts in the table: exclusive scan of the digit totals
    const uint32_t* dt = a.csum + (int64_t)t * NB;
    uint32_t x[DPT], xs = 0;
#pragma unroll
    for (int q = 0; q < DPT; ++q) {
      x[q] = d0 + q < NB ? dt[d0 + q] : 0u;
      xs += x[q];
    }
    uint32_t xi = xs;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(xi, o, 64);
      if (l >= o) xi += y;
    }
    if (l == 63) sm.wsum[w] = xi;  // (the tile-local reads of wsum are behind the barrier)
    __syncthreads();
    uint32_t xr = xi - xs;
#pragma unroll
    for (int k = 0; k < kScatWaves; ++k) xr += k < w ? sm.wsum[k] : 0u;
#pragma unroll
    for (int q = 0; q < DPT; ++q)
      if (d0 + q < NB) {
        sm.dbase[d0 + q] = xr;
        xr += x[q];
      }
    __syncthreads();
  }
  // stage the tile in digit order, then write it out: consecutive threads take
  // consecutive elements, so each digit's elements go out as one contiguous run
#pragma unroll
  for (int u = 0; u < kScatItems; ++u) {
    if (!ok[u]) continue;
    const uint32_t lp = sm.dstart[dig[u]] + sm.cnt[dig[u] * CS + w] + rank[u];
    sm.key[lp] = key[u];
    sm.pos[lp] = pos[u];
  }
  __syncthreads();
  const int nt = (int)((n - (int64_t)j * kTile) < kTile ? (n - (int64_t)j * kTile) : kTile);
  const uint32_t* h = a.hist + ((int64_t)t * a.J + j) * NB;
#pragma unroll
  for (int u = 0; u < kScatItems; ++u) {
    const int i = u * kScatThreads + tid;
    if (i >= nt) continue;
    const uint32_t k = sm.key[i];
    const uint32_t d = (k >> v.shift) & v.mask;
    const int64_t dst = s + h[d] + (a.wide ? sm.dbase[d] : 0u) + (i - sm.dstart[d]);
    if (v.last && !a.global)
      v.kout[dst] = k < (uint32_t)nrows ? (uint32_t)(rb + k) : a.sentinel;
    else
      v.kout[dst] = k;
    v.pout[dst] = sm.pos[i];
  }
}

// DB-bit digits, passes over `bits` key bits (local rows <= total_rows): 10-bit digits when
// they save a pass over 8-bit ones.
inline int tiled_digit_bits(int bits) {
  return (bits + 9) / 10 < (bits + 7) / 8 ? 10 : 8;
}

// The one place that turns a digit width into a template argument: f(int_tag<10 | 8>).
template <class F>
auto for_digit_bits(int db, F&& f) {
  return db == 10 ? f(int_tag<10>{}) : f(int_tag<8>{});
}

// ------------------------------------------------------------------ host path --
// One backward call as its entry point received it.  Every extern "C" entry point fills
// this by field name and adds the checks that are its own; everything below it takes the
// struct, so no list of same-typed neighbours (lr / eps, T / B, weights / momentum) is
// restated by hand.
struct BwdCall {
  const char* name;  // the entry point, for its messages
  int mode;          // MODE_* of the update (the sort-only entry has none)
  float* W;          // the weight rows (fp16 rows behind the cast) or the dense gradient buffer
  float* mom;        // row-wise momentum, element-wise state, or null
  int64_t D;
  const int64_t* row_base;
  int T, B;
  const void* idx;
  int index_bits;
  const void* off;
  int offset_bits;
  int64_t N, total_rows;
  const float* psw;
  const float* gout;
  int64_t gbs;
  float lr;             // the host rate; 0 where lr_dev replaces it
  const float* lr_dev;  // null, or the device fp32 read when the kernels run
  float eps;
  void* ws;
  size_t ws_bytes;
  int64_t max_seg;  // the caller's bound on any table's lookups (0: unknown)
  int32_t* err;
  int presorted;
  LaunchRole* role;  // non-null: the update's passes are deferred into this role
  const uint64_t* sr_state;
  dlrm_stream_t stream;
};

struct BwdWs {
  uint32_t* keys_in;
  uint32_t* keys_out;
  int32_t* pos_in;
  int32_t* pos_out;
  int32_t* bag_of;
  float* partial;  // block partials; the sorts' digit histograms before the block kernel
  size_t partial_words;
  size_t total;
};

BwdWs carve_bwd_ws(void* base, int64_t N, int64_t D) {
  BwdWs w{};
  WsCarver c(base);
  w.keys_in = c.take<uint32_t>(N);
  w.keys_out = c.take<uint32_t>(N);
  w.pos_in = c.take<int32_t>(N);
  w.pos_out = c.take<int32_t>(N);
  w.bag_of = c.take<int32_t>(N);
  const size_t part = (size_t)2 * ((N + CH - 1) / CH) * D;
  // global sort, 10-bit digits: per-tile counts + the scan's chunk sums
  const size_t hist = (size_t)((N + kTile - 1) / kTile) * 1024 + (size_t)kMaxScanChunks * 1024;
  w.partial_words = part > hist ? part : hist;
  w.partial = c.take<float>(w.partial_words);
  w.total = c.used + 256;
  return w;
}

// The tiled per-table sort of call c: J tiles per table, the digit histograms in the block
// kernel's partial buffer (free until the sort is done).  `bags`: see TiledPass::bag_of.
template <int DB, typename IdxT, typename OffT>
void launch_tiled_sort(const BwdCall& c, const IdxT* idx, const OffT* off, const BwdWs& w, int J,
                       const int32_t* bags, hipStream_t st) {
  const int T = c.T;
  const int off_bits = (int)sizeof(OffT) * 8;
  const uint32_t sentinel = (uint32_t)c.total_rows;
  uint32_t* hist = reinterpret_cast<uint32_t*>(w.partial);
  const KeysArgs keys{c.row_base, T, c.B, c.N, sentinel, w.keys_out, w.pos_out, w.bag_of, c.err,
                      keys_grid(T, c.B)};
  const int npass = (bit_width_u64((uint64_t)c.total_rows) + DB - 1) / DB;
  TiledPass a{};
  a.row_base = c.row_base, a.T = T, a.B = c.B, a.J = J, a.hist = hist, a.sentinel = sentinel;
  a.err = c.err;
  a.bag_of = bags;
  // per-table ping-pong (pass_view): each table's own last pass lands in (keys_out, pos_out)
  a.ka = w.keys_in, a.pa = w.pos_in, a.ko = w.keys_out, a.po = w.pos_out;
  a.npass = npass;
  plan_scan_chunks(a);
  a.csum = hist + (size_t)T * J * (1 << DB);  // after the per-tile counts
  a.wide = J <= kWideScanMaxJ && (1 << DB) % 64 == 0 && dlrm::tuning(DLRM_TUNE_TBE_SORT) != 2;
  // the keys pass rides on pass 0's count launch (tuning TBE_SORT 2: its own launch first)
  const bool merged = dlrm::tuning(DLRM_TUNE_TBE_SORT) != 2 &&
                      (int64_t)T * J + dlrm::ceil_div(keys.blocks, (int64_t)(kTileThreads / 256)) <
                          (int64_t)INT32_MAX;
  if (!merged)
    hipLaunchKernelGGL((tbe_bwd_keys_kernel<IdxT, OffT, uint32_t, false>), dim3(keys.blocks),
                       dim3(256), 0, st, idx, off, keys.row_base, keys.T, keys.B, keys.N,
                       keys.sentinel, keys.keys, keys.pos, keys.bag_of, keys.err);
  for (int ps = 0; ps < npass; ++ps) {
    a.shift = ps * DB;
    a.ps = ps;
    if (ps == 0 && merged)
      hipLaunchKernelGGL((tbe_keys_hist_kernel<IdxT, OffT, DB>),
                         dim3((unsigned)(T * J + dlrm::ceil_div(keys.blocks,
                                                                (int64_t)(kTileThreads / 256)))),
                         dim3(kTileThreads), 0, st, idx, off, a, keys);
    else
      hipLaunchKernelGGL((tbe_tiled_hist_kernel<IdxT, OffT, DB>), dim3(T * J), dim3(kTileThreads),
                         0, st, idx, off, a);
    if (a.wide)
      hipLaunchKernelGGL((tbe_tiled_wide_scan_kernel<DB>), dim3(T * ((1 << DB) / 64)),
                         dim3(kTileThreads), 0, st, a, static_cast<const void*>(off), off_bits);
    else if (a.C > 1)
      hipLaunchKernelGGL((tbe_tiled_csum_kernel<DB>), dim3(T * a.C), dim3(kTileThreads), 0, st,
                         a, static_cast<const void*>(off), off_bits);
    if (!a.wide)
      hipLaunchKernelGGL((tbe_tiled_scan_kernel<DB>), dim3(T * a.C), dim3(kTileThreads), 0, st,
                         a, static_cast<const void*>(off), off_bits);
    hipLaunchKernelGGL((tbe_tiled_scatter_kernel<IdxT, OffT, DB>), dim3(T * J),
                       dim3(kScatThreads), 0, st, idx, off, a);
  }
}

// The device-wide sort (no max_lookups_per_table bound): the tiled passes over ONE segment,
// the whole lookup array [0, N), of global keys (row_base[t] + row; sentinel for invalid
// and outside-bag lookups, written with their positions by the keys kernel into (k_x,
// p_x) = (keys_in, pos_in)).  Passes ping-pong between (k_x, p_x) and (k_y, p_y) =
// (keys_out, pos_out); returns true when the sorted pairs end in (k_y, p_y).  Stable: equal
// keys stay in position order, as a stable device-wide radix sort leaves them.
template <int DB, typename IdxT, typename OffT>
bool launch_global_sort(const BwdCall& c, const IdxT* idx, const OffT* off, const BwdWs& w,
                        const int32_t* bags, hipStream_t st) {
  uint32_t *const k_x = w.keys_in, *const k_y = w.keys_out;
  int32_t *const p_x = w.pos_in, *const p_y = w.pos_out;
  uint32_t* hist = reinterpret_cast<uint32_t*>(w.partial);
  const int npass = (bit_width_u64((uint64_t)c.total_rows) + DB - 1) / DB;
  TiledPass a{};
  a.row_base = c.row_base, a.T = 1, a.B = 1, a.hist = hist;
  a.sentinel = (uint32_t)c.total_rows, a.err = c.err;
  a.bag_of = bags;
  a.J = (int)dlrm::ceil_div(c.N, (int64_t)kTile);
  a.global = 1;
  a.n_all = c.N;
  plan_scan_chunks(a);
  a.csum = hist + (size_t)a.J * (1 << DB);
  a.wide = a.J <= kWideScanMaxJ && (1 << DB) % 64 == 0 && dlrm::tuning(DLRM_TUNE_TBE_SORT) != 2;
  for (int ps = 0; ps < npass; ++ps) {
    const bool fwd = (ps & 1) == 0;  // x -> y on even passes
    a.shift = ps * DB;
    a.first = ps == 0;
    a.last = ps == npass - 1;
    a.kin = fwd ? k_x : k_y;
    a.pin = fwd ? p_x : p_y;
    a.kout = fwd ? k_y : k_x;
    a.pout = fwd ? p_y : p_x;
    hipLaunchKernelGGL((tbe_tiled_hist_kernel<IdxT, OffT, DB>), dim3(a.J), dim3(kTileThreads), 0,
                       st, idx, off, a);
    if (a.wide)
      hipLaunchKernelGGL((tbe_tiled_wide_scan_kernel<DB>), dim3((1 << DB) / 64),
                         dim3(kTileThreads), 0, st, a, static_cast<const void*>(off),
                         (int)sizeof(OffT) * 8);
    else if (a.C > 1)
      hipLaunchKernelGGL((tbe_tiled_csum_kernel<DB>), dim3(a.C), dim3(kTileThreads), 0, st, a,
                         static_cast<const void*>(off), (int)sizeof(OffT) * 8);
    if (!a.wide)
      hipLaunchKernelGGL((tbe_tiled_scan_kernel<DB>), dim3(a.C), dim3(kTileThreads), 0, st, a,
                         static_cast<const void*>(off), (int)sizeof(OffT) * 8);
    hipLaunchKernelGGL((tbe_tiled_scatter_kernel<IdxT, OffT, DB>), dim3(a.J), dim3(kScatThreads),
                       0, st, idx, off, a);
  }
  return (npass & 1) == 1;
}

// The argument checks every backward entry point shares, in one order.  The sort-only entry
// takes no weights, gradient or presorted flag (with_update = false).
int check_bwd_call(const BwdCall& c, bool with_update) {
  DLRM_ARG((!with_update || (c.W && c.gout)) && c.row_base && (c.N == 0 || (c.idx && c.off)),
           "%s: null pointer", c.name);
  DLRM_ARG(!with_update || (c.presorted >= 0 && c.presorted <= DLRM_PRESORTED_ANY),
           "%s: bad presorted %d", c.name, c.presorted);
  DLRM_ARG(c.T > 0 && c.B > 0 && c.D > 0 && c.N >= 0 && c.total_rows > 0, "%s: bad sizes",
           c.name);
  DLRM_ARG(c.index_bits == 32 || c.index_bits == 64, "%s: index_bits must be 32 or 64", c.name);
  DLRM_ARG(c.offset_bits == 32 || c.offset_bits == 64, "%s: offset_bits must be 32 or 64",
           c.name);
  DLRM_REQUIRE(c.N < (int64_t)INT32_MAX && (int64_t)c.T * c.B < (int64_t)INT32_MAX,
               DLRM_ERR_UNSUPPORTED, "%s: more than 2^31 lookups/bags per call", c.name);
  DLRM_ARG(!with_update || c.gbs >= (int64_t)c.T * c.D, "%s: grad_batch_stride < T*D", c.name);
  DLRM_ARG(c.ws || c.N == 0, "%s: null workspace", c.name);
  // 32-bit row keys: the sorts key on global rows (< 2^32 - 1 rows per call, e.g. 2^32
  // rows of D = 16 fp32 is 275 GB, beyond one GPU's table budget; shard across calls)
  DLRM_REQUIRE((uint64_t)c.total_rows < 0xFFFFFFFFull, DLRM_ERR_UNSUPPORTED,
               "%s: %lld rows in one call (at most 2^32 - 2)", c.name, (long long)c.total_rows);
  return DLRM_OK;
}

int carve_checked(const BwdCall& c, BwdWs& w) {
  w = carve_bwd_ws(c.ws, c.N, c.D);
  DLRM_REQUIRE(c.ws_bytes >= w.total, DLRM_ERR_WORKSPACE, "%s: workspace %zu < required %zu",
               c.name, c.ws_bytes, w.total);
  return DLRM_OK;
}

// Where the sort stage left the lookups, grouped by row.
struct SortedRuns {
  const uint32_t* keys;   // global rows, ascending; the sentinel where there is no update
  const int32_t* pos;     // the sorted lookups' positions (their bags where the sort carried bags)
  const int32_t* bag_of;  // each lookup's bag: in sorted order (bags_sorted) or by position
  bool bags_sorted;
};

// The sort stage: this batch's (row, lookup) pairs sorted by row - already (presorted), or by
// the per-table LDS sort, the tiled per-table sort or the device-wide sort.
template <typename IdxT, typename OffT>
int sort_stage(const BwdCall& c, const IdxT* idx, const OffT* off, const BwdWs& w,
               SortedRuns& s) {
  hipStream_t st = dlrm::as_stream(c.stream);
  const int T = c.T;
  const int64_t N = c.N;
  const uint32_t sentinel = (uint32_t)c.total_rows;
  const int end_bit = bit_width_u64((uint64_t)c.total_rows);
  const bool per_table = presort_applies(c.max_seg, N);
  // large tables (> kSegCap lookups): the tiled per-table sort, its digit histograms in the
  // block kernel's partial buffer (free until the sort is done)
  const int64_t tiles_j = dlrm::ceil_div(c.max_seg > 0 ? c.max_seg : 1, (int64_t)kTile);
  const int tdb = tiled_digit_bits(end_bit);  // the device-wide sort (global keys)
  // the tiled sort passes over each table's OWN key bits (pass_view): 10-bit digits never
  // need more passes than 8-bit ones there, and only the tables that need them run them
  const int64_t part_space = (int64_t)w.partial_words;
  // per-tile counts + the scan's chunk sums (at most kMaxScanChunks per table)
  const int64_t sort_words = (int64_t)T * (tiles_j + kMaxScanChunks);
  const int tdb_t = sort_words * (1 << 10) <= part_space ? 10 : tdb;
  const bool tiled = !per_table && c.max_seg > kSegCap && N < (int64_t)0x7fffffff &&
                     (int64_t)T * tiles_j < (int64_t)INT32_MAX &&
                     sort_words * (1 << tdb_t) <= part_space &&
                     dlrm::tuning(DLRM_TUNE_TBE_SORT) != 1;
  // the tiled and global sorts carry each lookup's bag (not its position) when no
  // per-sample weights need the position: the block kernel then reads bags in sorted order
  const int32_t* bags = (!per_table && c.psw == nullptr) ? w.bag_of : nullptr;
  // every sort but the device-wide one ends in (keys_out, pos_out); that one ping-pongs from
  // (keys_in, pos_in) and ends there after an even number of passes
  bool in_out = true;
  if (c.presorted == DLRM_PRESORTED_ANY || (per_table && c.presorted)) {
    // this batch's sort already ran: inside dlrm_tbe_forward_presort (per-table), or in
    // dlrm_tbe_backward_sort (any variant; the device-wide one ends by its parity)
    if (!per_table && !tiled) in_out = ((end_bit + tdb - 1) / tdb) % 2 == 1;
  } else if (per_table) {
    hipLaunchKernelGGL((tbe_bwd_segsort_kernel<IdxT, OffT>), dim3(T + 1), dim3(kSegThreads), 0,
                       st, idx, off, c.row_base, T, c.B, N, sentinel, w.keys_out, w.pos_out,
                       w.bag_of, c.err);
  } else if (tiled) {
    for_digit_bits(tdb_t, [&](auto db) {
      launch_tiled_sort<decltype(db)::value>(c, idx, off, w, (int)tiles_j, bags, st);
    });
  } else {
    hipLaunchKernelGGL((tbe_bwd_keys_kernel<IdxT, OffT, uint32_t, true>), dim3(keys_grid(T, c.B)),
                       dim3(256), 0, st, idx, off, c.row_base, T, c.B, N, sentinel, w.keys_in,
                       w.pos_in, w.bag_of, c.err);
    DLRM_LAUNCH_CHECK(c.name);
    in_out = for_digit_bits(tdb, [&](auto db) {
      return launch_global_sort<decltype(db)::value>(c, idx, off, w, bags, st);
    });
  }
  DLRM_LAUNCH_CHECK(c.name);
  s.keys = in_out ? w.keys_out : w.keys_in;
  s.pos = in_out ? w.pos_out : w.pos_in;
  s.bags_sorted = per_table || bags;
  s.bag_of = per_table || !bags ? w.bag_of : s.pos;
  return DLRM_OK;
}

int run_sort(const BwdCall& c, const BwdWs& w, SortedRuns& s) {
  return for_csr_widths(c.index_bits, c.offset_bits, [&](auto i, auto o) {
    return sort_stage(c, i.ptr(c.idx), o.ptr(c.off), w, s);
  });
}

// The update's launch geometry.  It depends on the call alone, so it is planned (and a D
// the kernels do not cover refused) before the sort has enqueued anything.
struct UpdateGeom {
  bool vec4;
  LaneGeom lanes;
  int ch;          // sorted lookups per block
  int64_t blocks;  // workgroups of the block pass and of the combine pass
};

int plan_update(const BwdCall& c, UpdateGeom& u) {
  const bool f16_rows = c.mode == MODE_SGD_F16 || c.mode == MODE_SGD_F16_SR;
  // (element-wise Adagrad: the state rows are read and written like the weight rows)
  u.vec4 = (c.D % 4 == 0) && ((reinterpret_cast<uintptr_t>(c.W) & (f16_rows ? 7 : 15)) == 0) &&
           (c.mode != MODE_ADAGRAD_ELEM || (reinterpret_cast<uintptr_t>(c.mom) & 15) == 0) &&
           ((reinterpret_cast<uintptr_t>(c.gout) & 15) == 0) && (c.gbs % 4 == 0);
  u.lanes = lane_geom(u.vec4 ? c.D / 4 : c.D);
  DLRM_REQUIRE(u.lanes.maxv <= 8, DLRM_ERR_UNSUPPORTED, "%s: D=%lld too large", c.name,
               (long long)c.D);
  u.ch = c.N >= kLongChN ? kLongCH : CH;
  const int64_t tch = dlrm::tuning(DLRM_TUNE_TBE_BLOCK);  // (sweeps / coverage tests)
  if (tch == CH || tch == kLongCH) u.ch = (int)tch;
  u.blocks = lane_blocks(dlrm::ceil_div(c.N, (int64_t)u.ch), u.lanes.lpb, 4);
  return DLRM_OK;
}

// f(int_tag<MODE>): the update mode as a template argument.
template <class F>
void for_mode(int mode, F&& f) {
  switch (mode) {
    case MODE_SGD: return f(int_tag<MODE_SGD>{});
    case MODE_ADAGRAD: return f(int_tag<MODE_ADAGRAD>{});
    case MODE_SGD_F16: return f(int_tag<MODE_SGD_F16>{});
    case MODE_SGD_F16_SR: return f(int_tag<MODE_SGD_F16_SR>{});
    case MODE_ADAGRAD_ELEM: return f(int_tag<MODE_ADAGRAD_ELEM>{});
    default: return f(int_tag<MODE_DENSE>{});
  }
}

// The update stage: the block pass and the combine pass over the sorted lookups.
int update_stage(const BwdCall& c, const UpdateGeom& u, const SortedRuns& s, float* partial) {
  hipStream_t st = dlrm::as_stream(c.stream);
  const uint32_t sentinel = (uint32_t)c.total_rows;
  const int lpb = u.lanes.lpb;
  // the lean passes (4 gradient rows in flight per lane group at <= 128 VGPRs: twice the
  // resident waves of the 16-in-flight kernels, C1 block pass 100 -> ~65 us) wherever they
  // apply - deferred into later launches, or launched here
  if (u.vec4 && u.lanes.maxv == 1 && s.bags_sorted &&
      tbe_role_fusable(c.mode, lpb, c.psw, (int64_t)c.B * c.gbs) &&
      (c.role || dlrm::tuning(DLRM_TUNE_TBE_LEAN) != 1)) {
    LaunchRole local{};
    LaunchRole& r = c.role ? *c.role : local;
    r.W = c.W, r.mom = c.mom, r.psw = c.psw, r.gout = c.gout, r.partial = partial;
    r.keys = s.keys, r.pos = s.pos, r.bag_of = s.bag_of;
    r.D = c.D, r.gbs = c.gbs, r.N = c.N, r.lr = c.lr, r.lr_dev = c.lr_dev, r.eps = c.eps;
    r.sentinel = sentinel;
    r.B = c.B, r.ch = u.ch, r.mode = c.mode, r.lpb = lpb;
    // a multiple of 8 workgroups keeps the co-launched GEMM tiles' XCD remap aligned
    r.blocks = (int32_t)(dlrm::ceil_div(u.blocks, (int64_t)8) * 8);
    r.kind = kRoleUpdate;
    r.magic = kRoleMagic;
    if (c.role) return DLRM_OK;
    hipLaunchKernelGGL(tbe_update_pass_kernel<1>, dim3(r.blocks), dim3(256), 0, st, r);
    hipLaunchKernelGGL(tbe_update_pass_kernel<2>, dim3(r.blocks), dim3(256), 0, st, r);
    DLRM_LAUNCH_CHECK(c.name);
    return DLRM_OK;
  }
  for_row_width(u.vec4, [&](auto vw) {
    for_mode(c.mode, [&](auto mode) {
      for_lanes<1, 8>(u.lanes, [&](auto lanes, auto mv) {
        constexpr int LPB = decltype(lanes)::value, VW = decltype(vw)::value;
        constexpr int MV = decltype(mv)::value, MODE = decltype(mode)::value;
        const auto block = s.bags_sorted ? tbe_bwd_block_kernel<LPB, VW, MV, uint32_t, MODE, true>
                                         : tbe_bwd_block_kernel<LPB, VW, MV, uint32_t, MODE, false>;
        hipLaunchKernelGGL(block, dim3(u.blocks), dim3(256), 0, st, c.W, c.mom, c.D, c.B, s.keys,
                           s.pos, s.bag_of, c.psw, c.gout, c.gbs, c.N, c.lr, c.eps, sentinel,
                           partial, u.ch, c.lr_dev, c.sr_state);
        hipLaunchKernelGGL((tbe_bwd_combine_kernel<LPB, VW, MV, uint32_t, MODE>), dim3(u.blocks),
                           dim3(256), 0, st, c.W, c.mom, c.D, s.keys, c.N, c.lr, c.eps, sentinel,
                           partial, u.ch, c.lr_dev, c.sr_state);
      });
    });
  });
  DLRM_LAUNCH_CHECK(c.name);
  return DLRM_OK;
}

int bwd_dispatch(const BwdCall& c) {
  if (c.role) {  // until proven fusable: nothing deferred (the one place a role starts)
    *c.role = LaunchRole{};
    c.role->magic = kRoleMagic;
  }
  if (const int rc = check_bwd_call(c, true)) return rc;
  if (c.N == 0) return DLRM_OK;
  BwdWs w{};
  if (const int rc = carve_checked(c, w)) return rc;
  UpdateGeom u{};
  if (const int rc = plan_update(c, u)) return rc;
  SortedRuns s{};
  if (const int rc = run_sort(c, w, s)) return rc;
  return update_stage(c, u, s, w.partial);
}

// The deferred entries' own checks; their mode argument is 0 (sgd) | 1 (rowwise adagrad).
int bwd_defer(BwdCall& c, int32_t mode, dlrm_launch_role* role) {
  DLRM_ARG(role, "%s: null role", c.name);
  DLRM_ARG(mode == 0 || mode == 1, "%s: mode must be 0 (sgd) or 1 (rowwise adagrad)", c.name);
  DLRM_ARG(mode == 0 || c.mom, "%s: rowwise adagrad needs momentum", c.name);
  c.mode = mode == 0 ? MODE_SGD : MODE_ADAGRAD;
  if (mode == 0) c.mom = nullptr;
  c.role = reinterpret_cast<LaunchRole*>(role);
  return bwd_dispatch(c);
}

}  // namespace

extern "C" size_t dlrm_tbe_backward_workspace_size(int64_t num_lookups, int64_t total_rows,
                                                   int64_t D) {
  if (num_lookups <= 0) return 256;
  if (D < 1) D = 1;
  (void)total_rows;
  return carve_bwd_ws(nullptr, num_lookups, D).total;
}

extern "C" int dlrm_tbe_backward_sgd(float* weights, int64_t D, const int64_t* row_base,
                                     int32_t T, int32_t B, const void* indices,
                                     int32_t index_bits, const void* offsets,
                                     int32_t offset_bits, int64_t num_lookups,
                                     int64_t total_rows, const float* per_sample_weights,
                                     const float* grad_out, int64_t grad_batch_stride, float lr,
                                     int64_t max_lookups_per_table, void* workspace,
                                     size_t workspace_bytes, int32_t* error_flag,
                                     int32_t presorted, dlrm_stream_t stream) {
  BwdCall c{};
  c.name = "dlrm_tbe_backward_sgd", c.mode = MODE_SGD, c.W = weights;
  c.D = D, c.row_base = row_base, c.T = T, c.B = B;
  c.idx = indices, c.index_bits = index_bits, c.off = offsets, c.offset_bits = offset_bits;
  c.N = num_lookups, c.total_rows = total_rows, c.psw = per_sample_weights;
  c.gout = grad_out, c.gbs = grad_batch_stride, c.lr = lr;
  c.max_seg = max_lookups_per_table, c.ws = workspace, c.ws_bytes = workspace_bytes;
  c.err = error_flag, c.presorted = presorted, c.stream = stream;
  return bwd_dispatch(c);
}

extern "C" int dlrm_tbe_backward_sgd_dev(float* weights, int64_t D, const int64_t* row_base,
                                         int32_t T, int32_t B, const void* indices,
                                         int32_t index_bits, const void* offsets,
                                         int32_t offset_bits, int64_t num_lookups,
                                         int64_t total_rows, const float* per_sample_weights,
                                         const float* grad_out, int64_t grad_batch_stride,
                                         const float* lr_dev, int64_t max_lookups_per_table,
                                         void* workspace, size_t workspace_bytes,
                                         int32_t* error_flag, int32_t presorted,
                                         dlrm_stream_t stream) {
  DLRM_ARG(lr_dev, "dlrm_tbe_backward_sgd_dev: null lr_dev");
  BwdCall c{};
  c.name = "dlrm_tbe_backward_sgd_dev", c.mode = MODE_SGD, c.W = weights;
  c.D = D, c.row_base = row_base, c.T = T, c.B = B;
  c.idx = indices, c.index_bits = index_bits, c.off = offsets, c.offset_bits = offset_bits;
  c.N = num_lookups, c.total_rows = total_rows, c.psw = per_sample_weights;
  c.gout = grad_out, c.gbs = grad_batch_stride, c.lr_dev = lr_dev;
  c.max_seg = max_lookups_per_table, c.ws = workspace, c.ws_bytes = workspace_bytes;
  c.err = error_flag, c.presorted = presorted, c.stream = stream;
  return bwd_dispatch(c);
}

extern "C" int dlrm_tbe_backward_sgd_f16(void* weights, int64_t D, const int64_t* row_base,
                                         int32_t T, int32_t B, const void* indices,
                                         int32_t index_bits, const void* offsets,
                                         int32_t offset_bits, int64_t num_lookups,
                                         int64_t total_rows, const float* per_sample_weights,
                                         const float* grad_out, int64_t grad_batch_stride,
                                         float lr, int64_t max_lookups_per_table,
                                         void* workspace, size_t workspace_bytes,
                                         int32_t* error_flag, int32_t presorted,
                                         dlrm_stream_t stream) {
  BwdCall c{};
  c.name = "dlrm_tbe_backward_sgd_f16", c.mode = MODE_SGD_F16;
  c.W = static_cast<float*>(weights);
  c.D = D, c.row_base = row_base, c.T = T, c.B = B;
  c.idx = indices, c.index_bits = index_bits, c.off = offsets, c.offset_bits = offset_bits;
  c.N = num_lookups, c.total_rows = total_rows, c.psw = per_sample_weights;
  c.gout = grad_out, c.gbs = grad_batch_stride, c.lr = lr;
  c.max_seg = max_lookups_per_table, c.ws = workspace, c.ws_bytes = workspace_bytes;
  c.err = error_flag, c.presorted = presorted, c.stream = stream;
  return bwd_dispatch(c);
}

extern "C" int dlrm_tbe_backward_sgd_f16_dev(void* weights, int64_t D, const int64_t* row_base,
                                             int32_t T, int32_t B, const void* indices,
                                             int32_t index_bits, const void* offsets,
                                             int32_t offset_bits, int64_t num_lookups,
                                             int64_t total_rows, const float* per_sample_weights,
                                             const float* grad_out, int64_t grad_batch_stride,
                                             const float* lr_dev, int64_t max_lookups_per_table,
                                             void* workspace, size_t workspace_bytes,
                                             int32_t* error_flag, int32_t presorted,
                                             dlrm_stream_t stream) {
  DLRM_ARG(lr_dev, "dlrm_tbe_backward_sgd_f16_dev: null lr_dev");
  BwdCall c{};
  c.name = "dlrm_tbe_backward_sgd_f16_dev", c.mode = MODE_SGD_F16;
  c.W = static_cast<float*>(weights);
  c.D = D, c.row_base = row_base, c.T = T, c.B = B;
  c.idx = indices, c.index_bits = index_bits, c.off = offsets, c.offset_bits = offset_bits;
  c.N = num_lookups, c.total_rows = total_rows, c.psw = per_sample_weights;
  c.gout = grad_out, c.gbs = grad_batch_stride, c.lr_dev = lr_dev;
  c.max_seg = max_lookups_per_table, c.ws = workspace, c.ws_bytes = workspace_bytes;
  c.err = error_flag, c.presorted = presorted, c.stream = stream;
  return bwd_dispatch(c);
}

// ABI v16: the fp16 update with the store rounded stochastically; the stream's (seed, step)
// is read from sr_state when the kernels run, and advanced by dlrm_sr_tick only.
extern "C" int dlrm_tbe_backward_sgd_f16_sr(void* weights, int64_t D, const int64_t* row_base,
                                            int32_t T, int32_t B, const void* indices,
                                            int32_t index_bits, const void* offsets,
                                            int32_t offset_bits, int64_t num_lookups,
                                            int64_t total_rows, const float* per_sample_weights,
                                            const float* grad_out, int64_t grad_batch_stride,
                                            float lr, const float* lr_dev,
                                            const uint64_t* sr_state,
                                            int64_t max_lookups_per_table, void* workspace,
                                            size_t workspace_bytes, int32_t* error_flag,
                                            int32_t presorted, dlrm_stream_t stream) {
  BwdCall c{};
  c.name = "dlrm_tbe_backward_sgd_f16_sr", c.mode = MODE_SGD_F16_SR;
  DLRM_ARG(sr_state && (reinterpret_cast<uintptr_t>(sr_state) & 7) == 0,
           "%s: sr_state must be an 8-byte aligned device pointer", c.name);
  c.W = static_cast<float*>(weights);
  c.D = D, c.row_base = row_base, c.T = T, c.B = B;
  c.idx = indices, c.index_bits = index_bits, c.off = offsets, c.offset_bits = offset_bits;
  c.N = num_lookups, c.total_rows = total_rows, c.psw = per_sample_weights;
  c.gout = grad_out, c.gbs = grad_batch_stride;
  c.lr = lr_dev ? 0.f : lr, c.lr_dev = lr_dev, c.sr_state = sr_state;
  c.max_seg = max_lookups_per_table, c.ws = workspace, c.ws_bytes = workspace_bytes;
  c.err = error_flag, c.presorted = presorted, c.stream = stream;
  return bwd_dispatch(c);
}

extern "C" int dlrm_tbe_backward_rowwise_adagrad(
    float* weights, float* momentum, int64_t D, const int64_t* row_base, int32_t T, int32_t B,
    const void* indices, int32_t index_bits, const void* offsets, int32_t offset_bits,
    int64_t num_lookups, int64_t total_rows, const float* per_sample_weights,
    const float* grad_out, int64_t grad_batch_stride, float lr, float eps,
    int64_t max_lookups_per_table, void* workspace, size_t workspace_bytes, int32_t* error_flag,
    int32_t presorted, dlrm_stream_t stream) {
  DLRM_ARG(momentum, "dlrm_tbe_backward_rowwise_adagrad: null momentum");
  BwdCall c{};
  c.name = "dlrm_tbe_backward_rowwise_adagrad", c.mode = MODE_ADAGRAD;
  c.W = weights, c.mom = momentum;
  c.D = D, c.row_base = row_base, c.T = T, c.B = B;
  c.idx = indices, c.index_bits = index_bits, c.off = offsets, c.offset_bits = offset_bits;
  c.N = num_lookups, c.total_rows = total_rows, c.psw = per_sample_weights;
  c.gout = grad_out, c.gbs = grad_batch_stride, c.lr = lr, c.eps = eps;
  c.max_seg = max_lookups_per_table, c.ws = workspace, c.ws_bytes = workspace_bytes;
  c.err = error_flag, c.presorted = presorted, c.stream = stream;
  return bwd_dispatch(c);
}

extern "C" int dlrm_tbe_backward_rowwise_adagrad_dev(
    float* weights, float* momentum, int64_t D, const int64_t* row_base, int32_t T, int32_t B,
    const void* indices, int32_t index_bits, const void* offsets, int32_t offset_bits,
    int64_t num_lookups, int64_t total_rows, const float* per_sample_weights,
    const float* grad_out, int64_t grad_batch_stride, const float* lr_dev, float eps,
    int64_t max_lookups_per_table, void* workspace, size_t workspace_bytes, int32_t* error_flag,
    int32_t presorted, dlrm_stream_t stream) {
  BwdCall c{};
  c.name = "dlrm_tbe_backward_rowwise_adagrad_dev", c.mode = MODE_ADAGRAD;
  DLRM_ARG(momentum && lr_dev, "%s: null momentum or lr_dev", c.name);
  c.W = weights, c.mom = momentum;
  c.D = D, c.row_base = row_base, c.T = T, c.B = B;
  c.idx = indices, c.index_bits = index_bits, c.off = offsets, c.offset_bits = offset_bits;
  c.N = num_lookups, c.total_rows = total_rows, c.psw = per_sample_weights;
  c.gout = grad_out, c.gbs = grad_batch_stride, c.lr_dev = lr_dev, c.eps = eps;
  c.max_seg = max_lookups_per_table, c.ws = workspace, c.ws_bytes = workspace_bytes;
  c.err = error_flag, c.presorted = presorted, c.stream = stream;
  return bwd_dispatch(c);
}

// ABI v19: element-wise Adagrad (torch.optim.Adagrad, dlrm_s_pytorch.py:1642) on the rows
// the batch touched; state_sum is [total_rows, D] fp32 in the layout of weights.
extern "C" int dlrm_tbe_backward_adagrad(
    float* weights, float* state_sum, int64_t D, const int64_t* row_base, int32_t T, int32_t B,
    const void* indices, int32_t index_bits, const void* offsets, int32_t offset_bits,
    int64_t num_lookups, int64_t total_rows, const float* per_sample_weights,
    const float* grad_out, int64_t grad_batch_stride, float lr, const float* lr_dev, float eps,
    int64_t max_lookups_per_table, void* workspace, size_t workspace_bytes, int32_t* error_flag,
    int32_t presorted, dlrm_stream_t stream) {
  DLRM_ARG(state_sum, "dlrm_tbe_backward_adagrad: null state_sum");
  BwdCall c{};
  c.name = "dlrm_tbe_backward_adagrad", c.mode = MODE_ADAGRAD_ELEM;
  c.W = weights, c.mom = state_sum;
  c.D = D, c.row_base = row_base, c.T = T, c.B = B;
  c.idx = indices, c.index_bits = index_bits, c.off = offsets, c.offset_bits = offset_bits;
  c.N = num_lookups, c.total_rows = total_rows, c.psw = per_sample_weights;
  c.gout = grad_out, c.gbs = grad_batch_stride;
  c.lr = lr_dev ? 0.f : lr, c.lr_dev = lr_dev, c.eps = eps;
  c.max_seg = max_lookups_per_table, c.ws = workspace, c.ws_bytes = workspace_bytes;
  c.err = error_flag, c.presorted = presorted, c.stream = stream;
  return bwd_dispatch(c);
}

extern "C" int dlrm_tbe_backward_dense(float* grad_weights, int64_t D, const int64_t* row_base,
                                       int32_t T, int32_t B, const void* indices,
                                       int32_t index_bits, const void* offsets,
                                       int32_t offset_bits, int64_t num_lookups,
                                       int64_t total_rows, const float* per_sample_weights,
                                       const float* grad_out, int64_t grad_batch_stride,
                                       int64_t max_lookups_per_table, void* workspace,
                                       size_t workspace_bytes, int32_t* error_flag,
                                       int32_t presorted, dlrm_stream_t stream) {
  BwdCall c{};
  c.name = "dlrm_tbe_backward_dense", c.mode = MODE_DENSE, c.W = grad_weights;
  c.D = D, c.row_base = row_base, c.T = T, c.B = B;
  c.idx = indices, c.index_bits = index_bits, c.off = offsets, c.offset_bits = offset_bits;
  c.N = num_lookups, c.total_rows = total_rows, c.psw = per_sample_weights;
  c.gout = grad_out, c.gbs = grad_batch_stride;
  c.max_seg = max_lookups_per_table, c.ws = workspace, c.ws_bytes = workspace_bytes;
  c.err = error_flag, c.presorted = presorted, c.stream = stream;
  return bwd_dispatch(c);
}

static_assert(sizeof(LaunchRole) <= sizeof(dlrm_launch_role), "dlrm_launch_role too small");

// The sort stage alone: no update, so no weights, gradient, mode or D refusal.
extern "C" int dlrm_tbe_backward_sort(int64_t D, const int64_t* row_base, int32_t T, int32_t B,
                                      const void* indices, int32_t index_bits,
                                      const void* offsets, int32_t offset_bits,
                                      int64_t num_lookups, int64_t total_rows,
                                      const float* per_sample_weights,
                                      int64_t max_lookups_per_table, void* workspace,
                                      size_t workspace_bytes, int32_t* error_flag,
                                      dlrm_stream_t stream) {
  BwdCall c{};
  c.name = "dlrm_tbe_backward_sort";
  c.D = D, c.row_base = row_base, c.T = T, c.B = B;
  c.idx = indices, c.index_bits = index_bits, c.off = offsets, c.offset_bits = offset_bits;
  c.N = num_lookups, c.total_rows = total_rows, c.psw = per_sample_weights;
  c.max_seg = max_lookups_per_table, c.ws = workspace, c.ws_bytes = workspace_bytes;
  c.err = error_flag, c.stream = stream;
  if (const int rc = check_bwd_call(c, false)) return rc;
  if (c.N == 0) return DLRM_OK;
  BwdWs w{};
  if (const int rc = carve_checked(c, w)) return rc;
  SortedRuns s{};
  return run_sort(c, w, s);
}

extern "C" int dlrm_tbe_backward_defer(
    int32_t mode, float* weights, float* momentum, int64_t D, const int64_t* row_base,
    int32_t T, int32_t B, const void* indices, int32_t index_bits, const void* offsets,
    int32_t offset_bits, int64_t num_lookups, int64_t total_rows,
    const float* per_sample_weights, const float* grad_out, int64_t grad_batch_stride, float lr,
    float eps, int64_t max_lookups_per_table, void* workspace, size_t workspace_bytes,
    int32_t* error_flag, int32_t presorted, dlrm_launch_role* role, dlrm_stream_t stream) {
  BwdCall c{};
  c.name = "dlrm_tbe_backward_defer", c.W = weights, c.mom = momentum;
  c.D = D, c.row_base = row_base, c.T = T, c.B = B;
  c.idx = indices, c.index_bits = index_bits, c.off = offsets, c.offset_bits = offset_bits;
  c.N = num_lookups, c.total_rows = total_rows, c.psw = per_sample_weights;
  c.gout = grad_out, c.gbs = grad_batch_stride, c.lr = lr, c.eps = eps;
  c.max_seg = max_lookups_per_table, c.ws = workspace, c.ws_bytes = workspace_bytes;
  c.err = error_flag, c.presorted = presorted, c.stream = stream;
  return bwd_defer(c, mode, role);
}

extern "C" int dlrm_tbe_backward_defer_dev(
    int32_t mode, float* weights, float* momentum, int64_t D, const int64_t* row_base,
    int32_t T, int32_t B, const void* indices, int32_t index_bits, const void* offsets,
    int32_t offset_bits, int64_t num_lookups, int64_t total_rows,
    const float* per_sample_weights, const float* grad_out, int64_t grad_batch_stride,
    const float* lr_dev, float eps, int64_t max_lookups_per_table, void* workspace,
    size_t workspace_bytes, int32_t* error_flag, int32_t presorted, dlrm_launch_role* role,
    dlrm_stream_t stream) {
  DLRM_ARG(lr_dev, "dlrm_tbe_backward_defer_dev: null lr_dev");
  BwdCall c{};
  c.name = "dlrm_tbe_backward_defer_dev", c.W = weights, c.mom = momentum;
  c.D = D, c.row_base = row_base, c.T = T, c.B = B;
  c.idx = indices, c.index_bits = index_bits, c.off = offsets, c.offset_bits = offset_bits;
  c.N = num_lookups, c.total_rows = total_rows, c.psw = per_sample_weights;
  c.gout = grad_out, c.gbs = grad_batch_stride, c.lr_dev = lr_dev, c.eps = eps;
  c.max_seg = max_lookups_per_table, c.ws = workspace, c.ws_bytes = workspace_bytes;
  c.err = error_flag, c.presorted = presorted, c.stream = stream;
  return bwd_defer(c, mode, role);
}

extern "C" int32_t dlrm_role_blocks(const dlrm_launch_role* role) {
  const auto* r = reinterpret_cast<const LaunchRole*>(role);
  return r && r->magic == kRoleMagic ? r->blocks : 0;
}

extern "C" int dlrm_tbe_forward_presort(const float* weights, int64_t D, const int64_t* row_base,
                                        int32_t T, int32_t B, const void* indices,
                                        int32_t index_bits, const void* offsets,
                                        int32_t offset_bits, const float* per_sample_weights,
                                        float* out, int64_t out_batch_stride,
                                        int64_t num_lookups, int64_t total_rows,
                                        int64_t max_lookups_per_table, void* workspace,
                                        size_t workspace_bytes, int32_t* error_flag,
                                        const dlrm_mlp_chain* bottom, dlrm_stream_t stream) {
  const char* name = "dlrm_tbe_forward_presort";
  MlpChain mc{};
  int mlp_blocks = 0;
  if (bottom) {
    DLRM_ARG(mlp_chain_prepare(bottom, mc), "%s: unsupported bottom MLP chain", name);
    mlp_blocks = (int)mlp_chain_blocks(mc);
  }
  // (32-bit row keys, as in the backward)
  const bool sort = (uint64_t)total_rows < 0xFFFFFFFFull &&
                    presort_applies(max_lookups_per_table, num_lookups) && num_lookups > 0 &&
                    T * (int64_t)B < INT32_MAX;
  // no per-table sort (the backward sorts itself) but a bottom MLP to run: one launch of
  // the lookup and the MLP roles (D <= 512 keeps the gather within its 8 chunks per lane)
  const bool pair = !sort && bottom && out && num_lookups > 0 && T * (int64_t)B < INT32_MAX &&
                    D <= 512;
  if (!sort && !pair) {
    DLRM_REQUIRE(out, DLRM_ERR_UNSUPPORTED,
                 "%s: out = NULL needs the per-table sort (32-bit keys, bounded tables)", name);
    const int rc = dlrm_tbe_forward(weights, D, row_base, T, B, indices, index_bits, offsets,
                                    offset_bits, per_sample_weights, out, out_batch_stride,
                                    error_flag, stream);
    if (rc != DLRM_OK || !bottom) return rc;
    return dlrm_mlp_chain_forward(bottom, stream);
  }
  DLRM_ARG(weights && row_base && offsets && indices, "%s: null pointer", name);
  DLRM_ARG(T > 0 && B > 0 && D > 0 && total_rows > 0, "%s: bad sizes", name);
  DLRM_ARG(index_bits == 32 || index_bits == 64, "%s: index_bits must be 32|64", name);
  DLRM_ARG(offset_bits == 32 || offset_bits == 64, "%s: offset_bits must be 32|64", name);
  DLRM_ARG(out_batch_stride >= (int64_t)T * D, "%s: out_batch_stride < T*D", name);
  DLRM_ARG(workspace || !sort, "%s: null workspace", name);
  hipStream_t st = dlrm::as_stream(stream);
  BwdWs w{};
  if (sort) {
    w = carve_bwd_ws(workspace, num_lookups, D);
    DLRM_REQUIRE(workspace_bytes >= w.total, DLRM_ERR_WORKSPACE,
                 "%s: workspace %zu < required %zu", name, workspace_bytes, w.total);
  }
  const int nsort = sort ? T + 1 : 0;
  const bool vec4 = (D % 4 == 0) && ((reinterpret_cast<uintptr_t>(weights) & 15) == 0) &&
                    ((reinterpret_cast<uintptr_t>(out) & 15) == 0) && (out_batch_stride % 4 == 0);
  const LaneGeom g = lane_geom(vec4 ? D / 4 : D);
  DLRM_REQUIRE(g.maxv <= 8, DLRM_ERR_UNSUPPORTED, "%s: D=%lld too large", name, (long long)D);
  // out = NULL: the lookup is fused into its consumer (interaction gather)
  const int64_t gblocks = out ? lane_blocks((int64_t)T * B, g.lpb, kPreThreads / 64) : 0;
  const dim3 grid((unsigned)(nsort + mlp_blocks + gblocks)), block(kPreThreads);
  const uint32_t sentinel = (uint32_t)total_rows;
  for_csr_widths(index_bits, offset_bits, [&](auto i, auto o) {
    for_row_width(vec4, [&](auto vw) {
      for_lanes<1, 8>(g, [&](auto lpb, auto mv) {
        hipLaunchKernelGGL(
            (tbe_fwd_presort_kernel<decltype(lpb)::value, decltype(vw)::value, decltype(mv)::value,
                                    width_t<decltype(i)>, width_t<decltype(o)>>),
            grid, block, 0, st, weights, D, row_base, T, B, i.ptr(indices), o.ptr(offsets),
            per_sample_weights, out, out_batch_stride, error_flag, num_lookups, sentinel,
            w.keys_out, w.pos_out, w.bag_of, mc, mlp_blocks, nsort);
      });
    });
  });
  DLRM_LAUNCH_CHECK(name);
  return DLRM_OK;
}

extern "C" int dlrm_mlp_chain_supported(const dlrm_mlp_chain* chain) {
  MlpChain mc{};
  return mlp_chain_prepare(chain, mc);
}

extern "C" int dlrm_mlp_chain_forward(const dlrm_mlp_chain* chain, dlrm_stream_t stream) {
  const char* name = "dlrm_mlp_chain_forward";
  MlpChain mc{};
  DLRM_ARG(mlp_chain_prepare(chain, mc), "%s: unsupported chain", name);
  if (chain->rows == 0) return DLRM_OK;
  hipLaunchKernelGGL(mlp_chain_kernel, dim3((unsigned)mlp_chain_blocks(mc)),
                     dim3(kMlpWaves * 64), 0, dlrm::as_stream(stream), mc);
  DLRM_LAUNCH_CHECK(name);
  return DLRM_OK;
}
