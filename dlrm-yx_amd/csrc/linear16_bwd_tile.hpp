// The per-tile body of the 16-bit Linear backward, shared by its per-problem kernel
// (linear16_bwd.hip) and the grouped launch (linear16_group.hip), and the planner both use:
// the staging of an operand whose REDUCTION index is the row index in memory (StageT), the
// two-buffer LDS image and MFMA loop (bwd_tile_acc) and the epilogue (bwd_tile_store).
#pragma once
#include "linear16_stage.hpp"

namespace dlrm {
namespace l16 {

constexpr int kMaxSplits = 32;

// One thread's share of a [64 reduction rows][OUT columns] fp32 tile whose rows are
// contiguous along the columns: RG reduction rows x 4 columns.
template <int OUT>
struct StageT {
  static constexpr int kCG = OUT / 4;                  // groups of 4 columns
  static constexpr int kRG = kBK / (kThreads / kCG);   // reduction rows per thread
  static_assert(OUT == 32 || OUT == 64 || OUT == 128, "tile");
  float v[kRG][4];

  template <bool ALIGNED>
  __device__ __forceinline__ void load(const float* __restrict__ P, int64_t ld, int64_t r0,
                                       int64_t R, int64_t c0, int64_t C, int tid) {
    const int64_t c = c0 + (tid % kCG) * 4;
    const int64_t rb = r0 + (tid / kCG) * kRG;
#pragma unroll
    for (int i = 0; i < kRG; ++i) {
      const int64_t r = rb + i;
      if (r < R && c + 4 <= C) {
        const float* p = P + r * ld + c;
        if (ALIGNED) {
          const float4 a = *reinterpret_cast<const float4*>(p);
          v[i][0] = a.x, v[i][1] = a.y, v[i][2] = a.z, v[i][3] = a.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[i][j] = p[j];
        }
      } else if (r < R) {
        const float* p = P + r * ld + c;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = (c + j < C) ? p[j] : 0.0f;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = 0.0f;  // a reduction tail: zero, nothing read
      }
    }
  }

  template <typename T>
  __device__ __forceinline__ void store(typename Op16<T>::vec* lds, int tid) const {
    typedef T packed __attribute__((ext_vector_type(kRG)));
    T* base = reinterpret_cast<T*>(lds);
    const int e = (tid / kCG) * kRG;  // first reduction element of this thread
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      packed h;
#pragma unroll
      for (int i = 0; i < kRG; ++i) h[i] = static_cast<T>(v[i][j]);  // RNE
      const int row = (tid % kCG) * 4 + j;
      *reinterpret_cast<packed*>(base + lds_chunk(row, e >> 3) * 8 + (e & 7)) = h;
    }
  }
};

// The same share of a tile that is already 16-bit in memory ([64 reduction rows][OUT columns],
// rows contiguous along the columns): RG reduction rows x 8 columns, one 16-byte chunk per
// row, no conversion.  The registers are transposed as they are stored: column j of the RG
// chunks is one packed run of RG reduction elements in row 8 cg + j of the same image.
template <typename T, int OUT>
struct StageT16 {
  using vec = typename Op16<T>::vec;
  static constexpr int kCG = OUT / 8;                  // groups of 8 columns: 4 / 8 / 16
  static constexpr int kRG = kBK / (kThreads / kCG);   // reduction rows per thread: 1 / 2 / 4
  static_assert(OUT == 32 || OUT == 64 || OUT == 128, "tile");
  vec v[kRG];

  __device__ __forceinline__ void load(const T* __restrict__ P, int64_t ld, int64_t r0,
                                       int64_t R, int64_t c0, int64_t C, int tid) {
    const int64_t c = c0 + (tid % kCG) * 8;
    const int64_t rb = r0 + (tid / kCG) * kRG;
#pragma unroll
    for (int i = 0; i < kRG; ++i) {
      const int64_t r = rb + i;
      if (r < R && c + 8 <= C) {
        v[i] = *reinterpret_cast<const vec*>(P + r * ld + c);  // aligned: P is, ld % 8 == 0
      } else if (r < R && c < C) {
        // the one chunk that crosses the extent (wgrad's [inp | 1] ends in it): by element
        const T* p = P + r * ld + c;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i][j] = (c + j < C) ? p[j] : static_cast<T>(0.0f);
      } else {
        v[i] = vec{};  // a reduction tail or a chunk past the extent: zero, nothing read
      }
    }
  }

  __device__ __forceinline__ void store(vec* lds, int tid) const {
    typedef T packed __attribute__((ext_vector_type(kRG > 1 ? kRG : 2)));
    T* base = reinterpret_cast<T*>(lds);
    const int e = (tid / kCG) * kRG;  // first reduction element of this thread
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int row = (tid % kCG) * 8 + j;
      T* dst = base + lds_chunk(row, e >> 3) * 8 + (e & 7);
      if constexpr (kRG == 1) {
        *dst = v[0][j];
      } else {
        packed h;
#pragma unroll
        for (int i = 0; i < kRG; ++i) h[i] = v[i][j];
        *reinterpret_cast<packed*>(dst) = h;
      }
    }
  }
};

// One operand's stager behind one signature: TRANS = its reduction index is its memory row;
// H16 = it is 16-bit in memory.  (o0, O): the tile's origin and the extent along the output
// index; (r0, R): along the reduction.
template <typename T, int ROWS, bool TRANS, bool H16, bool ALIGNED>
struct BwdStage;
template <typename T, int ROWS, bool ALIGNED>
struct BwdStage<T, ROWS, false, false, ALIGNED> {
  Stage<ROWS> s;
  __device__ __forceinline__ void load(const void* P, int64_t ld, int64_t o0, int64_t O,
                                       int64_t r0, int64_t R, int tid) {
    const float* p = static_cast<const float*>(P);
    if (r0 + kBK <= R)
      s.template load<ALIGNED, true>(p, ld, o0, O, r0, R, tid);
    else
      s.template load<ALIGNED, false>(p, ld, o0, O, r0, R, tid);
  }
  __device__ __forceinline__ void store(typename Op16<T>::vec* lds, int tid) const {
    s.template store<T>(lds, tid);
  }
};
template <typename T, int ROWS, bool ALIGNED>
struct BwdStage<T, ROWS, false, true, ALIGNED> {  // R % 8 == 0: whole chunks
  Stage16<T, ROWS> s;
  __device__ __forceinline__ void load(const void* P, int64_t ld, int64_t o0, int64_t O,
                                       int64_t r0, int64_t R, int tid) {
    s.template load<false>(static_cast<const T*>(P), ld, o0, O, r0, R, tid);
  }
  __device__ __forceinline__ void store(typename Op16<T>::vec* lds, int tid) const {
    s.store(lds, tid);
  }
};
template <typename T, int ROWS, bool ALIGNED>
struct BwdStage<T, ROWS, true, false, ALIGNED> {
  StageT<ROWS> s;
  __device__ __forceinline__ void load(const void* P, int64_t ld, int64_t o0, int64_t O,
                                       int64_t r0, int64_t R, int tid) {
    s.template load<ALIGNED>(static_cast<const float*>(P), ld, r0, R, o0, O, tid);
  }
  __device__ __forceinline__ void store(typename Op16<T>::vec* lds, int tid) const {
    s.template store<T>(lds, tid);
  }
};
template <typename T, int ROWS, bool ALIGNED>
struct BwdStage<T, ROWS, true, true, ALIGNED> {
  StageT16<T, ROWS> s;
  __device__ __forceinline__ void load(const void* P, int64_t ld, int64_t o0, int64_t O,
                                       int64_t r0, int64_t R, int tid) {
    s.load(static_cast<const T*>(P), ld, r0, R, o0, O, tid);
  }
  __device__ __forceinline__ void store(typename Op16<T>::vec* lds, int tid) const {
    s.store(lds, tid);
  }
};

enum Epi { kEpiDgrad = 0, kEpiStore = 1, kEpiSgd = 2, kEpiPartial = 3 };

// A, B, mask and Out are fp32 except where a kernel is built for a 16-bit one (A16 / B16 /
// O16 of linear16_bwd_kernel; the mask is of Out's format); the leading dimensions count
// elements of the operand's own format.
struct BwdArgs {
  int64_t I, J, R;           // Out [I][J], reduction depth R
  const void* A;             // TRANS_A ? [R][I] : [I][R]
  int64_t lda;
  const void* B;             // [R][J]
  int64_t ldb;
  const void* mask;          // kEpiDgrad: [I][J] or NULL
  int64_t ldmask;
  void* Out;                 // kEpiPartial: the workspace, [split][I][J]
  int64_t ldo;
  int epi;
  float lr;
  const float* lr_dev;       // ABI v14: NULL, or the device fp32 that replaces lr (kEpiSgd)
  int tiles_j, tiles;
  int64_t steps_per_split;   // reduction steps of 64 per split
};

// The accumulators of one BM x BN tile over the reduction steps of `split`: `orig` is the
// workgroup's index among the problem's `p.tiles` tiles before the XCD remap; i0 / j0 return
// the tile's origin.  lds: 2 x (BM + BN) x 8 chunks of 16 bytes.  Ends behind a barrier (the
// LDS image is free again).  A16 / B16: that operand is 16-bit in memory.
template <typename T, int BM, int BN, bool TRANS_A, bool ALIGNED, bool A16 = false,
          bool B16 = false>
__device__ __forceinline__ void bwd_tile_acc(const BwdArgs& p, typename Op16<T>::vec* lds,
                                             int orig, int split,
                                             f32x4 (&acc)[BM / 32][BN / 32], int64_t& i0,
                                             int64_t& j0) {
  using vec = typename Op16<T>::vec;
  constexpr int WTM = BM / 2, WTN = BN / 2;  // a wave's part of the tile
  constexpr int FM = WTM / 16, FN = WTN / 16;
  constexpr int kBuf = (BM + BN) * 8;
  static_assert(BM % 32 == 0 && BN % 32 == 0, "tile");

  // consecutive tiles (j fastest: they share A) go to one XCD; bijective for any count
  const int q = p.tiles / 8, rem = p.tiles % 8, xcd = orig % 8;
  const int tile = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + orig / 8;
  i0 = int64_t(tile / p.tiles_j) * BM;
  j0 = int64_t(tile % p.tiles_j) * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * WTM, wn = (wave & 1) * WTN;
  const int fr = lane & 15, fc = lane >> 4;

#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  BwdStage<T, BM, TRANS_A, A16, ALIGNED> sa;
  BwdStage<T, BN, true, B16, ALIGNED> sb;
  const int64_t nk_all = (p.R + kBK - 1) / kBK;
  const int64_t kt0 = int64_t(split) * p.steps_per_split;
  const int64_t kt1 = kt0 + p.steps_per_split < nk_all ? kt0 + p.steps_per_split : nk_all;
  const int64_t ti0 = i0, tj0 = j0;
  auto fetch = [&](int64_t kt) {
    const int64_t r0 = kt * kBK;
    sa.load(p.A, p.lda, ti0, p.I, r0, p.R, tid);
    sb.load(p.B, p.ldb, tj0, p.J, r0, p.R, tid);
  };
  auto commit = [&](int buf) {
    sa.store(lds + buf * kBuf, tid);
    sb.store(lds + buf * kBuf + BM * 8, tid);
  };

  if (kt0 < kt1) {
    fetch(kt0);
    commit(0);
  }
  __syncthreads();
  for (int64_t kt = kt0; kt < kt1; ++kt) {
    const int buf = int((kt - kt0) & 1);
    if (kt + 1 < kt1) fetch(kt + 1);
    const vec* A = lds + buf * kBuf;
    const vec* B = A + BM * 8;
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
    if (kt + 1 < kt1) commit(buf ^ 1);
    __syncthreads();
  }
}

// The epilogue `epi` of that tile into out (leading dimension ldo).
// C/D map of 16x16: col = lane & 15, row = (lane >> 4) * 4 + reg
template <int BM, int BN>
__device__ __forceinline__ void bwd_tile_store(const BwdArgs& p, int epi, float lr,
                                               const f32x4 (&acc)[BM / 32][BN / 32], int64_t i0,
                                               int64_t j0, float* out, int64_t ldo) {
  constexpr int WTM = BM / 2, WTN = BN / 2;
  constexpr int FM = WTM / 16, FN = WTN / 16;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * WTM, wn = (wave & 1) * WTN;
  const int fr = lane & 15, fc = lane >> 4;
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int64_t cj = j0 + wn + j * 16 + fr;
    if (cj >= p.J) continue;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t ci = i0 + wm + i * 16 + fc * 4 + r;
        if (ci >= p.I) continue;
        float v = acc[i][j][r];
        float* o = out + ci * ldo + cj;
        if (epi == kEpiDgrad) {
          if (p.mask)  // selects, NaN -> 0
            v = static_cast<const float*>(p.mask)[ci * p.ldmask + cj] > 0.f ? v : 0.f;
        } else if (epi == kEpiSgd) {
          // ONE rounding, unlike DLRM_EPI_SGD: the __fsub_rn(*o, __fmul_rn(lr, v)) that stood
          // here always compiled to this fma (common.hpp, dlrm_scale), and the bf16 step
          // traces pin its bits.  Two roundings are dlrm_sgd_step(*o, dlrm_scale(lr, v)).
          v = fmaf(-lr, v, *o);
        }
        *o = v;
      }
    }
  }
}

// dgrad's epilogue to a 16-bit dX: mask > 0 ? r16(acc) : 0, the mask 16-bit too and tested as
// it is stored.  The tile passes through LDS once, as linear16_packed.hip's 16-bit Y does
// (bwd_tile_acc ended behind a barrier: no operand tile is read any more) - each lane writes
// its elements of a [BM][BN + 8] image, then the workgroup stores whole rows as 16-byte
// chunks.  J % 8 == 0, so no chunk crosses the extent.
template <typename T, int BM, int BN>
__device__ __forceinline__ void bwd_tile_store16(const BwdArgs& p, typename Op16<T>::vec* lds,
                                                 const f32x4 (&acc)[BM / 32][BN / 32],
                                                 int64_t i0, int64_t j0) {
  using vec = typename Op16<T>::vec;
  constexpr int WTM = BM / 2, WTN = BN / 2;
  constexpr int FM = WTM / 16, FN = WTN / 16;
  constexpr int YP = BN + 8;  // row pitch (elements) of the image
  static_assert(BM * YP * 2 <= 2 * (BM + BN) * 8 * 16, "the output image fits the operand LDS");
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * WTM, wn = (wave & 1) * WTN;
  const int fr = lane & 15, fc = lane >> 4;
  const T* mask = static_cast<const T*>(p.mask);
  T* img = reinterpret_cast<T*>(lds);
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int jl = wn + j * 16 + fr;
    const int64_t cj = j0 + jl;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int il = wm + i * 16 + fc * 4 + r;
        const int64_t ci = i0 + il;
        float v = acc[i][j][r];
        if (mask && ci < p.I && cj < p.J)  // past the extents: not read, and not stored below
          v = static_cast<float>(mask[ci * p.ldmask + cj]) > 0.f ? v : 0.f;
        img[il * YP + jl] = static_cast<T>(v);  // RNE
      }
    }
  }
  __syncthreads();
  T* out = static_cast<T*>(p.Out);
  constexpr int CPR = BN / 8;  // 16-byte chunks per row of the tile
  for (int e = tid; e < BM * CPR; e += kThreads) {
    const int il = e / CPR, c = e % CPR;
    const int64_t ci = i0 + il, cj = j0 + c * 8;
    if (ci >= p.I || cj >= p.J) continue;
    *reinterpret_cast<vec*>(out + ci * p.ldo + cj) =
        *reinterpret_cast<const vec*>(img + il * YP + c * 8);
  }
}

inline int64_t tiles_of(Tile t, int64_t I, int64_t J) {
  return ceil_div(I, t.bm) * ceil_div(J, t.bn);
}

// dgrad: the forward's rule on the [M][K] output - the largest tile that still gives every CU
// two workgroups, else the smallest.
inline Tile plan_dgrad(int64_t I, int64_t J, int cus) {
  for (const Tile& t : kTiles)
    if (tiles_of(t, I, J) >= 2 * int64_t(cus)) return t;
  return kTiles[kNumTiles - 1];
}

struct WgradPlan {
  Tile tile;
  int splits;
  int64_t steps;  // reduction steps per split
};

// wgrad: 128 x 128 and no split where that tile alone gives every CU two workgroups.
// Otherwise the tile by the number of 64 x 64 tiles of the [N][K] output (more than cus / 2:
// 128 x 64; at least cus / 8: 64 x 64; else 32 x 64) and the batch split into runs of four
// 64-row steps - more splits while the launch has fewer than cus / 2 workgroups, at most
// kMaxSplits, at least one step each.  Measured at the C3 layers, B = 2048
// (profiles/train16_wgrad_plan_sweep.json): 8 splits win at every layer, 128 x 64 at
// 1024 x 1024 and 512 x 1024, 64 x 64 at 1024 x 479 and 256 x 512, 32 x 64 at 512 x 13
// and 128 x 256.
inline WgradPlan plan_wgrad(int64_t R, int64_t I, int64_t J, int cus, int64_t forced_tile,
                            int64_t forced_split) {
  const int64_t nk = ceil_div(R, kBK);
  WgradPlan w{{int(forced_tile / 1000), int(forced_tile % 1000)}, 0, 0};
  bool whole = false;
  if (forced_tile == 0) {
    const int64_t t64 = tiles_of(kTiles[2], I, J);
    whole = tiles_of(kTiles[0], I, J) >= 2 * int64_t(cus);
    w.tile = whole ? kTiles[0] : t64 > cus / 2 ? kTiles[1] : t64 >= cus / 8 ? kTiles[2] : kTiles[3];
  }
  const int64_t tiles = tiles_of(w.tile, I, J);
  int64_t s = forced_split;
  if (s == 0 && !whole) {
    const int64_t fill = ceil_div(int64_t(cus) / 2, tiles > 0 ? tiles : 1);
    s = ceil_div(nk, 4) > fill ? ceil_div(nk, 4) : fill;
  }
  s = s < kMaxSplits ? s : kMaxSplits;
  s = s < nk ? s : nk;
  s = s > 1 ? s : 1;
  w.steps = nk > 0 ? ceil_div(nk, s) : 0;
  w.splits = nk > 0 ? int(ceil_div(nk, w.steps)) : 1;  // every split has at least one step
  return w;
}

// the plan of a wgrad call under the calling thread's tuning; false: a forced value is bad
inline bool wgrad_plan_checked(int64_t M, int64_t N, int64_t K, WgradPlan* w) {
  const int64_t ft = tuning(DLRM_TUNE_LINEAR16_WGRAD_TILE);
  const int64_t fs = tuning(DLRM_TUNE_LINEAR16_WGRAD_SPLIT);
  if (ft != 0 && !known_tile(Tile{int(ft / 1000), int(ft % 1000)})) return false;
  *w = plan_wgrad(M, N, K, device_cus(), ft, fs);
  return true;
}

inline bool aligned16(const void* a, int64_t lda, const void* b, int64_t ldb) {
  return reinterpret_cast<uintptr_t>(a) % 16 == 0 && reinterpret_cast<uintptr_t>(b) % 16 == 0 &&
         lda % 4 == 0 && ldb % 4 == 0;
}

}  // namespace l16
}  // namespace dlrm
