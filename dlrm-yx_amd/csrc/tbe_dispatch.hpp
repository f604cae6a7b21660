// Host-only dispatch shared by the embedding translation units (tbe.hip, tbe_rows.hip,
// tbe_bwd.hip): the three run-time choices that pick a kernel instantiation - the lane
// geometry of a row, the row's vector width and the index/offset widths - each written once.
// A choice reaches the kernel's template arguments as a tag type handed to a generic lambda.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace {

template <int V>
using int_tag = std::integral_constant<int, V>;

// ------------------------------------------------------------ lane geometry --
// A row of nchunks chunks (float4s, or floats where a float4 sweep does not apply) is swept
// by a group of lpb lanes: the power of two >= nchunks, at least min_lpb (4 for the
// packed-row lookup, whose smallest instantiation it is) and at most 64, the wave.  Above
// 64 chunks every lane owns maxv of them; the kernels hold at most 8 (the packed-row ones
// 2), which each caller checks with its own message.
struct LaneGeom {
  int lpb;
  int64_t maxv;
};

inline LaneGeom lane_geom(int64_t nchunks, int min_lpb = 1) {
  int lpb = min_lpb;
  while (lpb < nchunks && lpb < 64) lpb <<= 1;
  return {lpb, dlrm::ceil_div(nchunks, lpb)};
}

// Workgroups of `waves` wave64s for n rows (bags, sorted blocks), 64 / lpb of them per wave;
// the kernels grid-stride past 8192.
inline int64_t lane_blocks(int64_t n, int lpb, int waves) {
  const int64_t blocks = dlrm::ceil_div(dlrm::ceil_div(n, 64 / lpb), waves);
  return blocks > 8192 ? 8192 : blocks < 1 ? 1 : blocks;
}

// The lane ladder: f(int_tag<LPB>, int_tag<MAXV>) for the geometry's rung.  The rungs are
// LPB = MIN_LPB .. 32 with one chunk per lane, and LPB = 64 with 1 | 2 | 4 | 8 chunks per
// lane (maxv rounded up to the next of them), none above MAX_MV: exactly the instantiations
// a caller's kernels are compiled for.
template <int MIN_LPB, int MAX_MV, class F>
void for_lanes(const LaneGeom& g, F&& f) {
  static_assert(MAX_MV == 2 || MAX_MV == 8, "the ladders end at 2 or 8 chunks per lane");
  if constexpr (MIN_LPB < 64) {
    if (g.lpb == MIN_LPB)
      f(int_tag<MIN_LPB>{}, int_tag<1>{});
    else
      for_lanes<MIN_LPB * 2, MAX_MV>(g, f);
  } else if (g.maxv == 1) {
    f(int_tag<64>{}, int_tag<1>{});
  } else if constexpr (MAX_MV == 2) {
    f(int_tag<64>{}, int_tag<2>{});
  } else if (g.maxv == 2) {
    f(int_tag<64>{}, int_tag<2>{});
  } else if (g.maxv <= 4) {
    f(int_tag<64>{}, int_tag<4>{});
  } else {
    f(int_tag<64>{}, int_tag<8>{});
  }
}

// f(int_tag<4>) for rows swept as float4s, f(int_tag<1>) for scalar rows.  The predicate
// stays with each caller: its alignment conditions differ (fp16 rows, optimizer state, a
// lookup without an output).
template <class F>
void for_row_width(bool vec4, F&& f) {
  if (vec4)
    f(int_tag<4>{});
  else
    f(int_tag<1>{});
}

// ------------------------------------------------------ index / offset widths --
template <class T>
struct width_tag {
  using type = T;
  static const T* ptr(const void* p) { return static_cast<const T*>(p); }
};
template <class Tag>
using width_t = typename Tag::type;

// f(width_tag<IdxT>, width_tag<OffT>) for the CSR's (int32 | int64) x (int32 | int64); the
// caller has checked that both widths are 32 or 64.  Returns what f returns.
template <class F>
auto for_csr_widths(int index_bits, int offset_bits, F&& f) {
  if (index_bits == 32 && offset_bits == 32)
    return f(width_tag<int32_t>{}, width_tag<int32_t>{});
  if (index_bits == 32) return f(width_tag<int32_t>{}, width_tag<int64_t>{});
  if (offset_bits == 32) return f(width_tag<int64_t>{}, width_tag<int32_t>{});
  return f(width_tag<int64_t>{}, width_tag<int64_t>{});
}

}  // namespace
