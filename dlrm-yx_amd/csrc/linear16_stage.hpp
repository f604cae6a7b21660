// Pieces the 16-bit MFMA Linear kernels share (linear16.hip, linear16_bwd.hip): the operand
// types, the [rows][64 x 16-bit] LDS image and the staging of a tile whose reduction
// dimension is contiguous in memory.
#pragma once
#include "common.hpp"

namespace dlrm {
namespace l16 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kBK = 64;        // reduction elements per step
constexpr int kThreads = 256;  // 4 waves, 2 x 2

template <typename T>
struct Op16;
template <>
struct Op16<__bf16> {
  using vec = bf16x8;
  static __device__ __forceinline__ f32x4 mfma(vec a, vec b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};
template <>
struct Op16<_Float16> {
  using vec = f16x8;
  static __device__ __forceinline__ f32x4 mfma(vec a, vec b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};

// 16-byte chunk index of (row, chunk) in a [rows][8 chunks] LDS tile
__device__ __forceinline__ int lds_chunk(int row, int c) { return row * 8 + (c ^ ((row >> 1) & 7)); }

// One thread's share of a [ROWS][64] fp32 tile: chunk (tid & 7) of rows (tid >> 3) + 32 i.
template <int ROWS>
struct Stage {
  static constexpr int kIter = ROWS / 32;
  float v[kIter][8];

  // FULL: the whole k-step lies below K.  ALIGNED: 16-byte loads where the chunk does.
  template <bool ALIGNED, bool FULL>
  __device__ __forceinline__ void load(const float* __restrict__ P, int64_t ld, int64_t row0,
                                       int64_t rows, int64_t k0, int64_t K, int tid) {
    const int64_t k = k0 + (tid & 7) * 8;
#pragma unroll
    for (int i = 0; i < kIter; ++i) {
      int64_t r = row0 + (tid >> 3) + 32 * i;
      r = r < rows ? r : rows - 1;  // clamped rows are computed but never written
      const float* p = P + r * ld + k;
      if (FULL || k + 8 <= K) {
        if (ALIGNED) {
          const float4 a = *reinterpret_cast<const float4*>(p);
          const float4 b = *reinterpret_cast<const float4*>(p + 4);
          v[i][0] = a.x, v[i][1] = a.y, v[i][2] = a.z, v[i][3] = a.w;
          v[i][4] = b.x, v[i][5] = b.y, v[i][6] = b.z, v[i][7] = b.w;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[i][j] = p[j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i][j] = (k + j < K) ? p[j] : 0.0f;  // select, not multiply
      }
    }
  }

  template <typename T>
  __device__ __forceinline__ void store(typename Op16<T>::vec* lds, int tid) const {
#pragma unroll
    for (int i = 0; i < kIter; ++i) {
      typename Op16<T>::vec h;
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = static_cast<T>(v[i][j]);  // RNE
      lds[lds_chunk((tid >> 3) + 32 * i, tid & 7)] = h;
    }
  }
};

struct Tile {
  int bm, bn;
};
constexpr Tile kTiles[] = {{128, 128}, {128, 64}, {64, 64}, {32, 64}};  // largest first
constexpr int kNumTiles = sizeof(kTiles) / sizeof(kTiles[0]);

inline bool known_tile(Tile t) {
  bool known = false;
  for (const Tile& c : kTiles) known = known || (c.bm == t.bm && c.bn == t.bn);
  return known;
}

inline int device_cus() {
  static thread_local int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
      cus = n;
    else
      return 256;
  }
  return cus;
}

}  // namespace l16
}  // namespace dlrm
