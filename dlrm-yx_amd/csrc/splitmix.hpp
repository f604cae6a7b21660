// splitmix64 and the counter-based stream of the fp16 tables' stochastic rounding (ABI v16).
// Stateless: a draw is a hash of (seed, step, global row, column), so it does not depend on
// the sort path, the block length, the launch shape or the row's vector width.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DLRM_HD __host__ __device__ __forceinline__
#else
#define DLRM_HD inline
#endif

DLRM_HD uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// dlrm_sr_state (include/dlrm_hip.h): uint64 seed, uint64 step.
//   key          = splitmix64(splitmix64(seed) ^ step)
//   word(row, d) = splitmix64(key ^ (row * ceil(D / 4) + d / 4))     row: global row
//   r16(row, d)  = (word(row, d) >> (16 * (d % 4))) & 0xffff
DLRM_HD uint64_t sr_key(uint64_t seed, uint64_t step) {
  return splitmix64(splitmix64(seed) ^ step);
}
DLRM_HD uint64_t sr_word(uint64_t key, uint64_t row, uint64_t chunks4, uint64_t chunk4) {
  return splitmix64(key ^ (row * chunks4 + chunk4));
}

// fp32 -> fp16 bits, rounded stochastically with the 16-bit draw r: with ulp the fp16
// spacing at |v| (2^-24 through the subnormal range; the grid runs on past 65504 to 65536,
// stored as Inf), t = floor(|v| / ulp) * ulp and frac = (|v| - t) / ulp, the magnitude is
// t + ulp if r < frac * 65536 and t otherwise; v's sign is kept (a tiny negative may store
// -0).  A representable v has frac = 0 and is returned unchanged for every draw; NaN and
// +-Inf convert as the nearest-even conversion does.
DLRM_HD uint32_t sr16_bits(float v, uint32_t r) {
  // Branch-free (selects): the store is inlined at every run end of the block pass.
  const uint32_t b = __builtin_bit_cast(uint32_t, v);
  const uint32_t a = b & 0x7fffffffu;
  const uint32_t sign = (b >> 16) & 0x8000u;
  // |v| >= 65536, +-Inf, NaN: the nearest-even conversion (Inf, or the NaN), sign included
  const uint32_t big = (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)v);
  // normal range: frac = m13 / 8192 (the fp32's low 13 mantissa bits), and r < frac * 65536
  // exactly when (r >> 3) < m13 - the carry out of m13 + (0x1fff - (r >> 3)); a value
  // rounded up to 65536 comes out as 0x7c00
  const uint32_t nrm = ((a + (0x1fffu - (r >> 3))) >> 13) - (112u << 10);
  // subnormal range (and 0), ulp 2^-24: f = ceil(|v| * 2^40) < 2^26 is |v| / ulp in 16.16
  // fixed point with the low half rounded up (exact product; r is an integer, so
  // r < frac * 65536 exactly when r < the rounded-up low half): again the carry of an add.
  // 1024 is the smallest normal
  const bool tiny = a < 0x38800000u;
  const float s = __builtin_bit_cast(float, tiny ? a : 0u);
  const uint32_t f = (uint32_t)__builtin_ceilf(s * 1099511627776.f);
  const uint32_t sub = (f + (0xffffu - r)) >> 16;
  const uint32_t fin = sign | (tiny ? sub : nrm);
  return a >= 0x47800000u ? big : fin;
}

#if defined(__HIPCC__)
// The state's key, loaded once at kernel entry: no kernel that reads the state writes it
// (dlrm_sr_tick is a launch of its own), so the two loads go through the constant address
// space like dlrm_resolve_lr's - scalar loads, and the two hashes run on the scalar unit.
__device__ __forceinline__ uint64_t sr_load_key(const uint64_t* sr_state) {
  typedef const uint64_t __attribute__((address_space(4))) * const_u64;
  const const_u64 s = (const_u64)sr_state;
  return sr_key(s[0], s[1]);
}
#endif
