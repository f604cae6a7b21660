// The multi-hot lookup fused into the dot interaction (dlrm_interact_dot_forward_pool, ABI v20):
// apply_emb with any bag length (dlrm_s_pytorch.py:526-587, the reference's default
// --num-indices-per-lookup 10) followed by interact_features (:627-659), in one launch that
// reads the embedding rows straight from the table buffer and never needs the pooled
// [B, T, D] buffer (it is written only when the caller asks for it: the training step keeps
// it for dlrm_interact_dot_backward).
//
// Work split: one wave per sample, four waves per workgroup stepping through the batch.  With
// C4 = D/4 lanes per row and RPI = 64/C4 rows per wave instruction, a lane owns columns
// [4c, 4c + 4) of the features q * RPI + sub, q < NI = 32 / RPI, and keeps their pooled sums
// in NI float4 accumulators (D = 128: 64 VGPRs).  Lane f (1 <= f < F) also owns bag f - 1 of
// the sample: it reads the bag's two offsets once, and at step l the bag's l-th index; the row
// id travels by __shfl to the lanes that own the row.  The wave runs max-bag-length steps
// (a wave reduction); in a step every lane issues its NI row loads, all independent, before
// the first accumulate, and the next step's index load is issued before them.  Lanes without
// a row in a step (bag exhausted, feature >= F, index out of range, inactive wave) read valid
// bytes of x and accumulate nothing, so no load sits in a divergent branch.
//
// Arithmetic: the pooled value is bit for bit the lookups' (tbe_common.hpp tbe_fwd_body,
// tbe_rows.hip tbe_rows_fwd_kernel with no per-sample weights): accumulation from 0 in lookup
// order, acc + row for fp32 and (widened exactly) fp16 rows, fmaf(scale, q, acc + bias) for
// Q8 / Q4 rows.  The Gram product is interact_dot_fwd_v4's: the pooled rows go to the wave's
// LDS image (pitch D + 4), Z = T T^T on v_mfma_f32_32x32x2_f32 with the same two accumulator
// chains and k order, the triangle and x staged in LDS in output order and written as rows.
#include <algorithm>

#include "common.hpp"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ int pair_index(int i, int j, bool self) {
  return self ? i * (i + 1) / 2 + j : i * (i - 1) / 2 + j;
}

__device__ __forceinline__ float half_bits_to_float(uint32_t h) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
}

template <int FMT, int D>
constexpr int64_t pool_row_bytes() {
  return FMT == DLRM_ROWS_F32 ? 4 * D : FMT == DLRM_ROWS_F16 ? 2 * D
         : FMT == DLRM_ROWS_Q8 ? D + 8 : D / 2 + 4;
}

// What a lane holds of one row between its load and its accumulate: columns [4c, 4c + 4) as
// loaded (fp32 values, four halves, four or two bytes of levels) and, for Q8 / Q4, the row's
// scale and bias as loaded.
template <int FMT>
struct RowBits {
  float4 v;  // F32
  uint2 u;   // F16: four halves; Q8 / Q4: u.x = the levels
  uint2 sb;  // Q8: fp32 scale, bias bits; Q4: sb.x = fp16 scale | bias << 16
};

// `row`: the table row, or x's row for a lane without one (every read below stays inside the
// first 64 bytes + 4 D bytes of it; x's row holds 4 D >= 64 bytes).
template <int FMT, int D>
__device__ __forceinline__ void load_row(RowBits<FMT>& r, const uint8_t* row, int c) {
  if constexpr (FMT == DLRM_ROWS_F32) {
    r.v = *reinterpret_cast<const float4*>(row + 16 * c);
  } else if constexpr (FMT == DLRM_ROWS_F16) {
    r.u = *reinterpret_cast<const uint2*>(row + 8 * c);
  } else if constexpr (FMT == DLRM_ROWS_Q8) {
    r.u.x = *reinterpret_cast<const uint32_t*>(row + 4 * c);
    r.sb = *reinterpret_cast<const uint2*>(row + D);
  } else {
    r.u.x = *reinterpret_cast<const uint16_t*>(row + 2 * c);
    r.sb.x = *reinterpret_cast<const uint32_t*>(row + D / 2);
  }
}

// acc <- acc (+) row, the lookup kernels' arithmetic for a weightless bag.
template <int FMT>
__device__ __forceinline__ void pool_row(float4& acc, const RowBits<FMT>& r) {
  if constexpr (FMT == DLRM_ROWS_F32) {
    acc.x += r.v.x, acc.y += r.v.y, acc.z += r.v.z, acc.w += r.v.w;
  } else if constexpr (FMT == DLRM_ROWS_F16) {
    acc.x += half_bits_to_float(r.u.x & 0xffff);
    acc.y += half_bits_to_float(r.u.x >> 16);
    acc.z += half_bits_to_float(r.u.y & 0xffff);
    acc.w += half_bits_to_float(r.u.y >> 16);
  } else {
    float scale, bias;
    float4 q;
    const uint32_t u = r.u.x;
    if constexpr (FMT == DLRM_ROWS_Q8) {
      scale = __builtin_bit_cast(float, r.sb.x), bias = __builtin_bit_cast(float, r.sb.y);
      q = make_float4((float)(u & 0xff), (float)((u >> 8) & 0xff), (float)((u >> 16) & 0xff),
                      (float)(u >> 24));
    } else {
      scale = half_bits_to_float(r.sb.x & 0xffff), bias = half_bits_to_float(r.sb.x >> 16);
      q = make_float4((float)(u & 0xf), (float)((u >> 4) & 0xf), (float)((u >> 8) & 0xf),
                      (float)((u >> 12) & 0xf));
    }
    acc.x = fmaf(scale, q.x, acc.x + bias);
    acc.y = fmaf(scale, q.y, acc.y + bias);
    acc.z = fmaf(scale, q.z, acc.z + bias);
    acc.w = fmaf(scale, q.w, acc.w + bias);
  }
}

struct PoolArgs {
  const float* x;           // [B][x_bs] fp32, feature 0
  int64_t x_bs;
  const uint8_t* W;         // [rows][pool_row_bytes<FMT, D>()]
  const int64_t* row_base;  // [F] device: table starts, row_base[F-1] = total rows
  const int32_t* idx;       // table-batched CSR: bag (t, b) = t * B + b
  const int32_t* off;       // [(F-1) * B + 1]
  float* out;               // [B][ld_out]
  int64_t ld_out;
  float* pooled;            // [B][pooled_bs]: feature f at (f - 1) * D; may be null
  int64_t pooled_bs;
  int32_t* err;             // DLRM_TBE_ERR_INDEX on an index outside its table (may be null)
};

template <int D, int FMT>
__global__ __launch_bounds__(256) void interact_pool_fwd(int B, int F, int self, int width,
                                                         int vec_out, PoolArgs a) {
  constexpr int DP = D + 4, C4 = D / 4, RPI = 64 / C4, KH = D / 2, NI = 32 / RPI;
  constexpr int OUTP = D + 32 * 33 / 2 + 4;  // x + <= 528 pairs, rounded
  constexpr int64_t RB = pool_row_bytes<FMT, D>();
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int h = lane >> 5, l32 = lane & 31;
  float* Tl = lds + wave * (32 * DP + OUTP);
  float* Ol = Tl + 32 * DP;
  const int sub = lane / C4, c = lane - sub * C4;
  const bool rowok = l32 < F;
  const bool bagl = lane >= 1 && lane < F;  // this lane owns bag lane - 1 of the sample
  int64_t rb_lo = 0, nrows = 0;             // its table's bounds (once per kernel)
  if (bagl) {
    rb_lo = a.row_base[lane - 1];
    nrows = a.row_base[lane] - rb_lo;
  }
  for (int64_t b0 = (int64_t)blockIdx.x * 4; b0 < B; b0 += (int64_t)gridDim.x * 4) {
    const int64_t b = b0 + wave;
    const bool active = b < B;
    const int64_t bl = active ? b : 0;
    const uint8_t* xrow = reinterpret_cast<const uint8_t*>(a.x + bl * a.x_bs);
    const float4 xv = *reinterpret_cast<const float4*>(xrow + 16 * c);
    // the bag: [start, start + len) of idx; an inactive wave and a lane without a bag hold
    // an empty one (their offset loads read entry 0)
    const int32_t* op = a.off + (bagl && active ? (int64_t)(lane - 1) * B + b : 0);
    const int64_t start = op[0];
    int len = (int)(op[1] - start);
    if (!(bagl && active) || len < 0) len = 0;
    int steps = len;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) steps = max(steps, __shfl_xor(steps, o, 64));
    // an exhausted bag reads off[0]: a valid int32 even where idx holds no entry at all
    int32_t cur = *(len > 0 ? a.idx + start : a.off);
    float4 acc[NI];
#pragma unroll
    for (int q = 0; q < NI; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int l = 0; l < steps; ++l) {
      int64_t grow = -1;  // the row of this step: rb_lo + index, -1 = none
      if (l < len) {
        if (cur >= 0 && cur < nrows) grow = rb_lo + cur;
        else if (a.err) atomicOr(a.err, DLRM_TBE_ERR_INDEX);
      }
      cur = *(l + 1 < len ? a.idx + start + l + 1 : a.off);
      RowBits<FMT> r[NI];
      bool tab[NI];
#pragma unroll
      for (int q = 0; q < NI; ++q) {
        const int64_t g = __shfl(grow, q * RPI + sub, 64);
        tab[q] = g >= 0;  // (lane 0 and lanes >= F hold -1: feature 0 and rows >= F pool nothing)
        load_row<FMT, D>(r[q], tab[q] ? a.W + g * RB : xrow, c);
      }
#pragma unroll
      for (int q = 0; q < NI; ++q) {
        float4 s = acc[q];
        pool_row<FMT>(s, r[q]);
        if (tab[q]) acc[q] = s;
      }
    }
    if (sub == 0) acc[0] = xv;  // feature 0
    // unconditional stores (rows >= F hold zeros and are masked by rowok below; an inactive
    // wave's image is never read)
#pragma unroll
    for (int q = 0; q < NI; ++q)
      *reinterpret_cast<float4*>(Tl + (q * RPI + sub) * DP + 4 * c) = acc[q];
    if (a.pooled && active) {
      float* prow = a.pooled + b * a.pooled_bs + 4 * c;
#pragma unroll
      for (int q = 0; q < NI; ++q) {
        const int f = q * RPI + sub;
        if (f >= 1 && f < F) *reinterpret_cast<float4*>(prow + (int64_t)(f - 1) * D) = acc[q];
      }
    }
    __syncthreads();
    if (active) {
      const float* trow = Tl + l32 * DP + h * KH;
      f32x16 acc0, acc1;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
#pragma unroll
      for (int q = 0; q < KH / 4; ++q) {
        float4 v = *reinterpret_cast<const float4*>(trow + 4 * q);
        if (!rowok) v = make_float4(0.f, 0.f, 0.f, 0.f);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.x, v.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.y, v.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.z, v.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.w, v.w, acc1, 0, 0, 0);
      }
      for (int d = lane; d < D; d += 64) Ol[d] = Tl[d];  // x
      const int j = l32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
        if (i < F && (self ? i >= j : i > j)) Ol[D + pair_index(i, j, self)] = acc0[r] + acc1[r];
      }
    }
    __syncthreads();
    if (active) {
      float* orow = a.out + b * a.ld_out;
      if (vec_out) {
        const int w4 = width / 4;
        for (int q = lane; q < w4; q += 64)
          *reinterpret_cast<float4*>(orow + 4 * q) = *reinterpret_cast<const float4*>(Ol + 4 * q);
        for (int q = 4 * w4 + lane; q < width; q += 64) orow[q] = Ol[q];
      } else {
        for (int q = lane; q < width; q += 64) orow[q] = Ol[q];
      }
    }
    __syncthreads();
  }
}

template <int D, int FMT>
void launch_pool(int grid, size_t lds, hipStream_t st, int B, int F, int self, int width,
                 int vec_out, const PoolArgs& a) {
  hipLaunchKernelGGL((interact_pool_fwd<D, FMT>), dim3(grid), dim3(256), lds, st, B, F, self,
                     width, vec_out, a);
}

template <int FMT>
void launch_pool_d(int D, int grid, size_t lds, hipStream_t st, int B, int F, int self,
                   int width, int vec_out, const PoolArgs& a) {
  if (D == 16) launch_pool<16, FMT>(grid, lds, st, B, F, self, width, vec_out, a);
  else if (D == 32) launch_pool<32, FMT>(grid, lds, st, B, F, self, width, vec_out, a);
  else if (D == 64) launch_pool<64, FMT>(grid, lds, st, B, F, self, width, vec_out, a);
  else launch_pool<128, FMT>(grid, lds, st, B, F, self, width, vec_out, a);
}

}  // namespace

extern "C" int dlrm_interact_dot_forward_pool(int32_t B, int32_t F, int32_t D, const float* x,
                                              int64_t x_bstride, const void* weights,
                                              int32_t format, int64_t row_bytes,
                                              const int64_t* row_base, const int32_t* indices,
                                              const int32_t* offsets, int32_t self_interaction,
                                              float* out, int64_t ld_out, float* pooled_out,
                                              int64_t pooled_bstride, int32_t* error_flag,
                                              dlrm_stream_t stream) {
  const char* name = "dlrm_interact_dot_forward_pool";
  DLRM_REQUIRE(format == DLRM_ROWS_F32 || format == DLRM_ROWS_F16 || format == DLRM_ROWS_Q8 ||
                   format == DLRM_ROWS_Q4,
               DLRM_ERR_UNSUPPORTED, "%s: unknown row format %d", name, format);
  DLRM_ARG(B >= 0 && F >= 2 && F <= 32, "%s: need F in [2,32]", name);
  DLRM_REQUIRE(D == 16 || D == 32 || D == 64 || D == 128, DLRM_ERR_UNSUPPORTED,
               "%s: D must be 16, 32, 64 or 128", name);
  const int64_t want = format == DLRM_ROWS_F32 ? 4 * (int64_t)D : dlrm_tbe_row_bytes(format, D);
  DLRM_ARG(row_bytes == want, "%s: row_bytes %lld != %lld", name, (long long)row_bytes,
           (long long)want);
  if (B == 0) return DLRM_OK;
  // (indices may be null: a batch whose bags are all empty holds none)
  DLRM_ARG(x && weights && row_base && offsets && out, "%s: null pointer", name);
  const int walign = format == DLRM_ROWS_F16 ? 8 : 16;
  DLRM_ARG((reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
               (reinterpret_cast<uintptr_t>(weights) & (walign - 1)) == 0 && x_bstride % 4 == 0,
           "%s: x must be 16-B aligned, weights %d-B aligned, x_bstride %% 4 == 0", name, walign);
  DLRM_ARG(!pooled_out || ((reinterpret_cast<uintptr_t>(pooled_out) & 15) == 0 &&
                           pooled_bstride % 4 == 0 && pooled_bstride >= (int64_t)(F - 1) * D),
           "%s: pooled_out must be 16-B aligned, pooled_bstride %% 4 == 0 and >= (F-1)*D", name);
  const int npairs = self_interaction ? F * (F + 1) / 2 : F * (F - 1) / 2;
  DLRM_ARG(ld_out >= D + npairs, "%s: ld_out < D + pairs", name);
  const PoolArgs a{x, x_bstride, static_cast<const uint8_t*>(weights), row_base, indices, offsets,
                   out, ld_out, pooled_out, pooled_bstride, error_flag};
  const int width = D + npairs, self = self_interaction ? 1 : 0;
  const int vec_out = ((reinterpret_cast<uintptr_t>(out) & 15) == 0 && ld_out % 4 == 0) ? 1 : 0;
  const size_t lds = 4 * (32 * (size_t)(D + 4) + D + 32 * 33 / 2 + 4) * sizeof(float);
  const int grid = (int)std::min<int64_t>(dlrm::ceil_div(B, 4), 8192);
  hipStream_t st = dlrm::as_stream(stream);
  switch (format) {
    case DLRM_ROWS_F32: launch_pool_d<DLRM_ROWS_F32>(D, grid, lds, st, B, F, self, width, vec_out, a); break;
    case DLRM_ROWS_F16: launch_pool_d<DLRM_ROWS_F16>(D, grid, lds, st, B, F, self, width, vec_out, a); break;
    case DLRM_ROWS_Q8: launch_pool_d<DLRM_ROWS_Q8>(D, grid, lds, st, B, F, self, width, vec_out, a); break;
    default: launch_pool_d<DLRM_ROWS_Q4>(D, grid, lds, st, B, F, self, width, vec_out, a); break;
  }
  DLRM_LAUNCH_CHECK(name);
  return DLRM_OK;
}
