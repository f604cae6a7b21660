// Table-batched EmbeddingBag forward over reduced-precision rows:
//   DLRM_ROWS_F16 : fp16 weights, the fbgemm TBE's weights_precision=FP16 tables
//                   (DLRM_Net.create_emb_fbgemm, dlrm_s_pytorch.py:337-366);
//   DLRM_ROWS_Q8  : 8-bit row-wise quantized rows as packed by
//                   torch.ops.quantized.embedding_bag_byte_prepack (D uint8, then fp32
//                   scale, fp32 bias), looked up by embedding_bag_byte_rowwise_offsets
//                   (DLRM_Net.quantize_embedding / apply_emb, :554-567, 609-625);
//   DLRM_ROWS_Q4  : 4-bit row-wise (embedding_bag_4bit_prepack: ceil(D/2) bytes, element
//                   2i in the low nibble of byte i, then fp16 scale, fp16 bias).
// Dequantised value = q * scale + bias; a bag's sum accumulates in fp32 as
// acc = fma(w*scale, q, acc + w*bias) (w = per-sample weight or 1).
//
// Same data layout and launch shape as the fp32 lookup (tbe.hip): all tables in one
// buffer of fixed-size rows, table t = rows [row_base[t], row_base[t+1]), one group of LPB
// lanes per (table, bag), every lane owning 4 consecutive elements per 4*LPB, four rows of
// a bag in flight.  HBM-bound: a C3 row is 512 B in fp32, 256 B in fp16, 136 B in Q8 and
// 68 B in Q4, so the gather moves 2x / 3.8x / 7.5x fewer bytes.
//
// dlrm_rows_quantize (below the lookup) produces the Q8 / Q4 rows on the device from fp32 or
// fp16 rows, bitwise torch's packers.
#include "tbe_dispatch.hpp"

namespace {

using dlrm::kWave;

__device__ __forceinline__ float half_bits_to_float(uint32_t h) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
}

// Decode elements 4c .. 4c+3 of a row (quantized: the raw levels q).
template <int FMT>
__device__ __forceinline__ float4 load4(const uint8_t* __restrict__ row, int c) {
  if constexpr (FMT == DLRM_ROWS_F16) {
    const uint2 u = *reinterpret_cast<const uint2*>(row + 8 * c);
    return make_float4(half_bits_to_float(u.x & 0xffff), half_bits_to_float(u.x >> 16),
                       half_bits_to_float(u.y & 0xffff), half_bits_to_float(u.y >> 16));
  } else if constexpr (FMT == DLRM_ROWS_Q8) {
    const uint32_t u = *reinterpret_cast<const uint32_t*>(row + 4 * c);
    return make_float4((float)(u & 0xff), (float)((u >> 8) & 0xff), (float)((u >> 16) & 0xff),
                       (float)(u >> 24));
  } else {
    const uint32_t u = *reinterpret_cast<const uint16_t*>(row + 2 * c);
    return make_float4((float)(u & 0xf), (float)((u >> 4) & 0xf), (float)((u >> 8) & 0xf),
                       (float)((u >> 12) & 0xf));
  }
}

template <int FMT>
__device__ __forceinline__ float2 scale_bias(const uint8_t* __restrict__ row, int64_t D) {
  if constexpr (FMT == DLRM_ROWS_Q8) {  // rows are 4-byte aligned (D % 4 == 0)
    const float* sb = reinterpret_cast<const float*>(row + D);
    return make_float2(sb[0], sb[1]);
  } else if constexpr (FMT == DLRM_ROWS_Q4) {  // rows are 2-byte aligned
    const uint16_t* sb = reinterpret_cast<const uint16_t*>(row + (D + 1) / 2);
    return make_float2(half_bits_to_float(sb[0]), half_bits_to_float(sb[1]));
  } else {
    return make_float2(1.f, 0.f);
  }
}

template <int FMT, int LPB, int MAXV, typename IdxT, typename OffT>
__global__ __launch_bounds__(256) void tbe_rows_fwd_kernel(
    const uint8_t* __restrict__ Wb, int64_t row_bytes, int64_t D,
    const int64_t* __restrict__ row_base, int T, int B, const IdxT* __restrict__ idx,
    const OffT* __restrict__ off, const float* __restrict__ psw, float* __restrict__ out,
    int64_t out_bs, int32_t* __restrict__ err) {
  constexpr int GPW = kWave / LPB;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPB;
  const int gl = lane - g * LPB;
  const int nchunks = (int)(D / 4);
  const int64_t nbags = (int64_t)T * B;
  const int64_t wave_id = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / kWave);

  for (int64_t bag0 = wave_id * GPW; bag0 < nbags; bag0 += nwaves * GPW) {
    const int64_t bag = bag0 + g;
    const bool active = bag < nbags;
    int t = 0, b = 0;
    int64_t start = 0, end = 0, base = 0, nrows = 0;
    if (active) {
      t = (int)(bag / B);
      b = (int)(bag - (int64_t)t * B);
      start = (int64_t)off[bag];
      end = (int64_t)off[bag + 1];
      base = row_base[t];
      nrows = row_base[t + 1] - base;
    }
    float4 acc[MAXV];
#pragma unroll
    for (int c = 0; c < MAXV; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int64_t l0 = start; l0 < end; l0 += LPB) {
      const int n = (int)((end - l0) < LPB ? (end - l0) : LPB);
      int64_t my_row = -1;
      float my_w = 1.f;
      if (gl < n) {
        int64_t r = (int64_t)idx[l0 + gl];
        if (r < 0 || r >= nrows) {
          if (err) atomicOr(err, DLRM_TBE_ERR_INDEX);
          r = -1;
        }
        my_row = r;
        if (psw) my_w = psw[l0 + gl];
      }
      for (int j = 0; j < n; j += 4) {
        int64_t r[4];
        float w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int src = g * LPB + ((j + u) < LPB ? (j + u) : 0);
          r[u] = __shfl(my_row, src, kWave);
          w[u] = __shfl(my_w, src, kWave);
          if (j + u >= n) r[u] = -1;
        }
        // all four rows' loads issued before any is used (invalid rows read row 0 of the
        // table and are dropped at the accumulation)
        float4 v[4][MAXV];
        float2 sb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uint8_t* row = Wb + (base + (r[u] >= 0 ? r[u] : 0)) * row_bytes;
          sb[u] = scale_bias<FMT>(row, D);
#pragma unroll
          for (int c = 0; c < MAXV; ++c) {
            const int chunk = gl + c * LPB;
            v[u][c] = load4<FMT>(row, chunk < nchunks ? chunk : 0);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (r[u] >= 0) {
            const float ws = w[u] * sb[u].x, wb = w[u] * sb[u].y;
#pragma unroll
            for (int c = 0; c < MAXV; ++c) {
              if (FMT == DLRM_ROWS_F16) {
                acc[c].x = fmaf(w[u], v[u][c].x, acc[c].x);
                acc[c].y = fmaf(w[u], v[u][c].y, acc[c].y);
                acc[c].z = fmaf(w[u], v[u][c].z, acc[c].z);
                acc[c].w = fmaf(w[u], v[u][c].w, acc[c].w);
              } else {
                acc[c].x = fmaf(ws, v[u][c].x, acc[c].x + wb);
                acc[c].y = fmaf(ws, v[u][c].y, acc[c].y + wb);
                acc[c].z = fmaf(ws, v[u][c].z, acc[c].z + wb);
                acc[c].w = fmaf(ws, v[u][c].w, acc[c].w + wb);
              }
            }
          }
        }
      }
    }
    if (active) {
      float4* o = reinterpret_cast<float4*>(out + (int64_t)b * out_bs + (int64_t)t * D);
#pragma unroll
      for (int c = 0; c < MAXV; ++c) {
        const int chunk = gl + c * LPB;
        if (chunk < nchunks) o[chunk] = acc[c];
      }
    }
  }
}

int64_t min_row_bytes(int fmt, int64_t D) {
  switch (fmt) {
    case DLRM_ROWS_F16: return 2 * D;
    case DLRM_ROWS_Q8: return D + 8;
    case DLRM_ROWS_Q4: return (D + 1) / 2 + 4;
    default: return -1;
  }
}

// (the entry point has checked D % 4 == 0 and D <= 512: at most 2 float4 chunks per lane)
template <int FMT, typename IdxT, typename OffT>
int launch_rows_fwd(const uint8_t* W, int64_t row_bytes, int64_t D, const int64_t* row_base,
                    int T, int B, const IdxT* idx, const OffT* off, const float* psw, float* out,
                    int64_t out_bs, int32_t* err, hipStream_t st) {
  const LaneGeom g = lane_geom(D / 4, 4);
  const int64_t blocks = lane_blocks((int64_t)T * B, g.lpb, 4);
  for_lanes<4, 2>(g, [&](auto lpb, auto mv) {
    hipLaunchKernelGGL(
        (tbe_rows_fwd_kernel<FMT, decltype(lpb)::value, decltype(mv)::value, IdxT, OffT>),
        dim3(blocks), dim3(256), 0, st, W, row_bytes, D, row_base, T, B, idx, off, psw, out,
        out_bs, err);
  });
  DLRM_LAUNCH_CHECK("dlrm_tbe_forward_rows");
  return DLRM_OK;
}

// ------------------------------------------------------- row-wise quantizer --
// dlrm_rows_quantize: fp32 / fp16 rows -> Q8 / Q4 rows, bitwise what torch.ops.quantized
// .embedding_bag_byte_prepack / embedding_bag_4bit_prepack return for the same fp32 rows
// (DLRM_Net.quantize_embedding, dlrm_s_pytorch.py:609-625), on the device.  The lookup's lane
// groups: LPB lanes per row, each lane owning the columns [4 chunk, 4 chunk + 4) of chunk =
// gl (+ LPB above D = 256), 64 / LPB rows per wave.  A lane loads its columns once
// (nontemporal: the table is read once), the row's min and max meet by a butterfly inside
// the group (order-independent, so exact), every lane quantises and stores its own columns
// and the group's first lane stores scale and bias.  All arithmetic is fp32 with one
// rounding per operation (true division, rintf, no contraction).
typedef float f32x4_nt __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_nt __attribute__((ext_vector_type(2)));

template <int SRC>
__device__ __forceinline__ float4 quant_load4(const void* __restrict__ src, int64_t elem) {
  if constexpr (SRC == DLRM_ROWS_F32) {
    const f32x4_nt v = __builtin_nontemporal_load(
        reinterpret_cast<const f32x4_nt*>(static_cast<const float*>(src) + elem));
    return make_float4(v.x, v.y, v.z, v.w);
  } else {  // fp16 rows, widened exactly
    const u32x2_nt u = __builtin_nontemporal_load(
        reinterpret_cast<const u32x2_nt*>(static_cast<const uint16_t*>(src) + elem));
    return make_float4(half_bits_to_float(u.x & 0xffff), half_bits_to_float(u.x >> 16),
                       half_bits_to_float(u.y & 0xffff), half_bits_to_float(u.y >> 16));
  }
}

__device__ __forceinline__ float half_rne(float x) { return (float)(_Float16)x; }
__device__ __forceinline__ uint16_t half_bits(float x) {
  return __builtin_bit_cast(unsigned short, (_Float16)x);
}

__device__ __forceinline__ uint32_t quant_level(float x, float mn, float inv, float top) {
#pragma clang fp contract(off)
  const float d = x - mn;
  float q = rintf(d * inv);  // ties to even
  q = q < 0.f ? 0.f : (q > top ? top : q);
  return (uint32_t)q;
}

template <int SRC, int FMT, int LPB, int MAXV>
__global__ __launch_bounds__(256) void rows_quantize_kernel(const void* __restrict__ src,
                                                            int64_t rows, int D,
                                                            uint8_t* __restrict__ dst) {
#pragma clang fp contract(off)
  constexpr int GPW = kWave / LPB;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPB;
  const int gl = lane - g * LPB;
  const int nchunks = D / 4;
  const int64_t row_bytes = FMT == DLRM_ROWS_Q8 ? D + 8 : D / 2 + 4;
  const int64_t wave_id = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / kWave);
  for (int64_t r0 = wave_id * GPW; r0 < rows; r0 += nwaves * GPW) {  // wave-uniform trip count
    const int64_t r = r0 + g;
    float4 v[MAXV];
    bool ok[MAXV];
    float mn = __builtin_inff(), mx = -__builtin_inff();
#pragma unroll
    for (int c = 0; c < MAXV; ++c) {
      const int chunk = gl + c * LPB;
      ok[c] = r < rows && chunk < nchunks;
      v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ok[c]) {
        v[c] = quant_load4<SRC>(src, r * D + 4 * chunk);
        mn = fminf(fminf(mn, fminf(v[c].x, v[c].y)), fminf(v[c].z, v[c].w));
        mx = fmaxf(fmaxf(mx, fmaxf(v[c].x, v[c].y)), fmaxf(v[c].z, v[c].w));
      }
    }
#pragma unroll
    for (int o = LPB / 2; o >= 1; o >>= 1) {  // stays inside the aligned group of LPB lanes
      mn = fminf(mn, __shfl_xor(mn, o, kWave));
      mx = fmaxf(mx, __shfl_xor(mx, o, kWave));
    }
    uint8_t* row = dst + r * row_bytes;
    if constexpr (FMT == DLRM_ROWS_Q8) {
      const float range = mx - mn;
      const float scale = range / 255.0f;
      const float inv = 255.0f / (range + 1e-8f);
#pragma unroll
      for (int c = 0; c < MAXV; ++c) {
        if (ok[c]) {
          const uint32_t u = quant_level(v[c].x, mn, inv, 255.f) |
                             (quant_level(v[c].y, mn, inv, 255.f) << 8) |
                             (quant_level(v[c].z, mn, inv, 255.f) << 16) |
                             (quant_level(v[c].w, mn, inv, 255.f) << 24);
          *reinterpret_cast<uint32_t*>(row + 4 * (gl + c * LPB)) = u;
        }
      }
      if (gl == 0 && r < rows) {
        float* sb = reinterpret_cast<float*>(row + D);
        sb[0] = scale;
        sb[1] = mn;
      }
    } else {
      const float mnh = half_rne(mn);
      const float range = mx - mnh;
      float scale = half_rne(range / 15.0f);
      if (scale == 0.f) scale = 1.f;
      float inv = 1.0f / scale;
      if (__builtin_isinf(inv)) scale = inv = 1.f;
#pragma unroll
      for (int c = 0; c < MAXV; ++c) {
        if (ok[c]) {
          const uint32_t u = quant_level(v[c].x, mnh, inv, 15.f) |
                             (quant_level(v[c].y, mnh, inv, 15.f) << 4) |
                             (quant_level(v[c].z, mnh, inv, 15.f) << 8) |
                             (quant_level(v[c].w, mnh, inv, 15.f) << 12);
          *reinterpret_cast<uint16_t*>(row + 2 * (gl + c * LPB)) = (uint16_t)u;
        }
      }
      if (gl == 0 && r < rows) {  // Q4 rows are 2-byte aligned in general
        uint16_t* sb = reinterpret_cast<uint16_t*>(row + D / 2);
        sb[0] = half_bits(scale);
        sb[1] = half_bits(mnh);
      }
    }
  }
}

template <int SRC, int FMT>
int launch_rows_quantize(const void* src, int64_t rows, int D, uint8_t* dst, hipStream_t st) {
  const LaneGeom g = lane_geom(D / 4);  // (D <= 512: at most 2 chunks per lane)
  const int64_t blocks = lane_blocks(rows, g.lpb, 4);
  for_lanes<1, 2>(g, [&](auto lpb, auto mv) {
    hipLaunchKernelGGL((rows_quantize_kernel<SRC, FMT, decltype(lpb)::value, decltype(mv)::value>),
                       dim3(blocks), dim3(256), 0, st, src, rows, D, dst);
  });
  DLRM_LAUNCH_CHECK("dlrm_rows_quantize");
  return DLRM_OK;
}

}  // namespace

extern "C" int dlrm_rows_quantize(const void* src, int32_t src_format, int64_t rows, int64_t D,
                                  int32_t dst_format, void* dst, int64_t dst_row_bytes,
                                  dlrm_stream_t stream) {
  const char* name = "dlrm_rows_quantize";
  DLRM_ARG(src_format == DLRM_ROWS_F32 || src_format == DLRM_ROWS_F16,
           "%s: source format %d is not F32 | F16", name, src_format);
  DLRM_ARG(dst_format == DLRM_ROWS_Q8 || dst_format == DLRM_ROWS_Q4,
           "%s: destination format %d is not Q8 | Q4", name, dst_format);
  DLRM_ARG(rows >= 0 && D > 0, "%s: bad sizes", name);
  DLRM_REQUIRE(D % 4 == 0 && D <= 512, DLRM_ERR_UNSUPPORTED,
               "%s: D must be a multiple of 4 and <= 512 (D=%lld)", name, (long long)D);
  DLRM_ARG(dst_row_bytes == min_row_bytes(dst_format, D), "%s: dst_row_bytes %lld != %lld", name,
           (long long)dst_row_bytes, (long long)min_row_bytes(dst_format, D));
  if (rows == 0) return DLRM_OK;
  DLRM_ARG(src && dst, "%s: null pointer", name);
  DLRM_REQUIRE((reinterpret_cast<uintptr_t>(src) % (src_format == DLRM_ROWS_F32 ? 16 : 8)) == 0 &&
                   (reinterpret_cast<uintptr_t>(dst) % (dst_format == DLRM_ROWS_Q8 ? 4 : 2)) == 0,
               DLRM_ERR_UNSUPPORTED, "%s: misaligned source or destination", name);
  hipStream_t st = dlrm::as_stream(stream);
  uint8_t* out = static_cast<uint8_t*>(dst);
  if (src_format == DLRM_ROWS_F32)
    return dst_format == DLRM_ROWS_Q8
               ? launch_rows_quantize<DLRM_ROWS_F32, DLRM_ROWS_Q8>(src, rows, (int)D, out, st)
               : launch_rows_quantize<DLRM_ROWS_F32, DLRM_ROWS_Q4>(src, rows, (int)D, out, st);
  return dst_format == DLRM_ROWS_Q8
             ? launch_rows_quantize<DLRM_ROWS_F16, DLRM_ROWS_Q8>(src, rows, (int)D, out, st)
             : launch_rows_quantize<DLRM_ROWS_F16, DLRM_ROWS_Q4>(src, rows, (int)D, out, st);
}

extern "C" int64_t dlrm_tbe_row_bytes(int32_t format, int64_t D) { return min_row_bytes(format, D); }

extern "C" int dlrm_tbe_forward_rows(const void* weights, int32_t format, int64_t row_bytes,
                                     int64_t D, const int64_t* row_base, int32_t T, int32_t B,
                                     const void* indices, int32_t index_bits, const void* offsets,
                                     int32_t offset_bits, const float* per_sample_weights,
                                     float* out, int64_t out_batch_stride, int32_t* error_flag,
                                     dlrm_stream_t stream) {
  const char* name = "dlrm_tbe_forward_rows";
  DLRM_ARG(weights && row_base && out && offsets && indices, "%s: null pointer", name);
  DLRM_ARG(format == DLRM_ROWS_F16 || format == DLRM_ROWS_Q8 || format == DLRM_ROWS_Q4,
           "%s: bad row format %d", name, format);
  DLRM_ARG(T >= 0 && B >= 0 && D > 0, "%s: bad sizes", name);
  DLRM_ARG(index_bits == 32 || index_bits == 64, "%s: index_bits must be 32|64", name);
  DLRM_ARG(offset_bits == 32 || offset_bits == 64, "%s: offset_bits must be 32|64", name);
  DLRM_ARG(row_bytes >= min_row_bytes(format, D), "%s: row_bytes %lld < %lld", name,
           (long long)row_bytes, (long long)min_row_bytes(format, D));
  DLRM_ARG(out_batch_stride >= (int64_t)T * D, "%s: out_batch_stride < T*D", name);
  DLRM_REQUIRE(D % 4 == 0 && D <= 512, DLRM_ERR_UNSUPPORTED,
               "%s: D must be a multiple of 4 and <= 512 (D=%lld)", name, (long long)D);
  const int align = format == DLRM_ROWS_F16 ? 8 : (format == DLRM_ROWS_Q8 ? 4 : 2);
  DLRM_REQUIRE((reinterpret_cast<uintptr_t>(weights) % align) == 0 && row_bytes % align == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & 15) == 0 && out_batch_stride % 4 == 0,
               DLRM_ERR_UNSUPPORTED, "%s: misaligned rows or output", name);
  if ((int64_t)T * B == 0) return DLRM_OK;
  hipStream_t st = dlrm::as_stream(stream);
  const uint8_t* W = static_cast<const uint8_t*>(weights);
  return for_csr_widths(index_bits, offset_bits, [&](auto i, auto o) {
    const auto lookup = [&](auto fmt) {
      return launch_rows_fwd<decltype(fmt)::value>(W, row_bytes, D, row_base, T, B,
                                                   i.ptr(indices), o.ptr(offsets),
                                                   per_sample_weights, out, out_batch_stride,
                                                   error_flag, st);
    };
    switch (format) {
      case DLRM_ROWS_F16: return lookup(int_tag<DLRM_ROWS_F16>{});
      case DLRM_ROWS_Q8: return lookup(int_tag<DLRM_ROWS_Q8>{});
      default: return lookup(int_tag<DLRM_ROWS_Q4>{});
    }
  });
}
