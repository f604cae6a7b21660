// 16-bit row-block MLP chain (dlrm_mlp_chain16_forward, ABI v21): up to four Linear+ReLU
// layers with bf16 / fp16 MFMA operands in ONE launch,
//   Y_l[r][c] = relu_nan( sum_{k<K_l} r16(In_l[r][k]) * r16(W_l[c][k]) + bias_l[c * stride_l] )
// In_0 = X, In_l = Y_{l-1} (K_l = N_{l-1}); the arithmetic of dlrm_linear16_forward (linear16.hip)
// applied layer by layer, and the same bits: one fp32 accumulator chain per output element on
// v_mfma_f32_16x16x32_{bf16,f16}, the 32-k blocks in ascending order, lane group lane >> 4
// holding k = 32 blk + 8 (lane >> 4) .. + 7 of both operands, elements with k >= K_l selected
// to zero.  (The per-layer kernel pads K to 64, this one to 32: an all-zero MFMA more or less
// changes at most the sign of a zero.)
//
// Work split: one workgroup of 16 waves per 16 rows; wave w owns the 16-column tiles w and
// w + 16 of every layer (N_l <= 512).  No traffic between workgroups, no atomics.
//
// Activations live in LDS as two [16 rows][kC16Pitch] images of 16-bit elements.  An activation
// is rounded once, when the epilogue writes it - the value the next per-layer launch would
// round from the fp32 Y.  kC16Pitch is 65 chunks of 16 bytes: the A fragment is one ds_read_b128
// per lane and 32-k block (row lane & 15, chunk 4 blk + (lane >> 4)), and the 16 lanes of a
// group sit at chunk slots (65 r + c) mod 16 = (r + c) mod 16, sixteen different ones, so
// they cover the 64 banks once.
//
// B fragments are the fp32 weights read straight from global / L2 (two 16-byte loads per
// lane where the 32-k block lies wholly below K_l in a 16-byte aligned row, element loads
// under a select otherwise), kept in a register ring kC16Ring blocks deep and converted with
// four packed converts right before their MFMA.  Column K_l of W_l (the trainer's folded bias) and the
// padding behind it are never read.  A lane whose column is >= N_l reads the last row
// instead; its results are not stored.
#include "linear16_stage.hpp"

namespace dlrm {
namespace {

using namespace l16;

constexpr int kC16Rows = 16;    // samples per workgroup
constexpr int kC16Waves = 16;   // waves per workgroup (1024 threads)
constexpr int kC16Tiles = 2;    // 16-column tiles per wave: N <= 16 * 2 * 16 = 512
constexpr int kC16MaxW = kC16Waves * kC16Tiles * 16;
constexpr int kC16Pitch = kC16MaxW + 8;  // elements per LDS row: 65 chunks of 16 bytes
constexpr int kC16Ring = 4;     // 32-k blocks of weights in registers: 128 k in flight
static_assert(kC16Tiles == 2, "chain16_body dispatches chain16_kloop<1..2>");
static_assert((kC16Pitch / 8) % 2 == 1, "an odd chunk pitch keeps ds_read_b128 conflict-free");

struct Chain16 {
  int layers;
  int k0;
  int64_t rows;
  const float* X;
  int64_t ldx;
  int n[DLRM_MLP_MAX_LAYERS];
  int aligned[DLRM_MLP_MAX_LAYERS];  // W_l's rows start on 16-byte boundaries
  const float* W[DLRM_MLP_MAX_LAYERS];
  int64_t ldw[DLRM_MLP_MAX_LAYERS];
  const float* bias[DLRM_MLP_MAX_LAYERS];
  int64_t bias_stride[DLRM_MLP_MAX_LAYERS];
  float* Y[DLRM_MLP_MAX_LAYERS];
  int64_t ldy[DLRM_MLP_MAX_LAYERS];
};

// K loop of one layer for this wave's NTW column tiles: acc[j] += A(16 x K) . W_tile^T.
// wp[j]: the lane's weight row of tile j.  The blocks that lie wholly below K in a 16-byte
// aligned row (nfull of them) go through the ring: blocks c + 1 .. c + kC16Ring - 1 are in
// flight under block c's MFMAs; the tile count is a template argument, so that loop has no
// branch on it and the ring stays in registers.  The rest - the tail block of K % 32 != 0,
// every block of an unaligned W - follows one block ahead with element loads: the address of
// an element at k >= K is clamped to K - 1 and its value selected to zero, so nothing behind
// K is read and nothing is multiplied away.  Ascending block order throughout.
template <typename T, int NTW>
__device__ __forceinline__ void chain16_kloop(f32x4 (&acc)[kC16Tiles], const T* in,
                                              const float* (&wp)[kC16Tiles], int K,
                                              int nblk, int nfull, int l16, int g) {
  using vec = typename Op16<T>::vec;
  constexpr int R = kC16Ring;
  auto fetch = [&](int c, float4 (&bv)[NTW][2]) {
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      const float4* p = reinterpret_cast<const float4*>(wp[j] + 32 * c + 8 * g);
      bv[j][0] = p[0];
      bv[j][1] = p[1];
    }
  };
  auto fetch_elems = [&](int c, float4 (&bv)[NTW][2]) {
    const int k = 32 * c + 8 * g;
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      float e[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float v = wp[j][k + i < K ? k + i : K - 1];
        e[i] = k + i < K ? v : 0.0f;  // select, not multiply
      }
      bv[j][0] = make_float4(e[0], e[1], e[2], e[3]);
      bv[j][1] = make_float4(e[4], e[5], e[6], e[7]);
    }
  };
  auto lda = [&](int c) {
    return *reinterpret_cast<const vec*>(in + l16 * kC16Pitch + 32 * c + 8 * g);
  };
  vec a = lda(0);
  auto step = [&](int c, const float4 (&bv)[NTW][2]) {
    const vec an = lda(c + 1 < nblk ? c + 1 : c);
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      vec b;  // RNE, four packed converts
      b[0] = static_cast<T>(bv[j][0].x), b[1] = static_cast<T>(bv[j][0].y);
      b[2] = static_cast<T>(bv[j][0].z), b[3] = static_cast<T>(bv[j][0].w);
      b[4] = static_cast<T>(bv[j][1].x), b[5] = static_cast<T>(bv[j][1].y);
      b[6] = static_cast<T>(bv[j][1].z), b[7] = static_cast<T>(bv[j][1].w);
      acc[j] = Op16<T>::mfma(a, b, acc[j]);
    }
    a = an;
  };
  {
    float4 ring[R][NTW][2];
#pragma unroll
    for (int u = 0; u < R - 1; ++u)
      if (u < nfull) fetch(u, ring[u]);
    for (int c0 = 0; c0 < nfull; c0 += R) {
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int c = c0 + u;
        if (c >= nfull) break;
        if (c + R - 1 < nfull) fetch(c + R - 1, ring[(u + R - 1) % R]);
        step(c, ring[u]);
      }
    }
  }
  if (nfull < nblk) {
    float4 cur[NTW][2], nxt[NTW][2];
    fetch_elems(nfull, cur);
    for (int c = nfull; c < nblk; ++c) {
      if (c + 1 < nblk) fetch_elems(c + 1, nxt);
      step(c, cur);
#pragma unroll
      for (int j = 0; j < NTW; ++j) cur[j][0] = nxt[j][0], cur[j][1] = nxt[j][1];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kC16Waves * 64) void mlp_chain16_kernel(Chain16 mc) {
  constexpr int RB = kC16Rows, P = kC16Pitch, NW = kC16Waves, MT = kC16Tiles;
  constexpr int NT = NW * 64;
  __shared__ __attribute__((aligned(16))) T lds[2][RB * P];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // uniform: scalar tile tests
  const int g = lane >> 4, l16 = lane & 15;
  const int64_t r0 = int64_t(blockIdx.x) * RB;
  const int nrow = mc.rows - r0 < RB ? int(mc.rows - r0) : RB;
  T* in = lds[0];
  T* nx = lds[1];
  int K = mc.k0;
  {  // layer 0 input: r16(X), zeros for rows past the batch and up to the 32-k boundary
    const int kr = (K + 31) & ~31;
    for (int e = tid; e < RB * kr; e += NT) {
      const int r = e / kr, k = e - r * kr;
      float v = 0.0f;
      if (r < nrow && k < K) v = mc.X[(r0 + r) * mc.ldx + k];
      in[r * P + k] = static_cast<T>(v);
    }
  }
  __syncthreads();
  for (int l = 0; l < mc.layers; ++l) {
    const int n = mc.n[l];
    const int nblk = (K + 31) / 32, ntile = (n + 15) / 16;
    const int nfull = mc.aligned[l] ? K / 32 : 0;  // blocks the 16-byte loads take
    const float* W = mc.W[l];
    const int64_t ldw = mc.ldw[l];
    const int nt_w = ntile > wave ? (ntile - wave + NW - 1) / NW : 0;  // this wave's tiles
    f32x4 acc[MT];
    const float* wp[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int col = (wave + j * NW) * 16 + l16;
      wp[j] = W + int64_t(col < n ? col : n - 1) * ldw;  // clamped columns are never stored
    }
    switch (nt_w) {
      case 1: chain16_kloop<T, 1>(acc, in, wp, K, nblk, nfull, l16, g); break;
      case 2: chain16_kloop<T, 2>(acc, in, wp, K, nblk, nfull, l16, g); break;
      default: break;
    }
    // epilogue; C/D map of 16x16: col = lane & 15, row = (lane >> 4) * 4 + reg
    const float* bias = mc.bias[l];
    const int64_t bstride = mc.bias_stride[l];
    float* Y = mc.Y[l];
    const int64_t ldy = mc.ldy[l];
    const bool more = l + 1 < mc.layers;
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int col = (wave + j * NW) * 16 + l16;
      if (j < nt_w && col < n) {
        const float bv = bias ? bias[col * bstride] : 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 4 * g + r;
          float y = acc[j][r] + bv;
          y = (y != y) ? y : fmaxf(y, 0.0f);  // NaN propagates
          if (Y && row < nrow) Y[(r0 + row) * ldy + col] = y;
          if (more) nx[row * P + col] = static_cast<T>(y);
        }
      }
    }
    if (more) {  // zeros from n to the next layer's 32-k boundary
      const int extra = ((n + 31) & ~31) - n;
      for (int e = tid; e < RB * extra; e += NT) {
        const int r = e / extra, c = n + (e - r * extra);
        nx[r * P + c] = static_cast<T>(0.0f);
      }
    }
    __syncthreads();
    T* t = in;
    in = nx;
    nx = t;
    K = n;
  }
}

// Host-side check + conversion (the ABI struct -> the kernel argument).  Returns a dlrm_status
// and leaves its text in dlrm_last_error.
int chain16_prepare(const dlrm_mlp_chain16* c, Chain16& mc, const char* who) {
  DLRM_ARG(c != nullptr, "%s: null chain", who);
  DLRM_ARG(c->type == DLRM_MLP16_BF16 || c->type == DLRM_MLP16_F16, "%s: unknown type %d", who,
           (int)c->type);
  DLRM_ARG(c->rows >= 0, "%s: negative rows", who);
  DLRM_REQUIRE(c->layers >= 1 && c->layers <= DLRM_MLP_MAX_LAYERS, DLRM_ERR_UNSUPPORTED,
               "%s: %d layers (1..%d)", who, (int)c->layers, DLRM_MLP_MAX_LAYERS);
  const bool work = c->rows > 0;  // rows == 0: nothing is read or written
  DLRM_ARG(c->X != nullptr || !work, "%s: null X", who);
  DLRM_REQUIRE(c->in_width >= 1 && c->in_width <= kC16MaxW, DLRM_ERR_UNSUPPORTED,
               "%s: in_width %lld (1..%d)", who, (long long)c->in_width, kC16MaxW);
  DLRM_REQUIRE(c->ldx >= c->in_width, DLRM_ERR_SHAPE, "%s: ldx %lld < in_width %lld", who,
               (long long)c->ldx, (long long)c->in_width);
  DLRM_REQUIRE(ceil_div(c->rows, kC16Rows) <= INT32_MAX, DLRM_ERR_UNSUPPORTED,
               "%s: more than 2^31 - 1 row blocks", who);
  mc.layers = c->layers;
  mc.k0 = (int)c->in_width;
  mc.rows = c->rows;
  mc.X = c->X;
  mc.ldx = c->ldx;
  int64_t k = c->in_width;
  for (int l = 0; l < c->layers; ++l) {
    const int64_t n = c->out_width[l];
    DLRM_REQUIRE(n >= 1 && n <= kC16MaxW, DLRM_ERR_UNSUPPORTED,
                 "%s: out_width[%d] = %lld (1..%d)", who, l, (long long)n, kC16MaxW);
    DLRM_ARG(c->W[l] != nullptr || !work, "%s: null W[%d]", who, l);
    DLRM_ARG(c->Y[l] != nullptr || l + 1 < c->layers || !work,
             "%s: the last layer's Y is required", who);
    DLRM_REQUIRE(c->ldw[l] >= k && c->ldy[l] >= n, DLRM_ERR_SHAPE,
                 "%s: layer %d: ldw %lld < K %lld or ldy %lld < N %lld", who, l,
                 (long long)c->ldw[l], (long long)k, (long long)c->ldy[l], (long long)n);
    mc.n[l] = (int)n;
    mc.aligned[l] = reinterpret_cast<uintptr_t>(c->W[l]) % 16 == 0 && c->ldw[l] % 4 == 0;
    mc.W[l] = c->W[l];
    mc.ldw[l] = c->ldw[l];
    mc.bias[l] = c->bias[l];
    mc.bias_stride[l] = c->bias_stride[l];
    mc.Y[l] = c->Y[l];
    mc.ldy[l] = c->ldy[l];
    k = n;
  }
  return DLRM_OK;
}

}  // namespace
}  // namespace dlrm

extern "C" int dlrm_mlp_chain16_supported(const dlrm_mlp_chain16* chain) {
  dlrm::Chain16 mc{};
  return dlrm::chain16_prepare(chain, mc, "dlrm_mlp_chain16_supported") == DLRM_OK;
}

extern "C" int dlrm_mlp_chain16_forward(const dlrm_mlp_chain16* chain, dlrm_stream_t stream) {
  using namespace dlrm;
  Chain16 mc{};
  const int rc = chain16_prepare(chain, mc, "dlrm_mlp_chain16_forward");
  if (rc != DLRM_OK) return rc;
  if (mc.rows == 0) return DLRM_OK;
  const dim3 grid((unsigned)ceil_div(mc.rows, kC16Rows)), block(kC16Waves * 64);
  if (chain->type == DLRM_MLP16_BF16)
    hipLaunchKernelGGL(mlp_chain16_kernel<__bf16>, grid, block, 0, as_stream(stream), mc);
  else
    hipLaunchKernelGGL(mlp_chain16_kernel<_Float16>, grid, block, 0, as_stream(stream), mc);
  DLRM_LAUNCH_CHECK("dlrm_mlp_chain16_forward");
  return DLRM_OK;
}
