// The 16-bit Linear backward as ONE grouped launch (dlrm_linear16_bwd_group, ABI v22): up to
// four independent problems, each a dgrad or a wgrad of linear16_bwd.hip with that file's
// semantics, tile body (linear16_bwd_tile.hpp) and plan.
//
// Work split.  The launch is a flat list of workgroups; problem i owns the contiguous range
// [block0_i, block0_i + tiles_i * splits_i).  Inside its range a workgroup is (split, tile)
// with the per-problem kernel's XCD run remap over the tiles, and runs the body of its
// problem's kind (TRANS_A), tile and alignment.  The kernel is instantiated on the LARGEST
// tile class of the group (CLS, an index into kTiles): its LDS image and its register budget
// are that class's, and only bodies of that class and smaller ones are compiled into it, so
// a group of 64 x 64 and 32 x 64 tiles keeps the occupancy those tiles have stand-alone.
//
// Split wgrads finish inside the launch.  A split workgroup stores its accumulators as a
// record in FRAGMENT order - record[(f * 256 + tid) * 4 .. + 4] is accumulator f of thread
// tid, so a wave's 16-byte stores are contiguous - and takes the tile's ticket; the last
// arriver loads every split's record (its own too, from memory), sums them in split order
// p[0] + p[1] + ..., which is wgrad16_reduce_kernel's order element by element, and applies
// STORE / SGD through the shared epilogue.  Nobody waits on anybody; no floating-point
// atomics.  Publication across the per-XCD L2s is splitk_reduce's (gemm.hip): sc1 record
// stores, s_waitcnt vmcnt(0), barrier, relaxed agent-scope ticket, sc1 record loads; the last
// arriver zeroes the ticket, so the next launch (or a graph replay) finds zeros.
//
// Workspace: [kGroupTickets int32 tickets, zero between launches][records of the split
// problems, 256-byte aligned, [tile][split][BM * BN] fp32 each].
#include "linear16_bwd_tile.hpp"

namespace dlrm {
namespace {

using namespace l16;

constexpr int kMaxGroup = 4;
constexpr int kGroupTickets = 4096;  // split tiles of one launch (the workspace's head)

struct GroupProb {
  BwdArgs a;        // a.epi: the problem's FINAL epilogue (dgrad / store / sgd) into a.Out
  int block0;       // first workgroup
  int splits;
  int tile;         // index into kTiles
  int trans_a;      // 1: wgrad (dY is read transposed)
  int aligned;
  int* tickets;     // splits > 1: one per tile
  float* records;   // splits > 1
};

struct GroupArgs {
  GroupProb p[kMaxGroup];
  int n;
};

// A split tile's hand-off; true in the workgroup that must write the output, acc then holds
// the sum over the splits.
template <int BM, int BN>
__device__ __forceinline__ bool split_fold(const GroupProb& P, int tile, int split,
                                           f32x4 (&acc)[BM / 32][BN / 32], void* smem) {
  constexpr int FM = BM / 32, FN = BN / 32;
  constexpr int REC = BM * BN;
  using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
  const int tid = threadIdx.x;
  float* base = P.records + int64_t(tile) * P.splits * REC;
  const __amdgpu_buffer_rsrc_t rr =
      __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, P.splits * REC * 4, 0x00020000);
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
      __builtin_amdgcn_raw_buffer_store_b128(
          __builtin_bit_cast(u32x4, acc[i][j]), rr,
          (split * REC + ((i * FN + j) * kThreads + tid) * 4) * 4, 0, 16 /*sc1*/);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  volatile int* flag = reinterpret_cast<volatile int*>(smem);
  if (tid == 0) {
    const int t =
        __hip_atomic_fetch_add(P.tickets + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = t == P.splits - 1;
    if (last) __hip_atomic_store(P.tickets + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    flag[0] = last;
  }
  __syncthreads();
  if (!flag[0]) return false;
  for (int s = 0; s < P.splits; ++s) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const f32x4 t = __builtin_bit_cast(
            f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                       rr, (s * REC + ((i * FN + j) * kThreads + tid) * 4) * 4, 0, 16));
        acc[i][j] = s == 0 ? t : acc[i][j] + t;
      }
  }
  return true;
}

template <typename T, int BM, int BN, bool TRANS_A, bool ALIGNED>
__device__ __forceinline__ void group_tile(const GroupProb& P, typename Op16<T>::vec* lds,
                                           int local) {
  const BwdArgs& p = P.a;
  const float lr = dlrm_resolve_lr(p.lr_dev, p.lr);
  const int split = local / p.tiles, orig = local % p.tiles;
  f32x4 acc[BM / 32][BN / 32];
  int64_t i0, j0;
  bwd_tile_acc<T, BM, BN, TRANS_A, ALIGNED>(p, lds, orig, split, acc, i0, j0);
  // `orig` names the tile as well as its remapped index does: one ticket, one record run
  if (P.splits > 1 && !split_fold<BM, BN>(P, orig, split, acc, lds)) return;
  bwd_tile_store<BM, BN>(p, p.epi, lr, acc, i0, j0, static_cast<float*>(p.Out), p.ldo);
}

template <typename T, int BM, int BN>
__device__ __forceinline__ void group_body(const GroupProb& P, typename Op16<T>::vec* lds,
                                           int local) {
  if (P.trans_a) {
    if (P.aligned)
      group_tile<T, BM, BN, true, true>(P, lds, local);
    else
      group_tile<T, BM, BN, true, false>(P, lds, local);
  } else {
    if (P.aligned)
      group_tile<T, BM, BN, false, true>(P, lds, local);
    else
      group_tile<T, BM, BN, false, false>(P, lds, local);
  }
}

template <typename T, int CLS>
__global__ __launch_bounds__(kThreads) void linear16_group_kernel(const GroupArgs g) {
  using vec = typename Op16<T>::vec;
  __shared__ vec lds[2 * (kTiles[CLS].bm + kTiles[CLS].bn) * 8];
  const int b = blockIdx.x;
  // the workgroup's problem, picked with static indices only: a dynamic index into the
  // kernel arguments would copy them to scratch
  GroupProb P = g.p[0];
#pragma unroll
  for (int i = 1; i < kMaxGroup; ++i)
    if (i < g.n && b >= g.p[i].block0) P = g.p[i];
  const int local = b - P.block0;
#define DLRM_L16G_CASE(IDX)                                                  \
  if constexpr (IDX >= CLS) {                                                \
    if (P.tile == IDX) {                                                     \
      group_body<T, kTiles[IDX].bm, kTiles[IDX].bn>(P, lds, local);          \
      return;                                                                \
    }                                                                        \
  }
  DLRM_L16G_CASE(0)
  DLRM_L16G_CASE(1)
  DLRM_L16G_CASE(2)
  DLRM_L16G_CASE(3)
#undef DLRM_L16G_CASE
}

template <typename T>
void launch_group(int cls, const GroupArgs& g, int blocks, hipStream_t s) {
  const dim3 grid(blocks), block(kThreads);
  switch (cls) {
    case 0: hipLaunchKernelGGL((linear16_group_kernel<T, 0>), grid, block, 0, s, g); break;
    case 1: hipLaunchKernelGGL((linear16_group_kernel<T, 1>), grid, block, 0, s, g); break;
    case 2: hipLaunchKernelGGL((linear16_group_kernel<T, 2>), grid, block, 0, s, g); break;
    default: hipLaunchKernelGGL((linear16_group_kernel<T, 3>), grid, block, 0, s, g); break;
  }
}

int tile_index(Tile t) {
  for (int i = 0; i < kNumTiles; ++i)
    if (kTiles[i].bm == t.bm && kTiles[i].bn == t.bn) return i;
  return -1;
}

// The checks and the plan of one problem: the stand-alone dlrm_linear16_dgrad / _wgrad call's.
// gp->tile < 0: nothing to do for this problem.
int plan_problem(const dlrm_linear16_bwd_problem& q, int idx, GroupProb* gp) {
  *gp = GroupProb{};
  gp->tile = -1;
  const int64_t M = q.M, N = q.N, K = q.K;
  DLRM_ARG(q.kind == DLRM_BWD16_DGRAD || q.kind == DLRM_BWD16_WGRAD,
           "dlrm_linear16_bwd_group: problem %d: unknown kind %d", idx, (int)q.kind);
  DLRM_ARG(M >= 0 && N >= 0 && K >= 0, "dlrm_linear16_bwd_group: problem %d: negative size", idx);
  BwdArgs& a = gp->a;
  Tile t;
  if (q.kind == DLRM_BWD16_DGRAD) {
    if (M == 0 || K == 0) return DLRM_OK;
    DLRM_ARG(q.out && (N == 0 || (q.dY && q.B)),
             "dlrm_linear16_bwd_group: problem %d: null pointer", idx);
    DLRM_REQUIRE(q.lddy >= N && q.ldb >= K && q.ldout >= K && (!q.mask || q.ldmask >= K),
                 DLRM_ERR_SHAPE,
                 "dlrm_linear16_bwd_group: problem %d (dgrad): lddy %lld < N %lld or ldb %lld / "
                 "ldout %lld / ldmask %lld < K %lld",
                 idx, (long long)q.lddy, (long long)N, (long long)q.ldb, (long long)q.ldout,
                 (long long)q.ldmask, (long long)K);
    const int64_t forced = tuning(DLRM_TUNE_LINEAR16_DGRAD_TILE);
    t = Tile{int(forced / 1000), int(forced % 1000)};
    DLRM_ARG(forced == 0 || known_tile(t),
             "dlrm_linear16_bwd_group: DLRM_TUNE_LINEAR16_DGRAD_TILE %lld is not a tile",
             (long long)forced);
    DLRM_REQUIRE(ceil_div(M, 32) * ceil_div(K, 64) <= INT32_MAX, DLRM_ERR_UNSUPPORTED,
                 "dlrm_linear16_bwd_group: problem %d: more than 2^31 - 1 tiles", idx);
    if (forced == 0) t = plan_dgrad(M, K, device_cus());
    a.I = M, a.J = K, a.R = N;
    a.mask = q.mask, a.ldmask = q.ldmask;
    a.epi = kEpiDgrad, a.lr = 0.f, a.lr_dev = nullptr;
    a.steps_per_split = ceil_div(N, kBK);
    gp->splits = 1, gp->trans_a = 0;
  } else {
    DLRM_ARG(q.mode == DLRM_WGRAD16_STORE || q.mode == DLRM_WGRAD16_SGD,
             "dlrm_linear16_bwd_group: problem %d: unknown mode %d", idx, (int)q.mode);
    DLRM_ARG(q.mode == DLRM_WGRAD16_SGD || !q.lr_dev,
             "dlrm_linear16_bwd_group: problem %d: lr_dev with a mode other than SGD", idx);
    if (N == 0 || K == 0) return DLRM_OK;
    if (M == 0 && q.mode == DLRM_WGRAD16_SGD) return DLRM_OK;  // C - fl(lr * 0): C stays
    DLRM_ARG(q.out && (M == 0 || (q.dY && q.B)),
             "dlrm_linear16_bwd_group: problem %d: null pointer", idx);
    DLRM_REQUIRE(q.lddy >= N && q.ldb >= K && q.ldout >= K, DLRM_ERR_SHAPE,
                 "dlrm_linear16_bwd_group: problem %d (wgrad): lddy %lld < N %lld or ldb %lld / "
                 "ldout %lld < K %lld",
                 idx, (long long)q.lddy, (long long)N, (long long)q.ldb, (long long)q.ldout,
                 (long long)K);
    DLRM_REQUIRE(ceil_div(N, 32) * ceil_div(K, 64) <= INT32_MAX, DLRM_ERR_UNSUPPORTED,
                 "dlrm_linear16_bwd_group: problem %d: more than 2^31 - 1 tiles", idx);
    WgradPlan w;
    DLRM_ARG(wgrad_plan_checked(M, N, K, &w),
             "dlrm_linear16_bwd_group: DLRM_TUNE_LINEAR16_WGRAD_TILE %lld is not a tile",
             (long long)tuning(DLRM_TUNE_LINEAR16_WGRAD_TILE));
    t = w.tile;
    a.I = N, a.J = K, a.R = M;
    a.mask = nullptr, a.ldmask = 0;
    a.epi = q.mode == DLRM_WGRAD16_SGD ? kEpiSgd : kEpiStore;
    a.lr = q.lr, a.lr_dev = q.lr_dev;
    a.steps_per_split = w.steps;
    gp->splits = w.splits, gp->trans_a = 1;
  }
  a.A = q.dY, a.lda = q.lddy, a.B = q.B, a.ldb = q.ldb;
  a.Out = q.out, a.ldo = q.ldout;
  a.tiles_j = int(ceil_div(a.J, t.bn));
  a.tiles = int(ceil_div(a.I, t.bm)) * a.tiles_j;
  gp->aligned = aligned16(q.dY, q.lddy, q.B, q.ldb);
  gp->tile = tile_index(t);
  DLRM_REQUIRE(gp->tile >= 0, DLRM_ERR_UNSUPPORTED,
               "dlrm_linear16_bwd_group: problem %d: no kernel for the tile", idx);
  return DLRM_OK;
}

struct GroupPlan {
  GroupArgs g{};
  int64_t blocks = 0;
  int cls = kNumTiles;
  size_t bytes = 0;  // of the workspace; 0: no problem is split
};

// Plans every problem and carves the workspace (ws may be NULL: sizes only).
int plan_group(int32_t type, int32_t n, const dlrm_linear16_bwd_problem* problems, void* ws,
               GroupPlan* out) {
  DLRM_ARG(type == DLRM_MLP16_BF16 || type == DLRM_MLP16_F16,
           "dlrm_linear16_bwd_group: unknown type %d", (int)type);
  DLRM_ARG(n >= 1 && n <= kMaxGroup, "dlrm_linear16_bwd_group: %d problems (1 .. %d)", (int)n,
           kMaxGroup);
  DLRM_ARG(problems, "dlrm_linear16_bwd_group: null problems");
  WsCarver carve(ws);
  int* tickets = carve.take<int>(kGroupTickets);
  int64_t used_tickets = 0;
  GroupPlan& pl = *out;
  for (int i = 0; i < n; ++i) {
    GroupProb gp;
    const int rc = plan_problem(problems[i], i, &gp);
    if (rc != DLRM_OK) return rc;
    if (gp.tile < 0) continue;
    gp.block0 = int(pl.blocks);
    pl.blocks += int64_t(gp.a.tiles) * gp.splits;
    DLRM_REQUIRE(pl.blocks <= INT32_MAX, DLRM_ERR_UNSUPPORTED,
                 "dlrm_linear16_bwd_group: more than 2^31 - 1 workgroups");
    if (gp.splits > 1) {
      DLRM_REQUIRE(used_tickets + gp.a.tiles <= kGroupTickets, DLRM_ERR_UNSUPPORTED,
                   "dlrm_linear16_bwd_group: more than %d split tiles in one launch",
                   kGroupTickets);
      gp.tickets = tickets ? tickets + used_tickets : nullptr;
      used_tickets += gp.a.tiles;
      const Tile t = kTiles[gp.tile];
      gp.records = carve.take<float>(size_t(gp.a.tiles) * gp.splits * t.bm * t.bn);
    }
    pl.cls = gp.tile < pl.cls ? gp.tile : pl.cls;
    pl.g.p[pl.g.n++] = gp;
  }
  pl.bytes = used_tickets > 0 ? carve.used : 0;
  return DLRM_OK;
}

}  // namespace
}  // namespace dlrm

extern "C" size_t dlrm_linear16_bwd_group_workspace_size(
    int32_t type, int32_t n, const dlrm_linear16_bwd_problem* problems) {
  dlrm::GroupPlan pl;
  return dlrm::plan_group(type, n, problems, nullptr, &pl) == DLRM_OK ? pl.bytes : 0;
}

extern "C" int dlrm_linear16_bwd_group(int32_t type, int32_t n,
                                       const dlrm_linear16_bwd_problem* problems,
                                       void* workspace, size_t workspace_bytes,
                                       dlrm_stream_t stream) {
  using namespace dlrm;
  GroupPlan pl;
  const int rc = plan_group(type, n, problems, workspace, &pl);
  if (rc != DLRM_OK) return rc;
  DLRM_REQUIRE(pl.bytes == 0 || (workspace && workspace_bytes >= pl.bytes), DLRM_ERR_WORKSPACE,
               "dlrm_linear16_bwd_group: workspace of %zu bytes, %zu needed", workspace_bytes,
               pl.bytes);
  DLRM_ARG(pl.bytes == 0 || reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
           "dlrm_linear16_bwd_group: workspace not 16-byte aligned");
  if (pl.g.n == 0) return DLRM_OK;
  if (type == DLRM_MLP16_BF16)
    launch_group<__bf16>(pl.cls, pl.g, int(pl.blocks), as_stream(stream));
  else
    launch_group<_Float16>(pl.cls, pl.g, int(pl.blocks), as_stream(stream));
  DLRM_LAUNCH_CHECK("dlrm_linear16_bwd_group");
  return DLRM_OK;
}
