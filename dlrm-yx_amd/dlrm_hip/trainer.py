"""Fused DLRM training step on MI355X: every FLOP and byte of the step goes through the
HIP kernels of libdlrm_hip.so; torch provides device memory, streams and RCCL.

One step = the reference iteration (dlrm_s_pytorch.py:1886-1934): forward
(sequential_forward :732-770 or distributed_forward :686-730), loss, backward and the
optimizer update.  Layout decisions (MI355X-first):

* All local embedding tables live row-concatenated in ONE [sum rows, D] fp32 buffer with
  64-bit row bases (C3 = 54 M rows x 128 = 27.7 GB, resident in HBM); the batch is the
  reference's table-batched CSR (int32 offsets [T*B+1], int32 indices).
* All MLP parameters live in ONE flat fp32 bucket (bottom then top, W then b per layer)
  so the data-parallel gradient is one RCCL all-reduce and the dense update one kernel.
  Every layer's input width is padded to a multiple of 4 floats (zero columns in both
  the activation and the weight) so every GEMM operand row is 16-B aligned.
* Single GPU: the optimizer is fused into the backward — wgrad GEMMs run with the SGD
  epilogue (W -= lr * dY^T X after dX = dY W has consumed the old W), bias columns sums
  apply their update, the embedding backward applies exact SGD per unique row.
* Multi GPU (one process per GPU, RCCL over xGMI): tables are sharded table-wise with the
  reference sharders; pooled embeddings go through one all_to_all_single per direction
  (rank-major feature order, the W x embedding gradient of the reference is reproduced);
  the bottom MLP overlaps the forward exchange, the backward exchange overlaps the bottom
  MLP backward, and the dense all-reduce overlaps the embedding update.
* Mixed precision on request (TrainerConfig.mlp_precision = "bf16"): the MLP layers below the
  head run forward, data gradient and weight gradient on the bf16 MFMA from the same fp32
  buffers (the 16-bit closures of DLRMTrainer._build); everything above stays as described.
* fp16 tables on request (TrainerConfig.emb_precision = "fp16", one GPU, SGD): the row buffer
  is [sum rows, D] half (C3: 13.9 GB); the gather-fused interaction and the pooled lookup
  widen a row as they load it, the update rounds the new row to nearest even as it stores it
  (an update below half an fp16 ulp of the weight vanishes) or, with emb_rounding =
  "stochastic", up or down at random in proportion (a device (seed, step) stream, ticked
  behind the update), and runs as launches of its own; everything else stays fp32.
* Learning-rate schedule on request (TrainerConfig.lr_num_warmup_steps / lr_decay_start_step /
  lr_num_decay_steps, or device_lr): the step's rates live in device memory, a one-thread
  kernel at the head of the step advances the reference's LRPolicyScheduler and every update
  kernel reads its rate when it runs, so a captured step walks the schedule on replay.  With
  the defaults the rates are host floats and the step is unchanged.
* int8 / int4 tables for inference on request (quantize_embedding(bits), then emb_bits=bits on
  predict / capture_predict / evaluate; one GPU, plain tables): a row-wise quantized snapshot
  of the tables packed on the device (C3: 7.4 / 3.7 GB), read by the gather-fused interaction
  or the pooled Q8 / Q4 lookup; the masters stay and the training step never reads it.
* int8 MLP layers for inference on request (quantize_mlp(8), then mlp_bits=8 on predict /
  capture_predict / evaluate; one GPU): a per-tensor int8 snapshot of every MLP layer, each
  run as a range launch plus a dynamically quantized Linear on the i8 MFMA, bitwise torch's
  quantize_dynamic; slower than the fp32 and bf16 predicts at C3.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch.autograd.profiler import record_function

from . import ops
from .optim import check_lr_policy
from .sharders import shard


PRECISIONS = ("fp32", "bf16", "fp16")  # predict / evaluate: the MLP operands' precision


def _pad4(n: int) -> int:
    return (int(n) + 3) // 4 * 4


def _precision(precision: str) -> str:
    if precision not in PRECISIONS:
        raise ValueError(f"precision {precision!r}: one of {PRECISIONS}")
    return precision


@dataclass
class TrainerConfig:
    m_spa: int
    ln_emb: Sequence[int]
    ln_bot: Sequence[int]
    ln_top: Sequence[int]          # full top widths (first = number of interactions)
    arch_interaction_op: str = "dot"
    arch_interaction_itself: bool = False
    loss_function: str = "mse"     # mse | bce
    loss_threshold: float = 0.0
    learning_rate: float = 0.01
    emb_learning_rate: Optional[float] = None  # default: learning_rate
    # sgd | rwsadagrad | adagrad (torch.optim.Adagrad, the reference's --optimizer adagrad:
    # one accumulator per weight, the tables' in a second [rows, D] fp32 buffer)
    optimizer: str = "sgd"
    adagrad_eps: float = 1e-10
    sharder: str = "greedy"
    allocation: Optional[Sequence[int]] = None
    # QR compositional embeddings (--qr-flag, dlrm_s_pytorch.py:282-290): tables with more
    # than qr_threshold rows become a quotient table (ceil(n/c) rows) and a remainder table
    # (c rows) combined by qr_operation (mult | add)
    qr_flag: bool = False
    qr_collisions: int = 4
    qr_operation: str = "mult"
    qr_threshold: int = 200
    # operands of the MLP GEMMs below the head: "fp32", or "bf16" = mixed precision - every
    # such Linear's forward, data gradient and weight gradient on the 16-bit MFMA with
    # operands rounded in flight from the fp32 tensors, fp32 accumulation, fp32 master
    # weights and fp32 everything else (DLRMTrainer._build).  "fp16" would need loss
    # scaling for the gradients: not implemented
    mlp_precision: str = "fp32"
    # the reference's LRPolicyScheduler (--lr-num-warmup-steps, --lr-decay-start-step,
    # --lr-num-decay-steps; optim.lr_policy): linear warm-up, plateau, polynomial-2 decay,
    # applied to learning_rate and emb_learning_rate alike.  Any of them non-zero, or
    # device_lr, keeps the step's learning rates in device memory (lr_mode "device"): a
    # one-thread kernel at the head of the step advances the schedule and every update
    # kernel reads its rate from that memory, so a captured step walks the schedule on
    # replay and DLRMTrainer.set_learning_rate reaches graphs that are already captured.
    # All at their defaults (lr_mode "host"): the rates are host floats baked into the
    # launches, exactly the step of before
    lr_num_warmup_steps: int = 0
    lr_decay_start_step: int = 0
    lr_num_decay_steps: int = 0
    device_lr: bool = False
    # the embedding tables' storage: "fp32", or "fp16" = the row buffer held as [rows, D]
    # half (the reference's --fbgemm-emb tables: FP16 weights with EXACT_SGD,
    # dlrm_s_pytorch.py:337-366).  A row is widened to fp32 as it is loaded and the updated
    # row is rounded to nearest even as it is stored; pooled embeddings, interaction,
    # gradients and dense parameters stay fp32 (DESIGN.md §18 has the limits: SGD only, no
    # QR tables, one GPU, D % 4 == 0 and D <= 512)
    emb_precision: str = "fp32"
    # how the fp16 tables' updated row is stored: "nearest" (round to nearest even: an update
    # below half an fp16 ulp of the weight vanishes), or "stochastic" = fbgemm's
    # stochastic_rounding=True, its default and so the reference's run: the fp32 value is
    # rounded up or down with the probability of its position between the two fp16
    # neighbours, drawn from a counter-based stream of (emb_rounding_seed, step, row, column)
    # (DESIGN.md §19).  The step count lives on the device and a one-thread kernel after the
    # update advances it, so a captured step draws a fresh stream on every replay;
    # DLRMTrainer.rounding_state() / set_rounding_state() read and set it for a resume
    emb_rounding: str = "nearest"
    emb_rounding_seed: int = 0

    @property
    def lr_policy_steps(self):
        return (int(self.lr_num_warmup_steps), int(self.lr_decay_start_step),
                int(self.lr_num_decay_steps))

    @property
    def lr_mode(self) -> str:
        """"device": learning rates in device memory (a policy, or device_lr); else "host"."""
        return "device" if self.device_lr or any(self.lr_policy_steps) else "host"

    def __post_init__(self):
        if any(self.lr_policy_steps):
            check_lr_policy(*self.lr_policy_steps)
        if self.mlp_precision == "fp16":
            raise NotImplementedError("mlp_precision='fp16': fp16 gradients need loss scaling "
                                      "(predict(..., precision='fp16') is available)")
        if self.mlp_precision not in ("fp32", "bf16"):
            raise ValueError(f"mlp_precision {self.mlp_precision!r}: 'fp32' or 'bf16'")
        if self.emb_precision not in ("fp32", "fp16"):
            raise ValueError(f"emb_precision {self.emb_precision!r}: 'fp32' or 'fp16'")
        if self.emb_rounding not in ("nearest", "stochastic"):
            raise ValueError(f"emb_rounding {self.emb_rounding!r}: 'nearest' or 'stochastic'")
        if self.emb_rounding == "stochastic" and self.emb_precision != "fp16":
            raise ValueError("emb_rounding='stochastic' rounds the fp16 tables' update: it "
                             "needs emb_precision='fp16'")
        if self.emb_precision == "fp16":
            if self.optimizer == "adagrad":
                raise NotImplementedError(
                    "emb_precision='fp16' with optimizer='adagrad': the element-wise Adagrad "
                    "update takes fp32 tables and an fp32 accumulator (DESIGN.md §22)")
            if self.optimizer == "rwsadagrad":
                raise NotImplementedError(
                    "emb_precision='fp16' with optimizer='rwsadagrad': there is no fp16 "
                    "row-wise Adagrad kernel (the reference's fp16 tables are EXACT_SGD only; "
                    "DESIGN.md §18)")
            if self.qr_flag:
                raise NotImplementedError(
                    "emb_precision='fp16' with qr_flag: the QR combine runs on fp32 tables "
                    "only (DESIGN.md §18)")
            if int(self.m_spa) % 4 or int(self.m_spa) > 512:
                raise NotImplementedError(
                    f"emb_precision='fp16' with m_spa={self.m_spa}: the fp16 lookup takes D a "
                    "multiple of 4 and at most 512 (dlrm_tbe_forward_rows; DESIGN.md §18)")


@dataclass
class Batch:
    X: torch.Tensor        # [B_local, Kp0] dense input (padded, zero pad columns)
    offsets: torch.Tensor  # [T_local*B + 1] int32 CSR of the local tables, full batch
    indices: torch.Tensor  # int32 table-local rows
    target: torch.Tensor   # [B_local] fp32
    max_per_table: int = 0  # upper bound on one table's lookups (0 = unknown)
    one_hot: bool = False   # every bag holds exactly one index (offsets = arange)


@dataclass
class _Layer:
    N: int
    K: int
    Kp: int
    Np: int
    W: torch.Tensor
    b: torch.Tensor
    gW: Optional[torch.Tensor] = None
    gb: Optional[torch.Tensor] = None
    sumW: Optional[torch.Tensor] = None  # Adagrad state views
    sumb: Optional[torch.Tensor] = None


@dataclass
class _Layer8:
    """quantize_mlp's snapshot of one layer."""
    packed: Optional["ops.Linear8Weights"]  # int8 weights + their scale
    bias: torch.Tensor  # [N] fp32 copy
    rng: torch.Tensor   # the min / max partials of this layer's input, rewritten by every call


class DLRMTrainer:
    def __init__(self, cfg: TrainerConfig, device="cuda:0", rank: int = 0, world_size: int = 1,
                 process_group=None, seed: int = 0, init: bool = True, comm=None,
                 force_dist: bool = False):
        """``comm``: the step's collectives (default: TorchComm over ``process_group``, the
        dense all-reduce on a second group of the same ranks); EmulatedComm runs rank
        ``rank`` of ``world_size`` alone on one GPU (bench --emulate-world).
        ``force_dist``: the multi-GPU schedule (all-to-all, gradient bucket, all-reduce)
        even at world_size 1, on a 1-rank group (its tests run RCCL on one GPU)."""
        self.cfg = cfg
        self.emb_f16 = cfg.emb_precision == "fp16"
        if self.emb_f16 and (world_size > 1 or force_dist):
            raise NotImplementedError(
                "emb_precision='fp16' on the multi-GPU schedule: the fp16 tables run on one "
                "GPU only (DESIGN.md §18)")
        self.dev = torch.device(device)
        self.rank, self.world = rank, world_size
        self.pg = process_group
        self.distributed = world_size > 1 or bool(force_dist)
        if self.distributed and comm is None:
            if process_group is None:
                raise ValueError("the multi-GPU schedule needs a process group (or a comm)")
            comm = TorchComm(process_group)
        self.comm = comm
        D = int(cfg.m_spa)
        if int(cfg.ln_bot[-1]) != D:
            raise ValueError("trainer needs ln_bot[-1] == m_spa (the reference splits wider "
                             "tables into D-sized features; not on this path)")
        if D % 4:
            raise ValueError("trainer needs the embedding dim to be a multiple of 4")
        self.D = D
        T = len(cfg.ln_emb)
        self.T = T
        if world_size > 1:
            if T < world_size:
                raise ValueError(f"only {T} tables for {world_size} ranks")
            di = list(cfg.allocation) if cfg.allocation is not None else \
                shard(list(cfg.ln_emb), world_size, cfg.sharder)
        else:
            di = [0] * T
        self.device_indices = di
        self.local_tables = [t for t in range(T) if di[t] == rank]
        self.tables_per_rank = [sum(1 for t in range(T) if di[t] == r) for r in range(world_size)]
        # rank-major global feature order after the all-to-all (extend_distributed.py:475-487)
        self.feature_order = [t for r in range(world_size) for t in range(T) if di[t] == r]
        self.T_local = len(self.local_tables)
        rows = [int(cfg.ln_emb[t]) for t in self.local_tables]
        self.rows_local = rows
        # physical tables: the local tables, with every QR table split into its quotient and
        # remainder tables (the lookup runs on the physical CSR, a combine kernel forms the
        # logical features; the a2a / interaction see logical tables only)
        self.qr = bool(cfg.qr_flag)
        if self.qr and cfg.qr_operation not in ("mult", "add"):
            raise NotImplementedError("trainer QR: qr_operation mult or add (concat widens "
                                      "the feature; the module path DLRM_Net has it)")
        prow, psrc, pkind, pcoll, pq, pr = [], [], [], [], [], []
        for j, n in enumerate(rows):
            if self.qr and n > cfg.qr_threshold:
                c = int(cfg.qr_collisions)
                pq.append(len(prow))
                prow.append(int(math.ceil(n / c)))
                psrc.append(j), pkind.append(1), pcoll.append(c)
                pr.append(len(prow))
                prow.append(c)
                psrc.append(j), pkind.append(2), pcoll.append(c)
            else:
                pq.append(len(prow))
                pr.append(-1)
                prow.append(n)
                psrc.append(j), pkind.append(0), pcoll.append(1)
        self.phys_rows, self.phys_src, self.phys_kind = prow, psrc, pkind
        self.T_phys = len(prow)
        self.qr_active = self.T_phys != self.T_local
        i32 = dict(dtype=torch.int32, device=self.dev)
        self._qr_src = torch.tensor(psrc, **i32)
        self._qr_kind = torch.tensor(pkind, **i32)
        self._qr_coll = torch.tensor(pcoll, **i32)
        self._qr_pq = torch.tensor(pq, **i32)
        self._qr_pr = torch.tensor(pr, **i32)
        self._qr_csr = {}
        rows = prow
        # row bases of the physical tables: the host copy serves _rows without a device sync
        self._row_bases = [0] + np.cumsum(rows).tolist()
        self.row_base = torch.tensor(self._row_bases, dtype=torch.int64, device=self.dev)
        self.total_rows = int(sum(rows))
        ops.check_tbe_rows(self.total_rows, "DLRMTrainer (this rank's tables)")
        self.weights = torch.empty((max(self.total_rows, 1), D),
                                   dtype=torch.float16 if self.emb_f16 else torch.float32,
                                   device=self.dev)
        # row-wise quantized snapshots of the tables for predict(emb_bits=8 | 4), one buffer per
        # width, filled by quantize_embedding; the training step never reads them
        self._qrows = {}
        # the int8 snapshot of the MLP layers for predict(mlp_bits=8), filled by quantize_mlp
        # (DESIGN.md §21): id(layer) -> _Layer8; the training step never reads it
        self._mlp8 = None
        self.momentum = None
        self.emb_sum = None
        if cfg.optimizer == "rwsadagrad":
            self.momentum = torch.zeros(max(self.total_rows, 1), dtype=torch.float32,
                                        device=self.dev)
        elif cfg.optimizer == "adagrad":
            # torch.optim.Adagrad's state['sum'] of the tables: one accumulator per weight
            self.emb_sum = torch.zeros((max(self.total_rows, 1), D), dtype=torch.float32,
                                       device=self.dev)
        elif cfg.optimizer != "sgd":
            raise ValueError(f"optimizer {cfg.optimizer!r} not supported")
        # ---- dense parameters: one flat bucket
        ln_bot, ln_top = [int(v) for v in cfg.ln_bot], [int(v) for v in cfg.ln_top]
        if ln_top[-1] != 1:
            raise ValueError("the fused head needs a single output (ln_top[-1] == 1)")
        F = T + 1
        if cfg.arch_interaction_op == "dot":
            npairs = F * (F + 1) // 2 if cfg.arch_interaction_itself else F * (F - 1) // 2
            self.num_int = D + npairs
        else:
            self.num_int = F * D
        if ln_top[0] != self.num_int:
            raise ValueError(f"ln_top[0]={ln_top[0]} != number of interactions {self.num_int}")
        specs = [(ln_bot[i + 1], ln_bot[i]) for i in range(len(ln_bot) - 1)] + \
                [(ln_top[i + 1], ln_top[i]) for i in range(len(ln_top) - 1)]
        # Bias folding: layer l stores [W | b | 0-pad] as one [N, Kp] block with
        # Kp = pad4(K + 1); every layer input carries a constant-1 column at index K, so
        # the forward GEMM adds the bias as its last k-term and the wgrad GEMM yields db.
        sizes = [n * _pad4(k + 1) for n, k in specs]
        self.n_params = int(sum(sizes))
        self.params = torch.zeros(self.n_params, dtype=torch.float32, device=self.dev)
        # (both Adagrad modes: gradient bucket + dense Adagrad over it)
        dense_adagrad = cfg.optimizer in ("rwsadagrad", "adagrad")
        self.grads = torch.zeros_like(self.params) if (self.distributed or
                                                      dense_adagrad) else None
        self.adagrad_sum = torch.zeros_like(self.params) if dense_adagrad else None
        self.layers: List[_Layer] = []
        o = 0
        for n, k in specs:
            kp = _pad4(k + 1)
            W = self.params[o:o + n * kp].view(n, kp)
            L = _Layer(N=n, K=k, Kp=kp, Np=_pad4(n + 1), W=W, b=W[:, k])
            if self.grads is not None:
                L.gW = self.grads[o:o + n * kp].view(n, kp)
                L.gb = L.gW[:, k]
            o += n * kp
            self.layers.append(L)
        self.n_bot = len(ln_bot) - 1
        # DDP buckets of the flat gradient (bottom layers first): the top MLP's gradients
        # are complete after the top backward, the bottom's after the bottom backward
        self.n_bot_params = int(sum(sizes[:self.n_bot]))
        self.bot = self.layers[:self.n_bot]
        self.top = self.layers[self.n_bot:]
        self._bufs = {}
        # independent kernels of a step run on a side stream (see step())
        self.concurrent = True
        # which overlaps to use (attribute, A/B only): "fwd" (bottom MLP || lookup),
        # "bot" (bottom-MLP backward || embedding backward).  Off by default: measured on
        # MI355X, each cross-queue dependency in a replayed hipGraph costs ~10 us, more than
        # the overlap recovers at C3 (profiles/r01_overlap_ab.txt).
        self.overlaps = set()
        self._side = torch.cuda.Stream(device=self.dev)
        self._tbe_ws: Optional[torch.Tensor] = None
        # run the embedding backward's per-table sort inside the lookup launch
        # (dlrm_tbe_forward_presort); False: the backward sorts itself
        self.tbe_presort = True
        # (cfg.mlp_precision == "bf16", _build: a Linear is three 16-bit launches in
        # stream order and no launch role exists, so group_wgrad, full_last_wgrad, bot_sched,
        # fuse_bottom, dist_bottom_in_lookup, tbe_role, head_role, tbe_role_at and overlaps
        # below have no effect in that mode; tbe_presort, early_sort, fuse_gather and
        # feature_pad keep theirs)
        # MLP backward: a layer's split wgrad (partials only) in the same launch as its dgrad
        self.group_wgrad = True
        self.full_last_wgrad = False
        # bottom-MLP backward schedule: "partial" (split wgrads reduced in the next launch),
        # "full" (in-launch split-K, n_bot launches; bottom_bwd_full) or "auto": full at
        # <= 128 rows per GPU, else partial (measured, one MI355X: full 0.976 vs partial
        # 0.857 M samples/s at the Kaggle shape, B = 128; partial ahead at C3 B = 2048, 4.67
        # vs 4.54 M, and at B = 256, 1.21 vs 1.19 M; profiles/r04_bot_sched_ab.txt.  A third
        # schedule - the data gradients as one row-block launch - lost at every shape and
        # was removed in ABI v8)
        self.bot_sched = "auto"
        # one GPU: the bottom MLP forward as a role of the lookup launch (mlp_rows.hpp)
        self.fuse_bottom = True
        # several GPUs: the bottom MLP forward as a role of the lookup launch too (True), or
        # as its own chain launch beside the in-flight all-to-all (False).  The emulated
        # W = 8 rank 2 step: 16.3 us of chain launch -> a few us inside the lookup launch;
        # the cost is the all-to-all starting after the (longer) fused launch
        self.dist_bottom_in_lookup = True
        # one GPU, tables past the per-table LDS sort (C1's L = 100): the backward's tiled
        # sort (dlrm_tbe_backward_sort) on the side stream at the start of the step, beside
        # the forward, joined before the embedding backward.  The one cross-queue join of
        # the graph costs ~11 us of idle GPU; the 6 sort launches (~69 us) hide behind the
        # forward: C1 step 0.588 -> 0.572 ms (profiles/r06_early_sort_ab.txt).  2 = forked
        # after the lookup launch instead: ~5 % slower (profiles/r06_early_sort_fork_ab.txt)
        self.early_sort = True
        # one GPU: the pooled embeddings E and their gradient dE with a batch stride of an odd
        # number of 256-byte chunks.  The embedding update reads dE[b, t] in sorted-row order
        # (random b) and each XCD works through one table's lookups: at a stride of 8 chunks
        # (C1: 8 x 64 floats) every such read lands in the same two of an XCD's L2 channels.
        # Measured: C1's update pass 105.7 -> 99.1 us, the step -0.3..-0.8 %, C3 / C2 within
        # noise (profiles/r06_feature_pad_ab.txt) - an option, off by default
        self.feature_pad = False
        # one GPU, one-hot batches: the dot interaction gathers the embedding rows itself
        # (dlrm_interact_dot_forward_gather); the lookup launch keeps only its sort role
        self.fuse_gather = True
        # one GPU: the embedding update's passes as extra workgroups of the bottom-MLP
        # backward's GEMM launches (dlrm_gemm_f32_group_role); False: launches of their own
        self.tbe_role = True
        # one GPU: the head's finalize pass as a role of the top-MLP backward's first launch
        self.head_role = True
        # bottom-MLP forward workgroups per 16-row block in the lookup launch (0 = auto)
        self.bottom_parts = 0
        self._cus = torch.cuda.get_device_properties(self.dev).multi_processor_count \
            if torch.cuda.is_available() else 256
        self.tbe_role_at = (0, 1)  # bottom-backward launches carrying pass 1 and pass 2
        self._roles = []  # pending (role, phase) passes for the step's next GEMM launches
        self.gather_fused = False  # set by the last step
        self.bottom_fused = False  # set by the last step
        # device TBE error bits (ops.TBE_ERR_*): out-of-range indices are skipped by the
        # kernels and flagged here; check_errors() reads it (the step never syncs)
        self.tbe_error_flag = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._head_step_ws: Optional[torch.Tensor] = None
        self._rec_off = {}  # batch size -> the decode's private CSR offsets (_rec_offsets)
        self._rec_scratch = None  # the full-batch decode scratch of record_batch
        self.step_count = 0
        # lr_mode "device": slot 0 the dense rate, 1 the embedding rate, 2 the dense rate / W
        # (the dense update of the W-rank schedule); None: host floats
        self._lr_state = None
        if cfg.lr_mode == "device":
            self._lr_state = ops.lr_state(
                [self.lr, self.emb_lr, self.lr], [1.0, 1.0, 1.0 / self.world],
                *cfg.lr_policy_steps, device=self.dev)
        # fp16 tables rounded stochastically: the device (seed, step) of the update's stream
        self._sr_state = None
        if self.emb_f16 and cfg.emb_rounding == "stochastic":
            self._sr_state = ops.sr_state(cfg.emb_rounding_seed, 0, device=self.dev)
        self.capture_mode = None  # "whole" | "segments": how the last capture() was built
        self.graphs_per_step = 0  # hipGraphs one replay of the last capture() launches
        if init:
            self.init_random(seed)

    # ---------------------------------------------------------------- init --
    def init_random(self, seed: int = 0):
        """Reference-distribution random init on device: tables U(+-sqrt(1/n))
        (dlrm_s_pytorch.py:304-308), W ~ N(0, sqrt(2/(m+n))), b ~ N(0, sqrt(1/m)) (:240-247)."""
        for p, j in enumerate(self.phys_src):
            t = self.local_tables[j]
            n = int(self.cfg.ln_emb[t])
            a = math.sqrt(1.0 / n)
            view = self.weights[self._rows(p)]
            if self.emb_f16:  # the fp32 init of the same seed, rounded to nearest once
                self._fill_f16(view, -a, a, seed * 1000003 + t)
            elif self.phys_kind[p] == 0:
                ops.uniform_fill_(view, -a, a, seed * 1000003 + t)
            else:  # QR tables: uniform [sqrt(1/n), 1] (tricks/qr_embedding_bag.py:153-154)
                ops.uniform_fill_(view, a, 1.0, seed * 1000003 + t + 7919 * self.phys_kind[p])
        g = torch.Generator(device=self.dev)
        g.manual_seed(seed + 12345)
        with torch.no_grad():
            for L in self.layers:
                L.W.zero_()
                L.W[:, :L.K].normal_(0.0, math.sqrt(2.0 / (L.N + L.K)), generator=g)
                L.b.normal_(0.0, math.sqrt(1.0 / L.N), generator=g)

    _F16_INIT_CHUNK = 1 << 24  # fp32 elements staged per launch pair (64 MB)

    def _fill_f16(self, view: torch.Tensor, lo: float, hi: float, seed: int) -> None:
        """``view`` (fp16, contiguous rows) = uniform_fill_(fp32 of the same shape).half(),
        staged through a bounded fp32 scratch: no second full-size buffer at any table size."""
        flat = view.view(-1)
        n = flat.numel()
        scratch = torch.empty(min(n, self._F16_INIT_CHUNK), dtype=torch.float32, device=self.dev)
        for o in range(0, n, self._F16_INIT_CHUNK):
            m = min(self._F16_INIT_CHUNK, n - o)
            ops.uniform_fill_at_(scratch[:m], lo, hi, seed, o)
            flat[o:o + m].copy_(scratch[:m])  # fp32 -> fp16: round to nearest even

    def load_dense(self, mlp_params: Sequence[tuple], tables: Optional[Sequence] = None):
        """Copy (W [N,K], b [N]) per layer (bottom then top) and optionally GLOBAL tables
        (emb_precision "fp16": each table rounded to nearest even once, by the copy)."""
        with torch.no_grad():
            for L, (W, b) in zip(self.layers, mlp_params):
                L.W.zero_()
                L.W[:, :L.K].copy_(torch.as_tensor(W))
                L.b.copy_(torch.as_tensor(b))
            if tables is not None:  # QR tables: (weight_q, weight_r) pairs
                for p, j in enumerate(self.phys_src):
                    t = self.local_tables[j]
                    src = tables[t]
                    if self.phys_kind[p] != 0:
                        src = src[self.phys_kind[p] - 1]
                    self.weights[self._rows(p)].copy_(torch.as_tensor(src))

    @classmethod
    def from_oracle(cls, cfg: TrainerConfig, ref, device="cuda:0", **kw):
        """Build with the exact weights of an oracle.OracleDLRM (test/smoke helper)."""
        tr = cls(cfg, device=device, init=False, **kw)
        mlp = []
        for seq in (ref.bot_l, ref.top_l):
            for m in seq:
                if isinstance(m, torch.nn.Linear):
                    mlp.append((m.weight.detach(), m.bias.detach()))
        tabs = [(e.weight_q.detach(), e.weight_r.detach()) if hasattr(e, "weight_q")
                else e.weight.detach() for e in ref.emb_l]
        tr.load_dense(mlp, tabs)
        return tr

    def dense_state(self):
        return [(L.W[:, :L.K].detach().clone(), L.b.detach().clone()) for L in self.layers]

    def _rows(self, p: int) -> slice:
        """Physical table p's rows in the concatenated buffers."""
        return slice(int(self._row_bases[p]), int(self._row_bases[p + 1]))

    def _table_views(self, buf: torch.Tensor, t: int):
        j = self.local_tables.index(t)
        views = [buf[self._rows(p)] for p, jj in enumerate(self.phys_src) if jj == j]
        return views[0] if len(views) == 1 else tuple(views)

    def table(self, t: int):
        """Local table t's weights (a (quotient, remainder) pair for a QR table)."""
        return self._table_views(self.weights, t)

    def table_momentum(self, t: int):
        """RWSAdagrad row-wise momentum of local table t (a (quotient, remainder) pair for a
        QR table), the reference's optimizer state['momentum'] (optim/rwsadagrad.py:80-84)."""
        if self.momentum is None:
            raise ValueError("no row-wise momentum: optimizer is not rwsadagrad")
        return self._table_views(self.momentum, t)

    def table_sum(self, t: int):
        """Element-wise Adagrad's accumulator of local table t, shaped like table(t) (a
        (quotient, remainder) pair for a QR table): torch.optim.Adagrad's state['sum']."""
        if self.emb_sum is None:
            raise ValueError("no element-wise Adagrad state: optimizer is not adagrad")
        return self._table_views(self.emb_sum, t)

    def dense_adagrad_state(self):
        """Per layer (sum of squared W gradients [N, K], of b [N]): the dense branch's
        state['sum'] of RWSAdagrad (optim/rwsadagrad.py:116-119) and of torch.optim.Adagrad."""
        if self.adagrad_sum is None:
            raise ValueError("no Adagrad state: optimizer is not rwsadagrad or adagrad")
        out, o = [], 0
        for L in self.layers:
            S = self.adagrad_sum[o:o + L.N * L.Kp].view(L.N, L.Kp)
            out.append((S[:, :L.K].detach().clone(), S[:, L.K].detach().clone()))
            o += L.N * L.Kp
        return out

    # ------------------------------------------------------------- batches --
    @property
    def lr(self) -> float:
        return float(self.cfg.learning_rate)

    @property
    def emb_lr(self) -> float:
        return float(self.cfg.emb_learning_rate if self.cfg.emb_learning_rate is not None
                     else self.cfg.learning_rate)

    def _rates(self):
        """(dense rate, embedding rate, dense rate / W) as the step's launches take them:
        host floats, or (lr_mode "device") the 1-element views of the device slots."""
        if self._lr_state is None:
            lr = self.lr
            return lr, self.emb_lr, lr * (1.0 / self.world)
        s = self._lr_state
        return s.lr(0), s.lr(1), s.lr(2)

    def set_learning_rate(self, lr: float, emb_lr: Optional[float] = None) -> None:
        """New base learning rates (``emb_lr`` None: the embedding rate keeps following
        ``lr`` if cfg.emb_learning_rate was never set, else stays).  lr_mode "device": the
        bases are copied into the device block on the current stream and the next step -
        eager, or a replay of an ALREADY CAPTURED graph - trains at them (through the policy,
        if one is set).  lr_mode "host": cfg is updated; the next eager step and the next
        capture() use it, graphs captured before keep the rate they were captured with."""
        self.cfg.learning_rate = float(lr)
        if emb_lr is not None:
            self.cfg.emb_learning_rate = float(emb_lr)
        if self._lr_state is not None:
            base = torch.tensor([self.lr, self.emb_lr, self.lr], dtype=torch.float64)
            self._lr_state.base.copy_(base)

    @property
    def lr_step(self) -> int:
        """The device schedule's step count (the reference scheduler's _step_count: 1 before
        the first step); synchronises.  Set it to resume a schedule."""
        if self._lr_state is None:
            raise RuntimeError("lr_step: no device learning-rate state (cfg.lr_mode is 'host')")
        return int(self._lr_state.step.item())

    @lr_step.setter
    def lr_step(self, value: int) -> None:
        if self._lr_state is None:
            raise RuntimeError("lr_step: no device learning-rate state (cfg.lr_mode is 'host')")
        self._lr_state.step.fill_(int(value))

    def current_lr(self) -> List[float]:
        """[dense rate, embedding rate, dense rate / W] as fp32 values: the rates the last
        step trained at (lr_mode "device": read from the device, synchronises; before the
        first step, base * multiplier) or the next one will (lr_mode "host")."""
        if self._lr_state is None:
            return [float(np.float32(v)) for v in self._rates()]
        return [float(v) for v in self._lr_state.rates.cpu()]

    def rounding_state(self):
        """(seed, step) of the fp16 tables' stochastic-rounding stream: the step the NEXT
        update draws from (0 before the first, +1 per training step, eager or replayed);
        synchronises.  With the parameters, enough to resume a run that reproduces it."""
        if self._sr_state is None:
            raise RuntimeError("rounding_state: cfg.emb_rounding is not 'stochastic'")
        return ops.sr_state_values(self._sr_state)

    def set_rounding_state(self, seed: int, step: int) -> None:
        """Set the stream's (seed, step), in place on the current stream: the next step -
        eager, or a replay of an already captured graph - draws from it."""
        if self._sr_state is None:
            raise RuntimeError("set_rounding_state: cfg.emb_rounding is not 'stochastic'")
        self._sr_state.copy_(ops.sr_state(seed, step, device=self.dev))

    def local_batch_size(self, B: int) -> int:
        if B % self.world:
            raise ValueError(f"batch {B} not divisible by {self.world} ranks "
                             "(dlrm_s_pytorch.py:139-143)")
        return B // self.world

    def make_batch(self, X, lS_o, lS_i, target) -> Batch:
        """From the reference's non-batched layout (X [B,m_den] GLOBAL batch, lS_o [T,B],
        lS_i list of T index tensors) -> this rank's device Batch."""
        B = X.shape[0]
        Bl = self.local_batch_size(B)
        sl = slice(self.rank * Bl, (self.rank + 1) * Bl)
        L0 = self.bot[0]
        Xp = torch.zeros((Bl, L0.Kp), dtype=torch.float32, device=self.dev)
        Xp[:, :L0.K] = torch.as_tensor(X)[sl].to(self.dev)
        Xp[:, L0.K] = 1.0  # bias column
        offs, idxs, start = [], [], 0
        for t in self.local_tables:
            o = torch.as_tensor(lS_o[t]).to(torch.int64)
            ii = torch.as_tensor(lS_i[t]).to(torch.int64)
            offs.append(o + start)
            idxs.append(ii)
            start += ii.numel()
        offsets = torch.cat(offs + [torch.tensor([start])]).to(torch.int32).to(self.dev)
        indices = (torch.cat(idxs) if idxs else torch.zeros(0, dtype=torch.int64)).to(
            torch.int32).to(self.dev)  # a rank may own no table
        tg = torch.as_tensor(target).reshape(-1)[sl].to(torch.float32).to(self.dev)
        mx = max([int(i.numel()) for i in idxs], default=0)
        one_hot = all(torch.equal(torch.as_tensor(lS_o[t]).to(torch.int64),
                                  torch.arange(Bl * self.world)) and
                      int(torch.as_tensor(lS_i[t]).numel()) == Bl * self.world
                      for t in self.local_tables)
        return Batch(Xp, offsets, indices, tg, mx, one_hot and bool(self.local_tables))

    def batch_from_records(self, records: torch.Tensor, max_ind_range: int = -1) -> Batch:
        """A Batch straight from raw Criteo binary records on the device (int32
        [B_global, 1+13+26], the CriteoBinDataset block, data_loader_terabyte.py:237-252):
        one dlrm_criteo_decode launch writes log(x+1) into the padded X (bias column kept),
        the table-major indices (% max_ind_range) and the L = 1 CSR.  Same batch as
        make_batch on the reference's transformed tensors."""
        L0 = self.bot[0]
        nf = 1 + L0.K + self.T
        if records.dim() != 2 or records.shape[1] != nf:
            raise ValueError(f"batch_from_records: records must be [B, {nf}] (1 + m_den + T)")
        B = records.shape[0]
        Bl = self.local_batch_size(B)
        rec = records.reshape(-1).to(device=self.dev, dtype=torch.int32).contiguous()
        dense = torch.empty((B, L0.Kp), dtype=torch.float32, device=self.dev)
        dense[:, L0.K:] = 0.0
        dense[:, L0.K] = 1.0  # bias column
        X, offsets, indices, label = ops.criteo_decode(rec, L0.K, self.T, max_ind_range,
                                                       batched=True, dense=dense)
        sl = slice(self.rank * Bl, (self.rank + 1) * Bl)
        if self.T_local != self.T:
            indices = indices.view(self.T, B)[self.local_tables].reshape(-1).contiguous()
            offsets = offsets[:self.T_local * B + 1].contiguous()
        return Batch(dense[sl].contiguous() if Bl != B else dense, offsets, indices,
                     label.reshape(-1)[sl].contiguous(), B, True)

    def record_batch(self, B: int) -> Batch:
        """Fixed device buffers for global batches of B Criteo records (L = 1), filled by
        ``decode_into`` (data.RecordPipeline): the tensors keep their addresses, so a step
        graph captured on this Batch replays on every decoded batch."""
        Bl = self.local_batch_size(B)
        L0 = self.bot[0]
        X = torch.zeros((Bl, L0.Kp), dtype=torch.float32, device=self.dev)
        X[:, L0.K] = 1.0  # bias column
        offsets = torch.arange(0, self.T_local * B + 1, dtype=torch.int32, device=self.dev)
        indices = torch.zeros(self.T_local * B, dtype=torch.int32, device=self.dev)
        target = torch.zeros(Bl, dtype=torch.float32, device=self.dev)
        if self.world > 1 or self.T_local != self.T:  # full-batch decode scratch
            full = torch.zeros((B, L0.Kp), dtype=torch.float32, device=self.dev)
            self._rec_scratch = dict(
                X=full, label=torch.empty(B, dtype=torch.float32, device=self.dev),
                indices=torch.empty(self.T * B, dtype=torch.int32, device=self.dev),
                offsets=torch.empty(self.T * B + 1, dtype=torch.int32, device=self.dev),
                tables=torch.tensor(self.local_tables, dtype=torch.int64, device=self.dev))
        return Batch(X, offsets, indices, target, B, True)

    def decode_into(self, records: torch.Tensor, batch: Batch, max_ind_range: int = -1) -> Batch:
        """Decode device records int32 [B * (1 + m_den + T)] into ``batch`` (from
        ``record_batch``) on the current stream: one dlrm_criteo_decode launch (plus, on
        several ranks, the copies of this rank's batch slice and local tables).  Enqueues
        only; capturable."""
        L0 = self.bot[0]
        B = batch.max_per_table
        Bl = batch.X.shape[0]
        if self.world == 1 and self.T_local == self.T:
            ops.criteo_decode(records, L0.K, self.T, max_ind_range, batched=True,
                              dense=batch.X, label=batch.target, indices=batch.indices,
                              offsets=self._rec_offsets(B))
            return batch
        sc = self._rec_scratch
        ops.criteo_decode(records, L0.K, self.T, max_ind_range, batched=True, dense=sc["X"],
                          label=sc["label"], indices=sc["indices"], offsets=sc["offsets"])
        sl = slice(self.rank * Bl, (self.rank + 1) * Bl)
        batch.X[:, :L0.K].copy_(sc["X"][sl, :L0.K])
        batch.target.copy_(sc["label"][sl])
        torch.index_select(sc["indices"].view(self.T, B), 0, sc["tables"],
                           out=batch.indices.view(self.T_local, B))
        return batch

    def _rec_offsets(self, B: int) -> torch.Tensor:
        # the decode rewrites the L = 1 CSR offsets (arange); a private buffer keeps the
        # batch's own copy untouched while a graph may be reading it
        t = self._rec_off.get(B)
        if t is None:
            t = self._rec_off[B] = torch.empty(self.T * B + 1, dtype=torch.int32, device=self.dev)
        return t

    def synthetic_batch(self, B: int, L: int, seed: int, dist: str = "uniform",
                        zipf_a: float = 1.05) -> Batch:
        """Device-generated synthetic batch of the reference's shape: X ~ log(1+U[0,1))
        (dlrm_data_pytorch.py:727), L uniform indices per bag per table, targets U[0,1)
        (rounded for bce).  dist="zipf": the skew-sensitivity run of SURVEY.md §8d - each
        table's indices are Zipf(zipf_a) ranks - 1 folded onto its rows (row 0 hottest),
        drawn on the host (numpy) and uploaded."""
        if dist not in ("uniform", "zipf"):
            raise ValueError(f"dist {dist!r}: uniform or zipf")
        Bl = self.local_batch_size(B)
        L0 = self.bot[0]
        g = torch.Generator(device=self.dev)
        g.manual_seed(seed * 7919 + self.rank)
        Xp = torch.zeros((Bl, L0.Kp), dtype=torch.float32, device=self.dev)
        Xp[:, :L0.K] = torch.log1p(torch.rand((Bl, L0.K), generator=g, device=self.dev))
        Xp[:, L0.K] = 1.0  # bias column
        Tl = self.T_local
        indices = torch.empty(Tl * B * L, dtype=torch.int32, device=self.dev)
        rng = np.random.RandomState(seed) if dist == "zipf" else None
        for j, t in enumerate(self.local_tables):
            n = int(self.cfg.ln_emb[t])
            if rng is not None:
                z = (rng.zipf(zipf_a, B * L) - 1) % n
                indices[j * B * L:(j + 1) * B * L] = torch.from_numpy(z.astype(np.int32))
            else:
                ops.uniform_int_fill_(indices[j * B * L:(j + 1) * B * L], n,
                                      seed * 1000003 + t * 7 + 1)
        offsets = torch.arange(0, Tl * B * L + 1, L, dtype=torch.int32, device=self.dev)
        tg = torch.rand(Bl, generator=g, device=self.dev)
        if self.cfg.loss_function == "bce":
            tg = tg.round()
        return Batch(Xp, offsets, indices, tg, B * L, L == 1)

    # ------------------------------------------------------------- buffers --
    def _buffers(self, Bl: int, B: int):
        key = (Bl, B)
        if key in self._bufs:
            return self._bufs[key]
        dev, D = self.dev, self.D
        f32 = dict(dtype=torch.float32, device=dev)
        bufs = {}
        # activations carry the constant-1 bias column right after their N real columns
        bufs["bot_act"] = [torch.zeros((Bl, L.Np), **f32) for L in self.bot]
        self.ldR = _pad4(self.num_int + 1)
        bufs["R"] = torch.zeros((Bl, self.ldR), **f32)
        bufs["top_act"] = [torch.zeros((Bl, L.Np), **f32) for L in self.top[:-1]]
        for L, a in zip(self.bot + self.top[:-1], bufs["bot_act"] + bufs["top_act"]):
            a[:, L.N] = 1.0
        bufs["R"][:, self.num_int] = 1.0
        wmax = max([L.Kp for L in self.layers] + [self.ldR])
        # split-K workspaces: sized on the first step for this batch size (the step's gemm grows
        # them before any capture), zeroed because the split-K tile tickets must start at 0
        # (the kernels leave them at 0).  They belong to this batch size: a hipGraph
        # captured for it keeps their addresses, and the main and side streams never share.
        bufs["gemm_ws"] = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
        bufs["gemm_ws_side"] = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
        # three gradient buffers: a weight-gradient GEMM on the side stream may still read
        # g_l while the main stream's next two data-gradient GEMMs produce g_{l-1}, g_{l-2}
        bufs["g"] = [torch.zeros((Bl, wmax), **f32) for _ in range(3)]
        wbot = max(L.Kp for L in self.bot)
        bufs["gb"] = [torch.zeros((Bl, wbot), **f32) for _ in range(3)]
        bufs["dx"] = torch.zeros((Bl, D), **f32)
        bufs["gx"] = torch.zeros((Bl, D), **f32)
        Tl = max(self.T_local, 1)
        pad = 0
        if self.feature_pad and not self.distributed and not self.qr_active:
            pad = ((256 - (Tl * D * 4) % 512) % 512) // 4  # stride = 256 B mod 512 B
        for name in ("E", "dE"):
            store = torch.zeros((B, Tl * D + pad), **f32)
            bufs[name] = store[:, :Tl * D].view(B, Tl, D)
        if self.qr_active:  # pooled physical tables (quotient / remainder halves)
            bufs["P"] = torch.zeros((B, self.T_phys, D), **f32)
            bufs["dP"] = torch.zeros_like(bufs["P"])
        if self.distributed:
            bufs["recv"] = torch.zeros(self.T * Bl * D, **f32)
            bufs["drecv"] = torch.zeros_like(bufs["recv"])
        bufs["prob"] = torch.zeros(Bl, **f32)
        bufs["dz"] = torch.zeros(Bl, **f32)
        bufs["loss"] = torch.zeros(1, **f32)
        self._bufs[key] = bufs
        return bufs

    def _features(self, bufs, Bl: int, grad: bool = False):
        """(x, per-feature tensors) for the interaction: feature 0 = bottom-MLP output,
        then the embedding features in rank-major order (single GPU: table order)."""
        D = self.D
        x = bufs["dx"] if grad else bufs["bot_act"][-1][:, :D]
        if not self.distributed:
            return x, bufs["dE" if grad else "E"]
        flat = bufs["drecv" if grad else "recv"]
        feats, o = [], 0
        for r in range(self.world):
            Tr = self.tables_per_rank[r]
            chunk = flat[o:o + Bl * Tr * D].view(Bl, Tr, D)
            feats.extend(chunk[:, j, :] for j in range(Tr))
            o += Bl * Tr * D
        return x, feats

    # ---------------------------------------------------------------- step --
    def step(self, batch: Batch, profile=None):
        """One fwd + loss + bwd + update.  Returns (prob [B_local], loss [1]) device tensors.
        ``profile``: optional callable(name) -> context manager around kernel groups (the
        step then runs on one stream so each group's events bracket only its kernels)."""
        for _kind, fn in self.segments(batch, profile):
            fn()
        return self._cur["prob"], self._cur["loss"]

    def segments(self, batch: Batch, profile=None):
        """The step as an ordered list of ("gpu", fn) / ("a2a", fn) / ("ar", fn) /
        ("host", fn) items.  "gpu" items only enqueue HIP kernels on the current stream (no
        host sync, no allocation after the first step of a batch size): each one can be
        captured in a hipGraph.  "a2a" / "ar" items issue or wait for the all-to-alls / the
        dense all-reduces between them (multi GPU only): RCCL's all-reduces are captured
        with the kernels, its all-to-alls run eagerly between the graphs (capture); on
        gloo every collective runs eagerly.  "host" items are host bookkeeping, run on
        every replay.

        MLP backward: each layer's weight gradient is split-K into a per-layer partial
        buffer and its reduction (+ fused SGD on one GPU) is a REDUCE job inside the NEXT
        GEMM launch (the kernel boundary publishes the partials: no reduce launch, no
        in-launch hand-off); the dgrad in that launch reads W_l, never the W_{l+1} the job
        writes.  Optional side-stream overlaps (self.overlaps): "fwd" = bottom MLP || lookup,
        "bot" = bottom-MLP backward || embedding backward (joined inside the segment).

        cfg.mlp_precision == "bf16": the same list with the MLP layers on the 16-bit MFMA and,
        for now, no launch role, no fused bottom chain and no overlap (_build)."""
        return self._build(batch, profile)

    def _build(self, batch: Batch, profile=None, predict=None):
        """The segment list of the training step (segments) or, ``predict`` = (metrics,
        precision, emb_bits, mlp_bits), of the forward-only pass (predict_segments), from one set of pieces: the
        context of this call first, then the pieces both lists use, the forward-only list,
        the pieces of the backward and the step's four segment orders.

        The precision of the MLP operands selects only the MLP closures (mlp_fwd, top_bwd,
        bottom_bwd): "fp32" = grouped GEMM launches, "bf16" / "fp16" = one 16-bit launch per
        layer and pass.  Every other piece is the same code for both."""
        cfg = self.cfg
        train = predict is None
        metrics, precision, emb_bits, mlp_bits = \
            (None, cfg.mlp_precision, 32, 32) if train else predict
        # predict's mlp_bits = 8: like the 16-bit modes it selects only the MLP
        # closures below and runs without the fused bottom chain
        q8 = None if mlp_bits == 32 else self.quantized_mlp(mlp_bits)
        fp32 = precision == "fp32" and q8 is None
        D = self.D
        Bl = batch.X.shape[0]
        B = Bl * self.world
        # the all-to-all splits assume every rank holds B / W samples of a B-sample batch
        # (dlrm_s_pytorch.py:139-143); a batch built for another world size or table set
        # would send wrong-sized chunks
        n_off = self.T_local * B + 1
        if self.T_local > 0 and batch.offsets.numel() != n_off:
            raise ValueError(f"batch offsets hold {batch.offsets.numel()} entries, expected "
                             f"T_local*B+1 = {n_off} (B = {Bl} x {self.world} ranks)")
        bufs = self._buffers(Bl, B)
        prof = profile or (lambda name: _NullCtx())
        fused_opt = self.grads is None  # single GPU SGD: updates fused into backward
        lr, elr, lr_w = self._rates()  # host floats, or the device slots (lr_mode "device")
        conc = self.concurrent and profile is None
        dist = self.distributed
        st = {}  # state shared by the segments (collective handles, pending reductions)
        # the forward-only pass runs dlrm_tbe_forward: nothing of the backward's sort
        presort = train and self.tbe_presort
        gather = (presort or not train) and not dist and self._gather_applies(batch)
        # fp16 tables (cfg.emb_precision): the same pieces on the fp16 row buffer - the
        # gather-fused interaction reads half rows, the pooled lookup is dlrm_tbe_forward_rows
        # and the update MODE_SGD_F16 as launches of its own (no fp16 launch role: tbe_role
        # below is off for them)
        f16 = self.emb_f16
        # quantized tables (predict's emb_bits = 8 | 4, forward only): a switch beside f16 - the
        # gather-fused interaction reads the packed snapshot, the pooled lookup is
        # dlrm_tbe_forward_rows on it; the master tables are not read at all
        qrows = None if emb_bits == 32 else self.quantized_rows(emb_bits)
        qfmt = None if qrows is None else ops.quant_format(emb_bits)
        # The 16-bit step has no launch role, no bottom chain in the lookup launch and no
        # side-stream overlap (DESIGN.md §16 has the plan to give it them): they are switched
        # off here, once, and the pieces below take the branches they take in an fp32 step
        # with tbe_role, head_role, fuse_bottom and overlaps off.  The chain is an fp32
        # kernel, so a 16-bit predict does not use it either; it keeps the "fwd" overlap.
        plain = fp32 or not train
        overlaps = self.overlaps if plain and not dist else ()
        c_fwd = conc and "fwd" in overlaps
        c_bot = conc and "bot" in overlaps
        # the embedding update's passes, the head's finalize pass as roles of GEMM launches
        # (element-wise Adagrad is no launch role either: its update runs as launches of its own)
        tbe_role = (plain and self.tbe_role and profile is None
                    and self.weights.dtype == torch.float32 and self.emb_sum is None)
        head_role = plain and self.head_role and profile is None and len(self.top) > 1
        fuse_bottom = fp32 and self.fuse_bottom
        if train:
            self._cur = bufs
            self.gather_fused = gather
            ws, ws_keys = bufs, ("gemm_ws", "gemm_ws_side")
        else:
            # its own outputs and GEMM workspaces: it never touches self._cur, self._roles,
            # gather_fused, bottom_fused or step_count
            ws, ws_keys = self._predict_bufs(bufs), ("ws", "ws_side")

        def streams():
            s0 = torch.cuda.current_stream(self.dev)
            return s0, self._side if conc else s0

        def side_if(flag, s1):
            return torch.cuda.stream(s1) if flag else _NullCtx()

        def gemm(problems, side=False):
            """One grouped launch on this pass's workspace of the stream.  In a training step
            a main-stream launch also carries the next pending pass of a deferred embedding
            update or head (self._roles, set by the backward)."""
            with prof("gemm"):
                key = ws_keys[side]
                need = ops.gemm_group_workspace_size(problems) if problems else 0
                if need > ws[key].numel():  # first use of a new group shape (not in capture)
                    ws[key] = torch.zeros(need, dtype=torch.uint8, device=self.dev)
                nxt = self._roles.pop(0) if train and not side and self._roles else None
                role, phase = nxt if nxt is not None else (None, 0)
                ops.gemm_group(problems, ws[key], self.dev, role=role, phase=phase)

        def chain(**kw):
            return self._bottom_chain(batch, bufs, **kw) if fuse_bottom else None

        if fp32:
            def mlp_fwd(L, h, out, side=False):
                gemm([self._fwd(L, h, out)], side=side)
        elif q8 is not None:
            # int8, dynamically quantized: two launches per layer - the min / max partials of
            # the input, then the Linear on the i8 MFMA, whose workgroups derive the input's
            # scale and zero point from the partials themselves (no host read).  The packed
            # weights and the bias are quantize_mlp's snapshot, not the fp32 masters.
            def mlp_fwd(L, h, out, side=False, relu=True):
                with prof("gemm"):
                    s = q8[id(L)]
                    ops.linear8_range(h[:, :L.K], out=s.rng)
                    ops.linear8_forward(h[:, :L.K], s.packed, bias=s.bias, relu=relu,
                                        out=out[:, :L.N], rng=s.rng)
        else:
            # 16 bit: one launch, relu(r16(h[:, :K]) r16(W[:, :K])^T + b) -> out[:, :N], the
            # operands rounded to nearest-even in flight from the fp32 tensors (no weight
            # copy exists), fp32 accumulate; the constant-1 columns stay untouched
            def mlp_fwd(L, h, out, side=False):
                with prof("gemm"):
                    ops.linear16_forward(h[:, :L.K], L.W[:, :L.K], L.b, relu=True,
                                         out=out[:, :L.N], dtype=precision)

        # the reference's profiler phase names (dlrm_s_pytorch.py:692-721, 171, 1923), so a
        # torch.profiler trace of this step lines up with one of the reference's
        emb_sizes = "-".join(str(int(cfg.ln_emb[t])) for t in self.local_tables)

        def lookup(bottom=None):
            """Embeddings (full batch, local tables).  presort: the backward's per-table
            sort runs inside the lookup launch (alone, when the interaction gathers the rows
            itself); ``bottom``: the bottom MLP forward, a chain, as a further role of it."""
            with record_function("module::forward_pass::embedding_lookup", emb_sizes), \
                    prof("tbe_fwd"):
                if self.T_local == 0:
                    return
                if "csr" not in st:
                    st["csr"] = self._phys_csr(batch, B)
                idx, off = st["csr"]
                out = bufs["P"] if self.qr_active else bufs["E"]
                if qrows is not None:  # forward only, never with QR: one pooled Q lookup
                    ops.tbe_forward_rows(qrows, qfmt, D, self.row_base, self.T_phys, B, idx,
                                         off, out=out, out_batch_stride=out.stride(0),
                                         error_flag=self.tbe_error_flag)
                elif f16 and not gather:
                    # the pooled lookup on fp16 rows is a launch of its own; the lookup launch
                    # keeps its sort role (the sort never reads a row) and the bottom MLP's
                    # where the per-table sort applies, else the backward sorts itself
                    st["presorted"] = presort and self._presort_sorts(batch, idx, B)
                    if st["presorted"]:
                        ops.tbe_forward_presort(self.weights, self.row_base, self.T_phys, B,
                                                idx, off, self._ws_tbe(idx.numel()),
                                                batch.max_per_table,
                                                error_flag=self.tbe_error_flag, bottom=bottom,
                                                lookup=False)
                    elif bottom is not None:
                        ops.mlp_chain_forward(bottom, self.dev)
                    ops.tbe_forward_rows(self.weights, ops.ROWS_F16, D, self.row_base,
                                         self.T_phys, B, idx, off, out=out,
                                         out_batch_stride=out.stride(0),
                                         error_flag=self.tbe_error_flag)
                elif presort:
                    ops.tbe_forward_presort(self.weights, self.row_base, self.T_phys, B, idx,
                                            off, self._ws_tbe(idx.numel()),
                                            batch.max_per_table, out=None if gather else out,
                                            out_batch_stride=out.stride(0),
                                            error_flag=self.tbe_error_flag, bottom=bottom,
                                            lookup=not gather)
                else:
                    ops.tbe_forward(self.weights, self.row_base, self.T_phys, B, idx, off,
                                    out=out, out_batch_stride=out.stride(0),
                                    error_flag=self.tbe_error_flag)
                if self.qr_active:
                    ops.qr_pool_combine_forward(cfg.qr_operation, self.T_local, B, D,
                                                self._qr_pq, self._qr_pr, bufs["P"], bufs["E"])

        # the bottom MLP as one row-block chain launch of its own (activations in LDS between
        # layers, mlp_rows.hpp): several GPUs, while the all-to-all is in flight, and predict
        own_chain = not train or (dist and profile is None)

        def bottom_fwd():
            if st.pop("bottom_done", False):  # ran inside the lookup launch
                return _EMPTY
            with record_function("module::forward_pass::bottom_mlp"):
                c = chain(sort_wgs=0, standalone=True) if own_chain else None
                if c is not None:
                    ops.mlp_chain_forward(c, self.dev)
                    return
                h = batch.X
                for L, out in zip(self.bot, bufs["bot_act"]):
                    mlp_fwd(L, h, out, side=c_fwd)
                    h = out

        def beside_bottom(look):
            """One GPU: ``look`` (or nothing) on the main stream, then the bottom MLP - with
            the "fwd" overlap beside it, on the side stream."""
            s0, s1 = streams()
            if c_fwd:
                s1.wait_stream(s0)
            if look is not None:
                look()
            with side_if(c_fwd, s1):
                bottom_fwd()
            if c_fwd:
                s0.wait_stream(s1)

        def interaction_fwd():
            x, feats = self._features(bufs, Bl)
            with record_function("module::forward_pass::interaction"), prof("interaction_fwd"):
                if gather and qrows is not None:  # the same on the packed snapshot
                    ops.interact_forward_gather_rows(x, qrows, qfmt, D, self.row_base,
                                                     batch.indices, cfg.arch_interaction_itself,
                                                     out=bufs["R"], error_flag=self.tbe_error_flag)
                elif gather:  # one-hot lookup fused: rows read straight from the tables
                    ops.interact_forward_gather(x, self.weights, self.row_base, batch.indices,
                                                cfg.arch_interaction_itself, out=bufs["R"],
                                                error_flag=self.tbe_error_flag)
                else:
                    ops.interact_forward(cfg.arch_interaction_op, x, feats,
                                         cfg.arch_interaction_itself, out=bufs["R"])
            return x, feats

        def top_fwd():  # the top MLP below the head
            h = bufs["R"]
            for L, out in zip(self.top[:-1], bufs["top_act"]):
                mlp_fwd(L, h, out)
                h = out
            return h

        def wait(key):
            return lambda: st.pop(key).wait()

        a2a_fwd = lambda: st.__setitem__("a2a", self._alltoall_fwd(bufs, Bl))  # noqa: E731
        last = self.top[-1]

        if not train:
            def lookup_only():  # no launch when the interaction gathers the rows itself
                if self.T_local == 0 or gather:
                    return _EMPTY
                st.pop("csr", None)  # QR: every run expands the batch's current contents
                lookup()

            def score():
                interaction_fwd()
                with record_function("module::forward_pass::top_mlp"):
                    h = top_fwd()
                    hx, hw = h[:, :last.Kp], last.W[0, :last.Kp]
                    if q8 is not None:
                        # the reference quantizes every nn.Linear: the last one runs as an
                        # N = 1 int8 layer without ReLU, and the head takes its z as a
                        # one-column input with weight 1.0 (fmaf(z, 1, 0) and a wave sum with
                        # zeros: z itself), so the sigmoid, clamp and log stay the head's
                        mlp_fwd(last, h, ws["z8"], relu=False)
                        hx, hw = ws["z8"], ws["one8"]
                    ops.head_predict(hx, hw, cfg.loss_threshold,
                                     prob=ws["prob"],
                                     target=batch.target if metrics is not None else None,
                                     state=metrics)

            if not dist:
                return [("gpu", lambda: beside_bottom(lookup_only)), ("gpu", score)]
            return [
                ("gpu", lookup_only),
                ("a2a", a2a_fwd),
                ("gpu", bottom_fwd),
                ("a2a", wait("a2a")),
                ("gpu", score),
            ]

        def first(fn):
            """The step's first segment.  A launch role deferred by an aborted step (raw
            pointers of that step) must never ride on this step's launches; and in lr_mode
            "device" the step starts with the schedule's tick, on the main stream before
            anything forks off it (the early sort's side stream and the collectives wait for
            the main stream later, so they are ordered after it)."""
            def run():
                self._roles = []
                if self._lr_state is not None:
                    ops.lr_schedule_tick(self._lr_state)
                return fn()
            return run

        def early_sort():  # the backward's sort on the side stream, beside the forward
            s0, s1 = streams()
            idx, off = st["csr"] = self._phys_csr(batch, B)
            s1.wait_stream(s0)
            with torch.cuda.stream(s1), prof("tbe_sort"):
                ops.tbe_backward_sort(self.weights, self.row_base, self.T_phys, B, idx, off,
                                      self._ws_tbe(idx.numel()), batch.max_per_table,
                                      error_flag=self.tbe_error_flag)
            st["sorted"] = s1

        def fwd_single():  # one GPU: bottom MLP || lookup
            es = (self.early_sort and conc and self.T_local > 0 and presort
                  and not 0 < batch.max_per_table <= ops.TBE_PRESORT_SEG_CAP)
            late = es and self.early_sort == 2  # 2: forked after the lookup launch instead
            if es and not late:
                early_sort()
            c = chain() if presort and not c_fwd else None
            self.bottom_fused = c is not None
            if c is not None:  # the bottom MLP forward runs as a role of the lookup launch
                with record_function("module::forward_pass::bottom_mlp"):
                    lookup(c)
            elif late:
                lookup()
            if late:
                early_sort()
            if c is None:
                beside_bottom(None if late else lookup)

        def lookup_dist():
            # several GPUs: the bottom MLP forward as a role of the lookup launch too
            c = chain() if presort and profile is None and self.dist_bottom_in_lookup else None
            st["bottom_done"] = c is not None
            lookup(c)

        def head(h):
            """Last layer + sigmoid + loss + dz + input grad + [dw | db] (bias folded:
            [h | 1] . [w | b]) in two launches; the update follows every read of w.  Returns
            the gradient of the head's input.  head_role: the second launch (column sums +
            update or gradient + mean loss) rides on the top-MLP backward's first GEMM launch
            (dlrm_head_step_defer)."""
            g = bufs["g"][0][:, :last.Kp]
            with record_function("## Loss Compute ##"), prof("head"):
                r = ops.head_step(h[:, :last.Kp], last.W[0, :last.Kp], batch.target,
                                  cfg.loss_function, cfg.loss_threshold, 1.0, prob=bufs["prob"],
                                  dz=bufs["dz"], loss_out=bufs["loss"], dX=g,
                                  relu_mask=len(self.top) > 1,
                                  dw=None if fused_opt else last.gW[0, :last.Kp],
                                  lr=lr if fused_opt else 0.0,
                                  workspace=self._ws_head_step(Bl, last.Kp), defer=head_role)
                if head_role:
                    self._roles = [x for x in self._roles if x is not None] + [(r, 4)]
            return g

        # The MLP backward, from the head's input gradient down.  Both forms walk the layers
        # from the top; the gradient rotates over three buffers (bufs["g"]; the bottom MLP's
        # over bufs["gb"]); the top MLP's first layer has no ReLU mask (its input is the
        # interaction) and the bottom MLP's first layer no data gradient at all.
        if fp32:
            def top_bwd(g):
                """Returns the gradient of the interaction's output; the reduce jobs still
                to ride on a launch go to st["rq"]."""
                G, gi = bufs["g"], 0
                rq = []  # reduce jobs riding on the next launch
                for li in range(len(self.top) - 2, -1, -1):
                    L = self.top[li]
                    inp = bufs["top_act"][li - 1] if li > 0 else bufs["R"]
                    gn = (gi + 1) % 3
                    dg = self._dgrad(L, g, inp if li > 0 else None, G[gn])
                    # several GPUs: the top bucket is all-reduced right after this loop, so
                    # its last wgrad reduces its K split inside its own launch
                    w, r = self._wg(L, g, inp, fused_opt, lr, ("top", li),
                                    full=dist and li == 0)
                    if r is not None and self.group_wgrad:
                        # the split wgrad only writes partials (its update rides on the next
                        # launch's reduce job), so it may run beside the dgrad reading W
                        gemm([dg, w] + rq)
                        rq = [r]
                    elif r is None and not fused_opt:
                        # the wgrad writes the gradient bucket, not W: beside the dgrad
                        gemm([dg, w] + rq)
                        rq = []
                    elif r is not None:
                        # a split wgrad kept out of the dgrad's launch (group_wgrad off): its
                        # partials in a launch of their own, its reduce job on the next one
                        gemm([dg] + rq)
                        gemm([w])
                        rq = [r]
                    else:
                        # an unsplit wgrad updates W_l in its epilogue: it rides on the NEXT
                        # launch (dgrad of layer l-1 reads W_{l-1}, not W_l; its g_l buffer
                        # is not overwritten there: G rotates over three)
                        gemm([dg] + rq)
                        rq = [w]
                    g, gi = G[gn], gn
                st["rq"] = rq
                return g

            def bottom_bwd_full():
                """Bottom-MLP backward with in-launch split-K wgrads (FULL, SGD fused): the
                wgrad of layer l rides in the launch of dgrad(l-1), which does not read W_l,
                and the last launch holds the two lowest wgrads - n_bot launches, no trailing
                REDUCE.  dgrad(l) writes g_{l-1} into buffer l % 3: the wgrad it shares a
                launch with reads g_{l+1} from buffer (l+2) % 3."""
                rq = st.pop("rq")
                g = bufs["gx"]
                pending = []
                for li in range(self.n_bot - 1, -1, -1):
                    L = self.bot[li]
                    inp = bufs["bot_act"][li - 1] if li > 0 else batch.X
                    w = self._wgrad(L, g, inp, fused_opt, lr)
                    if li > 0:
                        out = bufs["gb"][li % 3]
                        gemm([self._dgrad(L, g, inp, out)] + pending + rq)
                        rq, pending, g = [], [w], out
                    else:
                        gemm(pending + [w] + rq)

            def bottom_bwd(hold_last=False):
                """hold_last: the last launch's problems go to st["bot_last"] instead of
                being launched (several GPUs: it then carries the embedding update's first
                pass once the reverse all-to-all has landed)."""
                sched = self.bot_sched
                if sched == "auto":
                    sched = "full" if Bl <= 128 else "partial"
                if sched == "full" and not c_bot and fused_opt:
                    return bottom_bwd_full()
                rq = st.pop("rq")
                g = bufs["gx"]  # dLoss/d(pre-ReLU bottom output), from the interaction backward
                bg = [bufs["gb"][0], bufs["gb"][1]]
                launches = []
                for li in range(self.n_bot - 1, -1, -1):
                    L = self.bot[li]
                    inp = bufs["bot_act"][li - 1] if li > 0 else batch.X
                    w, r = self._wg(L, g, inp, fused_opt, lr, ("bot", li), last=li == 0)
                    if li > 0 and r is not None and self.group_wgrad:
                        launches.append([self._dgrad(L, g, inp, bg[li % 2]), w] + rq)
                    elif li > 0 and r is None and not fused_opt:
                        # the wgrad writes the gradient bucket, not W: beside the dgrad
                        launches.append([self._dgrad(L, g, inp, bg[li % 2]), w] + rq)
                    else:
                        if li > 0:
                            launches.append([self._dgrad(L, g, inp, bg[li % 2])] + rq)
                            rq = []
                        launches.append([w] + rq)
                    rq = [r] if r is not None else []
                    if li > 0:
                        g = bg[li % 2]
                if rq:
                    launches.append(rq)
                if hold_last:
                    st["bot_last"] = launches.pop()
                for probs in launches:
                    gemm(probs, side=c_bot)
        else:
            # 16 bit (bf16): a layer is two launches in stream order, ops.linear16_dgrad
            # (mask = the layer's input activation) and then ops.linear16_wgrad over the
            # K + 1 columns [inp | 1] -> [W | b] (the constant-1 column yields
            # db = sum_m r16(g)), SGD-fused into W on one GPU with SGD, else stored into the
            # gradient bucket.  Stream order puts a layer's update after the dgrad that
            # reads its W.  group_wgrad, full_last_wgrad and bot_sched have no effect here.
            def dgrad16(L, g, inp, out):
                with prof("gemm"):
                    ops.linear16_dgrad(g[:, :L.N], L.W[:, :L.K],
                                       None if inp is None else inp[:, :L.K], out=out[:, :L.K],
                                       dtype=precision)

            def wgrad16(L, g, inp):
                C = L.W if fused_opt else L.gW
                with prof("gemm"):
                    ops.linear16_wgrad(g[:, :L.N], inp[:, :L.K + 1], C[:, :L.K + 1],
                                       lr=lr if fused_opt else None, dtype=precision,
                                       workspace=self._ws_wgrad16(bufs, Bl, L.N, L.K + 1))

            def top_bwd(g):
                G, gi = bufs["g"], 0
                for li in range(len(self.top) - 2, -1, -1):
                    L = self.top[li]
                    inp = bufs["top_act"][li - 1] if li > 0 else bufs["R"]
                    gn = (gi + 1) % 3
                    dgrad16(L, g, inp if li > 0 else None, G[gn])
                    wgrad16(L, g, inp)
                    g, gi = G[gn], gn
                return g

            def bottom_bwd():
                g = bufs["gx"]  # dLoss/d(pre-ReLU bottom output), from the interaction backward
                for li in range(self.n_bot - 1, -1, -1):
                    L = self.bot[li]
                    inp = bufs["bot_act"][li - 1] if li > 0 else batch.X
                    if li > 0:
                        dgrad16(L, g, inp, bufs["gb"][li % 2])
                    wgrad16(L, g, inp)
                    if li > 0:
                        g = bufs["gb"][li % 2]

        def top():  # interaction, top MLP, head, top backward
            x, feats = interaction_fwd()
            with record_function("module::forward_pass::top_mlp"):
                h = top_fwd()
            g = head(h)
            with record_function("## Backward ##"):
                g = top_bwd(g)
            st.update(x=x, feats=feats, g=g)

        def interaction_bwd():
            x, feats, g = st.pop("x"), st.pop("feats"), st.pop("g")
            with record_function("## Backward ##"):
                _, gfeats = self._features(bufs, Bl, grad=True)
                with prof("interaction_bwd"):  # + the backward of the bottom MLP's last ReLU
                    if gather:  # rows re-gathered (the embedding update comes later)
                        ops.interact_backward_gather(
                            x, self.weights, self.row_base, batch.indices, g[:, :self.num_int],
                            cfg.arch_interaction_itself, grad_x=bufs["gx"], grad_ly=gfeats,
                            relu_x=True)
                    else:
                        ops.interact_backward(
                            cfg.arch_interaction_op, x, feats, g[:, :self.num_int],
                            cfg.arch_interaction_itself, grad_x=bufs["gx"], grad_ly=gfeats,
                            relu_x=True)

        def middle():  # interaction, top MLP, head, top backward, interaction backward
            top()
            interaction_bwd()

        def emb_bwd(defer=False):  # embedding backward + fused update
            """defer=True: the update's two passes are returned as a role for the next two
            GEMM launches (None: it ran in full here)."""
            with prof("tbe_bwd"):
                if self.T_local > 0:
                    mode = "rowwise_adagrad" if cfg.optimizer == "rwsadagrad" else "sgd"
                    if f16:
                        mode = "sgd_f16"
                    emb_state = self.momentum
                    if self.emb_sum is not None:
                        mode, emb_state = "adagrad", self.emb_sum
                    idx, off = st["csr"]
                    grad = bufs["dE"]
                    if self.qr_active:
                        ops.qr_pool_combine_backward(cfg.qr_operation, self.T_local, B, D,
                                                     self._qr_pq, self._qr_pr, bufs["P"],
                                                     bufs["dE"], bufs["dP"])
                        grad = bufs["dP"]
                    fn = ops.tbe_backward_defer if defer else ops.tbe_backward
                    s1 = st.pop("sorted", None)
                    if s1 is not None:  # join the early sort
                        torch.cuda.current_stream(self.dev).wait_stream(s1)
                    kw = dict(lr=elr, eps=cfg.adagrad_eps, momentum=emb_state,
                              grad_batch_stride=grad.stride(0),
                              workspace=self._ws_tbe(idx.numel()),
                              max_lookups_per_table=batch.max_per_table,
                              error_flag=self.tbe_error_flag,
                              presorted=ops.PRESORTED_ANY if s1 is not None
                              else st.get("presorted", presort))
                    if self._sr_state is not None:
                        # the fp16 update storing sr16 of the row (never deferred: tbe_role
                        # is off for fp16 tables), then the stream's tick behind it
                        ops.tbe_backward(mode, self.weights, self.row_base, self.T_phys, B,
                                         idx, off, grad, sr_state=self._sr_state, **kw)
                        ops.sr_tick(self._sr_state)
                        return None
                    return fn(mode, self.weights, self.row_base, self.T_phys, B, idx, off,
                              grad, **kw)

        @record_function("## Backward ##")
        def backward_single():  # one GPU: bottom backward || embedding backward
            s0, s1 = streams()
            if c_bot:
                if st["rq"]:
                    gemm(st["rq"])
                st["rq"] = []
                s1.wait_stream(s0)
            # the embedding update's two HBM-bound passes ride as extra workgroups on the
            # first two (MFMA-bound) bottom-backward launches: overlap with no cross-queue
            # dependency (dlrm_tbe_backward_defer / dlrm_gemm_f32_group_role)
            deferred = tbe_role and not c_bot and self.T_local > 0
            if deferred:
                a, b = self._check_role_at(self.tbe_role_at)
                role = emb_bwd(defer=True)
                if role is not None:  # pass p rides on bottom-backward launch tbe_role_at[p-1]
                    self._roles = [None] * (b + 1)
                    self._roles[a], self._roles[b] = (role, 1), (role, 2)
            with side_if(c_bot, s1):
                bottom_bwd()
            while self._roles:  # a pass the bottom backward had no launch left for
                if self._roles[0] is None:
                    self._roles.pop(0)
                else:
                    gemm([])
            if not deferred:
                emb_bwd()
            if c_bot:
                s0.wait_stream(s1)

        def dense_update():
            with record_function("## Backward ##"), prof("dense_update"):
                if cfg.optimizer == "sgd" and st.pop("top_updated", False):
                    # the top bucket's update rode on the embedding update's second pass
                    nb = self.n_bot_params
                    ops.sgd_update(self.params[:nb], self.grads[:nb], lr_w)
                elif cfg.optimizer == "sgd":
                    ops.sgd_update(self.params, self.grads, lr_w)
                else:  # the 1/W folded into the update (one pass over the bucket)
                    ops.adagrad_update(self.params, self.grads, self.adagrad_sum, lr,
                                       cfg.adagrad_eps, grad_scale=1.0 / self.world)

        def done():
            self.step_count += 1

        if not dist:
            segs = [("gpu", first(fwd_single)), ("gpu", middle), ("gpu", backward_single)]
            if not fused_opt:
                segs.append(("gpu", dense_update))
            return segs + [("host", done)]
        # multi GPU (distributed_forward, dlrm_s_pytorch.py:686-730; DDP :1626-1633):
        #  * the pooled-embedding all-to-all overlaps the bottom MLP (one chain launch);
        #  * the top MLP's gradient bucket is all-reduced as soon as the top backward is
        #    done (DDP's per-module buckets), overlapping the interaction backward, the
        #    bottom backward and the embedding update; the bottom bucket follows the bottom
        #    backward.  The all-reduces run on a communicator of their own, so they never
        #    queue the reverse all-to-all that the embedding update waits for;
        #  * the reverse all-to-all overlaps the bottom backward.
        def ar(bucket):
            def start():
                g = self.grads[self.n_bot_params:] if bucket == "top" else \
                    self.grads[:self.n_bot_params]
                st["ar_" + bucket] = self.comm.allreduce(g)
            return start

        a2a_bwd = lambda: st.__setitem__("a2a", self._alltoall_bwd(bufs, Bl))  # noqa: E731
        bwd = lambda fn: record_function("## Backward ##")(fn)  # noqa: E731

        def bottom_tail():  # after All2All_Wait: the update's passes ride on GEMM launches
            role = emb_bwd(defer=True)
            if role is not None:
                self._roles = [(role, 1)]
                st["emb_role"] = role
            gemm(st.pop("bot_last"))
            self._roles = []

        def emb_pass2():
            role = st.pop("emb_role", None)
            if role is None:
                return
            jobs = []
            if cfg.optimizer == "sgd":  # the top bucket was all-reduced (waited) already
                nb = self.n_bot_params
                jobs = [ops.sgd_job(self.params[nb:], self.grads[nb:], lr_w)]
                st["top_updated"] = True
            self._roles = [(role, 2)]
            gemm(jobs)
            self._roles = []

        # RCCL: the all-reduces capture into hipGraphs, the all-to-alls do not (DESIGN.md §8:
        # a captured all_to_all_single or send/recv crashes hipStreamEndCapture on this
        # stack).  Each all-reduce is waited in the graph that issues it, so the step is FOUR
        # graphs around the two eager all-to-alls: the top bucket overlaps the bottom
        # backward and the reverse all-to-all, the bottom bucket the embedding update's
        # second pass.  gloo (host-staged, synchronous) runs the same order eagerly, with
        # the top bucket's all-reduce started right after the top backward.
        forward = [
            ("gpu", first(lookup_dist)),
            ("a2a", a2a_fwd),
            ("gpu", bottom_fwd),
            ("a2a", wait("a2a")),  # All2All_Wait (extend_distributed.py:489)
            ("gpu", top),
        ]
        if tbe_role:
            # the embedding update's two passes as launch roles (as on one GPU): the first on
            # the bottom backward's last launch, held back until the reverse all-to-all has
            # landed; the second on a launch that also applies the top bucket's SGD update.
            # The choice must not depend on the rank (T_local): every rank issues the same
            # collectives in the same order (a rank without tables just carries no role)
            return forward + [
                ("gpu", interaction_bwd),
                ("a2a", a2a_bwd),
                ("ar", ar("top")),
                ("gpu", bwd(lambda: bottom_bwd(hold_last=True))),
                ("ar", wait("ar_top")),
                ("a2a", wait("a2a")),
                ("gpu", bwd(bottom_tail)),
                ("ar", ar("bot")),
                ("gpu", bwd(emb_pass2)),
                ("ar", wait("ar_bot")),
                ("gpu", dense_update),
                ("host", done),
            ]
        if getattr(self.comm, "capture_ar", False):
            return forward + [
                ("gpu", interaction_bwd),
                ("a2a", a2a_bwd),
                ("ar", ar("top")),
                ("gpu", bwd(bottom_bwd)),
                ("ar", wait("ar_top")),
                ("a2a", wait("a2a")),
                ("ar", ar("bot")),
                ("gpu", bwd(emb_bwd)),
                ("ar", wait("ar_bot")),
                ("gpu", dense_update),
                ("host", done),
            ]
        return forward + [
            ("ar", ar("top")),
            ("gpu", interaction_bwd),
            ("a2a", a2a_bwd),
            ("gpu", bwd(bottom_bwd)),
            ("ar", ar("bot")),
            ("a2a", wait("a2a")),
            ("gpu", bwd(emb_bwd)),
            ("ar", wait("ar_top")),
            ("ar", wait("ar_bot")),
            ("gpu", dense_update),
            ("host", done),
        ]

    def _ws_wgrad16(self, bufs, M: int, N: int, K: int) -> Optional[torch.Tensor]:
        """The batch size's linear16_wgrad workspace (its layers run in stream order and
        share it), grown on the eager steps only: a captured graph keeps its address."""
        need = ops.linear16_wgrad_workspace_size(M, N, K, self.cfg.mlp_precision)
        ws = bufs.get("wgrad16_ws")
        if need and (ws is None or ws.numel() < need):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("capture() needs one eager step of this batch size first "
                                   "(the wgrad workspace)")
            ws = bufs["wgrad16_ws"] = torch.empty(need, dtype=torch.uint8, device=self.dev)
        return ws

    @staticmethod
    def _check_role_at(at):
        """tbe_role_at = (a, b): the bottom-backward launches carrying the update's block
        pass and its combine pass.  The combine pass reads what the block pass wrote, so it
        must ride on a LATER launch: 0 <= a < b."""
        a, b = (int(v) for v in at)
        if not 0 <= a < b:
            raise ValueError(f"tbe_role_at={tuple(at)}: need 0 <= a < b (the combine pass "
                             "rides on a later launch than the block pass)")
        return a, b

    def _gather_applies(self, batch: Batch) -> bool:
        """One-hot lookups gathered inside the dot interaction: one GPU, plain tables, every
        bag one index, and the lookup launch able to run its sort role alone (the per-table
        sort of dlrm_tbe_forward_presort: <= 4096 lookups per table, 32-bit row keys)."""
        return (self.fuse_gather and batch.one_hot and not self.distributed and not self.qr_active
                and self.cfg.arch_interaction_op == "dot" and self.D in (16, 32, 64, 128)
                and 1 <= self.T_local == self.T and self.T + 1 <= 32
                and 0 < batch.max_per_table <= ops.TBE_PRESORT_SEG_CAP
                and self.weights.shape[0] < 0xFFFFFFFF
                and batch.indices.numel() == self.T * batch.X.shape[0])

    def _presort_sorts(self, batch: Batch, idx: torch.Tensor, B: int) -> bool:
        """Whether the lookup launch runs the backward's per-table sort for this batch
        (dlrm_tbe_forward_presort's own rule: 32-bit row keys, every table within the LDS
        sort's bound); its sort-only form exists only then."""
        n = idx.numel()
        return (0 < batch.max_per_table <= ops.TBE_PRESORT_SEG_CAP
                and self.weights.shape[0] < 0xFFFFFFFF and 0 < n < 0x7FFFFFFF
                and self.T_phys * B < 0x7FFFFFFF)

    def _phys_csr(self, batch: Batch, B: int):
        """(indices, offsets) of the physical tables for this batch: the batch's own CSR, or
        (QR) the expanded CSR written by one dlrm_qr_expand_csr launch into buffers owned by
        this (batch size, lookup count) so captured graphs keep their addresses."""
        if not self.qr_active:
            return batch.indices, batch.offsets
        n_log = batch.indices.numel()
        mx = int(batch.max_per_table)
        if mx > 0 and mx * self.T_local == n_log:  # every table has mx lookups
            n = mx * self.T_phys
        else:  # bound: the tail past the last bag is skipped by the kernels
            n = n_log + (self.T_phys - self.T_local) * (mx if mx > 0 else n_log)
        key = (B, n)
        if key not in self._qr_csr:
            self._qr_csr[key] = (
                torch.zeros(max(n, 1), dtype=torch.int32, device=self.dev),
                torch.zeros(self.T_phys * B + 1, dtype=torch.int32, device=self.dev))
        pidx, poff = self._qr_csr[key]
        ops.qr_expand_csr(self.T_phys, B, batch.indices, batch.offsets, self._qr_src,
                          self._qr_kind, self._qr_coll, mx if mx > 0 else n_log, pidx, poff,
                          error_flag=self.tbe_error_flag)
        return pidx, poff

    def capture(self, batch: Batch, pool=None, whole: Optional[bool] = None):
        """A replayable step for ``batch``.  whole (default: one GPU, or a comm whose
        collectives all capture): the step's kernels AND its collectives in ONE hipGraph (a
        graph-to-graph boundary costs ~9 us of idle GPU, profiles/r05_step_timeline_emul8_
        r2.txt); else the "gpu" segments - with the collectives the comm can capture
        (``capture_ar``: RCCL's all-reduces) - as graphs, and the rest ("a2a": RCCL's
        all-to-alls, everything on gloo) run eagerly between them.  Run one eager step of
        this batch size first (allocations).  Returns a callable; each call is one full
        training step on the captured buffers."""
        run, self.capture_mode, self.graphs_per_step = self._capture_segments(
            lambda: self.segments(batch), pool, whole)
        return run

    def _capture_segments(self, make_segs, pool, whole):
        """capture()'s two modes over any segment list (``make_segs()`` builds a fresh one:
        the training step's or predict_segments').  Returns (callable, mode, graphs per
        replay)."""
        auto = whole is None
        if auto:
            whole = not self.distributed or bool(getattr(self.comm, "capturable", False))
        if whole:
            segs = make_segs()
            host = [fn for kind, fn in segs if kind == "host"]
            g = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(g, pool=pool):
                    for kind, fn in segs:
                        if kind != "host":
                            fn()
            except Exception as e:  # noqa: BLE001
                if not (auto and self.distributed):
                    raise
                import warnings
                warnings.warn(f"whole-step capture with the collectives failed ({e!r}); "
                              "capturing the kernel segments between eager collectives")
                torch.cuda.synchronize()
                return self._capture_segments(make_segs, pool, False)

            def run_whole():
                g.replay()
                for fn in host:
                    fn()
            return run_whole, "whole", 1
        in_graph = {"gpu"}
        if getattr(self.comm, "capture_ar", False):
            in_graph.add("ar")
        items = []
        pending = []
        segs = make_segs()
        graphs = [0]

        def flush():
            if not pending:
                return
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool):
                launched = [fn() is not _EMPTY for fn in pending]
            if any(launched):  # a segment that enqueued nothing is not replayed
                items.append(g.replay)
                graphs[0] += 1
            pending.clear()

        for kind, fn in segs:
            if kind in in_graph:
                pending.append(fn)
            elif kind == "host":
                items.append(fn)
            else:
                flush()
                items.append(fn)
        flush()

        def run():
            for f in items:
                f()
        return run, "segments", graphs[0]

    # ---------------------------------------------------------- evaluation --
    def _quant_refusals(self) -> None:
        if self.qr:
            raise NotImplementedError(
                "quantized embedding tables with qr_flag: the QR combine runs on fp32 tables "
                "only (DESIGN.md §20)")
        if self.distributed:
            raise NotImplementedError(
                "quantized embedding tables on the multi-GPU schedule: they run on one GPU "
                "only (DESIGN.md §20)")
        if self.D % 4 or self.D > 512:
            raise NotImplementedError(
                f"quantized embedding tables with m_spa={self.D}: the packed rows take D a "
                "multiple of 4 and at most 512 (dlrm_rows_quantize; DESIGN.md §20)")

    def quantize_embedding(self, bits: int) -> torch.Tensor:
        """Pack the engine's current tables (fp32, or emb_precision "fp16") row-wise to
        ``bits`` (8 | 4) on the device: one dlrm_rows_quantize over the whole row buffer into
        an engine-owned uint8 [rows, row_bytes] buffer that predict(..., emb_bits=bits) reads
        (the reference's --quantize-emb-with-bit, DLRM_Net.quantize_embedding,
        dlrm_s_pytorch.py:609-625; bitwise torch's CPU packers).  Row pitches are uniform, so
        ``row_base`` serves both buffers.

        There is one buffer per width and a second call re-packs into the same storage, so
        an already captured predict graph reads the new values.  The packed rows are a
        SNAPSHOT: the master tables stay, training is untouched, and training after this
        call does not move the packed rows until the next call."""
        ops.quant_format(bits)
        self._quant_refusals()
        self._qrows[bits] = ops.rows_quantize(self.weights, bits, out=self._qrows.get(bits))
        return self._qrows[bits]

    def quantized_rows(self, bits: int) -> torch.Tensor:
        """The packed buffer of ``bits`` (uint8 [rows, row_bytes], table t = rows
        [row_base[t], row_base[t+1]))."""
        ops.quant_format(bits)
        if bits not in self._qrows:
            raise RuntimeError(f"no {bits}-bit tables: call quantize_embedding({bits}) first")
        return self._qrows[bits]

    def _emb_bits(self, emb_bits: int) -> int:
        """Validate predict's ``emb_bits``: 32 = the master tables, 8 | 4 = the packed
        snapshot of that width (which must exist)."""
        if emb_bits == 32:
            return 32
        if emb_bits not in (4, 8):
            raise ValueError(f"emb_bits {emb_bits!r}: 32, 8 or 4")
        self._quant_refusals()
        self.quantized_rows(emb_bits)
        return int(emb_bits)

    def quantize_mlp(self, bits: int) -> None:
        """Pack every Linear of the bottom and top MLP, the last top layer included, for
        predict(..., mlp_bits=8): per-tensor symmetric int8 weights (dlrm_linear8_pack, the
        bias column left out of the range) and a copy of the bias, in engine-owned buffers
        (the reference's --quantize-mlp-with-bit 8: torch.quantization.quantize_dynamic over
        every nn.Linear, dlrm_s_pytorch.py:1757-1781).

        A SNAPSHOT, as quantize_embedding's: the fp32 masters stay, training is untouched and
        does not move the packed layers; a second call re-packs into the same storage, so an
        already captured predict graph reads the new values."""
        if bits != 8:
            raise ValueError(f"quantize_mlp({bits!r}): 8 (16-bit operands need no packing: "
                             "predict(..., precision='bf16' | 'fp16'))")
        self._mlp8_refusals()
        if self._mlp8 is None:
            self._mlp8 = {}
        for L in self.layers:
            s = self._mlp8.get(id(L))
            if s is None:
                s = self._mlp8[id(L)] = _Layer8(
                    packed=None, bias=torch.empty(L.N, dtype=torch.float32, device=self.dev),
                    rng=torch.zeros(ops.LINEAR8_RANGE_FLOATS, dtype=torch.float32,
                                    device=self.dev))
            s.packed = ops.linear8_pack(L.W[:, :L.K], out=s.packed)
            s.bias.copy_(L.b)

    def _mlp8_refusals(self) -> None:
        if self.distributed:
            raise NotImplementedError(
                "int8 MLP layers on the multi-GPU schedule: they run on one GPU only "
                "(DESIGN.md §21)")

    def quantized_mlp(self, bits: int = 8) -> dict:
        """The packed layers of quantize_mlp(bits), keyed by id(layer)."""
        if bits != 8:
            raise ValueError(f"mlp_bits {bits!r}: 32 or 8")
        if self._mlp8 is None:
            raise RuntimeError("no int8 MLP layers: call quantize_mlp(8) first")
        return self._mlp8

    def _mlp_bits(self, mlp_bits: int, precision: str) -> int:
        """Validate predict's ``mlp_bits``: 32 = the ``precision`` path, 8 = the packed
        snapshot of quantize_mlp(8) (which must exist; fp32 ``precision`` only)."""
        if mlp_bits == 32:
            return 32
        if mlp_bits != 8:
            raise ValueError(f"mlp_bits {mlp_bits!r}: 32 or 8")
        if precision != "fp32":
            raise ValueError(f"mlp_bits=8 with precision={precision!r}: the int8 layers replace "
                             "the MLP operands' precision; leave precision at 'fp32'")
        self._mlp8_refusals()
        self.quantized_mlp(8)
        return 8

    def predict(self, batch: Batch, metrics=None, precision: str = "fp32",
                emb_bits: int = 32, mlp_bits: int = 32) -> torch.Tensor:
        """Forward only: prob [B_local] for ``batch`` (a device tensor owned by this batch
        size, overwritten by the next predict of it).  Writes no weight, no optimizer
        state, no gradient and no pending launch role; with ``metrics`` (a
        metrics.EvalState) the head also logs every (prob, batch.target) sample.
        ``precision`` "bf16" | "fp16": the MLP layers below the head on the 16-bit MFMA
        (predict_segments).  ``emb_bits`` 8 | 4: the embedding rows from the packed snapshot
        of quantize_embedding(emb_bits) instead of the master tables.  ``mlp_bits`` 8: every
        MLP layer, the last one included, as a dynamically quantized int8 Linear on the
        snapshot of quantize_mlp(8)."""
        for _kind, fn in self.predict_segments(batch, metrics, precision, emb_bits, mlp_bits):
            fn()
        return self._predict_bufs(self._buffers(batch.X.shape[0],
                                                batch.X.shape[0] * self.world))["prob"]

    def _predict_bufs(self, bufs):
        """The forward-only path's own outputs and GEMM workspaces of a batch size (the
        activations are the step's scratch; a workspace it might have to grow is not: a
        captured training graph keeps the addresses of the step's)."""
        pb = bufs.get("predict")
        if pb is None:
            Bl = bufs["prob"].shape[0]
            pb = bufs["predict"] = {
                "prob": torch.zeros(Bl, dtype=torch.float32, device=self.dev),
                # mlp_bits = 8: the last Linear's output and the head's weight for it
                "z8": torch.zeros((Bl, 1), dtype=torch.float32, device=self.dev),
                "one8": torch.ones(1, dtype=torch.float32, device=self.dev),
                "ws": torch.zeros(1 << 20, dtype=torch.uint8, device=self.dev),
                "ws_side": torch.zeros(1 << 20, dtype=torch.uint8, device=self.dev)}
        return pb

    def predict_segments(self, batch: Batch, metrics=None, precision: str = "fp32",
                         emb_bits: int = 32, mlp_bits: int = 32):
        """The forward-only pass as ("gpu" | "a2a" | "host", fn) items, the form of
        ``segments()`` and built from the same pieces (_build): the lookup
        (dlrm_tbe_forward; nothing of the backward's sort), the bottom MLP (one GPU: beside
        the lookup on the side stream when the "fwd" overlap is on; several: beside the
        all-to-all), the interaction (one GPU, one-hot batches: the gather-fused one, then
        no lookup launch at all), the top MLP forwards and dlrm_head_predict.

        ``precision`` "bf16" | "fp16" (the reference's --inference-only
        --quantize-mlp-with-bit 16, dlrm_s_pytorch.py:1757-1781): every bottom- and top-MLP
        layer except the head runs as one dlrm_linear16_forward launch - input and weight
        rounded to nearest-even in flight from the fp32 tensors (no weight copy exists),
        fp32 accumulate, fp32 bias and ReLU, fp32 activations; the fused bottom chain is not
        used.  The lookup, the interaction, the all-to-all and the head (its K -> 1 layer
        stays fp32) are the fp32 path's.  Only out[:, :N] of an activation buffer is
        written, so the constant-1 columns the training step relies on stay.

        ``emb_bits`` 8 | 4 (the reference's --quantize-emb-with-bit): the rows come from the
        packed snapshot quantize_embedding built (RuntimeError without one) - the
        gather-fused interaction dequantises them in registers
        (dlrm_interact_dot_forward_gather_rows, still no lookup launch), otherwise the pooled
        lookup is one dlrm_tbe_forward_rows.  It composes with every ``precision`` and with
        ``metrics``; 32 is the path above, bit for bit.

        ``mlp_bits`` 8 (the reference's --quantize-mlp-with-bit 8): every
        bottom- and top-MLP layer runs as dlrm_linear8_range + dlrm_linear8_forward on the
        packed snapshot quantize_mlp(8) built (RuntimeError without one), bitwise torch's
        dynamically quantized nn.Linear; the last layer too, as N = 1 without ReLU, and
        dlrm_head_predict keeps the sigmoid, the clamp and the metric log.  The fused bottom
        chain is not used.  It needs ``precision`` "fp32" (ValueError otherwise), composes
        with ``emb_bits`` and ``metrics``, and runs on one GPU only."""
        return self._build(batch, predict=(metrics, _precision(precision),
                                           self._emb_bits(emb_bits),
                                           self._mlp_bits(mlp_bits, precision)))

    def capture_predict(self, batch: Batch, metrics=None, pool=None, precision: str = "fp32",
                        emb_bits: int = 32, mlp_bits: int = 32):
        """A replayable forward-only pass for ``batch`` (capture()'s modes over
        predict_segments).  Run one eager predict of this batch size first (allocations).
        Each call of the returned callable scores the batch's current contents into the
        tensor predict() returns; with ``metrics`` every call appends B_local samples (the
        log's cursor lives on the device).  ``precision``, ``emb_bits``: as predict_segments
        (the graph holds the packed buffer's address; quantize_embedding re-packs in place),
        ``mlp_bits`` likewise (quantize_mlp re-packs in place)."""
        _precision(precision)
        self._emb_bits(emb_bits)
        self._mlp_bits(mlp_bits, precision)
        run, _mode, _graphs = self._capture_segments(
            lambda: self.predict_segments(batch, metrics, precision, emb_bits, mlp_bits),
            pool, None)
        return run

    def evaluate(self, batches, metrics, precision: str = "fp32", emb_bits: int = 32,
                 mlp_bits: int = 32) -> dict:
        """Score every batch into ``metrics`` (a metrics.EvalState, not reset here) and
        return its compute() dict (on several ranks: over all ranks' samples).  One graph
        per batch shape - a smaller last batch gets its own - replayed on fixed buffers the
        batches are copied into.  Index errors are checked once, at the end.
        ``precision``, ``emb_bits``, ``mlp_bits``: as predict_segments (parts of the graph
        key)."""
        _precision(precision)
        self._emb_bits(emb_bits)
        self._mlp_bits(mlp_bits, precision)
        graphs = {}
        for batch in batches:
            key = (batch.X.shape[0], batch.indices.numel(), batch.offsets.numel(),
                   self._gather_applies(batch), precision, emb_bits, mlp_bits)
            if key not in graphs:
                fixed = Batch(batch.X.clone(), batch.offsets.clone(), batch.indices.clone(),
                              batch.target.clone(), batch.max_per_table, batch.one_hot)
                self.predict(fixed, precision=precision, emb_bits=emb_bits,
                             mlp_bits=mlp_bits)  # eager, unlogged: allocations
                torch.cuda.current_stream(self.dev).synchronize()
                graphs[key] = (fixed, self.capture_predict(fixed, metrics, precision=precision,
                                                           emb_bits=emb_bits,
                                                           mlp_bits=mlp_bits))
            fixed, run = graphs[key]
            fixed.X.copy_(batch.X)
            fixed.offsets.copy_(batch.offsets)
            fixed.indices.copy_(batch.indices)
            fixed.target.copy_(batch.target)
            run()
        self.check_errors()
        return metrics.compute(group=self.pg if self.world > 1 else None)

    def check_errors(self) -> None:
        """Raise (ops.TBEIndexError / ValueError) if any step since the last check hit an
        index outside its table or exceeded max_per_table; synchronises the device.  The
        reference's EmbeddingBag raises IndexError at the bad lookup itself."""
        ops.check_tbe_errors(self.tbe_error_flag)

    # -------------------------------------------------------------- pieces --
    @staticmethod
    def _fwd(L: _Layer, h, out):
        """[h | 1] . [W | b]^T with ReLU (bias folded into the last k-term)."""
        return ops.gemm_problem(h[:, :L.Kp], L.W, trans_b=True, C=out, epilogue=ops.EPI_RELU)[0]

    @staticmethod
    def _dgrad(L: _Layer, g, inp, out):
        """dX = g W (x ReLU'(inp) when inp is given).  Widths that are not a multiple of 4
        run over Kp (the bias column's gradient lands in a column nobody reads)."""
        n = L.K if L.K % 4 == 0 else L.Kp
        if inp is not None:
            return ops.gemm_problem(g[:, :L.N], L.W[:, :n], C=out[:, :n], epilogue=ops.EPI_DRELU,
                                    aux=inp)[0]
        return ops.gemm_problem(g[:, :L.N], L.W[:, :n], C=out[:, :n])[0]

    @staticmethod
    def _wgrad(L: _Layer, g, inp, fused_opt, lr, **part):
        """[dW | db] = g^T [inp | 1]; fused SGD on one GPU.  With K % 4 == 0 the bias
        gradient is the row sum of g^T (ones_col) and the GEMM covers only the K weight
        columns; otherwise the constant-1 column of inp is multiplied like a weight column."""
        C = L.W if fused_opt else L.gW
        kw = dict(alpha=lr, epilogue=ops.EPI_SGD) if fused_opt else {}
        if L.K % 4 == 0:
            return ops.gemm_problem(g[:, :L.N], inp[:, :L.K], trans_a=True, C=C, ones_col=L.K,
                                    **kw, **part)[0]
        return ops.gemm_problem(g[:, :L.N], inp[:, :L.Kp], trans_a=True, C=C, **kw, **part)[0]

    def _wg(self, L: _Layer, g, inp, fused_opt, lr, key, last=False, full=False):
        """The wgrad of L as (problem, reduce job or None): split-K wgrads write partials
        into a per-layer buffer and their reduction (+ SGD) runs in the NEXT launch.  The
        last GEMM of the step (last=True) has no next launch to carry a reduce job: its
        K split, if any, is reduced inside its own launch (FULL mode), and so is a wgrad
        whose result is needed right after its launch (full=True)."""
        if full or (last and self.full_last_wgrad):
            return self._wgrad(L, g, inp, fused_opt, lr), None
        bufs = self._cur
        sp = bufs.setdefault("splits", {})
        if key not in sp:
            sp[key] = ops.gemm_splits(self._wgrad(L, g, inp, fused_opt, lr), partial=True)
        s = sp[key]
        if s <= 1:
            return self._wgrad(L, g, inp, fused_opt, lr), None
        parts = bufs.setdefault("partials", {})
        M, N = L.N, (L.K if L.K % 4 == 0 else L.Kp)
        need = ops.gemm_partial_bytes(M, N, s)
        if key not in parts or parts[key].numel() * 4 < need:
            parts[key] = torch.empty((need + 3) // 4, dtype=torch.float32, device=self.dev)
        pr = self._wgrad(L, g, inp, fused_opt, lr, partial=parts[key], splits=s)
        return pr, ops.reduce_problem(pr)

    def _bottom_chain(self, batch: Batch, bufs, sort_wgs: Optional[int] = None,
                      standalone: bool = False):
        """The bottom MLP forward as a dlrm_mlp_chain (None when unsupported or disabled or,
        unless it runs as its own launch (standalone), when there are no local tables to
        share the lookup launch with)."""
        if not self.fuse_bottom or (self.T_local == 0 and not standalone):
            return None
        layers = [(L.W, out, L.Kp) for L, out in zip(self.bot, bufs["bot_act"])]
        # several workgroups per 16-row block while the lookup launch still fits the
        # chip in one wave (its T_local + 1 sort workgroups beside them): small batches
        # then run the bottom MLP on 2-4x the CUs (mlp_rows.hpp, split chains)
        nrb = (batch.X.shape[0] + 15) // 16
        parts = self.bottom_parts
        others = self.T_local + 1 if sort_wgs is None else sort_wgs
        if parts <= 0:
            parts = next((p for p in (4, 2) if nrb * p + others <= self._cus), 1)
        widest = max(range(len(layers)), key=lambda i: layers[i][2] * layers[i][0].shape[0])
        if (layers[widest][0].shape[0] + 15) // 16 < parts:
            parts = 1
        if parts > 1:
            tk = bufs.get("mlp_tickets")
            if tk is None or tk.numel() < nrb:
                tk = bufs["mlp_tickets"] = torch.zeros(nrb, dtype=torch.int32,
                                                       device=self.dev)
            chain = ops.mlp_chain(batch.X, layers, parts=parts, split_layer=widest,
                                  tickets=tk)
            if ops.mlp_chain_supported(chain):
                return chain
        chain = ops.mlp_chain(batch.X, layers)
        return chain if ops.mlp_chain_supported(chain) else None

    def _ws_tbe(self, n: int) -> torch.Tensor:
        need = ops.tbe_backward_workspace_size(n, self.total_rows, self.D)
        if self._tbe_ws is None or self._tbe_ws.numel() < need:
            self._tbe_ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        return self._tbe_ws

    def _ws_head_step(self, M: int, K: int) -> torch.Tensor:
        need = int(ops._lib.query("dlrm_head_step_workspace_size", M, K))
        if self._head_step_ws is None or self._head_step_ws.numel() < need:
            self._head_step_ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        return self._head_step_ws

    # ------------------------------------------------------ communication --
    def _split_sizes(self, Bl: int):
        D = self.D
        send = [Bl * self.T_local * D] * self.world
        recv = [Bl * self.tables_per_rank[r] * D for r in range(self.world)]
        return send, recv

    def _alltoall_fwd(self, bufs, Bl):
        """All2All_Req.forward (extend_distributed.py:405-444): [B, T_r*D] -> W chunks of
        [B/W, T_s*D] in rank order.  A rank that owns no table sends nothing (its E
        buffer is a 1-table placeholder: only the first sum(send) floats take part)."""
        send, recv = self._split_sizes(Bl)
        return self.comm.a2a(bufs["recv"], bufs["E"].view(-1)[:sum(send)], recv, send)

    def _alltoall_bwd(self, bufs, Bl):
        """All2All_Wait.backward (extend_distributed.py:489-508): reverse exchange."""
        send, recv = self._split_sizes(Bl)
        return self.comm.a2a(bufs["dE"].view(-1)[:sum(send)], bufs["drecv"], send, recv)

    def lookup_balance(self, B: int, L: int = 1):
        """Per-rank load of the table-wise sharding: tables, rows and lookups per step
        (greedy balances rows, not lookups: SURVEY.md §7 hard part 6)."""
        rows = [0] * self.world
        tabs = [0] * self.world
        for t, r in enumerate(self.device_indices):
            rows[r] += int(self.cfg.ln_emb[t])
            tabs[r] += 1
        look = [n * B * L for n in tabs]
        mean = sum(look) / max(self.world, 1)
        return {"tables": tabs, "rows": rows, "lookups": look,
                "lookup_max_over_mean": round(max(look) / mean, 3) if mean else None}

_EMPTY = object()  # returned by a "gpu" segment that enqueued nothing this step


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class _Done:
    def wait(self):
        return None


class TorchComm:
    """The step's collectives on torch.distributed (backend nccl = RCCL over xGMI).  The
    all-to-all runs on the trainer's process group; the dense all-reduce on a SECOND
    group of the same ranks (its own communicator, so its own stream): a 9.5 MB gradient
    all-reduce in flight never queues the reverse all-to-all the embedding update waits
    for.  gloo groups with CUDA tensors (tests: several ranks on one GPU) stage through
    the host, synchronously."""

    def __init__(self, pg, dense_pg=None, separate_dense: bool = True):
        """``separate_dense`` False: the all-reduces share the all-to-all's communicator
        (one stream; the fallback if two concurrent communicators misbehave at W > 1 -
        that overlap has run on 1-rank RCCL and multi-rank gloo only)."""
        import torch.distributed as dist
        self.pg = pg
        if dense_pg is None:
            if separate_dense:
                # the SAME ranks as pg (global rank ids: pg need not be WORLD)
                dense_pg = dist.new_group(ranks=dist.get_process_group_ranks(pg),
                                          backend=dist.get_backend(pg))
            else:
                dense_pg = pg
        self.dense_pg = dense_pg
        # What captures into a hipGraph on this stack (tools/rccl_capture_probe.py,
        # profiles/r06_rccl_capture_probe.txt): RCCL all-reduces (sync or async + wait, on
        # either communicator) and all-gathers capture and replay correctly; an
        # all_to_all_single - warmed eagerly first or not - crashes hipStreamEndCapture
        # (unbounded recursion inside libamdhip64).  So the all-reduces ride inside the
        # step's graphs and only the two all-to-alls run eagerly between them (the
        # round-5 "hang" was this crash in a spawned test worker, its parent waiting on a
        # queue that never filled).  gloo: nothing captures.
        nccl = dist.get_backend(pg) == "nccl" and dist.get_backend(dense_pg) == "nccl"
        self.capturable = False
        self.capture_ar = nccl

    def a2a(self, out: torch.Tensor, inp: torch.Tensor, out_splits, in_splits):
        import torch.distributed as dist
        if out.is_cuda and dist.get_backend(self.pg) == "gloo":
            o = torch.empty(out.shape, dtype=out.dtype)
            dist.all_to_all_single(o, inp.cpu(), out_splits, in_splits, group=self.pg)
            out.copy_(o)
            return _Done()
        return dist.all_to_all_single(out, inp, out_splits, in_splits, group=self.pg,
                                      async_op=True)

    def allreduce(self, t: torch.Tensor):
        import torch.distributed as dist
        if t.is_cuda and dist.get_backend(self.dense_pg) == "gloo":
            h = t.cpu()
            dist.all_reduce(h, group=self.dense_pg)
            t.copy_(h)
            return _Done()
        return dist.all_reduce(t, group=self.dense_pg, async_op=True)


class EmulatedComm:
    """Rank r of a W-rank job on ONE GPU with no peers (bench --emulate-world): every
    kernel of the step runs at rank r's W-rank shapes (its tables over the global batch,
    the B/W local batch, the rank-major features).  The all-to-all becomes one device copy
    of min(send, recv) bytes on the current stream (the rest of the receive buffer keeps
    whatever it holds); the all-reduce does nothing.  Times the rank's own work, not the
    fabric.  By default it captures like RCCL does (``capture_ar``: the all-reduces inside
    the step's graphs, the all-to-alls eager between four graphs), so the projection pays
    the same graph boundaries as the real path; ``whole=True``: one graph (what the step
    would cost if RCCL's all-to-all captured)."""

    def __init__(self, whole: bool = False):
        self.capturable = bool(whole)
        self.capture_ar = True

    def a2a(self, out: torch.Tensor, inp: torch.Tensor, out_splits, in_splits):
        n = min(int(sum(out_splits)), int(sum(in_splits)))
        if n:
            out.view(-1)[:n].copy_(inp.reshape(-1)[:n])
        return _Done()

    def allreduce(self, t: torch.Tensor):
        return _Done()
