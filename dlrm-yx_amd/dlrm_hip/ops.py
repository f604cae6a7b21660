"""Tensor-level launchers over the C-ABI (one function per dlrm_* entry point).

Every launcher enqueues on ``torch.cuda.current_stream()`` and returns without
synchronising; all device buffers (outputs, workspaces) are allocated here by the
torch caching allocator and handed to the C-ABI as raw pointers.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import _lib

EPI_STORE, EPI_BIAS, EPI_BIAS_RELU, EPI_DRELU, EPI_SGD, EPI_ACCUM, EPI_RELU = range(7)
TBE_ERR_INDEX, TBE_ERR_TABLE_CAP = 1, 2  # dlrm_tbe_error bits


class TBEIndexError(IndexError):
    """Raised by check_tbe_errors: the reference's EmbeddingBag raises IndexError for an
    index outside its table; the device kernels skip such lookups and flag them."""


def check_tbe_errors(flag: torch.Tensor, reset: bool = True) -> None:
    """Read a TBE error flag (synchronises with its stream) and raise on any bit."""
    v = int(flag.item())
    if reset:
        flag.zero_()
    if v & TBE_ERR_INDEX:
        raise TBEIndexError("embedding index out of range for its table (lookup skipped)")
    if v & TBE_ERR_TABLE_CAP:
        raise ValueError("a table had more lookups than max_lookups_per_table "
                         "(its backward update was skipped)")


def _raise_bits(v: int) -> None:
    if v & TBE_ERR_INDEX:
        raise TBEIndexError("embedding index out of range for its table (lookup skipped)")
    if v & TBE_ERR_TABLE_CAP:
        raise ValueError("a table had more lookups than max_lookups_per_table "
                         "(its backward update was skipped)")


class DeferredErrorCheck:
    """Reads a TBE error flag without a host sync on the calling step: ``post()`` enqueues
    an async copy of the flag into pinned host memory (then clears it) and records an event;
    ``poll()`` - at the next call, by then long complete - raises on what the previous call
    flagged.  ``flush()`` waits for the last copy and raises (end of training / tests).
    Skipped while the stream is being captured into a graph."""

    def __init__(self):
        self._host = None
        self._event = None

    def poll(self) -> None:
        if self._event is None:
            return
        self._event.synchronize()  # recorded a call ago: normally already complete
        self._event = None
        v = int(self._host[0])
        self._host[0] = 0
        _raise_bits(v)

    def post(self, flag: torch.Tensor) -> None:
        if torch.cuda.is_current_stream_capturing():
            return
        if self._host is None:
            self._host = torch.zeros(1, dtype=torch.int32, pin_memory=True)
            self._event = None
        self._host.copy_(flag, non_blocking=True)
        flag.zero_()
        self._event = torch.cuda.Event()
        self._event.record()

    def flush(self) -> None:
        self.poll()


# dlrm_tune_key (include/dlrm_hip.h): plan overrides for sweeps and coverage tests
TUNE_KEYS = {"gemm_tile": 1, "gemm_split": 2, "tbe_block": 3, "tbe_sort": 4, "tbe_lean": 5,
             "interact_bwd": 6, "interact_fwd": 7, "linear16_tile": 8, "linear16_dgrad_tile": 9,
             "linear16_wgrad_tile": 10, "linear16_wgrad_split": 11, "linear8_tile": 12}


class tuning:
    """Context manager over dlrm_set_tuning (thread-local plan overrides; results stay
    exact, only the plan changes), e.g. ``with ops.tuning(gemm_tile=64064, gemm_split=4):``
    or ``tuning(tbe_block=64)``; the previous values are restored on exit."""

    def __init__(self, **kw):
        for k in kw:
            if k not in TUNE_KEYS:
                raise KeyError(f"unknown tuning key {k!r} (one of {sorted(TUNE_KEYS)})")
        self.kw = kw
        self.prev = {}

    def __enter__(self):
        lib = _lib.load()
        for k, v in self.kw.items():
            self.prev[k] = int(lib.dlrm_get_tuning(TUNE_KEYS[k]))
            _lib.call("dlrm_set_tuning", TUNE_KEYS[k], int(v))
        return self

    def __exit__(self, *a):
        for k, v in self.prev.items():
            _lib.call("dlrm_set_tuning", TUNE_KEYS[k], int(v))
        return False


LOSS_MSE, LOSS_BCE = 0, 1
QR_OPS = {"mult": 0, "add": 1, "concat": 2}


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _lr_dev(lr, what: str = "lr"):
    """A learning-rate argument is a Python float (baked into the kernel arguments, so into a
    captured graph) or a 1-element fp32 device tensor, e.g. ``LRState.lr(k)`` (ABI v14: read
    when the kernel runs; the caller keeps it alive and orders its writer before the
    consumer).  Returns the tensor's device pointer, or None for a float."""
    if not isinstance(lr, torch.Tensor):
        return None
    if lr.dtype != torch.float32 or lr.numel() != 1 or not lr.is_cuda:
        raise ValueError(f"{what}: a float or a 1-element fp32 device tensor "
                         f"(got {lr.dtype}, {lr.numel()} elements, {lr.device})")
    return ctypes.c_void_p(lr.data_ptr())


def _stream(device: Optional[torch.device] = None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _check_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("dlrm_hip ops take device tensors (got a CPU tensor)")


def _bits(t: torch.Tensor) -> int:
    if t.dtype == torch.int32:
        return 32
    if t.dtype == torch.int64:
        return 64
    raise TypeError(f"index/offset tensors must be int32 or int64, got {t.dtype}")


class Workspace:
    """Grow-only device scratch buffer (one per owner, reused across calls).  Zeroed when
    allocated: the GEMM split-K tickets at its start must begin at 0 (the kernels leave
    them at 0 after every launch)."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None

    def get(self, nbytes: int, device) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != torch.device(device):
            self.buf = torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        return self.buf


_default_ws = {}


def _ws(tag: str, nbytes: int, device) -> torch.Tensor:
    key = (tag, str(device))
    w = _default_ws.get(key)
    if w is None:
        w = _default_ws[key] = Workspace()
    return w.get(nbytes, device)


# ------------------------------------------------------------------ TBE ----
def tbe_forward(weights: torch.Tensor, row_base: torch.Tensor, T: int, B: int,
                indices: torch.Tensor, offsets: torch.Tensor,
                per_sample_weights: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, out_batch_stride: Optional[int] = None,
                error_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Pooled-sum lookup -> [B, T, D] (or into ``out`` with a custom batch stride)."""
    _check_cuda(weights, row_base, indices, offsets, per_sample_weights)
    D = weights.shape[1]
    if out is None:
        out = torch.empty((B, T, D), dtype=torch.float32, device=weights.device)
        out_batch_stride = T * D
    elif out_batch_stride is None:
        out_batch_stride = T * D
    _lib.call("dlrm_tbe_forward", _p(weights), D, _p(row_base), T, B, _p(indices),
              _bits(indices), _p(offsets), _bits(offsets), _p(per_sample_weights), _p(out),
              out_batch_stride, _p(error_flag), _stream(weights.device))
    return out


def mlp_chain(X: torch.Tensor, layers, parts: int = 1, split_layer: int = -1,
              tickets: Optional[torch.Tensor] = None) -> "_lib.MlpChain":
    """dlrm_mlp_chain for a bias-folded Linear+ReLU stack: ``X`` [rows, >= in_width[0]]
    carries its own bias column; ``layers`` = [(W [n, >= kin], Y [rows, >= n], kin)].
    ``parts`` 2 / 4: that many workgroups per 16-row block, splitting layer ``split_layer``
    (default: the largest in_width * out_width) by output columns; ``tickets``: zeroed int32
    [ceil(rows / 16)] device buffer owned by this chain (allocated when None)."""
    c = _lib.MlpChain()
    if parts > 1:
        if split_layer < 0:
            split_layer = max(range(len(layers)), key=lambda i: layers[i][2] * layers[i][0].shape[0])
        if tickets is None:
            tickets = torch.zeros((X.shape[0] + 15) // 16, dtype=torch.int32, device=X.device)
        c.parts, c.split_layer, c.tickets = int(parts), int(split_layer), tickets.data_ptr()
        c._keep = tickets  # the chain struct refers to it
    c.layers = len(layers)
    c.rows = X.shape[0]
    c.X = X.data_ptr()
    c.ldx = X.stride(0)
    for i, (W, Y, kin) in enumerate(layers):
        c.in_width[i] = int(kin)
        c.out_width[i] = W.shape[0]
        c.W[i] = W.data_ptr()
        c.ldw[i] = W.stride(0)
        c.Y[i] = Y.data_ptr()
        c.ldy[i] = Y.stride(0)
    return c


def mlp_chain_supported(chain) -> bool:
    return bool(_lib.load().dlrm_mlp_chain_supported(ctypes.byref(chain)))


def mlp_chain_forward(chain, device=None) -> None:
    """Every layer of the chain in one launch (dlrm_mlp_chain_forward)."""
    dev = device if device is not None else torch.cuda.current_device()
    _lib.call("dlrm_mlp_chain_forward", ctypes.cast(ctypes.byref(chain), ctypes.c_void_p),
              _stream(dev))


# the TBE backward's sort keys are 32-bit global rows (ABI v4): a table set that one
# backward call serves must hold fewer rows (checked where tables are built, so a forward
# is never accepted for a configuration the backward would refuse)
TBE_MAX_ROWS = 0xFFFFFFFF - 1


def check_tbe_rows(total_rows: int, what: str) -> None:
    if int(total_rows) > TBE_MAX_ROWS:
        raise ValueError(f"{what}: {int(total_rows)} rows in one table-batched buffer; the "
                         f"embedding backward supports < 2^32 - 1 rows per call (shard the "
                         f"tables over more ranks or modules)")


# lookups per table the in-launch per-table sort handles (tbe_bwd.hip kSegCap)
TBE_PRESORT_SEG_CAP = 4096


def tbe_forward_presort(weights: torch.Tensor, row_base: torch.Tensor, T: int, B: int,
                        indices: torch.Tensor, offsets: torch.Tensor, workspace: torch.Tensor,
                        max_lookups_per_table: int, out: Optional[torch.Tensor] = None,
                        out_batch_stride: Optional[int] = None,
                        per_sample_weights: Optional[torch.Tensor] = None,
                        error_flag: Optional[torch.Tensor] = None, bottom=None,
                        lookup: bool = True) -> Optional[torch.Tensor]:
    """tbe_forward + this batch's backward sort in one launch (dlrm_tbe_forward_presort);
    follow with tbe_backward(..., workspace, presorted=True).  ``bottom``: an mlp_chain
    (the bottom MLP forward) run as a third role of the same launch.

    ``lookup=False``: the sort-only launch (the C-ABI's ``out = NULL``): no pooled output
    is allocated or written, the lookup is done by its consumer (the gather-fused dot
    interaction); returns None.  Only valid where the per-table sort applies (the library
    returns DLRM_ERR_UNSUPPORTED otherwise)."""
    _check_cuda(weights, row_base, indices, offsets, workspace, per_sample_weights)
    D = weights.shape[1]
    if not lookup:
        if out is not None:
            raise ValueError("tbe_forward_presort: lookup=False takes no out tensor")
        out_batch_stride = T * D
    elif out is None:
        out = torch.empty((B, T, D), dtype=torch.float32, device=weights.device)
        out_batch_stride = T * D
    elif out_batch_stride is None:
        out_batch_stride = T * D
    _lib.call("dlrm_tbe_forward_presort", _p(weights), D, _p(row_base), T, B, _p(indices),
              _bits(indices), _p(offsets), _bits(offsets), _p(per_sample_weights), _p(out),
              out_batch_stride, indices.numel(), weights.shape[0], int(max_lookups_per_table),
              _p(workspace), workspace.numel(), _p(error_flag),
              ctypes.cast(ctypes.byref(bottom), ctypes.c_void_p) if bottom is not None else None,
              _stream(weights.device))
    return out


def tbe_psw_grad(weights: torch.Tensor, row_base: torch.Tensor, T: int, B: int,
                 indices: torch.Tensor, offsets: torch.Tensor, grad_out: torch.Tensor,
                 grad_batch_stride: Optional[int] = None) -> torch.Tensor:
    """d loss / d per_sample_weights of a weighted lookup (dlrm_tbe_psw_grad)."""
    _check_cuda(weights, row_base, indices, offsets, grad_out)
    D = weights.shape[1]
    if grad_batch_stride is None:
        grad_batch_stride = T * D
    g = torch.empty(indices.numel(), dtype=torch.float32, device=weights.device)
    _lib.call("dlrm_tbe_psw_grad", _p(weights), D, _p(row_base), T, B, _p(indices),
              _bits(indices), _p(offsets), _bits(offsets), indices.numel(), _p(grad_out),
              grad_batch_stride, _p(g), _stream(weights.device))
    return g


ROWS_F32, ROWS_F16, ROWS_Q8, ROWS_Q4 = 0, 1, 2, 3


def tbe_row_bytes(fmt: int, D: int) -> int:
    return int(_lib.load().dlrm_tbe_row_bytes(fmt, D))


def tbe_forward_rows(weights: torch.Tensor, fmt: int, D: int, row_base: torch.Tensor, T: int,
                     B: int, indices: torch.Tensor, offsets: torch.Tensor,
                     per_sample_weights: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None, out_batch_stride: Optional[int] = None,
                     error_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dlrm_tbe_forward_rows: table-batched pooled lookup over F16 rows ([rows, D] half) or
    row-wise quantized rows ([rows, row_bytes] uint8, torch.ops.quantized prepack layout)."""
    _check_cuda(weights, row_base, indices, offsets, per_sample_weights)
    if fmt == ROWS_F16:
        assert weights.dtype == torch.float16 and weights.shape[1] == D
        row_bytes = 2 * weights.stride(0)
    else:
        assert weights.dtype == torch.uint8 and weights.dim() == 2
        row_bytes = weights.stride(0)
    if out is None:
        out = torch.empty((B, T, D), dtype=torch.float32, device=weights.device)
        out_batch_stride = T * D
    elif out_batch_stride is None:
        out_batch_stride = T * D
    _lib.call("dlrm_tbe_forward_rows", _p(weights), fmt, row_bytes, D, _p(row_base), T, B,
              _p(indices), _bits(indices), _p(offsets), _bits(offsets), _p(per_sample_weights),
              _p(out), out_batch_stride, _p(error_flag), _stream(weights.device))
    return out


def quant_format(bits: int) -> int:
    """ROWS_Q8 | ROWS_Q4 for a width of 8 | 4 bits (ValueError otherwise)."""
    if bits not in (4, 8):
        raise ValueError(f"row-wise quantized rows are 8 or 4 bits wide, not {bits!r}")
    return ROWS_Q4 if bits == 4 else ROWS_Q8


def rows_quantize(src: torch.Tensor, bits: int,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dlrm_rows_quantize: [rows, D] fp32 or fp16 rows packed row-wise to ``bits`` (8 | 4) on
    the device, bitwise torch.ops.quantized.embedding_bag_byte_prepack /
    embedding_bag_4bit_prepack of the same rows as fp32.  Returns uint8 [rows, row_bytes]
    (``out``: such a contiguous tensor to fill), the layout tbe_forward_rows and
    interact_forward_gather_rows read."""
    fmt = quant_format(bits)
    if src.dtype not in (torch.float32, torch.float16) or src.dim() != 2 \
            or not src.is_contiguous():
        raise ValueError("rows_quantize: contiguous [rows, D] fp32 or fp16 rows, not "
                         f"{src.dtype} {tuple(src.shape)}")
    _check_cuda(src, out)
    rows, D = src.shape
    row_bytes = tbe_row_bytes(fmt, D)
    if out is None:
        out = torch.empty((rows, row_bytes), dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (rows, row_bytes) \
            or not out.is_contiguous():
        raise ValueError(f"rows_quantize: out must be contiguous uint8 [{rows}, {row_bytes}]")
    _lib.call("dlrm_rows_quantize", _p(src), ROWS_F32 if src.dtype == torch.float32 else ROWS_F16,
              rows, D, fmt, _p(out), row_bytes, _stream(src.device))
    return out


def tbe_backward_workspace_size(num_lookups: int, total_rows: int, D: int) -> int:
    return _lib.query("dlrm_tbe_backward_workspace_size", num_lookups, total_rows, D)


PRESORTED_ANY = 2  # DLRM_PRESORTED_ANY


def _tbe_bwd_args(weights, row_base, T, B, indices, offsets, per_sample_weights, workspace,
                  max_lookups_per_table, error_flag, grad=None):
    """What the backward entry points share, as (head, tail) of their argument lists: head is
    D .. per_sample_weights, then ``grad`` = (grad_out, its batch stride or None for T * D)
    where there is a gradient; tail is the table bound, the workspace (by default this
    module's own, grown to the call's size), its size and the error flag."""
    D, N, total_rows = weights.shape[1], indices.numel(), weights.shape[0]
    head = (D, _p(row_base), T, B, _p(indices), _bits(indices), _p(offsets), _bits(offsets), N,
            total_rows, _p(per_sample_weights))
    if grad is not None:
        head += (_p(grad[0]), T * D if grad[1] is None else grad[1])
    if workspace is None:
        workspace = _ws("tbe_bwd", tbe_backward_workspace_size(N, total_rows, D), weights.device)
    return head, (int(max_lookups_per_table), _p(workspace), workspace.numel(), _p(error_flag))


# tbe_backward's entry points: the name, whether momentum= is passed, how the rate is passed
# ("split": the float to the entry or the device pointer to its _dev twin; "both": the float,
# 0 beside a device rate, and the pointer; None: no rate), and whether eps is passed
_TBE_BWD = {
    "sgd": ("dlrm_tbe_backward_sgd", False, "split", False),
    "sgd_f16": ("dlrm_tbe_backward_sgd_f16", False, "split", False),
    "rowwise_adagrad": ("dlrm_tbe_backward_rowwise_adagrad", True, "split", True),
    "adagrad": ("dlrm_tbe_backward_adagrad", True, "both", True),
    "dense": ("dlrm_tbe_backward_dense", False, None, False),
}
_TBE_BWD_SR = ("dlrm_tbe_backward_sgd_f16_sr", False, "both", False)  # then the sr state


def tbe_backward_sort(weights: torch.Tensor, row_base: torch.Tensor, T: int, B: int,
                      indices: torch.Tensor, offsets: torch.Tensor, workspace: torch.Tensor,
                      max_lookups_per_table: int = 0,
                      per_sample_weights: Optional[torch.Tensor] = None,
                      error_flag: Optional[torch.Tensor] = None) -> None:
    """The backward's sort alone (dlrm_tbe_backward_sort): it depends only on the indices,
    so it can run early (e.g. on a side stream beside the forward); follow with
    tbe_backward(..., workspace, presorted=PRESORTED_ANY) of the same batch (same bound and
    per_sample_weights nullness)."""
    _check_cuda(weights, row_base, indices, offsets, workspace, per_sample_weights)
    head, tail = _tbe_bwd_args(weights, row_base, T, B, indices, offsets, per_sample_weights,
                               workspace, max_lookups_per_table, error_flag)
    _lib.call("dlrm_tbe_backward_sort", *head, *tail, _stream(weights.device))


def tbe_backward(mode: str, weights: torch.Tensor, row_base: torch.Tensor, T: int, B: int,
                 indices: torch.Tensor, offsets: torch.Tensor, grad_out: torch.Tensor,
                 lr=0.0, eps: float = 0.0, momentum: Optional[torch.Tensor] = None,
                 per_sample_weights: Optional[torch.Tensor] = None,
                 grad_batch_stride: Optional[int] = None,
                 workspace: Optional[torch.Tensor] = None,
                 max_lookups_per_table: int = 0,
                 error_flag: Optional[torch.Tensor] = None, presorted: int = False,
                 sr_state: Optional[torch.Tensor] = None) -> None:
    """mode: 'sgd' (fused exact SGD; fp32 or fp16 weights; 'sgd_f16' names the fp16 case and
    refuses fp32 weights), 'rowwise_adagrad' (fused
    RWSAdagrad), 'adagrad' (fused element-wise torch.optim.Adagrad on fp32 weights;
    ``momentum`` is its "sum" state, contiguous fp32 of the weights' shape, and the result
    equals 'dense' into a zero buffer followed by adagrad_update over the whole table, bit
    for bit) or 'dense' (weights is a gradient buffer to accumulate into).  max_lookups_per_table:
    upper bound on any table's lookups (0 = unknown); <= 4096 selects the per-table LDS
    sort (bitwise the same result as the device-wide radix sort).  ``error_flag``: device
    int32 that receives TBE_ERR_INDEX / TBE_ERR_TABLE_CAP bits (see check_tbe_errors).
    ``presorted``: True - the per-table sort ran in tbe_forward_presort; PRESORTED_ANY -
    tbe_backward_sort ran for this batch.  ``lr``: a float, or ('sgd', fp32 or fp16
    weights, 'rowwise_adagrad' and 'adagrad') a 1-element fp32 device tensor read when the
    kernels run.
    ``sr_state`` (fp16 weights only; ops.sr_state): the updated row is stored rounded
    stochastically with the state's (seed, step) stream instead of to nearest even
    (dlrm_tbe_backward_sgd_f16_sr); the state is read when the kernels run, never written."""
    _check_cuda(weights, row_base, indices, offsets, grad_out, momentum, per_sample_weights)
    lr_dev = _lr_dev(lr, "tbe_backward: lr")
    if sr_state is not None and not (mode in ("sgd", "sgd_f16")
                                     and weights.dtype == torch.float16):
        raise ValueError("tbe_backward: sr_state goes with 'sgd' / 'sgd_f16' on fp16 weights")
    head, tail = _tbe_bwd_args(weights, row_base, T, B, indices, offsets, per_sample_weights,
                               workspace, max_lookups_per_table, error_flag,
                               (grad_out, grad_batch_stride))
    if mode == "sgd_f16" and weights.dtype != torch.float16:
        raise ValueError("tbe_backward: mode 'sgd_f16' takes fp16 weights")
    if sr_state is not None:
        entry = _TBE_BWD_SR
    elif mode in ("sgd", "sgd_f16") and weights.dtype == torch.float16:
        entry = _TBE_BWD["sgd_f16"]
    elif mode in _TBE_BWD:
        entry = _TBE_BWD[mode]
    else:
        raise ValueError(mode)
    if mode == "adagrad":
        if weights.dtype != torch.float32:
            raise ValueError("tbe_backward: mode 'adagrad' takes fp32 weights")
        if (momentum is None or momentum.dtype != torch.float32
                or tuple(momentum.shape) != tuple(weights.shape)
                or not momentum.is_contiguous()):
            raise ValueError("tbe_backward: mode 'adagrad' takes its state as momentum=, a "
                             f"contiguous fp32 tensor of the weights' shape "
                             f"{tuple(weights.shape)}")
    name, with_state, rate_as, with_eps = entry
    rate = ()
    if rate_as == "both":
        rate = (0.0 if lr_dev is not None else lr, lr_dev)
    elif rate_as == "split":
        rate = (lr,) if lr_dev is None else (lr_dev,)
        name += "" if lr_dev is None else "_dev"
    if sr_state is not None:
        rate += (_sr_ptr(sr_state, "tbe_backward"),)
    _lib.call(name, _p(weights), *((_p(momentum),) if with_state else ()), *head, *rate,
              *((eps,) if with_eps else ()), *tail, int(presorted), _stream(weights.device))


def tbe_backward_defer(mode: str, weights: torch.Tensor, row_base: torch.Tensor, T: int, B: int,
                       indices: torch.Tensor, offsets: torch.Tensor, grad_out: torch.Tensor,
                       lr=0.0, eps: float = 0.0,
                       momentum: Optional[torch.Tensor] = None,
                       per_sample_weights: Optional[torch.Tensor] = None,
                       grad_batch_stride: Optional[int] = None,
                       workspace: Optional[torch.Tensor] = None,
                       max_lookups_per_table: int = 0,
                       error_flag: Optional[torch.Tensor] = None, presorted: bool = False):
    """tbe_backward ('sgd' on fp32 weights or 'rowwise_adagrad') with its two update passes
    deferred (dlrm_tbe_backward_defer): returns the role to hand to gemm_group(...,
    role=, phase=1) and then phase=2 - or None when the update already ran in full (shape
    the fused passes do not cover).  The workspace, weights, momentum and grad_out must stay
    untouched until phase 2 has run.  ``lr``: a float or a 1-element fp32 device tensor (the
    role then carries its address: both passes read it when their launch runs)."""
    _check_cuda(weights, row_base, indices, offsets, grad_out, momentum, per_sample_weights)
    if weights.dtype != torch.float32 or mode not in ("sgd", "rowwise_adagrad"):
        raise ValueError("tbe_backward_defer: fp32 'sgd' or 'rowwise_adagrad' only")
    head, tail = _tbe_bwd_args(weights, row_base, T, B, indices, offsets, per_sample_weights,
                               workspace, max_lookups_per_table, error_flag,
                               (grad_out, grad_batch_stride))
    role = _lib.LaunchRole()
    lr_dev = _lr_dev(lr, "tbe_backward_defer: lr")
    _lib.call("dlrm_tbe_backward_defer" if lr_dev is None else "dlrm_tbe_backward_defer_dev",
              0 if mode == "sgd" else 1, _p(weights), _p(momentum), *head,
              lr if lr_dev is None else lr_dev, eps, *tail, int(presorted), ctypes.byref(role),
              _stream(weights.device))
    return role if role_blocks(role) > 0 else None


def role_blocks(role) -> int:
    """Workgroups a deferred update pass adds to the launch carrying it (0: none)."""
    return 0 if role is None else _lib.query("dlrm_role_blocks", ctypes.byref(role))


def tbe_expand_grad(D: int, T: int, B: int, offsets: torch.Tensor, num_lookups: int,
                    grad_out: torch.Tensor, per_sample_weights: Optional[torch.Tensor] = None,
                    grad_batch_stride: Optional[int] = None) -> torch.Tensor:
    _check_cuda(offsets, grad_out, per_sample_weights)
    values = torch.empty((num_lookups, D), dtype=torch.float32, device=grad_out.device)
    if grad_batch_stride is None:
        grad_batch_stride = T * D
    _lib.call("dlrm_tbe_expand_grad", D, T, B, _p(offsets), _bits(offsets), num_lookups,
              _p(per_sample_weights), _p(grad_out), grad_batch_stride, _p(values),
              _stream(grad_out.device))
    return values


# ------------------------------------------------------------------- QR ----
def qr_split_indices(indices: torch.Tensor, collisions: int):
    _check_cuda(indices)
    n = indices.numel()
    q = torch.empty(n, dtype=torch.int64, device=indices.device)
    r = torch.empty(n, dtype=torch.int64, device=indices.device)
    _lib.call("dlrm_qr_split_indices", _p(indices), _bits(indices), n, collisions, _p(q), _p(r),
              _stream(indices.device))
    return q, r


def qr_combine_forward(op: str, eq: torch.Tensor, er: torch.Tensor) -> torch.Tensor:
    n, D = eq.shape
    out = torch.empty((n, 2 * D if op == "concat" else D), dtype=torch.float32, device=eq.device)
    _lib.call("dlrm_qr_combine_forward", QR_OPS[op], n, D, _p(eq), _p(er), _p(out),
              _stream(eq.device))
    return out


def qr_combine_backward(op: str, eq: torch.Tensor, er: torch.Tensor, grad_out: torch.Tensor):
    n, D = eq.shape
    geq = torch.empty_like(eq)
    ger = torch.empty_like(er)
    _lib.call("dlrm_qr_combine_backward", QR_OPS[op], n, D, _p(eq), _p(er),
              _p(grad_out.contiguous()), _p(geq), _p(ger), _stream(eq.device))
    return geq, ger


def qr_expand_csr(T_phys: int, B: int, indices: torch.Tensor, offsets: torch.Tensor,
                  src: torch.Tensor, kind: torch.Tensor, coll: torch.Tensor,
                  max_lookups_per_table: int, phys_indices: torch.Tensor,
                  phys_offsets: torch.Tensor, error_flag: Optional[torch.Tensor] = None) -> None:
    """Logical table-batched CSR -> the physical CSR of the QR engine (dlrm_qr_expand_csr):
    physical table p = logical table src[p]'s bags with its indices (kind 0), quotients
    (kind 1) or remainders (kind 2) by coll[p]; int32 outputs.  Lookups past
    phys_indices.numel() are dropped and raise TBE_ERR_TABLE_CAP in ``error_flag``."""
    _check_cuda(indices, offsets, src, kind, coll, phys_indices, phys_offsets)
    _lib.call("dlrm_qr_expand_csr", T_phys, B, _p(indices), _bits(indices), _p(offsets),
              _bits(offsets), _p(src), _p(kind), _p(coll), int(max_lookups_per_table),
              _p(phys_indices), _p(phys_offsets), phys_indices.numel(), _p(error_flag),
              _stream(indices.device))


def qr_pool_combine_forward(op: str, T: int, B: int, D: int, pq: torch.Tensor, pr: torch.Tensor,
                            P: torch.Tensor, E: torch.Tensor) -> None:
    """E[b, t] = op(P[b, pq[t]], P[b, pr[t]]) (or P[b, pq[t]] where pr[t] < 0)."""
    _lib.call("dlrm_qr_pool_combine_forward", QR_OPS[op], T, B, D, _p(pq), _p(pr), _p(P),
              P.stride(0), _p(E), E.stride(0), _stream(P.device))


def qr_pool_combine_backward(op: str, T: int, B: int, D: int, pq: torch.Tensor,
                             pr: torch.Tensor, P: torch.Tensor, dE: torch.Tensor,
                             dP: torch.Tensor) -> None:
    _lib.call("dlrm_qr_pool_combine_backward", QR_OPS[op], T, B, D, _p(pq), _p(pr), _p(P),
              P.stride(0), _p(dE), dE.stride(0), _p(dP), dP.stride(0), _stream(P.device))


# ---------------------------------------------------------- interaction ----
def _feature_arrays(feats: Sequence[torch.Tensor], strides: Sequence[int]):
    F = len(feats)
    ptrs = (ctypes.c_void_p * F)(*[t.data_ptr() for t in feats])
    bs = (ctypes.c_int64 * F)(*[int(s) for s in strides])
    return ptrs, bs


def feature_views(x: torch.Tensor, ly) -> tuple:
    """(tensors, batch strides, D) for feature 0 = x and ly = [B,T,D] tensor or list of [B,D]."""
    feats = [x]
    strides = [x.stride(0)]
    if isinstance(ly, torch.Tensor):
        ly = [ly]
    for y in ly:
        if y.dim() == 3:  # [B, T, D], rows contiguous in D
            if y.stride(2) != 1:
                raise ValueError("interaction features must be contiguous in D")
            for t in range(y.shape[1]):
                feats.append(y[:, t, :])
                strides.append(y.stride(0))
        else:
            if y.stride(1) != 1:
                raise ValueError("interaction features must be contiguous in D")
            feats.append(y)
            strides.append(y.stride(0))
    return feats, strides


def interact_forward(op: str, x: torch.Tensor, ly, self_interaction: bool = False,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    feats, strides = feature_views(x, ly)
    _check_cuda(*feats)
    B, D = x.shape
    F = len(feats)
    ptrs, bs = _feature_arrays(feats, strides)
    if op == "dot":
        npairs = F * (F + 1) // 2 if self_interaction else F * (F - 1) // 2
        if out is None:
            out = torch.empty((B, D + npairs), dtype=torch.float32, device=x.device)
        _lib.call("dlrm_interact_dot_forward", B, F, D, ptrs, bs, int(self_interaction), _p(out),
                  out.stride(0), _stream(x.device))
    elif op == "cat":
        if out is None:
            out = torch.empty((B, F * D), dtype=torch.float32, device=x.device)
        _lib.call("dlrm_interact_cat_forward", B, F, D, ptrs, bs, _p(out), out.stride(0),
                  _stream(x.device))
    else:
        raise ValueError(op)
    return out


def interact_backward(op: str, x: torch.Tensor, ly, grad_out: torch.Tensor,
                      self_interaction: bool = False, grad_x: Optional[torch.Tensor] = None,
                      grad_ly=None, relu_x: bool = False):
    """Returns (grad_x, grad_ly) with grad_ly shaped like ly ([B,T,D] or list of [B,D]).
    relu_x: grad_x also gets ReLU'(x) applied (x = output of a ReLU layer; dot only)."""
    feats, strides = feature_views(x, ly)
    B, D = x.shape
    F = len(feats)
    if grad_x is None:
        grad_x = torch.empty_like(x, memory_format=torch.contiguous_format)
    if grad_ly is None:
        if isinstance(ly, torch.Tensor):
            grad_ly = torch.empty(ly.shape, dtype=torch.float32, device=x.device)
        else:
            grad_ly = [torch.empty(y.shape, dtype=torch.float32, device=x.device) for y in ly]
    gfeats, gstrides = feature_views(grad_x, grad_ly)
    ptrs, bs = _feature_arrays(feats, strides)
    gptrs, gbs = _feature_arrays(gfeats, gstrides)
    g = grad_out if grad_out.stride(1) == 1 else grad_out.contiguous()  # row stride is passed
    if op == "dot":
        _lib.call("dlrm_interact_dot_backward", B, F, D, ptrs, bs, int(self_interaction), _p(g),
                  g.stride(0), gptrs, gbs, int(relu_x), _stream(x.device))
    else:
        _lib.call("dlrm_interact_cat_backward", B, F, D, _p(g), g.stride(0), gptrs, gbs,
                  _stream(x.device))
        if relu_x:
            relu_backward(grad_x, x, out=grad_x)
    return grad_x, grad_ly


def _gather_entry(name: str, x: torch.Tensor, weights: torch.Tensor) -> str:
    """The gather entry point for the table's row type ([rows, D] fp32 or fp16)."""
    if weights.dtype == torch.float32:
        return name
    if weights.dtype == torch.float16:
        return name + "_f16"
    raise ValueError(f"gather interaction: fp32 or fp16 tables, not {weights.dtype}")


def interact_forward_gather(x: torch.Tensor, weights: torch.Tensor, row_base: torch.Tensor,
                            indices: torch.Tensor, self_interaction: bool = False,
                            out: Optional[torch.Tensor] = None,
                            error_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dot interaction of x and the one-hot lookups (L = 1) of T = len(row_base) - 1 tables
    gathered straight from ``weights`` (dlrm_interact_dot_forward_gather): the same R as
    interact_forward(x, tbe_forward(...)) without the pooled [B, T, D] buffer.  fp16
    ``weights`` take dlrm_interact_dot_forward_gather_f16: the rows are widened to fp32 as
    they are loaded, x, R and the arithmetic stay fp32."""
    _check_cuda(x, weights, row_base, indices)
    entry = _gather_entry("dlrm_interact_dot_forward_gather", x, weights)
    B, D = x.shape
    F = row_base.numel()
    npairs = F * (F + 1) // 2 if self_interaction else F * (F - 1) // 2
    if indices.dtype != torch.int32 or indices.numel() != (F - 1) * B:
        raise ValueError("gather interaction: int32 indices [(F-1) * B] (one per bag)")
    if out is None:
        out = torch.empty(B, D + npairs, dtype=torch.float32, device=x.device)
    _lib.call(entry, B, F, D, _p(x), x.stride(0), _p(weights),
              _p(row_base), _p(indices), int(self_interaction), _p(out), out.stride(0),
              _p(error_flag), _stream(x.device))
    return out


def interact_forward_gather_rows(x: torch.Tensor, packed: torch.Tensor, fmt: int, D: int,
                                 row_base: torch.Tensor, indices: torch.Tensor,
                                 self_interaction: bool = False,
                                 out: Optional[torch.Tensor] = None,
                                 error_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """interact_forward_gather on row-wise quantized tables (forward only):
    ``packed`` is uint8 [rows, row_bytes] in ``fmt`` ROWS_Q8 | ROWS_Q4 (rows_quantize's output),
    each level dequantised as fma(scale, q, bias) in registers.  Bitwise
    interact_forward_gather on the dequantised fp32 table
    (dlrm_interact_dot_forward_gather_rows)."""
    _check_cuda(x, packed, row_base, indices)
    if packed.dtype != torch.uint8 or packed.dim() != 2:
        raise ValueError(f"gather interaction on packed rows: uint8 [rows, row_bytes], not "
                         f"{packed.dtype}")
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != D:
        raise ValueError(f"gather interaction on packed rows: x is fp32 [B, {D}]")
    B = x.shape[0]
    F = row_base.numel()
    npairs = F * (F + 1) // 2 if self_interaction else F * (F - 1) // 2
    if indices.dtype != torch.int32 or indices.numel() != (F - 1) * B:
        raise ValueError("gather interaction: int32 indices [(F-1) * B] (one per bag)")
    if out is None:
        out = torch.empty(B, D + npairs, dtype=torch.float32, device=x.device)
    _lib.call("dlrm_interact_dot_forward_gather_rows", B, F, D, _p(x), x.stride(0), _p(packed),
              int(fmt), packed.stride(0), _p(row_base), _p(indices), int(self_interaction),
              _p(out), out.stride(0), _p(error_flag), _stream(x.device))
    return out


def interact_backward_gather(x: torch.Tensor, weights: torch.Tensor, row_base: torch.Tensor,
                             indices: torch.Tensor, grad_out: torch.Tensor,
                             self_interaction: bool = False,
                             grad_x: Optional[torch.Tensor] = None,
                             grad_ly: Optional[torch.Tensor] = None, relu_x: bool = False):
    """Backward of interact_forward_gather (rows re-gathered; call before the embedding
    update): grad_x [B, D] and grad_ly [B, T, D].  fp16 ``weights`` as in the forward."""
    entry = _gather_entry("dlrm_interact_dot_backward_gather", x, weights)
    B, D = x.shape
    T = row_base.numel() - 1
    if grad_x is None:
        grad_x = torch.empty_like(x, memory_format=torch.contiguous_format)
    if grad_ly is None:
        grad_ly = torch.empty(B, T, D, dtype=torch.float32, device=x.device)
    gfeats, gstrides = feature_views(grad_x, grad_ly)
    gptrs, gbs = _feature_arrays(gfeats, gstrides)
    g = grad_out if grad_out.stride(1) == 1 else grad_out.contiguous()
    _lib.call(entry, B, T + 1, D, _p(x), x.stride(0), _p(weights),
              _p(row_base), _p(indices), int(self_interaction), _p(g), g.stride(0), gptrs, gbs,
              int(relu_x), _stream(x.device))
    return grad_x, grad_ly


# ------------------------------------------------------------------ MLP ----
def gemm_workspace_size(M: int, N: int, K: int, trans_a: bool = False,
                        trans_b: bool = False) -> int:
    return _lib.query("dlrm_gemm_f32_workspace_size", int(trans_a), int(trans_b), M, N, K)


GEMM_FULL, GEMM_PARTIAL, GEMM_REDUCE = 0, 1, 2  # dlrm_gemm_mode


def gemm_problem(A: torch.Tensor, B: torch.Tensor, trans_a: bool = False,
                 trans_b: bool = False, C: Optional[torch.Tensor] = None, alpha=1.0,
                 epilogue: int = EPI_STORE, bias: Optional[torch.Tensor] = None,
                 aux: Optional[torch.Tensor] = None, ones_col: int = -1,
                 partial: Optional[torch.Tensor] = None, splits: int = 0):
    """One dlrm_gemm_problem: C = epilogue(alpha * op(A) @ op(B)) with row-major 2-D
    operands (unit inner stride); ones_col >= 0 also writes C[:, ones_col] =
    epilogue(alpha * op(A).sum(1)) (a Linear bias gradient).  With ``partial`` the problem
    is a PARTIAL one: K split ``splits`` ways, raw partials into ``partial``, C untouched
    until reduce_problem(...) runs in a later launch.  ``alpha``: a float, or a 1-element
    fp32 device tensor (alpha_dev: read when the kernel runs).  Returns (struct, C)."""
    _check_cuda(A, B, C, bias, aux)
    alpha_dev = _lr_dev(alpha, "gemm_problem: alpha")
    if A.stride(1) != 1 or B.stride(1) != 1:
        raise ValueError("gemm operands need unit inner stride")
    M = A.shape[1] if trans_a else A.shape[0]
    K = A.shape[0] if trans_a else A.shape[1]
    N = B.shape[0] if trans_b else B.shape[1]
    Kb = B.shape[1] if trans_b else B.shape[0]
    if K != Kb:
        raise ValueError(f"gemm inner dims differ: {K} vs {Kb}")
    if C is None:
        C = torch.empty((M, N if ones_col < 0 else max(N, ones_col + 1)), dtype=torch.float32,
                        device=A.device)
    if C.stride(1) != 1 or C.shape[0] != M or C.shape[1] < N:
        raise ValueError("gemm output must be [M, >= N] with unit inner stride")
    if ones_col >= 0 and not (N <= ones_col < C.shape[1]):
        raise ValueError("ones_col must be a column of C outside [0, N)")
    pr = _lib.GemmProblem(int(trans_a), int(trans_b), M, N, K,
                          0.0 if alpha_dev is not None else float(alpha), A.data_ptr(),
                          A.stride(0), B.data_ptr(), B.stride(0), C.data_ptr(), C.stride(0),
                          int(epilogue), bias.data_ptr() if bias is not None else None,
                          aux.data_ptr() if aux is not None else None,
                          aux.stride(0) if aux is not None else 0, int(ones_col),
                          GEMM_PARTIAL if partial is not None else GEMM_FULL, int(splits),
                          partial.data_ptr() if partial is not None else None, alpha_dev)
    return pr, C


def gemm_splits(pr, partial: bool = False, requested: int = 0) -> int:
    """The planner's K split for a problem launched alone (dlrm_gemm_f32_splits); with
    partial=True, as a PARTIAL problem (deferred reduction).  ``requested`` > 0 (PARTIAL):
    that count normalized to K - the count a PARTIAL launch accepts and its REDUCE repeats."""
    q = _lib.GemmProblem.from_buffer_copy(pr)
    if partial:
        q.mode = GEMM_PARTIAL
    q.splits = int(requested) if partial else 0
    return int(_lib.load().dlrm_gemm_f32_splits(ctypes.byref(q)))


def gemm_partial_bytes(M: int, N: int, splits: int) -> int:
    return _lib.query("dlrm_gemm_f32_partial_bytes", M, N, splits)


def sgd_job(param: torch.Tensor, grad: torch.Tensor, lr):
    """param -= lr * grad (flat fp32, numel % 4 == 0, 16-B aligned) as a one-split REDUCE job:
    an elementwise GEMM-group problem, so the update rides on a launch that exists anyway
    (C = SGD(alpha * sum_s part[s]) with one split: param - lr * grad, the SGD epilogue's
    rounding).  ``lr``: a float or a 1-element fp32 device tensor."""
    _check_cuda(param, grad)
    lr_dev = _lr_dev(lr, "sgd_job: lr")
    n = param.numel()
    if grad.numel() != n or n % 4 or param.data_ptr() % 16 or grad.data_ptr() % 16:
        raise ValueError("sgd_job: flat fp32 tensors of equal size, numel % 4 == 0, 16-B aligned")
    return _lib.GemmProblem(0, 0, 1, n, 0, 0.0 if lr_dev is not None else float(lr), None, 0,
                            None, 0, param.data_ptr(), n, EPI_SGD, None, None, 0, -1,
                            GEMM_REDUCE, 1, grad.data_ptr(), lr_dev)


def reduce_problem(pr_partial):
    """The REDUCE problem finishing a PARTIAL one (same C, alpha, epilogue, ones_col)."""
    q = _lib.GemmProblem.from_buffer_copy(pr_partial)
    q.mode = GEMM_REDUCE
    return q


def _problems(prs):
    arr = (_lib.GemmProblem * len(prs))(*prs)
    return arr


def gemm_group_workspace_size(problems) -> int:
    return _lib.query("dlrm_gemm_f32_group_workspace_size", len(problems),
                      ctypes.cast(_problems(problems), ctypes.c_void_p))


def gemm_group(problems, workspace: Optional[torch.Tensor] = None, device=None, role=None,
               phase: int = 0) -> None:
    """Launch up to 6 independent GEMM problems (gemm_problem structs) in ONE kernel.
    ``workspace``: zero-initialised uint8 buffer (split-K tickets + partials); a cached one
    is used when None.  ``role`` (tbe_backward_defer) + ``phase`` (1, then 2): that pass of
    the deferred embedding update runs as extra workgroups of the same launch (problems
    may then be empty)."""
    arr = _problems(problems)
    need = _lib.query("dlrm_gemm_f32_group_workspace_size", len(problems),
                      ctypes.cast(arr, ctypes.c_void_p)) if problems else 0
    dev = device if device is not None else torch.cuda.current_device()
    if need and workspace is None:
        workspace = _ws("gemm", need, dev)
    elif need and workspace.numel() < need:
        # never fall back to a shared buffer behind the caller's back: two streams could
        # then write split-K partials into the same scratch
        raise ValueError(f"gemm workspace too small: {workspace.numel()} < {need} bytes")
    if role is not None:
        _lib.call("dlrm_gemm_f32_group_role", len(problems), ctypes.cast(arr, ctypes.c_void_p),
                  _p(workspace) if need else None, workspace.numel() if need else 0,
                  ctypes.byref(role), int(phase), _stream(dev))
        return
    _lib.call("dlrm_gemm_f32_group", len(problems), ctypes.cast(arr, ctypes.c_void_p),
              _p(workspace) if need else None, workspace.numel() if need else 0,
              _stream(dev))


def gemm(A: torch.Tensor, B: torch.Tensor, trans_a: bool = False, trans_b: bool = False,
         C: Optional[torch.Tensor] = None, alpha=1.0, epilogue: int = EPI_STORE,
         bias: Optional[torch.Tensor] = None, aux: Optional[torch.Tensor] = None,
         workspace: Optional[torch.Tensor] = None, ones_col: int = -1) -> torch.Tensor:
    """C = epilogue(alpha * op(A) @ op(B)) with row-major 2-D operands (unit inner stride).
    Split-K uses ``workspace`` (or a cached one) when the planner asks for it."""
    pr, C = gemm_problem(A, B, trans_a, trans_b, C, alpha, epilogue, bias, aux, ones_col)
    gemm_group([pr], workspace, A.device)
    return C


def colsum(Y: torch.Tensor, scale: Optional[torch.Tensor] = None, alpha: float = 1.0,
           out: Optional[torch.Tensor] = None, accumulate: bool = False,
           sgd_param: Optional[torch.Tensor] = None, lr=0.0,
           workspace: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """``lr``: a float or a 1-element fp32 device tensor."""
    M, N = Y.shape
    need = _lib.query("dlrm_colsum_workspace_size", M, N)
    if workspace is None:  # (a caller's own buffer is never swapped: too small is refused)
        workspace = _ws("colsum", need, Y.device)
    lr_dev = _lr_dev(lr, "colsum: lr")
    _lib.call("dlrm_colsum_f32" if lr_dev is None else "dlrm_colsum_f32_dev", M, N, _p(Y),
              Y.stride(0), _p(scale), float(alpha), _p(out), int(accumulate), _p(sgd_param),
              float(lr) if lr_dev is None else lr_dev, _p(workspace), workspace.numel(),
              _stream(Y.device))
    return out


def head_forward_backward(X: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor],
                          target: Optional[torch.Tensor], loss: str = "mse",
                          clamp_lo: float = 0.0, grad_scale: float = 1.0,
                          prob: Optional[torch.Tensor] = None, dz: Optional[torch.Tensor] = None,
                          loss_out: Optional[torch.Tensor] = None,
                          workspace: Optional[torch.Tensor] = None):
    M, K = X.shape
    need = _lib.query("dlrm_head_workspace_size", M)
    if workspace is None:  # (a caller's own buffer is never swapped: too small is refused)
        workspace = _ws("head", need, X.device)
    _lib.call("dlrm_head_forward_backward", M, K, _p(X), X.stride(0), _p(w), _p(b), _p(target),
              LOSS_BCE if loss == "bce" else LOSS_MSE, float(clamp_lo), float(grad_scale),
              _p(prob), _p(dz), _p(loss_out), _p(workspace), workspace.numel(), _stream(X.device))
    return prob, dz, loss_out


def head_step(X: torch.Tensor, w: torch.Tensor, target: torch.Tensor, loss: str = "mse",
              clamp_lo: float = 0.0, grad_scale: float = 1.0,
              prob: Optional[torch.Tensor] = None, dz: Optional[torch.Tensor] = None,
              loss_out: Optional[torch.Tensor] = None, dX: Optional[torch.Tensor] = None,
              relu_mask: bool = True, dw: Optional[torch.Tensor] = None, accumulate: bool = False,
              lr=0.0, workspace: Optional[torch.Tensor] = None, defer: bool = False):
    """Fused head (dlrm_head_step): X [M, K] with the folded bias column, w [K] (updated in
    place by SGD when lr != 0 and dw is None).  ``defer``: the second launch (column sums,
    update, mean loss) becomes the returned role, pass 4 of a later gemm_group
    (dlrm_head_step_defer); w / dw / loss_out / workspace untouched until then.  ``lr``: a
    float or a 1-element fp32 device tensor (read by the update's launch when it runs)."""
    M, K = X.shape
    need = _lib.query("dlrm_head_step_workspace_size", M, K)
    if workspace is None:  # (a caller's own buffer is never swapped: too small is refused)
        workspace = _ws("head_step", need, X.device)
    _check_cuda(X, w, target)
    lr_dev = _lr_dev(lr, "head_step: lr")
    sfx = "" if lr_dev is None else "_dev"
    args = (M, K, _p(X), X.stride(0), _p(w), _p(target),
            LOSS_BCE if loss == "bce" else LOSS_MSE, float(clamp_lo), float(grad_scale),
            _p(prob), _p(dz), _p(loss_out), _p(dX), dX.stride(0) if dX is not None else 0,
            int(relu_mask), _p(dw), int(accumulate), float(lr) if lr_dev is None else lr_dev,
            _p(workspace), workspace.numel())
    if defer:
        role = _lib.LaunchRole()
        _lib.call("dlrm_head_step_defer" + sfx, *args, ctypes.byref(role), _stream(X.device))
        return role
    _lib.call("dlrm_head_step" + sfx, *args, _stream(X.device))
    return prob, dz, loss_out


def head_predict(X: torch.Tensor, w: torch.Tensor, clamp_lo: float = 0.0,
                 prob: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None,
                 state=None) -> torch.Tensor:
    """Forward-only head (dlrm_head_predict): X [M, K] with the folded bias column, w [K] ->
    prob [M], bit for bit head_step's prob; w is only read.  With ``target`` and ``state``
    (a metrics.EvalState) every row is also appended to the state's log and counted."""
    M, K = X.shape
    _check_cuda(X, w, prob, target)
    if prob is None:
        prob = torch.empty(M, dtype=torch.float32, device=X.device)
    if (state is None) != (target is None):
        raise ValueError("head_predict: target and state go together")
    if target is not None and (target.numel() != M or target.dtype != torch.float32
                               or not target.is_contiguous()):
        raise ValueError("head_predict: target must be M contiguous fp32 labels")
    st = ctypes.byref(state.c_struct()) if state is not None else None
    _lib.call("dlrm_head_predict", M, K, _p(X), X.stride(0), _p(w), float(clamp_lo), _p(prob),
              _p(target), st, _stream(X.device))
    return prob


MLP16_TYPES = {"bf16": 0, "fp16": 1}  # dlrm_mlp16_type
LINEAR16_TILES = (128128, 128064, 64064, 32064)  # DLRM_TUNE_LINEAR16_TILE values


def _row_major(t: torch.Tensor, what: str, fn: str = "linear16_forward") -> int:
    """The leading dimension of a 2-D fp32 tensor whose rows are contiguous."""
    if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{fn}: {what} must be 2-D fp32 with contiguous rows")
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1], 1)


def linear16_forward(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None,
                     relu: bool = False, out: Optional[torch.Tensor] = None,
                     dtype: str = "bf16") -> torch.Tensor:
    """Forward-only Linear on the 16-bit MFMA (dlrm_linear16_forward): out [M, N] =
    act(r16(x) r16(W)^T + bias), x [M, K] and W [N, K] fp32 tensors or views with contiguous
    rows, each element rounded to nearest-even ``dtype`` ("bf16" | "fp16") in flight, fp32
    accumulate, fp32 bias / ReLU / output.  ``bias`` may be a strided 1-D view (a column of
    W's buffer).  Only out[:M, :N] is written (``out`` may be a view of a wider buffer).
    The library takes 16-byte loads when both base addresses (storage offset included) are
    16-byte aligned and both row strides are multiples of 4, scalar loads otherwise; neither
    reads past column K of any row, so the extent of the last row never matters."""
    if dtype not in MLP16_TYPES:
        raise ValueError(f"linear16_forward: dtype {dtype!r} (one of {sorted(MLP16_TYPES)})")
    _check_cuda(x, W, bias, out)
    ldx, ldw = _row_major(x, "x"), _row_major(W, "W")
    (M, K), N = x.shape, W.shape[0]
    if W.shape[1] != K:
        raise ValueError(f"linear16_forward: x is [{M}, {K}], W is {list(W.shape)}")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    ldy = _row_major(out, "out")
    if tuple(out.shape) != (M, N):
        raise ValueError(f"linear16_forward: out is {list(out.shape)}, expected [{M}, {N}]")
    bstride = 0
    if bias is not None:
        if bias.dim() != 1 or bias.numel() != N or bias.dtype != torch.float32:
            raise ValueError("linear16_forward: bias must be N fp32 values")
        bstride = bias.stride(0) if N > 1 else 1
    _lib.call("dlrm_linear16_forward", MLP16_TYPES[dtype], M, N, K, _p(x), ldx, _p(W), ldw,
              _p(bias), bstride, int(bool(relu)), _p(out), ldy, _stream(x.device))
    return out


LINEAR8_TILES = LINEAR16_TILES  # DLRM_TUNE_LINEAR8_TILE values
LINEAR8_RANGE_FLOATS = 2048  # DLRM_LINEAR8_RANGE_FLOATS: min partials, then max partials
LINEAR8_MAX_K = 131072


class Linear8Weights:
    """The packed weights of one int8 Linear (dlrm_linear8_pack): ``wq`` int8 [N, ldwq] with
    ldwq a multiple of 64 (columns >= K are 0), ``s_w`` one fp32 scale, both on the device of
    the fp32 weights."""

    def __init__(self, wq: torch.Tensor, s_w: torch.Tensor, N: int, K: int):
        if wq.dtype != torch.int8 or wq.dim() != 2 or not wq.is_contiguous() \
                or wq.shape[0] != N or wq.shape[1] % 64 or wq.shape[1] < max(K, 64):
            raise ValueError(f"Linear8Weights: wq must be contiguous int8 [{N}, ldwq] with ldwq a "
                             f"multiple of 64 and >= {max(K, 64)}, not {wq.dtype} "
                             f"{list(wq.shape)}")
        if s_w.dtype != torch.float32 or s_w.numel() != 1 or s_w.device != wq.device:
            raise ValueError("Linear8Weights: s_w must be one fp32 value on wq's device")
        self.wq, self.s_w, self.N, self.K = wq, s_w, int(N), int(K)


def linear8_pack(W: torch.Tensor, out: Optional[Linear8Weights] = None) -> Linear8Weights:
    """dlrm_linear8_pack: W [N, K] fp32 (a view with contiguous rows: the columns past K of a
    wider buffer, e.g. a folded bias column, are not read) -> per-tensor symmetric int8 weights,
    bitwise torch's MinMaxObserver(qint8, per_tensor_symmetric) + quantize_per_tensor.  ``out``:
    a Linear8Weights of the same N and K to re-pack into (its storage is kept)."""
    ldw = _row_major(W, "W", "linear8_pack")
    _check_cuda(W)
    N, K = W.shape
    if out is None:
        ldwq = max((K + 63) // 64 * 64, 64)
        out = Linear8Weights(torch.zeros((N, ldwq), dtype=torch.int8, device=W.device),
                             torch.zeros(1, dtype=torch.float32, device=W.device), N, K)
    elif (out.N, out.K) != (N, K) or out.wq.device != W.device:
        raise ValueError(f"linear8_pack: out holds [{out.N}, {out.K}] weights, W is [{N}, {K}]")
    need = _lib.query("dlrm_linear8_pack_workspace_size", N, K)
    ws = _ws("linear8_pack", need, W.device)
    _lib.call("dlrm_linear8_pack", N, K, _p(W), ldw, _p(out.wq), out.wq.shape[1], _p(out.s_w),
              _p(ws), ws.numel(), _stream(W.device))
    return out


def linear8_range(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dlrm_linear8_range: the min / max partials of x [M, K] (fp32, contiguous rows) that
    linear8_forward folds: LINEAR8_RANGE_FLOATS fp32 values (``out``: such a tensor)."""
    ldx = _row_major(x, "x", "linear8_range")
    _check_cuda(x, out)
    if out is None:
        out = torch.empty(LINEAR8_RANGE_FLOATS, dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or out.numel() != LINEAR8_RANGE_FLOATS \
            or not out.is_contiguous():
        raise ValueError(f"linear8_range: out must be {LINEAR8_RANGE_FLOATS} contiguous fp32")
    _lib.call("dlrm_linear8_range", x.shape[0], x.shape[1], _p(x), ldx, _p(out),
              _stream(x.device))
    return out


def linear8_forward(x: torch.Tensor, packed: Linear8Weights,
                    bias: Optional[torch.Tensor] = None, relu: bool = False,
                    out: Optional[torch.Tensor] = None, rng: Optional[torch.Tensor] = None,
                    qparams: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Forward-only int8 Linear (dlrm_linear8_forward): out [M, N] = act(dequant(q(x) Wq^T) +
    bias), x [M, K] an fp32 tensor or view with contiguous rows quantized per call to 7-bit
    codes from its own range, bitwise torch's dynamically quantized nn.Linear on fbgemm.
    ``rng``: linear8_range(x) (computed here when None).  ``bias`` may be a strided 1-D view;
    only out[:M, :N] is written (``out`` may be a view of a wider buffer); no column >= K of x
    is read.  ``qparams``: 2 fp32 on the device that receive (s_x, zero point)."""
    if not isinstance(packed, Linear8Weights):
        raise ValueError("linear8_forward: packed must be a Linear8Weights (linear8_pack)")
    ldx = _row_major(x, "x", "linear8_forward")
    M, K = x.shape
    N = packed.N
    if K != packed.K:
        raise ValueError(f"linear8_forward: x is [{M}, {K}], the packed weights are "
                         f"[{N}, {packed.K}]")
    if K > LINEAR8_MAX_K:
        raise ValueError(f"linear8_forward: K {K} > {LINEAR8_MAX_K}")
    bstride = 0
    if bias is not None:
        if bias.dim() != 1 or bias.numel() != N or bias.dtype != torch.float32:
            raise ValueError("linear8_forward: bias must be N fp32 values")
        bstride = bias.stride(0) if N > 1 else 1
    if out is not None and (out.dim() != 2 or tuple(out.shape) != (M, N)):
        raise ValueError(f"linear8_forward: out is {list(out.shape)}, expected [{M}, {N}]")
    if rng is not None and (rng.dtype != torch.float32 or rng.numel() != LINEAR8_RANGE_FLOATS
                            or not rng.is_contiguous()):
        raise ValueError(f"linear8_forward: rng must be {LINEAR8_RANGE_FLOATS} contiguous fp32 "
                         "(linear8_range)")
    if qparams is not None and (qparams.dtype != torch.float32 or qparams.numel() != 2
                                or not qparams.is_contiguous()):
        raise ValueError("linear8_forward: qparams must be 2 contiguous fp32")
    _check_cuda(x, packed.wq, bias, out, rng, qparams)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    ldy = _row_major(out, "out", "linear8_forward")
    if rng is None:
        rng = linear8_range(x)
    _lib.call("dlrm_linear8_forward", M, N, K, _p(x), ldx, _p(rng), _p(packed.wq),
              packed.wq.shape[1], _p(packed.s_w), _p(bias), bstride, int(bool(relu)), _p(out),
              ldy, _p(qparams), _stream(x.device))
    return out


# DLRM_TUNE_LINEAR16_DGRAD_TILE / DLRM_TUNE_LINEAR16_WGRAD_TILE values
LINEAR16_DGRAD_TILES = LINEAR16_TILES
LINEAR16_WGRAD_TILES = LINEAR16_TILES
WGRAD16_STORE, WGRAD16_SGD = 0, 1  # dlrm_wgrad16_mode


def linear16_dgrad(g: torch.Tensor, W: torch.Tensor, mask: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, dtype: str = "bf16") -> torch.Tensor:
    """A Linear's data gradient on the 16-bit MFMA (dlrm_linear16_dgrad): out [M, K] =
    r16(g) r16(W) where ``mask`` > 0 (mask None: everywhere), 0 elsewhere; g [M, N], W [N, K],
    mask [M, K] fp32 tensors or views with contiguous rows, rounded to nearest-even ``dtype``
    in flight, fp32 accumulate.  Only out[:M, :K] is written.  Enqueues only; allocates
    nothing when ``out`` is given."""
    if dtype not in MLP16_TYPES:
        raise ValueError(f"linear16_dgrad: dtype {dtype!r} (one of {sorted(MLP16_TYPES)})")
    _check_cuda(g, W, mask, out)
    ldg, ldw = _row_major(g, "g", "linear16_dgrad"), _row_major(W, "W", "linear16_dgrad")
    (M, N), K = g.shape, W.shape[1]
    if W.shape[0] != N:
        raise ValueError(f"linear16_dgrad: g is [{M}, {N}], W is {list(W.shape)}")
    ldm = 0
    if mask is not None:
        ldm = _row_major(mask, "mask", "linear16_dgrad")
        if tuple(mask.shape) != (M, K):
            raise ValueError(f"linear16_dgrad: mask is {list(mask.shape)}, expected [{M}, {K}]")
    if out is None:
        out = torch.empty((M, K), dtype=torch.float32, device=g.device)
    ldo = _row_major(out, "out", "linear16_dgrad")
    if tuple(out.shape) != (M, K):
        raise ValueError(f"linear16_dgrad: out is {list(out.shape)}, expected [{M}, {K}]")
    _lib.call("dlrm_linear16_dgrad", MLP16_TYPES[dtype], M, N, K, _p(g), ldg, _p(W), ldw,
              _p(mask), ldm, _p(out), ldo, _stream(g.device))
    return out


def linear16_wgrad_workspace_size(M: int, N: int, K: int, dtype: str = "bf16") -> int:
    """Bytes of workspace linear16_wgrad needs for these sizes under the calling thread's
    tuning overrides (0: none)."""
    return _lib.query("dlrm_linear16_wgrad_workspace_size", MLP16_TYPES[dtype], M, N, K)


def linear16_wgrad(g: torch.Tensor, x: torch.Tensor, out: torch.Tensor,
                   lr=None, dtype: str = "bf16",
                   workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A Linear's weight gradient on the 16-bit MFMA (dlrm_linear16_wgrad): acc [N, K] =
    r16(g)^T r16(x), g [M, N] and x [M, K] fp32 with contiguous rows, rounded to nearest-even
    ``dtype`` in flight, fp32 accumulate.  ``lr`` None: out = acc; else (a float or a
    1-element fp32 device tensor) the fused SGD step out = out - fl(lr * acc).  Only out[:N, :K] is touched.  ``workspace`` (any contiguous
    tensor of at least linear16_wgrad_workspace_size bytes) holds the partial sums when the
    planner splits the batch; it is allocated here when needed and not given.  Enqueues only."""
    if dtype not in MLP16_TYPES:
        raise ValueError(f"linear16_wgrad: dtype {dtype!r} (one of {sorted(MLP16_TYPES)})")
    _check_cuda(g, x, out, workspace)
    ldg, ldx = _row_major(g, "g", "linear16_wgrad"), _row_major(x, "x", "linear16_wgrad")
    (M, N), K = g.shape, x.shape[1]
    if x.shape[0] != M:
        raise ValueError(f"linear16_wgrad: g is [{M}, {N}], x is {list(x.shape)}")
    ldc = _row_major(out, "out", "linear16_wgrad")
    if tuple(out.shape) != (N, K):
        raise ValueError(f"linear16_wgrad: out is {list(out.shape)}, expected [{N}, {K}]")
    need = linear16_wgrad_workspace_size(M, N, K, dtype)
    if workspace is None:
        if need:
            workspace = torch.empty(need, dtype=torch.uint8, device=g.device)
    elif not workspace.is_contiguous():
        raise ValueError("linear16_wgrad: workspace must be contiguous")
    ws_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    if ws_bytes < need:
        raise ValueError(f"linear16_wgrad: workspace of {ws_bytes} bytes, {need} needed")
    lr_dev = _lr_dev(lr, "linear16_wgrad: lr")
    if lr_dev is not None:
        _lib.call("dlrm_linear16_wgrad_dev", MLP16_TYPES[dtype], M, N, K, _p(g), ldg, _p(x),
                  ldx, WGRAD16_SGD, lr_dev, _p(out), ldc, _p(workspace), ws_bytes,
                  _stream(g.device))
        return out
    _lib.call("dlrm_linear16_wgrad", MLP16_TYPES[dtype], M, N, K, _p(g), ldg, _p(x), ldx,
              WGRAD16_STORE if lr is None else WGRAD16_SGD, 0.0 if lr is None else float(lr),
              _p(out), ldc, _p(workspace), ws_bytes, _stream(g.device))
    return out


def eval_update(prob: torch.Tensor, target: torch.Tensor, state) -> None:
    """Append n existing probabilities and their labels to an evaluation state's log and add
    their confusion counts (dlrm_eval_update); enqueues only, capturable."""
    _check_cuda(prob, target)
    prob = prob.reshape(-1)
    target = target.reshape(-1)
    if prob.dtype != torch.float32 or target.dtype != torch.float32 or \
            prob.numel() != target.numel():
        raise ValueError("eval_update: fp32 prob and target of the same length")
    prob, target = prob.contiguous(), target.contiguous()
    _lib.call("dlrm_eval_update", prob.numel(), _p(prob), _p(target),
              ctypes.byref(state.c_struct()), _stream(prob.device))


EVAL_SORT_TILE = 4096  # DLRM_EVAL_SORT_TILE: keys per workgroup tile of the metrics sort


def eval_metrics(keys: torch.Tensor, n: Optional[int] = None,
                 workspace: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sort the first n packed keys (int32 tensor holding the uint32 keys) IN PLACE and
    reduce their tie groups (dlrm_eval_metrics).  Returns the int64 device tensor
    [A2, P, N, tie groups, bits of the float64 average-precision sum]."""
    _check_cuda(keys)
    if keys.dtype != torch.int32 or not keys.is_contiguous():
        raise ValueError("eval_metrics: keys must be a contiguous int32 tensor")
    n = keys.numel() if n is None else int(n)
    if not 0 <= n <= keys.numel():
        raise ValueError("eval_metrics: n outside the key buffer")
    need = _lib.query("dlrm_eval_metrics_workspace_size", n)
    if workspace is None or workspace.numel() < need:
        workspace = _ws("eval_metrics", need, keys.device)
    if out is None:
        out = torch.empty(5, dtype=torch.int64, device=keys.device)
    _lib.call("dlrm_eval_metrics", _p(keys), n, _p(workspace), workspace.numel(), _p(out),
              _stream(keys.device))
    return out


def outer_drelu(dz: torch.Tensor, w: torch.Tensor, X: Optional[torch.Tensor], relu_mask: bool,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    M = dz.shape[0]
    K = w.numel()
    if out is None:
        out = torch.empty((M, K), dtype=torch.float32, device=dz.device)
    _lib.call("dlrm_outer_drelu", M, K, _p(dz), _p(w), _p(X), X.stride(0) if X is not None else 0,
              int(relu_mask), _p(out), out.stride(0), _stream(dz.device))
    return out


def sigmoid_forward(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    x = x.contiguous()
    out = torch.empty_like(x) if out is None else out
    _lib.call("dlrm_sigmoid_forward", x.numel(), _p(x), _p(out), _stream(x.device))
    return out


def sigmoid_backward(dy: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    dy = dy.contiguous()
    dx = torch.empty_like(dy)
    _lib.call("dlrm_sigmoid_backward", dy.numel(), _p(dy), _p(y), _p(dx), _stream(dy.device))
    return dx


def relu_backward(dy: torch.Tensor, y: torch.Tensor,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx = dy * (y > 0) for 2-D row-strided operands (unit inner stride)."""
    if dy.dim() == 1:
        dy, y = dy.view(1, -1), y.reshape(1, -1)
        out = None if out is None else out.view(1, -1)
    if dy.stride(1) != 1 or y.stride(1) != 1:
        raise ValueError("relu_backward needs unit inner strides")
    M, K = dy.shape
    dx = torch.empty((M, K), dtype=torch.float32, device=dy.device) if out is None else out
    _lib.call("dlrm_relu_backward", M, K, _p(dy), dy.stride(0), _p(y), y.stride(0), _p(dx),
              dx.stride(0), _stream(dy.device))
    return dx


# ----------------------------------------------------------- optimizers ----
def sgd_update(param: torch.Tensor, grad: torch.Tensor, lr) -> None:
    """param -= lr * grad; ``lr``: a float or a 1-element fp32 device tensor."""
    lr_dev = _lr_dev(lr, "sgd_update: lr")
    if lr_dev is not None:
        _lib.call("dlrm_sgd_update_dev", _p(param), _p(grad), param.numel(), lr_dev,
                  _stream(param.device))
        return
    _lib.call("dlrm_sgd_update", _p(param), _p(grad), param.numel(), float(lr),
              _stream(param.device))


def adagrad_update(param: torch.Tensor, grad: torch.Tensor, state_sum: torch.Tensor, clr,
                   eps: float, grad_scale: float = 1.0) -> None:
    """state_sum += g'^2; param -= clr * g' / (sqrt(state_sum) + eps) with g' = grad_scale * g
    (grad itself is not modified).  ``clr``: a float or a 1-element fp32 device tensor."""
    clr_dev = _lr_dev(clr, "adagrad_update: clr")
    sfx = "" if clr_dev is None else "_dev"
    c = float(clr) if clr_dev is None else clr_dev
    if grad_scale != 1.0:
        _lib.call("dlrm_adagrad_update_scaled" + sfx, _p(param), _p(grad), _p(state_sum),
                  param.numel(), float(grad_scale), c, float(eps), _stream(param.device))
        return
    _lib.call("dlrm_adagrad_update" + sfx, _p(param), _p(grad), _p(state_sum), param.numel(),
              c, float(eps), _stream(param.device))


# -------------------------------------------- device-resident learning rates ----
LR_MAX_SLOTS = 8  # DLRM_LR_MAX_SLOTS
# byte offsets of the dlrm_lr_state block (DLRM_LR_OFF_*, include/dlrm_hip.h)
_LR_OFF_STEP, _LR_OFF_POLICY, _LR_OFF_BASE, _LR_OFF_MULT, _LR_OFF_LR = 0, 8, 40, 104, 168


class LRState:
    """The dlrm_lr_state block of include/dlrm_hip.h in device memory: the scheduler's step
    count, the policy (W, S, D), and per slot a base rate, a multiplier and the fp32 rate in
    effect.  ``lr(k)`` is the 1-element view every ``lr`` / ``alpha`` / ``clr`` argument of
    this module accepts; ``lr_schedule_tick`` recomputes all of them and advances the count.
    The views alias ``buf``: writes to ``step`` / ``base`` / ``mult`` (copy_, on the stream
    whose kernels read them) take effect at the next tick."""

    def __init__(self, buf: torch.Tensor, n: int, policy):
        self.buf, self.n, self.policy = buf, int(n), tuple(int(v) for v in policy)
        self.step = buf[_LR_OFF_STEP:_LR_OFF_STEP + 8].view(torch.int64)
        self.base = buf[_LR_OFF_BASE:_LR_OFF_BASE + 8 * self.n].view(torch.float64)
        self.mult = buf[_LR_OFF_MULT:_LR_OFF_MULT + 8 * self.n].view(torch.float64)
        self.rates = buf[_LR_OFF_LR:_LR_OFF_LR + 4 * self.n].view(torch.float32)

    def lr(self, k: int) -> torch.Tensor:
        if not 0 <= k < self.n:
            raise IndexError(f"lr slot {k} of {self.n}")
        return self.rates[k:k + 1]


def lr_state(base: Sequence[float], mult: Optional[Sequence[float]] = None,
             num_warmup_steps: int = 0, decay_start_step: int = 0, num_decay_steps: int = 0,
             step_count: int = 1, device=None) -> LRState:
    """A device learning-rate block (dlrm_lr_state_init + one host-to-device copy) with one
    slot per entry of ``base``; slot k's rate is (float)(policy(step_count, base[k]) *
    mult[k]) after each tick and (float)(base[k] * mult[k]) before the first.  All-zero
    policy: no schedule (a tick only recomputes base * mult).  Raises ValueError for a policy
    the reference does not run (optim.check_lr_policy)."""
    n = len(base)
    mult = [1.0] * n if mult is None else list(mult)
    if not 1 <= n <= LR_MAX_SLOTS or len(mult) != n:
        raise ValueError(f"lr_state: 1..{LR_MAX_SLOTS} slots, one multiplier each")
    nbytes = _lib.query("dlrm_lr_state_bytes")
    host = torch.zeros(nbytes, dtype=torch.uint8)
    b = (ctypes.c_double * n)(*[float(v) for v in base])
    m = (ctypes.c_double * n)(*[float(v) for v in mult])
    try:
        _lib.call("dlrm_lr_state_init", ctypes.c_void_p(host.data_ptr()), int(step_count),
                  int(num_warmup_steps), int(decay_start_step), int(num_decay_steps), n, b, m)
    except _lib.DLRMHipError as e:
        raise ValueError(str(e)) from None
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    return LRState(host.to(dev), n, (num_warmup_steps, decay_start_step, num_decay_steps))


def lr_schedule_tick(state: LRState) -> None:
    """One launch of one thread (dlrm_lr_schedule_tick): every slot's rate for the current
    step count, then step count + 1.  Enqueues only; capturable."""
    _lib.call("dlrm_lr_schedule_tick", _p(state.buf), _stream(state.buf.device))


# ------------------------------- stochastic rounding of the fp16 tables' update ----
_U64 = (1 << 64) - 1


def _as_i64(v: int) -> int:
    """The uint64 ``v`` (mod 2^64) as the int64 with the same bits."""
    v = int(v) & _U64
    return v - (1 << 64) if v >> 63 else v


def sr_state(seed: int = 0, step: int = 0, device=None) -> torch.Tensor:
    """The dlrm_sr_state block (include/dlrm_hip.h) in device memory: a 2-element int64
    tensor holding the uint64 bits of (seed, step).  tbe_backward('sgd_f16', ...,
    sr_state=) reads it when its kernels run; sr_tick advances the step."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    return torch.tensor([_as_i64(seed), _as_i64(step)], dtype=torch.int64).to(dev)


def sr_state_values(state: torch.Tensor):
    """(seed, step) of an sr_state tensor as unsigned Python ints; synchronises."""
    s, t = (int(v) & _U64 for v in state.view(torch.int64).cpu().tolist())
    return s, t


def _sr_ptr(state: torch.Tensor, who: str):
    u64 = getattr(torch, "uint64", None)
    if (not isinstance(state, torch.Tensor) or not state.is_cuda or state.numel() != 2
            or state.dtype not in (torch.int64, u64) or not state.is_contiguous()):
        raise ValueError(f"{who}: sr_state is a contiguous 2-element int64/uint64 device "
                         "tensor (ops.sr_state)")
    return _p(state)


def sr_tick(state: torch.Tensor) -> None:
    """One launch of one thread (dlrm_sr_tick): step += 1.  Enqueues only; capturable."""
    _lib.call("dlrm_sr_tick", _sr_ptr(state, "sr_tick"), _stream(state.device))


def scale_(x: torch.Tensor, alpha: float) -> None:
    _lib.call("dlrm_scale_f32", _p(x), x.numel(), float(alpha), _stream(x.device))


# -------------------------------------------------------------- utility ----
def uniform_fill_(out: torch.Tensor, lo: float, hi: float, seed: int) -> torch.Tensor:
    _lib.call("dlrm_uniform_fill", _p(out), out.numel(), float(lo), float(hi),
              int(seed) & 0xFFFFFFFFFFFFFFFF, _stream(out.device))
    return out


def uniform_fill_at_(out: torch.Tensor, lo: float, hi: float, seed: int,
                     first: int) -> torch.Tensor:
    """Elements [first, first + out.numel()) of uniform_fill_'s stream for ``seed``."""
    _lib.call("dlrm_uniform_fill_at", _p(out), out.numel(), float(lo), float(hi),
              int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), _stream(out.device))
    return out


def uniform_int_fill_(out: torch.Tensor, hi: int, seed: int) -> torch.Tensor:
    _lib.call("dlrm_uniform_int_fill", _p(out), _bits(out), out.numel(), int(hi),
              int(seed) & 0xFFFFFFFFFFFFFFFF, _stream(out.device))
    return out


def csr_from_tables(table_offsets: Sequence[torch.Tensor], table_nnz: Sequence[int], B: int,
                    out_dtype=torch.int32) -> torch.Tensor:
    """Device CSR builder: per-table int64 offsets [B] -> batched offsets [T*B+1]."""
    T = len(table_offsets)
    offs = [o if o.dtype == torch.int64 else o.long() for o in table_offsets]
    _check_cuda(*offs)
    out = torch.empty(T * B + 1, dtype=out_dtype, device=offs[0].device)
    ptrs = (ctypes.c_void_p * T)(*[o.data_ptr() for o in offs])
    nnz = (ctypes.c_int64 * T)(*[int(n) for n in table_nnz])
    _lib.call("dlrm_csr_from_tables", T, B, ptrs, nnz, _p(out),
              32 if out_dtype == torch.int32 else 64, _stream(offs[0].device))
    return out


def criteo_decode(records: torch.Tensor, n_dense: int = 13, n_sparse: int = 26,
                  max_ind_range: int = -1, batched: bool = False,
                  dense: Optional[torch.Tensor] = None, label: Optional[torch.Tensor] = None,
                  indices: Optional[torch.Tensor] = None,
                  offsets: Optional[torch.Tensor] = None):
    """Device decode of raw Criteo binary records int32 [n, 1+n_dense+n_sparse]
    (dlrm_criteo_decode; data_loader_terabyte.py:83-114).  Returns (dense [n, n_dense]
    log(x+1), lS_o, lS_i, label [n, 1]) in the reference's layouts: batched -> int32
    offsets [T*n+1] and int32 indices [T*n]; else int64 lS_o [T, n] = arange and int64
    lS_i [T, n].  ``dense`` may be a caller buffer (row stride >= n_dense); so may
    ``label`` (n fp32), ``indices`` and (batched) ``offsets``, e.g. the fixed buffers a
    captured step graph reads."""
    _check_cuda(records, dense, label, indices, offsets)
    nf = 1 + n_dense + n_sparse
    if records.dtype != torch.int32 or not records.is_contiguous() or records.numel() % nf:
        raise ValueError(f"criteo_decode: need contiguous int32 records of {nf} fields")
    n = records.numel() // nf
    dev = records.device
    if dense is None:
        dense = torch.empty((n, n_dense), dtype=torch.float32, device=dev)
    elif dense.shape[0] != n or dense.shape[1] < n_dense or dense.stride(1) != 1:
        raise ValueError("criteo_decode: dense buffer must be [n, >= n_dense] row-major")
    idt = torch.int32 if batched else torch.int64
    if label is None:
        label = torch.empty((n, 1), dtype=torch.float32, device=dev)
    if indices is None:
        indices = torch.empty(n_sparse * n, dtype=idt, device=dev)
    if offsets is None and batched:
        offsets = torch.empty(n_sparse * n + 1, dtype=torch.int32, device=dev)
    if (label.numel() != n or label.dtype != torch.float32 or not label.is_contiguous()
            or indices.numel() != n_sparse * n or indices.dtype != idt
            or not indices.is_contiguous()
            or (batched and (offsets.numel() != n_sparse * n + 1 or offsets.dtype != torch.int32
                             or not offsets.is_contiguous()))):
        raise ValueError("criteo_decode: label / indices / offsets buffers of the wrong shape")
    _lib.call("dlrm_criteo_decode", _p(records), n, n_dense, n_sparse, int(max_ind_range),
              _p(dense), dense.stride(0) if n else n_dense, _p(label), _p(indices),
              32 if batched else 64, _p(offsets), 32, _stream(dev))
    if batched:
        return dense, offsets, indices, label
    lS_o = torch.arange(n, device=dev).reshape(1, -1).repeat(n_sparse, 1)
    return dense, lS_o, indices.view(n_sparse, n), label
