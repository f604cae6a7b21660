"""Exact-arithmetic tests of the embedding side: the pooled lookup, the sorted backward with
SGD / dense / fp16 SGD / row-wise Adagrad fused in, and the per-sample-weight and expanded
gradients, against the CPU references of tests/exact_tbe.py.

The operands are integer-valued (or one full-mantissa product per output), so every result must
equal the reference BIT FOR BIT whatever the sort variant, block length, lane group or
summation order: there is no tolerance in this file.  Weight and momentum rows no lookup
references hold NaN and must keep their bits; grad_out sits in a NaN-padded buffer, the pooled
output in a sentinel-padded one; the error flag must be exactly the expected bits.  DESIGN.md
("Exact-arithmetic coverage of the embedding side") says which case reaches which branch."""
import functools

import numpy as np
import pytest
import torch

import exact_tbe as E
from exact_inputs import SENTINEL, full_mantissa, int_matrix, padded, pads_intact

pytestmark = pytest.mark.gpu

dev = "cuda:0"
NAN = float("nan")
D_FWD = [1, 2, 4, 5, 8, 12, 16, 32, 64, 100, 128, 256, 260, 512, 1024, 2048]
D_BWD = [1, 4, 5, 8, 12, 16, 32, 64, 100, 128, 256, 260, 512, 1024, 2048]
D_LEAN = [16, 32, 64, 128]
MODES = ["sgd", "dense", "rowwise_adagrad"]


@pytest.fixture(scope="module")
def ops():
    from dlrm_hip import ops as _ops
    return _ops


# ---------------------------------------------------------------- shared cases ----
@functools.lru_cache(maxsize=None)
def _case(name):
    if name.startswith("sort_"):
        return E.sort_case(name[5:])
    named = {"skewed": E.skewed_case, "structure": E.structure_case, "cancel": E.cancel_case}
    if name in named:
        return named[name]()
    return {c.name: c for c in E.small_n_cases()}[name]


@functools.lru_cache(maxsize=64)
def _operands(name, D, weighted, lr=2.0 ** -4):
    """Operands and the coalesced gradient of (case, D): built once, shared, never changed."""
    c = _case(name)
    zero = None
    if name == "cancel":
        zero = int(c.runs_spec[c.runs_spec[:, 1] == 2][0, 2])
    o = E.operands_for(c, D, weighted, seed=D + 7 * weighted, zero_row=zero, lr=lr)
    return o, E.coalesced_grad(c, o)


def _reference(o, gsum, mode, half=False):
    """(start rows, reference rows, reference momentum) on the touched rows."""
    if mode == "dense":
        return o.acc0u, E.ref_dense(o.acc0u, gsum), None
    if mode == "sgd" and half:
        return o.W0u.half(), E.ref_sgd_f16(o.W0u.half(), gsum, o.lr), None
    if mode == "sgd":
        return o.W0u, E.ref_sgd(o.W0u, gsum, o.lr), None
    W, m = E.ref_adagrad(o.W0u, o.mom0u, gsum, o.D, o.lr, o.eps)
    return o.W0u, W, m


# -------------------------------------------------------------- device buffers ----
def _dev_rows(c, o, vals, misalign=False):
    """[total_rows, D] on the device: NaN everywhere but the touched rows; ``misalign``: the
    view starts one element into its buffer (no 16-byte rows: the scalar kernels)."""
    R, D = c.total_rows, vals.shape[1]
    flat = torch.full((R * D + 8,), NAN, dtype=vals.dtype, device=dev)
    a = 1 if misalign else 0
    W = flat[a:a + R * D].view(R, D)
    W[torch.from_numpy(o.urows).to(dev)] = vals.to(dev)
    return W


def _dev_vec(c, o, vals):
    m = torch.full((c.total_rows,), NAN, device=dev)
    m[torch.from_numpy(o.urows).to(dev)] = vals.to(dev)
    return m


def _dev_grad(o, pad=4, misalign=False):
    """grad_out [B, T*D] with batch stride T*D + pad, NaN in the pad columns."""
    B, T, D = o.G.shape
    gbs = T * D + pad
    if not misalign:
        return padded(o.G.reshape(B, T * D).to(dev), 2, pad, NAN), gbs
    flat = torch.full((B * gbs + 8,), NAN, device=dev)
    a = 1 if misalign else 0
    G = flat[a:a + B * gbs].view(B, gbs)
    G[:, :T * D] = o.G.reshape(B, T * D).to(dev)
    return G, gbs


def _out_buffer(c, D, pad):
    """Pooled output [B, T*D] inside a SENTINEL buffer: ``pad`` extra columns, 2 guard rows."""
    return padded(torch.full((c.B, c.T * D), SENTINEL, device=dev), 2, pad, SENTINEL)


def _where(c, o, got, ref):
    """The first differing touched row, placed for the reader: table, run, block edges."""
    bad = np.flatnonzero((got != ref).reshape(got.shape[0], -1).any(1).numpy())
    if bad.size == 0:
        return "equal"
    row = int(o.urows[bad[0]])
    t = int(np.searchsorted(c.row_base, row, side="right") - 1)
    s, n, _ = c.runs[c.runs[:, 2] == row][0]
    return (f"{bad.size} rows differ; first: global row {row} (table {t}), run [{s}, {s + n}) "
            f"of the device-wide order = {s % 16}+{n} mod 16, {s % 64}+{n} mod 64; "
            f"got {got[bad[0]].flatten()[:4].tolist()} ref {ref[bad[0]].flatten()[:4].tolist()}")


def _backward(ops, name, D, mode, weighted, mx=0, tune=None, path="plain", misalign=None,
              half=False, lr=2.0 ** -4, idx_dtypes=None, skip_tables=(), flag=None):
    """Run one backward and require the exact reference on the touched rows, the old bits
    everywhere else, and the expected error flag.  ``path``: plain | presort (the sort in the
    lookup launch) | sort_any (tbe_backward_sort first) | defer (the passes as roles of two
    grouped-GEMM launches).  ``skip_tables``: tables whose update a violated cap skips."""
    c = _case(name)
    if idx_dtypes is not None:
        c = c.with_dtypes(*idx_dtypes)
    o, gsum = _operands(name, D, weighted, lr)
    assert E.exact_conditions_ok(c, o, zero_rows=[int(c.runs_spec[c.runs_spec[:, 1] == 2][0, 2])]
                                 if name == "cancel" else ()) == (True, "")
    start, ref, mref = _reference(o, gsum, mode, half)
    for t in skip_tables:
        sk = torch.from_numpy((o.urows >= c.row_base[t]) & (o.urows < c.row_base[t + 1]))
        ref = torch.where(sk[:, None], start, ref)
        if mref is not None:
            mref = torch.where(sk, o.mom0u, mref)
    idx, off, rb = c.device_csr(dev)
    W = _dev_rows(c, o, start, misalign == "W")
    G, gbs = _dev_grad(o, pad=1 if misalign == "stride" else 4, misalign=misalign == "G")
    mom = _dev_vec(c, o, o.mom0u) if mode == "rowwise_adagrad" else None
    psw = None if o.psw is None else o.psw.to(dev)
    W_before = W.clone()
    mom_before = None if mom is None else mom.clone()
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.zeros(ops.tbe_backward_workspace_size(c.N, c.total_rows, D), dtype=torch.uint8,
                     device=dev)
    kw = dict(lr=o.lr, eps=o.eps, momentum=mom, per_sample_weights=psw, grad_batch_stride=gbs,
              workspace=ws, max_lookups_per_table=mx, error_flag=err)
    with ops.tuning(**(tune or {})):
        if path == "presort":
            out = _out_buffer(c, D, 4)
            ops.tbe_forward_presort(W, rb, c.T, c.B, idx, off, ws, mx, out=out,
                                    out_batch_stride=c.T * D + 4, per_sample_weights=psw,
                                    error_flag=err)
            ops.tbe_backward(mode, W, rb, c.T, c.B, idx, off, G, presorted=True, **kw)
            fwd = E.ref_forward(c, o, start)
            assert torch.equal(out.cpu().reshape(c.B, c.T, D), fwd) and pads_intact(out)
        elif path == "sort_any":
            ops.tbe_backward_sort(W, rb, c.T, c.B, idx, off, ws, mx, per_sample_weights=psw,
                                  error_flag=err)
            ops.tbe_backward(mode, W, rb, c.T, c.B, idx, off, G, presorted=ops.PRESORTED_ANY,
                             **kw)
        elif path == "defer":
            role = ops.tbe_backward_defer(mode, W, rb, c.T, c.B, idx, off, G, **kw)
            assert role is not None and ops.role_blocks(role) > 0
            assert bool(torch.equal(W.view(torch.int32), W_before.view(torch.int32)))
            ops.gemm_group([], ws, dev, role=role, phase=1)
            ops.gemm_group([], ws, dev, role=role, phase=2)
        else:
            ops.tbe_backward(mode, W, rb, c.T, c.B, idx, off, G, **kw)
    torch.cuda.synchronize()
    u = torch.from_numpy(o.urows).to(dev)
    got = W[u].cpu()
    assert torch.equal(got, ref), _where(c, o, got, ref)
    assert E.untouched_intact(W_before, W, o.urows), "an untouched weight row changed"
    if mom is not None:
        gm = mom[u].cpu()
        assert torch.equal(gm, mref), _where(c, o, gm[:, None], mref[:, None])
        assert E.untouched_intact(mom_before, mom, o.urows), "an untouched momentum changed"
    assert int(err.item()) == (c.flag if flag is None else flag)


# ------------------------------------------------------------------ a. forward ----
def _forward_case(D, invalid, pair):
    """Two tables (40 and 3 rows); bag lengths 0, 1, LPB-1, LPB, LPB+1 for the lane groups
    of the float4 and of the scalar kernel at this D, 9 (= 4k + 1) and 130."""
    lens = {0, 1, 9, 130}
    for aligned in (True, False):
        lpb = E.dispatch(D, aligned)[1]
        lens |= {max(lpb - 1, 0), lpb, lpb + 1}
    lens = sorted(lens)
    inv = [(3, 40), (sum(lens) + 5, -1)] if invalid else []
    return E.bags_csr(f"fwd{D}", [40, 3], [lens, lens[::-1]], seed=D, invalid=inv,
                      idx_dtype=pair[0], off_dtype=pair[1])


def _forward_operands(c, D, weighted, seed):
    gen = torch.Generator().manual_seed(seed)
    o = E.Operands()
    o.D = D
    o.urows = np.unique(c.row[c.valid])
    o.W0u = int_matrix((o.urows.size, D), -64, 64, gen)
    o.psw = int_matrix((c.N,), -3, 3, gen) if weighted else None
    assert 130 * 3 * 64 < 2 ** 24  # every partial sum of a bag is a representable integer
    return o


@pytest.mark.parametrize("D", D_FWD)
def test_forward_exact(ops, D):
    """Every LPB / VW / MAXV of the lookup: float4 rows (pad 4) and the scalar fallback (an
    out_batch_stride that is no multiple of 4), unweighted and weighted, with and without
    invalid indices, the four index / offset dtype pairs in turn; both entry points."""
    n = 0
    for pad in (4, 1):
        if E.dispatch(D, pad == 4)[2] > 8:
            continue  # the scalar kernel takes D <= 512 (refusal: test_d_2052_is_refused)
        for weighted in (False, True):
            for invalid in (False, True):
                c = _forward_case(D, invalid, E.IDX_PAIRS[n % 4])
                n += 1
                o = _forward_operands(c, D, weighted, n)
                ref = E.ref_forward(c, o, o.W0u)
                idx, off, rb = c.device_csr(dev)
                W = _dev_rows(c, o, o.W0u)
                psw = None if o.psw is None else o.psw.to(dev)
                for presort in (False, True):
                    out = _out_buffer(c, D, pad)
                    err = torch.zeros(1, dtype=torch.int32, device=dev)
                    kw = dict(out=out, out_batch_stride=c.T * D + pad, per_sample_weights=psw,
                              error_flag=err)
                    if presort:
                        ws = torch.zeros(ops.tbe_backward_workspace_size(c.N, c.total_rows, D),
                                         dtype=torch.uint8, device=dev)
                        ops.tbe_forward_presort(W, rb, c.T, c.B, idx, off, ws, c.max_table, **kw)
                    else:
                        ops.tbe_forward(W, rb, c.T, c.B, idx, off, **kw)
                    torch.cuda.synchronize()
                    what = (D, pad, weighted, invalid, presort)
                    assert torch.equal(out.cpu().reshape(c.B, c.T, D), ref), what
                    assert pads_intact(out), what
                    assert int(err.item()) == c.flag == (E.ERR_INDEX if invalid else 0), what


def test_forward_misaligned_weights_take_the_scalar_kernel(ops):
    D = 64
    for weighted in (False, True):
        c = _forward_case(D, True, E.IDX_PAIRS[1])
        o = _forward_operands(c, D, weighted, 3)
        idx, off, rb = c.device_csr(dev)
        W = _dev_rows(c, o, o.W0u, misalign=True)
        assert W.data_ptr() % 16 == 4
        out = _out_buffer(c, D, 4)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.tbe_forward(W, rb, c.T, c.B, idx, off, out=out, out_batch_stride=c.T * D + 4,
                        per_sample_weights=None if o.psw is None else o.psw.to(dev),
                        error_flag=err)
        assert torch.equal(out.cpu().reshape(c.B, c.T, D), E.ref_forward(c, o, o.W0u))
        assert pads_intact(out) and int(err.item()) == E.ERR_INDEX


@pytest.mark.parametrize("D", D_FWD)
def test_forward_full_mantissa_bags_of_one(ops, D):
    """Bags of length 1 over full-mantissa rows: the output is a bit copy of the row, or,
    weighted by a full-mantissa weight, the one correctly rounded product."""
    c = E.bags_csr(f"one{D}", [40, 9], [[1] * 8, [1] * 8], seed=D, distinct=True)
    gen = torch.Generator().manual_seed(D)
    o = E.Operands()
    o.urows = np.unique(c.row)
    Wu = full_mantissa((o.urows.size, D), gen) * int_matrix((o.urows.size, 1), -1, 1, gen)
    psw = full_mantissa((c.N,), gen)
    idx, off, rb = c.device_csr(dev)
    W = _dev_rows(c, o, Wu)
    rows = Wu[torch.from_numpy(np.searchsorted(o.urows, c.row))]  # lookup p = bag p
    for w in (None, psw):
        out = _out_buffer(c, D, 4)
        ops.tbe_forward(W, rb, c.T, c.B, idx, off, out=out, out_batch_stride=c.T * D + 4,
                        per_sample_weights=None if w is None else w.to(dev))
        got = out.cpu().reshape(c.B, c.T, D).permute(1, 0, 2).reshape(c.N, D)
        ref = rows if w is None else (w.double()[:, None] * rows.double()).float()
        assert E.bits_equal(got, ref) and pads_intact(out)
    assert not torch.equal((psw[:, None] * rows.double()).float().double(),
                           psw[:, None] * rows.double())  # the products do round


def test_d_2052_is_refused_and_nothing_is_written(ops):
    """513 float4 chunks need 9 per lane: UNSUPPORTED from the lookup and from every
    backward mode, before any row or output element is written."""
    from dlrm_hip import _lib
    D = 2052
    c = _case("n7")
    o = E.make_operands(c, D, False, seed=1)
    idx, off, rb = c.device_csr(dev)
    W = _dev_rows(c, o, o.W0u)
    before = W.clone()
    out = _out_buffer(c, D, 4)
    with pytest.raises(_lib.DLRMHipError, match="UNSUPPORTED"):
        ops.tbe_forward(W, rb, c.T, c.B, idx, off, out=out, out_batch_stride=c.T * D + 4)
    G, gbs = _dev_grad(o)
    mom = _dev_vec(c, o, o.mom0u)
    mom_before = mom.clone()
    for mode in MODES:
        with pytest.raises(_lib.DLRMHipError, match="UNSUPPORTED"):
            ops.tbe_backward(mode, W, rb, c.T, c.B, idx, off, G, lr=o.lr, eps=o.eps,
                             momentum=mom, grad_batch_stride=gbs)
    torch.cuda.synchronize()
    assert bool((out._base == SENTINEL).all())
    assert E.bits_equal(W, before) and E.bits_equal(mom, mom_before)


# ------------------------------------------------------ b. backward dispatch on D ----
@pytest.mark.parametrize("block", [16, 64])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", D_BWD)
def test_backward_dispatch_on_d(ops, D, mode, weighted, block):
    _backward(ops, "skewed", D, mode, weighted, tune=dict(tbe_block=block))


@pytest.mark.parametrize("block", [16, 64])
@pytest.mark.parametrize("mode", ["sgd", "rowwise_adagrad"])
@pytest.mark.parametrize("passes", ["in_flight_16", "deferred"])
@pytest.mark.parametrize("D", D_LEAN)
def test_backward_lean_16_in_flight_and_deferred(ops, D, passes, mode, block):
    """float4 rows of one chunk per lane without per-sample weights: test_backward_dispatch_on_d
    ran the lean passes (the default); here the 16-in-flight kernels and the same lean bodies
    as roles of two grouped-GEMM launches that carry no GEMM."""
    if passes == "deferred":
        _backward(ops, "skewed", D, mode, False, tune=dict(tbe_block=block), path="defer")
    else:
        _backward(ops, "skewed", D, mode, False, tune=dict(tbe_block=block, tbe_lean=1))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("misalign", ["W", "G", "stride"])
def test_backward_scalar_fallback_at_d64(ops, misalign, mode, weighted):
    """D = 64 is float4 work unless the weights or grad_out are not 16-byte aligned or the
    grad_out batch stride is T*D + 1: then VW = 1, LPB = 64."""
    _backward(ops, "skewed", 64, mode, weighted, misalign=misalign)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [4, 12, 32, 100, 256, 512])
def test_backward_scalar_rows_of_every_lane_group(ops, D, mode):
    """The D list reaches the scalar kernels only at LPB 1, 8 and 64 / MAXV 1; a grad_out
    batch stride of T*D + 1 runs them at LPB 4, 16, 32 and at 2, 4 and 8 rows per lane
    (scalar rows of D > 64)."""
    assert E.dispatch(D, aligned=False) == {4: (1, 4, 1), 12: (1, 16, 1), 32: (1, 32, 1),
                                            100: (1, 64, 2), 256: (1, 64, 4),
                                            512: (1, 64, 8)}[D]
    for weighted in (False, True):
        _backward(ops, "skewed", D, mode, weighted, misalign="stride",
                  tune=dict(tbe_block=64 if weighted else 16))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("D,misalign", [(16, None), (64, None), (128, None), (512, None),
                                        (64, "W")])
def test_backward_sgd_fp16_rows(ops, D, misalign, weighted):
    """fp16 rows: w - lr g is exact in fp32, then rounded once to fp16 (lr = 2^-9: the fp16
    rounding does happen); a view one half into its buffer takes the scalar kernel."""
    for block in (16, 64):
        _backward(ops, "skewed", D, "sgd", weighted, half=True, lr=2.0 ** -9, misalign=misalign,
                  tune=dict(tbe_block=block))
    o, gsum = _operands("skewed", D, weighted, 2.0 ** -9)
    exact = o.W0u.double() - o.lr * gsum
    assert not torch.equal(exact.float().half().double(), exact)


# --------------------------------------------------- c. backward run structure ----
@pytest.mark.parametrize("block", [16, 64])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("sort", ["device_wide", "per_table"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [16, 128])
def test_backward_run_structure(ops, D, mode, sort, weighted, block):
    """Every way a run can lie against the block edges (test_exact_tbe_cpu asserts the case
    holds them all, at 16 and at 64 lookups per block, in either sorted layout)."""
    c = _case("structure")
    _backward(ops, "structure", D, mode, weighted, tune=dict(tbe_block=block),
              mx=0 if sort == "device_wide" else c.max_table)


@pytest.mark.parametrize("block", [16, 64])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["n1", "n7", "n128"])
def test_backward_small_n(ops, name, mode, block):
    """N = 1, N < 16, N a multiple of both block lengths."""
    for D in (16, 128):
        for weighted in (False, True):
            _backward(ops, name, D, mode, weighted, tune=dict(tbe_block=block))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [16, 128])
def test_backward_cancelled_gradient_leaves_the_row(ops, D, mode):
    """A touched row whose two gradients cancel, eps > 0: weights and momentum keep their
    values (the reference holds them: w - lr 0 / (sqrt(m) + eps), m + 0)."""
    c = _case("cancel")
    row = int(c.runs_spec[c.runs_spec[:, 1] == 2][0, 2])
    for weighted in (False, True):
        o, gsum = _operands("cancel", D, weighted)
        k = int(np.searchsorted(o.urows, row))
        assert not gsum[k].any() and o.eps > 0
        start, ref, mref = _reference(o, gsum, mode)
        assert torch.equal(ref[k], start[k]) and (mref is None or mref[k] == o.mom0u[k])
        for block in (16, 64):
            _backward(ops, "cancel", D, mode, weighted, tune=dict(tbe_block=block))


# ------------------------------------------------------- d. backward sort variants ----
def _modes_once_dense(i):
    return ["sgd", "rowwise_adagrad"] + (["dense"] if i == 0 else [])


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("path", ["plain", "presort", "sort_any"])
@pytest.mark.parametrize("kind", ["rank", "radix"])
def test_backward_per_table_lds_sort(ops, kind, path, idx_dtype):
    """Tables of <= 512 lookups (rank sort) and of 513..4096 (radix passes), sorted in the
    backward, in the lookup launch, or by tbe_backward_sort.  (The packed position form of
    segsort_body is a template argument no kernel of the library instantiates.)"""
    name = "sort_" + kind
    c = _case(name)
    for i, weighted in enumerate((False, True)):
        for mode in _modes_once_dense(i):
            _backward(ops, name, 16, mode, weighted, mx=c.max_table, path=path,
                      idx_dtypes=(idx_dtype, torch.int64 if weighted else torch.int32))


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("scan", ["wide", "chunked"])
@pytest.mark.parametrize("name,D", [("sort_tiled", 16), ("sort_tiled10", 128)])
def test_backward_tiled_sort(ops, name, D, scan, idx_dtype):
    """One table of two tiles beside a small and an empty table.  At D = 16 the workspace
    (sized by N and D alone) is too small for the 10-bit histograms of 3 tables, so the
    sort falls back to the 8-bit digits of the device-wide class; sort_tiled10 at D = 128
    is the smallest batch whose workspace holds them."""
    c = _case(name)
    assert E.SEG_CAP < c.max_table <= 2 * E.SEG_CAP
    words10 = c.T * (2 + 64) * 1024  # T * (tiles + scan chunks) * 2^10
    part = max(2 * -(-c.N // 16) * D, -(-c.N // 4096) * 1024 + 64 * 1024)
    assert (words10 <= part) == (name == "sort_tiled10")
    tune = dict(tbe_sort=2) if scan == "chunked" else {}
    for i, weighted in enumerate((False, True)):
        for mode in _modes_once_dense(i):
            _backward(ops, name, D, mode, weighted, mx=c.max_table, tune=tune,
                      idx_dtypes=(idx_dtype, torch.int32))
    _backward(ops, name, D, "sgd", False, mx=c.max_table, tune=tune, path="sort_any",
              idx_dtypes=(idx_dtype, torch.int64))


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("bound", ["none", "forced"])
@pytest.mark.parametrize("rows", sorted(E.GLOBAL_ROW_CLASSES))
def test_backward_device_wide_sort_digit_classes(ops, rows, bound, idx_dtype):
    """The five (digit width, pass count) classes of the device-wide sort, without a bound
    and forced (tbe_sort=1) under a bound above 4096; unweighted the sort carries bags,
    weighted positions; an even pass count leaves the result in the other buffer pair."""
    name = f"sort_rows{rows}"
    c = _case(name)
    assert E.digit_class(c.total_rows) == E.GLOBAL_ROW_CLASSES[rows]
    mx, tune = (0, {}) if bound == "none" else (5000, dict(tbe_sort=1))
    for i, weighted in enumerate((False, True)):
        for mode in _modes_once_dense(i):
            _backward(ops, name, 16, mode, weighted, mx=mx, tune=tune,
                      idx_dtypes=(idx_dtype, torch.int32))
    _backward(ops, name, 16, "rowwise_adagrad", True, mx=mx, tune=tune, path="sort_any",
              idx_dtypes=(idx_dtype, torch.int64))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_backward_violated_table_cap_skips_that_table_only(ops, mode, weighted):
    """A bound of 4096 under a table of 4201 lookups: that table is skipped and flagged, the
    other tables are updated exactly, every other row keeps its bits."""
    c = _case("sort_tiled")
    assert c.table_lookups[2] > E.SEG_CAP >= c.table_lookups[0] > 0
    _backward(ops, "sort_tiled", 16, mode, weighted, mx=E.SEG_CAP, skip_tables=(2,),
              flag=E.ERR_INDEX | E.ERR_TABLE_CAP)


# ----------------------------------------------- e. psw_grad and expand_grad ----
@pytest.mark.parametrize("D", [d for d in D_FWD if d <= 512])
def test_psw_grad_and_expand_grad_exact(ops, D):
    """Integer dot products and integer products on the variable-length case; lookups
    outside every bag give 0 in both, an out-of-range index gives 0 in psw_grad (expand_grad
    does not see the indices)."""
    for n, pad in enumerate((4, 1)):
        c = _case("sort_rank").with_dtypes(*E.IDX_PAIRS[(D + n) % 4])
        o = E.make_operands(c, D, True, seed=D)  # (no update here: no backward conditions)
        assert D * 8 * 64 < 2 ** 24  # every dot product is a representable integer
        idx, off, rb = c.device_csr(dev)
        W = _dev_rows(c, o, o.W0u)
        G, gbs = _dev_grad(o, pad=pad)
        got = ops.tbe_psw_grad(W, rb, c.T, c.B, idx, off, G, grad_batch_stride=gbs).cpu()
        ref = E.ref_psw_grad(c, o, o.W0u)
        assert torch.equal(got, ref) and not ref[torch.from_numpy(~c.valid)].any()
        for psw in (None, o.psw):
            o2 = E.Operands()
            o2.G, o2.psw, o2.D = o.G, psw, D
            got = ops.tbe_expand_grad(D, c.T, c.B, off, c.N, G, grad_batch_stride=gbs,
                                      per_sample_weights=None if psw is None else psw.to(dev))
            ref = E.ref_expand_grad(c, o2)
            assert torch.equal(got.cpu(), ref)
            assert not ref[torch.from_numpy(c.bag < 0)].any()
