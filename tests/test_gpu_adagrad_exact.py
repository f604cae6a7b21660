"""Exact-arithmetic tests of the embedding backward's element-wise Adagrad mode
(ops.tbe_backward("adagrad"), MODE_ADAGRAD_ELEM): against exact_adagrad.ref_adagrad_elem on
the cases of test_gpu_tbe_exact.py, and - on full-mantissa data at the default eps - against the
dense accumulation followed by the dense Adagrad kernel over the whole table.

BIT FOR BIT, no tolerance in this file.  Weight and state rows no lookup references hold NaN and
must keep their bits; the error flag must be exactly the expected bits."""
import functools

import numpy as np
import pytest
import torch

import exact_adagrad as A
import exact_tbe as E
import test_gpu_tbe_exact as T

pytestmark = pytest.mark.gpu

dev = T.dev
D_BWD = T.D_BWD


@pytest.fixture(scope="module")
def ops():
    from dlrm_hip import ops as _ops
    return _ops


@functools.lru_cache(maxsize=64)
def _reference(name, D, weighted, lr=2.0 ** -4):
    """(operands, start state, reference rows, reference state): built once, never changed."""
    o, gsum = T._operands(name, D, weighted, lr)
    S0 = A.start_state(o)
    W, S = A.ref_adagrad_elem(o.W0u, S0, gsum, o.lr, o.eps)
    return o, S0, W, S


def _adagrad(ops, name, D, weighted, mx=0, tune=None, path="plain", misalign=None,
             idx_dtypes=None, skip_tables=(), flag=None, device_lr=False):
    """One backward in mode 'adagrad': the exact reference on the touched rows of W and S, the
    old bits (NaN guard rows) everywhere else, the expected error flag.  ``misalign``: W | S |
    G | stride (the scalar kernels).  Returns (W, S) of the touched rows."""
    c = T._case(name)
    if idx_dtypes is not None:
        c = c.with_dtypes(*idx_dtypes)
    o, S0, Wref, Sref = _reference(name, D, weighted)
    for t in skip_tables:
        sk = torch.from_numpy((o.urows >= c.row_base[t]) & (o.urows < c.row_base[t + 1]))
        Wref = torch.where(sk[:, None], o.W0u, Wref)
        Sref = torch.where(sk[:, None], S0, Sref)
    idx, off, rb = c.device_csr(dev)
    W = T._dev_rows(c, o, o.W0u, misalign == "W")
    S = T._dev_rows(c, o, S0, misalign == "S")
    assert W.data_ptr() % 16 == (4 if misalign == "W" else 0)
    assert S.data_ptr() % 16 == (4 if misalign == "S" else 0)
    G, gbs = T._dev_grad(o, pad=1 if misalign == "stride" else 4, misalign=misalign == "G")
    psw = None if o.psw is None else o.psw.to(dev)
    W_before, S_before = W.clone(), S.clone()
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.zeros(ops.tbe_backward_workspace_size(c.N, c.total_rows, D), dtype=torch.uint8,
                     device=dev)
    lr = torch.tensor([o.lr], dtype=torch.float32, device=dev) if device_lr else o.lr
    kw = dict(lr=lr, eps=o.eps, momentum=S, per_sample_weights=psw, grad_batch_stride=gbs,
              workspace=ws, max_lookups_per_table=mx, error_flag=err)
    with ops.tuning(**(tune or {})):
        if path == "presort":
            out = T._out_buffer(c, D, 4)
            ops.tbe_forward_presort(W, rb, c.T, c.B, idx, off, ws, mx, out=out,
                                    out_batch_stride=c.T * D + 4, per_sample_weights=psw,
                                    error_flag=err)
            ops.tbe_backward("adagrad", W, rb, c.T, c.B, idx, off, G, presorted=True, **kw)
        elif path == "sort_any":
            ops.tbe_backward_sort(W, rb, c.T, c.B, idx, off, ws, mx, per_sample_weights=psw,
                                  error_flag=err)
            ops.tbe_backward("adagrad", W, rb, c.T, c.B, idx, off, G,
                             presorted=ops.PRESORTED_ANY, **kw)
        else:
            ops.tbe_backward("adagrad", W, rb, c.T, c.B, idx, off, G, **kw)
    torch.cuda.synchronize()
    u = torch.from_numpy(o.urows).to(dev)
    gotW, gotS = W[u].cpu(), S[u].cpu()
    assert E.bits_equal(gotS, Sref), "S: " + T._where(c, o, gotS, Sref)
    assert E.bits_equal(gotW, Wref), "W: " + T._where(c, o, gotW, Wref)
    assert E.untouched_intact(W_before, W, o.urows), "an untouched weight row changed"
    assert E.untouched_intact(S_before, S, o.urows), "an untouched state row changed"
    assert int(err.item()) == (c.flag if flag is None else flag)
    return gotW, gotS


# ------------------------------------------------------------ dispatch on D ----
@pytest.mark.parametrize("block", [16, 64])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("D", D_BWD)
def test_adagrad_dispatch_on_d(ops, D, weighted, block):
    """Every LPB / VW / MAXV that BY_LPB dispatches, both block lengths, per-sample weights."""
    _adagrad(ops, "skewed", D, weighted, tune=dict(tbe_block=block))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("misalign", ["W", "S", "G", "stride"])
def test_adagrad_scalar_fallback_at_d64(ops, misalign, weighted):
    """D = 64 is float4 work unless W, S or grad_out is not 16-byte aligned or the grad_out
    batch stride is T*D + 1: then VW = 1, LPB = 64."""
    _adagrad(ops, "skewed", 64, weighted, misalign=misalign)


@pytest.mark.parametrize("D", [4, 12, 32, 100, 256, 512])
def test_adagrad_scalar_rows_of_every_lane_group(ops, D):
    """The scalar kernels at LPB 4, 16, 32 and at 2, 4 and 8 rows per lane."""
    assert E.dispatch(D, aligned=False)[0] == 1
    for weighted in (False, True):
        _adagrad(ops, "skewed", D, weighted, misalign="stride",
                 tune=dict(tbe_block=64 if weighted else 16))


# ------------------------------------------------------------ run structure ----
@pytest.mark.parametrize("block", [16, 64])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("sort", ["device_wide", "per_table"])
@pytest.mark.parametrize("D", [16, 128])
def test_adagrad_run_structure(ops, D, sort, weighted, block):
    """Every way a run can lie against the block edges: rows finalised in the block pass
    (finalize_row_pf at D = 16 .. 128, one chunk per lane) and in the combine pass."""
    c = T._case("structure")
    _adagrad(ops, "structure", D, weighted, tune=dict(tbe_block=block),
             mx=0 if sort == "device_wide" else c.max_table)


def test_adagrad_run_structure_without_the_prefetch(ops):
    """D = 260 takes two chunks per lane: finalize_row in the block pass (no prefetch)."""
    assert E.dispatch(260)[2] == 2
    for block in (16, 64):
        _adagrad(ops, "structure", 260, False, tune=dict(tbe_block=block))


@pytest.mark.parametrize("block", [16, 64])
@pytest.mark.parametrize("name", ["n1", "n7", "n128"])
def test_adagrad_small_n(ops, name, block):
    for D in (16, 128):
        for weighted in (False, True):
            _adagrad(ops, name, D, weighted, tune=dict(tbe_block=block))


@pytest.mark.parametrize("D", [16, 128])
def test_adagrad_cancelled_gradient_leaves_the_row(ops, D):
    """g = 0 on a touched row: S + 0 and W - lr * 0 / (sqrt(S) + eps) keep their bits, also
    where S is 0 (eps > 0)."""
    c = T._case("cancel")
    row = int(c.runs_spec[c.runs_spec[:, 1] == 2][0, 2])
    for weighted in (False, True):
        o, S0, Wref, Sref = _reference("cancel", D, weighted)
        k = int(np.searchsorted(o.urows, row))
        assert o.eps > 0 and bool((S0[k] == 0).any())
        assert torch.equal(Wref[k], o.W0u[k]) and torch.equal(Sref[k], S0[k])
        for block in (16, 64):
            gotW, gotS = _adagrad(ops, "cancel", D, weighted, tune=dict(tbe_block=block))
            assert E.bits_equal(gotW[k], o.W0u[k]) and E.bits_equal(gotS[k], S0[k])


# ------------------------------------------------------------ sort variants, paths ----
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("path", ["plain", "presort", "sort_any"])
@pytest.mark.parametrize("kind", ["rank", "radix"])
def test_adagrad_per_table_lds_sort(ops, kind, path, idx_dtype):
    """The per-table sort run in the backward, in the lookup launch (presorted = True) or by
    tbe_backward_sort (PRESORTED_ANY); the four index / offset widths."""
    name = "sort_" + kind
    c = T._case(name)
    for weighted in (False, True):
        _adagrad(ops, name, 16, weighted, mx=c.max_table, path=path,
                 idx_dtypes=(idx_dtype, torch.int64 if weighted else torch.int32))


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("name,D", [("sort_tiled", 16), ("sort_tiled10", 128)])
def test_adagrad_tiled_sort(ops, name, D, idx_dtype):
    c = T._case(name)
    assert E.SEG_CAP < c.max_table <= 2 * E.SEG_CAP
    for weighted in (False, True):
        _adagrad(ops, name, D, weighted, mx=c.max_table, idx_dtypes=(idx_dtype, torch.int32))
    _adagrad(ops, name, D, False, mx=c.max_table, path="sort_any",
             idx_dtypes=(idx_dtype, torch.int64))


@pytest.mark.parametrize("rows", sorted(E.GLOBAL_ROW_CLASSES))
def test_adagrad_device_wide_sort_digit_classes(ops, rows):
    """The device-wide sort's (digit width, pass count) classes: unweighted the sort carries
    bags, weighted positions; an even pass count leaves the result in the other buffers."""
    name = f"sort_rows{rows}"
    for weighted in (False, True):
        _adagrad(ops, name, 16, weighted,
                 idx_dtypes=(torch.int64 if weighted else torch.int32, torch.int32))
    _adagrad(ops, name, 16, True, path="sort_any", idx_dtypes=(torch.int32, torch.int64))


@pytest.mark.parametrize("weighted", [False, True])
def test_adagrad_violated_table_cap_skips_that_table_only(ops, weighted):
    c = T._case("sort_tiled")
    assert c.table_lookups[2] > E.SEG_CAP >= c.table_lookups[0] > 0
    _adagrad(ops, "sort_tiled", 16, weighted, mx=E.SEG_CAP, skip_tables=(2,),
             flag=E.ERR_INDEX | E.ERR_TABLE_CAP)


@pytest.mark.parametrize("D,misalign", [(16, None), (128, None), (260, None), (64, "S")])
def test_adagrad_device_rate_equals_host_rate(ops, D, misalign):
    """lr as a 1-element device tensor: the same bits (both equal the reference)."""
    a = _adagrad(ops, "skewed", D, False, misalign=misalign)
    b = _adagrad(ops, "skewed", D, False, misalign=misalign, device_lr=True)
    assert E.bits_equal(a[0], b[0]) and E.bits_equal(a[1], b[1])


# ---------------------------------------------- sparse equals dense, full mantissa ----
@pytest.mark.parametrize("D", [16, 128, 260])
def test_adagrad_sparse_equals_dense_on_full_mantissa_data(ops, D):
    """Normal-random W and G, S = |normal|, multi-hot bags with duplicate rows, eps = 1e-10
    (the default): tbe_backward('dense') into a zero buffer, then the dense Adagrad kernel
    over the whole table and state, must equal tbe_backward('adagrad') on every row of W and
    S.  Both coalesce with the same sort and the same compensated sums, and both apply
    s = fma(g, g, S); W = fma(-lr, g / (sqrt(s) + eps), W): no tolerance could pin the kernel
    on data this ill-conditioned, the identity does."""
    rng = np.random.default_rng(D)
    rows = [50, 7, 300]
    lens = [rng.integers(0, 7, 40).tolist() for _ in rows]
    c = E.bags_csr(f"sd{D}", rows, lens, seed=D)
    assert np.unique(c.row).size < c.N  # duplicates
    gen = torch.Generator().manual_seed(D)
    R = c.total_rows
    W = torch.randn(R, D, generator=gen).to(dev)
    S = torch.randn(R, D, generator=gen).abs().to(dev)
    G = torch.randn(c.B, c.T * D, generator=gen).to(dev)
    lr, eps = 0.01, 1e-10
    idx, off, rb = c.device_csr(dev)
    for mx in (0, c.max_table):
        Wd, Sd = W.clone(), S.clone()
        Gd = torch.zeros(R, D, device=dev)
        ops.tbe_backward("dense", Gd, rb, c.T, c.B, idx, off, G, max_lookups_per_table=mx)
        ops.adagrad_update(Wd.view(-1), Gd.view(-1), Sd.view(-1), lr, eps)
        Ws, Ss = W.clone(), S.clone()
        ops.tbe_backward("adagrad", Ws, rb, c.T, c.B, idx, off, G, lr=lr, eps=eps, momentum=Ss,
                         max_lookups_per_table=mx)
        torch.cuda.synchronize()
        assert E.bits_equal(Ss, Sd) and E.bits_equal(Ws, Wd), (D, mx)
        touched = torch.from_numpy(np.unique(c.row)).to(dev)
        assert not E.bits_equal(Ws[touched], W[touched])  # the update did happen


# ------------------------------------------------------------------- refusals ----
def test_adagrad_mode_argument_checks(ops):
    c = T._case("n7")
    o, S0, _, _ = _reference("n7", 16, False)
    idx, off, rb = c.device_csr(dev)
    W = T._dev_rows(c, o, o.W0u)
    S = T._dev_rows(c, o, S0)
    G, gbs = T._dev_grad(o)
    W0, S0d = W.clone(), S.clone()
    kw = dict(lr=o.lr, eps=o.eps, grad_batch_stride=gbs)
    wide = torch.zeros(c.total_rows, 32, device=dev)
    bad_states = [None, S[:-1], S.double(), S.half(), wide[:, :16], S.view(-1)]
    for bad in bad_states:
        with pytest.raises(ValueError, match="adagrad"):
            ops.tbe_backward("adagrad", W, rb, c.T, c.B, idx, off, G, momentum=bad, **kw)
    with pytest.raises(ValueError, match="fp32 weights"):
        ops.tbe_backward("adagrad", W.half(), rb, c.T, c.B, idx, off, G, momentum=S, **kw)
    with pytest.raises(ValueError, match="sr_state"):
        ops.tbe_backward("adagrad", W, rb, c.T, c.B, idx, off, G, momentum=S,
                         sr_state=ops.sr_state(1, 0, device=dev), **kw)
    with pytest.raises(ValueError, match="tbe_backward_defer"):
        ops.tbe_backward_defer("adagrad", W, rb, c.T, c.B, idx, off, G, momentum=S, **kw)
    torch.cuda.synchronize()
    assert E.bits_equal(W, W0) and E.bits_equal(S, S0d)


def test_optim_adagrad_steps_like_torch_on_exact_data(ops):
    """dlrm_hip.optim.Adagrad on a sparse=True EmbeddingBag and on a dense parameter: the bits
    of torch.optim.Adagrad on the CPU (integer data, lr a power of two)."""
    from dlrm_hip import optim
    c = T._case("n128")
    o, S0, Wref, Sref = _reference("n128", 16, False)
    D, t = 16, 1
    idx, off, _ = A.table_csr(c, t)
    lo, hi = int(c.row_base[t]), int(c.row_base[t + 1])
    W0 = torch.full((hi - lo, D), 3.0)
    mine = (o.urows >= lo) & (o.urows < hi)
    k = torch.from_numpy(o.urows[mine] - lo)
    W0[k] = o.W0u[torch.from_numpy(mine)]
    S_init = torch.zeros(hi - lo, D)
    S_init[k] = S0[torch.from_numpy(mine)]
    res = []
    for device, cls in (("cpu", torch.optim.Adagrad), (dev, optim.Adagrad)):
        emb = torch.nn.EmbeddingBag(hi - lo, D, mode="sum", sparse=True).to(device)
        emb.weight.data = W0.clone().to(device)
        dense = torch.nn.Parameter(o.W0u.clone().to(device))
        opt = cls(list(emb.parameters()) + [dense], lr=o.lr, eps=o.eps)
        opt.state[emb.weight]["sum"].copy_(S_init)
        out = emb(torch.from_numpy(idx).to(device), torch.from_numpy(off).to(device))
        (out * o.G[:, t].to(device)).sum().backward()
        dense.grad = o.acc0u.clone().to(device)
        assert emb.weight.grad.is_sparse
        opt.step()
        res.append((emb.weight.detach().cpu(), opt.state[emb.weight]["sum"].cpu(),
                    dense.detach().cpu(), opt.state[dense]["sum"].cpu()))
        assert set(opt.state[dense]) == {"sum", "step"}
    for a, b in zip(*res):
        assert E.bits_equal(a, b)
    assert E.bits_equal(res[1][0][k], Wref[torch.from_numpy(mine)])
