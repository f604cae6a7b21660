"""Exact-arithmetic tests of the step's tail: the fused head through all four of its entry
points (dlrm_head_step, its deferred finalize in a grouped GEMM launch, dlrm_head_predict,
dlrm_head_forward_backward), the bias-gradient column sums, the dense optimizers, the small
elementwise / QR / CSR kernels and the device RNG fills, against the CPU references of
tests/exact_head.py.

Sections 1, 3 and 4 have no tolerance: the operands make fp32 arithmetic exact (or one
correctly rounded operation per output), so "equal" is torch.equal on a NaN-free result.
Section 2 (general logits) bounds the transcendental part by the ulp error MEASURED on the
MI355X plus one ulp, and holds everything after expf bitwise to the kernel's own prob.
Operands sit in NaN-padded buffers with a leading dimension wider than the row, outputs in
sentinel-padded buffers with guard rows, and the pads must be intact after every call.
DESIGN.md section 6 ("Exact-arithmetic coverage of the step's tail") says which case reaches
which branch."""
import functools

import numpy as np
import pytest
import torch

import exact_head as H
from eval_ref import pack_keys
from exact_inputs import SENTINEL, full_mantissa, gemm_close, int_matrix, padded, pads_intact

pytestmark = pytest.mark.gpu

dev = "cuda:0"
NAN = float("nan")
f32, f64 = np.float32, np.float64

# Largest fp32 ulp error of prob against the fp64 sigmoid of the exact logit, measured on an
# MI355X over every half-integer z in [-100, 24] whose sigmoid is a normal float32 (z >= -87;
# test_prob_sweep says what happens below): 1.147 ulp, the same through head_step,
# head_predict, head_forward_backward and sigmoid_forward.
PROB_ULP_MEASURED = 1.15
# Largest fp32 ulp error of the BCE row loss -logf(pc) / -logf(1 - pc) against the fp64 log of
# the same float32 argument, same sweep (read through loss_out at M = 1): 1.996 ulp.
LOGF_ULP_MEASURED = 2.0
LOSS_C = LOGF_ULP_MEASURED + 2  # the loss bound's c: the logf error plus two roundings

CLAMP_SHAPES = [(M, K) for (M, K) in H.HEAD_SHAPES if K in (2, 65, 2048) or (M, K) == (257, 321)]
GENERAL_SHAPES = [(5, 2), (37, 1089), (257, 65), (257, 2048), (1023, 321)]
KINDS = [("mse", "anchor"), ("bce", "anchor"), ("bce", "saturated")]


@pytest.fixture(scope="module")
def ops():
    from dlrm_hip import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib():
    from dlrm_hip import _lib
    return _lib


# -------------------------------------------------------------- device buffers ----
def _vec(src, fill=SENTINEL, guard=8):
    """A 1-D view (a copy of ``src``, or ``src`` elements of ``fill``) at the start of a
    buffer whose ``guard`` trailing elements hold ``fill``."""
    n = src if isinstance(src, int) else src.numel()
    dtype = torch.float32 if isinstance(src, int) else src.dtype
    buf = torch.full((n + guard,), fill, dtype=dtype, device=dev)
    v = buf[:n]
    if not isinstance(src, int):
        v.copy_(src)
    return v


def _vec_intact(v, fill=SENTINEL):
    tail = v._base[v.numel():]
    f = torch.full((), fill, dtype=tail.dtype, device=dev)
    if tail.dtype == torch.float32:
        return bool((tail.view(torch.int32) == f.view(torch.int32)).all())
    return bool((tail == f).all())


def _untouched(*views):
    """Every view still holds SENTINEL everywhere (nothing was written at all)."""
    return all(bool((v == SENTINEL).all()) and
               (pads_intact(v) if v.dim() == 2 else _vec_intact(v)) for v in views)


def _eq(got, ref, what=""):
    """torch.equal on a NaN-free result (signed zeros compare equal)."""
    got = got.detach().cpu()
    ref = torch.as_tensor(ref)
    assert not torch.isnan(got).any(), f"{what}: NaN in the output"
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} differ, first at {i}: "
                             f"got {got[i].item()!r} ref {ref[i].item()!r}")


def _bits_eq(got, ref, what=""):
    """Bitwise equality (for outputs that must carry a NaN through)."""
    g = got.detach().cpu().contiguous().view(torch.int32)
    r = torch.as_tensor(ref).contiguous().view(torch.int32)
    assert torch.equal(g, r), f"{what}: {(g != r).sum().item()} words differ"


# ------------------------------------------------------------------ head cases ----
@functools.lru_cache(maxsize=None)
def _hcase(M, K, loss, kind="anchor", grad_scale=None):
    return H.head_case(M, K, loss, kind, grad_scale=grad_scale)


@functools.lru_cache(maxsize=None)
def _href(M, K, loss, kind, lo, grad_scale=None):
    """The reference of a case: computed once, shared by every entry point, never changed."""
    return H.head_reference(_hcase(M, K, loss, kind, grad_scale), lo=lo)


class HeadBuffers:
    """Operands (NaN-padded) and outputs (SENTINEL-padded) of one head call on the device."""

    def __init__(self, c, w=None):
        self.c = c
        self.X = padded(c.X.to(dev), 2, 3, NAN)
        self.w = _vec(c.w if w is None else w, NAN)
        self.t = _vec(c.t, NAN)
        self.prob, self.dz, self.loss = _vec(c.M), _vec(c.M), _vec(1)
        self.dX = padded(torch.full((c.M, c.K), SENTINEL, device=dev), 2, 3, SENTINEL)
        self.dw = _vec(c.K)

    def kw(self, dw=True, dX=True):
        return dict(prob=self.prob, dz=self.dz, loss_out=self.loss,
                    dX=self.dX if dX else None, dw=self.dw if dw else None)

    def pads_ok(self):
        return (pads_intact(self.dX) and all(_vec_intact(v) for v in
                                             (self.prob, self.dz, self.loss, self.dw)) and
                _vec_intact(self.w, NAN))


def _loss_is_exact(c, lo):
    return c.loss == "mse" or (c.kind == "saturated" and lo == 0.0)


def _check_rows(b, r, lo, masked=True, loss=True, what=""):
    _eq(b.prob, r["prob"], what + " prob")
    _eq(b.dz, r["dz"], what + " dz")
    _eq(b.dX, r["dXm"] if masked else r["dXu"], what + " dX")
    if loss and _loss_is_exact(b.c, lo):
        _eq(b.loss, r["loss"], what + " loss")


def _head_shapes(shapes):
    return [pytest.param(M, K, loss, kind, id=f"{M}x{K}-{loss}-{kind}")
            for (M, K) in shapes for (loss, kind) in KINDS if K > 1 or kind == "anchor"]


# ---------------------------------------------------- 1. the head: anchor rows ----
@pytest.mark.parametrize("M,K,loss,kind", _head_shapes(H.HEAD_SHAPES))
def test_head_step_anchor(ops, M, K, loss, kind):
    """dlrm_head_step on anchor rows: prob, dz, dX (masked and unmasked), dw (stored and
    accumulated onto integers), the fused SGD on w (lr as a float and as a device tensor) and
    loss_out equal the reference; no tolerance."""
    c, r = _hcase(M, K, loss, kind), _href(M, K, loss, kind, 0.0)
    b = HeadBuffers(c)
    ops.head_step(b.X, b.w, b.t, loss, 0.0, c.grad_scale, relu_mask=True, **b.kw())
    _check_rows(b, r, 0.0, what="masked")
    _eq(b.dw, r["dw"], "dw stored")
    _eq(b.w, c.w, "w (dw given: no update)")
    assert b.pads_ok()

    b = HeadBuffers(c)
    g = torch.Generator().manual_seed(K)
    dw0 = int_matrix((K,), -8, 8, g)
    b.dw.copy_(dw0)
    ops.head_step(b.X, b.w, b.t, loss, 0.0, c.grad_scale, relu_mask=False, accumulate=True,
                  **b.kw())
    _check_rows(b, r, 0.0, masked=False, what="unmasked")
    _eq(b.dw, (dw0.double().numpy() + r["dw64"]).astype(f32), "dw accumulated")
    assert b.pads_ok()

    w_ref = H.ref_sgd_w(c.w.numpy(), r["dw64"], 2.0 ** -3)
    for lr in (2.0 ** -3, torch.tensor([2.0 ** -3], device=dev)):
        b = HeadBuffers(c)
        ops.head_step(b.X, b.w, b.t, loss, 0.0, c.grad_scale, lr=lr, **b.kw(dw=False))
        _check_rows(b, r, 0.0, what="sgd")
        _eq(b.w, w_ref, "fused SGD on w")
        assert b.pads_ok() and _untouched(b.dw)


@pytest.mark.parametrize("M,K,loss,kind", _head_shapes(CLAMP_SHAPES))
def test_head_step_clamp(ops, M, K, loss, kind):
    """clamp_lo = 0.25: the saturated rows lie outside the clamp - prob is lo or fl(1 - lo),
    dz and dX are 0 and the rows add nothing to dw."""
    c, r = _hcase(M, K, loss, kind), _href(M, K, loss, kind, 0.25)
    sat = c.z != 0
    assert set(np.unique(r["prob"][sat])) <= {f32(0.25), f32(0.75)}
    assert not r["dz"][sat].any() and not r["dXu"][sat].any()
    b = HeadBuffers(c)
    ops.head_step(b.X, b.w, b.t, loss, 0.25, c.grad_scale, relu_mask=True, **b.kw())
    _check_rows(b, r, 0.25, what="clamp")
    _eq(b.dw, r["dw"], "dw")
    assert b.pads_ok()


def _int_gemm():
    g = torch.Generator().manual_seed(3)
    A, B = int_matrix((70, 36), -3, 3, g, device=dev), int_matrix((36, 64), -3, 3, g, device=dev)
    return A, B, (A.double() @ B.double()).float().cpu()


@pytest.mark.parametrize("M,K,loss,kind", _head_shapes(H.HEAD_SHAPES))
def test_head_step_deferred(ops, M, K, loss, kind):
    """dlrm_head_step_defer + phase 4 of a grouped GEMM launch (an empty one; beside a real
    problem at K = 65 and 2048): the rows are written by the first launch, w / dw / loss_out
    only by the role's pass, and everything equals the reference - not merely head_step."""
    c, r = _hcase(M, K, loss, kind), _href(M, K, loss, kind, 0.0)
    beside = K in (65, 2048)
    A, B, Cref = _int_gemm() if beside else (None, None, None)
    for sgd in (False, True):
        b = HeadBuffers(c)
        lr = torch.tensor([2.0 ** -3], device=dev) if sgd and M % 2 else 2.0 ** -3
        role = ops.head_step(b.X, b.w, b.t, loss, 0.0, c.grad_scale, relu_mask=True,
                             lr=lr if sgd else 0.0, defer=True, **b.kw(dw=not sgd))
        assert ops.role_blocks(role) % 8 == 0 and ops.role_blocks(role) * 4 >= K
        _check_rows(b, r, 0.0, loss=False, what="deferred rows")
        _eq(b.w, c.w, "w before the role's pass")
        assert _untouched(b.dw, b.loss)
        probs = []
        if beside:
            p1, c1 = ops.gemm_problem(A, B)
            probs = [p1]
        ops.gemm_group(probs, None, dev, role=role, phase=4)
        _check_rows(b, r, 0.0, what="deferred")
        if sgd:
            _eq(b.w, H.ref_sgd_w(c.w.numpy(), r["dw64"], 2.0 ** -3), "deferred SGD on w")
            assert _untouched(b.dw)
        else:
            _eq(b.dw, r["dw"], "deferred dw")
            _eq(b.w, c.w, "w")
        if beside:
            _eq(c1, Cref, "the GEMM beside the role")
        assert b.pads_ok()


def _predict_params():
    out = []
    for (M, K) in H.HEAD_SHAPES:
        for lo in (0.0, 0.25) if (M, K) in CLAMP_SHAPES else (0.0,):
            out += [pytest.param(M, K, loss, "anchor", lo, id=f"{M}x{K}-{loss}-lo{lo}")
                    for loss in ("mse", "bce")]
    return out


@pytest.mark.parametrize("M,K,loss,kind,lo", _predict_params())
def test_head_predict_anchor(ops, M, K, loss, kind, lo):
    """dlrm_head_predict: prob equals the reference (not merely head_step's prob); with an
    EvalState the logged keys are pack_keys(reference prob, target)."""
    from dlrm_hip.metrics import EvalState
    c, r = _hcase(M, K, loss, kind), _href(M, K, loss, kind, lo)
    b = HeadBuffers(c)
    ops.head_predict(b.X, b.w, lo, prob=b.prob)
    _eq(b.prob, r["prob"], "prob")
    _eq(b.w, c.w, "w")
    assert b.pads_ok() and _untouched(b.dz, b.loss, b.dw, b.dX)
    if loss == "bce":
        keys = torch.full((M + 8,), -1, dtype=torch.int32, device=dev)
        st = EvalState(M, dev, keys=keys[:M])
        b = HeadBuffers(c)
        ops.head_predict(b.X, b.w, lo, prob=b.prob, target=b.t.contiguous(), state=st)
        _eq(b.prob, r["prob"], "prob (logging)")
        want = pack_keys(r["prob"], c.t.numpy()).view(np.int32)
        assert st.count == M
        assert torch.equal(keys[:M].cpu(), torch.from_numpy(want))
        assert bool((keys[M:] == -1).all())


@pytest.mark.parametrize("M,K,loss,kind", _head_shapes([s for s in H.HEAD_SHAPES if s[1] > 1]))
def test_head_forward_backward_anchor(ops, M, K, loss, kind):
    """dlrm_head_forward_backward (its own kernel, a separate bias pointer): prob, dz and the
    loss equal the same reference, at clamp_lo 0 and 0.25."""
    c = _hcase(M, K, loss, kind)
    for lo in (0.0, 0.25):
        r = _href(M, K, loss, kind, lo)
        b = HeadBuffers(c)
        Xv, wv, bias = b.X[:, :K - 1], b.w[:K - 1], _vec(c.w[K - 1:], NAN)
        ops.head_forward_backward(Xv, wv, bias, b.t, loss, lo, c.grad_scale, prob=b.prob,
                                  dz=b.dz, loss_out=b.loss)
        _eq(b.prob, r["prob"], f"prob lo={lo}")
        _eq(b.dz, r["dz"], f"dz lo={lo}")
        if _loss_is_exact(c, lo):
            _eq(b.loss, r["loss"], f"loss lo={lo}")
        assert b.pads_ok() and _untouched(b.dX, b.dw)


@pytest.mark.parametrize("loss", ["mse", "bce"])
def test_head_forward_backward_grid_wrap(ops, loss):
    """M = 16388 rows on the capped 4096-workgroup grid: the wave-stride loop wraps."""
    M, K = 16388, 2
    c = _hcase(M, K, loss, "anchor", 1.0)
    r = _href(M, K, loss, "anchor", 0.0, 1.0)
    b = HeadBuffers(c)
    ops.head_forward_backward(b.X[:, :1], b.w[:1], _vec(c.w[1:], NAN), b.t, loss, 0.0, 1.0,
                              prob=b.prob, dz=b.dz, loss_out=b.loss)
    _eq(b.prob, r["prob"], "prob")
    _eq(b.dz, r["dz"], "dz")
    if loss == "mse":
        _eq(b.loss, r["loss"], "loss")
    assert b.pads_ok()


def test_head_refusals_write_nothing(ops, lib):
    """K = 2049 is refused (UNSUPPORTED) and a workspace one byte short is refused
    (WORKSPACE); neither writes anything."""
    g = torch.Generator().manual_seed(1)
    M, K = 5, 2049
    X = padded(int_matrix((M, K), -1, 3, g, nonzero=False, device=dev), 2, 3, NAN)
    w, t = _vec(int_matrix((K,), -2, 2, g)), _vec(torch.zeros(M))
    outs = dict(prob=_vec(M), dz=_vec(M), loss_out=_vec(1), dw=_vec(K),
                dX=padded(torch.full((M, K), SENTINEL, device=dev), 2, 3, SENTINEL))
    w0 = w.clone()
    for defer in (False, True):
        with pytest.raises(lib.DLRMHipError) as e:
            ops.head_step(X, w, t, "mse", 0.0, 1.0, defer=defer, **outs)
        assert e.value.code == 3
    with pytest.raises(lib.DLRMHipError) as e:
        ops.head_predict(X, w, 0.0, prob=outs["prob"])
    assert e.value.code == 3
    assert _untouched(*outs.values()) and torch.equal(w, w0)

    c = _hcase(37, 65, "mse")
    b = HeadBuffers(c)
    need = lib.query("dlrm_head_step_workspace_size", 37, 65)
    for defer in (False, True):
        with pytest.raises(lib.DLRMHipError) as e:
            ops.head_step(b.X, b.w, b.t, "mse", 0.0, 1.0, defer=defer,
                          workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev), **b.kw())
        assert e.value.code == 4
    need = lib.query("dlrm_head_workspace_size", 37)
    with pytest.raises(lib.DLRMHipError) as e:
        ops.head_forward_backward(b.X, b.w, None, b.t, "mse", prob=b.prob, dz=b.dz,
                                  loss_out=b.loss,
                                  workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    assert e.value.code == 4
    assert _untouched(b.prob, b.dz, b.loss, b.dw, b.dX)
    _eq(b.w, c.w, "w")


# ------------------------------------------------ 2. the head on general logits ----
def _sweep_case():
    """One row per half-integer z in [-100, 24]: X = [z - 1, 1], w = [1, 1] (exact)."""
    z = H.SWEEP_Z
    X = torch.from_numpy(np.stack([z - 1.0, np.ones_like(z)], 1)).float()
    return z, padded(X.to(dev), 2, 3, NAN), _vec(torch.ones(2), NAN)


def _prob_bound_ok(got, z, lo=0.0):
    """(max ulp error over the rows whose sigmoid is a normal float32, max absolute error
    over the others).  A clamp only moves both values toward each other."""
    ref = H.sigmoid64(z)
    if lo:
        ref = np.clip(ref, f64(f32(lo)), f64(f32(1) - f32(lo)))
    normal = ref >= 2.0 ** -126
    got = np.asarray(got, dtype=f64)
    ulps = H.ulp_error(got[normal], ref[normal]).max(initial=0.0)
    absd = np.abs(got[~normal] - ref[~normal]).max(initial=0.0)
    return ulps, absd


def test_prob_sweep(ops):
    """prob against the fp64 sigmoid over every half-integer z in [-100, 24], through the
    three head kernels and dlrm_sigmoid_forward: at most PROB_ULP_MEASURED + 1 ulp wherever
    the sigmoid is a normal float32 (z >= -87).  Below, the true value is a denormal;
    expf(-z) overflows from z = -89 on and prob is exactly 0 there: an absolute error under
    2^-126, counted as such and not in ulps of a denormal."""
    z, X, w = _sweep_case()
    M = len(z)
    t = _vec(torch.zeros(M))
    got = {}
    p = _vec(M)
    ops.head_step(X, w, t, "mse", 0.0, 1.0, prob=p)
    got["head_step"] = p.cpu().numpy()
    p = _vec(M)
    ops.head_predict(X, w, 0.0, prob=p)
    got["head_predict"] = p.cpu().numpy()
    p = _vec(M)
    ops.head_forward_backward(X[:, :1], w[:1], w[1:], t, "mse", prob=p)
    got["head_forward_backward"] = p.cpu().numpy()
    zs = _vec(torch.from_numpy(z).float(), NAN)
    y = _vec(M)
    ops.sigmoid_forward(zs, out=y)
    assert _vec_intact(y)
    got["sigmoid_forward"] = y.cpu().numpy()
    worst = {k: _prob_bound_ok(v, z) for k, v in got.items()}
    print("prob ulp / abs error by entry point:", worst)
    for k, v in got.items():
        assert not np.isnan(v).any(), k
        assert worst[k][0] <= PROB_ULP_MEASURED + 1, (k, worst[k])
        assert worst[k][1] <= 2.0 ** -126, (k, worst[k])
        for za, pa in H.ANCHOR_P.items():  # the three anchors exactly
            assert v[z == za][0] == f32(pa), (k, za)
        assert (v[z <= -89] == 0).all() and (v[z >= 20] == 1).all(), k


def test_logf_sweep(ops):
    """The BCE row loss at M = 1 is -logf(pc) (target 1) or -logf(1 - pc) (target 0) with no
    other rounding: its ulp error against the fp64 log of the same float32 argument, over the
    sweep, is at most LOGF_ULP_MEASURED + 1; the -100 guard holds where the argument is 0."""
    z = H.SWEEP_Z
    X = torch.from_numpy(np.stack([z - 1.0, np.ones_like(z)], 1)).float().to(dev)
    w = torch.ones(2, device=dev)
    worst = 0.0
    for tv in (1.0, 0.0):
        t = torch.full((1,), tv, device=dev)
        prob, loss = torch.empty(len(z), device=dev), torch.empty(len(z), device=dev)
        for i in range(len(z)):
            ops.head_step(X[i:i + 1], w, t, "bce", 0.0, 1.0, prob=prob[i:i + 1],
                          loss_out=loss[i:i + 1])
        pc, ls = prob.cpu().numpy(), loss.cpu().numpy()
        ref = H.row_loss64(pc, np.full(len(z), tv), "bce")
        assert not np.isnan(ls).any()
        sat = ref == 100.0
        assert (ls[sat] == 100.0).all() and sat.any()
        zero = ref == 0.0
        assert (ls[zero] == 0.0).all()
        rest = ~(sat | zero)
        worst = max(worst, H.ulp_error(ls[rest], ref[rest]).max())
    print("logf ulp error over the sweep:", worst)
    assert worst <= LOGF_ULP_MEASURED + 1


@pytest.mark.parametrize("lo", [0.0, 0.2])
@pytest.mark.parametrize("loss", ["mse", "bce"])
@pytest.mark.parametrize("M,K", GENERAL_SHAPES)
def test_head_step_general(ops, M, K, loss, lo):
    """Integer logits in [-16, 16]: prob within the measured ulp bound of the fp64 sigmoid;
    dz bit for bit the float32 restatement of head_row_math at the kernel's own prob
    (where prob is p: every row at clamp_lo = 0, the rows inside the clamp otherwise; 0
    outside); dX = fl(dz w) masked, bitwise; dw within the project's
    accumulation bound of the fp64 sum over the kernel's dz; loss_out within
    (M + c) 2^-24 mean|l| of the fp64 mean of the row loss at the kernel's prob."""
    c = _hcase(M, K, loss, "general")
    b = HeadBuffers(c)
    ops.head_step(b.X, b.w, b.t, loss, lo, c.grad_scale, relu_mask=True, **b.kw())
    assert b.pads_ok()
    prob, dz = b.prob.cpu().numpy(), b.dz.cpu().numpy()
    assert not (np.isnan(prob).any() or np.isnan(dz).any())
    ulps, absd = _prob_bound_ok(prob, c.z, lo)
    print(f"prob ulp {ulps}")
    assert ulps <= PROB_ULP_MEASURED + 1 and absd == 0.0
    _, dz_ref, _ = H.head_row_ref(prob, c.t.numpy(), loss, 0.0, c.grad_scale, M)
    if lo:  # integer logits: |z| >= 2 is far outside [0.2, 0.8], |z| <= 1 far inside, where
        lo32, hi32 = f32(lo), f32(1) - f32(lo)  # prob is p again
        assert (prob >= lo32).all() and (prob <= hi32).all()
        out = np.abs(c.z) >= 2
        assert out.any() and set(np.unique(prob[out])) <= {lo32, hi32}
        dz_ref[out] = 0
    _eq(b.dz, dz_ref, "dz from the kernel's prob")
    X, w = c.X.numpy(), c.w.numpy()
    dX_ref = np.where(X > 0, (dz[:, None].astype(f64) * w[None, :].astype(f64)).astype(f32), 0)
    _eq(b.dX, dX_ref.astype(f32), "dX = fl(dz w), masked")
    dw64 = (dz[:, None].astype(f64) * X.astype(f64)).sum(0)
    absprod = (np.abs(dz)[:, None].astype(f64) * np.abs(X).astype(f64)).sum(0)
    ok, worst = gemm_close(b.dw.cpu().numpy(), dw64, absprod, M)
    assert ok, f"dw: worst |err| / tol = {worst}"
    rl = H.row_loss64(prob, c.t.numpy(), loss)
    err = abs(float(b.loss.cpu()[0]) - rl.mean())
    bound = (M + LOSS_C) * 2.0 ** -24 * np.abs(rl).mean()
    print(f"loss err {err:.3e} bound {bound:.3e}")
    assert err <= bound


# ------------------------------------- 3. column sums and elementwise kernels ----
@pytest.mark.parametrize("N", H.COLSUM_NS)
@pytest.mark.parametrize("M", H.COLSUM_MS)
def test_colsum_exact(ops, M, N):
    """dlrm_colsum_f32 on integers with dyadic scale / alpha: plain, scaled + alpha +
    accumulate onto integers, out + fused SGD (float lr), SGD only with a device lr."""
    g = torch.Generator().manual_seed(M + N)
    out0, p0 = int_matrix((N,), -8, 8, g), int_matrix((N,), -8, 8, g)
    lr = 2.0 ** -3
    variants = [dict(scaled=False, alpha=1.0, acc=False, sgd=None, out=True),
                dict(scaled=True, alpha=0.5, acc=True, sgd=None, out=True),
                dict(scaled=True, alpha=-2.0, acc=False, sgd=lr, out=True),
                dict(scaled=False, alpha=-2.0, acc=True, sgd=lr, out=True),
                dict(scaled=True, alpha=1.0, acc=False, sgd="dev", out=False)]
    for v in variants:
        Y, scale = H.colsum_case(M, N, v["scaled"])
        ref_out, ref_p = H.ref_colsum(Y, scale, v["alpha"], out0 if v["acc"] else None,
                                      p0 if v["sgd"] else None, lr)
        Yd = padded(Y.to(dev), 2, 3, NAN)
        assert Yd.stride(0) == N + 3
        sd = _vec(scale, NAN) if scale is not None else None
        out = _vec(out0) if v["acc"] else _vec(N)
        par = _vec(p0)
        ops.colsum(Yd, scale=sd, alpha=v["alpha"], out=out if v["out"] else None,
                   accumulate=v["acc"], sgd_param=par if v["sgd"] else None,
                   lr=torch.tensor([lr], device=dev) if v["sgd"] == "dev" else (v["sgd"] or 0.0))
        if v["out"]:
            _eq(out, ref_out, f"out {v}")
        else:
            assert _untouched(out)
        _eq(par, ref_p if v["sgd"] else p0, f"sgd_param {v}")
        assert _vec_intact(out) and _vec_intact(par)


def test_colsum_refuses_a_short_workspace(ops, lib):
    Y, _ = H.colsum_case(65, 300, False)
    out, par = _vec(300), _vec(300)
    need = lib.query("dlrm_colsum_workspace_size", 65, 300)
    with pytest.raises(lib.DLRMHipError) as e:
        ops.colsum(Y.to(dev), out=out, sgd_param=par, lr=0.5,
                   workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    assert e.value.code == 4 and _untouched(out, par)


@functools.lru_cache(maxsize=None)
def _sgd_case(n):
    return H.sgd_case(n)


@pytest.mark.parametrize("dev_lr", [False, True])
@pytest.mark.parametrize("n", H.OPT_NS)
def test_sgd_update_exact(ops, n, dev_lr):
    p0, g0 = _sgd_case(n)
    p, g = _vec(p0), _vec(g0, NAN)
    ops.sgd_update(p, g, torch.tensor([0.25], device=dev) if dev_lr else 0.25)
    _eq(p, H.ref_sgd(p0, g0, 0.25), "param")
    _eq(g, g0, "grad")
    assert _vec_intact(p) and _vec_intact(g, NAN)


@functools.lru_cache(maxsize=None)
def _adagrad_case(n):
    return H.adagrad_case(n)


@pytest.mark.parametrize("gs,dev_clr", [(1.0, False), (1.0, True), (2.0 ** -3, False),
                                        (1.0 / 3.0, False), (1.0 / 3.0, True)])
@pytest.mark.parametrize("n", H.OPT_NS)
def test_adagrad_update_exact(ops, n, gs, dev_clr):
    """g^2 + state_sum = r^2 (r an integer), eps = 2^-10: sqrtf and the add are exact, the
    division and the two fmas round once each; grad_scale = 1/3 is the one inexact multiply."""
    p0, g0, s0 = _adagrad_case(n)
    clr, eps = 2.0 ** -3, 2.0 ** -10
    p_ref, s_ref = H.ref_adagrad_dense(p0, g0, s0, clr, eps, gs)
    p, g, s = _vec(p0), _vec(g0, NAN), _vec(s0)
    ops.adagrad_update(p, g, s, torch.tensor([clr], device=dev) if dev_clr else clr, eps,
                       grad_scale=gs)
    _eq(s, s_ref, "state_sum")
    _eq(p, p_ref, "param")
    _eq(g, g0, "grad")
    assert _vec_intact(p) and _vec_intact(s) and _vec_intact(g, NAN)


@pytest.mark.parametrize("n", [1, 257, 4194304 + 3])
def test_scale_exact(ops, n):
    g = torch.Generator().manual_seed(n)
    x0 = full_mantissa((n,), g)
    a = float(full_mantissa((1,), g)[0])
    x = _vec(x0)
    ops.scale_(x, a)
    _eq(x, (x0.double() * a).float(), "x")
    assert _vec_intact(x)


def _signed_full_mantissa(shape, g):
    v = full_mantissa(shape, g)
    return torch.where(torch.randint(0, 2, shape, generator=g) == 0, v, -v)


@pytest.mark.parametrize("M,K", [(5, 51), (16, 16), (257, 1), (3, 100)])
def test_outer_drelu_exact(ops, M, K):
    """dX = fl(dz w) with full-mantissa operands (one rounding per output), masked by X > 0
    with -0.0, 0 and negatives in X, and unmasked with X = None; M K = 255, 256, 257, 300."""
    g = torch.Generator().manual_seed(M * K)
    dz, w = _signed_full_mantissa((M,), g), _signed_full_mantissa((K,), g)
    X = torch.tensor([-0.0, 0.0, -1.5, 2.0, 1e-30])[torch.randint(0, 5, (M, K), generator=g)]
    ref = (dz.double()[:, None] * w.double()[None, :]).float()
    dzd, wd, Xd = _vec(dz, NAN), _vec(w, NAN), padded(X.to(dev), 2, 3, NAN)
    for mask in (True, False):
        out = padded(torch.full((M, K), SENTINEL, device=dev), 2, 5, SENTINEL)
        ops.outer_drelu(dzd, wd, Xd if mask else None, mask, out=out)
        _eq(out, torch.where(X > 0, ref, torch.zeros(())) if mask else ref, f"mask={mask}")
        assert pads_intact(out)


@pytest.mark.parametrize("M,K", [(1, 1), (5, 51), (3, 100), (300, 7), (4099, 1024)])
def test_relu_backward_exact(ops, M, K):
    """Row-strided dy, y and dx; NaN in dy is dropped where y <= 0 (or y is NaN) and carried
    bit for bit where y > 0.  4099 x 1024 elements cross the grid-stride cap."""
    g = torch.Generator().manual_seed(M + K)
    dy = _signed_full_mantissa((M, K), g)
    dy[torch.randint(0, 4, (M, K), generator=g) == 0] = NAN
    y = torch.tensor([-0.0, 0.0, -1.5, 2.0, 1e-30, NAN])[torch.randint(0, 6, (M, K), generator=g)]
    ref = torch.where(y > 0, dy, torch.zeros(()))
    out = padded(torch.full((M, K), SENTINEL, device=dev), 2, 5, SENTINEL)
    ops.relu_backward(padded(dy.to(dev), 2, 3, NAN), padded(y.to(dev), 2, 1, NAN), out=out)
    _bits_eq(out, ref, "dx")
    assert pads_intact(out)


@pytest.mark.parametrize("n", [1, 257, 4194304 + 3])
def test_sigmoid_backward_exact(ops, n):
    g = torch.Generator().manual_seed(n)
    dy, y = _signed_full_mantissa((n,), g), full_mantissa((n,), g) * 0.5
    ref = (dy.numpy() * (f32(1) - y.numpy())) * y.numpy()
    assert ref.dtype == f32
    _eq(ops.sigmoid_backward(_vec(dy, NAN), _vec(y, NAN)), ref, "dx")


@pytest.mark.parametrize("n", [1, 5, 67])
@pytest.mark.parametrize("D", [4, 6, 8, 64])
@pytest.mark.parametrize("op", ["mult", "add", "concat"])
def test_qr_combine_exact(ops, op, D, n):
    g = torch.Generator().manual_seed(D + n)
    eq, er = _signed_full_mantissa((n, D), g), _signed_full_mantissa((n, D), g)
    go = _signed_full_mantissa((n, 2 * D if op == "concat" else D), g)
    if op == "mult":
        ref = (eq.double() * er.double()).float()
        rq, rr = (go.double() * er.double()).float(), (go.double() * eq.double()).float()
    elif op == "add":
        ref, rq, rr = eq + er, go, go
    else:
        ref, rq, rr = torch.cat((eq, er), 1), go[:, :D], go[:, D:]
    eqd, erd = _vec(eq.reshape(-1), NAN).view(n, D), _vec(er.reshape(-1), NAN).view(n, D)
    _eq(ops.qr_combine_forward(op, eqd, erd), ref, "forward")
    gq, gr = ops.qr_combine_backward(op, eqd, erd, _vec(go.reshape(-1), NAN).view(n, -1))
    _eq(gq, rq, "grad eq")
    _eq(gr, rr, "grad er")


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("D", [4, 8, 64])
@pytest.mark.parametrize("op", ["mult", "add"])
def test_qr_pool_combine_exact(ops, op, D, B):
    """Three logical tables over five pooled ones: (q, r) pairs and a pass-through (pr < 0);
    batch strides wider than the rows; one rounding per output."""
    T, Tp = 3, 5
    pq = torch.tensor([3, 2, 0], dtype=torch.int32, device=dev)
    pr = torch.tensor([1, -1, 4], dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(D + B)
    P = _signed_full_mantissa((B, Tp, D), g)
    dE = _signed_full_mantissa((B, T, D), g)
    E_ref, dP_ref = torch.empty(B, T, D), torch.empty(B, Tp, D)
    for t, (q, r) in enumerate(zip(pq.tolist(), pr.tolist())):
        if r < 0:
            E_ref[:, t], dP_ref[:, q] = P[:, q], dE[:, t]
        elif op == "mult":
            E_ref[:, t] = (P[:, q].double() * P[:, r].double()).float()
            dP_ref[:, q] = (dE[:, t].double() * P[:, r].double()).float()
            dP_ref[:, r] = (dE[:, t].double() * P[:, q].double()).float()
        else:
            E_ref[:, t] = P[:, q] + P[:, r]
            dP_ref[:, q] = dP_ref[:, r] = dE[:, t]
    Pd = padded(P.reshape(B, Tp * D).to(dev), 2, 4, NAN)
    dEd = padded(dE.reshape(B, T * D).to(dev), 2, 8, NAN)
    E = padded(torch.full((B, T * D), SENTINEL, device=dev), 2, 8, SENTINEL)
    dP = padded(torch.full((B, Tp * D), SENTINEL, device=dev), 2, 4, SENTINEL)
    ops.qr_pool_combine_forward(op, T, B, D, pq, pr, Pd, E)
    _eq(E, E_ref.reshape(B, T * D), "E")
    ops.qr_pool_combine_backward(op, T, B, D, pq, pr, Pd, dEd, dP)
    _eq(dP, dP_ref.reshape(B, Tp * D), "dP")
    assert pads_intact(E) and pads_intact(dP)


def test_qr_pool_combine_refuses_d6(ops, lib):
    T, B, D = 1, 2, 6
    pq = torch.zeros(1, dtype=torch.int32, device=dev)
    pr = torch.ones(1, dtype=torch.int32, device=dev)
    P = torch.ones(B, 2 * D + 4, device=dev)
    E = padded(torch.full((B, D), SENTINEL, device=dev), 2, 2, SENTINEL)
    dP = padded(torch.full((B, 2 * D), SENTINEL, device=dev), 2, 4, SENTINEL)
    for op in ("mult", "add"):
        with pytest.raises(lib.DLRMHipError) as e:
            ops.qr_pool_combine_forward(op, T, B, D, pq, pr, P, E)
        assert e.value.code == 1
        with pytest.raises(lib.DLRMHipError) as e:
            ops.qr_pool_combine_backward(op, T, B, D, pq, pr, P, E, dP)
        assert e.value.code == 1
    assert _untouched(E, dP)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("c", [4, 1000, 60000])
def test_qr_split_indices_exact(ops, c, dtype):
    """Quotient by float32 true division (truncated) and integer remainder, as the oracle's
    QREmbeddingBagOracle.split: at 2^24 +- 1, 2^31 - 1 and multiples of c +- 1 above 2^24 the
    float32 quotient differs from integer division."""
    import oracle as O
    vals = H.qr_split_values(c)
    idx = torch.tensor(vals, dtype=dtype)
    q_ref, r_ref = O.QREmbeddingBagOracle.split(idx, c)
    assert not torch.equal(q_ref, torch.tensor([v // c for v in vals]))
    q, r = ops.qr_split_indices(idx.to(dev), c)
    assert torch.equal(q.cpu(), q_ref) and torch.equal(r.cpu(), r_ref)


@pytest.mark.parametrize("out_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("T", [1, 64])
def test_csr_from_tables_exact(ops, T, out_dtype):
    B = 5
    g = torch.Generator().manual_seed(T)
    lens = torch.randint(0, 3, (T, B), generator=g)  # empty bags included
    lens[0, 0] = lens[T - 1, B - 1] = 0
    offs = [torch.cat((torch.zeros(1, dtype=torch.int64), lens[t].cumsum(0)[:-1]))
            for t in range(T)]
    nnz = [int(lens[t].sum()) for t in range(T)]
    out = ops.csr_from_tables([o.to(dev) for o in offs], nnz, B, out_dtype)
    assert out.dtype == out_dtype
    assert torch.equal(out.cpu().long(), H.ref_csr(offs, nnz))


def test_csr_from_tables_refusals(ops, lib):
    o = torch.zeros(2, dtype=torch.int64, device=dev)
    with pytest.raises(lib.DLRMHipError) as e:
        ops.csr_from_tables([o] * 65, [0] * 65, 2)
    assert e.value.code == 1
    with pytest.raises(lib.DLRMHipError) as e:
        ops.csr_from_tables([o, o], [2 ** 30, 2 ** 30], 2, torch.int32)
    assert e.value.code == 3
    out = ops.csr_from_tables([o, o], [2 ** 30, 2 ** 30], 2, torch.int64)
    assert out.cpu().tolist() == [0, 0, 2 ** 30, 2 ** 30, 2 ** 31]


# ---------------------------------------------------- 4. the fill streams, pinned ----
@functools.lru_cache(maxsize=None)
def _fill_ref(n, lo, hi, seed):
    return H.ref_uniform_fill(n, lo, hi, seed)


@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-0.5, 0.5)])
@pytest.mark.parametrize("seed", H.FILL_SEEDS)
@pytest.mark.parametrize("n", H.FILL_NS)
def test_uniform_fill_stream(ops, n, seed, lo, hi):
    """dlrm_uniform_fill equals the numpy splitmix64 reference bit for bit (the stream
    init_random depends on); n = 4194304 + 3 crosses the grid-stride cap."""
    out = _vec(n)
    ops.uniform_fill_(out, lo, hi, seed)
    _eq(out, _fill_ref(n, lo, hi, seed), "stream")
    assert _vec_intact(out)


@pytest.mark.parametrize("seed", H.FILL_SEEDS)
def test_uniform_fill_at_chunks(ops, seed):
    """Three uneven chunks through dlrm_uniform_fill_at equal one whole dlrm_uniform_fill
    (and the reference)."""
    n, cuts = 70001, [0, 1000, 33337, 70001]
    whole, parts = _vec(n), _vec(n)
    ops.uniform_fill_(whole, -0.5, 0.5, seed)
    for a, b in zip(cuts[:-1], cuts[1:]):
        ops.uniform_fill_at_(parts[a:b], -0.5, 0.5, seed, a)
    _eq(parts, whole.cpu(), "chunks vs whole")
    _eq(whole, _fill_ref(n, -0.5, 0.5, seed), "whole vs reference")
    assert _vec_intact(whole) and _vec_intact(parts)


@pytest.mark.parametrize("n", [257, 4194304 + 3])
@pytest.mark.parametrize("dtype,hi", [(torch.int32, 1), (torch.int32, 1000), (torch.int32, 2 ** 31),
                                      (torch.int64, 1), (torch.int64, 1000),
                                      (torch.int64, 2 ** 31), (torch.int64, 2 ** 40)])
def test_uniform_int_fill_stream(ops, dtype, hi, n):
    """dlrm_uniform_int_fill equals (x * hi) >> 64 of the same stream: in Python integers at
    n = 257, by the limb product proved equal to them (test_exact_head_cpu.py) above the
    grid-stride cap."""
    seed = H.FILL_SEEDS[hi % 2]
    out = _vec(torch.zeros(n, dtype=dtype), fill=-7)
    ops.uniform_int_fill_(out, hi, seed)
    ref = H.ref_uniform_int(n, hi, seed, exact_python=n <= 257)
    assert torch.equal(out.cpu().long(), ref)
    assert _vec_intact(out, -7)
    assert hi == 1 or int(out.max()) > 0
