"""Exact-arithmetic tests of the MFMA users (fp32 GEMM, bottom-MLP chain, dot interaction).

The kernels get inputs for which fp32 arithmetic is exact (tests/exact_inputs.py), so every
result must equal the fp64 reference BIT FOR BIT, whatever the tile, split, layout, epilogue
or summation order: there is no tolerance anywhere in this file.  Operands sit in NaN-padded
buffers (a pad that reaches a sum poisons it), outputs in sentinel-padded ones with two guard
rows (a write outside [M, N] is seen bitwise)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from exact_inputs import (SENTINEL, exact_bound_ok, full_mantissa, int_matrix, one_hot_rows,
                          padded, pads_intact)

pytestmark = pytest.mark.gpu

dev = "cuda:0"
NAN = float("nan")
GEMM_CFGS = [64064, 128064, 64128, 64032, 32064, 32032]  # as test_gpu_kernels.GEMM_CFGS
LAYOUTS = [(0, 1), (0, 0), (1, 0), (1, 1)]  # (trans_a, trans_b) of plan layouts 0, 1, 2, 3
ALPHAS = (1.0, 0.5, -2.0)
TICKET_BYTES = 4 * 16384  # the workspace's fixed ticket head
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from dlrm_hip import ops as _ops
    return _ops


def _gen(seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _workspace():
    return torch.zeros(64 << 20, dtype=torch.uint8, device=dev)


def _tickets_zero(ws):
    return int(ws[:TICKET_BYTES].view(torch.int32).abs().sum()) == 0


def _all_epilogues(ops):
    return [ops.EPI_STORE, ops.EPI_BIAS, ops.EPI_BIAS_RELU, ops.EPI_DRELU, ops.EPI_SGD,
            ops.EPI_ACCUM, ops.EPI_RELU]


def _nan_vector(v):
    buf = torch.full((v.numel() + 4,), NAN, device=v.device)
    buf[:v.numel()] = v
    return buf[:v.numel()]


class IntCase:
    """One integer GEMM problem: NaN-padded A, B, aux and bias, the old C, and the fp64
    accumulator op(A) @ op(B) with the row sums of op(A); built once per (shape, layout) and
    shared (the kernels only read it)."""

    def __init__(self, M, N, K, ta, tb, seed=0):
        g = _gen(1000 * seed + 17 * M + 5 * N + K + 2 * ta + tb)
        self.M, self.N, self.K, self.ta, self.tb = M, N, K, ta, tb
        self.A = padded(int_matrix((K, M) if ta else (M, K), -4, 4, g), 2, 4, NAN)
        self.B = padded(int_matrix((N, K) if tb else (K, N), -4, 4, g), 2, 4, NAN)
        self.bias = _nan_vector(int_matrix((N,), -8, 8, g, nonzero=False))
        self.aux = padded(int_matrix((M, N), -2, 2, g, nonzero=False), 2, 4, NAN)
        self.C0 = int_matrix((M, N + 4), -64, 64, g, nonzero=False)  # + a ones_col layer's pad
        opA = self.A.double().t() if ta else self.A.double()
        opB = self.B.double().t() if tb else self.B.double()
        self.acc = opA @ opB
        self.rowsum = opA.sum(1)
        # |alpha| <= 2 and the half-integers of alpha = 0.5 (one more bit), + |bias| + |old C|
        self.exact = exact_bound_ok(2 * opA.abs(), opB.abs(), extra=8 + 64)

    def reference(self, ops, epi, alpha, ones_col):
        """fp64 epi(alpha * acc) over the old C (width N, or N + 4 with column N the row
        sums), cast to fp32."""
        old = self.C0.double() if ones_col else self.C0[:, :self.N].double()
        v = alpha * self.acc
        if ones_col:
            v = torch.cat([v, alpha * self.rowsum[:, None]], 1)
            assert epi in (ops.EPI_STORE, ops.EPI_SGD, ops.EPI_ACCUM)  # no bias / aux column
        w = v.shape[1]
        r = {ops.EPI_STORE: lambda: v,
             ops.EPI_BIAS: lambda: v + self.bias.double(),
             ops.EPI_BIAS_RELU: lambda: torch.relu(v + self.bias.double()),
             ops.EPI_DRELU: lambda: torch.where(self.aux.double() > 0, v, torch.zeros_like(v)),
             ops.EPI_SGD: lambda: old[:, :w] - v,
             ops.EPI_ACCUM: lambda: old[:, :w] + v,
             ops.EPI_RELU: lambda: torch.relu(v)}[epi]()
        ref = old.clone()
        ref[:, :w] = r
        assert torch.equal(ref.float().double(), ref)  # the reference itself is fp32-exact
        return ref.float()

    def output(self, ones_col):
        """A fresh C: the old values inside a sentinel buffer with 4 pad columns, 2 guard rows."""
        return padded(self.C0 if ones_col else self.C0[:, :self.N], 2, 4, SENTINEL)

    def problem(self, ops, C, epi, alpha, ones_col, **kw):
        return ops.gemm_problem(self.A, self.B, bool(self.ta), bool(self.tb), C=C, alpha=alpha,
                                epilogue=epi, bias=self.bias, aux=self.aux,
                                ones_col=self.N if ones_col else -1, **kw)[0]

    def run_and_check(self, ops, ws, epi, alpha, ones_col=False, what=()):
        assert self.exact
        C = self.output(ones_col)
        ops.gemm_group([self.problem(ops, C, epi, alpha, ones_col)], ws)
        self.check(ops, C, epi, alpha, ones_col, what)

    def check(self, ops, C, epi, alpha, ones_col, what=()):
        ref = self.reference(ops, epi, alpha, ones_col)
        tag = (self.M, self.N, self.K, self.ta, self.tb, epi, alpha, ones_col) + tuple(what)
        assert torch.equal(C, ref), (tag, _first_diff(C, ref))
        assert pads_intact(C), tag


def _first_diff(C, ref):
    bad = (C != ref) | torch.isnan(C)
    i = bad.nonzero()[0].tolist()
    return f"{int(bad.sum())} differ, first at {i}: got {C[tuple(i)].item()!r} " \
           f"ref {ref[tuple(i)].item()!r}"


@functools.lru_cache(maxsize=None)
def _case(M, N, K, ta, tb, seed=0):
    return IntCase(M, N, K, ta, tb, seed)


# ------------------------------------------------------------- a. epilogue matrix --
@pytest.mark.parametrize("cfg", GEMM_CFGS)
def test_gemm_exact_epilogue_matrix(ops, cfg):
    """Every tile x split (1, 3) x layout x epilogue on shapes ragged in M and N against every
    tile, K % 32 != 0 (the K-tail masking) and K, M, N % 4 == 0 (all four layouts stay on the
    pipelined path): epi(alpha * A @ B) bitwise, pads and guard rows untouched."""
    ws = _workspace()
    n = 0
    for (M, N, K) in [(130, 72, 300), (36, 8, 1028)]:
        for ta, tb in LAYOUTS:
            c = _case(M, N, K, ta, tb)
            for split in (1, 3):
                for epi in _all_epilogues(ops):
                    alpha = ALPHAS[n % 3]
                    n += 1
                    with ops.tuning(gemm_tile=cfg, gemm_split=split):
                        c.run_and_check(ops, ws, epi, alpha, what=(cfg, split))
    assert _tickets_zero(ws)


# -------------------------------------------------------------------- b. precision --
def _one_hot_pair(ta, tb, swapped, M=128, N=96, K=512, seed=7):
    """(A, B, ref): one operand with a single full-mantissa nonzero per output row (or, with
    ``swapped``, per output column), the other dense full-mantissa; every C[m][n] is one
    correctly rounded product plus exact zeros."""
    g = _gen(seed + 2 * ta + tb + 4 * swapped)
    if swapped:
        opA, opB = full_mantissa((M, K), g), one_hot_rows(N, K, g).t()
    else:
        opA, opB = one_hot_rows(M, K, g), full_mantissa((K, N), g)
    ref = (opA.double() @ opB.double()).float()
    A = (opA.t() if ta else opA).contiguous()
    B = (opB.t() if tb else opB).contiguous()
    return A, B, ref


def _offset_by_one_float(t, pad_rows=0, pad_cols=0):
    """``t`` in a NaN buffer whose base pointer is one float off 16-byte alignment."""
    r, c = t.shape
    buf = torch.full(((r + pad_rows) * (c + pad_cols) + 4,), NAN, device=t.device)
    v = buf[1:1 + (r + pad_rows) * (c + pad_cols)].view(r + pad_rows, c + pad_cols)[:r, :c]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _run_one_hot(ops, ws, ta, tb, swapped, generic=False, what=()):
    A, B, ref = _one_hot_pair(ta, tb, swapped)
    if generic:
        A, B = _offset_by_one_float(A, 2, 4), padded(B, 2, 4, NAN)
    else:
        A, B = padded(A, 2, 4, NAN), padded(B, 2, 4, NAN)
    C = padded(torch.zeros_like(ref), 2, 4, SENTINEL)
    ops.gemm_group([ops.gemm_problem(A, B, bool(ta), bool(tb), C=C)[0]], ws)
    tag = (ta, tb, swapped, generic) + tuple(what)
    assert torch.equal(C, ref), (tag, _first_diff(C, ref))
    assert pads_intact(C), tag


@pytest.mark.parametrize("cfg", GEMM_CFGS + ["default", "generic"])
def test_gemm_exact_full_mantissa_products(ops, cfg):
    """One-hot x full-mantissa operands (either operand the one-hot one): every output is the
    fp64 product rounded once - any lost operand mantissa bit changes it.  Every tile, the
    forward and wgrad layouts, unsplit and split 4; the default plan; the generic kernel."""
    ws = _workspace()
    for swapped in (False, True):
        if cfg in ("default", "generic"):
            for ta, tb in LAYOUTS:
                _run_one_hot(ops, ws, ta, tb, swapped, generic=cfg == "generic")
            continue
        for ta, tb in [(0, 1), (1, 0)]:
            for split in (1, 4):
                with ops.tuning(gemm_tile=cfg, gemm_split=split):
                    _run_one_hot(ops, ws, ta, tb, swapped, what=(cfg, split))
    assert _tickets_zero(ws)


# ----------------------------------------------------------- c. the measured plans --
def _plan_entries():
    path = os.path.join(ROOT, "dlrm-yx_amd", "csrc", "gemm_plans.inc")
    with open(path) as f:
        text = f.read()
    pat = r"^\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\},"
    return [tuple(int(x) for x in m.groups()) for m in re.finditer(pat, text, re.M)]


def _normalized_splits(s, K):
    """gemm.hip make_plan: the split count a launch really runs for a requested one."""
    s = max(1, min(s, 32, -(-K // 32)))
    kchunk = max(32, -(-(-(-K // s)) // 32) * 32)
    return -(-K // kchunk)


PLAN_CHUNKS = 4


@pytest.mark.parametrize("chunk", range(PLAN_CHUNKS))
def test_gemm_exact_every_measured_plan(ops, chunk):
    """Each entry of gemm_plans.inc - the (shape, layout, tile, split) the product runs - on
    the default plan: the planner's split is the entry's (the entry was hit) and the integer
    product is exact; wgrad-layout entries once more as the trainer uses them (fused SGD
    with the bias row sums in column N of a [M, N + 4] weight)."""
    entries = _plan_entries()
    assert len(entries) >= 70, len(entries)
    ws = _workspace()
    for i, (M, N, K, layout, bm, bn, split) in enumerate(entries):
        if i % PLAN_CHUNKS != chunk:
            continue
        ta, tb = LAYOUTS[layout]
        c = IntCase(M, N, K, ta, tb, seed=1)
        assert c.exact
        C = c.output(False)
        pr = c.problem(ops, C, ops.EPI_STORE, ALPHAS[i % 3], False)
        assert ops.gemm_splits(pr) == _normalized_splits(split, K), (M, N, K, layout)
        assert ops.gemm_group_workspace_size([pr]) <= ws.numel()
        ops.gemm_group([pr], ws)
        c.check(ops, C, ops.EPI_STORE, ALPHAS[i % 3], False, what=("plan", bm, bn, split))
        if layout == 2:
            c.run_and_check(ops, ws, ops.EPI_SGD, ALPHAS[(i + 1) % 3], ones_col=True,
                            what=("plan", bm, bn, split))
    assert _tickets_zero(ws)


# ------------------------------------------------------- d. PARTIAL / REDUCE, sgd_job --
@pytest.mark.parametrize("ones", [False, True])
@pytest.mark.parametrize("requested", [0, 2, 5, 32])
def test_gemm_exact_partial_then_reduce(ops, ones, requested):
    """A PARTIAL problem leaves C alone; the REDUCE job of a later launch writes exactly the
    fp64 result (fused SGD, with and without the ones_col row sums), for the planner's split
    and for requested counts normalized by dlrm_gemm_f32_splits."""
    ws = _workspace()
    c = _case(72, 64, 1028, 1, 0)
    assert c.exact
    alpha = ALPHAS[(requested + ones) % 3]
    C = c.output(ones)
    full = c.problem(ops, C, ops.EPI_SGD, alpha, ones)
    s = ops.gemm_splits(full, partial=True, requested=requested)
    if requested:
        assert s == _normalized_splits(requested, c.K)
    assert 1 <= s <= 32 and ops.gemm_splits(full, partial=True, requested=s) == s
    part = torch.full((ops.gemm_partial_bytes(c.M, c.N, s) // 4,), NAN, device=dev)
    pp = c.problem(ops, C, ops.EPI_SGD, alpha, ones, partial=part, splits=s)
    ops.gemm_group([pp], ws)
    before = c.output(ones)
    assert torch.equal(C._base.view(torch.int32), before._base.view(torch.int32))  # untouched
    ops.gemm_group([ops.reduce_problem(pp)], ws)
    c.check(ops, C, ops.EPI_SGD, alpha, ones, what=("reduce", requested, s))
    assert _tickets_zero(ws)


@pytest.mark.parametrize("beside_gemm", [False, True])
def test_gemm_exact_sgd_job(ops, beside_gemm):
    """ops.sgd_job (a one-split REDUCE job: param -= lr * grad) alone in a launch and beside
    a GEMM problem: exactly p - lr * g on integers with lr = 0.5; nothing past the parameter
    is written; the GEMM beside it is exact too."""
    ws = _workspace()
    g = _gen(31)
    n = 4100
    buf = torch.full((n + 64,), SENTINEL, device=dev)
    p0 = int_matrix((n,), -64, 64, g, nonzero=False)
    grad = int_matrix((n,), -9, 9, g, nonzero=False)
    p = buf[:n]
    p.copy_(p0)
    job = ops.sgd_job(p, grad, 0.5)
    c = _case(130, 72, 300, 1, 0)
    if beside_gemm:
        C = c.output(False)
        ops.gemm_group([c.problem(ops, C, ops.EPI_ACCUM, -2.0, False), job], ws)
        c.check(ops, C, ops.EPI_ACCUM, -2.0, False, what=("beside sgd_job",))
    else:
        ops.gemm_group([job], ws)
    ref = (p0.double() - 0.5 * grad.double()).float()
    assert torch.equal(p, ref)
    assert bool((buf[n:] == SENTINEL).all())
    assert _tickets_zero(ws)


# --------------------------------------------------------------- e. grouped launches --
def _group_cases():
    """Six problems covering every body kind: layouts 0..3, layout 2 with the row sums
    (kind 4), and a K = 1028 dgrad that splits in-launch.  (case, epilogue, alpha, ones)"""
    import dlrm_hip.ops as o
    return [(_case(68, 40, 132, 0, 1), o.EPI_BIAS_RELU, 1.0, False),
            (_case(130, 72, 300, 0, 0), o.EPI_DRELU, 0.5, False),
            (_case(72, 64, 1028, 1, 0), o.EPI_SGD, -2.0, False),
            (_case(36, 8, 1028, 1, 1), o.EPI_STORE, 1.0, False),
            (_case(68, 40, 132, 1, 0), o.EPI_SGD, 0.5, True),
            (_case(36, 8, 1028, 0, 0), o.EPI_ACCUM, -2.0, False)]


def _run_group(ops, ws, cases, what, **kw):
    outs, probs = [], []
    for c, epi, alpha, ones in cases:
        assert c.exact
        C = c.output(ones)
        outs.append(C)
        probs.append(c.problem(ops, C, epi, alpha, ones))
    ops.gemm_group(probs, ws, dev, **kw)
    for C, (c, epi, alpha, ones) in zip(outs, cases):
        c.check(ops, C, epi, alpha, ones, what=what)


def test_gemm_exact_grouped_launches(ops):
    """Grouped launches against fp64, exactly: six problems of every body kind in one launch
    (the all-kinds instantiation), each compiled kind pair (dgrad + wgrad with row sums,
    dgrad + wgrad, wgrad + wgrad with row sums), a group whose plans disagree (a 32x32 table
    entry beside heuristic 64x32 problems: the launch falls back to 64x32), and the six
    problems once more beside a deferred head role (the role kernel's retile)."""
    ws = _workspace()
    six = _group_cases()
    _run_group(ops, ws, six, ("all kinds",))
    dgrad, wgrad, wgrad_rs = six[1], six[2], six[4]
    for pair in ((dgrad, wgrad_rs), (dgrad, wgrad), (wgrad, wgrad_rs)):
        _run_group(ops, ws, list(pair), ("pair",))
    table = (_case(128, 16, 68, 0, 1), ops.EPI_RELU, 1.0, False)  # gemm_plans.inc: 32x32
    one = table[0].problem(ops, table[0].output(False), ops.EPI_RELU, 1.0, False)
    assert ops.gemm_splits(one) == 1
    _run_group(ops, ws, [table, dgrad, wgrad], ("plans disagree",))
    X = torch.rand(64, 20, device=dev)
    role = ops.head_step(X, torch.rand(20, device=dev), torch.rand(64, device=dev), "mse",
                         defer=True, lr=0.1)
    _run_group(ops, ws, six, ("role",), role=role, phase=4)
    assert _tickets_zero(ws)


# ------------------------------------------- f. generic kernel and degenerate sizes --
def test_gemm_exact_generic_kernel(ops):
    """The element-guarded fallback (K % 4 != 0, odd lda / ldb; and an aligned shape whose A
    is one float off 16-byte alignment): every layout x epilogue exact, and the fused-SGD
    ones_col row sums (the fallback's row-sum kernel)."""
    ws = _workspace()
    n = 0
    for (M, N, K) in [(33, 129, 67), (2, 4, 10)]:
        for ta, tb in LAYOUTS:
            c = _case(M, N, K, ta, tb)
            assert K % 4 != 0  # never the pipelined path
            for epi in _all_epilogues(ops):
                c.run_and_check(ops, ws, epi, ALPHAS[n % 3], what=("generic",))
                n += 1
            c.run_and_check(ops, ws, ops.EPI_SGD, ALPHAS[n % 3], ones_col=True,
                            what=("generic",))
    for ta, tb in LAYOUTS:  # aligned but for A's base pointer
        c = IntCase(36, 8, 68, ta, tb, seed=2)
        c.A = _offset_by_one_float(c.A, 2, 4)
        for epi in (ops.EPI_BIAS, ops.EPI_SGD):
            c.run_and_check(ops, ws, epi, ALPHAS[n % 3], ones_col=epi == ops.EPI_SGD,
                            what=("offset",))
            n += 1
    assert _tickets_zero(ws)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_gemm_k_zero_is_the_epilogue_of_zero(ops, ta, tb):
    """K == 0 (routed to the generic kernel): STORE writes zeros, BIAS the bias, SGD and
    ACCUM leave C as it was, and ones_col writes epi(0); pads and guard rows untouched."""
    ws = _workspace()
    c = IntCase(37, 20, 0, ta, tb, seed=3)
    assert c.A.shape == ((0, 37) if ta else (37, 0)) and float(c.acc.abs().sum()) == 0
    for epi in _all_epilogues(ops):
        c.run_and_check(ops, ws, epi, -2.0, what=("K0",))
    for epi in (ops.EPI_STORE, ops.EPI_SGD, ops.EPI_ACCUM):
        c.run_and_check(ops, ws, epi, 0.5, ones_col=True, what=("K0",))
    ref = c.reference(ops, ops.EPI_STORE, 1.0, False)
    assert float(ref.abs().sum()) == 0
    assert torch.equal(c.reference(ops, ops.EPI_SGD, 1.0, False), c.C0[:, :c.N])
    assert torch.equal(c.reference(ops, ops.EPI_BIAS, 1.0, False), c.bias.expand(c.M, c.N))
    assert _tickets_zero(ws)


@pytest.mark.parametrize("M,N", [(0, 24), (24, 0)])
def test_gemm_empty_output_is_a_no_op(ops, M, N):
    """M == 0 or N == 0: DLRM_OK and not one byte written, in every layout."""
    ws = _workspace()
    for ta, tb in LAYOUTS:
        c = IntCase(M, N, 40, ta, tb, seed=4)
        C = padded(torch.zeros(M, N, device=dev), 2, 4, SENTINEL)
        for epi in (ops.EPI_STORE, ops.EPI_SGD):
            ops.gemm_group([ops.gemm_problem(c.A, c.B, bool(ta), bool(tb), C=C, alpha=1.0,
                                             epilogue=epi)[0]], ws)
        torch.cuda.synchronize()
        assert bool((C._base == SENTINEL).all()), (ta, tb)
    assert int(ws.view(torch.int64).abs().sum()) == 0


# -------------------------------------------------------------- g. epilogue rounding --
# The epilogue is TWO roundings, fl(old -+ fl(alpha * acc)) and fl(fl(alpha * acc) + bias)
# (common.hpp dlrm_scale, then one rounded add or subtract), on every output path.  The
# integer cases above cannot tell that from one fused multiply-add: every rounding is exact
# for them.  Here op(A) is one-hot and op(B) full-mantissa (section b: every accumulator is
# one correctly rounded product, every row sum the row's single nonzero, a K split adds exact
# zeros), alpha is fp32(0.7) and the old C and the bias are full-mantissa with random signs,
# so the fused result differs from the two-rounding one in a large share of the elements -
# asserted before anything runs.  All references are float64 on the CPU: alpha * acc of two
# fp32 values has 48 significant bits and is exact there, and so is its sum with a third fp32
# value of a similar exponent, so each .float() below is exactly one fp32 rounding.
ALPHA_R = float(np.float32(0.7))  # not a "round" rate: at 0.1 only 5 % of the elements differ


def _signed_mantissas(shape, g):
    sign = torch.randint(0, 2, shape, generator=g, device=g.device).float() * 2 - 1
    return full_mantissa(shape, g) * sign


def _two_and_fused(epi_name, acc64, old64, bias64, alpha=ALPHA_R):
    """(two, fused) as fp32: the two-rounding epilogue and the single fused multiply-add."""
    prod = alpha * acc64                  # exact in float64
    scaled = prod.float().double()        # fl(alpha * acc)
    if epi_name == "sgd":
        return (old64 - scaled).float(), (old64 - prod).float()
    if epi_name == "accum":
        return (old64 + scaled).float(), (old64 + prod).float()
    assert epi_name == "bias"
    return (scaled + bias64).float(), (prod + bias64).float()


class RoundingCase:
    """One-hot op(A) [M, K] x full-mantissa op(B) [K, N] in layout (ta, tb), the old C
    [M, N + 4] (column N takes the row sums of a ones_col problem) and a bias; built once per
    (M, layout) and shared - the kernels only read it."""

    def __init__(self, ta, tb, M, N=96, K=512, seed=7):
        self.M, self.N, self.ta, self.tb = M, N, ta, tb
        self.A, self.B, acc = _one_hot_pair(ta, tb, False, M, N, K, seed)
        g = _gen(4000 + 16 * seed + 2 * ta + tb + 8 * M)
        self.C0 = _signed_mantissas((M, N + 4), g)
        self.bias = _nan_vector(_signed_mantissas((N,), g))
        opA = self.A.t() if ta else self.A
        self.rowsum64 = opA.double().sum(1).cpu()  # one nonzero per row: exact
        assert int((opA != 0).sum(1).max()) == 1
        self.acc64 = acc.double().cpu()

    def references(self, epi_name, ones):
        """(two, fused, old) over the written width: N, or N + 1 with the row-sum column."""
        acc = self.acc64
        if ones:
            assert epi_name != "bias"  # no bias column
            acc = torch.cat([acc, self.rowsum64[:, None]], 1)
        w = acc.shape[1]
        old = self.C0.cpu()
        bias = self.bias.double().cpu() if epi_name == "bias" else None
        two, fused = _two_and_fused(epi_name, acc, old[:, :w].double(), bias)
        return two, fused, old

    def condition(self, epi_name, ones, min_rowsums=None):
        """two != fused in >= 25 % of the M x N block and >= 10 % of the ones_col column (or
        ``min_rowsums`` of its elements, for a small M)."""
        two, fused, _ = self.references(epi_name, ones)
        d = two != fused
        share = float(d[:, :self.N].float().mean())
        assert share >= 0.25, (epi_name, share)
        if ones:
            n = int(d[:, self.N].sum())
            need = min_rowsums if min_rowsums is not None else 0.10 * self.M
            assert n >= need, (epi_name, "row sums", n, self.M)

    def output(self, ones):
        return padded(self.C0 if ones else self.C0[:, :self.N], 2, 4, SENTINEL)

    def problem(self, ops, C, epi_name, ones, A=None, **kw):
        epi = {"sgd": ops.EPI_SGD, "accum": ops.EPI_ACCUM, "bias": ops.EPI_BIAS}[epi_name]
        A = padded(self.A, 2, 4, NAN) if A is None else A
        return ops.gemm_problem(A, padded(self.B, 2, 4, NAN), bool(self.ta), bool(self.tb), C=C,
                                alpha=ALPHA_R, epilogue=epi, bias=self.bias,
                                ones_col=self.N if ones else -1, **kw)[0]

    def check(self, C, epi_name, ones, what=()):
        """C equals the two-rounding reference bitwise; its other columns keep the old C."""
        two, fused, old = self.references(epi_name, ones)
        ref = old[:, :C.shape[1]].clone()
        ref[:, :two.shape[1]] = two
        got = C.cpu()
        tag = (self.M, self.ta, self.tb, epi_name, ones) + tuple(what)
        if not torch.equal(got, ref):
            as_fused = int(((got[:, :two.shape[1]] == fused) & (two != fused)).sum())
            raise AssertionError((tag, _first_diff(got, ref),
                                  f"{as_fused} of {int((two != fused).sum())} elements that "
                                  f"can tell hold the FUSED result"))

    def run_and_check(self, ops, ws, epi_name, ones, what=(), A=None):
        C = self.output(ones)
        ops.gemm_group([self.problem(ops, C, epi_name, ones, A=A)], ws)
        self.check(C, epi_name, ones, what)
        assert pads_intact(C), what


# (layout, epilogue, ones_col): the forward with its bias, the wgrad with the fused update
ROUNDING_KINDS = [((0, 1), "bias", False), ((1, 0), "sgd", True), ((1, 0), "accum", True)]


@functools.lru_cache(maxsize=None)
def _rounding_case(ta, tb, M=128):
    return RoundingCase(ta, tb, M)


def _rounding_cases(M=128, kinds=ROUNDING_KINDS, min_rowsums=None):
    out = []
    for (ta, tb), epi_name, ones in kinds:
        c = _rounding_case(ta, tb, M)
        c.condition(epi_name, ones, min_rowsums)
        out.append((c, epi_name, ones))
    return out


@pytest.mark.parametrize("cfg", GEMM_CFGS)
def test_gemm_rounding_pipelined(ops, cfg):
    """The batched epilogue of the pipelined body: every tile, unsplit and split 4, the
    forward layout with EPI_BIAS and the wgrad layout with EPI_SGD and EPI_ACCUM and the
    ones_col row sums - each element the two-rounding result, bitwise."""
    cases = _rounding_cases()
    ws = _workspace()
    for split in (1, 4):
        for c, epi_name, ones in cases:
            with ops.tuning(gemm_tile=cfg, gemm_split=split):
                c.run_and_check(ops, ws, epi_name, ones, what=(cfg, split))
    assert _tickets_zero(ws)


def test_gemm_rounding_64bit_epilogue(ops):
    """finish_tile's 64-bit fallback: the same problem at M = 16 with C a strided view whose
    rows lie 1 972 832 floats apart, so (M + 256) * ldc * 4 passes the 32-bit offset limit
    and the batched epilogue is not taken.  EPI_SGD with the row sums and EPI_BIAS, unsplit
    and split 4 on the default tile; every other float of the buffer keeps its sentinel."""
    M, ldc = 16, 1_972_832
    cases = _rounding_cases(M, [ROUNDING_KINDS[1], ROUNDING_KINDS[0]], min_rowsums=2)
    ws = _workspace()
    buf = torch.full((M * ldc,), SENTINEL, device=dev)
    for split in (1, 4):
        for c, epi_name, ones in cases:
            w = c.N + 4 if ones else c.N
            C = buf.as_strided((M, w), (ldc, 1))
            assert C.stride(0) == ldc and C.data_ptr() == buf.data_ptr()
            assert (M + 256) * C.stride(0) * 4 >= 0x7ff00000  # gemm.hip epi_fits: false
            C.copy_(c.C0[:, :w])
            with ops.tuning(gemm_split=split):
                ops.gemm_group([c.problem(ops, C, epi_name, ones)], ws)
            c.check(C, epi_name, ones, what=("64-bit", split))
            C.fill_(SENTINEL)  # what is left must be the untouched fill, bit for bit
            assert bool((buf.view(torch.int32) ==
                         torch.tensor(SENTINEL).view(torch.int32).item()).all()), (epi_name, split)
    assert _tickets_zero(ws)


@pytest.mark.parametrize("epi_name", ["sgd", "accum"])
@pytest.mark.parametrize("requested", [1, 3])
def test_gemm_rounding_partial_then_reduce(ops, epi_name, requested):
    """PARTIAL, then the REDUCE job of a later launch: the weight columns (the float4 path)
    and the bias column (one element per thread) both hold the two-rounding result, hence
    agree with each other."""
    (c, _, ones), = _rounding_cases(kinds=[((1, 0), epi_name, True)])
    ws = _workspace()
    C = c.output(ones)
    s = ops.gemm_splits(c.problem(ops, C, epi_name, ones), partial=True, requested=requested)
    assert s == _normalized_splits(requested, 512)
    part = torch.full((ops.gemm_partial_bytes(c.M, c.N, s) // 4,), NAN, device=dev)
    pp = c.problem(ops, C, epi_name, ones, partial=part, splits=s)
    ops.gemm_group([pp], ws)
    assert torch.equal(C, c.C0)  # PARTIAL leaves C alone
    ops.gemm_group([ops.reduce_problem(pp)], ws)
    c.check(C, epi_name, ones, what=("reduce", requested))
    assert pads_intact(C)
    assert _tickets_zero(ws)


def test_gemm_rounding_generic_and_rowsum_kernels(ops):
    """The element-guarded fallback and its row-sum kernel (A one float off 16-byte
    alignment): EPI_SGD with ones_col, and EPI_BIAS."""
    ws = _workspace()
    for c, epi_name, ones in _rounding_cases(kinds=[ROUNDING_KINDS[1], ROUNDING_KINDS[0]]):
        c.run_and_check(ops, ws, epi_name, ones, what=("generic",),
                        A=_offset_by_one_float(c.A, 2, 4))
    assert _tickets_zero(ws)


def test_gemm_rounding_sgd_job(ops):
    """ops.sgd_job alone in a launch on flat full-mantissa p and g: fl(p - fl(lr * g)), not
    the fused multiply-add; nothing past the parameter is written."""
    ws = _workspace()
    g = _gen(53)
    n = 4100
    p0, grad = _signed_mantissas((n,), g), _signed_mantissas((n,), g)
    two, fused = _two_and_fused("sgd", grad.double().cpu(), p0.double().cpu(), None)
    assert float((two != fused).float().mean()) >= 0.25
    buf = torch.full((n + 64,), SENTINEL, device=dev)
    p = buf[:n]
    p.copy_(p0)
    ops.gemm_group([ops.sgd_job(p, grad, ALPHA_R)], ws)
    got = p.cpu()
    assert torch.equal(got, two), (_first_diff(got, two),
                                   int(((got == fused) & (two != fused)).sum()), "hold fused")
    assert bool((buf[n:] == SENTINEL).all())
    assert _tickets_zero(ws)


# ------------------------------------------------------------ bottom-MLP chain --
def _pad4(n):
    return (n + 3) // 4 * 4


def _exact_mlp(rows, dims, seed=5):
    """The trainer's bias-folded layout (test_gpu_kernels._mlp_setup) with X in {0, 1} and W
    in {-1, 0, 1}, operands NaN-padded, outputs sentinel-filled; and the fp64 reference walked
    layer by layer with max(|h| @ |W|^T) < 2^24 asserted (W thinned by the seeded generator
    until it holds, never the comparison loosened).  -> X, layers, refs"""
    g = _gen(seed)
    k0 = dims[0]
    X0 = torch.zeros(rows, _pad4(k0 + 1), device=dev)
    X0[:, :k0] = int_matrix((rows, k0), 0, 1, g, nonzero=False)
    X0[:, k0] = 1.0
    X = padded(X0, 2, 4, NAN)
    layers, refs = [], []
    h = X0.double()
    for k, n in zip(dims[:-1], dims[1:]):
        kin = _pad4(k + 1)
        W0 = torch.zeros(n, kin, device=dev)
        W0[:, :k + 1] = int_matrix((n, k + 1), -1, 1, g, nonzero=False)
        while not exact_bound_ok(h[:, :kin].abs(), W0.double().abs().t()):
            W0 *= (torch.rand(W0.shape, generator=g, device=dev) >= 0.25)  # zero a quarter
        assert exact_bound_ok(h[:, :kin].abs(), W0.double().abs().t())
        y = torch.relu(h[:, :kin] @ W0.double().t())
        refs.append(y.float())
        assert torch.equal(refs[-1].double(), y)
        Y = padded(torch.full((rows, _pad4(n + 1)), SENTINEL, device=dev), 2, 4, SENTINEL)
        layers.append((padded(W0, 2, 4, NAN), Y, kin))
        h = torch.zeros(rows, _pad4(n + 1), dtype=torch.float64, device=dev)
        h[:, :n] = y
        h[:, n] = 1.0
    return X, layers, refs


def _check_mlp(layers, refs, what):
    torch.cuda.synchronize()
    for l, ((W, Y, _), r) in enumerate(zip(layers, refs)):
        n = W.shape[0]
        assert torch.equal(Y[:, :n], r), (what, l, _first_diff(Y[:, :n], r))
        assert bool((Y[:, n:] == SENTINEL).all()) and pads_intact(Y), (what, l)
        Y._base.fill_(SENTINEL)


@pytest.mark.parametrize("rows,dims", [(37, [13, 512, 256, 128]), (100, [3, 64, 16]),
                                       (48, [200, 120, 500, 33])])
def test_mlp_chain_exact(ops, rows, dims):
    """The row-block bottom-MLP chain on {0, 1} inputs and {-1, 0, 1} weights: every layer's
    activations bitwise the fp64 chain's, columns >= out_width and the guard rows untouched -
    as one workgroup per row block, split in two on the first splittable layer, and fused
    into the presort launch (sort + bottom MLP, no lookup)."""
    X, layers, refs = _exact_mlp(rows, dims)
    chain = ops.mlp_chain(X, layers)
    assert ops.mlp_chain_supported(chain)
    ops.mlp_chain_forward(chain)
    _check_mlp(layers, refs, "chain")
    split = next(l for l, (W, _, _) in enumerate(layers) if (W.shape[0] + 15) // 16 >= 2)
    tk = torch.zeros((rows + 15) // 16, dtype=torch.int32, device=dev)
    chain2 = ops.mlp_chain(X, layers, parts=2, split_layer=split, tickets=tk)
    assert ops.mlp_chain_supported(chain2)
    ops.mlp_chain_forward(chain2)
    _check_mlp(layers, refs, "parts=2")
    assert int(tk.abs().sum()) == 0
    T, B = 3, rows
    idx = torch.randint(0, 50, (T * B,), dtype=torch.int32, device=dev)
    off = torch.arange(T * B + 1, dtype=torch.int32, device=dev)
    row_base = torch.arange(T + 1, dtype=torch.int64, device=dev) * 50
    Wt = torch.zeros(T * 50, 16, device=dev)
    ws = torch.zeros(ops.tbe_backward_workspace_size(T * B, T * 50, 16), dtype=torch.uint8,
                     device=dev)
    assert ops.tbe_forward_presort(Wt, row_base, T, B, idx, off, ws, B, bottom=chain,
                                   lookup=False) is None
    _check_mlp(layers, refs, "fused into the presort launch")


# ------------------------------------------------------------- dot interaction --
def _interact_reference(x, ly, gR, self_int):
    """fp64 bmm + tril gather and autograd on it -> R, grad_x (ReLU'(x) applied), grad_ly."""
    F = ly.shape[1] + 1
    xr = x.double().requires_grad_(True)
    lr_ = ly.double().requires_grad_(True)
    T = torch.cat([xr[:, None, :], lr_], 1)
    Z = torch.bmm(T, T.transpose(1, 2))
    li, lj = torch.tril_indices(F, F, 0 if self_int else -1, device=dev)
    R = torch.cat([xr, Z[:, li, lj]], 1)
    (R * gR.double()).sum().backward()
    gx = xr.grad * (x > 0)
    for t in (R, gx, lr_.grad):
        assert float(t.detach().abs().max()) < 2 ** 24
    return R.detach().float(), gx.float(), lr_.grad.float()


def _grad_buffers(B, T, D):
    gx = padded(torch.zeros(B, D, device=dev), 2, 4, SENTINEL)
    gl2 = padded(torch.zeros(B, T * D, device=dev), 2, 4, SENTINEL)
    return gx, gl2, gl2.view(B, T, D)


def _misaligned(t):
    buf = torch.full((t.numel() + 4,), NAN, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("B,F,D", [(5, 2, 16), (70, 27, 128), (33, 32, 64), (7, 9, 4),
                                   (5, 41, 8)])
@pytest.mark.parametrize("self_int", [False, True])
def test_interact_dot_exact(ops, B, F, D, self_int):
    """Dot interaction forward and backward on integers in [-3, 3] (x with zeros and
    negatives, relu_x fused): R, grad_x and grad_ly bitwise the fp64 bmm + tril reference
    and its autograd - LDS-staged kernels under every forced version (v3 / v4 / v5), the
    runtime-D kernel (16-byte-misaligned features; D = 4), the VALU path (F = 41), the
    list-of-tensors layout, and the gather-fused forward / backward; NaN-padded x, ly,
    tables and grad_out, sentinel-padded outputs."""
    g = _gen(100 * B + F + D + self_int)
    T = F - 1
    x0 = int_matrix((B, D), -3, 3, g, nonzero=False)
    assert bool((x0 == 0).any()) and bool((x0 < 0).any())
    rows = [int(r) for r in torch.randint(1, 60, (T,), generator=g, device=dev)]
    row_base = torch.tensor([0] + list(np.cumsum(rows)), dtype=torch.int64, device=dev)
    W = padded(int_matrix((int(row_base[-1]), D), -3, 3, g, nonzero=False), 2, 0, NAN)
    idx = torch.cat([torch.randint(0, n, (B,), generator=g, device=dev) for n in rows])
    ly0 = W[(row_base[:-1, None] + idx.view(T, B)).t()]  # [B, T, D]: the looked-up rows
    ly = padded(ly0.reshape(B, T * D), 2, 4, NAN).view(B, T, D)  # batch stride T * D + 4
    assert W.is_contiguous() and torch.equal(ly, ly0)
    npairs = F * (F + 1) // 2 if self_int else F * (F - 1) // 2
    gR0 = int_matrix((B, D + npairs), -3, 3, g, nonzero=False)
    R_ref, gx_ref, gly_ref = _interact_reference(x0, ly, gR0, self_int)
    x, gR = padded(x0, 2, 4, NAN), padded(gR0, 2, 4, NAN)

    def check_fwd(R, what):
        assert torch.equal(R, R_ref), (what, _first_diff(R, R_ref))
        assert R._base is None or pads_intact(R), what

    def check_bwd(gx, gly, what, bufs=()):
        assert torch.equal(gx, gx_ref), (what, "gx", _first_diff(gx, gx_ref))
        gly = torch.stack(list(gly), 1) if isinstance(gly, (list, tuple)) else gly
        assert torch.equal(gly, gly_ref), (what, "gly", _first_diff(gly, gly_ref))
        for b in bufs:
            assert pads_intact(b), what

    def out_buf():
        return padded(torch.zeros(B, D + npairs, device=dev), 2, 4, SENTINEL)

    for v in (4, 5, 0):  # staged (compile-time D) where it applies, else runtime-D / VALU
        with ops.tuning(interact_fwd=v):
            check_fwd(ops.interact_forward("dot", x, ly, self_int, out=out_buf()), ("fwd", v))
    for v in (4, 3, 5, 0):
        gx, gl2, gl = _grad_buffers(B, T, D)
        with ops.tuning(interact_bwd=v):
            ops.interact_backward("dot", x, ly, gR, self_int, grad_x=gx, grad_ly=gl,
                                  relu_x=True)
        check_bwd(gx, gl, ("bwd", v), (gx, gl2))
    # 16-byte-misaligned features: the runtime-D MFMA kernel (F <= 32) + the mask pass
    xm, lym = _misaligned(x0), _misaligned(ly0)
    check_fwd(ops.interact_forward("dot", xm, lym, self_int, out=out_buf()), "misaligned")
    check_bwd(*ops.interact_backward("dot", xm, lym, gR, self_int, relu_x=True),
              what="misaligned")
    # list-of-[B, D] layout
    lyl = [ly[:, t].contiguous() for t in range(T)]
    check_fwd(ops.interact_forward("dot", x, lyl, self_int, out=out_buf()), "list")
    check_bwd(*ops.interact_backward("dot", x, lyl, gR, self_int, relu_x=True), what="list")
    if D in (16, 32, 64, 128) and F <= 32:  # the lookup fused in
        i32 = idx.to(torch.int32)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        for v in (4, 5, 0):
            with ops.tuning(interact_fwd=v):
                R = ops.interact_forward_gather(x, W, row_base, i32, self_int, out=out_buf(),
                                                error_flag=err)
            check_fwd(R, ("gather fwd", v))
        assert int(err.item()) == 0
        for v in (4, 3, 5, 0):
            gx, gl2, gl = _grad_buffers(B, T, D)
            with ops.tuning(interact_bwd=v):
                ops.interact_backward_gather(x, W, row_base, i32, gR, self_int, grad_x=gx,
                                             grad_ly=gl, relu_x=True)
            check_bwd(gx, gl, ("gather bwd", v), (gx, gl2))
