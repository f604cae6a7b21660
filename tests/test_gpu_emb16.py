"""fp16 embedding tables in the fused engine (TrainerConfig.emb_precision = "fp16", ABI v15).

The reference of every test is the existing fp32 path run on the same half values upcast to
fp32: fp16 -> fp32 is exact and nothing after the load changes, so every comparison is
BITWISE (int views), never a tolerance.

Shapes are the smallest that reach every kernel: (B, D) of the gather tests cross one
workgroup (B = 5), a ragged last workgroup (70), and kV5MaxBatch = 1024 (1028: forward v4 and
backward v3 by default at D >= 64); DLRM_TUNE_INTERACT_FWD / _BWD force the other variants, as
the fp32 interaction tests do."""
import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu
dev = "cuda:0"
V5_MAX_BATCH = 1024  # interact.hip kV5MaxBatch


@pytest.fixture(scope="module")
def ops():
    from dlrm_hip import ops as _ops
    return _ops


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------- 1. gather kernels --
GATHER_SHAPES = [(5, 16), (5, 32), (70, 64), (70, 128), (1028, 64), (1028, 128)]
GATHER_F = [(2, False), (9, True), (27, False), (32, False)]


def _fwd_version(D, B, t):
    """interact.hip fwd_version: the forward kernel DLRM_TUNE_INTERACT_FWD = t selects."""
    if t == 4:
        return 4
    if t == 5:
        return 5 if D >= 64 else 4
    return 5 if D >= 64 and B <= V5_MAX_BATCH else 4


def _bwd_version(D, B, t):
    if t in (3, 4):
        return t
    if t == 5:
        return 5 if D >= 64 else 4
    if D <= 32:
        return 4
    return 5 if B <= V5_MAX_BATCH else 3


def test_gather_cases_reach_every_variant():
    """The (B, D) list with the tuning values the tests below force reaches forward v4 and v5
    and backward v3, v4 and v5 - by default dispatch too, not only when forced."""
    fwd = {_fwd_version(D, B, t) for B, D in GATHER_SHAPES for t in (0, 4, 5)}
    bwd = {_bwd_version(D, B, t) for B, D in GATHER_SHAPES for t in (0, 3, 4, 5)}
    assert fwd == {4, 5} and bwd == {3, 4, 5}
    assert {_fwd_version(D, B, 0) for B, D in GATHER_SHAPES} == {4, 5}
    assert {_bwd_version(D, B, 0) for B, D in GATHER_SHAPES} == {3, 4, 5}


def _gather_case(B, D, F, seed, bad=False):
    """T = F - 1 tiny fp16 tables (<= 50 rows, the second-to-last of 1 row), every row that no
    index names NaN; indices with duplicates (B lookups into <= 50 rows, and the first two
    samples share their rows); strided x.  ``bad``: one index past its table."""
    g = torch.Generator().manual_seed(seed)
    T = F - 1
    rows = [int(r) for r in torch.randint(2, 51, (T,), generator=g)]
    rows[max(T - 2, 0)] = 1
    base = [0] + np.cumsum(rows).tolist()
    idx = torch.stack([torch.randint(0, n, (B,), generator=g) for n in rows])  # [T, B]
    if B > 1:
        idx[:, 1] = idx[:, 0]
    W = torch.full((base[-1], D), float("nan"), dtype=torch.float16)
    named = torch.cat([base[t] + idx[t] for t in range(T)]).unique()
    W[named] = (torch.randn(named.numel(), D, generator=g) * 0.5).half()
    if bad:
        t = T // 2
        idx[t, B // 2] = rows[t]  # one past the table's last row: the next table's first
    x = torch.randn(B, D + 4, generator=g).to(dev)[:, :D]
    row_base = torch.tensor(base, dtype=torch.int64, device=dev)
    return x, W.to(dev), row_base, idx.reshape(-1).to(torch.int32).to(dev), T


def _guarded(rows, *shape, fill, used=None):
    """[rows + 2, ...] filled with a sentinel; the middle ``rows`` (their first ``used``
    columns) are the kernel's output, the rest are guards that must keep their bits."""
    buf = torch.full((rows + 2,) + shape, fill, dtype=torch.float32, device=dev)
    out = buf[1:rows + 1]
    return buf, out if used is None else out[:, :used]


def _guards_intact(buf, fill, used=None):
    want = torch.full_like(buf, fill)
    ok = _same(buf[0], want[0]) and _same(buf[-1], want[-1])
    return ok and (used is None or _same(buf[:, used:], want[:, used:]))


def _run_gather(ops, x, W, row_base, idx, T, self_int, gR, fwd_t, bwd_t, flag=None):
    B, D = x.shape
    width = gR.shape[1]
    ld = (width + 3) // 4 * 4 + 4  # 16-byte aligned rows (the float4 stores) and pad columns
    obuf, out = _guarded(B, ld, fill=-77.0, used=width)
    xbuf, gx = _guarded(B, D, fill=-78.0)
    lbuf, gly = _guarded(B, T, D, fill=-79.0)
    with ops.tuning(interact_fwd=fwd_t, interact_bwd=bwd_t):
        ops.interact_forward_gather(x, W, row_base, idx, self_int, out=out, error_flag=flag)
        ops.interact_backward_gather(x, W, row_base, idx, gR, self_int, grad_x=gx, grad_ly=gly,
                                     relu_x=True)
    torch.cuda.synchronize()
    assert _guards_intact(obuf, -77.0, used=width) and _guards_intact(xbuf, -78.0)
    assert _guards_intact(lbuf, -79.0)
    return out.clone(), gx.clone(), gly.clone()


@pytest.mark.parametrize("F,self_int", GATHER_F)
@pytest.mark.parametrize("B,D", GATHER_SHAPES)
def test_gather_f16_is_the_fp32_gather_on_the_same_values(ops, B, D, F, self_int):
    x, W, row_base, idx, T = _gather_case(B, D, F, seed=B * 1000 + D * 10 + F)
    Wf = W.float()
    npairs = F * (F + 1) // 2 if self_int else F * (F - 1) // 2
    gR = torch.randn(B, D + npairs, device=dev)
    for fwd_t, bwd_t in ((0, 0), (4, 3), (5, 4), (0, 5)):
        got = _run_gather(ops, x, W, row_base, idx, T, self_int, gR, fwd_t, bwd_t)
        want = _run_gather(ops, x, Wf, row_base, idx, T, self_int, gR, fwd_t, bwd_t)
        for name, a, b in zip(("R", "grad_x", "grad_ly"), got, want):
            assert torch.isfinite(b).all(), (name, fwd_t, bwd_t)  # no NaN row was read
            assert _same(a, b), (name, fwd_t, bwd_t)
        assert not (got[2] == -79.0).any()  # every grad_ly element written


@pytest.mark.parametrize("B,D", [(70, 64), (5, 16), (1028, 128)])
def test_gather_f16_out_of_range_index(ops, B, D):
    """One index past its table: the flag is set and the row reads as zeros, exactly as in
    the fp32 kernel (whose result on the upcast table is the reference)."""
    F = 9
    x, W, row_base, idx, T = _gather_case(B, D, F, seed=D + B, bad=True)
    gR = torch.randn(B, D + F * (F - 1) // 2, device=dev)
    for fwd_t, bwd_t in ((0, 0), (4, 3), (5, 5)):
        f16 = torch.zeros(1, dtype=torch.int32, device=dev)
        f32 = torch.zeros(1, dtype=torch.int32, device=dev)
        got = _run_gather(ops, x, W, row_base, idx, T, False, gR, fwd_t, bwd_t, flag=f16)
        want = _run_gather(ops, x, W.float(), row_base, idx, T, False, gR, fwd_t, bwd_t, flag=f32)
        assert int(f16.item()) == int(f32.item()) == ops.TBE_ERR_INDEX
        for a, b in zip(got, want):
            assert torch.isfinite(b).all() and _same(a, b)
        t, b_bad = T // 2, B // 2
        assert not got[2][b_bad, t].isnan().any()


def test_gather_rejects_other_row_types(ops):
    x, W, row_base, idx, T = _gather_case(5, 16, 3, seed=1)
    with pytest.raises(ValueError):
        ops.interact_forward_gather(x, W.to(torch.bfloat16), row_base, idx)


# ------------------------------------------- 2. sgd_f16 with a device-resident rate --
@pytest.mark.parametrize("mx_kind", ["cap", "none"])  # per-table and device-wide sort
@pytest.mark.parametrize("D", [16, 128])
def test_tbe_backward_sgd_f16_device_rate(ops, D, mx_kind):
    torch.manual_seed(D)
    rows, B, L = [3, 5000, 4, 700], 512, 2
    T = len(rows)
    lo = [torch.arange(B) * L for _ in rows]
    li = [torch.randint(0, n, (B * L,)) for n in rows]
    li[1][: B * L * 3 // 4] = 7  # the skewed table: three quarters of its lookups hit one row
    off, idx = O.batched_csr(lo, li)
    off, idx = off.to(dev), idx.to(dev)
    row_base = torch.tensor([0] + np.cumsum(rows).tolist(), dtype=torch.int64, device=dev)
    G = torch.randn(B, T, D, device=dev)
    W0 = (torch.randn(sum(rows), D) * 0.5).half().to(dev)
    mx = B * L if mx_kind == "cap" else 0
    lr = 0.05
    lr_dev = torch.tensor([lr], dtype=torch.float32, device=dev)
    Wh, Wd, Wn = W0.clone(), W0.clone(), W0.clone()
    ops.tbe_backward("sgd_f16", Wh, row_base, T, B, idx, off, G, lr=lr, max_lookups_per_table=mx)
    ops.tbe_backward("sgd_f16", Wd, row_base, T, B, idx, off, G, lr=lr_dev,
                     max_lookups_per_table=mx)
    ops.tbe_backward("sgd", Wn, row_base, T, B, idx, off, G, lr=lr_dev, max_lookups_per_table=mx)
    torch.cuda.synchronize()
    assert _same(Wd, Wh) and _same(Wn, Wh)
    assert (_bits(Wh) != _bits(W0)).any()
    lr_dev.fill_(0.0)  # the rate is read when the kernel runs
    Wz = W0.clone()
    ops.tbe_backward("sgd_f16", Wz, row_base, T, B, idx, off, G, lr=lr_dev,
                     max_lookups_per_table=mx)
    assert _same(Wz, W0)
    with pytest.raises(ValueError):
        ops.tbe_backward("sgd_f16", W0.float(), row_base, T, B, idx, off, G, lr=lr)


# ------------------------------------------------------------------ trainers --------
MODELS = {
    "d16": dict(D=16, rows=[30, 1000, 257, 64], bot=[13, 32, 16], top=[64, 32, 1], B=48),
    "d64": dict(D=64, rows=[1000, 30, 500], bot=[13, 64, 32, 64], top=[48, 1], B=260),
}


def _cfg(model, **kw):
    from dlrm_hip.trainer import TrainerConfig
    m = MODELS[model]
    F = len(m["rows"]) + 1
    return TrainerConfig(m_spa=m["D"], ln_emb=m["rows"], ln_bot=m["bot"],
                         ln_top=[m["D"] + F * (F - 1) // 2] + m["top"], loss_function="bce",
                         learning_rate=0.1, emb_learning_rate=0.3, **kw)


def _pair(model, fuse_gather=True, **kw):
    """A: fp16 tables.  S (the shadow): fp32 tables holding A's values, same dense bucket."""
    from dlrm_hip.trainer import DLRMTrainer
    A = DLRMTrainer(_cfg(model, emb_precision="fp16", **kw), device=dev, seed=3)
    S = DLRMTrainer(_cfg(model, **kw), device=dev, seed=3)
    assert A.weights.dtype == torch.float16 and S.weights.dtype == torch.float32
    S.weights.copy_(A.weights.float())
    S.params.copy_(A.params)
    A.fuse_gather = S.fuse_gather = fuse_gather
    return A, S


def _assert_shadow(A, S, what):
    for i, (a, s) in enumerate(zip(A.layers, S.layers)):
        assert _same(a.W, s.W), f"{what}: layer {i}"
    for t in range(A.T):
        assert A.table(t).dtype == torch.float16
        assert _same(A.table(t), S.table(t).half()), f"{what}: table {t}"


def _round_shadow(S):
    S.weights.copy_(S.weights.half().float())


@pytest.mark.parametrize("model", sorted(MODELS))
def test_init_random_is_the_fp32_init_rounded_once(model):
    from dlrm_hip.trainer import DLRMTrainer
    A = DLRMTrainer(_cfg(model, emb_precision="fp16"), device=dev, seed=0, init=False)
    S = DLRMTrainer(_cfg(model), device=dev, seed=0, init=False)
    A._F16_INIT_CHUNK = 1000  # several staging chunks per table, a ragged last one
    for seed in (0, 5):
        A.init_random(seed)
        S.init_random(seed)
        for t in range(A.T):
            assert A.table(t).dtype == torch.float16 and A.table(t).shape == S.table(t).shape
            assert _same(A.table(t), S.table(t).half())
        assert _same(A.params, S.params)
    assert A.weights.element_size() * 2 == S.weights.element_size()


SHADOW_CASES = [
    # model, gather-fused, graph replay, mlp_precision, device rates with a schedule
    ("d16", True, False, "fp32", False),
    ("d16", True, True, "fp32", False),
    ("d16", False, False, "fp32", False),
    ("d16", False, True, "bf16", True),
    ("d16", True, False, "bf16", True),
    ("d16", True, True, "fp32", True),
    ("d64", True, False, "fp32", False),
    ("d64", True, True, "bf16", False),
    ("d64", False, False, "fp32", True),
    ("d64", False, True, "fp32", False),
    ("d64", True, True, "bf16", True),
    ("d64", False, False, "bf16", False),
]
POLICY = dict(lr_num_warmup_steps=2, lr_decay_start_step=3, lr_num_decay_steps=2)


@pytest.mark.parametrize("model,gather,graph,mlp,dev_lr", SHADOW_CASES)
def test_shadow_trajectory(model, gather, graph, mlp, dev_lr):
    """Four steps over two alternating one-hot batches: the fp16-table trainer against an fp32
    trainer on the same values whose tables are rounded to fp16 after every step.  Loss,
    probabilities, every dense parameter and every table are bit-equal after every step, and
    no row outside the batches changes."""
    kw = dict(mlp_precision=mlp, **(POLICY if dev_lr else {}))
    A, S = _pair(model, fuse_gather=gather, **kw)
    assert A.cfg.lr_mode == ("device" if dev_lr else "host")
    B = MODELS[model]["B"]
    batches = [A.synthetic_batch(B, 1, seed=s) for s in (11, 12)]
    W0 = A.weights.clone()
    touched = torch.zeros(A.total_rows, dtype=torch.bool, device=dev)
    for b in batches:
        rows = b.indices.view(A.T, B).long() + A.row_base[:-1, None]
        touched[rows.reshape(-1)] = True
    assert 0 < int(touched.sum()) < A.total_rows
    run_a = None
    if graph:  # one eager step for the allocations, then the state and the schedule put back
        from dlrm_hip.trainer import Batch
        fixed = Batch(*(t.clone() for t in (batches[0].X, batches[0].offsets, batches[0].indices,
                                             batches[0].target)),
                      batches[0].max_per_table, batches[0].one_hot)
        P0 = A.params.clone()
        A.step(fixed)
        A.weights.copy_(W0)
        A.params.copy_(P0)
        if dev_lr:
            A.lr_step = 1
        run_a = A.capture(fixed)
        assert A.capture_mode == "whole" and A.graphs_per_step == 1
    for i in range(4):
        b = batches[i % 2]
        if graph:
            for dst, src in ((fixed.X, b.X), (fixed.indices, b.indices), (fixed.target, b.target)):
                dst.copy_(src)
            run_a()
            pa, la = A._cur["prob"], A._cur["loss"]
        else:
            pa, la = A.step(b)
        ps, ls = S.step(b)
        _round_shadow(S)
        what = f"step {i + 1}"
        assert A.gather_fused == S.gather_fused == gather, what
        assert _same(la, ls), f"{what}: loss {la.item()} vs {ls.item()}"
        assert _same(pa, ps), what
        _assert_shadow(A, S, what)
        assert _same(A.weights[~touched], W0[~touched]), what
        if dev_lr:
            assert A.current_lr() == S.current_lr(), what
    assert (_bits(A.weights[touched]) != _bits(W0[touched])).any()
    A.check_errors()
    S.check_errors()


@pytest.mark.parametrize("known_bound", [True, False])  # False: the early side-stream sort
@pytest.mark.parametrize("model", sorted(MODELS))
def test_multi_hot_first_step(model, known_bound):
    """Bags of 0-3 lookups.  Table entries are multiples of 2^-8 in [-1, 1]: any summation
    order of <= 3 of them is exact in fp32, so the fp16 pooled lookup and the fp32 one cannot
    differ by order, and step 1 is bit-equal.  (Later steps are not required to be: the updated
    rows are arbitrary halves.)"""
    A, S = _pair(model)
    g = torch.Generator().manual_seed(17)
    W = torch.randint(-256, 257, tuple(A.weights.shape), generator=g).float() / 256.0
    A.weights.copy_(W)
    S.weights.copy_(W)
    assert _same(A.weights.float(), S.weights)
    m = MODELS[model]
    B = m["B"]
    lS_o, lS_i = [], []
    for n in m["rows"]:
        lens = torch.randint(0, 4, (B,), generator=g)
        lS_o.append(torch.cumsum(lens, 0) - lens)
        lS_i.append(torch.randint(0, n, (int(lens.sum()),), generator=g))
    X = torch.rand(B, m["bot"][0], generator=g)
    tg = torch.rand(B, generator=g).round()
    ba, bs = A.make_batch(X, lS_o, lS_i, tg), S.make_batch(X, lS_o, lS_i, tg)
    assert not ba.one_hot and ba.max_per_table > 0
    if not known_bound:
        ba.max_per_table = bs.max_per_table = 0
    W0 = A.weights.clone()
    pa, la = A.step(ba)
    ps, ls = S.step(bs)
    _round_shadow(S)
    assert not A.gather_fused and not S.gather_fused
    assert _same(la, ls) and _same(pa, ps)
    _assert_shadow(A, S, "step 1")
    touched = torch.zeros(A.total_rows, dtype=torch.bool, device=dev)
    for t, ii in enumerate(lS_i):
        touched[(ii + int(A.row_base[t])).to(dev)] = True
    assert _same(A.weights[~touched], W0[~touched])
    assert (_bits(A.weights) != _bits(W0)).any()
    A.check_errors()


@pytest.mark.parametrize("gather", [True, False])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_predict_and_evaluate(model, gather):
    from dlrm_hip import metrics
    A, S = _pair(model, fuse_gather=gather)
    B = MODELS[model]["B"]
    batches = [A.synthetic_batch(B, 1, seed=s) for s in (21, 22)]
    W0, P0 = A.weights.clone(), A.params.clone()
    for dt in ("fp32", "bf16", "fp16"):
        want = S.predict(batches[0], precision=dt).clone()
        got = A.predict(batches[0], precision=dt).clone()
        assert _same(got, want), dt
        run = A.capture_predict(batches[0], precision=dt)
        A.predict(batches[1], precision=dt)  # overwrite the output, then replay
        run()
        assert _same(A._predict_bufs(A._buffers(B, B))["prob"], want), dt
        sa, ss = metrics.EvalState(2 * B, dev), metrics.EvalState(2 * B, dev)
        ra = A.evaluate(batches, sa, precision=dt)
        rs = S.evaluate(batches, ss, precision=dt)
        assert sa.count == ss.count == 2 * B
        assert ra == rs, dt
    assert _same(A.weights, W0) and _same(A.params, P0)  # forward only


# ---------------------------------------------------------------- 7. refusals -------
def test_multi_gpu_is_refused_at_construction():
    from dlrm_hip.trainer import DLRMTrainer, EmulatedComm
    cfg = _cfg("d16", emb_precision="fp16")
    with pytest.raises(NotImplementedError) as e:
        DLRMTrainer(cfg, device=dev, rank=0, world_size=2, comm=EmulatedComm())
    assert "DESIGN.md §18" in str(e.value)
    DLRMTrainer(_cfg("d16"), device=dev, rank=0, world_size=2, comm=EmulatedComm())
