"""Stochastic rounding of the fp16 tables' SGD update (ABI v16).

Every comparison is BITWISE against tests/exact_sr16.py, the host restatement of the
specification (tests/test_exact_sr16_cpu.py proves it): the fp32 value before the store comes
from inputs that make it exact, or from the existing fp32 update on the same half values (the
same sort, run order and fma - §18's claim), and the host rounds it with the draw of its
(seed, step, global row, column).

Shapes are the smallest that reach every store path: D = 4 (one lane per row), 6 (scalar
columns), 16, 128, 260 (64 lanes x 2 chunks), a misaligned view (scalar columns at D % 4 == 0),
96 rows (several 16-lookup blocks), and a 40-lookup run that is finalised by the combine pass."""
import numpy as np
import pytest
import torch

import exact_sr16 as X

pytestmark = pytest.mark.gpu
dev = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from dlrm_hip import ops as _ops
    return _ops


def _hbits(t):
    """fp16 tensor / array -> uint16 numpy bits."""
    if isinstance(t, torch.Tensor):
        return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return np.ascontiguousarray(t).view(np.uint16)


def _same(a, b):
    a, b = a.contiguous(), b.contiguous()
    v = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(v), b.view(v))


# ------------------------------------------- 1. the rounding function through the kernel --
def _specials():
    f = np.float32
    v = [1.0, -1.0, 0.5, 1.5, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -11, -(1.0 + 2.0 ** -11),   # halves, midpoints
         1.0 + 3 * 2.0 ** -12, 1.0 - 2.0 ** -13, -(1.0 - 2.0 ** -13), 0.05, -0.05, 1 / 3, -2 / 3,
         3.14159, 1000.123, -12345.678, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12),       # the normal edge
         2.0 ** -15, 3 * 2.0 ** -26, -3 * 2.0 ** -26, 2.0 ** -24, 2.0 ** -25, -2.0 ** -25,  # subnormal range
         1023.5 * 2.0 ** -24, 5.3e-6, -7.7e-7, 2.0 ** -30, 1e-12,
         0.0, -0.0, -2.0 ** -40, -1e-30, 1e-40, -1e-45,                                    # zeros, tiny
         65504.0, 65519.0, 65520.0, 65530.0, -65530.0, 65535.996,                          # the last binade
         65536.0, -65536.0, 1e6, -3e38, np.inf, -np.inf, np.nan]
    return np.array(v, dtype=f)


def _kernel_case(ops, D, seed, step, misaligned=False):
    R = 96
    sp = _specials()
    v = sp[(np.arange(R * D) * 10 + 3) % sp.size].reshape(R, D)  # every value, many draws
    assert np.unique(v.view(np.uint32)).size == np.unique(sp.view(np.uint32)).size
    # +-Inf and NaN cannot arrive through the gradient (the run's compensated sum turns an
    # infinite term into NaN before the update): there the table holds the value and g is 0
    fin = np.isfinite(v)
    g = np.where(fin, -v, np.float32(0.0))
    # guard rows of NaN around the table; the misaligned view starts 2 halves into the buffer
    pad = 2 if misaligned else 0
    flat = torch.full(((R + 2) * D + pad,), float("nan"), dtype=torch.float16, device=dev)
    W = flat[pad + D: pad + D + R * D].view(R, D)
    assert D % 4 or (W.data_ptr() % 8 != 0) == misaligned
    w0 = np.where(np.signbit(v) & (v == 0), np.float32(-0.0), np.float32(0.0))  # -0 + -0 = -0
    w0 = np.where(fin, w0, v)
    W.copy_(torch.from_numpy(w0).half())
    guard0 = flat.clone()
    perm = np.random.RandomState(D).permutation(R)
    idx = torch.tensor(perm, dtype=torch.int32, device=dev)
    off = torch.arange(R + 1, dtype=torch.int32, device=dev)
    G = torch.from_numpy(g[perm]).to(dev).view(R, 1, D).contiguous()
    row_base = torch.tensor([0, R], dtype=torch.int64, device=dev)
    st = ops.sr_state(seed, step, device=dev)
    ops.tbe_backward("sgd_f16", W, row_base, 1, R, idx, off, G, lr=1.0, sr_state=st)
    torch.cuda.synchronize()
    with np.errstate(invalid="ignore"):
        v_eff = np.float32(-1.0) * g + w0  # the kernel's fma(-lr, g, w): exact here
    assert np.array_equal(v_eff.view(np.uint32), v.view(np.uint32))
    want = X.sr16_table(v_eff, seed, step)
    got = _hbits(W)
    bad = np.argwhere(got != _hbits(want))
    assert bad.size == 0, (D, bad[:5].tolist(), [(v[i, j], hex(got[i, j]), hex(_hbits(want)[i, j]))
                                                for i, j in bad[:5]])
    inside = torch.zeros_like(flat, dtype=torch.bool)
    inside[pad + D: pad + D + R * D] = True
    assert torch.equal(flat.view(torch.int16)[~inside], guard0.view(torch.int16)[~inside])
    with np.errstate(over="ignore", invalid="ignore"):
        nearest = _hbits(v_eff.astype(np.float16))
    assert (got != nearest).any()  # the store is not the nearest-even one
    return got


@pytest.mark.parametrize("D", [4, 6, 16, 128, 260])
def test_sr16_through_the_kernel(ops, D):
    _kernel_case(ops, D, seed=123, step=5)


def test_sr16_through_the_kernel_misaligned_rows(ops):
    """A table view 4 bytes off 8-byte alignment: the scalar-column store at D % 4 == 0."""
    a = _kernel_case(ops, 16, seed=9, step=2, misaligned=True)
    b = _kernel_case(ops, 16, seed=9, step=2)
    assert np.array_equal(a, b)  # the draw does not depend on the row's vector width


# ----------------------------------------------------------------- 2. invariance --
def _multi_hot_case(itype=torch.int32, otype=torch.int32):
    """T = 3, B = 40, bags of 0-3 lookups; table 1's bags all hold row 3 as well (a 40-lookup
    run: it crosses 16-lookup blocks and is finalised by the combine pass); per-sample weights;
    one index past its table."""
    g = torch.Generator().manual_seed(40)
    rows, B, D = [50, 7, 300], 40, 16
    T = len(rows)
    lo, li = [], []
    for t, n in enumerate(rows):
        lens = torch.randint(0, 4, (B,), generator=g)
        if t == 1:
            lens = lens + 1
        starts = torch.cumsum(lens, 0) - lens
        ii = torch.randint(0, n, (int(lens.sum()),), generator=g)
        if t == 1:
            ii[starts] = 3
        lo.append(starts)
        li.append(ii)
    li[2][5] = rows[2]  # out of range: skipped and flagged
    counts = [int(x.numel()) for x in li]
    # CSR over T * B bags: table t's bag b starts at sum(counts[:t]) + lo[t][b]
    off = torch.cat([lo[t].to(torch.int64) + sum(counts[:t]) for t in range(T)]
                    + [torch.tensor([sum(counts)], dtype=torch.int64)])
    idx = torch.cat(li)
    psw = torch.rand(idx.numel(), generator=g) + 0.5
    W16 = (torch.randn(sum(rows), D, generator=g) * 0.05).half()
    G = torch.randn(B, T, D, generator=g)
    row_base = torch.tensor([0] + np.cumsum(rows).tolist(), dtype=torch.int64)
    return dict(T=T, B=B, D=D, W16=W16.to(dev), G=G.to(dev), psw=psw.to(dev),
                idx=idx.to(itype).to(dev), off=off.to(otype).to(dev), row_base=row_base.to(dev),
                mx=max(counts), total=sum(rows))


def _sr_update(ops, c, W, st, lr, mx, flag=None, presort=False):
    kw = dict(per_sample_weights=c["psw"], max_lookups_per_table=mx, error_flag=flag)
    if presort:
        ws = torch.empty(ops.tbe_backward_workspace_size(c["idx"].numel(), c["total"], c["D"]),
                         dtype=torch.uint8, device=dev)
        ops.tbe_backward_sort(W, c["row_base"], c["T"], c["B"], c["idx"], c["off"], ws, mx,
                              per_sample_weights=c["psw"], error_flag=flag)
        kw.update(workspace=ws, presorted=ops.PRESORTED_ANY)
    ops.tbe_backward("sgd_f16", W, c["row_base"], c["T"], c["B"], c["idx"], c["off"], c["G"],
                     lr=lr, sr_state=st, **kw)


def _expected(ops, c, lr, seed, step, W16=None):
    """The fp32 update on the same half values, then the host's sr16 of every row (rows the
    batch does not touch are representable and come back unchanged)."""
    Wf = (c["W16"] if W16 is None else W16).float()
    ops.tbe_backward("sgd", Wf, c["row_base"], c["T"], c["B"], c["idx"], c["off"], c["G"], lr=lr,
                     per_sample_weights=c["psw"], max_lookups_per_table=c["mx"])
    torch.cuda.synchronize()
    return X.sr16_table(Wf.cpu().numpy(), seed, step)


def test_invariance_across_sort_block_width_and_rate(ops):
    seed, step, lr = 77, 3, 0.37
    c = _multi_hot_case()
    want = _hbits(_expected(ops, c, lr, seed, step))
    assert (want != _hbits(c["W16"])).any()
    st = ops.sr_state(seed, step, device=dev)
    lr_dev = torch.tensor([lr], dtype=torch.float32, device=dev)
    variants = []
    for it, ot in ((torch.int32, torch.int32), (torch.int64, torch.int64)):
        cc = _multi_hot_case(it, ot)
        for mx in (cc["mx"], 0):                 # per-table sort, device-wide sort
            for presort in (False, True):         # the sort run early
                for blk in (16, 64):              # DLRM_TUNE_TBE_BLOCK
                    for rate in (lr, lr_dev):     # host and device rate
                        variants.append((cc, mx, presort, blk, rate))
    assert c["mx"] <= 4096
    for cc, mx, presort, blk, rate in variants:
        W = cc["W16"].clone()
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        with ops.tuning(tbe_block=blk):
            _sr_update(ops, cc, W, st, rate, mx, flag=flag, presort=presort)
        torch.cuda.synchronize()
        what = (str(cc["idx"].dtype), mx, presort, blk, isinstance(rate, torch.Tensor))
        assert int(flag.item()) == ops.TBE_ERR_INDEX, what
        assert np.array_equal(_hbits(W), want), what


# ---------------------------------------------------------------------- 3. state --
def test_state_tick_and_graph_replay(ops):
    c = _multi_hot_case()
    lr, seed, s0 = 0.37, 5, (1 << 40) + 7
    st = ops.sr_state(seed, s0, device=dev)
    assert ops.sr_state_values(st) == (seed, s0)
    before = st.clone()
    Wa, Wb = c["W16"].clone(), c["W16"].clone()
    _sr_update(ops, c, Wa, st, lr, c["mx"])
    _sr_update(ops, c, Wb, st, lr, c["mx"])
    torch.cuda.synchronize()
    assert torch.equal(st, before)          # the update never writes the state
    assert _same(Wa, Wb)                    # the same state twice: the same bits
    assert np.array_equal(_hbits(Wa), _hbits(_expected(ops, c, lr, seed, s0)))
    for sd, sp in ((seed, s0 + 1), (seed + 1, s0), ((1 << 64) - 1, 0)):
        Wc = c["W16"].clone()
        _sr_update(ops, c, Wc, ops.sr_state(sd, sp, device=dev), lr, c["mx"])
        torch.cuda.synchronize()
        assert not _same(Wc, Wa)
        assert np.array_equal(_hbits(Wc), _hbits(_expected(ops, c, lr, sd, sp))), (sd, sp)
    ops.sr_tick(st)
    assert ops.sr_state_values(st) == (seed, s0 + 1)
    wrap = ops.sr_state(3, (1 << 64) - 1, device=dev)
    ops.sr_tick(wrap)
    assert ops.sr_state_values(wrap) == (3, 0)  # uint64 arithmetic wraps
    with pytest.raises(ValueError):
        ops.tbe_backward("sgd", c["W16"].float(), c["row_base"], c["T"], c["B"], c["idx"],
                         c["off"], c["G"], lr=lr, sr_state=st)
    with pytest.raises(ValueError):
        ops.sr_tick(torch.zeros(2, dtype=torch.int32, device=dev))

    # a captured {update, tick}, replayed three times on restored tables = three eager calls
    st.copy_(ops.sr_state(seed, s0, device=dev))
    W = c["W16"].clone()
    ws = torch.empty(ops.tbe_backward_workspace_size(c["idx"].numel(), c["total"], c["D"]),
                     dtype=torch.uint8, device=dev)

    def body():
        ops.tbe_backward("sgd_f16", W, c["row_base"], c["T"], c["B"], c["idx"], c["off"], c["G"],
                         lr=lr, sr_state=st, per_sample_weights=c["psw"],
                         max_lookups_per_table=c["mx"], workspace=ws)
        ops.sr_tick(st)

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        body()  # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    st.copy_(ops.sr_state(seed, s0, device=dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        body()
    for k in range(3):
        W.copy_(c["W16"])
        graph.replay()
        torch.cuda.synchronize()
        assert ops.sr_state_values(st) == (seed, s0 + k + 1)
        assert np.array_equal(_hbits(W), _hbits(_expected(ops, c, lr, seed, s0 + k))), k


# ------------------------------------------------------------- trainers (4, 5) --------
MODEL = dict(D=16, rows=[30, 1000, 257, 64], bot=[13, 32, 16], top=[64, 32, 1], B=48)
POLICY = dict(lr_num_warmup_steps=2, lr_decay_start_step=3, lr_num_decay_steps=2)
SEED = 2024


def _cfg(emb_lr=0.3, **kw):
    from dlrm_hip.trainer import TrainerConfig
    m = MODEL
    F = len(m["rows"]) + 1
    return TrainerConfig(m_spa=m["D"], ln_emb=m["rows"], ln_bot=m["bot"],
                         ln_top=[m["D"] + F * (F - 1) // 2] + m["top"], loss_function="bce",
                         learning_rate=0.1, emb_learning_rate=emb_lr, **kw)


def _trainers(fuse_gather=True, rounding="stochastic", tables=None, emb_lr=0.3, **kw):
    """A: fp16 tables.  S (the shadow): fp32 tables holding A's values, same dense bucket."""
    from dlrm_hip.trainer import DLRMTrainer
    sr = dict(emb_rounding=rounding, emb_rounding_seed=SEED) if rounding else {}
    A = DLRMTrainer(_cfg(emb_lr, emb_precision="fp16", **sr, **kw), device=dev, seed=3)
    S = DLRMTrainer(_cfg(emb_lr, **kw), device=dev, seed=3)
    if tables is not None:
        A.weights.copy_(tables)
    S.weights.copy_(A.weights.float())
    S.params.copy_(A.params)
    A.fuse_gather = S.fuse_gather = fuse_gather
    return A, S


def _sr_shadow(S, seed, step):
    """§18's shadow, with the host's stochastic rounding of the step in place of .half():
    sr16 of the whole table - untouched rows are representable and come back unchanged, so
    this is exactly 'round the touched rows'."""
    h = X.sr16_table(S.weights.cpu().numpy(), seed, step)
    S.weights.copy_(torch.from_numpy(h.astype(np.float32)))
    return h


def _assert_step(A, S, h, pa, la, ps, ls, what):
    assert _same(la, ls), f"{what}: loss {la.item()} vs {ls.item()}"
    assert _same(pa, ps), what
    for i, (a, s) in enumerate(zip(A.layers, S.layers)):
        assert _same(a.W, s.W), f"{what}: layer {i}"
    assert np.array_equal(_hbits(A.weights), _hbits(h)), f"{what}: tables"


SHADOW_CASES = [
    # gather-fused, graph replay, mlp_precision, device rates with a schedule
    (True, False, "fp32", False),
    (True, True, "fp32", False),
    (False, False, "fp32", False),
    (False, True, "fp32", False),
    (True, True, "bf16", False),
    (False, True, "fp32", True),
]


@pytest.mark.parametrize("gather,graph,mlp,dev_lr", SHADOW_CASES)
def test_shadow_trajectory(gather, graph, mlp, dev_lr):
    """Four steps over two alternating one-hot batches: loss, probabilities, every dense
    parameter and every table bit-equal to the fp32 shadow after every step."""
    kw = dict(mlp_precision=mlp, **(POLICY if dev_lr else {}))
    A, S = _trainers(fuse_gather=gather, **kw)
    assert A.rounding_state() == (SEED, 0)
    B = MODEL["B"]
    batches = [A.synthetic_batch(B, 1, seed=s) for s in (11, 12)]
    W0 = A.weights.clone()
    run_a = None
    if graph:  # one eager step for the allocations, then every state put back
        from dlrm_hip.trainer import Batch
        b0 = batches[0]
        fixed = Batch(*(t.clone() for t in (b0.X, b0.offsets, b0.indices, b0.target)),
                      b0.max_per_table, b0.one_hot)
        P0 = A.params.clone()
        A.step(fixed)
        assert A.rounding_state() == (SEED, 1)
        A.weights.copy_(W0)
        A.params.copy_(P0)
        A.set_rounding_state(SEED, 0)
        if dev_lr:
            A.lr_step = 1
        run_a = A.capture(fixed)
        assert A.rounding_state() == (SEED, 0)  # capturing runs nothing
    snap = None
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
        h = _sr_shadow(S, SEED, i)
        assert A.gather_fused == S.gather_fused == gather
        _assert_step(A, S, h, pa, la, ps, ls, f"step {i + 1}")
        if dev_lr:
            assert A.current_lr() == S.current_lr()
        if i == 1:
            snap = (A.weights.clone(), A.params.clone())
    assert A.rounding_state() == (SEED, 4)
    assert (A.weights.view(torch.int16) != W0.view(torch.int16)).any()
    A.predict(batches[0])  # forward only: never ticks
    assert A.rounding_state() == (SEED, 4)
    A.check_errors()
    if not graph and not dev_lr:  # a resume from (tables, dense, (seed, step)) reproduces the tail
        R, _ = _trainers(fuse_gather=gather, **kw)
        R.weights.copy_(snap[0])
        R.params.copy_(snap[1])
        R.set_rounding_state(SEED, 2)
        for i in (2, 3):
            R.step(batches[i % 2])
        assert R.rounding_state() == (SEED, 4)
        assert _same(R.weights, A.weights) and _same(R.params, A.params)


def _ulp16(w):
    """The fp16 spacing at |w| (fp64 array)."""
    a = np.abs(w.astype(np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return np.ldexp(1.0, (np.maximum(e, -14) - 10).astype(np.int64))


def test_small_updates_survive_only_with_stochastic_rounding():
    """Tables in one binade (|w| in [2^-5, 2^-4), ulp 2^-15) and an embedding rate at which the
    fp32 shadow's every table change of the first three steps is below a quarter ulp of its
    weight - asserted, so the premise cannot rot.  Nearest rounding then keeps the tables
    bit-identical to their init; stochastic rounding does not, and gives the shadow's tables."""
    steps, B = 3, MODEL["B"]
    g = torch.Generator().manual_seed(8)
    total = sum(MODEL["rows"])
    tables = ((torch.rand(total, MODEL["D"], generator=g) + 1.0) * 2.0 ** -5
              * (torch.randint(0, 2, (total, MODEL["D"]), generator=g) * 2 - 1)).half().to(dev)
    w0 = tables.float().cpu().numpy()
    assert (np.abs(w0) >= 2.0 ** -5).all() and (np.abs(w0) <= 2.0 ** -4).all()

    def fp32_changes(emb_lr):
        """max over elements and steps of |change| / ulp16(weight), on a plain fp32 trainer."""
        _, S = _trainers(rounding=None, tables=tables, emb_lr=emb_lr)
        worst = 0.0
        for i in range(steps):
            before = S.weights.cpu().numpy()
            S.step(batches[i % 2])
            worst = max(worst, float(np.max(np.abs(S.weights.cpu().numpy().astype(np.float64)
                                                   - before) / _ulp16(before))))
        return worst

    A0, _ = _trainers(rounding=None, tables=tables)
    batches = [A0.synthetic_batch(B, 1, seed=s) for s in (11, 12)]
    # the rate: a probe's largest change, scaled to 0.2 ulp (the changes are linear in the
    # rate up to the tables' own tiny movement); the premise itself is asserted below
    probe = fp32_changes(1e-4)
    assert probe > 0
    emb_lr = 1e-4 * 0.2 / probe
    worst = fp32_changes(emb_lr)
    print(f"emb_lr {emb_lr:.3e}: largest fp32 change {worst:.4f} ulp16")
    assert 0.1 < worst < 0.25

    N, _ = _trainers(rounding="nearest", tables=tables, emb_lr=emb_lr)
    A, S = _trainers(rounding="stochastic", tables=tables, emb_lr=emb_lr)
    for i in range(steps):
        b = batches[i % 2]
        N.step(b)
        pa, la = A.step(b)
        ps, ls = S.step(b)
        h = _sr_shadow(S, SEED, i)
        _assert_step(A, S, h, pa, la, ps, ls, f"step {i + 1}")
    assert _same(N.weights, tables)          # every update vanished
    moved = int((A.weights.view(torch.int16) != tables.view(torch.int16)).sum())
    print(f"stochastic rounding moved {moved} table elements")
    assert moved > 0


# ------------------------------------------------------- 6. module path, refusals --
def test_module_stochastic_rounding(ops):
    from dlrm_hip.modules import SplitTableBatchedEmbeddingBags
    c = _multi_hot_case()
    rows = np.diff(c["row_base"].cpu().numpy()).tolist()
    specs = [(n, c["D"]) for n in rows]
    tabs = [c["W16"][a:b].float().cpu() for a, b in zip(np.cumsum([0] + rows[:-1]),
                                                        np.cumsum(rows))]
    lr, seed = 0.25, 31
    idx = c["idx"].clone()
    idx[idx >= 300] = 0  # the module raises on a bad index: keep them in range here
    cc = dict(c, idx=idx, psw=None)
    M = SplitTableBatchedEmbeddingBags(specs, learning_rate=lr, tables=tabs, seed=seed,
                                       device=dev, stochastic_rounding=True)
    N0 = SplitTableBatchedEmbeddingBags(specs, learning_rate=lr, tables=tabs, seed=seed,
                                        device=dev, stochastic_rounding=False)
    N1 = SplitTableBatchedEmbeddingBags(specs, learning_rate=lr, tables=tabs, seed=seed,
                                        device=dev)
    assert "sr_state" in M.state_dict() and "sr_state" not in N0.state_dict()
    assert ops.sr_state_values(M.sr_state) == (seed, 0)
    G = c["G"].reshape(c["B"], -1)
    Wref = M.weights.data.clone()
    for step in range(2):
        for m in (M, N0, N1):
            m(idx, c["off"]).backward(G)
        want = _expected(ops, cc, lr, seed, step, W16=Wref)
        assert np.array_equal(_hbits(M.weights.data), _hbits(want)), step
        Wref = torch.from_numpy(want.copy()).to(dev)
        assert ops.sr_state_values(M.sr_state) == (seed, step + 1)
    assert _same(N0.weights.data, N1.weights.data)  # False is today's call
    Wn = c["W16"].clone()
    for _ in range(2):
        ops.tbe_backward("sgd", Wn, c["row_base"], c["T"], c["B"], idx, c["off"], c["G"], lr=lr)
    assert _same(N0.weights.data, Wn)
    assert not _same(M.weights.data, Wn)


def test_dlrm_net_passes_the_keyword_through():
    from dlrm_hip.dlrm_net import DLRM_Net
    kw = dict(m_spa=16, ln_emb=np.array([40, 30]), ln_bot=np.array([13, 16]),
              ln_top=np.array([19, 8, 1]), arch_interaction_op="dot", sigmoid_top=1,
              fbgemm_emb=True)
    assert not DLRM_Net(**kw).emb_l.stochastic_rounding
    assert DLRM_Net(**kw, fbgemm_stochastic_rounding=True).emb_l.stochastic_rounding


def test_refusals():
    from dlrm_hip.trainer import DLRMTrainer
    with pytest.raises(ValueError):
        _cfg(emb_rounding="stochastic")                      # fp32 tables
    with pytest.raises(ValueError):
        _cfg(emb_precision="fp16", emb_rounding="up")        # any other string
    T = DLRMTrainer(_cfg(emb_precision="fp16"), device=dev, seed=0)  # "nearest": no state
    with pytest.raises(RuntimeError):
        T.rounding_state()
    with pytest.raises(NotImplementedError):                 # the fp16 mode's refusals stay
        _cfg(emb_precision="fp16", emb_rounding="stochastic", optimizer="rwsadagrad")
