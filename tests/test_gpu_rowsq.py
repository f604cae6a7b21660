"""int8 / int4 embedding tables in the fused engine (ABI v17): the device
row-wise quantizer, the gather-fused interaction forward on Q8 / Q4 rows, and
DLRMTrainer.quantize_embedding / predict(emb_bits=).

Every comparison is BITWISE.  The quantizer is compared with the host restatement of the rule
(tests/exact_rowsq.pack_rows, itself bitwise torch's packers: tests/test_exact_rowsq_cpu.py);
the gather kernel and the engine with the existing fp32 path on the exactly dequantised
table (fma(scale, q, bias), one rounding).  Shapes as in tests/test_gpu_emb16.py: (B, D) cross
one workgroup (B = 5), a ragged last workgroup (70) and kV5MaxBatch (1028)."""
import numpy as np
import pytest
import torch

import exact_rowsq as Q

pytestmark = pytest.mark.gpu
dev = "cuda:0"
V5_MAX_BATCH = 1024  # interact.hip kV5MaxBatch
BITS = [8, 4]


@pytest.fixture(scope="module")
def ops():
    from dlrm_hip import ops as _ops
    return _ops


def _fmt(ops, bits):
    return ops.ROWS_Q4 if bits == 4 else ops.ROWS_Q8


def _ibits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_ibits(a), _ibits(b))


def _dequant_t(packed, bits, D):
    """Exact host dequantisation of a device packed buffer -> fp32 device tensor."""
    return torch.from_numpy(Q.dequant(packed.cpu().numpy(), bits, D)).to(dev)


# ------------------------------------------------------------------- 1. quantizer --
QUANT_DIMS = [4, 16, 20, 64, 128, 200, 512]


def _quantize_guarded(ops, src, bits):
    """rows_quantize into the middle of a sentinel-filled byte buffer; the bytes before and
    after the output must keep their bits.  The output starts 16-byte aligned."""
    rows, D = src.shape
    n = rows * Q.row_bytes(bits, D)
    guard = 64
    buf = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device=dev)
    out = buf[guard:guard + n].view(rows, Q.row_bytes(bits, D))
    got = ops.rows_quantize(src, bits, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + n:] == 0xA5).all())
    return out.clone()


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("D", QUANT_DIMS)
def test_rows_quantize_is_pack_rows(ops, D, bits):
    gen = np.random.default_rng(77 * D + bits)
    fam = Q.families(300, D, gen, bits)
    w = np.concatenate(list(fam.values()))
    w = w[gen.permutation(w.shape[0])]  # the families interleaved inside every wave
    for rows in (1, 3, 67, 1031, w.shape[0]):
        src = np.ascontiguousarray(w[:rows])
        got = _quantize_guarded(ops, torch.from_numpy(src).to(dev), bits).cpu().numpy()
        want = Q.pack_rows(src, bits)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, ("fp32", rows, bad.size, bad[:5])
        # + 0: a tiny negative entry rounds to -0 in fp16; a row whose minimum is then both
        # -0 and +0 has no defined sign of the stored bias, so zeros are made +0
        h = torch.from_numpy(src).half() + 0
        got = _quantize_guarded(ops, h.to(dev), bits).cpu().numpy()
        want = Q.pack_rows(h.float().numpy(), bits)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, ("fp16", rows, bad.size, bad[:5])


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("D", QUANT_DIMS)
def test_quantize_then_lookup_round_trip(ops, D, bits):
    """dlrm_tbe_forward_rows of one lookup per row on the packed rows == dequant."""
    gen = np.random.default_rng(D + bits)
    rows = 67
    w = Q.families(rows, D, gen, bits)["normal"]
    packed = ops.rows_quantize(torch.from_numpy(w).to(dev), bits)
    row_base = torch.tensor([0, rows], dtype=torch.int64, device=dev)
    idx = torch.arange(rows, dtype=torch.int32, device=dev)
    off = torch.arange(rows + 1, dtype=torch.int32, device=dev)
    out = ops.tbe_forward_rows(packed, _fmt(ops, bits), D, row_base, 1, rows, idx, off)
    assert _same(out.view(rows, D), _dequant_t(packed, bits, D))


def test_rows_quantize_empty_and_errors(ops):
    out = ops.rows_quantize(torch.zeros(0, 16, device=dev), 8)
    assert tuple(out.shape) == (0, 24)
    w = torch.zeros(3, 16, device=dev)
    with pytest.raises(ValueError):
        ops.rows_quantize(w, 16)
    with pytest.raises(ValueError):
        ops.rows_quantize(w.double(), 8)
    with pytest.raises(ValueError):
        ops.rows_quantize(w, 8, out=torch.zeros(3, 25, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        ops.rows_quantize(w, 8, out=torch.zeros(3, 24, dtype=torch.int8, device=dev))
    from dlrm_hip._lib import DLRMHipError
    with pytest.raises(DLRMHipError, match="UNSUPPORTED"):
        ops.rows_quantize(torch.zeros(2, 516, device=dev), 8)


# ------------------------------------------------------------------ 2. gather kernel --
GATHER_SHAPES = [(5, 16), (5, 32), (70, 64), (70, 128), (1028, 64), (1028, 128)]
GATHER_F = [(2, False), (9, True), (27, False), (32, False)]


def _fwd_version(D, B, t):
    """interact.hip fwd_version: the forward kernel DLRM_TUNE_INTERACT_FWD = t selects."""
    if t == 4:
        return 4
    if t == 5:
        return 5 if D >= 64 else 4
    return 5 if D >= 64 and B <= V5_MAX_BATCH else 4


def test_gather_cases_reach_every_variant():
    fwd = {_fwd_version(D, B, t) for B, D in GATHER_SHAPES for t in (0, 4, 5)}
    assert fwd == {4, 5}
    assert {_fwd_version(D, B, 0) for B, D in GATHER_SHAPES} == {4, 5}


def _gather_case(ops, B, D, F, bits, seed, bad=False):
    """T = F - 1 tiny tables (<= 50 rows, the second-to-last of 1 row), packed by
    rows_quantize from random fp32 rows; every row that no index names is 0xFF bytes (NaN
    scale and bias in both widths); indices with duplicates, the first two samples sharing
    their rows; strided x.  ``bad``: one index one past its table.  Returns the packed table
    and its exact fp32 dequantisation (NaN rows where unnamed)."""
    g = torch.Generator().manual_seed(seed)
    T = F - 1
    rows = [int(r) for r in torch.randint(2, 51, (T,), generator=g)]
    rows[max(T - 2, 0)] = 1
    base = [0] + np.cumsum(rows).tolist()
    idx = torch.stack([torch.randint(0, n, (B,), generator=g) for n in rows])  # [T, B]
    if B > 1:
        idx[:, 1] = idx[:, 0]
    W = (torch.randn(base[-1], D, generator=g) * 0.5).to(dev)
    packed = ops.rows_quantize(W, bits)
    named = torch.zeros(base[-1], dtype=torch.bool)
    named[torch.cat([base[t] + idx[t] for t in range(T)])] = True
    packed[~named.to(dev)] = 0xFF
    Wd = _dequant_t(packed, bits, D)
    assert bool(torch.isfinite(Wd[named.to(dev)]).all())
    assert named.all() or bool(Wd[~named.to(dev)].isnan().all())
    if bad:
        t = T // 2
        idx[t, B // 2] = rows[t]  # one past the table's last row: the next table's first
    x = torch.randn(B, D + 4, generator=g).to(dev)[:, :D]
    row_base = torch.tensor(base, dtype=torch.int64, device=dev)
    return x, packed, Wd, row_base, idx.reshape(-1).to(torch.int32).to(dev)


def _run(ops, x, table, row_base, idx, self_int, fwd_t, fmt=None, flag=None):
    """One gather forward into a guarded output (fmt None: the fp32 kernel on ``table``)."""
    B, D = x.shape
    F = row_base.numel()
    width = D + (F * (F + 1) // 2 if self_int else F * (F - 1) // 2)
    ld = (width + 3) // 4 * 4 + 4  # 16-byte aligned rows and pad columns
    buf = torch.full((B + 2, ld), -77.0, dtype=torch.float32, device=dev)
    out = buf[1:B + 1, :width]
    with ops.tuning(interact_fwd=fwd_t):
        if fmt is None:
            ops.interact_forward_gather(x, table, row_base, idx, self_int, out=out,
                                        error_flag=flag)
        else:
            ops.interact_forward_gather_rows(x, table, fmt, D, row_base, idx, self_int,
                                             out=out, error_flag=flag)
    torch.cuda.synchronize()
    guard = torch.full_like(buf, -77.0)
    assert _same(buf[0], guard[0]) and _same(buf[-1], guard[-1])
    assert _same(buf[:, width:], guard[:, width:])
    return out.clone()


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("F,self_int", GATHER_F)
@pytest.mark.parametrize("B,D", GATHER_SHAPES)
def test_gather_rows_is_the_fp32_gather_on_the_dequantised_table(ops, B, D, F, self_int, bits):
    x, packed, Wd, row_base, idx = _gather_case(ops, B, D, F, bits, seed=B * 1000 + D * 10 + F)
    for fwd_t in (0, 4, 5):
        got = _run(ops, x, packed, row_base, idx, self_int, fwd_t, fmt=_fmt(ops, bits))
        want = _run(ops, x, Wd, row_base, idx, self_int, fwd_t)
        assert torch.isfinite(want).all(), fwd_t  # no unnamed (NaN) row was read
        assert _same(got, want), fwd_t


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("B,D", [(70, 64), (5, 16), (1028, 128)])
def test_gather_rows_out_of_range_index(ops, B, D, bits):
    """One index one past its table: flagged, the row reads as zeros, as in the fp32 kernel
    (whose result on the dequantised table is the reference).  The index is checked before
    any row is addressed: nothing is read out of bounds."""
    F = 9
    x, packed, Wd, row_base, idx = _gather_case(ops, B, D, F, bits, seed=D + B, bad=True)
    for fwd_t in (0, 4, 5):
        fq = torch.zeros(1, dtype=torch.int32, device=dev)
        f32 = torch.zeros(1, dtype=torch.int32, device=dev)
        got = _run(ops, x, packed, row_base, idx, False, fwd_t, fmt=_fmt(ops, bits), flag=fq)
        want = _run(ops, x, Wd, row_base, idx, False, fwd_t, flag=f32)
        assert int(fq.item()) == int(f32.item()) == ops.TBE_ERR_INDEX
        assert torch.isfinite(want).all() and _same(got, want)


def test_gather_rows_rejects_formats_pitches_and_alignment(ops):
    from dlrm_hip._lib import DLRMHipError
    x, packed, Wd, row_base, idx = _gather_case(ops, 5, 16, 3, 8, seed=1)
    for fmt in (ops.ROWS_F32, ops.ROWS_F16, 99):
        with pytest.raises(DLRMHipError, match="UNSUPPORTED"):
            ops.interact_forward_gather_rows(x, packed, fmt, 16, row_base, idx)
    with pytest.raises(DLRMHipError, match="INVALID_ARG"):  # a Q8 pitch read as Q4
        ops.interact_forward_gather_rows(x, packed, ops.ROWS_Q4, 16, row_base, idx)
    wide = torch.zeros(packed.shape[0], 32, dtype=torch.uint8, device=dev)
    with pytest.raises(DLRMHipError, match="INVALID_ARG"):
        ops.interact_forward_gather_rows(x, wide[:, :24], ops.ROWS_Q8, 16, row_base, idx)
    flat = torch.zeros(packed.numel() + 16, dtype=torch.uint8, device=dev)
    off = flat[8:8 + packed.numel()].view(packed.shape)  # 8-byte, not 16-byte aligned
    assert off.data_ptr() % 16 == 8
    with pytest.raises(DLRMHipError, match="INVALID_ARG"):
        ops.interact_forward_gather_rows(x, off, ops.ROWS_Q8, 16, row_base, idx)
    with pytest.raises(ValueError):
        ops.interact_forward_gather_rows(x, Wd, ops.ROWS_Q8, 16, row_base, idx)  # fp32 rows
    with pytest.raises(ValueError):
        ops.interact_forward_gather_rows(x, packed, ops.ROWS_Q8, 16, row_base, idx.long())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------ trainers --
MODELS = {
    "d16": dict(D=16, rows=[30, 200, 1, 64, 17], bot=[13, 32, 16], top=[32, 1], B=5),
    "d64": dict(D=64, rows=[200, 30, 150], bot=[13, 64, 32, 64], top=[48, 1], B=70),
}


def _cfg(model, **kw):
    from dlrm_hip.trainer import TrainerConfig
    m = MODELS[model]
    F = len(m["rows"]) + 1
    return TrainerConfig(m_spa=m["D"], ln_emb=m["rows"], ln_bot=m["bot"],
                         ln_top=[m["D"] + F * (F - 1) // 2] + m["top"], loss_function="bce",
                         learning_rate=0.1, emb_learning_rate=0.3, **kw)


def _trainer(model, seed=3, **kw):
    from dlrm_hip.trainer import DLRMTrainer
    return DLRMTrainer(_cfg(model, **kw), device=dev, seed=seed)


def _shadow(A, bits, S=None):
    """An fp32 trainer with A's dense parameters whose tables are the exact dequantisation
    of A's packed rows."""
    if S is None:
        from dlrm_hip.trainer import DLRMTrainer
        cfg = _cfg("d16" if A.D == 16 else "d64")
        S = DLRMTrainer(cfg, device=dev, seed=3)
        S.fuse_gather = A.fuse_gather
    S.params.copy_(A.params)
    S.weights.copy_(_dequant_t(A.quantized_rows(bits), bits, A.D))
    return S


def _prob(tr, B):
    return tr._predict_bufs(tr._buffers(B, B))["prob"]


@pytest.mark.parametrize("emb", ["fp32", "fp16"])
@pytest.mark.parametrize("gather", [True, False])
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("model", sorted(MODELS))
def test_engine_shadow(model, bits, gather, emb):
    from dlrm_hip import metrics
    A = _trainer(model, emb_precision=emb)
    A.fuse_gather = gather
    B = MODELS[model]["B"]
    batches = [A.synthetic_batch(B, 1, seed=s) for s in (21, 22)]
    assert A._gather_applies(batches[0]) == gather
    W0, P0 = A.weights.clone(), A.params.clone()
    packed = A.quantize_embedding(bits)
    assert packed.dtype == torch.uint8 and packed.data_ptr() == A.quantized_rows(bits).data_ptr()
    assert tuple(packed.shape) == (A.total_rows, Q.row_bytes(bits, A.D))
    want_rows = Q.pack_rows(A.weights.float().cpu().numpy(), bits)
    assert np.array_equal(packed.cpu().numpy(), want_rows)
    S = _shadow(A, bits)
    for dt in ("fp32", "bf16", "fp16"):
        want = S.predict(batches[0], precision=dt).clone()
        got = A.predict(batches[0], precision=dt, emb_bits=bits).clone()
        assert _same(got, want), dt
        run = A.capture_predict(batches[0], precision=dt, emb_bits=bits)
        A.predict(batches[1], precision=dt, emb_bits=bits)  # overwrite the output, then replay
        run()
        assert _same(_prob(A, B), want), dt
    sa, ss = metrics.EvalState(2 * B, dev), metrics.EvalState(2 * B, dev)
    ra = A.evaluate(batches, sa, emb_bits=bits)
    rs = S.evaluate(batches, ss)
    assert sa.count == ss.count == 2 * B and ra == rs
    assert _same(A.weights, W0) and _same(A.params, P0)  # forward only
    assert np.array_equal(A.quantized_rows(bits).cpu().numpy(), want_rows)
    A.check_errors()


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("model", sorted(MODELS))
def test_engine_multi_hot_on_exact_tables(model, bits):
    """Bags of 0-8 lookups on tables that quantise without error: every bag sum is exact in
    either formula, so predict(emb_bits=) is bit-equal to the same trainer's fp32 predict."""
    A = _trainer(model)
    gen = np.random.default_rng(bits)
    A.weights.copy_(torch.from_numpy(Q.exact_table(bits, A.total_rows, A.D, gen)))
    A.quantize_embedding(bits)
    assert _same(_dequant_t(A.quantized_rows(bits), bits, A.D), A.weights)
    m = MODELS[model]
    B = m["B"]
    g = torch.Generator().manual_seed(17)
    lS_o, lS_i = [], []
    for n in m["rows"]:
        lens = torch.randint(0, 9, (B,), generator=g)
        lens[0], lens[-1] = 0, 8
        lS_o.append(torch.cumsum(lens, 0) - lens)
        lS_i.append(torch.randint(0, n, (int(lens.sum()),), generator=g))
    X = torch.rand(B, m["bot"][0], generator=g)
    tg = torch.rand(B, generator=g).round()
    batch = A.make_batch(X, lS_o, lS_i, tg)
    assert not batch.one_hot and not A._gather_applies(batch)
    want = A.predict(batch).clone()
    got = A.predict(batch, emb_bits=bits).clone()
    assert _same(got, want)
    A.check_errors()


@pytest.mark.parametrize("bits", BITS)
def test_snapshot_and_repack(bits):
    A = _trainer("d64")
    T = _trainer("d64")  # the same trainer without a packed buffer
    B = MODELS["d64"]["B"]
    batch = A.synthetic_batch(B, 1, seed=31)
    A.quantize_embedding(bits)
    ptr = A.quantized_rows(bits).data_ptr()
    snap, W0 = A.quantized_rows(bits).clone(), A.weights.clone()
    S = _shadow(A, bits)
    p32 = A.predict(batch).clone()
    pq = A.predict(batch, emb_bits=bits).clone()
    assert _same(pq, S.predict(batch))
    run = A.capture_predict(batch, emb_bits=bits)
    # one training step: bit-equal with and without a packed buffer present
    pa, la = A.step(batch)
    pt, lt = T.step(batch)
    assert _same(pa, pt) and _same(la, lt)
    assert _same(A.weights, T.weights) and _same(A.params, T.params)
    # the step moved the masters, not the snapshot; only the dense parameters moved the scores
    assert not _same(A.predict(batch).clone(), p32)
    assert not _same(A.weights, W0) and _same(A.quantized_rows(bits), snap)
    S.params.copy_(A.params)
    want = S.predict(batch).clone()
    assert _same(A.predict(batch, emb_bits=bits), want)
    run()
    assert _same(_prob(A, B), want)
    # re-pack (of masters moved far enough to change every level): the same storage, so the
    # captured graph reads the new rows
    A.weights.mul_(-0.5)
    A.quantize_embedding(bits)
    assert A.quantized_rows(bits).data_ptr() == ptr
    _shadow(A, bits, S)
    want2 = S.predict(batch).clone()
    assert not _same(want2, want)
    A.predict(batch)  # overwrite the output
    run()
    assert _same(_prob(A, B), want2)
    A.check_errors()


def test_refusals_and_errors():
    from dlrm_hip.trainer import DLRMTrainer, EmulatedComm
    A = _trainer("d16")
    batch = A.synthetic_batch(5, 1, seed=1)
    for bits in (8, 4):
        with pytest.raises(RuntimeError):
            A.quantized_rows(bits)
        with pytest.raises(RuntimeError):
            A.predict(batch, emb_bits=bits)
    A.quantize_embedding(8)
    A.predict(batch, emb_bits=8)
    with pytest.raises(RuntimeError):  # one buffer per width
        A.capture_predict(batch, emb_bits=4)
    for bad in (0, 16, 2, "8"):
        with pytest.raises(ValueError):
            A.predict(batch, emb_bits=bad)
        with pytest.raises(ValueError):
            A.quantize_embedding(bad)
    from dlrm_hip import metrics
    with pytest.raises(ValueError):
        A.evaluate([batch], metrics.EvalState(5, dev), emb_bits=3)
    with pytest.raises(ValueError):
        A.predict_segments(batch, emb_bits=64)
    cfg = _cfg("d16", qr_flag=True, qr_threshold=50, qr_collisions=4)
    R = DLRMTrainer(cfg, device=dev, seed=3)
    D2 = DLRMTrainer(_cfg("d16"), device=dev, rank=0, world_size=2, comm=EmulatedComm())
    from dlrm_hip.trainer import TrainerConfig
    wide = TrainerConfig(m_spa=516, ln_emb=[10, 10], ln_bot=[13, 516], ln_top=[516 + 3, 1],
                         loss_function="bce")
    Wd = DLRMTrainer(wide, device=dev, seed=3)  # an embedding dim above 512
    for tr in (R, D2, Wd):
        with pytest.raises(NotImplementedError) as e:
            tr.quantize_embedding(8)
        assert "DESIGN.md §20" in str(e.value)
        with pytest.raises(NotImplementedError) as e:
            tr.predict_segments(batch, emb_bits=4)
        assert "DESIGN.md §20" in str(e.value)
