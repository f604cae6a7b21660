"""ops.interact_forward_pool and DLRMTrainer.fuse_pool (ABI v20) against plain
fp64 torch on the CPU.  Exact cases: every pooled sum and dot product is representable in fp32
(integers in [-8, 8] or 0.5 q + bias, bags <= 9, D <= 128: below 2^24 quarter units), so the
kernel must equal fp64 bit for bit.  Full mantissa: the pooled features bitwise the lookup
kernels', R within 1.01 (4 Lmax + D + 2) 2^-24 sum_k A_ik A_jk of fp64, A the pool of absolute
values: two roundings per lookup per operand and D for the Gram chain."""
import numpy as np
import pytest
import torch

import exact_rowsq as Q

pytestmark = pytest.mark.gpu
dev = "cuda:0"
LENS = torch.tensor([0, 1, 2, 5, 9])
FMTS = ["f32", "f16", "q8", "q4"]


def _fmt(fmt):
    from dlrm_hip import ops
    return ops, FMTS.index(fmt)  # ROWS_F32, ROWS_F16, ROWS_Q8, ROWS_Q4 = 0, 1, 2, 3


def _exact_rows(fmt, rows, D, g):
    """(rows as the kernel reads them, their values in fp64) for the exact cases."""
    if fmt in ("f32", "f16"):
        w = torch.randint(-8, 9, (rows, D), generator=g).float()
        return (w if fmt == "f32" else w.half()), w.double()
    if fmt == "q8":  # D levels <= 32, fp32 scale 0.5, fp32 bias -8
        q = torch.randint(0, 33, (rows, D), generator=g, dtype=torch.uint8)
        lv, bias, tail = q, -8.0, torch.tensor([0.5, -8.0]).view(torch.uint8)
    else:  # element 2i in the low nibble of byte i, fp16 scale 0.5, fp16 bias -4
        q = torch.randint(0, 16, (rows, D), generator=g, dtype=torch.uint8)
        lv, bias = q[:, 0::2] | (q[:, 1::2] << 4), -4.0
        tail = torch.tensor([0.5, -4.0], dtype=torch.float16).view(torch.uint8)
    return torch.cat([lv, tail.expand(rows, -1)], 1).contiguous(), 0.5 * q.double() + bias


def _case(fmt, D, F, B, seed):
    """x, rows, fp64 values, row_base and a table-batched CSR whose bag lengths cycle through
    LENS (every length in every wave of F >= 6)."""
    g = torch.Generator().manual_seed(seed)
    T = F - 1
    nrows = torch.arange(T) % 7 + 3
    row_base = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(nrows, 0)])
    rows, vals = _exact_rows(fmt, int(row_base[-1]), D, g)
    x = torch.randint(-8, 9, (B, D), generator=g).float()
    lens = LENS[(torch.arange(T * B) * 3 + seed) % 5]
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(lens, 0)])
    tab = torch.repeat_interleave(torch.arange(T * B) // B, lens)
    idx = (torch.rand(int(off[-1]), generator=g) * nrows[tab]).long()
    return x, rows, vals, row_base, idx.int(), off.int()


def _reference(x, vals, row_base, idx, off, self_i):
    """fp64: (R, pooled [B, T, D], sum_k A_ik A_jk per pair); an index outside its table is
    dropped."""
    (B, D), T = x.shape, row_base.numel() - 1
    pooled = torch.zeros(B, T, D, dtype=torch.float64)
    apool = torch.zeros_like(pooled)
    for t in range(T):
        for b in range(B):
            r = idx[off[t * B + b]:off[t * B + b + 1]].long()
            r = r[(r >= 0) & (r < row_base[t + 1] - row_base[t])] + row_base[t]
            pooled[b, t], apool[b, t] = vals[r].sum(0), vals[r].abs().sum(0)
    li, lj = torch.tril_indices(T + 1, T + 1, 0 if self_i else -1)
    Tm = torch.cat([x.double()[:, None], pooled], 1)
    Am = torch.cat([x.double().abs()[:, None], apool], 1)
    R = torch.cat([x.double(), (Tm @ Tm.transpose(1, 2))[:, li, lj]], 1)
    return R, pooled, (Am @ Am.transpose(1, 2))[:, li, lj]


def _run(fmt, D, x, rows, row_base, idx, off, **kw):
    ops, f = _fmt(fmt)
    return ops.interact_forward_pool(x.to(dev), rows.to(dev), f, D, row_base.to(dev),
                                     idx.to(dev), off.to(dev), **kw)


@pytest.mark.parametrize("self_i,B,keep", [(0, 5, True), (1, 5, False), (1, 1, True)])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("F", [2, 27, 32])
@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_exact(D, F, fmt, self_i, B, keep):
    x, rows, vals, row_base, idx, off = _case(fmt, D, F, B, seed=D + F + B)
    want, pooled, _ = _reference(x, vals, row_base, idx, off, self_i)
    keep_t = torch.full((B, F - 1, D), 7.0, device=dev) if keep else None
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    got = _run(fmt, D, x, rows, row_base, idx, off, self_interaction=bool(self_i),
               pooled_out=keep_t, error_flag=err)
    assert torch.equal(got.cpu().double(), want) and int(err) == 0
    assert not keep or torch.equal(keep_t.cpu().double(), pooled)


@pytest.mark.parametrize("fmt", FMTS)
def test_full_mantissa(fmt):
    D, F, B = 128, 27, 5
    ops, f = _fmt(fmt)
    _, _, _, row_base, idx, off = _case("f32", D, F, B, seed=5)
    g = torch.Generator().manual_seed(9)
    W, x = torch.randn(int(row_base[-1]), D, generator=g).to(dev), torch.randn(B, D, generator=g)
    csr = (row_base.to(dev), F - 1, B, idx.to(dev), off.to(dev))
    if fmt == "f32":
        rows, vals, look = W, W.cpu().double(), ops.tbe_forward(W, *csr)
    elif fmt == "f16":
        rows, vals = W.half(), W.half().cpu().double()
    else:
        rows = ops.rows_quantize(W, 8 if fmt == "q8" else 4)
        q, scale, bias = Q.decode(rows.cpu().numpy(), 8 if fmt == "q8" else 4, D)
        vals = torch.from_numpy(scale.astype(np.float64)[:, None] * q + bias[:, None])
    if fmt != "f32":
        look = ops.tbe_forward_rows(rows, f, D, *csr)
    keep = torch.empty(B, F - 1, D, device=dev)
    got = _run(fmt, D, x, rows, row_base, idx, off, pooled_out=keep).cpu()
    assert torch.equal(keep.view(torch.int32), look.view(torch.int32))
    want, _, AA = _reference(x, vals, row_base, idx, off, 0)
    e, unit = (got.double() - want).abs()[:, D:], 2.0 ** -24 * AA  # (an empty bag: 0 <= 0)
    print("max err in units of 2^-24 sum_k A_ik A_jk:", float((e / unit)[AA > 0].max()))
    assert torch.equal(got[:, :D], x) and bool((e <= 1.01 * (4 * 9 + D + 2) * unit).all())


@pytest.mark.parametrize("fmt", ["f32", "q4"])
def test_bad_index_and_scalar_stores(fmt):
    """A dropped, flagged index; an output pitch that is no multiple of 4 (scalar stores)."""
    D, F, B = 32, 27, 5
    x, rows, vals, row_base, idx, off = _case(fmt, D, F, B, seed=3)
    assert off[7 * B + 3] > off[7 * B + 2]
    idx[int(off[7 * B + 2])] = 1000  # the first index of bag (7, 2)
    want, _, _ = _reference(x, vals, row_base, idx, off, 0)
    width = want.shape[1]  # 32 + 351
    out = torch.full((B, width + 2), -1.0, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _run(fmt, D, x, rows, row_base, idx, off, out=out, error_flag=err)
    assert out.stride(0) % 4 and torch.equal(out[:, :width].cpu().double(), want)
    assert bool((out[:, width:] == -1.0).all()) and int(err) == 1


def test_empty_batch():
    got = _run("f32", 16, torch.zeros(0, 16), torch.zeros(4, 16), torch.tensor([0, 4]),
               torch.zeros(0, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    assert tuple(got.shape) == (0, 17)


# ------------------------------------------------------------------------- engine --
ROWS, BOT, B_ENG = [30, 200, 17], [13, 32, 16], 5


def _trainer(op="dot", **kw):
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    D, F = 16, len(ROWS) + 1
    cfg = TrainerConfig(m_spa=D, ln_emb=ROWS, ln_bot=BOT, loss_function="bce",
                        ln_top=[D * F if op == "cat" else D + F * (F - 1) // 2, 32, 1],
                        learning_rate=0.1, emb_learning_rate=0.3, arch_interaction_op=op, **kw)
    tr = DLRMTrainer(cfg, device=dev, seed=3)
    g = torch.Generator().manual_seed(17)
    lens = [LENS[(torch.arange(B_ENG) * 3 + t) % 5] for t in range(len(ROWS))]
    multi_hot = tr.make_batch(
        torch.rand(B_ENG, BOT[0], generator=g), [torch.cumsum(n, 0) - n for n in lens],
        [torch.randint(0, r, (int(n.sum()),), generator=g) for r, n in zip(ROWS, lens)],
        torch.rand(B_ENG, generator=g).round())
    return tr, multi_hot


@pytest.mark.parametrize("emb", ["fp32", "fp16"])
def test_engine_bitwise(emb):
    """fuse_pool on against off (D = 16: both run the LDS-staged Gram, so equality holds)."""
    (A, batch_a), (T, batch_t) = _trainer(emb_precision=emb), _trainer(emb_precision=emb)
    A.fuse_pool = True
    prob = A._predict_bufs(A._buffers(B_ENG, B_ENG))["prob"]
    for bits in (32, 8, 4):
        if bits != 32:
            A.quantize_embedding(bits), T.quantize_embedding(bits)
        want = T.predict(batch_t, emb_bits=bits).clone()
        assert torch.equal(A.predict(batch_a, emb_bits=bits), want), bits
        run = A.capture_predict(batch_a, emb_bits=bits)
        prob.zero_()
        run()
        assert torch.equal(prob, want), bits
    pa, la = A.step(batch_a)
    pt, lt = T.step(batch_t)
    assert A.pool_fused and not T.pool_fused
    assert torch.equal(pa, pt) and torch.equal(la, lt) and torch.equal(A.params, T.params)
    assert torch.equal(A.weights.view(torch.int16), T.weights.view(torch.int16))
    A.check_errors()


@pytest.mark.parametrize("what", ["one_hot", "qr", "cat"])
def test_engine_keeps_two_launches(what):
    kw = dict(qr_flag=True, qr_threshold=100) if what == "qr" else {}
    tr, multi_hot = _trainer("cat" if what == "cat" else "dot", **kw)
    tr.fuse_pool = True
    tr.step(tr.synthetic_batch(B_ENG, 1, seed=4) if what == "one_hot" else multi_hot)
    assert not tr.pool_fused
    tr.check_errors()
