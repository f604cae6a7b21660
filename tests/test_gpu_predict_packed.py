"""DLRMTrainer.pack_mlp16 and predict / capture_predict / evaluate with mlp_store=16: bit for
bit the 16-bit ``precision`` path on the weights that were packed, the snapshot semantics, the
untouched default path and the refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda:0"
ROWS, D, B = [50, 30, 20], 16, 70
# 16-bit buffers after 13 -> 64 and 22 -> 64; 64 -> 36 reads one and leaves an fp32 buffer (36 is
# no multiple of 8); 64 -> 16 and 36 -> 32 feed the interaction and the head, in fp32
LN_BOT, LN_TOP = [13, 64, 16], [D + 4 * 3 // 2, 64, 36, 32, 1]


def _engine(L, seed=11):
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    cfg = TrainerConfig(m_spa=D, ln_emb=ROWS, ln_bot=LN_BOT, ln_top=LN_TOP,
                        loss_function="bce", learning_rate=0.5)
    tr = DLRMTrainer(cfg, device=dev, seed=seed)
    rng = np.random.RandomState(seed)
    X = np.log1p(rng.rand(B, LN_BOT[0]).astype(np.float32))
    lS_o = np.array([np.arange(B) * L for _ in ROWS], dtype=np.int64)
    lS_i = [rng.randint(0, n, size=B * L).astype(np.int64) for n in ROWS]
    T = np.round(rng.rand(B, 1).astype(np.float32))
    return tr, tr.make_batch(X, lS_o, lS_i, T)


def _same(a, b):
    return a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_bit_equal_snapshot_and_default(dt, L):
    tr, batch = _engine(L)
    kw = dict(precision=dt, mlp_store=16)
    p_default = tr.predict(batch).clone()
    want = tr.predict(batch, precision=dt).clone()
    tr.pack_mlp16(dt)
    assert _same(tr.predict(batch), p_default)  # the default path does not see the snapshot
    assert _same(tr.predict(batch, **kw), want)
    torch.cuda.synchronize()
    run = tr.capture_predict(batch, **kw)
    prob = tr._predict_bufs(tr._buffers(B, B))["prob"]
    for _ in range(2):
        prob.zero_()
        run()
        assert _same(prob, want)
    # one training step moves the fp32 masters; the packed layers stay until the re-pack
    below = tr.bot + tr.top[:-1]
    old = [lay.W.clone() for lay in below]
    ptrs = [s.packed.wp.data_ptr() for s in tr.packed_mlp16(dt).values()]
    tr.step(batch)
    new = [lay.W.clone() for lay in below]
    for lay, w in zip(below, old):
        lay.W.copy_(w)
    want_old = tr.predict(batch, precision=dt).clone()  # the old layers, today's tables and head
    for lay, w in zip(below, new):
        lay.W.copy_(w)
    want_new = tr.predict(batch, precision=dt).clone()
    assert not torch.equal(want_old, want_new)
    assert _same(tr.predict(batch, **kw), want_old)
    run()
    assert _same(prob, want_old)
    tr.pack_mlp16(dt)  # into the same storage: the captured graph reads the new values
    assert ptrs == [s.packed.wp.data_ptr() for s in tr.packed_mlp16(dt).values()]
    assert _same(tr.predict(batch, **kw), want_new)
    prob.zero_()
    run()
    assert _same(prob, want_new)


def test_refusals():
    from dlrm_hip import metrics
    tr, batch = _engine(1)
    st = metrics.EvalState(B, dev)
    calls = lambda **kw: (lambda: tr.predict(batch, **kw),
                          lambda: tr.predict_segments(batch, **kw),
                          lambda: tr.capture_predict(batch, **kw),
                          lambda: tr.evaluate([batch], st, **kw))
    for call in calls(precision="bf16", mlp_store=16):  # no snapshot yet
        with pytest.raises(RuntimeError, match="pack_mlp16"):
            call()
    with pytest.raises(ValueError, match="pack_mlp16"):
        tr.pack_mlp16("int8")
    tr.pack_mlp16("bf16")
    for call in calls(precision="fp16", mlp_store=16):  # a snapshot of the other dtype
        with pytest.raises(RuntimeError, match="pack_mlp16"):
            call()
    for kw in (dict(mlp_store=16), dict(precision="fp32", mlp_store=16),
               dict(precision="bf16", mlp_store=8), dict(precision="bf16", mlp_store="16")):
        for call in calls(**kw):
            with pytest.raises(ValueError):
                call()
    tr.quantize_mlp(8)
    for call in calls(precision="bf16", mlp_store=16, mlp_bits=8):
        with pytest.raises(ValueError):
            call()
    tr.distributed = True  # the multi-GPU schedule
    try:
        with pytest.raises(NotImplementedError, match="§27"):
            tr.pack_mlp16("bf16")
        with pytest.raises(NotImplementedError, match="§27"):
            tr.predict_segments(batch, precision="bf16", mlp_store=16)
    finally:
        tr.distributed = False
    assert tr.predict(batch, precision="bf16", mlp_store=16).shape == (B,)
