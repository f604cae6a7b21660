"""DLRMTrainer.quantize_mlp(8) and predict / capture_predict / evaluate with mlp_bits=8: the
whole pass reproduced from the rule of tests/exact_mlp8 on a model whose other stages only
copy, random weights against a CPU emulation, the snapshot semantics, the captured and the
evaluate paths, the promise that int8 predicts never touch training state, and the refusals."""
import numpy as np
import pytest
import torch

import eval_ref
import exact_mlp8 as E
import exact_rowsq as Q
import linear16_ref as R
import oracle as O
from test_gpu_predict16 import _bits_equal, _make, _rand_batch, _state, _u32

pytestmark = pytest.mark.gpu
dev = "cuda:0"
F32 = np.float32
FP32_ALLOWANCE = 1e-5  # as test_gpu_predict16


def _linears(seq):
    return [(m.weight.detach().numpy().astype(F32), m.bias.detach().numpy().astype(F32))
            for m in seq if isinstance(m, torch.nn.Linear)]


def forward8(ref, X, lS_o, lS_i, rows=None):
    """prob [B] (fp64) of OracleDLRM ``ref`` with every Linear under the int8 rule; the
    interaction in fp64 from the fp32 activations, rounded to fp32 (exact for "cat").
    ``rows``: per-table fp32 tables to look up instead of the oracle's."""
    with torch.no_grad():
        lb, lt = _linears(ref.bot_l), _linears(ref.top_l)
        x = E.stack(np.asarray(X, F32), [(W, b, True) for W, b in lb])
        if rows is None:
            ly = [y.double() for y in ref.apply_emb(torch.as_tensor(lS_o),
                                                    [torch.as_tensor(i) for i in lS_i])]
        else:  # one-hot bags
            ly = [torch.from_numpy(rows[t][np.asarray(lS_i[t])]).double()
                  for t in range(len(rows))]
        z = O.interact(torch.from_numpy(x).double(), ly, ref.op, ref.itself).numpy().astype(F32)
        layers = [(W, b, True) for W, b in lt[:-1]] + [(lt[-1][0], lt[-1][1], False)]
        zz = E.stack(z, layers).astype(np.float64).ravel()
    return 1.0 / (1.0 + np.exp(-zz))


# ------------------------------------------------------------ 1. bitwise end to end --
CAT = dict(D=8, rows=[50, 30, 20], bot=[13, 32, 8], top=[64, 16, 1], B=70)


def _cat_model(seed):
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    D, rows = CAT["D"], CAT["rows"]
    ln_top = [(len(rows) + 1) * D] + CAT["top"]
    np.random.seed(seed)
    ref = O.OracleDLRM(D, rows, CAT["bot"], ln_top, arch_interaction_op="cat",
                       loss_function="bce")
    cfg = TrainerConfig(m_spa=D, ln_emb=rows, ln_bot=CAT["bot"], ln_top=ln_top,
                        arch_interaction_op="cat", loss_function="bce")
    tr = DLRMTrainer.from_oracle(cfg, ref, device=dev)
    raw = _rand_batch(np.random.RandomState(seed), rows, CAT["B"], 1, CAT["bot"][0], "bce")
    return ref, tr, raw


@pytest.mark.parametrize("seed", [1, 2])
def test_bitwise_end_to_end(seed):
    """arch_interaction_op="cat" with one-hot lookups: everything before and between the MLPs
    is a copy, so z is the rule stack's and prob its sigmoid (1e-6: the fp32 expf of the head,
    as test_gpu_predict16 allows it)."""
    ref, tr, raw = _cat_model(seed)
    X, lS_o, lS_i, T = raw
    batch = tr.make_batch(*raw)
    tr.quantize_mlp(8)
    p8 = tr.predict(batch, mlp_bits=8).cpu().numpy().astype(np.float64)
    want = forward8(ref, X, lS_o, lS_i)
    assert np.abs(p8 - want).max() <= 1e-6
    # z itself is bitwise the rule's
    Bl = CAT["B"]
    z = tr._predict_bufs(tr._buffers(Bl, Bl))["z8"].cpu().numpy().ravel()
    lb, lt = _linears(ref.bot_l), _linears(ref.top_l)
    x = E.stack(X, [(W, b, True) for W, b in lb])
    rows = [e.weight.detach().numpy() for e in ref.emb_l]
    zin = np.concatenate([x] + [rows[t][lS_i[t]] for t in range(len(rows))], axis=1)
    zrule = E.stack(zin, [(W, b, True) for W, b in lt[:-1]] + [(lt[-1][0], lt[-1][1], False)])
    assert np.array_equal(z.view(np.uint32), zrule.ravel().view(np.uint32))
    p32 = tr.predict(batch).cpu().numpy()
    assert (p8 != p32).any()
    # with 8-bit tables: the same composition on the dequantised rows
    tr.quantize_embedding(8)
    deq = [Q.dequant(Q.pack_rows(np.ascontiguousarray(r, dtype=F32), 8), 8, CAT["D"])
           for r in rows]
    p88 = tr.predict(batch, mlp_bits=8, emb_bits=8).cpu().numpy().astype(np.float64)
    want88 = forward8(ref, X, lS_o, lS_i, rows=deq)
    assert np.abs(p88 - want88).max() <= 1e-6
    assert (want88 != want).any()
    tr.check_errors()


# --------------------------------------------------------------- 2. random weights --
@pytest.mark.parametrize("name", ["c2_small", "c3_small"])
def test_random_weights_vs_emulation(name):
    """As test_gpu_predict16's: q = max |p8_emul - p32_oracle| from CPU references only; the
    GPU's int8 result differs from the emulation only through the fp32 interaction's rounding
    and the code flips it causes, bounded by 2 q plus the fp32 path's own allowance.
    Measured on MI355X: c2_small q 1.326e-3, |gpu - emul| 5.3e-8;
    c3_small q 1.581e-3, |gpu - emul| 2.8e-5."""
    c, ref, tr = _make(name)
    X, lS_o, lS_i, T = _rand_batch(np.random.RandomState(3), c["rows"], c["B"], c["L"],
                                   c["bot"][0], c["loss"])
    p32_oracle = R.forward(ref, X, lS_o, lS_i, None)
    p8_emul = forward8(ref, X, lS_o, lS_i)
    q = float(np.abs(p8_emul - p32_oracle).max())
    assert q > 0.0
    batch = tr.make_batch(X, lS_o, lS_i, T)
    tr.quantize_mlp(8)
    p32 = tr.predict(batch).cpu().numpy().astype(np.float64)
    p8 = tr.predict(batch, mlp_bits=8).cpu().numpy().astype(np.float64)
    d_emul = float(np.abs(p8 - p8_emul).max())
    d_fp32 = float(np.abs(p8 - p32).max())
    print(f"predict8 {name}: q {q:.3e} |gpu-emul| {d_emul:.3e} |gpu-fp32| {d_fp32:.3e}")
    assert d_emul <= 2.0 * q + FP32_ALLOWANCE
    assert (p8 != p32).any()
    tr.check_errors()


# ------------------------------------------------------------ 3. snapshot semantics --
def test_snapshot_semantics():
    c, ref, tr = _make("c2_small")
    batch = tr.make_batch(*_rand_batch(np.random.RandomState(5), c["rows"], c["B"], 1,
                                       c["bot"][0], "bce"))
    tr.quantize_mlp(8)
    first = tr.predict(batch, mlp_bits=8).clone()
    torch.cuda.synchronize()
    run = tr.capture_predict(batch, mlp_bits=8)
    run()
    prob = tr._predict_bufs(tr._buffers(c["B"], c["B"]))["prob"]
    assert _bits_equal(prob, first)
    ptrs = [s.packed.wq.data_ptr() for s in tr.quantized_mlp(8).values()]
    p32 = tr.predict(batch).clone()
    with torch.no_grad():
        for L in tr.layers:  # the fp32 masters move: weights and biases
            L.W[:, :L.K].mul_(1.25)
            L.b.add_(0.01)
    assert not torch.equal(tr.predict(batch).clone(), p32)
    assert _bits_equal(tr.predict(batch, mlp_bits=8), first)  # the snapshot did not
    run()
    assert _bits_equal(prob, first)
    tr.quantize_mlp(8)  # re-pack into the same storage
    assert ptrs == [s.packed.wq.data_ptr() for s in tr.quantized_mlp(8).values()]
    second = tr.predict(batch, mlp_bits=8).clone()
    assert not torch.equal(second, first)
    prob.zero_()
    run()  # the graph captured before the re-pack reads the new values
    assert _bits_equal(prob, second)


# --------------------------------------------------- 4. capture_predict and evaluate --
def test_capture_and_evaluate():
    from dlrm_hip import metrics
    c, ref, tr = _make("c2_small")
    tr.quantize_mlp(8)
    tr.quantize_embedding(8)
    rng = np.random.RandomState(21)
    sizes = (128, 128, 37)
    raw = [_rand_batch(rng, c["rows"], B, 1, c["bot"][0], "bce") for B in sizes]
    lab = np.concatenate([T.ravel() for *_, T in raw])
    batches = [tr.make_batch(*r) for r in raw]
    for kw in (dict(mlp_bits=8), dict(mlp_bits=8, emb_bits=8)):
        eager8 = [tr.predict(b, **kw).clone() for b in batches]
        eager32 = [tr.predict(b).clone() for b in batches]
        torch.cuda.synchronize()
        for b, want in zip(batches, eager8):
            run = tr.capture_predict(b, **kw)
            run()
            Bl = b.X.shape[0]
            assert _bits_equal(tr._predict_bufs(tr._buffers(Bl, Bl))["prob"], want)
        n = sum(sizes)
        st32, st8 = metrics.EvalState(n, dev), metrics.EvalState(n, dev)
        tr.evaluate(batches, st32)  # fp32 first: its graphs must not serve the next call
        res8 = tr.evaluate(batches, st8, **kw)
        assert st32.count == st8.count == n
        own8 = np.concatenate([p.cpu().numpy() for p in eager8])
        own32 = np.concatenate([p.cpu().numpy() for p in eager32])
        assert (own8 != own32).any()
        mine = eval_ref.full(own8, lab)
        for k in ("tp", "fp", "tn", "fn", "roc_auc", "accuracy"):
            assert res8[k] == mine[k], (k, res8[k], mine[k])
        assert np.array_equal(_u32(st8.keys[:n]), np.sort(eval_ref.pack_keys(own8, lab)))


# ------------------------------------------------------------ 5. state is untouched --
def test_predict8_leaves_training_untouched():
    """Trainer B packs and runs int8 predicts (eager and captured) between training steps,
    trainer A does not: weights, optimizer state, losses and the step's own probabilities end
    bitwise equal."""
    out = {}
    for who in ("A", "B"):
        c, ref, tr = _make("c2_small")
        rng = np.random.RandomState(4)
        mk = lambda: tr.make_batch(*_rand_batch(rng, c["rows"], c["B"], 1, c["bot"][0], "bce"))
        train0, train1, test = mk(), mk(), mk()
        losses = [tr.step(train0)[1].clone()]
        if who == "B":
            tr.quantize_mlp(8)
            tr.predict(test, mlp_bits=8)
        losses.append(tr.step(train1)[1].clone())
        torch.cuda.synchronize()
        replay = tr.capture(train0)
        replay()
        if who == "B":
            tr.quantize_mlp(8)
            tr.predict(test, mlp_bits=8)
            torch.cuda.synchronize()
            run = tr.capture_predict(test, mlp_bits=8)
            for _ in range(2):
                run()
        replay()
        prob = tr._bufs[(c["B"], c["B"])]["prob"].clone()
        torch.cuda.synchronize()
        assert tr._roles == [] and tr.step_count == 4
        out[who] = losses + [prob] + _state(tr)
    assert len(out["A"]) == len(out["B"]) == 5
    for a, b in zip(out["A"], out["B"]):
        assert torch.equal(a, b)


# --------------------------------------------------------------------- 6. refusals --
def test_refusals():
    from dlrm_hip import metrics
    c, ref, tr = _make("c2_small")
    batch = tr.make_batch(*_rand_batch(np.random.RandomState(1), c["rows"], c["B"], 1,
                                       c["bot"][0], "bce"))
    st = metrics.EvalState(c["B"], dev)
    calls = lambda **kw: (lambda: tr.predict(batch, **kw),
                          lambda: tr.predict_segments(batch, **kw),
                          lambda: tr.capture_predict(batch, **kw),
                          lambda: tr.evaluate([batch], st, **kw))
    for call in calls(mlp_bits=8):  # no snapshot yet
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        tr.quantize_mlp(4)
    tr.quantize_mlp(8)
    for bad in (16, 4, "int8"):
        for call in calls(mlp_bits=bad):
            with pytest.raises(ValueError):
                call()
    for prec in ("bf16", "fp16"):
        for call in calls(mlp_bits=8, precision=prec):
            with pytest.raises(ValueError):
                call()
    for call in calls(precision="int8"):  # the name keeps refusing
        with pytest.raises(ValueError):
            call()
    # the multi-GPU schedule
    tr.distributed = True
    try:
        with pytest.raises(NotImplementedError, match="§21"):
            tr.quantize_mlp(8)
        with pytest.raises(NotImplementedError, match="§21"):
            tr.predict_segments(batch, mlp_bits=8)
    finally:
        tr.distributed = False
    assert tr.predict(batch, mlp_bits=8).shape == (c["B"],)
