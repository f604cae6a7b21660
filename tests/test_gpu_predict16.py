"""DLRMTrainer.predict / capture_predict / evaluate with precision = "bf16" | "fp16" and the
module front-end's DLRM_Net.quantize_mlp: exact wiring on an all-integer model (bitwise the
fp32 path), random weights against the fp64 emulation of the rounded operands
(linear16_ref), and the promise that a 16-bit predict never touches training state."""
import numpy as np
import pytest
import torch

import eval_ref
import linear16_ref as R
import oracle as O

pytestmark = pytest.mark.gpu
dev = "cuda:0"
DTS = ["bf16", "fp16"]
FP32_ALLOWANCE = 1e-5  # conftest.fp32_close's bound for values in [0, 1]: 1e-5 * max(1, |ref|)

CASES = {  # as test_gpu_eval.CASES
    "c3_small": dict(D=128, rows=[min(r, 2000) for r in O.TERABYTE_ROWS], bot=[13, 512, 256, 128],
                     top=[1024, 1024, 512, 256, 1], B=256, L=1, loss="bce", lr=0.1),
    "c2_small": dict(D=16, rows=[min(r, 5000) for r in O.KAGGLE_ROWS],
                     bot=[13, 512, 256, 64, 16], top=[512, 256, 1], B=128, L=1, loss="bce",
                     lr=0.1),
}


def _num_int(T, D, itself=False):
    F = T + 1
    return D + (F * (F + 1) // 2 if itself else F * (F - 1) // 2)


def _rand_batch(rng, rows, B, L, m_den, loss):
    X = np.log1p(rng.rand(B, m_den).astype(np.float32))
    lS_o = np.array([np.arange(B) * L for _ in rows], dtype=np.int64)
    lS_i = [rng.randint(0, n, size=B * L).astype(np.int64) for n in rows]
    T = rng.rand(B, 1).astype(np.float32)
    if loss == "bce":
        T = np.round(T)
    return X, lS_o, lS_i, T


def _make(name, seed=7, **cfg_kw):
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    c = CASES[name]
    D, rows = c["D"], c["rows"]
    ln_top = [_num_int(len(rows), D)] + c["top"]
    np.random.seed(seed)
    ref = O.OracleDLRM(D, rows, c["bot"], ln_top, loss_function=c["loss"])
    cfg = TrainerConfig(m_spa=D, ln_emb=rows, ln_bot=c["bot"], ln_top=ln_top,
                        loss_function=c["loss"], learning_rate=c["lr"], **cfg_kw)
    return c, ref, DLRMTrainer.from_oracle(cfg, ref, device=dev)


def _bits_equal(a, b):
    return a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32),
                                                               b.view(torch.int32))


def _u32(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ 1. exact wiring --
VARIANTS = [("default", False, {}), ("lookup_gemms", False, dict(fuse_gather=False,
                                                                 fuse_bottom=False)),
            ("itself", True, {})]


# self-dot terms up to 484 are not exact in bf16: the "itself" variant is fp16's
WIRING = [(dt, v[0]) for dt in DTS for v in VARIANTS if not (v[1] and dt != "fp16")]


@pytest.mark.parametrize("dt,variant", WIRING)
def test_exact_wiring(dt, variant):
    """An all-integer model whose Linear inputs are exact in the 16-bit type (asserted with
    the fp64 oracle): the 16-bit predict equals the fp32 predict bit for bit, also after the
    fp32 weights change in place (there is no stale 16-bit copy)."""
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    _, itself, attrs = [v for v in VARIANTS if v[0] == variant][0]
    for seed in R.TINY_SEEDS:
        ref, X, lS_o, lS_i, T = R.tiny_exact_model(seed, itself)
        ok, worst = R.linear_inputs_exact(ref, X, lS_o, lS_i, dt)
        assert ok, worst
        cfg = TrainerConfig(m_spa=R.TINY["D"], ln_emb=R.TINY["rows"], ln_bot=R.TINY["bot"],
                            ln_top=R.tiny_ln_top(itself), arch_interaction_itself=itself,
                            loss_function="bce")
        tr = DLRMTrainer.from_oracle(cfg, ref, device=dev)
        for k, v in attrs.items():
            setattr(tr, k, v)
        batch = tr.make_batch(X, lS_o, lS_i, T)
        p32 = tr.predict(batch).clone()
        p16 = tr.predict(batch, precision=dt).clone()
        assert _bits_equal(p16, p32), (seed, (p16 - p32).abs().max())
        assert np.allclose(p32.cpu().numpy(), R.forward(ref, X, lS_o, lS_i), rtol=0, atol=1e-6)
        # the fp32 master weights move: both precisions must follow
        assert R.bump_weights(ref) == len(tr.layers)
        ok, worst = R.linear_inputs_exact(ref, X, lS_o, lS_i, dt)
        assert ok, worst
        for L in tr.layers:
            L.W[0, 0] += 1.0
        q32 = tr.predict(batch).clone()
        q16 = tr.predict(batch, precision=dt).clone()
        assert _bits_equal(q16, q32), seed
        assert not torch.equal(q32, p32)
        assert np.allclose(q32.cpu().numpy(), R.forward(ref, X, lS_o, lS_i), rtol=0, atol=1e-6)
        tr.check_errors()


# --------------------------------------------------------------- 2. random weights --
@pytest.mark.parametrize("name", ["c2_small", "c3_small"])
@pytest.mark.parametrize("dt", DTS)
def test_random_weights_vs_emulation(dt, name):
    """q = max |p16_emul - p32_oracle| (CPU references only) is the size of the quantization
    effect; the GPU's 16-bit result differs from the emulation only by fp32 summation order
    and the rounding flips it causes - another realisation of the same noise, bounded by
    2 q plus the fp32 path's own allowance.
    The measured figures are in DESIGN.md (forward-only section)."""
    c, ref, tr = _make(name)
    X, lS_o, lS_i, T = _rand_batch(np.random.RandomState(3), c["rows"], c["B"], c["L"],
                                   c["bot"][0], c["loss"])
    p32_oracle = R.forward(ref, X, lS_o, lS_i, None)
    p16_emul = R.forward(ref, X, lS_o, lS_i, dt)
    q = float(np.abs(p16_emul - p32_oracle).max())
    assert q > 0.0
    batch = tr.make_batch(X, lS_o, lS_i, T)
    p32 = tr.predict(batch).cpu().numpy().astype(np.float64)
    p16 = tr.predict(batch, precision=dt).cpu().numpy().astype(np.float64)
    d_emul = float(np.abs(p16 - p16_emul).max())
    d_fp32 = float(np.abs(p16 - p32).max())
    print(f"predict16 {name} {dt}: q {q:.3e} |gpu-emul| {d_emul:.3e} |gpu-fp32| {d_fp32:.3e}")
    assert d_emul <= 2.0 * q + FP32_ALLOWANCE
    assert d_fp32 <= 2.0 * q + FP32_ALLOWANCE
    assert (p16 != p32).any()
    tr.check_errors()


# ------------------------------------------------------------ 3. state is untouched --
def _state(tr):
    parts = [tr.weights, tr.params]
    for extra in (tr.momentum, tr.adagrad_sum, tr.grads):
        if extra is not None:
            parts.append(extra)
    return [p.clone() for p in parts]


@pytest.mark.parametrize("optimizer", ["sgd", "rwsadagrad"])
@pytest.mark.parametrize("dt", DTS)
def test_predict16_leaves_training_untouched(dt, optimizer):
    """Trainer B runs 16-bit predicts (eager and captured) between training steps and between
    replays of a captured training graph, trainer A does not: weights, optimizer state,
    losses and the step's own probabilities end bitwise equal - the activation buffers'
    constant-1 columns and every workspace survive the 16-bit launches."""
    out = {}
    for who in ("A", "B"):
        c, ref, tr = _make("c2_small", optimizer=optimizer)
        rng = np.random.RandomState(4)
        mk = lambda: tr.make_batch(*_rand_batch(rng, c["rows"], c["B"], 1, c["bot"][0], "bce"))
        train0, train1, test = mk(), mk(), mk()
        losses = [tr.step(train0)[1].clone()]
        if who == "B":
            first = tr.predict(test, precision=dt).clone()
        losses.append(tr.step(train1)[1].clone())
        torch.cuda.synchronize()
        replay = tr.capture(train0)
        replay()
        if who == "B":
            tr.predict(test, precision=dt)
            torch.cuda.synchronize()
            run = tr.capture_predict(test, precision=dt)
            for _ in range(2):
                run()
            assert tr.predict(test, precision=dt).shape == first.shape
        replay()
        prob = tr._bufs[(c["B"], c["B"])]["prob"].clone()
        torch.cuda.synchronize()
        assert tr._roles == [] and tr.step_count == 4
        out[who] = losses + [prob] + _state(tr)
    assert len(out["A"]) == len(out["B"]) == 3 + (2 if optimizer == "sgd" else 5)
    for a, b in zip(out["A"], out["B"]):
        assert torch.equal(a, b)


# --------------------------------------------------- 4. capture_predict and evaluate --
@pytest.mark.parametrize("dt", DTS)
def test_capture_and_evaluate(dt):
    from dlrm_hip import metrics
    c, ref, tr = _make("c2_small")
    rng = np.random.RandomState(21)
    sizes = (128, 128, 37)
    raw = [_rand_batch(rng, c["rows"], B, 1, c["bot"][0], "bce") for B in sizes]
    lab = np.concatenate([T.ravel() for *_, T in raw])
    batches = [tr.make_batch(*r) for r in raw]
    eager16 = [tr.predict(b, precision=dt).clone() for b in batches]
    eager32 = [tr.predict(b).clone() for b in batches]
    torch.cuda.synchronize()
    for b, want in zip(batches, eager16):
        run = tr.capture_predict(b, precision=dt)
        run()
        got = tr.predict(b, precision=dt)  # the tensor the replay wrote, then the eager rerun
        assert _bits_equal(got, want)
        run()
        assert _bits_equal(tr._predict_bufs(tr._buffers(b.X.shape[0], b.X.shape[0]))["prob"], want)
    n = sum(sizes)
    st32, st16 = metrics.EvalState(n, dev), metrics.EvalState(n, dev)
    res32 = tr.evaluate(batches, st32)  # fp32 first: its graphs must not serve the next call
    res16 = tr.evaluate(batches, st16, precision=dt)
    assert st32.count == st16.count == n
    own16 = np.concatenate([p.cpu().numpy() for p in eager16])
    own32 = np.concatenate([p.cpu().numpy() for p in eager32])
    assert (own16 != own32).any()
    for res, own in ((res16, own16), (res32, own32)):
        mine = eval_ref.full(own, lab)
        for k in ("tp", "fp", "tn", "fn", "n_pos", "n_neg", "roc_auc", "recall", "precision",
                  "f1", "accuracy"):
            assert res[k] == mine[k], (k, res[k], mine[k])
        assert res["auc_num2"] == mine["a2"] and abs(res["ap"] - mine["ap"]) <= 1e-12
    # compute() sorted the logs in place: compare them as sorted key sets
    assert np.array_equal(_u32(st16.keys[:n]), np.sort(eval_ref.pack_keys(own16, lab)))
    assert np.array_equal(_u32(st32.keys[:n]), np.sort(eval_ref.pack_keys(own32, lab)))


# ------------------------------------------------------------------ 5. bad argument --
def test_bad_precision_raises():
    from dlrm_hip import metrics
    c, ref, tr = _make("c2_small")
    batch = tr.make_batch(*_rand_batch(np.random.RandomState(1), c["rows"], c["B"], 1,
                                       c["bot"][0], "bce"))
    for call in (lambda: tr.predict(batch, precision="int8"),
                 lambda: tr.predict_segments(batch, precision="int8"),
                 lambda: tr.capture_predict(batch, precision="int8"),
                 lambda: tr.evaluate([batch], metrics.EvalState(c["B"], dev), precision="int8")):
        with pytest.raises(ValueError):
            call()


# -------------------------------------------------------------- 6. module front-end --
@pytest.mark.parametrize("dt", DTS)
def test_module_front_end(dt):
    """DLRM_Net.quantize_mlp(16, dt): HipMLP forwards (a contiguous K = 13 first layer with
    ldw = 13, a sigmoid N = 1 last layer) on integer weights are bitwise the fp32 forwards;
    with grad enabled they raise; 8 bits is not implemented; 32 restores fp32.  Every weight
    row has two nonzeros from {-1, 1}, biases and tables are in {-1, 0, 1}, X in {0, 1, 2}:
    the Linear inputs are integers <= 11 (bottom), 44 (dot terms), 89 (top), exact in both
    types."""
    from dlrm_hip.dlrm_net import DLRM_Net
    from dlrm_hip.modules import HipMLP
    np.random.seed(3)
    net = DLRM_Net(4, np.array([20, 20, 20]), np.array([13, 8, 4]), np.array([10, 4, 1]),
                   arch_interaction_op="dot", sigmoid_top=1, loss_function="bce").to(dev)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for mlp in (net.bot_l, net.top_l):
            assert isinstance(mlp, HipMLP)
            for m in mlp:
                if isinstance(m, torch.nn.Linear):
                    W = torch.zeros(m.weight.shape)
                    for n in range(W.shape[0]):
                        cols = torch.randperm(W.shape[1], generator=g)[:2]
                        W[n, cols] = torch.randint(0, 2, (2,), generator=g).float() * 2 - 1
                    m.weight.copy_(W)
                    m.bias.copy_(torch.randint(-1, 2, m.bias.shape, generator=g).float())
        for e in net.emb_l.parameters():
            e.copy_(torch.randint(-1, 2, e.shape, generator=g).float())
    assert net.bot_l[0].weight.stride(0) == 13 and net.top_l[2].weight.shape == (1, 4)
    B = 37
    X = torch.randint(0, 3, (B, 13), generator=g).float().to(dev)
    Zin = torch.randint(-9, 10, (B, 10), generator=g).float().to(dev)
    lS_o = torch.arange(B).repeat(3, 1).to(dev)
    lS_i = [torch.randint(0, 20, (B,), generator=g).to(dev) for _ in range(3)]
    keys = list(net.state_dict())
    with torch.no_grad():
        want = [net.bot_l(X).clone(), net.top_l(Zin).clone(), net(X, lS_o, lS_i).clone()]
    assert float(want[0].abs().max()) <= 11 and len(torch.unique(want[1])) >= 2
    with pytest.raises(NotImplementedError):
        net.quantize_mlp(8)
    net.quantize_mlp(16, dt)
    assert list(net.state_dict()) == keys
    with torch.no_grad():
        got = [net.bot_l(X), net.top_l(Zin), net(X, lS_o, lS_i)]
    for a, b in zip(got, want):
        assert a.shape == b.shape and _bits_equal(a.contiguous(), b.contiguous())
    with pytest.raises(RuntimeError):
        net.bot_l(X)
    with torch.no_grad():  # the fp32 parameters are the only weights: a change shows at once
        net.top_l[0].weight[0, 0] += 1.0
        moved = net.top_l(Zin)
        net.quantize_mlp(32)
        assert _bits_equal(moved, net.top_l(Zin)) and not torch.equal(moved, want[1])
    net.bot_l(X).sum().backward()  # fp32 again: trains
