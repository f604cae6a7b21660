"""DLRMTrainer with mlp_precision="bf16" (the mixed-precision step: every MLP Linear below the
head on the 16-bit MFMA, forward, data gradient and weight gradient) against the fp64
emulation of the rounded operands (train16_ref), plus its wiring: graphs, determinism, the
two update paths, the multi-GPU schedule, and the promise that "fp32" runs what it ran.

Measured on one MI355X (worst |gpu - emulation| / q per group, one bf16 step; the bound is
2 q + 1e-5 max(1, |ref|)): see DESIGN.md §16."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import linear16_ref as R
import oracle as O
import train16_ref as T16

pytestmark = pytest.mark.gpu
dev = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ADAGRAD_LR = 1e-3
FP32_ALLOWANCE = 1e-5  # conftest.fp32_close's bound: 1e-5 * max(1, |ref|)

CASES = {  # as test_gpu_predict16.CASES
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


_REFS = {}


def _oracle(name, seed=7):
    """The case's oracle model, built once and only read (from_oracle and clone64 copy)."""
    if (name, seed) not in _REFS:
        c = CASES[name]
        ln_top = [_num_int(len(c["rows"]), c["D"])] + c["top"]
        np.random.seed(seed)
        _REFS[(name, seed)] = (ln_top, O.OracleDLRM(c["D"], c["rows"], c["bot"], ln_top,
                                                    loss_function=c["loss"]))
    return _REFS[(name, seed)]


def _make(name, seed=7, trainer_kw=None, lr=None, **cfg_kw):
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    c = CASES[name]
    ln_top, ref = _oracle(name, seed)
    cfg = TrainerConfig(m_spa=c["D"], ln_emb=c["rows"], ln_bot=c["bot"], ln_top=ln_top,
                        loss_function=c["loss"], learning_rate=lr or c["lr"], **cfg_kw)
    return c, ref, DLRMTrainer.from_oracle(cfg, ref, device=dev, **(trainer_kw or {}))


def _batches(name, n, seed=3):
    c = CASES[name]
    rng = np.random.RandomState(seed)
    return [_rand_batch(rng, c["rows"], c["B"], c["L"], c["bot"][0], c["loss"]) for _ in range(n)]


def _bits_equal(a, b):
    return a.dtype == b.dtype == torch.float32 and torch.equal(
        a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _state(tr):
    parts = [tr.weights, tr.params]
    for extra in (tr.momentum, tr.adagrad_sum, tr.grads):
        if extra is not None:
            parts.append(extra)
    return [p.clone() for p in parts]


# ------------------------------------------------------- 1, 3. one step vs emulation --
def _emulate(ref, batches, dt, optimizer, lr):
    """One training step on batches[0], then the step-2 forward on batches[1], in fp64."""
    m = T16.clone64(ref)
    opt = O.RWSAdagradOracle(m.parameters(), lr=lr) if optimizer == "rwsadagrad" else None
    prob, loss = T16.train_step(m, *batches[0], lr, dt, opt)
    out = {"prob": prob, "loss": np.array([loss]),
           "prob2": T16.predict(m, *batches[1][:3], dt)}
    lin = [x for seq in (m.bot_l, m.top_l) for x in seq if isinstance(x, torch.nn.Linear)]
    for i, x in enumerate(lin):
        out[f"W{i}"] = x.weight.detach().numpy()
        out[f"b{i}"] = x.bias.detach().numpy()
    out["tables"] = np.concatenate([e.weight.detach().numpy().ravel() for e in m.emb_l])
    if opt is not None:
        out["momentum"] = np.concatenate(
            [opt.state[id(e.weight)]["momentum"].numpy().ravel() for e in m.emb_l])
    return out


def _device(tr, batches):
    b0, b1 = (tr.make_batch(*b) for b in batches[:2])
    prob, loss = tr.step(b0)
    out = {"prob": prob.cpu().numpy(), "loss": loss.cpu().numpy()}
    for i, (W, b) in enumerate(tr.dense_state()):
        out[f"W{i}"], out[f"b{i}"] = W.cpu().numpy(), b.cpu().numpy()
    out["tables"] = np.concatenate([tr.table(t).cpu().numpy().ravel() for t in tr.local_tables])
    if tr.momentum is not None:
        out["momentum"] = np.concatenate(
            [tr.table_momentum(t).cpu().numpy().ravel() for t in tr.local_tables])
    out["prob2"] = tr.step(b1)[0].cpu().numpy()  # the second step's forward: updated weights
    tr.check_errors()
    return out


@pytest.mark.parametrize("name,optimizer", [("c2_small", "sgd"), ("c3_small", "sgd"),
                                            ("c2_small", "rwsadagrad")])
def test_one_step_against_the_emulation(name, optimizer):
    """For every dense tensor, all tables together, prob, loss and the second step's prob:
    q = max |emulation(bf16) - emulation(None)| from the CPU references alone (> 0), and the
    device's bf16 step within 2 q + 1e-5 max(1, |ref|) of emulation(bf16): the device is
    another realisation of the same rounding noise, plus fp32 summation order.  "sgd" takes
    the fused-epilogue update, "rwsadagrad" the gradient bucket + adagrad_update and the
    tables' row-wise momentum (at lr = 1e-3: Adagrad's first step moves every weight by lr,
    and at the cases' 0.1 the second step's prob saturates at 0 / 1 in every realisation).
    The result also differs from the fp32 step's."""
    lr = ADAGRAD_LR if optimizer == "rwsadagrad" else CASES[name]["lr"]
    c, ref, tr = _make(name, optimizer=optimizer, mlp_precision="bf16", lr=lr)
    assert tr.cfg.mlp_precision == "bf16" and (tr.grads is None) == (optimizer == "sgd")
    batches = _batches(name, 2)
    e0 = _emulate(ref, batches, None, optimizer, lr)
    eb = _emulate(ref, batches, "bf16", optimizer, lr)
    got = _device(tr, batches)
    assert tr._roles == [] and tr.step_count == 2 and not tr.bottom_fused
    _, _, tr32 = _make(name, optimizer=optimizer, lr=lr)
    got32 = _device(tr32, batches)
    worst, failed = 0.0, []
    for k in eb:
        q = float(np.abs(eb[k] - e0[k]).max())
        d = float(np.abs(got[k].astype(np.float64).ravel() - eb[k].ravel()).max())
        tol = 2.0 * q + FP32_ALLOWANCE * np.maximum(1.0, np.abs(eb[k].ravel()))
        over = np.abs(got[k].astype(np.float64).ravel() - eb[k].ravel()) > tol
        print(f"train16 {name} {optimizer} {k:8s} q {q:.3e} d {d:.3e} d/q {d / q if q else 0:.3f}")
        assert q > 0.0, k
        worst = max(worst, d / q)
        if over.any():
            failed.append((k, q, d))
    print(f"train16 {name} {optimizer}: worst d/q {worst:.3f}")
    assert not failed, failed
    assert any((got[k] != got32[k]).any() for k in got if k.startswith("W"))
    assert (got["prob"] != got32["prob"]).any()


# --------------------------------------------------------- 2. exact forward wiring --
@pytest.mark.parametrize("seed", R.TINY_SEEDS)
def test_exact_forward_wiring(seed):
    """On the all-integer tiny model every Linear input is exact in bf16: the bf16 step's
    prob is bitwise the fp32 step's prob from the same weights."""
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    ref, X, lS_o, lS_i, T = R.tiny_exact_model(seed)
    ok, worst = R.linear_inputs_exact(ref, X, lS_o, lS_i, "bf16")
    assert ok, worst
    probs = {}
    for prec in ("fp32", "bf16"):
        cfg = TrainerConfig(m_spa=R.TINY["D"], ln_emb=R.TINY["rows"], ln_bot=R.TINY["bot"],
                            ln_top=R.tiny_ln_top(), loss_function="bce", mlp_precision=prec)
        tr = DLRMTrainer.from_oracle(cfg, ref, device=dev)
        probs[prec] = tr.step(tr.make_batch(X, lS_o, lS_i, T))[0].clone()
        tr.check_errors()
    assert _bits_equal(probs["bf16"], probs["fp32"])
    assert len(torch.unique(probs["fp32"])) >= 4


# ------------------------------------------------------ 4. graphs and determinism --
@pytest.mark.parametrize("predicts", [False, True])
@pytest.mark.parametrize("optimizer", ["sgd", "rwsadagrad"])
def test_graph_replay_is_bitwise_the_eager_step(optimizer, predicts):
    """Two eager steps against one eager step + one replay of capture(), from the same
    weights: parameters, tables, optimizer state, prob and loss bitwise equal - also with
    bf16 predicts (eager and captured) between the steps of the second trainer."""
    out = {}
    raw = _batches("c2_small", 3, seed=4)
    for who in ("eager", "graph"):
        c, ref, tr = _make("c2_small", optimizer=optimizer, mlp_precision="bf16")
        b0, b1, test = (tr.make_batch(*b) for b in raw)
        tr.step(b0)
        if who == "eager":
            prob, loss = tr.step(b1)
        else:
            if predicts:
                tr.predict(test, precision="bf16")
            torch.cuda.synchronize()
            run = tr.capture(b1)
            if predicts:
                torch.cuda.synchronize()
                tr.capture_predict(test, precision="bf16")()
            run()
            if predicts:
                tr.predict(test, precision="bf16")
            assert tr.capture_mode == "whole" and tr.graphs_per_step == 1
            prob, loss = tr._cur["prob"], tr._cur["loss"]
        torch.cuda.synchronize()
        tr.check_errors()
        assert tr.step_count == 2 and tr._roles == []
        out[who] = [prob.clone(), loss.clone()] + _state(tr)
    assert len(out["eager"]) == len(out["graph"])
    for a, b in zip(out["eager"], out["graph"]):
        assert _bits_equal(a, b)


# --------------------------------------------------------------- 5. fp32 untouched --
def test_fp32_is_untouched_and_bad_values_raise():
    from dlrm_hip.trainer import TrainerConfig
    raw = _batches("c2_small", 2, seed=5)
    out = []
    for kw in ({}, dict(mlp_precision="fp32")):
        c, ref, tr = _make("c2_small", **kw)
        res = []
        for b in raw:
            prob, loss = tr.step(tr.make_batch(*b))
            res += [prob.clone(), loss.clone()]
        out.append(res + _state(tr))
    for a, b in zip(*out):
        assert _bits_equal(a, b)
    kw = dict(m_spa=4, ln_emb=[8], ln_bot=[4, 4], ln_top=[5, 1])
    with pytest.raises(NotImplementedError):
        TrainerConfig(**kw, mlp_precision="fp16")
    with pytest.raises(ValueError):
        TrainerConfig(**kw, mlp_precision="int8")


# --------------------------------------------------------- 6. distributed schedule --
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _one_rank_worker(port, q):
    """One process: the single-GPU bf16 step and the multi-GPU schedule's (force_dist on a
    1-rank RCCL group), eager, from the same weights on the same batch."""
    try:
        sys.path[:0] = [ROOT, os.path.join(ROOT, "dlrm-yx_amd"), HERE]
        import torch.distributed as dist
        d = torch.device("cuda", 0)
        torch.cuda.set_device(d)
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0,
                                world_size=1, device_id=d)
        raw = _batches("c2_small", 1, seed=6)[0]
        out = {}
        for name, kw in (("single", {}),
                         ("nccl", dict(force_dist=True, process_group=dist.group.WORLD))):
            c, ref, tr = _make("c2_small", trainer_kw=kw, mlp_precision="bf16")
            assert tr.distributed == (name == "nccl")
            prob, loss = tr.step(tr.make_batch(*raw))
            torch.cuda.synchronize()
            tr.check_errors()
            out[name] = dict(prob=prob.cpu().numpy(), loss=loss.cpu().numpy(),
                             tables=tr.weights.cpu().numpy(), dense=tr.params.cpu().numpy(),
                             roles=len(tr._roles))
        dist.destroy_process_group()
        q.put(out)
    except Exception:  # pragma: no cover
        import traceback
        q.put(traceback.format_exc())


def test_distributed_schedule_on_one_rank():
    """The role-free multi-GPU segment list (wgrads STORE into the bucket, all-reduce, dense
    update) after one bf16 step: prob bitwise the single-GPU bf16 step's (the same forward
    launches), weights and tables within fp32_close (only the update's rounding differs)."""
    from conftest import fp32_close
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_one_rank_worker, args=(_free_port(), q), daemon=True)
    p.start()
    out = q.get(timeout=300)
    p.join(timeout=60)
    assert isinstance(out, dict), out
    a, b = out["single"], out["nccl"]
    assert np.array_equal(a["prob"].view(np.uint32), b["prob"].view(np.uint32))
    assert a["roles"] == b["roles"] == 0
    for k in ("loss", "dense", "tables"):
        ok, msg = fp32_close(b[k], a[k])
        assert ok, (k, msg)
    assert (a["dense"] != _make("c2_small")[2].params.cpu().numpy()).any()


# -------------------------------------------------------------------- 7. sanity --
def test_twenty_steps_reduce_the_loss():
    c, ref, tr = _make("c2_small", mlp_precision="bf16")
    batch = tr.make_batch(*_batches("c2_small", 1, seed=8)[0])
    losses = [float(tr.step(batch)[1]) for _ in range(20)]
    print("train16 losses:", " ".join(f"{v:.4f}" for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    tr.check_errors()
