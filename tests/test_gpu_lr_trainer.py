"""DLRMTrainer with device-resident learning rates (TrainerConfig.lr_num_warmup_steps /
lr_decay_start_step / lr_num_decay_steps / device_lr): the scheduled step, eager and as one
captured graph replayed, against an unscheduled trainer that is handed optim.lr_policy's rate
before every eager step.  Policy (W=3, S=5, D=3) over 10 steps: warm-up, plateau, decay and
the frozen tail.  Every comparison is bitwise; no test uses RCCL (EmulatedComm stands in for
the multi-rank schedule)."""
import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu
dev = "cuda:0"
POLICY = (3, 5, 3)
STEPS = 10
RATES = {"sgd": (0.1, 0.05), "rwsadagrad": (1e-3, 2e-3)}  # (dense, embedding) base rates

CASES = {  # the shapes of test_gpu_trainer / test_gpu_train16
    "c3_small": dict(D=128, rows=[min(r, 2000) for r in O.TERABYTE_ROWS], bot=[13, 512, 256, 128],
                     top=[1024, 1024, 512, 256, 1], B=256),
    "c2_small": dict(D=16, rows=[min(r, 5000) for r in O.KAGGLE_ROWS],
                     bot=[13, 512, 256, 64, 16], top=[512, 256, 1], B=128),
}

# kinds of the segment list a default-config trainer builds, recorded from the parent commit
PARENT_KINDS = {
    ("one", "sgd", "fp32"): ["gpu"] * 3 + ["host"],
    ("one", "rwsadagrad", "fp32"): ["gpu"] * 4 + ["host"],
    ("one", "sgd", "bf16"): ["gpu"] * 3 + ["host"],
    ("w8", "sgd", "fp32"): ["gpu", "a2a", "gpu", "a2a", "gpu", "gpu", "a2a", "ar", "gpu", "ar",
                            "a2a", "gpu", "ar", "gpu", "ar", "gpu", "host"],
    ("w8", "sgd", "bf16"): ["gpu", "a2a", "gpu", "a2a", "gpu", "gpu", "a2a", "ar", "gpu", "ar",
                            "a2a", "ar", "gpu", "ar", "gpu", "host"],
}


def _num_int(T, D):
    F = T + 1
    return D + F * (F - 1) // 2


def _trainer(name, optimizer, precision, world, **cfg_kw):
    """A fresh trainer (its own config object) from a fixed seed: one GPU, or rank 2 of 8
    with the collectives emulated and captured whole."""
    from dlrm_hip.trainer import DLRMTrainer, EmulatedComm, TrainerConfig
    c = CASES[name]
    lr, elr = RATES[optimizer]
    cfg = TrainerConfig(m_spa=c["D"], ln_emb=c["rows"], ln_bot=c["bot"],
                        ln_top=[_num_int(len(c["rows"]), c["D"])] + c["top"],
                        loss_function="bce", learning_rate=lr, emb_learning_rate=elr,
                        optimizer=optimizer, mlp_precision=precision, **cfg_kw)
    if world == "one":
        return DLRMTrainer(cfg, device=dev, seed=3)
    return DLRMTrainer(cfg, device=dev, rank=2, world_size=8, comm=EmulatedComm(whole=True),
                       seed=3)


def _state(tr):
    """Every tensor a step trains: the whole embedding buffer, the dense bucket, and with
    RWSAdagrad the row-wise momentum and the dense sum of squares."""
    parts = [tr.weights, tr.params]
    for extra in (tr.momentum, tr.adagrad_sum):
        if extra is not None:
            parts.append(extra)
    return parts


def _clone(tensors):
    return [t.clone() for t in tensors]


def _load(tr, saved):
    for dst, src in zip(_state(tr), saved):
        dst.copy_(src)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


def _assert_states(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert _same(a, b), f"{what}: state tensor {i} differs"


def _assert_outs(got, want, what, first=0):
    assert len(got) == len(want)
    for i, ((p, l), (pr, lr_)) in enumerate(zip(got, want)):
        assert _same(l, lr_), f"{what}: loss of step {first + i + 1}: {l.item()} vs {lr_.item()}"
        assert _same(p, pr), f"{what}: prob of step {first + i + 1}"


_BASE = {}


def _baseline(name, optimizer, precision, world):
    """The unscheduled trainer stepped eagerly with the policy's rate set before each step:
    per-step (prob, loss), and the state after steps 5 and 10.  Built once per case."""
    from dlrm_hip.optim import lr_policy
    key = (name, optimizer, precision, world)
    if key not in _BASE:
        tr = _trainer(name, optimizer, precision, world)
        assert tr.cfg.lr_mode == "host" and tr._lr_state is None
        lr, elr = RATES[optimizer]
        batch = tr.synthetic_batch(CASES[name]["B"], 1, seed=11)
        outs, snaps = [], {}
        for i in range(STEPS):
            tr.set_learning_rate(lr_policy(i + 1, lr, *POLICY), lr_policy(i + 1, elr, *POLICY))
            prob, loss = tr.step(batch)
            outs.append((prob.clone(), loss.clone()))
            if i + 1 in (5, STEPS):
                snaps[i + 1] = _clone(_state(tr))
        tr.check_errors()
        _BASE[key] = (outs, snaps)
    return _BASE[key]


def _scheduled(name, optimizer, precision, world):
    W, S, D = POLICY
    tr = _trainer(name, optimizer, precision, world, lr_num_warmup_steps=W,
                  lr_decay_start_step=S, lr_num_decay_steps=D)
    assert tr.cfg.lr_mode == "device"
    return tr, tr.synthetic_batch(CASES[name]["B"], 1, seed=11)


def _captured(tr, batch):
    """capture() needs one eager step of the batch size first; that step trains and ticks, so
    the state and the schedule's counter are put back before the graph is replayed."""
    start = _clone(_state(tr))
    tr.step(batch)
    _load(tr, start)
    tr.lr_step = 1
    run = tr.capture(batch)
    assert tr.capture_mode == "whole" and tr.graphs_per_step == 1
    return run


def _replay(tr, run, n):
    outs = []
    for _ in range(n):
        run()
        outs.append((tr._cur["prob"].clone(), tr._cur["loss"].clone()))
    return outs


@pytest.mark.parametrize("world", ["one", "w8"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("optimizer", ["sgd", "rwsadagrad"])
@pytest.mark.parametrize("name", ["c2_small", "c3_small"])
def test_scheduled_step_equals_the_host_driven_baseline(name, optimizer, precision, world):
    want_outs, snaps = _baseline(name, optimizer, precision, world)
    # eager
    tr, batch = _scheduled(name, optimizer, precision, world)
    assert tr.lr_step == 1
    outs = []
    for _ in range(STEPS):
        prob, loss = tr.step(batch)
        outs.append((prob.clone(), loss.clone()))
    tr.check_errors()
    assert tr.lr_step == STEPS + 1
    _assert_outs(outs, want_outs, "eager")
    _assert_states(_state(tr), snaps[STEPS], "eager")
    assert not _same(snaps[5][1], snaps[STEPS][1])  # the later steps trained
    # one captured whole-step graph, replayed on the same batch buffers
    tr, batch = _scheduled(name, optimizer, precision, world)
    run = _captured(tr, batch)
    outs = _replay(tr, run, STEPS)
    tr.check_errors()
    assert tr.lr_step == STEPS + 1
    _assert_outs(outs, want_outs, "graph")
    _assert_states(_state(tr), snaps[STEPS], "graph")


def test_rates_walk_the_policy_and_resume_from_lr_step():
    """current_lr() after each replay is the policy's value as fp32 (dense, embedding, dense / W);
    predict between replays leaves the counter alone; setting lr_step = 6 on the state after
    step 5 replays the baseline's steps 6 to 10."""
    from dlrm_hip.optim import lr_policy
    name, optimizer, precision, world = "c2_small", "sgd", "fp32", "w8"
    want_outs, snaps = _baseline(name, optimizer, precision, world)
    lr, elr = RATES[optimizer]
    tr, batch = _scheduled(name, optimizer, precision, world)
    assert tr.current_lr() == [float(np.float32(lr)), float(np.float32(elr)),
                               float(np.float32(lr * (1.0 / 8)))]
    run = _captured(tr, batch)
    outs = []
    for i in range(STEPS):
        outs += _replay(tr, run, 1)
        want = [np.float32(lr_policy(i + 1, lr, *POLICY)), np.float32(lr_policy(i + 1, elr, *POLICY)),
                np.float32(lr_policy(i + 1, lr, *POLICY) * (1.0 / 8))]
        assert tr.current_lr() == [float(v) for v in want], (i, tr.current_lr(), want)
        if i == 3:
            before = tr.lr_step
            tr.predict(batch)
            tr.predict(batch, precision="bf16")
            assert tr.lr_step == before == i + 2
    _assert_outs(outs, want_outs, "graph with predict in between")
    _assert_states(_state(tr), snaps[STEPS], "graph with predict in between")
    # resume: the state after step 5, the counter at 6
    _load(tr, snaps[5])
    tr.lr_step = 6
    assert tr.lr_step == 6
    outs = _replay(tr, run, STEPS - 5)
    _assert_outs(outs, want_outs[5:], "resumed", first=5)
    _assert_states(_state(tr), snaps[STEPS], "resumed")


@pytest.mark.parametrize("optimizer,world", [("sgd", "one"), ("rwsadagrad", "w8")])
def test_device_lr_without_a_policy_follows_set_learning_rate(optimizer, world):
    """device_lr=True and no policy: set_learning_rate between replays of ONE captured graph
    equals a host-rate trainer stepped eagerly at the same rates."""
    name, precision = "c2_small", "fp32"
    lr, elr = RATES[optimizer]
    seq = [(lr, elr), (lr * 0.2, elr * 3.0), (lr * 3.0, None), (lr * 3.0, elr)]
    host = _trainer(name, optimizer, precision, world)
    batch = host.synthetic_batch(CASES[name]["B"], 1, seed=12)
    want = []
    for a, b in seq:
        host.set_learning_rate(a, b)
        prob, loss = host.step(batch)
        want.append((prob.clone(), loss.clone()))
    tr = _trainer(name, optimizer, precision, world, device_lr=True)
    assert tr.cfg.lr_mode == "device"
    batch = tr.synthetic_batch(CASES[name]["B"], 1, seed=12)
    run = _captured(tr, batch)
    outs = []
    for a, b in seq:
        tr.set_learning_rate(a, b)
        outs += _replay(tr, run, 1)
        e = tr.emb_lr
        scale = 1.0 if world == "one" else 1.0 / 8
        assert tr.current_lr() == [float(np.float32(a)), float(np.float32(e)),
                                   float(np.float32(a * scale))]
    _assert_outs(outs, want, "device_lr")
    _assert_states(_state(tr), _state(host), "device_lr")
    with pytest.raises(RuntimeError):
        host.lr_step


@pytest.mark.parametrize("world,optimizer,precision", sorted(PARENT_KINDS))
def test_default_config_builds_the_parents_segment_list(world, optimizer, precision):
    """With the four new fields at their defaults the step is the parent's: the same number
    and kinds of segments, no state block, host floats.  The scheduled step has the same
    kinds too: its tick is part of the first "gpu" segment."""
    tr = _trainer("c2_small", optimizer, precision, world)
    batch = tr.synthetic_batch(CASES["c2_small"]["B"], 1, seed=1)
    kinds = [k for k, _ in tr.segments(batch)]
    assert kinds == PARENT_KINDS[(world, optimizer, precision)]
    assert tr._lr_state is None and all(isinstance(v, float) for v in tr._rates())
    sched, batch = _scheduled("c2_small", optimizer, precision, world)
    assert [k for k, _ in sched.segments(batch)] == kinds
    assert all(isinstance(v, torch.Tensor) for v in sched._rates())
