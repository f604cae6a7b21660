"""TrainerConfig(optimizer="adagrad"): element-wise Adagrad (torch.optim.Adagrad) in the fused
engine.  (a) three-step trajectories against the CPU oracle stepped by torch.optim.Adagrad;
(b) bitwise identities inside the engine (replayed = eager, device rate = host rate, the LR
schedule, the bf16-MLP step's update = the kernel on its own dE); (c) two ranks; (d) refusals.

(a) and (c) run at the adagrad_eps of tests/exact_adagrad.py (1e-4) and lr = 0.01: there the
fp32 oracle alone stays within a tenth of fp32_close's tolerance of its fp64 copy
(test_exact_adagrad_cpu.py); the default eps = 1e-10 is pinned bit for bit by
test_gpu_adagrad_exact.py instead."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import exact_adagrad as A
import oracle as O
from conftest import fp32_close

pytestmark = pytest.mark.gpu
dev = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _cfg(name, **kw):
    from dlrm_hip.trainer import TrainerConfig
    _, op = A.TRAJ_CASES[name]
    t = A.TRAJ
    qr = {} if op is None else dict(qr_flag=True, qr_collisions=t["qr_collisions"],
                                   qr_operation=op, qr_threshold=t["qr_threshold"])
    base = dict(m_spa=t["D"], ln_emb=t["rows"], ln_bot=t["bot"], ln_top=A.traj_ln_top(),
                loss_function="bce", learning_rate=t["lr"], optimizer="adagrad",
                adagrad_eps=A.TRAJ_EPS[name])
    base.update(qr)
    base.update(kw)
    return TrainerConfig(**base)


def _close(got, want, what):
    ok, msg = fp32_close(got.detach().cpu().numpy(), want.detach().cpu().numpy())
    assert ok, (what, msg)


# ------------------------------------------------- (a) trajectories vs the oracle ----
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("name", sorted(A.TRAJ_CASES))
def test_adagrad_steps_vs_oracle(name, graph):
    """Three steps against oracle.OracleDLRM stepped by torch.optim.Adagrad on the CPU: Z, the
    loss, the tables, the dense parameters, table_sum and dense_adagrad_state, eager or
    replayed from a captured graph.  plain_onehot takes the gather-fused interaction,
    plain_multihot (L = 3) the pooled lookup."""
    from dlrm_hip.trainer import DLRMTrainer
    ref = A.traj_model(O, name)
    opt = torch.optim.Adagrad(ref.parameters(), lr=A.TRAJ["lr"], eps=A.TRAJ_EPS[name])
    tr = DLRMTrainer.from_oracle(_cfg(name), ref, device=dev)
    run = None
    for s, (X, lS_o, lS_i, T) in enumerate(A.traj_batches(name)):
        Zr, Er = A.oracle_step(ref, opt, X, lS_o, lS_i, T)
        b = tr.make_batch(X, lS_o, lS_i, T)
        if graph and s == 1:
            static = b
            run = tr.capture(static)
        if run is not None:
            for dst, src in zip((static.X, static.offsets, static.indices, static.target),
                                (b.X, b.offsets, b.indices, b.target)):
                dst.copy_(src)
            run()
            Z, E = tr._cur["prob"], tr._cur["loss"]
        else:
            Z, E = tr.step(b)
        print(f"{name} graph={graph} step {s}: Z {A.rel_diff(Z.cpu().numpy(), Zr.numpy().ravel()):.3e}"
              f" loss {A.rel_diff(E.cpu().numpy(), [Er.item()]):.3e}")
        _close(Z, Zr.ravel(), (s, "Z"))
        _close(E, Er.reshape(1), (s, "loss"))
        assert tr.gather_fused == (name == "plain_onehot")
    tr.check_errors()
    for k, e in enumerate(ref.emb_l):
        want = (e.weight_q, e.weight_r) if hasattr(e, "weight_q") else (e.weight,)
        got, gsum = tr.table(k), tr.table_sum(k)
        got = got if isinstance(got, tuple) else (got,)
        gsum = gsum if isinstance(gsum, tuple) else (gsum,)
        assert len(got) == len(gsum) == len(want)
        for g_, s_, w_ in zip(got, gsum, want):
            assert s_.shape == g_.shape == w_.shape
            _close(g_, w_, ("emb", k))
            _close(s_, opt.state[w_]["sum"], ("emb sum", k))
    lin = [m for seq in (ref.bot_l, ref.top_l) for m in seq if isinstance(m, torch.nn.Linear)]
    for i, ((W, b), (SW, Sb)) in enumerate(zip(tr.dense_state(), tr.dense_adagrad_state())):
        _close(W, lin[i].weight, ("W", i))
        _close(b, lin[i].bias, ("b", i))
        _close(SW, opt.state[lin[i].weight]["sum"], ("sum W", i))
        _close(Sb, opt.state[lin[i].bias]["sum"], ("sum b", i))


# ------------------------------------------------------ (b) bitwise in the engine ----
SMALL = dict(D=16, rows=[min(r, 5000) for r in O.KAGGLE_ROWS], bot=[13, 512, 256, 64, 16],
             top=[512, 256, 1], B=128)
RATES = (1e-3, 2e-3)  # (dense, embedding) base rates, as test_gpu_lr_trainer's rwsadagrad case
POLICY = (2, 3, 4)    # warm-up 2, decay from step 3 over 4 steps
STEPS = 8


def _small(precision="fp32", L=1, **kw):
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    c = SMALL
    F = len(c["rows"]) + 1
    cfg = TrainerConfig(m_spa=c["D"], ln_emb=c["rows"], ln_bot=c["bot"],
                        ln_top=[c["D"] + F * (F - 1) // 2] + c["top"], loss_function="bce",
                        learning_rate=RATES[0], emb_learning_rate=RATES[1], optimizer="adagrad",
                        mlp_precision=precision, **kw)
    tr = DLRMTrainer(cfg, device=dev, seed=3)
    return tr, tr.synthetic_batch(c["B"], L, seed=11)


def _state(tr):
    return [tr.weights, tr.emb_sum, tr.params, tr.adagrad_sum]


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


def _assert_same(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert _same(a, b), f"{what}: tensor {i} differs"


def _run(tr, batch, n, graph, before=None):
    """n steps, eager or as one captured graph replayed (after the eager step capture() needs,
    undone); ``before(i)`` runs ahead of step i.  Returns per-step (prob, loss) and the state."""
    run = None
    if graph:
        start = [t.clone() for t in _state(tr)]
        tr.step(batch)
        for dst, src in zip(_state(tr), start):
            dst.copy_(src)
        if tr.cfg.lr_mode == "device":
            tr.lr_step = 1
        run = tr.capture(batch)
    outs = []
    for i in range(n):
        if before is not None:
            before(i)
        if run is None:
            tr.step(batch)
        else:
            run()
        outs.append((tr._cur["prob"].clone(), tr._cur["loss"].clone()))
    tr.check_errors()
    return outs, [t.clone() for t in _state(tr)]


_BASE = {}


def _baseline(precision, L):
    """Eager steps at the host rate: built once per (precision, L), never changed."""
    if (precision, L) not in _BASE:
        tr, batch = _small(precision, L)
        assert tr.cfg.lr_mode == "host" and tr.emb_sum is not None and tr.momentum is None
        start = [t.clone() for t in _state(tr)]
        _BASE[(precision, L)] = _run(tr, batch, 3, False) + (start,)
    return _BASE[(precision, L)]


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_replayed_equals_eager_and_device_rate_equals_host_rate(precision, L):
    outs, state, start = _baseline(precision, L)
    assert not _same(state[0], start[0]) and not _same(state[1], start[1])  # it trained
    assert bool((start[1] == 0).all()) and bool((state[1] >= 0).all())
    for graph, device_lr in ((True, False), (False, True), (True, True)):
        tr, batch = _small(precision, L, device_lr=device_lr)
        assert tr.cfg.lr_mode == ("device" if device_lr else "host")
        o2, s2 = _run(tr, batch, 3, graph)
        what = f"graph={graph} device_lr={device_lr}"
        for (p, l), (pr, lr_) in zip(o2, outs):
            assert _same(p, pr) and _same(l, lr_), what
        _assert_same(s2, state, what)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_scheduled_lr_equals_the_host_driven_baseline(precision):
    """Warm-up 2, decay from step 3 over 4 steps, 8 steps: the device schedule, eager and
    replayed, against a host-rate trainer handed optim.lr_policy's rates before every step."""
    from dlrm_hip.optim import lr_policy
    host, batch = _small(precision)
    want, state = _run(host, batch, STEPS, False, before=lambda i: host.set_learning_rate(
        lr_policy(i + 1, RATES[0], *POLICY), lr_policy(i + 1, RATES[1], *POLICY)))
    W, S, D = POLICY
    for graph in (False, True):
        tr, batch = _small(precision, lr_num_warmup_steps=W, lr_decay_start_step=S,
                           lr_num_decay_steps=D)
        assert tr.cfg.lr_mode == "device"
        outs, s2 = _run(tr, batch, STEPS, graph)
        assert tr.lr_step == STEPS + 1
        for (p, l), (pr, lr_) in zip(outs, want):
            assert _same(p, pr) and _same(l, lr_), f"graph={graph}"
        _assert_same(s2, state, f"graph={graph}")


@pytest.mark.parametrize("L", [1, 3])
def test_bf16_step_updates_the_tables_as_the_kernel_on_its_own_de(L):
    """The mixed-precision step's embedding update is ops.tbe_backward('adagrad') on the dE
    that step produced: the engine adds nothing to the kernel."""
    from dlrm_hip import ops
    tr, batch = _small("bf16", L)
    tr.step(batch)  # a first step, so that the state is not all zeros
    W0, S0 = tr.weights.clone(), tr.emb_sum.clone()
    tr.step(batch)
    torch.cuda.synchronize()
    dE = tr._cur["dE"]
    ops.tbe_backward("adagrad", W0, tr.row_base, tr.T_phys, SMALL["B"], batch.indices,
                     batch.offsets, dE, lr=tr.emb_lr, eps=tr.cfg.adagrad_eps, momentum=S0,
                     grad_batch_stride=dE.stride(0), max_lookups_per_table=batch.max_per_table)
    torch.cuda.synchronize()
    assert _same(tr.weights, W0) and _same(tr.emb_sum, S0)
    assert bool((S0 > 0).any())


def test_sgd_and_rwsadagrad_allocate_no_element_state():
    from dlrm_hip.trainer import DLRMTrainer
    for optimizer in ("sgd", "rwsadagrad"):
        tr = DLRMTrainer(_cfg("plain_onehot", optimizer=optimizer), device=dev, seed=1)
        assert tr.emb_sum is None and (tr.momentum is not None) == (optimizer == "rwsadagrad")
        with pytest.raises(ValueError, match="not adagrad"):
            tr.table_sum(0)


# ------------------------------------------------------------------ (c) two ranks ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, W, port, q):
    try:
        sys.path[:0] = [ROOT, os.path.join(ROOT, "dlrm-yx_amd"), HERE]
        import torch.distributed as dist
        from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                                world_size=W)
        c = A.TWO_RANKS
        cfg = TrainerConfig(**A.TWO_RANKS_CFG, loss_function="bce", learning_rate=c["lr"],
                            sharder=c["sharder"], optimizer="adagrad", adagrad_eps=c["eps"])
        ref, _, data = A.two_ranks_setup(O)
        tr = DLRMTrainer.from_oracle(cfg, ref, device="cuda:0", rank=rank, world_size=W,
                                     process_group=dist.group.WORLD)
        res = {"Z": [], "E": [], "local": tr.local_tables}
        for X, lS_o, lS_i, T in data:
            Z, E = tr.step(tr.make_batch(X, lS_o, lS_i, T))
            res["Z"].append(Z.cpu().numpy())
            res["E"].append(float(E.cpu()))
        tr.check_errors()
        res["tables"] = {t: tr.table(t).cpu().numpy() for t in tr.local_tables}
        res["table_sum"] = {t: tr.table_sum(t).cpu().numpy() for t in tr.local_tables}
        res["dense"] = [(w.cpu().numpy(), b.cpu().numpy()) for w, b in tr.dense_state()]
        res["sum"] = [(w.cpu().numpy(), b.cpu().numpy()) for w, b in tr.dense_adagrad_state()]
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, res))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))


def test_two_ranks_match_oracle_distributed_step_with_adagrad():
    """W = 2 (gloo, one GPU): each rank updates its own tables and their sums; the dense
    Adagrad runs on the averaged bucket.  Against oracle.distributed_step handed
    torch.optim.Adagrad."""
    c = A.TWO_RANKS
    W = c["W"]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, W, port, q), daemon=True) for r in range(W)]
    for p in ps:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(W))
    for p in ps:
        p.join(timeout=60)
    for r in range(W):
        assert isinstance(res[r], dict), res[r]
    ref, di, data = A.two_ranks_setup(O)
    opt = torch.optim.Adagrad(ref.parameters(), lr=c["lr"], eps=c["eps"])
    for s, (X, lS_o, lS_i, T) in enumerate(data):
        Zs, Es = O.distributed_step(ref, W, di, X, lS_o, lS_i, T, c["lr"], optimizer=opt)
        for r in range(W):
            ok, msg = fp32_close(res[r]["Z"][s], Zs[r].numpy().ravel())
            assert ok, (s, r, msg)
            ok, msg = fp32_close(np.array([res[r]["E"][s]]), Es[r].numpy().reshape(1))
            assert ok, (s, r, msg)
    lin = [m for seq in (ref.bot_l, ref.top_l) for m in seq if isinstance(m, torch.nn.Linear)]
    seen = set()
    for r in range(W):
        for t, w in res[r]["tables"].items():
            assert di[t] == r
            seen.add(t)
            p = ref.emb_l[t].weight
            ok, msg = fp32_close(w, p.detach().numpy())
            assert ok, (r, t, msg)
            ok, msg = fp32_close(res[r]["table_sum"][t], opt.state[p]["sum"].numpy())
            assert ok, (r, "sum", t, msg)
        for i, ((w, b), (sw, sb)) in enumerate(zip(res[r]["dense"], res[r]["sum"])):
            for got, want in ((w, lin[i].weight.detach()), (b, lin[i].bias.detach()),
                              (sw, opt.state[lin[i].weight]["sum"]),
                              (sb, opt.state[lin[i].bias]["sum"])):
                ok, msg = fp32_close(got, want.numpy())
                assert ok, (r, i, msg)
    assert seen == set(range(len(A.TWO_RANKS_CFG["ln_emb"])))


# ------------------------------------------------------------------- (d) refusals ----
def test_refusals_and_table_sum_errors():
    from dlrm_hip.trainer import DLRMTrainer
    with pytest.raises(NotImplementedError, match="DESIGN.md §22"):
        _cfg("plain_onehot", emb_precision="fp16")
    for bad in ("adam", "Adagrad", "rowwise_adagrad"):
        with pytest.raises(ValueError, match="not supported"):
            DLRMTrainer(_cfg("plain_onehot", optimizer=bad), device=dev)
    tr = DLRMTrainer(_cfg("qr_mult"), device=dev, seed=1)
    assert tr.emb_sum.shape == tr.weights.shape and tr.emb_sum.dtype == torch.float32
    assert bool((tr.emb_sum == 0).all())
    with pytest.raises(ValueError, match="rwsadagrad"):
        tr.table_momentum(0)
    q, r = tr.table_sum(1)  # 5000 rows > qr_threshold: a (quotient, remainder) pair
    wq, wr = tr.table(1)
    assert q.shape == wq.shape and r.shape == wr.shape and r.shape[0] == A.TRAJ["qr_collisions"]
    assert tr.table_sum(0).shape == tr.table(0).shape
    with pytest.raises(ValueError):
        tr.table_sum(len(A.TRAJ["rows"]))  # no such local table
