"""DLRMTrainer's whole training step against exact_step.py's fp64 reference, BIT FOR BIT, in
every schedule the trainer can build: prob, every dense W and b, every table (each with a
sentinel row no index names), the row-wise momentum and the Adagrad sums; the loss by
exact_head's rule (exact for MSE; a BCE mean holds log 2 rows and is bounded as in
test_gpu_misc_exact.py).  Every case also asserts the path it means to reach - from the
trainer's own flags and from a record of the ops it called (launch roles ride on gemm_group
launches as a phase) - so a switch that silently falls back does not pass.

test_exact_step_cpu.py proves the reference, and that the tolerance of test_step_vs_oracle
admits errors this test cannot."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import exact_step as S

pytestmark = pytest.mark.gpu
dev = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LOSS_C = 4.0  # test_gpu_misc_exact.LOSS_C: logf's measured 2 ulp plus two roundings

SPIED = ["gemm_group", "tbe_forward_presort", "tbe_forward", "tbe_backward", "tbe_backward_defer",
         "tbe_backward_sort", "interact_forward_gather", "interact_forward",
         "interact_backward_gather", "interact_backward", "mlp_chain", "mlp_chain_forward",
         "qr_pool_combine_forward", "qr_pool_combine_backward", "sgd_update", "adagrad_update",
         "lr_schedule_tick", "head_step", "linear16_forward", "linear16_dgrad",
         "linear16_wgrad"]


class Spy:
    """Records the trainer's calls into dlrm_hip.ops: (name, detail).  gemm_group's detail is
    (phase of the role riding on the launch or 0, number of problems)."""

    def __init__(self, monkeypatch):
        from dlrm_hip import ops
        self.calls, self.recording = [], True
        for name in SPIED:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def wrapped(*a, **kw):
            if name == "gemm_group":
                detail = (kw.get("phase", 0) if kw.get("role") is not None else 0, len(a[0]))
            elif name == "tbe_forward_presort":
                detail = (kw.get("lookup", True), kw.get("bottom") is not None)
            elif name == "mlp_chain":
                detail = kw.get("parts", 1)
            elif name in ("tbe_backward", "tbe_backward_defer"):
                detail = (a[0], int(kw.get("presorted", 0)), kw.get("max_lookups_per_table", 0))
            else:
                detail = None
            if self.recording:
                self.calls.append((name, detail))
            return fn(*a, **kw)
        return wrapped

    def names(self):
        return [n for n, _ in self.calls]

    def phases(self):
        return [d[0] for n, d in self.calls if n == "gemm_group"]

    def roles(self):
        return [p for p in self.phases() if p]

    def detail(self, name):
        return [d for n, d in self.calls if n == name]


def _config(c, optimizer="sgd", **kw):
    from dlrm_hip.trainer import TrainerConfig
    m = c.model
    return TrainerConfig(m_spa=S.D, ln_emb=S.ROWS, ln_bot=S.ln_bot(c), ln_top=S.ln_top(c),
                         arch_interaction_itself=m.itself, loss_function=m.loss,
                         learning_rate=S.LR, emb_learning_rate=S.EMB_LR, optimizer=optimizer,
                         adagrad_eps=S.EPS, qr_flag=m.qr_op is not None, qr_collisions=S.QR_C,
                         qr_operation=m.qr_op or "mult", qr_threshold=S.QR_THRESHOLD, **kw)


def _trainer(c, optimizer="sgd", attrs=None, trainer_kw=None, **cfg_kw):
    from dlrm_hip.trainer import DLRMTrainer
    tr = DLRMTrainer.from_oracle(_config(c, optimizer, **cfg_kw), S.to_oracle(c), device=dev,
                                 **(trainer_kw or {}))
    for k, v in (attrs or {}).items():
        assert hasattr(tr, k), k
        setattr(tr, k, v)
    return tr


_STATE = ("weights", "params", "momentum", "emb_sum", "adagrad_sum", "grads")


def _snapshot(tr):
    return {k: getattr(tr, k).clone() for k in _STATE if getattr(tr, k) is not None}


def _restore(tr, snap):
    for k, v in snap.items():
        getattr(tr, k).copy_(v)


def _collect(tr, prob, loss):
    """Everything the step left behind, as numpy (this rank's tables)."""
    def flat(get):
        out = []
        for t in tr.local_tables:
            v = get(t)
            # fp16 tables: widened (exact), the reference's values are asserted exact in fp16
            out.append([x.float().cpu().numpy() for x in (v if isinstance(v, tuple) else (v,))])
        return out
    torch.cuda.synchronize()
    tr.check_errors()
    out = dict(prob=prob.cpu().numpy(), loss=loss.cpu().numpy(), local=list(tr.local_tables),
               dense=[(W.cpu().numpy(), b.cpu().numpy()) for W, b in tr.dense_state()],
               tables=flat(tr.table))
    if tr.momentum is not None:
        out["momentum"] = flat(tr.table_momentum)
    if tr.emb_sum is not None:
        out["table_sum"] = flat(tr.table_sum)
    if tr.adagrad_sum is not None:
        out["dense_sum"] = [(W.cpu().numpy(), b.cpu().numpy())
                            for W, b in tr.dense_adagrad_state()]
    return out


def _compare(c, r, out, rank=0, what=""):
    """``out`` (_collect) against reference ``r``: bits, everywhere."""
    Bl = c.B // c.W
    sl = slice(rank * Bl, (rank + 1) * Bl)
    bad = []
    if not S.bits_equal(out["prob"], r["prob"][sl]):
        bad.append("prob")
    for i, ((W0, b0), (W1, b1)) in enumerate(zip(r["dense"], out["dense"])):
        bad += [f"W{i}"] * (not S.bits_equal(W0, W1)) + [f"b{i}"] * (not S.bits_equal(b0, b1))
    fi = S.flat_index(c)
    for key in ("tables", "momentum", "table_sum"):
        if key not in out:
            assert not r[key], key
            continue
        for t, got in zip(out["local"], out[key]):
            for k, g in zip(fi[t], got):
                bad += [f"{key}[{t}]:{k}"] * (not S.bits_equal(r[key][k], g))
    if "dense_sum" in out:
        for i, ((W0, b0), (W1, b1)) in enumerate(zip(r["dense_sum"], out["dense_sum"])):
            bad += [f"sumW{i}"] * (not S.bits_equal(W0, W1))
            bad += [f"sumb{i}"] * (not S.bits_equal(b0, b1))
    assert not bad, (what, c.name, rank, bad)
    rl = r["row_loss"][sl]
    if S.loss_is_exact(c):
        assert S.bits_equal(out["loss"], r["loss"][rank:rank + 1]), (what, "loss")
    else:
        err = abs(float(out["loss"][0]) - rl.mean())
        assert err <= (Bl + LOSS_C) * 2.0 ** -24 * np.abs(rl).mean(), (what, "loss", err)


_REF = {}


def _reference(name, optimizer="sgd"):
    """Computed once per (variant, optimizer), shared and never changed."""
    if (name, optimizer) not in _REF:
        _REF[(name, optimizer)] = S.reference(S.build(name), optimizer)
    return _REF[(name, optimizer)]


def _step(monkeypatch, name, optimizer="sgd", attrs=None, graph=False, mpt=None,
          trainer_kw=None, **cfg_kw):
    """One eager step from the case's weights - and, ``graph``, the state restored, the step
    captured and replayed once - each compared with the reference.  Returns (trainer, spy of
    the eager step)."""
    c, r = S.build(name), _reference(name, optimizer)
    tr = _trainer(c, optimizer, attrs, trainer_kw, **cfg_kw)
    b = tr.make_batch(c.X, c.lS_o, c.lS_i, c.T)
    if mpt is not None:
        b.max_per_table = mpt
    snap = _snapshot(tr)
    spy = Spy(monkeypatch)
    prob, loss = tr.step(b)
    spy.recording = False  # the eager step's calls only, not the capture's
    print(f"{name} {optimizer} {attrs or ''} {cfg_kw or ''}: gather {tr.gather_fused} bottom "
          f"{tr.bottom_fused} launches {spy.phases()} "
          f"ops {[n for n in dict.fromkeys(spy.names()) if n != 'gemm_group']}")
    _compare(c, r, _collect(tr, prob, loss), what="eager")
    assert tr._roles == [], "a launch role was left pending"
    if graph:
        _restore(tr, snap)
        run = tr.capture(b)
        assert tr.capture_mode == "whole" and tr.graphs_per_step == 1
        _restore(tr, snap)
        torch.cuda.synchronize()
        run()
        _compare(c, r, _collect(tr, tr._cur["prob"], tr._cur["loss"]), what="replayed")
    return tr, spy


def _default_path(tr, spy, one_hot=True):
    """The one-GPU default: bottom MLP and sort inside the lookup launch, the interaction
    gathering one-hot rows itself, the head's finalize pass on the top backward's first
    launch, the embedding update's two passes on the bottom backward's first two."""
    assert tr.bottom_fused and tr.gather_fused == one_hot
    assert spy.detail("tbe_forward_presort") == [(not one_hot, True)]
    assert ("interact_forward_gather" in spy.names()) == one_hot
    assert ("interact_forward" in spy.names()) != one_hot
    assert spy.roles() == [4, 1, 2], spy.phases()
    assert "tbe_backward" not in spy.names() and "tbe_backward_defer" in spy.names()
    assert "sgd_update" not in spy.names()  # fused into the wgrad epilogues


# ------------------------------------------------------------------ one GPU: switches ----
@pytest.mark.parametrize("name", ["onehot", "multihot", "itself", "mse", "wide"])
def test_default_schedule(monkeypatch, name):
    tr, spy = _step(monkeypatch, name)
    _default_path(tr, spy, one_hot=S.build(name).L == 1)
    # bot_sched "auto" at B <= 128: "full", one launch per bottom layer
    if name == "wide":
        assert spy.phases()[-3:] == [1, 2, 0]
        assert spy.detail("mlp_chain")[0] == 4  # auto: four workgroups per row block
    else:
        assert spy.phases()[-2:] == [1, 2]


@pytest.mark.parametrize("op", ["mult", "add"])
def test_qr_tables(monkeypatch, op):
    tr, spy = _step(monkeypatch, "qr_" + op)
    assert tr.qr_active and tr.T_phys == 4 and not tr.gather_fused and tr.bottom_fused
    assert "qr_pool_combine_forward" in spy.names() and "qr_pool_combine_backward" in spy.names()
    assert spy.roles() == [4, 1, 2]


@pytest.mark.parametrize("fuse", [True, False])
def test_fuse_gather(monkeypatch, fuse):
    tr, spy = _step(monkeypatch, "onehot", attrs=dict(fuse_gather=fuse))
    assert tr.gather_fused == fuse
    assert ("interact_backward_gather" in spy.names()) == fuse
    assert ("interact_backward" in spy.names()) != fuse
    assert spy.detail("tbe_forward_presort") == [(not fuse, True)]


@pytest.mark.parametrize("fuse", [True, False])
def test_fuse_bottom(monkeypatch, fuse):
    tr, spy = _step(monkeypatch, "onehot", attrs=dict(fuse_bottom=fuse))
    assert tr.bottom_fused == fuse
    assert ("mlp_chain_forward" in spy.names()) is False  # never a launch of its own here
    assert spy.detail("tbe_forward_presort") == [(False, fuse)]
    # the bottom MLP as GEMM launches: two more of them, before the top MLP's
    assert len(spy.phases()) == (6 if fuse else 8), spy.phases()


@pytest.mark.parametrize("parts", [2, 4])
def test_bottom_parts(monkeypatch, parts):
    tr, spy = _step(monkeypatch, "wide", attrs=dict(bottom_parts=parts))
    assert tr.bottom_fused and spy.detail("mlp_chain") == [parts]


@pytest.mark.parametrize("sched", ["full", "partial"])
def test_bot_sched(monkeypatch, sched):
    tr, spy = _step(monkeypatch, "multihot", attrs=dict(bot_sched=sched))
    assert tr.bot_sched == sched and spy.roles() == [4, 1, 2]
    n_bottom = len(spy.phases()) - spy.phases().index(1)
    assert (n_bottom == 2) == (sched == "full"), spy.phases()


@pytest.mark.parametrize("role,at", [(True, (0, 1)), (True, (1, 2)), (False, (0, 1))])
def test_tbe_role(monkeypatch, role, at):
    tr, spy = _step(monkeypatch, "multihot", attrs=dict(tbe_role=role, tbe_role_at=at))
    if not role:
        assert spy.roles() == [4] and "tbe_backward_defer" not in spy.names()
        assert [d[0] for d in spy.detail("tbe_backward")] == ["sgd"]
    elif at == (0, 1):
        assert spy.phases()[-2:] == [1, 2]
    else:  # the block pass on the second bottom launch, the combine pass on an empty one
        assert spy.phases()[-3:] == [0, 1, 2]
        assert [d for n, d in spy.calls if n == "gemm_group"][-1] == (2, 0)


@pytest.mark.parametrize("role", [True, False])
def test_head_role(monkeypatch, role):
    tr, spy = _step(monkeypatch, "onehot", attrs=dict(head_role=role))
    assert spy.roles() == ([4, 1, 2] if role else [1, 2])


@pytest.mark.parametrize("early", [0, 1, 2])
def test_early_sort_and_unknown_max_per_table(monkeypatch, early):
    """batch.max_per_table = 0 (unknown): no per-table LDS sort, the device-wide sort - inside
    the backward (0), on the side stream before the lookup (1) or after it (2)."""
    tr, spy = _step(monkeypatch, "multihot", attrs=dict(early_sort=early), mpt=0)
    names = spy.names()
    assert not tr.gather_fused
    assert ("tbe_backward_sort" in names) == bool(early)
    if early:
        assert (names.index("tbe_backward_sort") < names.index("tbe_forward_presort")) \
            == (early == 1)
    bwd = spy.detail("tbe_backward_defer")
    assert len(bwd) == 1 and bwd[0][2] == 0


def test_unknown_max_per_table_one_hot(monkeypatch):
    tr, spy = _step(monkeypatch, "onehot", mpt=0)
    assert not tr.gather_fused and "tbe_backward_sort" in spy.names()


def test_feature_pad(monkeypatch):
    tr, spy = _step(monkeypatch, "multihot", attrs=dict(feature_pad=True))
    E = tr._cur["E"]
    assert E.stride(0) == 64 and E.shape == (64, 3, 16)  # 48 floats + 16 of padding
    assert tr.bottom_fused and spy.roles() == [4, 1, 2]


@pytest.mark.parametrize("conc", [False, True])
def test_concurrent(monkeypatch, conc):
    attrs = dict(concurrent=conc)
    if conc:
        attrs["overlaps"] = {"fwd", "top", "bot"}
    tr, spy = _step(monkeypatch, "multihot", attrs=attrs)
    if conc:  # bottom MLP beside the lookup, bottom backward beside the embedding backward
        assert not tr.bottom_fused and spy.detail("tbe_forward_presort") == [(True, False)]
        assert spy.roles() == [4] and "tbe_backward" in spy.names()
    else:
        _default_path(tr, spy, one_hot=False)


# ----------------------------------------------------------- optimizers, rates, graphs ----
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("optimizer", ["sgd", "rwsadagrad", "adagrad"])
@pytest.mark.parametrize("name", ["onehot", "multihot", "qr_mult"])
def test_optimizers_eager_and_replayed(monkeypatch, name, optimizer, graph):
    tr, spy = _step(monkeypatch, name, optimizer, graph=graph)
    names = spy.names()
    if optimizer == "sgd":
        assert "sgd_update" not in names and "adagrad_update" not in names
        assert spy.roles() == [4, 1, 2]
    else:  # gradient bucket + one dense Adagrad pass
        assert names.count("adagrad_update") == 1
        mode = "rowwise_adagrad" if optimizer == "rwsadagrad" else "adagrad"
        called = spy.detail("tbe_backward_defer" if optimizer == "rwsadagrad" else
                            "tbe_backward")
        assert [d[0] for d in called] == [mode]
        assert spy.roles() == ([4, 1, 2] if optimizer == "rwsadagrad" else [4])


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
def test_device_learning_rates(monkeypatch, optimizer, graph):
    """device_lr: the rates read from device memory.  LR != EMB_LR in every case of this
    file, so a swapped rate shows; here also through the device slots."""
    tr, spy = _step(monkeypatch, "multihot", optimizer, graph=graph, device_lr=True)
    assert tr.cfg.lr_mode == "device" and spy.names()[0] == "lr_schedule_tick"
    assert tr.current_lr() == [S.LR, S.EMB_LR, S.LR]


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("name", ["onehot", "multihot"])
def test_fp16_tables(monkeypatch, name, graph):
    """emb_precision="fp16", nearest rounding: exact_step.build asserts every table value,
    before and after the update, exact in fp16 - the same reference, the same bits."""
    tr, spy = _step(monkeypatch, name, graph=graph, emb_precision="fp16")
    assert tr.weights.dtype == torch.float16 and tr.gather_fused == (name == "onehot")
    assert [d[0] for d in spy.detail("tbe_backward")] == ["sgd_f16"] and spy.roles() == [4]


@pytest.mark.parametrize("optimizer,graph", [("sgd", False), ("sgd", True), ("rwsadagrad", False)])
@pytest.mark.parametrize("name", ["onehot", "multihot", "itself"])
def test_bf16_mlp(monkeypatch, name, optimizer, graph):
    """mlp_precision="bf16": exact_step.build asserts every operand of an MLP GEMM below the
    head is at most 256 quanta, exact in bf16; the accumulation is fp32 - the same bits."""
    assert S.build(name).operand <= 256
    tr, spy = _step(monkeypatch, name, optimizer, graph=graph, mlp_precision="bf16")
    n = len(tr.layers) - 1  # every Linear below the head; the bottom MLP's first has no dgrad
    names = spy.names()
    assert "gemm_group" not in names and not tr.bottom_fused
    assert (names.count("linear16_forward"), names.count("linear16_dgrad"),
            names.count("linear16_wgrad")) == (n, n - 1, n)


def test_swapped_rates_differ():
    """The reference itself separates the two rates (no GPU work: guards the cases above)."""
    c = S.build("onehot")
    a, b = S.reference(c), S.reference(c, lr=S.EMB_LR, emb_lr=S.LR)
    assert len(S.state_equal(a, b["dense"], b["tables"])) == 2 * 5 + 3


# -------------------------------------------------------- the multi-GPU schedule ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# Eager steps only.  A capture in this process raced ProcessGroupNCCL's watchdog thread: it
# polls the events of the eager step's collectives every 100 ms, an event query from any thread
# is refused while another captures in the default "global" mode, and the watchdog then ends
# the process (seen once in four runs of a captured case here).  The captured multi-GPU
# schedule is compared bitwise in test_two_ranks (gloo: no device events) and, against the
# single-GPU schedule, in test_gpu_dist.py.
ONE_RANK_RUNS = [("onehot", "sgd"), ("multihot", "sgd"), ("qr_mult", "rwsadagrad"),
                 ("multihot", "adagrad"), ("itself", "sgd")]


def _one_rank_worker(port, q):
    """force_dist on a 1-rank RCCL group: all-to-all, gradient buckets, all-reduces."""
    try:
        sys.path[:0] = [ROOT, os.path.join(ROOT, "dlrm-yx_amd"), HERE]
        import torch.distributed as dist
        d = torch.device("cuda", 0)
        torch.cuda.set_device(d)
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0,
                                world_size=1, device_id=d)
        res = []
        for name, optimizer in ONE_RANK_RUNS:
            c = S.build(name)
            tr = _trainer(c, optimizer, trainer_kw=dict(force_dist=True,
                                                        process_group=dist.group.WORLD))
            assert tr.distributed and tr.grads is not None
            assert dist.get_backend(tr.comm.pg) == dist.get_backend(tr.comm.dense_pg) == "nccl"
            prob, loss = tr.step(tr.make_batch(c.X, c.lS_o, c.lS_i, c.T))
            res.append(_collect(tr, prob, loss))
        dist.destroy_process_group()
        q.put(res)
    except Exception:  # pragma: no cover
        import traceback
        q.put(traceback.format_exc())


def test_multi_gpu_schedule_on_one_rank():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_one_rank_worker, args=(_free_port(), q), daemon=True)
    p.start()
    res = q.get(timeout=300)
    p.join(timeout=60)
    assert isinstance(res, list), res
    assert len(res) == len(ONE_RANK_RUNS)
    for (name, optimizer), out in zip(ONE_RANK_RUNS, res):
        _compare(S.build(name), _reference(name, optimizer), out, what=("one rank", optimizer))


TWO_RANK_RUNS = [("two_ranks", "sgd", False), ("two_ranks_multihot", "sgd", True),
                 ("two_ranks_qr", "rwsadagrad", False), ("two_ranks_multihot", "adagrad", False)]


def _two_rank_worker(rank, port, q):
    try:
        sys.path[:0] = [ROOT, os.path.join(ROOT, "dlrm-yx_amd"), HERE]
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                                world_size=2)
        res = []
        for name, optimizer, graph in TWO_RANK_RUNS:
            c = S.build(name)
            tr = _trainer(c, optimizer, allocation=S.DI2,
                          trainer_kw=dict(rank=rank, world_size=2,
                                          process_group=dist.group.WORLD))
            assert tr.feature_order == S.ORDER2
            b = tr.make_batch(c.X, c.lS_o, c.lS_i, c.T)
            snap = _snapshot(tr)
            prob, loss = tr.step(b)
            out = [_collect(tr, prob, loss)]
            if graph:
                _restore(tr, snap)
                run = tr.capture(b)
                _restore(tr, snap)
                torch.cuda.synchronize()
                dist.barrier()
                run()
                bufs = tr._bufs[(b.X.shape[0], b.X.shape[0] * 2)]
                out.append(_collect(tr, bufs["prob"], bufs["loss"]))
            res.append(out)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, res))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))


def test_two_ranks():
    """Two ranks sharing the GPU over gloo (test_gpu_dist.py's worker pattern) against the
    reference of oracle.distributed_step's semantics: rank-major feature order [0, 2, 1], W x
    embedding gradients, averaged dense gradients, each rank's loss over its own rows."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_two_rank_worker, args=(r, port, q), daemon=True) for r in range(2)]
    for p in ps:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(2))
    for p in ps:
        p.join(timeout=60)
    for rank in range(2):
        assert isinstance(res[rank], list), res[rank]
        for (name, optimizer, graph), outs in zip(TWO_RANK_RUNS, res[rank]):
            assert len(outs) == 1 + graph
            assert outs[0]["local"] == [t for t in range(3) if S.DI2[t] == rank]
            for out in outs:
                _compare(S.build(name), _reference(name, optimizer), out, rank=rank,
                         what=("two ranks", optimizer))
