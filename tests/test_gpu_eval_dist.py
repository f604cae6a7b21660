"""The forward-only path on the multi-GPU schedule: two gloo ranks sharing one GPU (each
logs its own B/W samples; EvalState.compute(group) returns the same numbers on both), and
the one-rank force_dist schedule against the single-GPU path."""
import os
import queue
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEADLINE_S = 240


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fixture_trainer(rank, W, pg, **kw):
    import dist_fixture as DF
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    g = DF.load()
    cfg = TrainerConfig(**DF.config(g), loss_function="bce", learning_rate=float(g["lr"][0]),
                        sharder="greedy")
    tr = DLRMTrainer(cfg, device="cuda:0", rank=rank, world_size=W, process_group=pg,
                     init=False, **kw)
    tr.load_dense(DF.init_mlp(g), DF.init_tables(g))
    data = [(X.numpy(), lS_o.numpy(), [i.numpy() for i in lS_i], T.numpy())
            for X, lS_o, lS_i, T in DF.batches(g)]
    return tr, data


def _two_rank_worker(rank, W, port, q):
    try:
        sys.path[:0] = [ROOT, os.path.join(ROOT, "dlrm-yx_amd"), HERE]
        import torch.distributed as dist
        from dlrm_hip import metrics
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                                world_size=W)
        tr, data = _fixture_trainer(rank, W, dist.group.WORLD)
        batches = [tr.make_batch(*d) for d in data]
        Bl = batches[0].X.shape[0]
        st = metrics.EvalState(len(batches) * Bl, "cuda:0")
        res = {"prob": [], "order": tr.feature_order}
        for i, b in enumerate(batches):
            if i == 0:  # eager, logged by the head
                prob = tr.predict(b, metrics=st)
            else:  # captured segments around the eager all-to-all
                tr.predict(b)
                torch.cuda.synchronize()
                tr.capture_predict(b, metrics=st)()
                prob = tr.predict(b)
            res["prob"].append(prob.cpu().numpy().copy())
        tr.check_errors()
        res["count"] = st.count
        res["dict"] = st.compute(group=dist.group.WORLD)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, res))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))


def _one_rank_worker(rank, W, port, q):
    try:
        sys.path[:0] = [ROOT, os.path.join(ROOT, "dlrm-yx_amd"), HERE]
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0,
                                world_size=1)
        res = {}
        for name, kw in (("single", {}), ("dist", dict(force_dist=True))):
            tr, data = _fixture_trainer(0, 1, dist.group.WORLD if kw else None, **kw)
            assert tr.distributed == bool(kw)
            res[name] = [tr.predict(tr.make_batch(*d)).cpu().numpy().copy() for d in data]
            tr.check_errors()
        dist.destroy_process_group()
        q.put((rank, res))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))


def _spawn(target, W):
    """Run W workers; a worker that dies without reporting fails the test at once."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=target, args=(r, W, port, q), daemon=True) for r in range(W)]
    for p in ps:
        p.start()
    res = {}
    t0 = time.monotonic()
    try:
        while len(res) < W:
            try:
                r, v = q.get(timeout=0.5)
                res[r] = v
                assert isinstance(v, dict), v
            except queue.Empty:
                dead = [p.exitcode for p in ps if p.exitcode not in (None, 0)]
                assert not dead, f"a worker died with exit code {dead}"
                if all(p.exitcode == 0 for p in ps) and q.empty():
                    raise AssertionError("the workers exited without reporting")
                assert time.monotonic() - t0 < DEADLINE_S, "workers timed out"
    finally:
        for p in ps:
            p.join(timeout=0.1 if len(res) < W else 60)
            if p.is_alive():
                p.kill()
    return res


def _oracle_rank_forward(W, order):
    """The oracle's forward on each rank's batch slice, features in the rank-major order the
    all-to-all delivers (OracleDLRM.forward with the reference's distributed feature order:
    oracle.distributed_step's forward half)."""
    import dist_fixture as DF
    import oracle as O
    g = DF.load()
    c = DF.config(g)
    ref = O.OracleDLRM(c["m_spa"], c["ln_emb"], c["ln_bot"], c["ln_top"], loss_function="bce",
                       tables=DF.init_tables(g))
    lin = [m for seq in (ref.bot_l, ref.top_l) for m in seq if isinstance(m, torch.nn.Linear)]
    for m, (Wt, b) in zip(lin, DF.init_mlp(g)):
        m.weight.data = torch.tensor(Wt)
        m.bias.data = torch.tensor(b)
    out = []
    with torch.no_grad():
        for X, lS_o, lS_i, T in DF.batches(g):
            ly = [ref.emb_l[t](lS_i[t], lS_o[t]) for t in range(len(ref.emb_l))]
            per_rank = []
            for s in range(W):
                sl = O.get_my_slice(X.shape[0], s, W)
                z = O.interact(ref.bot_l(X[sl]), [ly[t][sl] for t in order], ref.op, ref.itself)
                per_rank.append((ref.top_l(z).numpy().ravel(), T[sl].numpy().ravel()))
            out.append(per_rank)
    return out


def test_two_ranks_predict_and_gathered_metrics():
    import eval_ref
    from conftest import fp32_close
    W = 2
    res = _spawn(_two_rank_worker, W)
    assert res[0]["order"] == res[1]["order"]
    want = _oracle_rank_forward(W, res[0]["order"])
    probs, labs = [], []
    for s, per_rank in enumerate(want):
        for r, (p_ref, t) in enumerate(per_rank):
            ok, msg = fp32_close(res[r]["prob"][s], p_ref)
            assert ok, (s, r, msg)
            probs.append(res[r]["prob"][s])
            labs.append(t)
    n = sum(p.size for p in probs)
    assert res[0]["count"] + res[1]["count"] == n
    assert res[0]["dict"] == res[1]["dict"]  # identical on both ranks
    mine = eval_ref.full(np.concatenate(probs), np.concatenate(labs))
    d = res[0]["dict"]
    for k in ("tp", "fp", "tn", "fn", "n_pos", "n_neg"):
        assert d[k] == mine[k], k
    assert d["auc_num2"] == mine["a2"] and d["roc_auc"] == mine["roc_auc"]
    assert abs(d["ap"] - mine["ap"]) <= 1e-12


def test_force_dist_one_rank_matches_single_gpu_path():
    from conftest import fp32_close
    res = _spawn(_one_rank_worker, 1)[0]
    for a, b in zip(res["dist"], res["single"]):
        ok, msg = fp32_close(a, b)
        assert ok, msg
