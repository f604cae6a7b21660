"""The evaluation path on the GPU: the device metrics against the numpy reference
(eval_ref), the forward-only head against the training head, DLRMTrainer.predict against
the oracle's forward, and the promise that predicting never touches training state."""
import numpy as np
import pytest
import torch

import eval_ref
import oracle as O
from conftest import fp32_close

pytestmark = pytest.mark.gpu
dev = "cuda:0"


def _mods():
    from dlrm_hip import metrics, ops
    return metrics, ops


def _u32(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _bits_equal(a, b):
    return a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32),
                                                               b.view(torch.int32))


def _ap(out):
    return float(out.cpu().numpy().view(np.float64)[4])


def _ints(out):
    a2, p, n, groups, _ = out.cpu().tolist()
    return dict(a2=a2, n_pos=p, n_neg=n, groups=groups)


def _counts(st):
    c = st.ctrl.cpu().tolist()
    return dict(tp=c[1], fp=c[2], tn=c[3], fn=c[4])


def _same_ints(got, ref, keys):
    for k in keys:
        assert got[k] == ref[k], (k, got[k], ref[k])


def _cases():
    from dlrm_hip import ops
    return eval_ref.auc_ap_inputs(ops.EVAL_SORT_TILE)


_REF = {}


def _ref(name, prob, lab):  # computed once per input, shared by the tests
    if name not in _REF:
        _REF[name] = eval_ref.full(prob, lab)
    return _REF[name]


CASE_NAMES = ["n1", "n2", "n63", "n64", "n65", "n255", "n256", "n257", "n4095", "n4096", "n4097",
              "distinct", "quant8", "equal", "half"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_update_and_metrics_vs_ref(name):
    metrics, ops = _mods()
    cases = {c[0]: c for c in _cases()}
    assert sorted(cases) == sorted(CASE_NAMES)
    _, prob, lab = cases[name]
    ref = _ref(name, prob, lab)
    n = prob.size
    st = metrics.EvalState(n, dev)
    st.update(torch.tensor(prob, device=dev), torch.tensor(lab, device=dev))
    assert st.count == n
    assert np.array_equal(_u32(st.keys), eval_ref.pack_keys(prob, lab))  # log order
    _same_ints(_counts(st), ref, ("tp", "fp", "tn", "fn"))
    outs = []
    for _ in range(2):
        keys = st.keys.clone()
        out = ops.eval_metrics(keys)
        assert np.array_equal(_u32(keys), ref["sorted"])
        _same_ints(_ints(out), ref, ("a2", "n_pos", "n_neg", "groups"))
        ap = _ap(out)
        print(name, "ap", repr(ap), "ref", repr(ref["ap"]), "diff", abs(ap - ref["ap"]))
        assert abs(ap - ref["ap"]) <= 1e-12
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])  # bitwise-equal ap (and integers)
    if name == "n1":
        with pytest.raises(ValueError):
            st.compute()
        return
    res = st.compute()
    _same_ints(res, ref, ("tp", "fp", "tn", "fn", "n_pos", "n_neg"))
    assert res["auc_num2"] == ref["a2"]
    assert res["roc_auc"] == ref["roc_auc"]
    assert abs(res["ap"] - ref["ap"]) <= 1e-12
    for k in ("recall", "precision", "f1", "accuracy"):
        assert res[k] == ref[k], k
    if name == "equal":
        assert res["auc_num2"] == res["n_pos"] * res["n_neg"] and res["roc_auc"] == 0.5
    assert np.array_equal(_u32(st.keys), ref["sorted"])  # compute sorts the log in place


@pytest.mark.parametrize("name", eval_ref.BIG_NAMES)
def test_metrics_many_tiles_per_workgroup(name):
    """More than kMaxSortWgs tiles: every sort workgroup walks a run of tiles, so the tile
    loops of sort_hist_kernel / sort_scatter_kernel, the carry of each digit's destination
    from a workgroup's tile to its next, hist_row_scan_kernel with hundreds of live entries
    and scan_u32_kernel / group_final_kernel with more than 256 tiles (a chunk above 1, more
    than one partial per thread) all run.  Integers and sorted keys are exact."""
    metrics, ops = _mods()
    tile = ops.EVAL_SORT_TILE
    prob, lab = eval_ref.big_input(name, tile)
    n = prob.size
    ntiles, per_wg, wgs = eval_ref.sort_plan(n, tile)
    assert (ntiles, per_wg, wgs) == dict(big_distinct=(1025, 2, 513), big_ties=(1025, 2, 513),
                                         big_three=(2052, 3, 684))[name]
    assert ntiles == -(-n // tile) > 1024 and per_wg > 1 and (ntiles - 1) // per_wg == wgs - 1
    ref = _ref(name, prob, lab)
    if name == "big_distinct":
        assert ref["groups"] == n
    st = metrics.EvalState(n, dev)
    st.update(torch.tensor(prob, device=dev), torch.tensor(lab, device=dev))  # one call
    assert st.count == n
    _same_ints(_counts(st), ref, ("tp", "fp", "tn", "fn"))
    assert np.array_equal(_u32(st.keys), eval_ref.pack_keys(prob, lab))  # log order
    # |ap - ap_fsum| <= (h + 8) 2^-53 ap_fsum.  h = 32 + ceil(ntiles / 256) is the deepest
    # addition chain of the device's fixed-order sum: a thread adds its 16 terms serially,
    # an 8-level tree joins the tile's 256 threads, then a thread adds ceil(ntiles / 256) tile
    # partials serially and another 8-level tree follows; every term is non-negative, so each
    # addition costs at most 2^-53 of the total.  Each term carries three roundings (two
    # divisions and a product) on the device and three in the reference: 6; fsum rounds
    # once: 1/2; the rest is slack for the second-order terms.
    h = 32 + -(-ntiles // 256)
    bound = (h + 8) * 2.0 ** -53 * ref["ap_fsum"]
    outs = []
    for _ in range(2):
        keys = st.keys.clone()
        out = ops.eval_metrics(keys)
        assert np.array_equal(_u32(keys), ref["sorted"])
        _same_ints(_ints(out), ref, ("a2", "n_pos", "n_neg", "groups"))
        ap = _ap(out)
        print(name, "ap", repr(ap), "ref", repr(ref["ap"]), "diff", abs(ap - ref["ap"]),
              "fsum", repr(ref["ap_fsum"]), "diff", abs(ap - ref["ap_fsum"]), "bound", bound)
        assert abs(ap - ref["ap"]) <= 1e-12
        assert abs(ap - ref["ap_fsum"]) <= bound
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])  # two runs: bitwise-equal ap and integers


def test_appending_in_pieces():
    metrics, ops = _mods()
    _, prob, lab = [c for c in _cases() if c[0] == "distinct"][0]
    ref = _ref("distinct", prob, lab)
    p, t = torch.tensor(prob, device=dev), torch.tensor(lab, device=dev)
    st = metrics.EvalState(prob.size, dev)
    for i in range(35):
        st.update(p[2000 * i:2000 * (i + 1)], t[2000 * i:2000 * (i + 1)])
    st.update(p[70000:], t[70000:])
    assert st.count == 70001
    _same_ints(_counts(st), ref, ("tp", "fp", "tn", "fn"))
    out = ops.eval_metrics(st.keys)
    _same_ints(_ints(out), ref, ("a2", "n_pos", "n_neg", "groups"))
    assert np.array_equal(_u32(st.keys), ref["sorted"])


def test_module_front_end_logs_through_eval_update():
    """DLRM_Net.log_eval (the reference driver's Z_test / T_test, [B, 1] tensors with
    autograd history) logs what EvalState.update logs."""
    metrics, _ = _mods()
    from dlrm_hip.dlrm_net import DLRM_Net
    rng = np.random.RandomState(8)
    prob = rng.rand(300, 1).astype(np.float32)
    lab = (rng.rand(300, 1) < 0.3).astype(np.float32)
    Z = torch.tensor(prob, device=dev, requires_grad=True) * 1.0
    st = metrics.EvalState(300, dev)
    DLRM_Net.log_eval(st, Z, torch.tensor(lab, device=dev))
    ref = eval_ref.full(prob, lab)
    res = st.compute()
    _same_ints(res, ref, ("tp", "fp", "tn", "fn", "n_pos", "n_neg"))
    assert res["auc_num2"] == ref["a2"] and abs(res["ap"] - ref["ap"]) <= 1e-12


SENT = -0x12345678


def _guarded_state(cap):
    metrics, _ = _mods()
    big = torch.full((cap + 128,), SENT, dtype=torch.int32, device=dev)
    return big, metrics.EvalState(cap, dev, keys=big[64:64 + cap])


def _sentinels_intact(big, cap):
    b = big.cpu().numpy()
    return bool((b[:64] == SENT).all() and (b[64 + cap:] == SENT).all())


def test_guard_overflow_then_reset():
    rng = np.random.RandomState(5)
    prob = rng.rand(128).astype(np.float32)
    lab = (rng.rand(128) < 0.3).astype(np.float32)
    p, t = torch.tensor(prob, device=dev), torch.tensor(lab, device=dev)
    big, st = _guarded_state(100)
    st.update(p[:64], t[:64])
    st.update(p[64:], t[64:])  # 128 > 100: refused as a whole
    assert st.count == 64
    assert np.array_equal(_u32(st.keys[:64]), eval_ref.pack_keys(prob[:64], lab[:64]))
    assert (st.keys[64:].cpu().numpy() == SENT).all()
    with pytest.raises(OverflowError):
        st.compute()
    assert _sentinels_intact(big, 100)
    st.reset()
    st.update(p[64:], t[64:])
    ref = eval_ref.full(prob[64:], lab[64:])
    res = st.compute()
    _same_ints(res, ref, ("tp", "fp", "tn", "fn", "n_pos", "n_neg"))
    assert res["auc_num2"] == ref["a2"]
    assert _sentinels_intact(big, 100)


@pytest.mark.parametrize("bad", ["nan", "above", "below", "label"])
def test_guard_bad_rows(bad):
    rng = np.random.RandomState(6)
    prob = rng.rand(64).astype(np.float32)
    lab = (rng.rand(64) < 0.3).astype(np.float32)
    if bad == "label":
        lab[17] = 0.3
    else:
        prob[17] = dict(nan=np.nan, above=1.0000001, below=-1e-9)[bad]
    big, st = _guarded_state(100)
    st.update(torch.tensor(prob, device=dev), torch.tensor(lab, device=dev))
    with pytest.raises(ValueError):
        st.compute()
    keep = np.arange(64) != 17
    good = eval_ref.confusion(prob[keep], lab[keep])
    assert tuple(_counts(st).values()) == good  # the bad row is not counted
    assert int(st.keys[17]) == SENT              # ... and not logged
    assert _sentinels_intact(big, 100)


@pytest.mark.parametrize("clamp", [0.0, 0.01])
@pytest.mark.parametrize("K", [1, 2, 64, 65, 257, 1024])
def test_head_predict_bitwise_head_step(K, clamp):
    metrics, ops = _mods()
    rng = np.random.RandomState(100 + K)
    for M in (1, 3, 4, 5, 257):
        X = torch.tensor((rng.randn(M, K) * (4.0 / np.sqrt(K))).astype(np.float32), device=dev)
        w = torch.tensor(rng.randn(K).astype(np.float32), device=dev)
        t = torch.tensor((rng.rand(M) < 0.3).astype(np.float32), device=dev)
        w_train = w.clone()
        ref_prob = torch.empty(M, dtype=torch.float32, device=dev)
        ops.head_step(X.clone(), w_train, t, "bce", clamp, 1.0, prob=ref_prob,
                      loss_out=torch.zeros(1, device=dev), relu_mask=False, lr=0.1)
        prob = ops.head_predict(X, w, clamp)
        assert _bits_equal(prob, ref_prob), (M, K, clamp)
        st = metrics.EvalState(M + 3, dev)
        w_before = w.clone()
        prob2 = ops.head_predict(X, w, clamp, target=t, state=st)
        assert _bits_equal(prob2, ref_prob) and torch.equal(w, w_before)
        assert st.count == M
        pn, tn_ = prob2.cpu().numpy(), t.cpu().numpy()
        assert np.array_equal(_u32(st.keys[:M]), eval_ref.pack_keys(pn, tn_))
        assert tuple(_counts(st).values()) == eval_ref.confusion(pn, tn_)
        ops.head_predict(X, w, clamp, target=t, state=st)  # M more rows: M + 3 < 2 M for M > 3
        assert st.count == (2 * M if 2 * M <= M + 3 else M)


# ------------------------------------------------------------------ the trainer --
CASES = {  # the shapes of test_gpu_trainer.py's CASES
    "c3_small": dict(D=128, rows=[min(r, 2000) for r in O.TERABYTE_ROWS], bot=[13, 512, 256, 128],
                     top=[1024, 1024, 512, 256, 1], B=256, L=1, loss="bce", lr=0.1),
    "c1_small": dict(D=64, rows=[20000] * 8, bot=[512, 512, 64], top=[1024, 1024, 1024, 1],
                     B=128, L=100, loss="mse", lr=0.1),
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


def _oracle_forward(ref, X, lS_o, lS_i):
    with torch.no_grad():
        return ref(torch.tensor(X), torch.tensor(lS_o),
                   [torch.tensor(i) for i in lS_i]).numpy().ravel()


def _make(name, itself=False, seed=7, threshold=0.0, **cfg_kw):
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    c = CASES[name]
    D, rows = c["D"], c["rows"]
    ln_top = [_num_int(len(rows), D, itself)] + c["top"]
    np.random.seed(seed)
    ref = O.OracleDLRM(D, rows, c["bot"], ln_top, arch_interaction_itself=itself,
                       loss_function=c["loss"], loss_threshold=threshold)
    cfg = TrainerConfig(m_spa=D, ln_emb=rows, ln_bot=c["bot"], ln_top=ln_top,
                        arch_interaction_itself=itself, loss_function=c["loss"],
                        loss_threshold=threshold, learning_rate=c["lr"], **cfg_kw)
    return c, ref, DLRMTrainer.from_oracle(cfg, ref, device=dev)


VARIANTS = {
    "c3_small": ("c3_small", {}, {}),
    "c1_small": ("c1_small", {}, {}),
    "c2_small": ("c2_small", {}, {}),
    "c2_itself": ("c2_small", dict(itself=True), {}),
    "c2_clamp": ("c2_small", dict(threshold=0.3), {}),
    # the pooled lookup (no gather fusion), the bottom MLP as GEMMs on the side stream
    "c2_lookup_overlap": ("c2_small", {}, dict(fuse_gather=False, fuse_bottom=False,
                                               overlaps={"fwd"})),
    "c3_lookup": ("c3_small", {}, dict(fuse_gather=False)),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_predict_vs_oracle(variant):
    name, mk, attrs = VARIANTS[variant]
    c, ref, tr = _make(name, **mk)
    for k, v in attrs.items():
        setattr(tr, k, v)
    rng = np.random.RandomState(3)
    for _ in range(2):
        X, lS_o, lS_i, T = _rand_batch(rng, c["rows"], c["B"], c["L"], c["bot"][0], c["loss"])
        batch = tr.make_batch(X, lS_o, lS_i, T)
        assert tr._gather_applies(batch) == (c["L"] == 1 and attrs.get("fuse_gather", True))
        prob = tr.predict(batch)
        ok, msg = fp32_close(prob.cpu().numpy(), _oracle_forward(ref, X, lS_o, lS_i))
        assert ok, (variant, msg)
    tr.check_errors()


@pytest.mark.parametrize("op", ["mult", "add"])
def test_predict_qr_vs_oracle(op):
    """QR tables (the C4 model), as test_gpu_trainer.py::test_qr_step_vs_oracle builds it."""
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    D, B, c, thr = 32, 256, 4, 200
    rows = [3, 5000, 150, 201, 2000, 64, 1000, 7]
    bot, top = [13, 64, 32], [64, 1]
    ln_top = [_num_int(len(rows), D)] + top
    np.random.seed(11)
    ref = O.OracleDLRM(D, rows, bot, ln_top, loss_function="bce")
    torch.manual_seed(5)
    for k, n in enumerate(rows):
        if n > thr:
            ref.emb_l[k] = O.QREmbeddingBagOracle(n, D, c, op)
    cfg = TrainerConfig(m_spa=D, ln_emb=rows, ln_bot=bot, ln_top=ln_top, loss_function="bce",
                        learning_rate=0.05, qr_flag=True, qr_collisions=c, qr_operation=op,
                        qr_threshold=thr)
    tr = DLRMTrainer.from_oracle(cfg, ref, device=dev)
    assert tr.qr_active
    X, lS_o, lS_i, T = _rand_batch(np.random.RandomState(3), rows, B, 1, bot[0], "bce")
    prob = tr.predict(tr.make_batch(X, lS_o, lS_i, T))
    ok, msg = fp32_close(prob.cpu().numpy(), _oracle_forward(ref, X, lS_o, lS_i))
    assert ok, msg
    tr.check_errors()


def _state(tr):
    parts = [tr.weights, tr.params]
    for extra in (tr.momentum, tr.adagrad_sum, tr.grads):
        if extra is not None:
            parts.append(extra)
    return [p.clone() for p in parts]


@pytest.mark.parametrize("optimizer", ["sgd", "rwsadagrad"])
def test_predict_leaves_state_untouched(optimizer):
    c, ref, tr = _make("c2_small", optimizer=optimizer)
    rng = np.random.RandomState(4)
    batches = [tr.make_batch(*_rand_batch(rng, c["rows"], c["B"], 1, c["bot"][0], "bce"))
               for _ in range(2)]
    tr.step(batches[0])  # non-trivial optimizer state and gradient buffers
    before = _state(tr)
    assert len(before) == (2 if optimizer == "sgd" else 5)
    for b in (batches[1], batches[0], batches[1]):
        tr.predict(b)
    torch.cuda.synchronize()
    for a, b in zip(before, _state(tr)):
        assert torch.equal(a, b)
    assert tr._roles == [] and tr.step_count == 1


def test_predict_between_training_graph_replays():
    """The --test-freq pattern: a captured training graph stays valid when predict (eager
    and captured) runs between its replays."""
    out = {}
    for who in ("A", "B"):
        c, ref, tr = _make("c2_small")
        rng = np.random.RandomState(4)
        train = tr.make_batch(*_rand_batch(rng, c["rows"], c["B"], 1, c["bot"][0], "bce"))
        test = tr.make_batch(*_rand_batch(rng, c["rows"], c["B"], 1, c["bot"][0], "bce"))
        tr.step(train)
        torch.cuda.synchronize()
        replay = tr.capture(train)
        replay()
        if who == "B":
            first = tr.predict(test).clone()
            torch.cuda.synchronize()
            run = tr.capture_predict(test)
            for _ in range(2):
                run()
            assert torch.equal(tr.predict(test), first)
        replay()
        prob = tr._bufs[(c["B"], c["B"])]["prob"].clone()
        torch.cuda.synchronize()
        out[who] = (prob, tr.weights.clone(), tr.params.clone())
        assert tr.step_count == 3
    for a, b in zip(out["A"], out["B"]):
        assert torch.equal(a, b)


def test_capture_predict_appends_on_every_replay():
    metrics, _ = _mods()
    c, ref, tr = _make("c2_small")
    B = c["B"]
    rng = np.random.RandomState(9)
    batch = tr.make_batch(*_rand_batch(rng, c["rows"], B, 1, c["bot"][0], "bce"))
    eager = tr.predict(batch).clone()
    st_e = metrics.EvalState(5 * B, dev)
    for _ in range(5):
        st_e.update(tr.predict(batch), batch.target)
    torch.cuda.synchronize()
    st = metrics.EvalState(5 * B + 7, dev)
    run = tr.capture_predict(batch, metrics=st)
    assert st.count == 0  # capturing logs nothing
    for _ in range(5):
        run()
    assert st.count == 5 * B
    assert torch.equal(tr.predict(batch), eager)
    keys1 = eval_ref.pack_keys(eager.cpu().numpy(), batch.target.cpu().numpy())
    assert np.array_equal(_u32(st.keys[:5 * B]), np.tile(keys1, 5))  # positions 0 .. 5B-1
    assert _counts(st) == _counts(st_e)
    a, b = st.compute(), st_e.compute()
    assert a == b


EVAL_SEED = 21


def test_evaluate_six_batches():
    metrics, _ = _mods()
    c, ref, tr = _make("c2_small")
    rng = np.random.RandomState(EVAL_SEED)
    raw = [_rand_batch(rng, c["rows"], B, 1, c["bot"][0], "bce") for B in (128,) * 5 + (37,)]
    orc = np.concatenate([_oracle_forward(ref, X, o, i) for X, o, i, _ in raw])
    lab = np.concatenate([T.ravel() for *_, T in raw])
    near = int(np.sum(np.abs(orc.astype(np.float64) - 0.5) <= 1e-5))
    assert near <= 2, near
    batches = [tr.make_batch(*r) for r in raw]
    st = metrics.EvalState(5 * 128 + 37, dev)
    res = tr.evaluate(batches, st)
    assert st.count == 677
    want = eval_ref.full(orc, lab)
    for k in ("tp", "fp", "tn", "fn"):
        assert abs(res[k] - want[k]) <= near, (k, res[k], want[k])
    n = 677
    assert abs(res["accuracy"] - want["accuracy"]) <= near / n
    for k in ("recall", "precision", "f1"):
        # a ratio of counts that each moved by at most `near` samples
        den = min(want["tp"] + want["fn"], want["tp"] + want["fp"]) - near
        assert abs(res[k] - want[k]) <= (2.0 * near / den if near else 0.0), k
    # the device's own probabilities (eager predict = the replayed graph, bit for bit)
    own = np.concatenate([tr.predict(b).cpu().numpy() for b in batches])
    mine = eval_ref.full(own, lab)
    assert res["auc_num2"] == mine["a2"] and res["roc_auc"] == mine["roc_auc"]
    assert (res["n_pos"], res["n_neg"]) == (mine["n_pos"], mine["n_neg"])
    assert abs(res["ap"] - mine["ap"]) <= 1e-12
    ok, msg = fp32_close(own, orc)
    assert ok, msg
