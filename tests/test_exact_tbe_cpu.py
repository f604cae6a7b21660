"""CPU proofs of tests/exact_tbe.py: the generator does what it promises, the references agree
with independent CPU implementations on the same inputs, and the comparisons fail for the
right reasons (models of kernel bugs on the lookup list each change a result)."""
import numpy as np
import pytest
import torch

import exact_tbe as E
import oracle as O
from conftest import fp32_close


def _named_cases():
    cases = [E.skewed_case(), E.structure_case(), E.cancel_case()] + E.small_n_cases()
    cases += [E.sort_case(k) for k in ("rank", "radix", "tiled")]
    cases += [E.sort_case(f"rows{n}") for n in E.GLOBAL_ROW_CLASSES]
    return cases


CASES = {c.name: c for c in _named_cases()}


# ------------------------------------------------------------------ generator ----
@pytest.mark.parametrize("name", sorted(CASES))
def test_run_table_is_the_stable_argsort_of_the_keys(name):
    c = CASES[name]
    order = np.argsort(c.keys, kind="stable")
    sk = c.keys[order]
    assert np.array_equal(sk, c.sorted_keys("global"))
    assert np.array_equal(E.runs_of(sk, c.total_rows), c.runs_spec)
    assert np.array_equal(c.runs, c.runs_spec)
    # positions ascend inside every run (the sort is stable), and a run is one row's lookups
    for s, n, r in c.runs_spec:
        assert (np.diff(order[s:s + n]) > 0).all() and (c.row[order[s:s + n]] == r).all()
    # with every index valid and no lookup outside the bags, the per-table layout is the same
    if c.flag == 0 and c.offsets[0] == 0 and c.offsets[-1] == c.N:
        assert np.array_equal(c.sorted_keys("per_table"), sk)


def test_bag_shapes_tables_and_outside_lookups():
    c = E.sort_case("rank")
    assert (c.bag_len == 0).any() and c.bag_len.max() > 1
    for t in (0, 2):  # first and last bag of a table empty, the table not
        assert c.bag_len[t * c.B] == 0 and c.bag_len[(t + 1) * c.B - 1] == 0
    assert c.table_lookups[1] == 0 and min(c.table_lookups[0], c.table_lookups[2]) > 0
    assert c.offsets[0] == 3 and c.N - c.offsets[-1] == 5
    assert (c.bag[:3] == -1).all() and (c.bag[-5:] == -1).all() and not c.valid[-5:].any()
    bad = (c.bag >= 0) & ~c.valid
    assert bad.sum() == 2 and (c.indices[bad] < 0).any() and (c.indices[bad] > 0).any()
    assert c.flag == E.ERR_INDEX
    for first, mid, last in ((0, 1, 2), (1, 0, 2), (1, 2, 0)):  # the empty table anywhere
        tabs = [None] * 3
        tabs[first], tabs[mid], tabs[last] = (4, []), (9, [3, 2]), (5, [1, 6])
        e = E.run_csr("e", tabs, B=4, seed=first)
        assert e.table_lookups[first] == 0 and e.N == 12 and np.array_equal(e.runs, e.runs_spec)
    assert CASES["sort_radix"].table_lookups[0] > E.RANK_SORT_MAX
    assert E.RANK_SORT_MAX < CASES["sort_radix"].max_table <= E.SEG_CAP
    assert CASES["sort_rank"].max_table <= E.RANK_SORT_MAX
    assert E.SEG_CAP < CASES["sort_tiled"].max_table <= 2 * E.SEG_CAP
    for n, cls in E.GLOBAL_ROW_CLASSES.items():
        assert E.digit_class(CASES[f"sort_rows{n}"].total_rows) == cls


@pytest.mark.parametrize("idx_dtype,off_dtype", E.IDX_PAIRS)
def test_index_and_offset_dtypes_are_independent(idx_dtype, off_dtype):
    c = E.sort_case("rank", idx_dtype, off_dtype)
    idx, off, rb = c.device_csr("cpu")
    assert idx.dtype == idx_dtype and off.dtype == off_dtype and rb.dtype == torch.int64
    assert np.array_equal(idx.numpy(), c.indices) and np.array_equal(off.numpy(), c.offsets)
    d = CASES["sort_rank"].with_dtypes(idx_dtype, off_dtype)
    assert d.idx_dtype == idx_dtype and np.array_equal(d.indices, c.indices)


@pytest.mark.parametrize("ch", [E.CH, E.LONG_CH])
@pytest.mark.parametrize("variant", ["global", "per_table"])
def test_structure_case_holds_every_alignment_class(ch, variant):
    c = CASES["structure"]
    for D in (16, 128):
        lpb = E.dispatch(D)[1]
        got = E.alignment_classes(c.sorted_keys(variant), c.total_rows, ch, lpb)
        assert got == set(E.ALIGN_CLASSES), set(E.ALIGN_CLASSES) - got
    assert c.N % E.CH != 0 and c.rows[0] == 1 and c.table_lookups[0] == c.runs[0, 1] == 64
    n1, n7, n128 = E.small_n_cases()
    assert n1.N == 1 and n7.N < 16 and n128.N % E.LONG_CH == 0 and n128.N % E.CH == 0
    # the classifier itself, on hand-made arrays (sentinel 99, blocks of 4)
    k = np.array([0, 0, 0, 0, 1, 2, 2, 2, 3, 3, 3, 3, 3, 3, 4, 5, 99, 99])
    assert E.alignment_classes(k, 99, 4, 1) == {
        "one_block_at_edge", "single_first_of_block", "mid_to_edge", "edge_to_mid",
        "single_last_of_block", "run_then_sentinel"}
    k = np.array([7] + [8] * 6 + [9] * 10 + [10] * 2)
    assert E.alignment_classes(k, 99, 4, 1) == {
        "single_first_of_block", "mid_to_mid_3_blocks", "end_and_start_in_one_block"}
    assert "long_run" in E.alignment_classes(np.zeros(4 * 19 + 1), 99, 4, 1)
    assert "long_run" not in E.alignment_classes(np.zeros(4 * 18), 99, 4, 1)
    assert "k_blocks_edge_to_edge" in E.alignment_classes(np.zeros(8), 99, 4, 1)


def test_dispatch_classes_of_the_d_lists():
    D_FWD = [1, 2, 4, 5, 8, 12, 16, 32, 64, 100, 128, 256, 260, 512, 1024, 2048]
    vec = {E.dispatch(D) for D in D_FWD if D % 4 == 0}
    sca = {E.dispatch(D, aligned=False) for D in D_FWD if D <= 512}
    for side, vw in ((vec, 4), (sca, 1)):
        assert {l for v, l, m in side if v == vw} == {1, 2, 4, 8, 16, 32, 64}
        assert {m for v, l, m in side if v == vw} == {1, 2, 4, 8}
    assert E.dispatch(2052)[2] > 8 and E.dispatch(100) == (4, 32, 1)  # 25 chunks: not 2^k


# ----------------------------------------------------------------- conditions ----
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("weighted", [False, True])
def test_exactness_conditions_hold_on_every_case(name, weighted):
    c = CASES[name]
    # the D list of the dispatch tests on the skewed case, D = 16 / 128 elsewhere
    for D in ((1, 5, 16, 100, 2048) if name == "skewed" else (16, 128)):
        o = E.operands_for(c, D, weighted, seed=3)
        assert E.exact_conditions_ok(c, o) == (True, "")
        assert o.gmax in (8, 4, 2, 1) and float(o.G.abs().max()) <= 8 and bool((o.G != 0).all())
        if weighted:
            assert float(o.psw.abs().max()) <= 3 and bool((o.psw != 0).all())


def test_exactness_conditions_reject_a_bad_case():
    c = CASES["skewed"]
    o = E.make_operands(c, 16, True, seed=3)
    assert E.exact_conditions_ok(c, o)[0]
    bad = E.make_operands(c, 16, True, seed=3)
    bad.G[5, 1] = bad.G[4, 1]
    assert "neighbouring bags" in E.exact_conditions_ok(c, bad)[1]
    bad = E.make_operands(c, 16, True, seed=3)
    bad.G *= 2.0 ** 17
    assert "run sum" in E.exact_conditions_ok(c, bad)[1]
    bad = E.make_operands(c, 16, True, seed=3, lr=2.0 ** -22)
    assert "update bound" in E.exact_conditions_ok(c, bad)[1]
    bad = E.make_operands(c, 16, True, seed=3)
    bad.G *= 64
    assert "Adagrad" in E.exact_conditions_ok(c, bad)[1]
    assert E.exact_conditions_ok(c, bad, adagrad=False)[0]
    assert "zero" in E.exact_conditions_ok(c, o, zero_rows=(0,))[1]
    z = CASES["cancel"]
    row = int(z.runs_spec[z.runs_spec[:, 1] == 2][0, 2])
    oz = E.operands_for(z, 16, True, seed=3, zero_row=row)
    assert not E.exact_conditions_ok(z, oz)[0]
    gs = E.coalesced_grad(z, oz)
    assert bool((gs[np.searchsorted(oz.urows, row)] == 0).all())


# ----------------------------------------------------------------- references ----
def _full(c, o, Wu, fill=float("nan")):
    W = torch.full((c.total_rows, Wu.shape[1]), fill, dtype=Wu.dtype)
    W[torch.from_numpy(o.urows)] = Wu
    return W


def _table_csr(c, t):
    a, e = c.offsets[t * c.B], c.offsets[(t + 1) * c.B]
    p = np.arange(a, e)[c.valid[a:e]]  # EmbeddingBag raises on a bad index: take them out
    lens = np.bincount(c.bag[p] - t * c.B, minlength=c.B)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return p, torch.from_numpy(c.indices[p]), torch.from_numpy(off)


@pytest.mark.parametrize("name", ["skewed", "sort_rank", "cancel"])
@pytest.mark.parametrize("weighted", [False, True])
def test_references_agree_with_torch(name, weighted):
    c = CASES[name]
    D = 12
    o = E.operands_for(c, D, weighted, seed=5)
    W = _full(c, o, o.W0u, fill=0.0)
    params = [torch.nn.Parameter(W[c.row_base[t]:c.row_base[t + 1]].clone()) for t in range(c.T)]
    out = torch.zeros(c.B, c.T, D)
    psw_grad = torch.zeros(c.N)
    for t in range(c.T):
        p, idx, off = _table_csr(c, t)
        w = None if o.psw is None else o.psw[torch.from_numpy(p)].clone().requires_grad_(True)
        y = torch.nn.functional.embedding_bag(idx, params[t], off, mode="sum",
                                              per_sample_weights=w)
        out[:, t] = y.detach()
        (y * o.G[:, t]).sum().backward()
        if w is not None:
            psw_grad[torch.from_numpy(p)] = w.grad
    assert torch.equal(E.ref_forward(c, o, o.W0u), out)
    dense = torch.cat([p.grad for p in params])  # autograd's dense gradient
    gsum = E.coalesced_grad(c, o)
    got = _full(c, o, E.ref_dense(torch.zeros_like(o.W0u), gsum), fill=0.0)
    assert torch.equal(got, dense)
    if weighted:
        assert torch.equal(E.ref_psw_grad(c, o, o.W0u), psw_grad)
    eg = E.ref_expand_grad(c, o)
    ins = torch.from_numpy(c.bag >= 0)
    assert not eg[~ins].any() and bool((eg[ins] != 0).all())
    vp = torch.from_numpy(np.flatnonzero(c.valid))
    assert torch.equal(E.coalesce(o.urows, c.row[c.valid], eg[vp].double().numpy()), gsum)
    # sgd / fp16 sgd against torch's own arithmetic
    sgd = E.ref_sgd(o.W0u, gsum, o.lr)
    assert torch.equal(sgd, o.W0u - o.lr * gsum.float())
    lr16 = 2.0 ** -9
    h = E.ref_sgd_f16(o.W0u.half(), gsum, lr16)
    assert h.dtype == torch.float16 and torch.equal(h, (o.W0u - lr16 * gsum.float()).half())
    assert not torch.equal(h.float(), o.W0u - lr16 * gsum.float())  # fp16 does round here


@pytest.mark.parametrize("weighted", [False, True])
def test_adagrad_reference_agrees_with_the_oracle(weighted):
    c = CASES["skewed"]
    D = 16
    o = E.operands_for(c, D, weighted, seed=6)
    W = _full(c, o, o.W0u, fill=0.0)
    params = [torch.nn.Parameter(W[c.row_base[t]:c.row_base[t + 1]].clone()) for t in range(c.T)]
    opt = O.RWSAdagradOracle(params, lr=o.lr, eps=o.eps)
    for t in range(c.T):
        p, idx, off = _table_csr(c, t)
        w = None if o.psw is None else o.psw[torch.from_numpy(p)]
        y = torch.nn.functional.embedding_bag(idx, params[t], off, mode="sum", sparse=True,
                                              per_sample_weights=w)
        (y * o.G[:, t]).sum().backward()
    opt.step()
    mom0 = torch.zeros_like(o.mom0u)  # the oracle's initial accumulator
    Wr, mr = E.ref_adagrad(o.W0u, mom0, E.coalesced_grad(c, o), D, o.lr, o.eps)
    want = torch.cat([p.data for p in params])[torch.from_numpy(o.urows)]
    ok, msg = fp32_close(Wr.numpy(), want.numpy())
    assert ok, msg
    mom = torch.cat([opt.state[id(p)]["momentum"] for p in params])[torch.from_numpy(o.urows)]
    ok, msg = fp32_close(mr.numpy(), mom.numpy())
    assert ok, msg
    # one operation per rounding: redo the chain on one row in numpy scalars
    g = E.coalesced_grad(c, o).numpy()[0]
    f = np.float32
    m = f(o.mom0u[0]) + f(float((g * g).sum())) / f(D)
    den = f(np.sqrt(m)) + f(o.eps)
    w1 = (o.W0u[0].numpy().astype(np.float64) - o.lr * (g.astype(f) / den).astype(np.float64))
    Wr, mr = E.ref_adagrad(o.W0u, o.mom0u, E.coalesced_grad(c, o), D, o.lr, o.eps)
    assert mr[0] == m and np.array_equal(Wr[0].numpy(), w1.astype(f))


# ----------------------------------------------------- the comparisons can fail ----
@pytest.mark.parametrize("model", sorted(E.BUG_MODELS))
@pytest.mark.parametrize("ch", [E.CH, E.LONG_CH])
def test_bug_models_change_the_result(model, ch):
    c = CASES["structure"]
    o = E.operands_for(c, 16, True, seed=7)
    gsum = E.coalesced_grad(c, o)
    lk = E.Lookups(c, o)
    assert torch.equal(lk.gsum(), gsum)  # the unedited list is the reference
    bad = E.BUG_MODELS[model](lk, ch).gsum()
    assert not torch.equal(bad, gsum)
    assert not torch.equal(E.ref_sgd(o.W0u, bad, o.lr), E.ref_sgd(o.W0u, gsum, o.lr))
    assert not torch.equal(E.ref_dense(o.acc0u, bad), E.ref_dense(o.acc0u, gsum))
    a, b = E.ref_adagrad(o.W0u, o.mom0u, bad, 16, o.lr, o.eps), \
        E.ref_adagrad(o.W0u, o.mom0u, gsum, 16, o.lr, o.eps)
    assert not torch.equal(a[0], b[0])


def test_adagrad_mean_over_a_padded_d_changes_the_result():
    c = CASES["skewed"]
    o = E.operands_for(c, 100, False, seed=8)
    gsum = E.coalesced_grad(c, o)
    W, m = E.ref_adagrad(o.W0u, o.mom0u, gsum, 100, o.lr, o.eps)
    Wp, mp = E.ref_adagrad(o.W0u, o.mom0u, gsum, 128, o.lr, o.eps)  # 32 lanes x float4
    assert not torch.equal(m, mp) and not torch.equal(W, Wp)


def test_an_update_reaching_an_untouched_row_is_seen():
    c = CASES["skewed"]
    o = E.operands_for(c, 16, False, seed=9)
    before = _full(c, o, o.W0u)
    after = _full(c, o, E.ref_sgd(o.W0u, E.coalesced_grad(c, o), o.lr))
    assert E.untouched_intact(before, after, o.urows)
    free = np.setdiff1d(np.arange(c.total_rows), o.urows)
    assert free.size > 0
    for v in (0.0, 1.0, float("-nan")):  # any write, a NaN with another sign bit too
        worse = after.clone()
        worse[int(free[0]), 3] = v
        assert not E.untouched_intact(before, worse, o.urows)
    mom = torch.full((c.total_rows,), float("nan"))
    assert E.bits_equal(mom, mom.clone()) and not E.bits_equal(mom, -mom)
    assert E.bits_equal(torch.zeros(2).half(), torch.zeros(2).half())
