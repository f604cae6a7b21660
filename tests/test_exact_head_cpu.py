"""CPU proof of tests/exact_head.py: the generators' exactness conditions hold at every shape
test_gpu_misc_exact.py uses, the references agree with independent ones (fp64 torch autograd,
Python integers, fractions.Fraction, a known splitmix64 vector), and every bug model changes
the reference on the data of every case it could affect - so no GPU case is blind to it."""
import numpy as np
import pytest
import torch

import exact_head as H
import oracle as O

f32, f64 = np.float32, np.float64
ANCHOR_KINDS = [("mse", "anchor"), ("bce", "anchor")]


# ------------------------------------------------------------------- the head ----
def test_grad_scale_condition():
    """fl(fl(1/M) M) == 1 holds for the batch sizes used and fails for 41, 47, 55, 61."""
    assert all(H.inv_m_exact(M) for M in H.HEAD_MS)
    assert not any(H.inv_m_exact(M) for M in (41, 47, 55, 61))


def test_shapes_cover_every_nc_edge():
    assert {H.head_nc(K) for K in H.HEAD_KS} == {2, 4, 5, 8, 12, 17, 24, 32}
    for edge in (128, 256, 320, 512, 768, 1088, 1536):
        assert edge in H.HEAD_KS and edge + 1 in H.HEAD_KS
        assert H.head_nc(edge) != H.head_nc(edge + 1)
    assert H.head_nc(2048) == 32 and len(H.HEAD_SHAPES) == 40 + 24 - 6


@pytest.mark.parametrize("loss", ["mse", "bce"])
def test_anchor_conditions_hold_everywhere(loss):
    """Every anchor case: the dot products are the chosen logits, X stays in the small-integer
    range but for the logit column, dz is dyadic and the dw bound holds (head_case asserts
    it) - also under the clamp - and the row losses sum exactly where loss_out is asserted."""
    for (M, K) in H.HEAD_SHAPES:
        kinds = ["anchor"] + (["saturated"] if loss == "bce" and K > 1 else [])
        for kind in kinds:
            c = H.head_case(M, K, loss, kind)
            X, w = c.X.numpy().astype(f64), c.w.numpy().astype(f64)
            assert np.array_equal(X @ w, c.z) and (X[:, K - 1] == 1).all()
            free = np.delete(X, K - 2, axis=1) if K > 1 else X
            assert free.min() >= -1 and free.max() <= 3 and np.abs(w).max() <= 2
            assert set(np.unique(c.z)) <= set(H.ANCHOR_P)
            for lo in (0.0, 0.25):
                ok, why = H.head_exact_ok(c, lo)
                assert ok, (M, K, kind, lo, why)
            r = H.head_reference(c)
            if kind == "saturated":
                assert not r["dz"].any() and set(np.unique(r["row_loss"])) <= {0.0, 100.0}
            else:
                m = np.arange(M)
                assert r["dz"][(m % 4 == 3) | (m == M - 1)].all() and not r["dz"][c.z != 0].any()
                assert (r["dz"][c.z == 0] != 0).sum() >= (c.z == 0).sum() * 0.6
                assert set(np.unique(np.abs(r["dz"]))) <= {0.0, 2.0 ** -4, 2.0 ** -5, 2.0 ** -6}
            tset = {0.0, 1.0} if loss == "bce" else set(H.MSE_TARGETS)
            assert set(np.unique(c.t.numpy())) <= tset
            # 0, negatives and positives under the ReLU mask
            if M * K >= 64 and K > 2:
                assert (free == 0).any() and (free < 0).any() and (free > 0).any()


def test_grid_wrap_case_is_valid():
    for loss in ("mse", "bce"):
        c = H.head_case(16388, 2, loss, grad_scale=1.0)
        r = H.head_reference(c)
        assert r["dz"][np.arange(16388) % 4 == 3].all() and 16388 > 4096 * 4


def _autograd(c):
    z = torch.tensor(c.z.astype(f64), requires_grad=True)
    X = c.X.double()
    p = torch.sigmoid(z)
    fn = torch.nn.MSELoss() if c.loss == "mse" else torch.nn.BCELoss()
    E = fn(p, c.t.double())
    E.backward()
    dz = z.grad * c.grad_scale
    return p.detach().numpy(), dz.numpy(), (dz[:, None] * X).sum(0).numpy(), E.item()


@pytest.mark.parametrize("loss", ["mse", "bce"])
@pytest.mark.parametrize("M,K", [(5, 2), (37, 65), (257, 321)])
def test_float32_reference_agrees_with_fp64_autograd(loss, M, K):
    """head_row_ref / head_reference at p = fl(sigmoid(z)) against torch's sigmoid + MSELoss /
    BCELoss in float64: prob, dz, dw and the loss to within float32 rounding."""
    c = H.head_case(M, K, loss, "general")
    r = H.head_reference(c)
    p, dz, dw, E = _autograd(c)
    assert H.ulp_error(r["prob"], p).max() <= 0.5
    # dz: a handful of float32 operations on p; 1 - p loses up to 2^-24 / (1 - p) relative
    rel = 8 * 2.0 ** -24 * (1.0 + 1.0 / (1.0 - p))
    assert (np.abs(r["dz"] - dz) <= rel * np.abs(dz) + 1e-30).all()
    absprod = (np.abs(dz)[:, None] * np.abs(c.X.numpy())).sum(0)
    assert (np.abs(r["dw64"] - dw) <= 64 * 2.0 ** -24 * absprod + 1e-30).all()
    # the loss: logf's argument 1 - pc is a float32 difference, off by up to 2^-24 absolute
    slack = 0.0 if loss == "mse" else np.mean(2.0 ** -23 / (1.0 - p) + 2.0 ** -23 / p)
    tol = 1e-6 * abs(E) + slack
    assert abs(float(r["loss"][0]) - E) <= tol


@pytest.mark.parametrize("loss,kind", ANCHOR_KINDS)
@pytest.mark.parametrize("model", H.HEAD_MODELS)
def test_head_bug_models_change_every_case(model, loss, kind):
    """Each bug model, applied to the reference, changes an asserted output on the data of
    every anchor case it could affect (model_applies says where it cannot: fewer than 4 rows,
    M a multiple of 4, K <= 2 has no free column, K not 1 mod 64)."""
    n = 0
    for (M, K) in H.HEAD_SHAPES:
        if not H.model_applies(model, M, K):
            continue
        c = H.head_case(M, K, loss, kind)
        r, b = H.head_reference(c), H.head_reference(c, model=model)
        keys = {"mask_ge": ["dXm"], "row_dropped": ["dw"], "block_dropped": ["dw"],
                "col_skipped": ["dw"]}.get(model, ["dz", "dw"])
        for k in keys:
            assert not np.array_equal(r[k], b[k]), (model, M, K, k)
        n += 1
    assert n >= 6


def test_model_applies_is_not_too_generous():
    """Where model_applies says a model cannot matter, it really changes nothing."""
    for (M, K) in H.HEAD_SHAPES:
        c = H.head_case(M, K, "mse")
        r = H.head_reference(c)
        for model in ("row_dropped", "m_rounded_up", "col_skipped"):
            if not H.model_applies(model, M, K):
                b = H.head_reference(c, model=model)
                assert all(np.array_equal(r[k], b[k]) for k in ("prob", "dz", "dXm", "dw"))


def test_general_rows_sit_clear_of_the_clamp():
    for (M, K) in [(5, 2), (37, 1089), (257, 65), (257, 2048), (1023, 321)]:
        for loss in ("mse", "bce"):
            c = H.head_case(M, K, loss, "general")
            assert np.abs(c.z).max() <= 16 and (np.abs(c.z) >= 2).any()
            p = H.sigmoid64(c.z)
            inside = np.abs(c.z) <= 1
            assert ((p[inside] > 0.25) & (p[inside] < 0.75)).all()
            assert ((p[~inside] < 0.15) | (p[~inside] > 0.85)).all()


def test_sweep_has_the_anchors_and_exact_inputs():
    z = H.SWEEP_Z
    assert z[0] == -100 and z[-1] == 24 and len(z) == 249 and all(a in z for a in H.ANCHOR_P)
    assert np.array_equal((z - 1.0).astype(f32).astype(f64) + 1.0, z)
    p = H.sigmoid64(z)
    assert (p[z >= -87] >= 2.0 ** -126).all() and (p[z < -87.4] < 2.0 ** -126).all()


# ---------------------------------------------------------------------- colsum ----
def test_colsum_models_change_every_case():
    """The 64-row chunk's last row dropped (M >= 64) and alpha ignored under accumulate
    (alpha != 1) change the reference at every shape, scaled or not."""
    for M in H.COLSUM_MS:
        for N in H.COLSUM_NS:
            g = torch.Generator().manual_seed(M + N)
            out0 = torch.randint(-8, 9, (N,), generator=g).float()
            for scaled in (False, True):
                Y, scale = H.colsum_case(M, N, scaled)
                assert Y.shape == (M, N) and (Y != 0).all() and (Y.abs() <= 4).all()
                ref, _ = H.ref_colsum(Y, scale, 0.5, out0)
                if M >= 64:
                    bad, _ = H.ref_colsum(Y, scale, 0.5, out0, model="chunk_row_dropped")
                    assert not np.array_equal(ref, bad), (M, N)
                if M >= 1:
                    bad, _ = H.ref_colsum(Y, scale, 0.5, out0, model="alpha_ignored")
                    assert not np.array_equal(ref, bad), (M, N)
                _, p = H.ref_colsum(Y, scale, -2.0, None, out0, 2.0 ** -3)
                s = Y.double().numpy() * (1 if scale is None else scale.double().numpy()[:, None])
                assert np.array_equal(p.astype(f64), out0.numpy() - s.sum(0) / 8)


# ------------------------------------------------------------------ optimizers ----
@pytest.mark.parametrize("gs", [1.0, 2.0 ** -3, 1.0 / 3.0])
def test_adagrad_reference_matches_fractions(gs):
    """round_sum_f32's single rounding of each fma equals the Fraction one."""
    for n in (1, 257, 2000):
        p, g, ss = H.adagrad_case(n)
        r2 = g.double() ** 2 + ss.double()
        assert torch.equal(r2.sqrt(), r2.sqrt().round()) and (r2 < 2 ** 24).all()
        a = H.ref_adagrad_dense(p, g, ss, 2.0 ** -3, 2.0 ** -10, gs)
        b = H.ref_adagrad_fraction(p, g, ss, 2.0 ** -3, 2.0 ** -10, gs)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert not torch.equal(a[0], p)
        if gs == 1.0:  # sqrt(s) + eps is exact: s = r^2, r < 4096
            assert torch.equal(a[1].double(), r2)


def test_round_sum_breaks_ties_by_the_lost_part():
    """A float64 sum that lands exactly halfway between two float32 values is rounded by the
    part float64 lost, as the fma's single rounding does; _round_f32 is numpy's rounding."""
    from fractions import Fraction
    tiny = 2.0 ** -80
    a = np.array([1 + 2.0 ** -24, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 + 3 * 2.0 ** -24,
                  -(1 + 2.0 ** -24), 2 - 2.0 ** -24, 1 - 2.0 ** -25])
    b = np.array([tiny, -tiny, tiny, -tiny, -tiny, tiny, -tiny])
    want = [H._round_f32(Fraction(x) + Fraction(y)) for x, y in zip(a, b)]
    assert list(H.round_sum_f32(a, b)) == want
    assert list(H.round_sum_f32(a, 0 * b)) == list(a.astype(f32))
    assert want[0] != want[1] and want[2] != want[3]
    rng = np.random.RandomState(0)
    x = rng.randn(2000) * 10.0 ** rng.randint(-40, 30, 2000)
    assert [H._round_f32(Fraction(v)) for v in x] == list(x.astype(f32))


def test_adagrad_third_is_inexact():
    p, g, ss = H.adagrad_case(257)
    gj = g.numpy() * f32(1.0 / 3.0)
    assert (gj.astype(f64) != g.numpy().astype(f64) * f64(f32(1.0 / 3.0))).any()


def test_sgd_case_is_exact():
    p, g = H.sgd_case(257)
    assert torch.equal(H.ref_sgd(p, g, 0.25).double(), p.double() - 0.25 * g.double())
    assert H.OPT_NS[-1] > 16384 * 256


# ----------------------------------------------------------------- fill streams ----
def test_splitmix64_known_vector():
    """The published SplitMix64 sequence for seed 0 (state advanced by the golden gamma)."""
    gamma = 0x9E3779B97F4A7C15
    state = np.array([(k * gamma) % 2 ** 64 for k in range(4)], dtype=np.uint64)
    assert [int(v) for v in H.splitmix64(state)] == [
        0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC]


def _py_splitmix(z):
    m = 2 ** 64 - 1
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_fill_references_match_python_integers():
    for seed in H.FILL_SEEDS:
        key = _py_splitmix(seed)
        xs = [_py_splitmix(key ^ j) for j in range(1000, 1300)]
        assert [int(v) for v in H.fill_stream(300, seed, first=1000)] == xs
        for lo, hi in ((0.0, 1.0), (-0.5, 0.5)):
            ref = H.ref_uniform_fill(300, lo, hi, seed, first=1000).numpy()
            want = [f32(lo + (hi - lo) * ((x >> 40) / 2.0 ** 24)) for x in xs]  # exact in fp64
            assert ref.dtype == f32 and list(ref) == want
            assert ref.min() >= lo and ref.max() < hi
        for hi in (1, 1000, 2 ** 31, 2 ** 40):
            a = H.ref_uniform_int(300, hi, seed)
            b = H.ref_uniform_int(300, hi, seed, exact_python=True)
            assert torch.equal(a, b) and int(a.max()) < hi
    x = np.array([0, 1, 2 ** 64 - 1, 2 ** 63, 0xFFFFFFFF, 2 ** 32], dtype=np.uint64)
    for hi in (1, 2 ** 31, 2 ** 40, 2 ** 63 - 1):
        assert [int(v) for v in H.mulhi64(x, hi)] == [(int(v) * hi) >> 64 for v in x]


def test_fill_chunks_are_the_stream():
    whole = H.ref_uniform_fill(5000, -0.5, 0.5, 7)
    parts = [H.ref_uniform_fill(b - a, -0.5, 0.5, 7, first=a)
             for a, b in ((0, 100), (100, 3333), (3333, 5000))]
    assert torch.equal(torch.cat(parts), whole)
    assert not torch.equal(H.ref_uniform_fill(100, -0.5, 0.5, 7, first=100), whole[:100])


# --------------------------------------------------------------------- QR / CSR ----
@pytest.mark.parametrize("c", [4, 1000, 60000])
def test_qr_split_values_part_from_integer_division(c):
    vals = H.qr_split_values(c)
    assert {2 ** 24 - 1, 2 ** 24 + 1, 2 ** 31 - 1} <= set(vals)
    q, r = O.QREmbeddingBagOracle.split(torch.tensor(vals), c)
    assert r.tolist() == [v % c for v in vals]
    diff = [v for v, qq in zip(vals, q.tolist()) if qq != v // c]
    assert any(2 ** 24 < v < 2 ** 27 for v in diff) and any(v > 2 ** 27 for v in diff)


def test_ref_csr():
    offs = [torch.tensor([0, 0, 2]), torch.tensor([0, 1, 1])]
    assert H.ref_csr(offs, [3, 1]).tolist() == [0, 0, 2, 3, 4, 4, 4]
