"""CPU proof of tests/exact_interact.py: the fp64 reference is bitwise the oracle's interaction
and its autograd on every case and bitwise the golden interaction fixtures (in their fp32
arithmetic); every bug model changes bits on every case it is stated to affect; the
full-mantissa cases tell reduced operand precision apart; and the plans of the GPU tests reach
every class of interact.hip's launch ladder by the restated formulas."""
import numpy as np
import pytest
import torch

import exact_interact as X
import oracle as O

GOLDEN = ["F4_D4_s0", "F9_D64_s0", "F27_D128_s0", "F27_D16_s0", "F9_D64_s1", "F27_D128_s1"]
INVALID = ((-1, 1, 0), ("rows", 8, 4), ("rows", 1, 4), (-1, 8, 0))


def _int_cases():
    """The integer cases of the GPU tests at their small batches: the staged plan, the
    runtime-D and elementwise shapes, and gather cases with and without invalid indices."""
    cases = [X.int_case(B, F, D, s) for D, F, s, B, _, _ in X.staged_plan()]
    cases += [X.gather_case(B, F, D, s) for D, F, s, B, _, g in X.staged_plan() if g]
    cases += [X.int_case(3, F, D, D % 2 == 0) for D in (1, 5, 13, 65, 100)
              for F in (X.RUNTIME_SMALL_F, 32)]
    cases += [X.int_case(2, F, D, s) for F in X.ELEMENTWISE_F for D in (1, 8)
              for s in (False, True)]
    cases += [X.gather_case(5, 9, 16, s, invalid=(inv,)) for inv in INVALID
              for s in (False, True)]
    cases.append(X.gather_case(5, 9, 64, False, invalid=INVALID))
    return cases


def _fm_cases():
    return [X.fm_case(kind, 5, F, D, s) for kind in X.FM_OPERANDS for s in (False, True)
            for F, D in ((9, 16), (32, 32), (13, 13), (41, 64))]


def _bits(t):
    return t.contiguous().numpy().view(np.int32)


def _oracle(case, relu_x):
    x = case.x.clone().requires_grad_(True)
    ly = [case.ly[:, t].clone().requires_grad_(True) for t in range(case.F - 1)]
    R = O.interact(x, ly, "dot", case.self_int)
    (R * case.dR).sum().backward()
    gx = torch.where(case.x > 0, x.grad, torch.zeros(())) if relu_x else x.grad
    gly = torch.stack([y.grad for y in ly], 1) if ly else torch.zeros(case.B, 0, case.D)
    return {"R": R.detach(), "gx": gx, "gly": gly}


def test_reference_is_the_oracle_and_its_autograd():
    for case in _int_cases() + _fm_cases():
        assert X.terms_ok(case)
        for relu_x in (True, False):
            ref, orc = X.reference(case, relu_x), _oracle(case, relu_x)
            f64 = X.formula(case.x, case.ly, case.dR, case.self_int, relu_x)
            for k, f in zip(("R", "gx", "gly"), f64):
                if k not in ref:
                    continue
                what = (case.kind, case.B, case.F, case.D, case.self_int, relu_x, k)
                assert torch.equal(ref[k], orc[k]), what
                assert torch.equal(ref[k], f.float()), what
                if case.kind == "int":
                    assert torch.equal(ref[k].double(), f), what


@pytest.mark.parametrize("name", GOLDEN)
def test_formula_is_the_golden_fixture(golden, name):
    g = golden(f"interact_{name}.npz")
    out = X.formula(torch.tensor(g["x"]), torch.tensor(g["ly"]), torch.tensor(g["g"]),
                    bool(g["itself"][0]), False, torch.float32)
    for got, key in zip(out, ("R", "gx", "gly")):
        assert np.array_equal(_bits(got), g[key].view(np.int32)), key


def test_cat_is_the_golden_fixture(golden):
    g = golden("interact_cat.npz")
    R = X.cat_ref(torch.tensor(g["x"]), torch.tensor(g["ly"]))
    assert np.array_equal(_bits(R), g["R"].view(np.int32))
    gx, gly = X.cat_backward_ref(R, 5, 16)
    assert np.array_equal(_bits(gx), g["x"].view(np.int32))
    assert np.array_equal(_bits(gly), g["ly"].view(np.int32))


def test_every_bug_model_changes_bits_where_it_can():
    """Which cases a model affects is BUG_MODELS' statement (a predicate on the case and on
    relu_x), not a discovery: on each of them the model's outputs differ from the reference."""
    seen = {name: 0 for name in X.BUG_MODELS}
    for case in _int_cases():
        for relu_x in (True, False):
            ref = X.reference(case, relu_x)
            for name, (model, affects) in X.BUG_MODELS.items():
                if affects(case, relu_x):
                    seen[name] += 1
                    assert not X._same(model(case, relu_x), ref), (
                        name, case.B, case.F, case.D, case.self_int, relu_x)
    assert all(n >= 8 for n in seen.values()), seen


def test_full_mantissa_cases_see_reduced_precision():
    """fm_case asserts it while it builds; here once more, per model and operand, and that the
    integer cases do NOT see it (why the older exact test could not)."""
    for case in _fm_cases():
        ref = X.reference(case, False)
        alts = X.reduced_precision_results(case)
        assert {k[0] for k in alts} == set(X.REDUCED)
        assert {k[1] for k in alts} == set(X.FM_OPERANDS[case.kind])
        for key, alt in alts.items():
            assert not X._same(alt, ref), (case.kind, key)
    case = X.int_case(5, 9, 16, False)
    for op in X.REDUCED.values():
        assert torch.equal(X.forward_ref(case, A=op), X.forward_ref(case))


def test_pair_of_restatement():
    for s in (False, True):
        li, lj = X.tril(X.K_MAX_F, s)
        assert [X.pair_of(p, s) for p in range(li.size)] == list(zip(li.tolist(), lj.tolist()))
    assert X.npairs(64, True) - 1 == 2079


def test_staged_plan_reaches_every_template():
    plan = X.staged_plan()
    assert X.templates_of(plan) == X.instantiated_templates()
    for D in X.STAGED_D:
        mine = [e for e in plan if e[0] == D]
        assert {1, 32} <= {e[1] for e in mine} and {e[1] for e in mine} == set(X.STAGED_F)
        assert {e[3] % 4 for e in mine} == {1, 3} and {e[3] for e in mine} == set(X.STAGED_B)
        assert {e[2] for e in mine} == {False, True} == {e[4] for e in mine}
        f32 = [e for e in mine if e[1] == 32]
        assert {e[2] for e in f32} == {False, True}
        # every entry runs under every forced version, so F = 32 meets each kernel version
        assert {X.fwd_kernel(f32[0][3], 32, D, v)[0] for v in X.FWD_FORCED} == (
            {"v4", "v5"} if D >= 64 else {"v4"})
        assert {X.bwd_kernel(f32[0][3], 32, D, v)[0] for v in X.BWD_FORCED} == (
            {"v3", "v4", "v5"} if D >= 64 else {"v3", "v4"})
        # no pooled entry of the plan falls off the staged ladder
        assert all(X.fwd_kernel(e[3], e[1], D, 0)[0] in ("v4", "v5") for e in mine)


def test_runtime_plan_reaches_every_wave_class():
    fwd = {X.fwd_waves(32, D) for D in X.RUNTIME_D}
    bwd = {X.bwd_waves(32, D) for D in X.RUNTIME_D}
    assert fwd == {4, 2, 1, 0} == bwd
    assert {X.fwd_waves(X.RUNTIME_SMALL_F, D) for D in X.RUNTIME_D} == {4}
    for D in X.RUNTIME_D:
        assert D not in X.STAGED_D
        for F in (X.RUNTIME_SMALL_F, 32):
            assert X.fwd_kernel(3, F, D)[0] == ("mfma" if X.fwd_waves(F, D) else "generic")
            assert X.bwd_kernel(3, F, D)[0] == ("mfma" if X.bwd_waves(F, D) else "generic")
    # odd D and a second trip of the d += 64 lane loops
    assert any(D % 2 and D > 64 for D in X.RUNTIME_D) and 1 in X.RUNTIME_D
    for F in X.ELEMENTWISE_F + (64,):
        assert X.fwd_kernel(2, F, 8)[0] == X.bwd_kernel(2, F, 8)[0] == "generic"
    # misaligned features or gradient rows leave the staged ladder
    assert X.fwd_kernel(3, 9, 64, aligned=False)[0] == "mfma"
    assert X.bwd_kernel(3, 9, 64, grads_aligned=False)[0] == "mfma"


def test_cap_cases_cross_their_caps():
    want = {"v4 forward": "v4", "v3 backward": "v3", "v4 backward": "v4", "v5 forward": "v5",
            "v5 backward": "v5", "runtime-D forward": "mfma", "runtime-D backward": "mfma"}
    for what, side, forced, B, D in X.CAP_CASES:
        kern = (X.fwd_kernel if side == "fwd" else X.bwd_kernel)(B, 2, D, forced)
        assert kern[0] == want[what] and X.crosses_cap(kern), (what, kern)
        # the smallest such batch with a partly filled last group, give or take a group
        fewer = (X.fwd_kernel if side == "fwd" else X.bwd_kernel)(B - 8, 2, D, forced)
        assert not X.crosses_cap(fewer), (what, fewer)
    assert {c[0] for c in X.CAP_CASES} == set(want)
    assert X.fwd_kernel(1024, 2, 64)[0] == "v5" and X.fwd_kernel(1025, 2, 64)[0] == "v4"
    assert X.bwd_kernel(1024, 2, 64)[0] == "v5" and X.bwd_kernel(1025, 2, 64)[0] == "v3"


def test_layout_shapes_have_and_lack_a_vector_tail():
    for D in X.STAGED_D:
        tail, none = X.LAYOUT_SHAPES["tail"], X.LAYOUT_SHAPES["no tail"]
        assert (D + X.npairs(tail[0], tail[1])) % 4 != 0
        assert (D + X.npairs(none[0], none[1])) % 4 == 0
    assert X.list_strides(5, 16) == [16, 20, 24, 28, 32]
