"""The trainer's step and predict pass against tests/golden/step_trace.json: the launches
(entry point and arguments of every dlrm_hip._lib.call, segment by segment, eager and under
capture), the segment kinds, the graphs per step and the SHA-256 of every tensor the step
leaves, recorded from the trainer as it was before its three segment builders (fp32 step,
bf16 step, predict) became one.  Equality, case by case: the fixture pins the new builder to
the old ones, which the other trainer tests (against the oracle, or the trainer against
itself) cannot.  tests/golden/make_golden_step_trace.py holds the cases and the recorder and
wrote the fixture."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_step_trace", os.path.join(GOLDEN, "make_golden_step_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()
with open(os.path.join(GOLDEN, "step_trace.json")) as _f:
    FIXTURE = json.load(_f)
_GOT = {}  # case name -> its record on this tree


def _record(name):
    """The case's record, as the generator takes it (through JSON, as the fixture went)."""
    # plans and chain parts depend on the device: the one reason to skip
    here = G.device_id()
    if here != FIXTURE["device"]:
        pytest.skip(f"fixture recorded on {FIXTURE['device']}, this is {here}")
    if name not in _GOT:
        _GOT[name] = json.loads(json.dumps(G.run_case(G.CASES[name])))
    return _GOT[name]


def test_fixture_holds_every_case():
    assert sorted(FIXTURE["cases"]) == sorted(G.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(G.CASES))
def test_step_trace(name):
    got, want = _record(name), FIXTURE["cases"][name]
    assert got == want, f"{name}: first difference at {G.first_diff(got, want)}"


@pytest.mark.gpu
def test_bf16_ignores_the_fp32_only_options():
    """The bf16 step with group_wgrad, full_last_wgrad, bot_sched, tbe_role, tbe_role_at,
    head_role, fuse_bottom, dist_bottom_in_lookup and overlaps all off their defaults: the
    launches and bits of the default one."""
    flipped, base = _record(G.NO_EFFECT_CASE), _record(G.NO_EFFECT_BASE)
    assert flipped == base, G.first_diff(flipped, base)
