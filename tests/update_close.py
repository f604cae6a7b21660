"""An update-relative check for the trainer's tolerance tests (plain helper module, no GPU
import).

conftest.fp32_close compares STATES: |a - b| <= 1e-5 max(1, |ref|).  After one step at the
cases' shapes that is about the size of the whole update (test_exact_step_cpu.py records what
it admits).  This module compares UPDATES instead.  Given a tensor before the step, the
engine's after it, the fp32 oracle's and an fp64 twin's (train16_ref.clone64):

    d = max |(engine - before) - (twin - before)|
    e = max(max |(oracle - before) - (twin - before)|, ulp(max |before|))

e is what one fp32 realisation of the step - the oracle - is away from the fp64 step, and at
least one rounding of the stored weight.  The engine is another fp32 realisation with another
summation order, so d <= MARGIN e with a margin of a few.  The check is only accepted where
it is sharp: MARGIN e <= SHARP max |twin - before|, so an error of 10 % of the largest update
cannot hide.  Valid for the FIRST step only, where all three start from identical weights.

MARGIN is twice the largest d / e measured on an MI355X over every tensor of
test_gpu_trainer.test_step_vs_oracle's three cases: 0.512 (c2_small table15; c3_small 0.502,
c1_small 0.500; profiles/update_close_ratios.txt).  The ratios sit at one half because on most
tensors e is its floor, one ulp of the largest weight, and the engine's stored update is within
half an ulp of the twin's."""
import numpy as np

MARGIN = 1.03  # 2 x 0.512, rounded up
SHARP = 0.05
# case -> tensors that cannot meet the sharpness condition (at most two per case).  None: on
# the CPU the worst e / max |update| is 6.7e-3 (c3_small table5), 1.4e-3 (c2_small table19)
# and 2.1e-4 (c1_small W0), so MARGIN e stays below 0.7 % of every tensor's largest update
EXCLUDED = {"c2_small": (), "c3_small": (), "c1_small": ()}


def figures(before, engine, oracle32, twin64):
    """(d, e, top): the engine's and the oracle's worst update error against the twin, and
    the largest update of the twin."""
    b = np.asarray(before, dtype=np.float64)
    d64 = np.asarray(twin64, dtype=np.float64) - b
    d = np.abs((np.asarray(engine, dtype=np.float64) - b) - d64).max()
    e32 = np.abs((np.asarray(oracle32, dtype=np.float64) - b) - d64).max()
    ulp = float(np.spacing(np.float32(np.abs(b).max())))
    return float(d), float(max(e32, ulp)), float(np.abs(d64).max())


def sharp(e, top, margin=MARGIN):
    return margin * e <= SHARP * top


def check(case, name, before, engine, oracle32, twin64, touched=None):
    """Asserts the update check for one tensor and returns (d, e, top).  ``touched`` (tables):
    a boolean mask of the rows some index names; every other row must keep its bits."""
    d, e, top = figures(before, engine, oracle32, twin64)
    print(f"update_close {case} {name}: d {d:.3e} e {e:.3e} d/e {d / e:.2f} "
          f"max|update| {top:.3e} margin*e/max|update| {MARGIN * e / top:.2e}")
    if touched is not None:
        keep = ~np.asarray(touched, dtype=bool)
        a = np.ascontiguousarray(np.asarray(engine, dtype=np.float32)[keep]).view(np.int32)
        b = np.ascontiguousarray(np.asarray(before, dtype=np.float32)[keep]).view(np.int32)
        assert np.array_equal(a, b), f"{case} {name}: a row no index names changed"
    if name in EXCLUDED.get(case, ()):
        return d, e, top
    assert top > 0, f"{case} {name}: no update at all"
    assert sharp(e, top), f"{case} {name}: the check is not sharp (e {e:.3e}, update {top:.3e})"
    assert d <= MARGIN * e, f"{case} {name}: update error {d:.3e} > {MARGIN} x {e:.3e}"
    return d, e, top
