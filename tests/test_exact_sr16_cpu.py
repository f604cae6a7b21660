"""tests/exact_sr16.py (the host restatement of the fp16 tables' stochastic rounding, ABI v16)
proved on the CPU: the specification's known answers, exact counts over all 65536 draws, the
normal-range bit trick, the special values, and two conditions on the hashed stream."""
import math
import os
import re

import numpy as np
import pytest

import exact_sr16 as X
from conftest import ROOT

ALL_DRAWS = np.arange(65536, dtype=np.uint32)


def test_known_answers():
    want = {
        0: [46911, 56321, 5886, 63977, 50935, 63841, 62353, 57118],
        1: [45927, 55886, 42083, 61247, 57261, 6337, 46552, 8618],
        2 ** 32 - 3: [4792, 48832, 43811, 3401, 53859, 28993, 19557, 42452],
    }
    got = X.r16(123, 5, list(want), 8)
    for i, row in enumerate(want):
        assert got[i].tolist() == want[row], row
    # a draw depends on (seed, step, row, column) only: not on which rows it is asked with
    assert np.array_equal(X.r16(123, 5, [1], 8)[0], got[1])
    # ... and D enters through C = ceil(D / 4) alone: row 0 does not see it
    assert np.array_equal(X.r16(123, 5, [0], 6)[0], got[0][:6])


def test_splitmix64_is_the_librarys():
    """The same constants as the shared header the kernels include."""
    src = open(os.path.join(ROOT, "dlrm-yx_amd", "csrc", "splitmix.hpp")).read()
    for c in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB"):
        assert c in src
    misc = open(os.path.join(ROOT, "dlrm-yx_amd", "csrc", "misc.hip")).read()
    assert "uint64_t splitmix64(" not in misc and '#include "splitmix.hpp"' in misc
    assert int(X.splitmix64(0)) == 0xE220A8397B1DCDAF  # the published first output of seed 0


def test_every_finite_half_is_unchanged():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    h = bits.view(np.float16)
    fin = np.isfinite(h)
    v = h[fin].astype(np.float32)
    for r in (0, 1, 7, 8, 32767, 32768, 65528, 65535):
        got = X.sr16(v, r)
        assert np.array_equal(got.view(np.uint16), bits[fin]), r


@pytest.mark.parametrize("v,lo,hi,up", [
    (1.0 - 2.0 ** -13, 1.0 - 2.0 ** -11, 1.0, 49152),      # frac 3/4 (the worked value)
    (3 * 2.0 ** -26, 0.0, 2.0 ** -24, 49152),                # subnormal range, frac 3/4
    (65530.0, 65504.0, math.inf, 53248),                     # ulp 32: frac 26/32; 65536 = Inf
])
def test_exact_counts_over_all_draws(v, lo, hi, up):
    for s in (1.0, -1.0):
        x = np.full(65536, s * v, dtype=np.float32)
        assert float(x[0]) == s * v  # representable in fp32
        got = X.sr16(x, ALL_DRAWS).astype(np.float64)
        assert int((got == s * hi).sum()) == up
        assert int((got == s * lo).sum()) == 65536 - up
        assert np.array_equal(np.signbit(got), np.full(65536, s < 0))  # -0 included
        # the draws that round up are exactly the r16 < frac * 65536
        assert np.array_equal(got == s * hi, ALL_DRAWS < up)


def test_bit_trick_equals_the_definition_in_the_normal_range():
    rng = np.random.RandomState(5)
    e = rng.randint(-14, 16, 200000)
    v = (np.ldexp(1.0 + rng.rand(200000), e) * rng.choice([-1.0, 1.0], 200000)).astype(np.float32)
    v = v[(np.abs(v) >= 2.0 ** -14) & (np.abs(v) < 65536.0)]
    assert v.size > 190000
    r = rng.randint(0, 65536, v.size).astype(np.uint32)
    a, b = X.sr16(v, r), X.sr16_bit_trick(v, r)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
    # edges of the range, every low-mantissa pattern near a binade end
    edge = np.array([2.0 ** -14, 65535.99, 65504.0, 65519.0, 65520.0, 2.0 ** -14 * (1 + 2.0 ** -23)],
                    dtype=np.float32)
    for r in (0, 7, 8, 65535):
        assert np.array_equal(X.sr16(edge, r).view(np.uint16),
                              X.sr16_bit_trick(edge, r).view(np.uint16))


def test_special_values():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    for r in (0, 12345, 65535):
        got = X.sr16(np.array([inf, -inf, 0.0, -0.0, 65536.0, -65536.0, 1e9, -3e38],
                              dtype=np.float32), r)
        assert got.view(np.uint16).tolist() == [0x7C00, 0xFC00, 0x0000, 0x8000, 0x7C00, 0xFC00,
                                                0x7C00, 0xFC00]
        n = X.sr16(np.array([nan, -nan], dtype=np.float32), r)
        assert np.isnan(n).all()
        assert np.array_equal(n.view(np.uint16), np.array([nan, -nan], dtype=np.float32).astype(
            np.float16).view(np.uint16))
    # a tiny negative rounds to -0 or to the smallest subnormal
    t = X.sr16(np.full(65536, -2.0 ** -40, dtype=np.float32), ALL_DRAWS)
    assert set(t.view(np.uint16).tolist()) == {0x8000, 0x8001}
    assert int((t.view(np.uint16) == 0x8001).sum()) == 1  # frac * 65536 = 2^-16 * 65536 = 1


SEEDS, STEPS = (0, 1, 2, 3), (0, 1, 2)


def test_hashed_stream_is_unbiased():
    """Rows 0..4095, D = 16, frac = 3/4: the number rounded up over n = 65536 draws lies within
    4 sigma of n * 3/4 (sigma = sqrt(n * 3/16)); these fixed seeds and steps lie within 1.2."""
    n = 4096 * 16
    sigma = math.sqrt(n * 3 / 16)
    v = np.full((4096, 16), 1.0 - 2.0 ** -13, dtype=np.float32)
    worst = 0.0
    for seed in SEEDS:
        for step in STEPS:
            got = X.sr16(v, X.r16(seed, step, np.arange(4096), 16))
            assert set(np.unique(got.astype(np.float64))) <= {1.0, 1.0 - 2.0 ** -11}
            up = int((got.astype(np.float64) == 1.0).sum())
            z = abs(up - n * 0.75) / sigma
            assert z <= 4.0, (seed, step, up)
            worst = max(worst, z)
    assert worst <= 1.2, worst


def test_steps_of_one_seed_are_independent():
    """Two steps of one seed agree on about half of their r16 < 32768 decisions: the count of
    agreements is Binomial(n, 1/2), held to 4 sigma."""
    n = 4096 * 16
    sigma = math.sqrt(n / 4)
    for seed in SEEDS:
        d = [X.r16(seed, step, np.arange(4096), 16) < 32768 for step in STEPS]
        for i in range(len(d)):
            for j in range(i + 1, len(d)):
                agree = int((d[i] == d[j]).sum())
                assert abs(agree - n / 2) <= 4 * sigma, (seed, i, j, agree)
    a, b = X.r16(0, 0, np.arange(4096), 16), X.r16(1, 0, np.arange(4096), 16)
    assert abs(int(((a < 32768) == (b < 32768)).sum()) - n / 2) <= 4 * sigma


def test_abi_v16_bindings():
    from dlrm_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()
    assert int(re.search(r"#define\s+DLRM_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 16
    assert int(re.search(r"#define\s+DLRM_SR_STATE_BYTES\s+(\d+)", hdr).group(1)) == 16
    assert _lib.ABI_VERSION >= 16 and _lib.load().dlrm_abi_version() == _lib.ABI_VERSION
    f16 = _lib.SIGNATURES["dlrm_tbe_backward_sgd_f16"][1]
    sr = _lib.SIGNATURES["dlrm_tbe_backward_sgd_f16_sr"][1]
    i = f16.index(_lib.c_float)
    assert sr == f16[:i + 1] + [_lib.P, _lib.P] + f16[i + 1:]  # lr, then lr_dev and sr_state
    # a null state is refused on the host, before any launch
    with pytest.raises(_lib.DLRMHipError) as e:
        _lib.call("dlrm_tbe_backward_sgd_f16_sr", 256, 4, 256, 1, 1, 256, 32, 256, 32, 1, 1, None,
                  256, 4, 0.1, None, None, 0, 256, 1 << 20, None, 0, None)
    assert e.value.code == 1 and "sr_state" in str(e.value)
    with pytest.raises(_lib.DLRMHipError) as e:
        _lib.call("dlrm_sr_tick", None, None)
    assert e.value.code == 1


def test_config_refusals():
    from dlrm_hip.trainer import TrainerConfig
    kw = dict(m_spa=16, ln_emb=[10, 10], ln_bot=[13, 16], ln_top=[19, 1])
    assert TrainerConfig(**kw).emb_rounding == "nearest"
    TrainerConfig(emb_precision="fp16", emb_rounding="stochastic", emb_rounding_seed=7, **kw)
    with pytest.raises(ValueError):
        TrainerConfig(emb_precision="fp32", emb_rounding="stochastic", **kw)
    with pytest.raises(ValueError):
        TrainerConfig(emb_precision="fp16", emb_rounding="random", **kw)
