"""The learning-rate schedule on the host: optim.lr_policy against the reference's own
LRPolicyScheduler (tests/golden/lr_schedule.json, written by tests/golden/make_golden_lr.py),
the configurations it refuses, and TrainerConfig's choice between host and device rates."""
import json
import os

import pytest

from conftest import GOLDEN


def _configs():
    with open(os.path.join(GOLDEN, "lr_schedule.json")) as f:
        return json.load(f)["configs"]


def test_fixture_holds_the_issue_configurations():
    got = {(float.fromhex(c["base"]), c["W"], c["S"], c["D"]): c for c in _configs()}
    small = [(0.1, 4, 6, 5), (24.0, 5, 5, 3), (1.0, 0, 0, 0), (1.0, 3, 3, 0), (0.3, 7, 9, 11),
             (1.0, 0, 0, 4), (1e-6, 2, 2, 50)]
    for key in small:
        c = got[key]
        assert c["step_counts"] == list(range(1, len(c["lr"]) + 1))
        assert len(c["lr"]) >= key[2] + key[3] + 3  # at least three past S + D
    big = got[(24.0, 2750, 49315, 27772)]
    assert big["step_counts"] == [1, 2, 2749, 2750, 2751, 49314, 49315, 49316, 77086, 77087,
                                  77088, 100000]
    # the last small configuration reaches the floor
    assert float.fromhex(got[small[-1]]["lr"][-1]) == 1e-7


def test_lr_policy_equals_the_reference_to_the_last_bit():
    from dlrm_hip.optim import lr_policy
    n = 0
    for c in _configs():
        base = float.fromhex(c["base"])
        for sc, h in zip(c["step_counts"], c["lr"]):
            got = lr_policy(sc, base, c["W"], c["S"], c["D"])
            assert got.hex() == h, (c["W"], c["S"], c["D"], sc, got, float.fromhex(h))
            n += 1
    assert n >= 100


def test_lr_policy_refuses_what_the_reference_cannot_run():
    from dlrm_hip.optim import check_lr_policy, lr_policy
    from dlrm_hip.trainer import TrainerConfig
    with pytest.raises(ValueError):  # the reference sys.exit()s: decay starts inside the warm-up
        lr_policy(1, 0.1, 5, 4, 3)
    # the reference raises AttributeError (last_lr never set): a plateau with W < 2
    for W, S, D in [(0, 2, 4), (1, 2, 4), (1, 7, 1)]:
        with pytest.raises(ValueError):
            lr_policy(1, 0.1, W, S, D)
        with pytest.raises(ValueError):
            check_lr_policy(W, S, D)
        with pytest.raises(ValueError):
            TrainerConfig(m_spa=4, ln_emb=[10], ln_bot=[3, 4], ln_top=[5, 1],
                          lr_num_warmup_steps=W, lr_decay_start_step=S, lr_num_decay_steps=D)
    with pytest.raises(ValueError):
        TrainerConfig(m_spa=4, ln_emb=[10], ln_bot=[3, 4], ln_top=[5, 1], lr_num_warmup_steps=5,
                      lr_decay_start_step=4, lr_num_decay_steps=3)
    # its neighbours run: no plateau (S <= max(W, 1)), or no decay
    for W, S, D in [(0, 1, 4), (1, 1, 4), (0, 0, 4), (1, 9, 0), (0, 9, 0), (2, 9, 3)]:
        check_lr_policy(W, S, D)
        assert lr_policy(1, 0.1, W, S, D) >= 0.0


def test_default_config_keeps_host_learning_rates():
    from dlrm_hip.trainer import TrainerConfig
    kw = dict(m_spa=4, ln_emb=[10], ln_bot=[3, 4], ln_top=[5, 1])
    cfg = TrainerConfig(**kw)
    assert cfg.lr_mode == "host"
    assert (cfg.lr_num_warmup_steps, cfg.lr_decay_start_step, cfg.lr_num_decay_steps,
            cfg.device_lr) == (0, 0, 0, False)
    assert TrainerConfig(device_lr=True, **kw).lr_mode == "device"
    assert TrainerConfig(lr_num_warmup_steps=3, lr_decay_start_step=3, **kw).lr_mode == "device"
    assert TrainerConfig(lr_decay_start_step=2, **kw).lr_mode == "device"
    assert TrainerConfig(lr_num_decay_steps=2, **kw).lr_mode == "device"


def test_bindings_cover_every_dev_entry_point_of_the_header():
    """Every `_dev` function and the lr-state functions the header declares have a ctypes
    signature, and dlrm_gemm_problem's trailing alpha_dev is mirrored."""
    import re
    from dlrm_hip import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "dlrm_hip.h")) as f:
        hdr = f.read()
    names = set(re.findall(r"\b(dlrm_\w+_dev|dlrm_lr_\w+)\s*\(", hdr))
    assert len(names) >= 13, names  # ten consumers, three lr-state functions
    assert names <= set(_lib.SIGNATURES), names - set(_lib.SIGNATURES)
    assert _lib.GemmProblem._fields_[-1][0] == "alpha_dev"
    assert _lib.ABI_VERSION >= 14
