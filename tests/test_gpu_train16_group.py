"""DLRMTrainer.group_bwd16: the bf16 step's MLP backward as grouped launches
(dlrm_linear16_bwd_group) must leave bitwise what the per-layer launches leave - every dense
parameter, the tables, the optimizer state and prob - after an eager step and a captured and
replayed one, on the fused-SGD path and the gradient-bucket path (rwsadagrad).  The bottom MLPs
of the two models have 4 and 3 layers: the deferred wgrad needs the third gradient buffer."""
import contextlib

import pytest
import torch

from test_gpu_train16 import ADAGRAD_LR, _batches, _bits_equal, _make, _state

pytestmark = pytest.mark.gpu


def _run(name, optimizer, grouped):
    lr = ADAGRAD_LR if optimizer == "rwsadagrad" else None
    c, ref, tr = _make(name, optimizer=optimizer, mlp_precision="bf16", lr=lr)
    tr.group_bwd16 = grouped
    b0, b1 = (tr.make_batch(*b) for b in _batches(name, 2, seed=9))
    names = []

    def profile(what):
        names.append(what)
        return contextlib.nullcontext()

    prob, _ = tr.step(b0, profile=profile)
    out = [prob.clone()]
    torch.cuda.synchronize()
    tr.capture(b1)()
    torch.cuda.synchronize()
    tr.check_errors()
    assert tr.bwd16_grouped == grouped and tr.step_count == 2
    out += [tr._cur["prob"].clone()] + _state(tr)
    for W, b in tr.dense_state():
        out += [W.clone(), b.clone()]
    return out, names.count("gemm"), len(tr.top) - 1, tr.n_bot


@pytest.mark.parametrize("name,optimizer", [("c2_small", "sgd"), ("c3_small", "sgd"),
                                            ("c2_small", "rwsadagrad")])
def test_grouped_backward_is_bitwise_the_per_layer_one(name, optimizer):
    off, gemm_off, n_top, n_bot = _run(name, optimizer, False)
    on, gemm_on, _, _ = _run(name, optimizer, True)
    assert len(on) == len(off)
    for a, b in zip(on, off):
        assert _bits_equal(a, b)
    # per layer: a dgrad (not for the bottom's first layer) and a wgrad; grouped: one launch
    # per dgrad with the wgrad of the layer above riding in it, the top's last wgrad alone and
    # the bottom's two lowest wgrads together
    forward = gemm_off - (2 * n_top + 2 * n_bot - 1)
    assert forward >= 0 and gemm_on == forward + (n_top + 1) + n_bot
