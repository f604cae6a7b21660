"""DLRMTrainer.store16: the bf16 training step with 16-bit activations and data gradients in
memory against the same step on fp32 buffers - two trainers from one oracle model on the same
batches.  Every consumer of such a buffer used it only as r16(value) or through the sign of a
ReLU mask, so every dense parameter, every table, the optimizer state and the loss are
torch.equal after each step.  The bottom MLP has one inner width (36) that is no multiple of
8: that boundary stays fp32.

The one known non-equality is an fp32 activation that is positive but rounds
to 0 in bf16 (below 4.6e-41): its mask flips.  The test checks that no activation of the
fp32-buffer trainer is such a value."""
import numpy as np
import pytest
import torch

import oracle as O
from test_gpu_train16 import _rand_batch

pytestmark = pytest.mark.gpu
dev = "cuda:0"
CASE = dict(D=16, rows=[50, 60, 70], bot=[13, 64, 36, 24, 16], top=[64, 48, 32, 1], B=100)


def _trainer(optimizer, device_lr=False, **attrs):
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    c = CASE
    F = len(c["rows"]) + 1
    ln_top = [c["D"] + F * (F - 1) // 2] + c["top"]
    np.random.seed(7)
    ref = O.OracleDLRM(c["D"], c["rows"], c["bot"], ln_top, loss_function="bce")
    cfg = TrainerConfig(m_spa=c["D"], ln_emb=c["rows"], ln_bot=c["bot"], ln_top=ln_top,
                        loss_function="bce", optimizer=optimizer,
                        learning_rate=0.1 if optimizer == "sgd" else 0.01,  # Adagrad: no saturation
                        device_lr=device_lr,
                        mlp_precision=attrs.pop("mlp_precision", "bf16"))
    tr = DLRMTrainer.from_oracle(cfg, ref, device=dev)
    for k, v in attrs.items():
        setattr(tr, k, v)
    return tr


def _state(tr):
    parts = [tr._cur["loss"], tr.params, tr.weights]
    parts += [p for p in (tr.momentum, tr.adagrad_sum, tr.grads) if p is not None]
    return [p.clone() for p in parts]


def _no_flipped_mask(tr):
    for a in tr._cur["bot_act"] + tr._cur["top_act"]:
        assert not bool(((a > 0) & (a.bfloat16() == 0)).any())


@pytest.mark.parametrize("captured", [False, True])
@pytest.mark.parametrize("optimizer, device_lr",
                         [("sgd", False), ("sgd", True), ("rwsadagrad", False)])
def test_store16_step_equals_the_fp32_buffer_step(optimizer, device_lr, captured):
    """device_lr: the fused SGD wgrads read the rate from device memory
    (dlrm_linear16_wgrad_fmt_dev)."""
    rng = np.random.RandomState(3)
    raw = [_rand_batch(rng, CASE["rows"], CASE["B"], 1, CASE["bot"][0], "bce") for _ in range(3)]
    states = {}
    for store16 in (False, True):
        tr = _trainer(optimizer, device_lr, store16=store16)
        batches = [tr.make_batch(*b) for b in raw]
        tr.step(batches[0])
        seen = [_state(tr)]
        if not store16:
            _no_flipped_mask(tr)
        else:  # both 16-bit gradient rotations were written
            assert all(any(bool(g.any()) for g in rot) for rot in tr._cur["store16"][1:])
        run = tr.capture(batches[1]) if captured else None
        for b in batches[1:]:
            run() if captured else tr.step(b)  # captured: two replays of one graph
            torch.cuda.synchronize()
            seen.append(_state(tr))
            if not store16:
                _no_flipped_mask(tr)
        tr.check_errors()
        twins = tr._cur.get("store16", ({},))[0]
        assert len(twins) == (4 if store16 else 0)  # widths 64, 24 (bottom; not 36) and 64, 48
        # the 16-bit path ran: a twinned fp32 buffer was never written, its twin holds r16(y)
        # of the fp32-buffer trainer's activation and kept its constant-1 column
        acts = tr._cur["bot_act"] + tr._cur["top_act"]
        if not store16:
            want = [a.clone() for a in acts]
        for a, w in zip(acts, want):
            t = twins.get(id(a))
            if t is not None:
                N = t.shape[1] - 8
                assert not bool(a[:, :N].any())
                assert torch.equal(t[:, :N], w[:, :N].bfloat16()) and bool((t[:, N] == 1).all())
        states[store16] = seen
    for step, (a, b) in enumerate(zip(states[False], states[True])):
        for x, y in zip(a, b):
            assert torch.equal(x, y), step


def test_store16_refusals():
    rng = np.random.RandomState(3)
    raw = _rand_batch(rng, CASE["rows"], CASE["B"], 1, CASE["bot"][0], "bce")
    tr = _trainer("sgd", store16=True, mlp_precision="fp32")
    with pytest.raises(ValueError, match="store16"):
        tr.step(tr.make_batch(*raw))
    for other in ("group_bwd16", "fuse_bottom16"):
        tr = _trainer("sgd", store16=True, **{other: True})
        with pytest.raises(NotImplementedError, match="§9"):
            tr.step(tr.make_batch(*raw))
    tr = _trainer("sgd", store16=True)
    tr.distributed = True  # what a world_size > 1 trainer sets; no second process needed
    with pytest.raises(NotImplementedError, match="§9"):
        tr._store16({}, "bf16")
