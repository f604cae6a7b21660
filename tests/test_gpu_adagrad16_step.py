"""fp16 tables under row-wise Adagrad in the engine and the module.  §18's
criterion, BITWISE: the fp16-table trainer against the fp32-table trainer of the same config and
seed whose tables are rounded to fp16 after every step (.half(), or the host's sr16 of the step's
stream) - tables, momentum, dense weights and loss."""
import pytest
import torch

import exact_sr16 as X
from exact_tbe import bits_equal

pytestmark = pytest.mark.gpu
dev = "cuda:0"
ROWS, D, B, SEED = [300, 257, 64], 16, 32, 2024
STATE = ("weights", "params", "momentum", "adagrad_sum")
POLICY = dict(lr_num_warmup_steps=2, lr_decay_start_step=3, lr_num_decay_steps=2)


def _trainer(**kw):
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    cfg = TrainerConfig(m_spa=D, ln_emb=ROWS, ln_bot=[13, 32, D], ln_top=[D + 6, 32, 1],
                        loss_function="bce", learning_rate=0.1, emb_learning_rate=0.3, **kw)
    return DLRMTrainer(cfg, device=dev, seed=3)


def _pair(stochastic, **kw):
    """A: fp16 tables.  S, the shadow: fp32 tables holding A's values, the same dense bucket."""
    kw.setdefault("optimizer", "rwsadagrad")
    sr = dict(emb_rounding="stochastic", emb_rounding_seed=SEED) if stochastic else {}
    A = _trainer(emb_precision="fp16", emb_optimizer="rwsadagrad", **sr, **kw)
    S = _trainer(emb_optimizer="rwsadagrad", **kw)
    S.weights.copy_(A.weights.float())
    S.params.copy_(A.params)
    return A, S


def _captured(A, batch):
    """A replayable step on a batch of its own: one eager step for the allocations, then every
    state put back."""
    from dlrm_hip.trainer import Batch
    fixed = Batch(*(t.clone() for t in (batch.X, batch.offsets, batch.indices, batch.target)),
                  batch.max_per_table, batch.one_hot)
    live = [getattr(A, n) for n in STATE if getattr(A, n) is not None]
    keep = [t.clone() for t in live]
    A.step(fixed)
    for dst, src in zip(live, keep):
        dst.copy_(src)
    if A.cfg.emb_rounding == "stochastic":
        A.set_rounding_state(SEED, 0)
    if A.cfg.lr_mode == "device":
        A.lr_step = 1
    return fixed, A.capture(fixed)


@pytest.mark.parametrize("L,graph,stochastic,kw", [  # bag length, captured, store, extra config
    (1, False, False, {}), (1, True, False, {}), (3, False, False, {}), (3, True, False, {}),
    (1, False, True, {}), (3, True, True, {}),
    (1, True, True, dict(optimizer="sgd", mlp_precision="bf16", **POLICY))])
def test_step_equals_the_rounded_fp32_shadow(L, graph, stochastic, kw):
    A, S = _pair(stochastic, **kw)
    batches = [A.synthetic_batch(B, L, seed=s) for s in (11, 12)]
    W0 = A.weights.clone()
    if graph:
        fixed, run = _captured(A, batches[0])
    for i in range(3):
        b = batches[i % 2]
        if graph:
            for dst, src in zip((fixed.X, fixed.indices, fixed.target),
                                (b.X, b.indices, b.target)):
                dst.copy_(src)
            run()
            la = A._cur["loss"]
        else:
            la = A.step(b)[1]
        ls = S.step(b)[1]
        w = S.weights.cpu()  # the shadow's tables, rounded as the step's store rounds
        h = torch.from_numpy(X.sr16_table(w.numpy(), SEED, i)) if stochastic else w.half()
        S.weights.copy_(h.float())
        assert A.gather_fused == S.gather_fused == (L == 1)  # else the pooled fp16 lookup
        assert bits_equal(la, ls), (i, la.item(), ls.item())
        assert bits_equal(A.weights.cpu(), h) and bits_equal(A.momentum, S.momentum), i
        assert bits_equal(A.params, S.params), i
    assert not bits_equal(A.weights, W0) and float(A.momentum.max()) > 0
    if stochastic and not graph:  # a resume from (state, (seed, step)) continues exactly
        assert A.rounding_state() == (SEED, 3)
        R, _ = _pair(stochastic, **kw)
        for n in STATE:
            getattr(R, n).copy_(getattr(S, n))
        R.set_rounding_state(SEED, 3)
        A.step(batches[1]), R.step(batches[1])
        assert R.rounding_state() == (SEED, 4)
        assert bits_equal(R.weights, A.weights) and bits_equal(R.momentum, A.momentum)
    A.check_errors()


def test_dense_sgd_with_rowwise_adagrad_tables():
    """optimizer="sgd", emb_optimizer="rwsadagrad" on fp32 tables: the dense weights as the
    all-SGD run's (same gradients: one step from the same state), the tables and momentum as
    ops.tbe_backward("rowwise_adagrad") applies the step's embedding gradient."""
    from dlrm_hip import ops
    M, G = _trainer(optimizer="sgd", emb_optimizer="rwsadagrad"), _trainer(optimizer="sgd")
    assert M.momentum is not None and M.adagrad_sum is None and G.momentum is None
    b = M.synthetic_batch(B, 3, seed=11)
    W0, mom = M.weights.clone(), torch.zeros_like(M.momentum)
    M.step(b), G.step(b)
    assert bits_equal(M.params, G.params)
    dE = G._cur["dE"]  # the step's gradient of the pooled embeddings, [B, T, D]
    ops.tbe_backward("rowwise_adagrad", W0, M.row_base, len(ROWS), B, b.indices, b.offsets, dE,
                     lr=M.emb_lr, eps=M.cfg.adagrad_eps, momentum=mom,
                     grad_batch_stride=dE.stride(0), max_lookups_per_table=b.max_per_table)
    assert bits_equal(M.weights, W0) and bits_equal(M.momentum, mom) and float(mom.max()) > 0


@pytest.mark.parametrize("sr", [False, True])
def test_module_rowwise_adagrad(sr):
    from dlrm_hip import ops
    from dlrm_hip.modules import SplitTableBatchedEmbeddingBags
    g = torch.Generator().manual_seed(5)
    tabs = [torch.randn(n, D, generator=g) * 0.05 for n in ROWS]
    M = SplitTableBatchedEmbeddingBags([(n, D) for n in ROWS], learning_rate=0.25, eps=1e-3,
                                       tables=tabs, seed=SEED, device=dev, stochastic_rounding=sr,
                                       optimizer="rowwise_adagrad")
    assert M.state_dict()["momentum"].dtype == torch.float32
    idx = torch.cat([torch.randint(0, n, (B * 2,), generator=g) for n in ROWS]).int().to(dev)
    off = (torch.arange(len(ROWS) * B + 1) * 2).int().to(dev)
    G = torch.randn(B, len(ROWS) * D, generator=g).to(dev)
    W, mom = M.weights.data.clone(), torch.zeros(sum(ROWS), device=dev)
    for step in range(2):
        M(idx, off).backward(G)
        ops.tbe_backward("rowwise_adagrad", W, M.table_offsets, len(ROWS), B, idx, off, G,
                         lr=0.25, eps=1e-3, momentum=mom,
                         sr_state=ops.sr_state(SEED, step, device=dev) if sr else None)
        assert bits_equal(M.weights.data, W) and bits_equal(M.momentum, mom), step
    assert float(mom.max()) > 0
