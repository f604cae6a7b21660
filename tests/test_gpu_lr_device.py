"""Device-resident learning rates at kernel level (ABI v14): the schedule's tick kernel
against the reference's recorded doubles, and every consumer of a learning rate called with
a 1-element device tensor against the same call with a Python float, from identical inputs.
Every comparison is bitwise."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
dev = "cuda:0"
LR = 0.3  # as a float argument: np.float32(0.3); as a tensor: the same fp32


@pytest.fixture(scope="module")
def ops():
    from dlrm_hip import ops as o
    return o


def _lr_t(v=LR):
    return torch.tensor([v], dtype=torch.float32, device=dev)


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _both(run):
    """run(lr) -> list of output tensors, with lr a float and then the device tensor: the
    outputs must agree bit for bit (and the float call must have done something)."""
    a = [t.clone() for t in run(LR)]
    b = [t.clone() for t in run(_lr_t())]
    torch.cuda.synchronize()
    assert len(a) == len(b) and a
    for i, (x, y) in enumerate(zip(a, b)):
        assert _same(x, y), f"output {i}: tensor lr differs from float lr"
    return a


# ------------------------------------------------------------------------- tick --
def _configs():
    with open(os.path.join(GOLDEN, "lr_schedule.json")) as f:
        return json.load(f)["configs"]


def _f32_bits(values):
    return np.asarray(values, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("ci", range(7))
def test_tick_walks_every_recorded_iteration(ops, ci):
    c = _configs()[ci]
    base, W, S, D = float.fromhex(c["base"]), c["W"], c["S"], c["D"]
    rec = [float.fromhex(h) for h in c["lr"]]
    assert c["step_counts"] == list(range(1, len(rec) + 1))
    mult = [1.0, 1.0 / 8]
    st = ops.lr_state([base, base], mult, W, S, D, device=dev)
    assert int(st.step.item()) == 1
    # before the first tick: base * mult
    assert (_f32_bits(st.rates.cpu().numpy()) == _f32_bits([np.float32(base * m) for m in mult])).all()
    hist = torch.zeros(len(rec), 2, dtype=torch.float32, device=dev)
    steps = torch.zeros(len(rec), dtype=torch.int64, device=dev)
    for i in range(len(rec)):
        ops.lr_schedule_tick(st)
        hist[i].copy_(st.rates)
        steps[i:i + 1].copy_(st.step)
    got = hist.cpu().numpy()
    assert steps.cpu().tolist() == [sc + 1 for sc in c["step_counts"]]
    for k, m in enumerate(mult):
        want = _f32_bits([np.float32(v * m) for v in rec])
        bad = np.nonzero(_f32_bits(got[:, k]) != want)[0]
        assert bad.size == 0, (W, S, D, k, bad[:4], got[bad[:4], k], [rec[j] * m for j in bad[:4]])


def test_tick_at_the_mlperf_step_counts(ops):
    c = _configs()[7]
    base, W, S, D = float.fromhex(c["base"]), c["W"], c["S"], c["D"]
    assert (base, W, S, D) == (24.0, 2750, 49315, 27772)
    mult = [1.0, 1.0 / 8]
    st = ops.lr_state([base, base], mult, W, S, D, device=dev)
    n = len(c["step_counts"])
    hist = torch.zeros(n, 2, dtype=torch.float32, device=dev)
    steps = torch.zeros(n, dtype=torch.int64, device=dev)
    for i, sc in enumerate(c["step_counts"]):
        st.step.fill_(sc)
        ops.lr_schedule_tick(st)
        hist[i].copy_(st.rates)
        steps[i:i + 1].copy_(st.step)
    got = hist.cpu().numpy()
    assert steps.cpu().tolist() == [sc + 1 for sc in c["step_counts"]]
    for k, m in enumerate(mult):
        want = _f32_bits([np.float32(float.fromhex(h) * m) for h in c["lr"]])
        assert (_f32_bits(got[:, k]) == want).all(), (k, got[:, k])


def test_tick_without_a_policy_and_bad_policies(ops):
    st = ops.lr_state([0.1, 0.05, 0.1], [1.0, 1.0, 1.0 / 8], device=dev)
    for _ in range(3):
        ops.lr_schedule_tick(st)
    assert int(st.step.item()) == 4
    want = _f32_bits([np.float32(0.1), np.float32(0.05), np.float32(0.1 * (1.0 / 8))])
    assert (_f32_bits(st.rates.cpu().numpy()) == want).all()
    st.base.copy_(torch.tensor([0.2, 0.01, 0.2], dtype=torch.float64))
    ops.lr_schedule_tick(st)
    want = _f32_bits([np.float32(0.2), np.float32(0.01), np.float32(0.2 * (1.0 / 8))])
    assert (_f32_bits(st.rates.cpu().numpy()) == want).all()
    for W, S, D in [(5, 4, 3), (0, 2, 4), (1, 2, 4)]:
        with pytest.raises(ValueError):
            ops.lr_state([0.1], None, W, S, D, device=dev)
    with pytest.raises(ValueError):
        ops.lr_state([0.1] * 9, device=dev)
    with pytest.raises(ValueError):  # a rate argument must be ONE fp32 on the device
        ops.sgd_update(torch.zeros(4, device=dev), torch.zeros(4, device=dev),
                       torch.zeros(2, device=dev))
    with pytest.raises(ValueError):
        ops.sgd_update(torch.zeros(4, device=dev), torch.zeros(4, device=dev), torch.zeros(1))


# ------------------------------------------------------------- dense optimizers --
@pytest.mark.parametrize("n", [1, 1025])
def test_sgd_update(ops, n):
    torch.manual_seed(n)
    p0, g = torch.randn(n, device=dev), torch.randn(n, device=dev)

    def run(lr):
        p = p0.clone()
        ops.sgd_update(p, g, lr)
        return [p]
    assert not _same(_both(run)[0], p0)


@pytest.mark.parametrize("n", [1, 1025])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_adagrad_update_and_its_scaled_form(ops, n, grad_scale):
    torch.manual_seed(n + 1)
    p0, g, s0 = torch.randn(n, device=dev), torch.randn(n, device=dev), torch.rand(n, device=dev)

    def run(lr):
        p, s = p0.clone(), s0.clone()
        ops.adagrad_update(p, g, s, lr, 1e-8, grad_scale=grad_scale)
        return [p, s]
    assert not _same(_both(run)[0], p0)


def test_colsum_with_sgd_param(ops):
    torch.manual_seed(2)
    M, N = 33, 5
    Y, scale = torch.randn(M, N, device=dev), torch.randn(M, device=dev)
    w0 = torch.randn(N, device=dev)

    def run(lr):
        w, out = w0.clone(), torch.zeros(N, device=dev)
        ops.colsum(Y, scale=scale, alpha=0.5, out=out, sgd_param=w, lr=lr)
        return [w, out]
    assert not _same(_both(run)[0], w0)


@pytest.mark.parametrize("K", [5, 260])
@pytest.mark.parametrize("defer", [False, True])
def test_head_step_and_its_deferred_role_pass(ops, K, defer):
    torch.manual_seed(K)
    M = 33
    X = torch.randn(M, K, device=dev).relu()
    X[:, K - 1] = 1.0
    w0 = torch.randn(K, device=dev) * 0.1
    t = torch.rand(M, device=dev).round()
    A1, B1 = torch.randn(70, 36, device=dev), torch.randn(36, 64, device=dev)

    def run(lr):
        w = w0.clone()
        prob, dz, L = (torch.empty(M, device=dev), torch.empty(M, device=dev),
                       torch.empty(1, device=dev))
        dX = torch.empty(M, K, device=dev)
        kw = dict(prob=prob, dz=dz, loss_out=L, dX=dX, relu_mask=True, lr=lr)
        if defer:
            role = ops.head_step(X, w, t, "bce", 0.0, 1.0, defer=True, **kw)
            assert ops.role_blocks(role) > 0
            p1, c1 = ops.gemm_problem(A1, B1)
            ops.gemm_group([p1], None, dev, role=role, phase=4)
        else:
            ops.head_step(X, w, t, "bce", 0.0, 1.0, **kw)
        return [w, prob, dz, L, dX]
    assert not _same(_both(run)[0], w0)


# ------------------------------------------------------------------------- GEMM --
def _gemm_case(M, N, K, seed):
    """A wgrad-shaped problem: C [M, ldc] -= alpha * A^T B, A [K, M], B [K, N(+pad)]."""
    torch.manual_seed(seed)
    A = torch.randn(K, M, device=dev)
    Bm = torch.randn(K, N, device=dev)
    C0 = torch.randn(M, N + 4, device=dev)
    return A, Bm, C0


@pytest.mark.parametrize("ones", [False, True])
@pytest.mark.parametrize("M,N,K,split", [(64, 64, 64, False), (64, 64, 2048, True)])
def test_gemm_epi_sgd_aligned_and_split_k(ops, M, N, K, split, ones):
    A, Bm, C0 = _gemm_case(M, N, K, K + ones)
    ws = torch.zeros(32 << 20, dtype=torch.uint8, device=dev)

    def run(lr):
        C = C0.clone()
        pr, _ = ops.gemm_problem(A, Bm, trans_a=True, C=C[:, :N + 4] if ones else C[:, :N],
                                 alpha=lr, epilogue=ops.EPI_SGD, ones_col=N if ones else -1)
        assert (ops.gemm_splits(pr) > 1) == split
        ops.gemm_group([pr], ws, dev)
        return [C]
    assert not _same(_both(run)[0], C0)


@pytest.mark.parametrize("ones", [False, True])
def test_gemm_partial_then_reduce_across_two_launches(ops, ones):
    M, N, K = 64, 64, 2048
    A, Bm, C0 = _gemm_case(M, N, K, 5 + ones)
    ws = torch.zeros(32 << 20, dtype=torch.uint8, device=dev)

    def run(lr):
        C = C0.clone()
        kw = dict(trans_a=True, C=C[:, :N + 4] if ones else C[:, :N], alpha=lr,
                  epilogue=ops.EPI_SGD, ones_col=N if ones else -1)
        s = ops.gemm_splits(ops.gemm_problem(A, Bm, **kw)[0], partial=True)
        assert s > 1
        part = torch.empty(ops.gemm_partial_bytes(M, N, s) // 4, device=dev)
        pp, _ = ops.gemm_problem(A, Bm, partial=part, splits=s, **kw)
        ops.gemm_group([pp], ws, dev)
        assert _same(C, C0)  # PARTIAL does not touch C
        ops.gemm_group([ops.reduce_problem(pp)], ws, dev)
        return [C]
    assert not _same(_both(run)[0], C0)


@pytest.mark.parametrize("ones", [False, True])
def test_gemm_unaligned_generic_path(ops, ones):
    M, N, K = 33, 20, 13  # K % 4 != 0: the generic kernel (+ its row-sum kernel)
    torch.manual_seed(13 + ones)
    A = torch.randn(M, K, device=dev)
    Bm = torch.randn(K, N, device=dev)
    C0 = torch.randn(M, N + 4, device=dev)

    def run(lr):
        C = C0.clone()
        pr, _ = ops.gemm_problem(A, Bm, C=C[:, :N + 4] if ones else C[:, :N], alpha=lr,
                                 epilogue=ops.EPI_SGD, ones_col=N if ones else -1)
        ops.gemm_group([pr], None, dev)
        return [C]
    assert not _same(_both(run)[0], C0)


def test_sgd_job(ops):
    torch.manual_seed(9)
    n = 1028
    p0, g = torch.randn(n, device=dev), torch.randn(n, device=dev)
    A1, B1 = torch.randn(70, 36, device=dev), torch.randn(36, 64, device=dev)

    def run(lr):
        p = p0.clone()
        p1, c1 = ops.gemm_problem(A1, B1)
        ops.gemm_group([p1, ops.sgd_job(p, g, lr)], None, dev)
        return [p, c1]
    assert not _same(_both(run)[0], p0)


# -------------------------------------------------------------------------- TBE --
def _tbe_case(D, seed):
    """T = 3 tables, B = 16, two lookups per bag; table 0 has three rows, so its 32 lookups
    form runs longer than a 16-lookup block (they cross blocks: the combine pass runs)."""
    T, B, L = 3, 16, 2
    rows = [3, 50, 7]
    rng = np.random.RandomState(seed)
    idx = np.concatenate([rng.randint(0, n, size=B * L) for n in rows]).astype(np.int32)
    off = np.arange(0, T * B * L + 1, L, dtype=np.int32)
    row_base = torch.tensor([0] + np.cumsum(rows).tolist(), dtype=torch.int64, device=dev)
    torch.manual_seed(seed)
    W0 = torch.randn(sum(rows), D, device=dev) * 0.1
    mom0 = torch.rand(sum(rows), device=dev)
    G = torch.randn(B, T, D, device=dev)
    return T, B, L, torch.tensor(idx, device=dev), torch.tensor(off, device=dev), row_base, W0, \
        mom0, G


@pytest.mark.parametrize("mode", ["sgd", "rowwise_adagrad"])
@pytest.mark.parametrize("D", [4, 128])
def test_tbe_backward(ops, mode, D):
    T, B, L, idx, off, row_base, W0, mom0, G = _tbe_case(D, D)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def run(lr):
        W, mom = W0.clone(), mom0.clone()
        ops.tbe_backward(mode, W, row_base, T, B, idx, off, G, lr=lr, eps=1e-8, momentum=mom,
                         max_lookups_per_table=B * L, error_flag=flag)
        return [W, mom]
    out = _both(run)
    assert not _same(out[0], W0) and int(flag.item()) == 0


@pytest.mark.parametrize("mode", ["sgd", "rowwise_adagrad"])
@pytest.mark.parametrize("D", [4, 128])
def test_tbe_backward_defer_with_both_role_phases(ops, mode, D):
    T, B, L, idx, off, row_base, W0, mom0, G = _tbe_case(D, D + 1)
    A1, B1 = torch.randn(70, 36, device=dev), torch.randn(36, 64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def run(lr):
        W, mom = W0.clone(), mom0.clone()
        role = ops.tbe_backward_defer(mode, W, row_base, T, B, idx, off, G, lr=lr, eps=1e-8,
                                      momentum=mom, max_lookups_per_table=B * L,
                                      error_flag=flag)
        assert (role is not None) == (D == 128)  # D = 4: the update ran in full already
        p1, c1 = ops.gemm_problem(A1, B1)
        ops.gemm_group([p1], None, dev, role=role, phase=1)
        if role is not None:
            ops.gemm_group([], None, dev, role=role, phase=2)
        return [W, mom, c1]
    out = _both(run)
    assert not _same(out[0], W0) and int(flag.item()) == 0
    # the deferred update is the undeferred one
    W, mom = W0.clone(), mom0.clone()
    ops.tbe_backward(mode, W, row_base, T, B, idx, off, G, lr=_lr_t(), eps=1e-8, momentum=mom,
                     max_lookups_per_table=B * L, error_flag=flag)
    torch.cuda.synchronize()
    assert _same(W, out[0]) and _same(mom, out[1])


# --------------------------------------------------------------- 16-bit wgrad --
@pytest.mark.parametrize("split", [0, 1, 4])
def test_linear16_wgrad_sgd(ops, split):
    torch.manual_seed(split)
    M, N, K = 130, 33, 14
    g, x = torch.randn(M, N, device=dev), torch.randn(M, K, device=dev)
    C0 = torch.randn(N, K, device=dev)

    def run(lr):
        C = C0.clone()
        ops.linear16_wgrad(g, x, C, lr=lr, dtype="bf16")
        return [C]
    with ops.tuning(**({"linear16_wgrad_split": split} if split else {})):
        assert not _same(_both(run)[0], C0)


# ---------------------------------------------------------------- graph replay --
def test_captured_update_follows_the_tensor(ops):
    """The property the feature exists for: a captured launch reads its rate when it runs."""
    torch.manual_seed(4)
    n = 1025
    p0, g = torch.randn(n, device=dev), torch.randn(n, device=dev)
    want = []
    for lr in (0.3, 0.07):
        p = p0.clone()
        ops.sgd_update(p, g, lr)
        want.append(p)
    lr_t = _lr_t(0.3)
    p = p0.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.sgd_update(p, g, lr_t)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.sgd_update(p, g, lr_t)
    p.copy_(p0)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(p, want[0])
    p.copy_(p0)
    lr_t.fill_(0.07)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(p, want[1]) and not _same(want[0], want[1])
