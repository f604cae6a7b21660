"""Host side of the mixed-precision training step (no GPU): the CPU reference train16_ref
against the oracle, the exactness of its rounded Linear on integer inputs, the config field,
and the ABI of dlrm_linear16_dgrad / dlrm_linear16_wgrad with their argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import oracle as O
import train16_ref as T16
from conftest import ROOT, fp32_close
from linear16_ref import r16

P = ctypes.c_void_p


def _small_model(seed=5):
    rows, bot = [50, 60, 70], [13, 32, 8]
    ln_top = [8 + 6, 16, 8, 1]
    np.random.seed(seed)
    ref = O.OracleDLRM(8, rows, bot, ln_top, loss_function="bce")
    rng = np.random.RandomState(seed)
    B = 64
    X = np.log1p(rng.rand(B, 13).astype(np.float32))
    lS_o = np.array([np.arange(B) for _ in rows], dtype=np.int64)
    lS_i = [rng.randint(0, n, size=B).astype(np.int64) for n in rows]
    T = np.round(rng.rand(B, 1)).astype(np.float32)
    return ref, X, lS_o, lS_i, T


def test_reference_without_rounding_is_the_oracles_train_step():
    ref, X, lS_o, lS_i, T = _small_model()
    m = T16.clone64(ref)
    before = [p.detach().clone() for p in ref.parameters()]
    prob, loss = T16.train_step(m, X, lS_o, lS_i, T, 0.1, None)
    for p, b in zip(ref.parameters(), before):  # the caller's model is untouched
        assert torch.equal(p.detach(), b)
    Z, E = ref.train_step(torch.tensor(X), torch.tensor(lS_o), [torch.tensor(i) for i in lS_i],
                          torch.tensor(T), 0.1)
    ok, msg = fp32_close(prob, Z.numpy().ravel())
    assert ok, msg
    ok, msg = fp32_close([loss], [float(E)])
    assert ok, msg
    moved = 0
    for (name, p), q, b in zip(ref.named_parameters(), m.parameters(), before):
        ok, msg = fp32_close(q.detach().numpy(), p.detach().numpy())
        assert ok, (name, msg)
        moved += int(not torch.equal(p.detach(), b))
    assert moved == len(before)


def test_rounding_changes_the_step_by_about_the_types_epsilon():
    ref, X, lS_o, lS_i, T = _small_model()
    m0, mb = T16.clone64(ref), T16.clone64(ref)
    p0, _ = T16.train_step(m0, X, lS_o, lS_i, T, 0.1, None)
    pb, _ = T16.train_step(mb, X, lS_o, lS_i, T, 0.1, "bf16")
    assert 0.0 < np.abs(pb - p0).max() < 0.05
    head = [m for m in mb.top_l if isinstance(m, torch.nn.Linear)][-1]
    for (name, a), b in zip(m0.named_parameters(), mb.parameters()):
        q = float((a - b).abs().max())
        assert 0.0 < q < 0.05, (name, q)
    assert head.weight.dtype == torch.float64
    # a second step runs from the updated fp64 weights
    p1 = T16.predict(mb, X, lS_o, lS_i, "bf16")
    assert p1.shape == pb.shape and (p1 != pb).any()


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_rounded_linear_is_exact_on_integers(dt):
    """Integer x, W, g in [-4, 4] are exact in both types: the three gradients of the rounded
    Linear are bitwise the integer results, through linear16_grads and through autograd."""
    g = torch.Generator().manual_seed(9)
    M, N, K = 33, 17, 13
    x = torch.randint(-4, 5, (M, K), generator=g).double()
    W = torch.randint(-4, 5, (N, K), generator=g).double().requires_grad_()
    b = torch.randint(-4, 5, (N,), generator=g).double().requires_grad_()
    go = torch.randint(-4, 5, (M, N), generator=g).double()
    xin = x.clone().requires_grad_()
    y = T16.Linear16.apply(xin, W, b, dt)
    assert torch.equal(y.detach(), x @ W.detach().t() + b.detach())
    y.backward(go)
    want = (go @ W.detach(), go.t() @ x, go.sum(0))
    for got, w in zip((xin.grad, W.grad, b.grad), want):
        assert torch.equal(got, w)
    for got, w in zip(T16.linear16_grads(x, W.detach(), go, dt), want):
        assert torch.equal(got, w)
    # ... and on full-mantissa values every one of the three sees the rounded g
    gf = torch.rand(M, N, generator=g, dtype=torch.float64) + 1.0
    gx, gW, gb = T16.linear16_grads(x, W.detach(), gf, dt)
    assert torch.equal(gb, r16(gf, dt).sum(0)) and not torch.equal(gb, gf.sum(0))
    assert torch.equal(gx, r16(gf, dt) @ W.detach()) and torch.equal(gW, r16(gf, dt).t() @ x)


def test_trainer_config_field():
    from dlrm_hip.trainer import TrainerConfig
    kw = dict(m_spa=4, ln_emb=[8], ln_bot=[4, 4], ln_top=[5, 1])
    assert TrainerConfig(**kw).mlp_precision == "fp32"
    assert TrainerConfig(**kw, mlp_precision="bf16").mlp_precision == "bf16"
    with pytest.raises(NotImplementedError) as e:
        TrainerConfig(**kw, mlp_precision="fp16")
    assert "loss scaling" in str(e.value)
    with pytest.raises(ValueError):
        TrainerConfig(**kw, mlp_precision="int8")


def _proto(hdr, name):
    text = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"(int|size_t) " + name + r"\((.*?)\);", text, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
             "size_t": ctypes.c_size_t}
    args = [a.strip() for a in m.group(2).split(",")]
    return m.group(1), [P if "*" in a or a.startswith("dlrm_stream_t") else ctype[a.split()[0]]
                        for a in args]


def test_header_bindings_and_source_agree():
    from dlrm_hip import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()
    assert int(re.search(r"#define\s+DLRM_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 13
    assert _lib.ABI_VERSION >= 13 and _lib.load().dlrm_abi_version() == _lib.ABI_VERSION
    assert re.search(r"^ \* 13:", hdr, flags=re.M)  # the version history line
    src = open(os.path.join(ROOT, "dlrm-yx_amd", "csrc", "linear16_bwd.hip")).read()
    for name, nargs, res in (("dlrm_linear16_dgrad", 13, ctypes.c_int32),
                             ("dlrm_linear16_wgrad", 15, ctypes.c_int32),
                             ("dlrm_linear16_wgrad_workspace_size", 4, ctypes.c_size_t)):
        kind, want = _proto(hdr, name)
        got_res, sig = _lib.SIGNATURES[name]
        assert got_res is res and sig == want and len(sig) == nargs, name
        assert hasattr(_lib.load(), name)
        assert f'extern "C" {kind} {name}(' in src
    assert "linear16_bwd.hip" in open(os.path.join(ROOT, "dlrm-yx_amd", "csrc", "Makefile")).read()
    assert re.search(r"DLRM_WGRAD16_STORE = 0, DLRM_WGRAD16_SGD = 1", hdr)
    assert (ops.WGRAD16_STORE, ops.WGRAD16_SGD) == (0, 1)
    for key, enum in (("linear16_dgrad_tile", "DLRM_TUNE_LINEAR16_DGRAD_TILE"),
                      ("linear16_wgrad_tile", "DLRM_TUNE_LINEAR16_WGRAD_TILE"),
                      ("linear16_wgrad_split", "DLRM_TUNE_LINEAR16_WGRAD_SPLIT")):
        assert ops.TUNE_KEYS[key] == int(re.search(enum + r" = (\d+)", hdr).group(1))
    # appended: the existing keys keep their values
    assert [ops.TUNE_KEYS[k] for k in ("gemm_tile", "gemm_split", "tbe_block", "tbe_sort",
                                       "tbe_lean", "interact_bwd", "interact_fwd",
                                       "linear16_tile")] == list(range(1, 9))
    assert ops.LINEAR16_DGRAD_TILES == ops.LINEAR16_WGRAD_TILES == (128128, 128064, 64064, 32064)


def test_argument_validation_without_a_device():
    """Every check runs before the first HIP call (fake non-null pointers are never used)."""
    from dlrm_hip import _lib, ops
    lib = _lib.load()
    p = P(4096)
    OK, INVALID, SHAPE, WORKSPACE = 0, 1, 2, 4
    good = dict(type=0, M=4, N=3, K=8, dY=p, lddy=3, W=p, ldw=8, mask=None, ldmask=0, dX=p,
                lddx=8, stream=None)

    def dgrad(**kw):
        a = dict(good, **kw)
        return int(lib.dlrm_linear16_dgrad(*[a[k] for k in good]))

    assert dgrad(type=2) == INVALID and dgrad(M=-1) == INVALID and dgrad(N=-1) == INVALID
    assert dgrad(dY=None) == INVALID and dgrad(W=None) == INVALID and dgrad(dX=None) == INVALID
    assert "null" in lib.dlrm_last_error().decode()
    assert dgrad(lddy=2) == SHAPE and dgrad(ldw=7) == SHAPE and dgrad(lddx=7) == SHAPE
    assert dgrad(mask=p, ldmask=7) == SHAPE
    assert dgrad(M=0) == OK and dgrad(K=0, ldw=0, lddx=0) == OK and dgrad(M=0, type=5) == INVALID
    with ops.tuning(linear16_dgrad_tile=64032):
        assert dgrad() == INVALID

    goodw = dict(type=0, M=256, N=3, K=8, dY=p, lddy=3, X=p, ldx=8, mode=0, lr=0.0, C=p, ldc=8,
                 ws=None, wsb=0, stream=None)

    def wgrad(**kw):
        a = dict(goodw, **kw)
        return int(lib.dlrm_linear16_wgrad(*[a[k] for k in goodw]))

    assert wgrad(type=2) == INVALID and wgrad(mode=2) == INVALID and wgrad(K=-1) == INVALID
    assert wgrad(dY=None) == INVALID and wgrad(X=None) == INVALID and wgrad(C=None) == INVALID
    assert wgrad(lddy=2) == SHAPE and wgrad(ldx=7) == SHAPE and wgrad(ldc=7) == SHAPE
    assert wgrad(N=0) == OK and wgrad(M=0, mode=1, dY=None, X=None) == OK
    with ops.tuning(linear16_wgrad_tile=64032):
        assert wgrad() == INVALID
        assert ops.linear16_wgrad_workspace_size(256, 3, 8) == 0
    with ops.tuning(linear16_wgrad_split=4):
        assert ops.linear16_wgrad_workspace_size(256, 3, 8) == 4 * 3 * 8 * 4
        assert ops.linear16_wgrad_workspace_size(100, 3, 8) == 2 * 3 * 8 * 4  # two 64-row steps
        assert wgrad() == WORKSPACE and wgrad(ws=p, wsb=4 * 3 * 8 * 4 - 1) == WORKSPACE
    with ops.tuning(linear16_wgrad_split=1):
        assert ops.linear16_wgrad_workspace_size(4096, 512, 15) == 0
    for key in ("linear16_dgrad_tile", "linear16_wgrad_tile"):
        for tile in ops.LINEAR16_TILES:
            with ops.tuning(**{key: tile}):
                assert lib.dlrm_get_tuning(ops.TUNE_KEYS[key]) == tile
        assert lib.dlrm_get_tuning(ops.TUNE_KEYS[key]) == 0


def test_ops_wrappers_reject_cpu_tensors_and_bad_dtype():
    from dlrm_hip import ops
    g, w, x = torch.zeros(2, 3), torch.zeros(3, 4), torch.zeros(2, 4)
    with pytest.raises(ValueError):
        ops.linear16_dgrad(g, w)
    with pytest.raises(ValueError):
        ops.linear16_dgrad(g, w, dtype="int8")
    with pytest.raises(ValueError):
        ops.linear16_wgrad(g, x, torch.zeros(3, 4))
    with pytest.raises(ValueError):
        ops.linear16_wgrad(g, x, torch.zeros(3, 4), dtype="int8")
