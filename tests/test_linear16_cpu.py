"""Host side of the 16-bit MLP inference path (no GPU): the ABI of dlrm_linear16_forward, its
argument checks, the CPU reference linear16_ref against the oracle, and proofs that the
inputs of the GPU tests discriminate (a truncating or an unrounded kernel gives another
expected matrix; the tiny exact model's activations stay exact in the 16-bit types)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import linear16_ref as R
import oracle as O
from conftest import ROOT, fp32_close
from exact_inputs import full_mantissa, one_hot_rows, truncate_mantissa

P = ctypes.c_void_p


def test_header_bindings_and_source_agree():
    from dlrm_hip import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()
    assert int(re.search(r"#define\s+DLRM_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 12
    assert _lib.ABI_VERSION >= 12 and _lib.load().dlrm_abi_version() == _lib.ABI_VERSION
    assert re.search(r"^ \* 12:", hdr, flags=re.M)  # the version history line
    proto = re.search(r"int dlrm_linear16_forward\((.*?)\);", re.sub(r"/\*.*?\*/", "", hdr,
                                                                     flags=re.S), flags=re.S)
    args = [a.strip() for a in proto.group(1).split(",")]
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    want = [P if "*" in a or a.startswith("dlrm_stream_t") else ctype[a.split()[0]] for a in args]
    res, sig = _lib.SIGNATURES["dlrm_linear16_forward"]
    assert res is ctypes.c_int32 and sig == want and len(sig) == 14
    assert hasattr(_lib.load(), "dlrm_linear16_forward")
    src = open(os.path.join(ROOT, "dlrm-yx_amd", "csrc", "linear16.hip")).read()
    assert 'extern "C" int dlrm_linear16_forward(' in src
    assert "linear16.hip" in open(os.path.join(ROOT, "dlrm-yx_amd", "csrc", "Makefile")).read()
    # enum values and the tuning key the Python side mirrors
    assert re.search(r"DLRM_MLP16_BF16 = 0, DLRM_MLP16_F16 = 1", hdr)
    assert ops.MLP16_TYPES == {"bf16": 0, "fp16": 1}
    key = int(re.search(r"DLRM_TUNE_LINEAR16_TILE = (\d+)", hdr).group(1))
    assert ops.TUNE_KEYS["linear16_tile"] == key


def _status(*args):
    from dlrm_hip import _lib
    return int(_lib.load().dlrm_linear16_forward(*args))


def test_argument_validation_without_a_device():
    """Every check runs before the first HIP call (fake non-null pointers are never used)."""
    from dlrm_hip import _lib, ops
    p = P(4096)
    OK, INVALID, SHAPE = 0, 1, 2
    good = dict(type=0, M=4, N=3, K=8, X=p, ldx=8, W=p, ldw=8, bias=None, bs=0, relu=0, Y=p,
                ldy=3, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return _status(*[a[k] for k in good])

    assert call(type=2) == INVALID and call(type=-1) == INVALID
    assert call(M=-1) == INVALID and call(N=-1) == INVALID and call(K=-1) == INVALID
    assert call(X=None) == INVALID and call(W=None) == INVALID and call(Y=None) == INVALID
    assert "null" in _lib.load().dlrm_last_error().decode()
    assert call(ldx=7) == SHAPE and call(ldw=7) == SHAPE and call(ldy=2) == SHAPE
    assert call(M=0) == OK and call(M=0, X=None, Y=None) == OK  # nothing to do
    assert call(M=0, type=5) == INVALID  # ... but still a checked call
    with ops.tuning(linear16_tile=64032):  # not one of this kernel's tiles
        assert call() == INVALID
    with pytest.raises(_lib.DLRMHipError) as e:
        _lib.call("dlrm_linear16_forward", 0, 4, 3, 8, p, 4, p, 8, None, 0, 0, p, 3, None)
    assert e.value.code == SHAPE
    for tile in ops.LINEAR16_TILES:  # every tile is a value the key accepts
        with ops.tuning(linear16_tile=tile):
            assert _lib.load().dlrm_get_tuning(ops.TUNE_KEYS["linear16_tile"]) == tile
    assert _lib.load().dlrm_get_tuning(ops.TUNE_KEYS["linear16_tile"]) == 0


def test_ops_wrapper_rejects_cpu_tensors_and_bad_dtype():
    from dlrm_hip import ops
    x, w = torch.zeros(2, 4), torch.zeros(3, 4)
    with pytest.raises(ValueError):
        ops.linear16_forward(x, w)
    with pytest.raises(ValueError):
        ops.linear16_forward(x, w, dtype="int8")


def test_trainer_and_module_reject_bad_precision():
    from dlrm_hip.dlrm_net import DLRM_Net
    from dlrm_hip.modules import HipMLP
    from dlrm_hip import trainer
    assert trainer.PRECISIONS == ("fp32", "bf16", "fp16")
    np.random.seed(1)
    net = DLRM_Net(4, np.array([10, 10]), np.array([3, 4]), np.array([7, 1]),
                   arch_interaction_op="dot", sigmoid_top=0)
    keys = list(net.state_dict())
    with pytest.raises(NotImplementedError) as e:
        net.quantize_mlp(8)
    assert "quantize-mlp-with-bit" in str(e.value)
    with pytest.raises(ValueError):
        net.quantize_mlp(16, "int8")
    with pytest.raises(ValueError):
        net.quantize_mlp(4)
    assert isinstance(net.bot_l, HipMLP) and net.bot_l.mlp16 is None
    net.quantize_mlp(16)
    assert net.bot_l.mlp16 == net.top_l.mlp16 == "fp16"  # the reference's type by default
    assert list(net.state_dict()) == keys
    with pytest.raises(RuntimeError):  # grad enabled: refused before any launch
        net.bot_l(torch.zeros(2, 3))
    net.quantize_mlp(16, "bf16")
    assert net.top_l.mlp16 == "bf16"
    net.quantize_mlp(32)
    assert net.bot_l.mlp16 is None and net.top_l.mlp16 is None


def _small_model(seed=5):
    rows, bot = [50, 60, 70], [13, 32, 8]
    ln_top = [8 + 6, 16, 1]
    np.random.seed(seed)
    ref = O.OracleDLRM(8, rows, bot, ln_top, loss_function="bce")
    rng = np.random.RandomState(seed)
    B = 64
    X = np.log1p(rng.rand(B, 13).astype(np.float32))
    lS_o = np.array([np.arange(B) for _ in rows], dtype=np.int64)
    lS_i = [rng.randint(0, n, size=B).astype(np.int64) for n in rows]
    return ref, X, lS_o, lS_i


def test_reference_without_rounding_is_the_oracle():
    ref, X, lS_o, lS_i = _small_model()
    with torch.no_grad():
        want = ref(torch.tensor(X), torch.tensor(lS_o), [torch.tensor(i) for i in lS_i])
    got = R.forward(ref, X, lS_o, lS_i, None)
    ok, msg = fp32_close(got, want.numpy().ravel())
    assert ok, msg
    for dt in ("bf16", "fp16"):  # and rounding changes it, by about the type's epsilon
        q = np.abs(R.forward(ref, X, lS_o, lS_i, dt) - got).max()
        assert 0.0 < q < 0.05, (dt, q)


def test_r16_is_round_to_nearest_even():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -9], dtype=torch.float64)
    assert R.r16(x, "bf16").tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0]  # ties to even
    x = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 70000.0], dtype=torch.float64)
    assert R.r16(x, "fp16").tolist() == [1.0, 1.0 + 2.0 ** -9, float("inf")]
    assert R.r16(x, None) is x


@pytest.mark.parametrize("dt,bits", [("bf16", 7), ("fp16", 10)])
def test_rounding_inputs_discriminate(dt, bits):
    """On test_gpu_linear16's rounding-mode inputs a truncating conversion, and no conversion
    at all, both give expected matrices different from the RNE one."""
    tdt = R.DTYPES[dt]
    for (M, N, K) in ((33, 40, 96), (5, 3, 13)):
        g = torch.Generator().manual_seed(100 * M + K)
        x, w = one_hot_rows(M, K, g), full_mantissa((N, K), g)
        k = x.abs().argmax(1)
        xv = x[torch.arange(M), k]

        def prod(cx, cw):
            return (cx(xv).double()[:, None] * cw(w).double()[:, k].t()).float()

        rne = prod(lambda t: t.to(tdt), lambda t: t.to(tdt))
        trunc = prod(lambda t: truncate_mantissa(t, bits), lambda t: truncate_mantissa(t, bits))
        plain = prod(lambda t: t, lambda t: t)
        assert (rne != trunc).float().mean() > 0.5
        assert (rne != plain).float().mean() > 0.9
        # the RNE product of two <= 11-bit significands is exact in fp32
        assert torch.equal(rne.double(), xv.to(tdt).double()[:, None] * w.to(tdt).double()[:, k].t())


@pytest.mark.parametrize("seed", R.TINY_SEEDS)
def test_tiny_exact_model_bounds(seed):
    """The activations of the tiny integer model stay exact in both types for the seeds the
    GPU test uses, before and after the weight bump; the self-interaction variant in fp16."""
    for itself, dts in ((False, ("bf16", "fp16")), (True, ("fp16",))):
        ref, X, lS_o, lS_i, _ = R.tiny_exact_model(seed, itself)
        assert ref.ln_top == R.tiny_ln_top(itself) and ref.ln_top[0] == (14 if itself else 10)
        p0 = R.forward(ref, X, lS_o, lS_i, None)
        for dt in dts:
            ok, worst = R.linear_inputs_exact(ref, X, lS_o, lS_i, dt)
            assert ok and worst <= (1939 if itself else 179), (dt, worst)
            assert np.array_equal(R.forward(ref, X, lS_o, lS_i, dt), p0)  # rounding is a no-op
        assert R.bump_weights(ref) == 5
        for dt in dts:
            ok, worst = R.linear_inputs_exact(ref, X, lS_o, lS_i, dt)
            assert ok, (dt, worst)
        p1 = R.forward(ref, X, lS_o, lS_i, None)
        assert not np.array_equal(p0, p1)
        assert len(np.unique(p0)) >= 4  # not a saturated, constant output
