"""The int8 dynamic-quantized Linear's rule on the host (no GPU): tests/exact_mlp8 is bitwise
torch.quantization.quantize_dynamic(..., {nn.Linear}, torch.qint8) on the fbgemm engine, its
(scale, zero point) are torch._choose_qparams_per_tensor's, the MFMA operand d = xq - zp
stays inside [-127, 127] on every input class, and the host wiring of the v18 entry points."""
import os
import re

import numpy as np
import pytest
import torch

import exact_mlp8 as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
RANDN_SHAPES = [(257, 9, 479), (128, 1024, 1024), (257, 9, 13)]


def _fbgemm():
    if "fbgemm" not in torch.backends.quantized.supported_engines:
        pytest.skip("torch has no fbgemm quantized engine")
    torch.backends.quantized.engine = "fbgemm"


def input_classes(gen):
    """(name, x [M, K], (N, K)) over the issue's table."""
    out = []
    for M, N, K in RANDN_SHAPES:
        x = gen.standard_normal((M, K)).astype(F32)
        out.append((f"randn{M}x{K}", x, N))
        out.append((f"relu{M}x{K}", np.maximum(x, 0), N))
    out.append(("zero", np.zeros((5, 13), F32), 7))
    out.append(("tiny_pos", (gen.random((9, 65)) * 1e-4).astype(F32), 3))
    out.append(("tiny_mixed", ((gen.random((9, 65)) - 0.3) * 1e-4).astype(F32), 3))
    out.append(("tiny_neg", (-gen.random((9, 65)) * 1e-4).astype(F32), 3))
    out.append(("all_neg", (-1 - gen.random((33, 65))).astype(F32), 1))
    out.append(("huge", (gen.standard_normal((17, 64)) * 1e30).astype(F32), 5))
    out.append(("subnormal", (gen.standard_normal((17, 64)) * 1e-41).astype(F32), 5))
    out.append(("pm1_k7", (gen.integers(0, 2, (16, 7)) * 2 - 1).astype(F32), 4))
    out.append(("pm1_k2048", (gen.integers(0, 2, (8, 2048)) * 2 - 1).astype(F32), 4))
    # half-integers on an asymmetric range whose scale is exactly 0.5: x / scale + zp ties
    h = (gen.integers(-20, 108, (31, 40)) * 0.25).astype(F32)
    h[0, 0], h[0, 1] = -5.0, 26.75
    h = np.clip(h, -5.0, 26.75)
    out.append(("half_integers", h, 6))
    s = (gen.integers(0, 2, (8, 2048)) * 2 - 1).astype(F32) * 3.0
    out.append(("saturating_k2048", s, 4))
    out.append(("single", np.array([[0.37]], F32), 1))
    return out


def _weights(name, N, K, gen):
    if name.startswith("saturating"):
        return (np.sign(gen.standard_normal((N, K))) * 2.0).astype(F32), None
    if name.startswith("pm1") or name == "half_integers":
        return gen.integers(-3, 4, (N, K)).astype(F32), gen.integers(-2, 3, N).astype(F32)
    return (gen.standard_normal((N, K)) / np.sqrt(K)).astype(F32), \
        gen.standard_normal(N).astype(F32)


def _torch_linear(W, b):
    lin = torch.nn.Linear(W.shape[1], W.shape[0], bias=b is not None)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(W))
        if b is not None:
            lin.bias.copy_(torch.from_numpy(b))
    return lin


def _quantized(lin):
    """The dynamically quantized module of one Linear (quantize_dynamic swaps children only)."""
    q = torch.quantization.quantize_dynamic(torch.nn.Sequential(lin), {torch.nn.Linear},
                                            torch.qint8)[0]
    assert "quantized.dynamic" in type(q).__module__, type(q)
    return q


def _run(q, x):
    with torch.no_grad():
        return q(torch.from_numpy(x)).numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def test_rule_is_quantize_dynamic_bitwise():
    _fbgemm()
    gen = np.random.default_rng(8)
    seen128 = False
    for name, x, N in input_classes(gen):
        K = x.shape[1]
        W, b = _weights(name, N, K, gen)
        q = _quantized(_torch_linear(W, b))
        want = _run(q, x)
        info = {}
        got = E.layer(x, W, b, want=info)
        # the packed weights are torch's
        wq, s_w = E.pack(W)
        tw = q.weight()
        assert np.array_equal(tw.int_repr().numpy(), wq), name
        assert F32(tw.q_scale()) == s_w and tw.q_zero_point() == 0, name
        # the activation parameters are torch's
        ts, tz = torch._choose_qparams_per_tensor(torch.from_numpy(x), True)
        assert F32(ts) == info["s_x"] and int(tz) == info["zp"], (name, ts, tz, info["s_x"],
                                                                  info["zp"])
        d = info["d"]
        assert d.min() >= -127 and d.max() <= 127, (name, d.min(), d.max())
        seen128 = seen128 or bool((d + info["zp"] == 128).any())
        bad = np.flatnonzero(_bits(got + F32(0)) != _bits(want + F32(0)))  # -0 == +0
        assert bad.size == 0, (name, bad.size, got.ravel()[bad[:3]], want.ravel()[bad[:3]])
    assert seen128, "no input produced the code 128 (the clamp is at 255, not 127)"


def test_accumulator_rounds_above_2_24():
    """K = 2048 of |d| = 127 and |wq| = 127 reaches |acc| > 2^24: float(acc) rounds."""
    x = np.ones((4, 2048), F32)
    x[:, ::7] = 0.0  # one-sided: d is 0 or 127
    x[1, ::3] = 0.5
    W = np.full((3, 2048), 2.0, F32)
    W[1, ::11] = -2.0
    W[2, ::5] = 0.75
    info = {}
    E.layer(x, W, None, want=info)
    wq, _ = E.pack(W)
    acc = info["d"].astype(np.int64) @ wq.astype(np.int64).T
    assert np.abs(acc).max() > 2 ** 24
    _fbgemm()
    q = _quantized(_torch_linear(W, None))
    assert np.array_equal(_bits(E.layer(x, W)), _bits(_run(q, x)))


def test_stack_is_quantize_dynamic_bitwise():
    _fbgemm()
    gen = np.random.default_rng(11)
    dims = [13, 64, 33, 1]
    Ws = [(gen.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(F32)
          for i in range(3)]
    bs = [gen.standard_normal(dims[i + 1]).astype(F32) for i in range(3)]
    mods = []
    for i in range(3):
        mods.append(_torch_linear(Ws[i], bs[i]))
        if i < 2:
            mods.append(torch.nn.ReLU())
    q = torch.quantization.quantize_dynamic(torch.nn.Sequential(*mods), {torch.nn.Linear},
                                            torch.qint8)
    x = np.log1p(gen.random((257, 13))).astype(F32)
    want = _run(q, x)
    got = E.stack(x, [(Ws[0], bs[0], True), (Ws[1], bs[1], True), (Ws[2], bs[2], False)])
    assert np.array_equal(_bits(got + F32(0)), _bits(want + F32(0)))


def test_qparams_random_ranges():
    """(scale, zp) against torch._choose_qparams_per_tensor over many two-value tensors,
    tiny and stretched ranges included."""
    gen = np.random.default_rng(5)
    for _ in range(4000):
        e = gen.uniform(-12, 3, 2)
        a = F32(-(10.0 ** e[0]) * gen.integers(0, 2))
        b = F32((10.0 ** e[1]) * gen.integers(0, 2))
        x = np.array([a, b, gen.uniform(a, b)], F32)
        s_x, _inv, zp = E.qparams(x)
        ts, tz = torch._choose_qparams_per_tensor(torch.from_numpy(x), True)
        assert F32(ts) == s_x and int(tz) == zp, (x, ts, tz, s_x, zp)


# ------------------------------------------------------------------- host wiring --
def test_abi_is_18_everywhere():
    from dlrm_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()
    ver = int(re.search(r"#define\s+DLRM_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert ver >= 18 and _lib.ABI_VERSION == ver
    assert int(_lib.load().dlrm_abi_version()) == ver


def _header_args(hdr, name):
    m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [a.strip() for a in body.split(",") if a.strip()]


def test_signature_table_matches_header():
    import ctypes
    from dlrm_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()
    for name in ("dlrm_linear8_pack_workspace_size", "dlrm_linear8_pack", "dlrm_linear8_range",
                 "dlrm_linear8_forward"):
        args = _header_args(hdr, name)
        res, sig = _lib.SIGNATURES[name]
        assert len(sig) == len(args), (name, args)
        for a, c in zip(args, sig):
            if "*" in a or a.startswith("dlrm_stream_t"):
                assert c is ctypes.c_void_p, (name, a)
            elif a.startswith("int64_t"):
                assert c is ctypes.c_int64, (name, a)
            elif a.startswith("int32_t"):
                assert c is ctypes.c_int32, (name, a)
            else:
                assert a.startswith("size_t") and c is ctypes.c_size_t, (name, a)
        assert res is (ctypes.c_size_t if name.endswith("_size") else ctypes.c_int32)
        assert hasattr(_lib.load(), name)


def test_ops_argument_errors():
    """The checks that need no device."""
    from dlrm_hip import ops
    W = torch.zeros(4, 8)
    with pytest.raises(ValueError):
        ops.linear8_pack(W)  # a CPU tensor
    with pytest.raises(ValueError):
        ops.linear8_pack(W.double())
    with pytest.raises(ValueError):
        ops.linear8_pack(torch.zeros(8))
    with pytest.raises(ValueError):
        ops.linear8_pack(torch.zeros(4, 8).t())  # rows not contiguous
    with pytest.raises(ValueError):
        ops.linear8_range(torch.zeros(4, 8, dtype=torch.float16))
    with pytest.raises(ValueError):
        ops.linear8_range(torch.zeros(4, 8))  # a CPU tensor
    packed = ops.Linear8Weights(torch.zeros(4, 64, dtype=torch.int8), torch.ones(1), 4, 8)
    with pytest.raises(ValueError):
        ops.linear8_forward(torch.zeros(3, 9), packed)  # K mismatch
    with pytest.raises(ValueError):
        ops.linear8_forward(torch.zeros(3, 8), packed, bias=torch.zeros(5))
    with pytest.raises(ValueError):
        ops.linear8_forward(torch.zeros(3, 8), packed, out=torch.zeros(3, 5))
    with pytest.raises(ValueError):
        ops.linear8_forward(torch.zeros(3, 8), packed, rng=torch.zeros(7))
    with pytest.raises(ValueError):
        ops.Linear8Weights(torch.zeros(4, 60, dtype=torch.int8), torch.ones(1), 4, 8)
    with pytest.raises(ValueError):
        ops.Linear8Weights(torch.zeros(4, 64, dtype=torch.uint8), torch.ones(1), 4, 8)
