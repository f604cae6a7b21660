"""dlrm_linear8_pack / dlrm_linear8_range / dlrm_linear8_forward on the GPU, bitwise against
the rule of tests/exact_mlp8 (which tests/test_exact_mlp8_cpu.py proves to be torch's
quantize_dynamic on the CPU): the packer, the forward over every input class, option and
tile, a three-layer stack chained on the device, and a captured graph that must follow the
range of new inputs."""
import numpy as np
import pytest
import torch

import exact_mlp8 as E

pytestmark = pytest.mark.gpu
dev = "cuda:0"
F32 = np.float32

PACK_SHAPES = [(1, 1), (7, 13), (16, 64), (9, 65), (33, 479), (64, 1024)]
FWD_SHAPES = [(1, 1, 1), (5, 7, 13), (33, 1, 65), (16, 16, 64), (257, 9, 479), (64, 40, 1024),
              (8, 4, 2048)]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _check_pack(packed, W, what):
    wq, s_w = E.pack(W)
    N, K = W.shape
    got = packed.wq.cpu().numpy()
    assert got.shape[1] % 64 == 0 and got.shape[1] >= max(K, 64), what
    assert np.array_equal(got[:, :K], wq), what
    assert not got[:, K:].any(), what
    assert _bits(packed.s_w.cpu().numpy())[0] == _bits(np.array([s_w]))[0], what


@pytest.mark.parametrize("N,K", PACK_SHAPES)
def test_pack(N, K):
    from dlrm_hip import ops
    gen = np.random.default_rng(100 * N + K)
    W = (gen.standard_normal((N, K)) * 0.3).astype(F32)
    _check_pack(ops.linear8_pack(_t(W)), W, "contiguous")
    # the engine's [N, Kp] layer: column K holds a large bias that must not move s_w
    Kp = (K + 1 + 3) // 4 * 4
    buf = np.zeros((N, Kp), F32)
    buf[:, :K] = W
    buf[:, K] = 1e6
    view = _t(buf)[:, :K]
    packed = ops.linear8_pack(view)
    _check_pack(packed, W, "view")
    # re-pack into the same storage
    W2 = (W * 3 + 0.01).astype(F32)
    ptr = packed.wq.data_ptr()
    again = ops.linear8_pack(_t(W2), out=packed)
    assert again is packed and packed.wq.data_ptr() == ptr
    _check_pack(packed, W2, "re-pack")
    Z = np.zeros((N, K), F32)
    pz = ops.linear8_pack(_t(Z))
    _check_pack(pz, Z, "zero")
    assert float(pz.s_w.item()) == float(E.FLT_EPSILON)


def _device_inputs(x, wide, aligned):
    """x as a view of a wider buffer whose columns >= K hold NaN and a constant 1."""
    M, K = x.shape
    if not wide:
        return _t(x)
    ld = (K + 2 + 3) // 4 * 4 if aligned else (K + 3) | 1  # odd: rows off the 16-byte grid
    buf = np.full((M, ld), np.nan, F32)
    buf[:, :K] = x
    buf[:, K] = 1.0
    return _t(buf)[:, :K]


def _run_case(ops, x, W, b, relu, bias_mode, wide, aligned, what):
    M, K = x.shape
    N = W.shape[0]
    info = {}
    bias = None if bias_mode == "none" else b
    want = E.layer(x, W, bias, relu, want=info)
    assert info["d"].min() >= -127 and info["d"].max() <= 127, what
    packed = ops.linear8_pack(_t(W))
    xd = _device_inputs(x, wide, aligned)
    if bias_mode == "none":
        bd = None
    elif bias_mode == "contiguous":
        bd = _t(b)
    else:
        bd = _t(np.stack([b, np.full_like(b, 55.0), np.full_like(b, -9.0)], axis=1))[:, 0]
        assert N == 1 or bd.stride(0) == 3
    ybuf = torch.full((M + 2, N + 3), 777.0, device=dev)
    y = ybuf[1:M + 1, 1:N + 1]
    qp = torch.zeros(2, device=dev)
    got = ops.linear8_forward(xd, packed, bias=bd, relu=relu, out=y, qparams=qp)
    assert got is y
    full = ybuf.cpu().numpy()
    inner = full[1:M + 1, 1:N + 1]
    bad = np.flatnonzero(_bits(inner) != _bits(want))
    assert bad.size == 0, (what, bad.size, inner.ravel()[bad[:4]], want.ravel()[bad[:4]])
    full[1:M + 1, 1:N + 1] = 777.0
    assert (full == 777.0).all(), what  # the surroundings survive
    s_x, zp = qp.cpu().numpy()
    assert _bits(np.array([s_x]))[0] == _bits(np.array([info["s_x"]]))[0] and zp == info["zp"], \
        (what, s_x, zp, info["s_x"], info["zp"])


@pytest.mark.parametrize("M,N,K", FWD_SHAPES)
def test_forward_classes_and_options(M, N, K):
    from dlrm_hip import ops
    gen = np.random.default_rng(M * 7 + N * 3 + K)
    modes = ("none", "contiguous", "strided")
    for i, cls in enumerate(E.CLASSES):
        x = E.make_input(cls, M, K, gen)
        W, b = E.make_weights(cls, N, K, gen)
        _run_case(ops, x, W, b, relu=bool(i % 2), bias_mode=modes[i % 3], wide=i % 4 != 3,
                  aligned=bool((i // 2) % 2), what=(cls, M, N, K))
    # every option on the mixed-sign class
    x = E.make_input("randn", M, K, gen)
    W, b = E.make_weights("randn", N, K, gen)
    for relu in (False, True):
        for mode in modes:
            for wide, aligned in ((False, True), (True, True), (True, False)):
                _run_case(ops, x, W, b, relu, mode, wide, aligned,
                          ("randn", relu, mode, wide, aligned))


@pytest.mark.parametrize("M,N,K", FWD_SHAPES + [(300, 150, 130)])
def test_every_tile(M, N, K):
    from dlrm_hip import ops
    gen = np.random.default_rng(M + N + K)
    x = E.make_input("randn", M, K, gen)
    W, b = E.make_weights("randn", N, K, gen)
    for tile in ops.LINEAR8_TILES:
        with ops.tuning(linear8_tile=tile):
            _run_case(ops, x, W, b, True, "contiguous", True, True, ("tile", tile))
    with ops.tuning(linear8_tile=64032):
        with pytest.raises(Exception):
            ops.linear8_forward(_t(x), ops.linear8_pack(_t(W)))


def test_large_accumulator_rounds():
    """|acc| > 2^24 at K = 2048: float(acc) rounds to nearest even before the scale."""
    from dlrm_hip import ops
    x = np.ones((4, 2048), F32)
    x[:, ::7] = 0.0
    x[1, ::3] = 0.5
    W = np.full((3, 2048), 2.0, F32)
    W[1, ::11] = -2.0
    W[2, ::5] = 0.75
    info = {}
    want = E.layer(x, W, None, want=info)
    acc = info["d"].astype(np.int64) @ E.pack(W)[0].astype(np.int64).T
    assert np.abs(acc).max() > 2 ** 24
    got = ops.linear8_forward(_t(x), ops.linear8_pack(_t(W))).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))


def test_refusals():
    from dlrm_hip import _lib, ops
    packed = ops.linear8_pack(torch.zeros(4, 8, device=dev))
    x = torch.zeros(3, 8, device=dev)
    with pytest.raises(ValueError):
        ops.linear8_forward(x.double(), packed)
    with pytest.raises(ValueError):
        ops.linear8_forward(x, packed, out=torch.zeros(3, 4, device=dev).t().contiguous().t())
    with pytest.raises(ValueError):
        ops.linear8_forward(x.cpu(), packed)
    rng = ops.linear8_range(x)
    with pytest.raises(_lib.DLRMHipError) as e:  # K past the int32 accumulator's safe range
        _lib.call("dlrm_linear8_forward", 1, 1, 131073, ops._p(x), 131073, ops._p(rng),
                  ops._p(packed.wq), 131136, ops._p(packed.s_w), None, 0, 0, ops._p(x), 1, None,
                  None)
    assert e.value.code == 3


def _stack_layers(gen):
    dims = [13, 64, 33, 1]
    Ws = [(gen.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(F32)
          for i in range(3)]
    bs = [gen.standard_normal(dims[i + 1]).astype(F32) for i in range(3)]
    return dims, [(Ws[i], bs[i], i < 2) for i in range(3)]


def test_stack_and_capture():
    from dlrm_hip import ops
    gen = np.random.default_rng(11)
    dims, layers = _stack_layers(gen)
    M = 257
    x = np.log1p(gen.random((M, 13))).astype(F32)
    packed = [ops.linear8_pack(_t(W)) for W, _, _ in layers]
    biases = [_t(b) for _, b, _ in layers]
    xd = _t(x)
    acts = [torch.zeros(M, n, device=dev) for n in dims[1:]]
    rngs = [torch.zeros(ops.LINEAR8_RANGE_FLOATS, device=dev) for _ in layers]

    def run():
        h = xd
        for i, (_, _, relu) in enumerate(layers):
            ops.linear8_range(h, out=rngs[i])
            ops.linear8_forward(h, packed[i], bias=biases[i], relu=relu, out=acts[i],
                                rng=rngs[i])
            h = acts[i]
        return h

    want = E.stack(x, layers)
    assert np.array_equal(_bits(run().cpu().numpy()), _bits(want))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    acts[-1].zero_()
    g.replay()
    assert np.array_equal(_bits(acts[-1].cpu().numpy()), _bits(want))
    # ten times the input: the replay must derive the new range, not replay stale qparams
    x10 = (x * F32(10)).astype(F32)
    xd.copy_(_t(x10))
    g.replay()
    want10 = E.stack(x10, layers)
    assert not np.array_equal(_bits(want10), _bits(want))
    assert np.array_equal(_bits(acts[-1].cpu().numpy()), _bits(want10))
