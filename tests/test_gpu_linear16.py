"""dlrm_linear16_forward (the 16-bit MFMA inference Linear) against exact references.

Y = act(r16(X) r16(W)^T + bias) with r16 = round-to-nearest-even to bf16 / fp16 and fp32
accumulation.  Integer operands and one-hot operands make the result independent of the
summation order, so tests 1, 2 and 4 compare bitwise; only test 3 (random operands) has a
bound, the fp32-accumulation bound of exact_inputs.gemm_close.  Operands sit in NaN-padded
buffers (a pad element that reaches a sum - multiplied by zero instead of masked - poisons
it), outputs in sentinel-padded buffers with guard rows."""
import numpy as np
import pytest
import torch

from exact_inputs import (SENTINEL, exact_bound_ok, full_mantissa, gemm_close, int_matrix,
                          one_hot_rows, padded, pads_intact)

pytestmark = pytest.mark.gpu

dev = "cuda:0"
NAN = float("nan")
TILES = [0, 128128, 128064, 64064, 32064]  # DLRM_TUNE_LINEAR16_TILE values; 0 = the planner
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
SHAPES = [(1, 1, 1), (3, 1, 256), (33, 17, 13), (64, 64, 64), (130, 129, 33), (70, 36, 479),
          (16, 256, 1028), (257, 130, 96)]


@pytest.fixture(scope="module")
def ops():
    from dlrm_hip import ops as _ops
    assert tuple(TILES[1:]) == tuple(_ops.LINEAR16_TILES)
    return _ops


def _gen(seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _pad4(n):
    return (n + 3) // 4 * 4


def _offset_view(t, ld):
    """``t`` inside a NaN-filled flat buffer, starting one element in, with row stride ld:
    a base that is not 16-byte aligned."""
    r, c = t.shape
    flat = torch.full((1 + (r + 2) * ld,), NAN, device=t.device)
    view = flat[1:1 + r * ld].view(r, ld)[:, :c]
    view.copy_(t)
    return view


class IntCase:
    """Integer operands of one shape in both layouts, built once and only read."""

    def __init__(self, M, N, K):
        g = _gen(17 * M + 5 * N + K)
        self.M, self.N, self.K = M, N, K
        self.x = int_matrix((M, K), -4, 4, g)
        self.w = int_matrix((N, K), -4, 4, g)
        self.b = int_matrix((N,), -8, 8, g, nonzero=False)
        ld = _pad4(K + 1)
        # aligned: ld = pad4(K + 1), column K of W's buffer holds the bias (the trainer's
        # layout), the rest of the pads NaN
        self.xa = padded(self.x, 2, ld - K, NAN)
        self.wa = padded(self.w, 2, ld - K, NAN)
        self.wa._base[:N, K] = self.b
        # guarded: a contiguous [N, K] W, or (for the strided bias) W in an odd-stride buffer
        # with the bias in column K; X one element into its buffer
        ldg = K + 1 if (K + 1) % 4 else K + 3
        self.xg = _offset_view(self.x, K + 1)
        self.wg = self.w.clone()
        self.wgs = padded(self.w, 2, ldg - K, NAN)
        self.wgs._base[:N, K] = self.b
        self.bc = torch.full((N + 4,), NAN, device=dev)
        self.bc[:N] = self.b
        self.acc = self.x.double() @ self.w.double().t()
        self.exact = exact_bound_ok(self.x.abs(), self.w.abs().t(), extra=8)

    def operands(self, path, bias):
        """(x, W, bias tensor) of a load path and a bias kind."""
        if path == "aligned":
            x, W, buf = self.xa, self.wa, self.wa._base
        else:
            x, W, buf = self.xg, (self.wgs if bias == "strided" else self.wg), self.wgs._base
        b = {"none": None, "contiguous": self.bc[:self.N], "strided": buf[:self.N, self.K]}[bias]
        return x, W, b

    def reference(self, bias, relu):
        ref = self.acc + (self.b.double() if bias != "none" else 0.0)
        return (torch.relu(ref) if relu else ref).float()


_CASES = {}


def _case(shape):
    if shape not in _CASES:
        _CASES[shape] = IntCase(*shape)
    return _CASES[shape]


def test_alignment_of_the_two_layouts():
    """The layouts above really select the two load paths' conditions."""
    c = _case((70, 36, 479))
    x, W, _ = c.operands("aligned", "strided")
    assert x.data_ptr() % 16 == 0 and W.data_ptr() % 16 == 0
    assert x.stride(0) == W.stride(0) == _pad4(479 + 1)
    x, W, _ = c.operands("guarded", "none")
    assert x.data_ptr() % 16 != 0 and W.stride(0) == 479 and W.is_contiguous()
    assert c.operands("guarded", "strided")[1].stride(0) % 4 != 0


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_integer_exact(ops, dt, tile):
    """1. Integer operands (exact in both 16-bit types): bitwise the fp64 reference, for
    every shape, epilogue, bias kind and load path; nothing outside Y[0:M][0:N] is written."""
    for shape in SHAPES:
        c = _case(shape)
        assert c.exact
        for t in (c.x, c.w):
            assert torch.equal(t.to(DTYPES[dt]).float(), t)
        for path in ("aligned", "guarded"):
            for bias in ("none", "contiguous", "strided"):
                x, W, b = c.operands(path, bias)
                for relu in (0, 1):
                    Y = padded(torch.zeros(c.M, c.N, device=dev), 2, 4, SENTINEL)
                    with ops.tuning(linear16_tile=tile):
                        ops.linear16_forward(x, W, b, relu=bool(relu), out=Y, dtype=dt)
                    what = (shape, path, bias, relu)
                    assert torch.equal(Y, c.reference(bias, relu)), what
                    assert pads_intact(Y), what


def rounding_expected(x, w, torch_dt):
    """x [M, K] one-hot rows, w [N, K] dense: out[m][n] = fl32(r16(x[m][k_m]) r16(w[n][k_m]))
    (a product of two <= 11-bit mantissas is exact in fp32, the other terms are zeros)."""
    k = x.abs().argmax(1)
    xv = x.to(torch_dt).double()[torch.arange(x.shape[0], device=x.device), k]
    return (xv[:, None] * w.to(torch_dt).double()[:, k].t()).float()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_rounding_mode(ops, dt, tile):
    """2. One-hot rows against a dense full-mantissa operand: every output is ONE product of
    the two RNE-rounded operands; truncation or an unrounded operand changes it
    (test_linear16_cpu proves that on these inputs)."""
    for (M, N, K) in ((33, 40, 96), (5, 3, 13)):
        g = _gen(100 * M + K)
        x1, wd = one_hot_rows(M, K, g), full_mantissa((N, K), g)
        xd, w1 = full_mantissa((M, K), g), one_hot_rows(N, K, g)
        with ops.tuning(linear16_tile=tile):
            Y = ops.linear16_forward(padded(x1, 2, 4, NAN), padded(wd, 2, 4, NAN), dtype=dt)
            Yt = ops.linear16_forward(xd, w1, dtype=dt)
        assert torch.equal(Y, rounding_expected(x1, wd, DTYPES[dt])), (M, N, K)
        assert torch.equal(Yt, rounding_expected(w1, xd, DTYPES[dt]).t()), (M, N, K)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_random_operands(ops, dt, tile):
    """3. Random operands vs fp64 of the ROUNDED operands: the 16-bit products are exact in
    fp32, what remains is an fp32 accumulation of K terms (gemm_close's bound)."""
    M, N, K = 256, 512, 479
    g = _gen(3)
    x = torch.randn(M, K, generator=g, device=dev)
    w = torch.randn(N, K, generator=g, device=dev) * 0.05
    b = torch.randn(N, generator=g, device=dev)
    with ops.tuning(linear16_tile=tile):
        Y = ops.linear16_forward(x, w, b, dtype=dt)
    xr, wr = x.to(DTYPES[dt]).double(), w.to(DTYPES[dt]).double()
    ref = xr @ wr.t() + b.double()
    absprod = xr.abs() @ wr.abs().t() + b.double().abs()
    ok, worst = gemm_close(Y.cpu().numpy(), ref.cpu().numpy(), absprod.cpu().numpy(), K)
    print(f"linear16 {dt} tile {tile}: worst |err| / tol = {worst:.4f}")
    assert ok, worst


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_isolation_and_determinism(ops, dt, tile):
    """4. One NaN in X[m0][k0 < K] makes row m0 of Y NaN and changes no other row bitwise
    (with and without ReLU); two identical calls give identical bits."""
    M, N, K = 130, 129, 96
    g = _gen(4)
    x = torch.randn(M, K, generator=g, device=dev)
    w = torch.randn(N, K, generator=g, device=dev)
    b = torch.randn(N, generator=g, device=dev)
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    for relu in (False, True):
        with ops.tuning(linear16_tile=tile):
            Y0 = ops.linear16_forward(x, w, b, relu=relu, dtype=dt)
            Y1 = ops.linear16_forward(x, w, b, relu=relu, dtype=dt)
            xn = x.clone()
            xn[77, 41] = NAN
            Yn = ops.linear16_forward(xn, w, b, relu=relu, dtype=dt)
        assert torch.equal(bits(Y0), bits(Y1))
        assert bool(torch.isnan(Yn[77]).all())
        keep = torch.arange(M, device=dev) != 77
        assert torch.equal(bits(Yn[keep]), bits(Y0[keep]))
        assert not bool(torch.isnan(Y0).any())


def test_inf_and_fp16_overflow(ops):
    """Inf propagates; an fp16 operand above 65504 rounds to Inf (documented), bf16 keeps it."""
    x = torch.tensor([[1.0, 2.0], [float("inf"), 1.0], [1.0e5, 1.0]], device=dev)
    w = torch.tensor([[1.0, 1.0]], device=dev)
    yb = ops.linear16_forward(x, w, dtype="bf16").cpu().numpy().ravel()
    yh = ops.linear16_forward(x, w, dtype="fp16").cpu().numpy().ravel()
    assert yb[0] == yh[0] == 3.0 and np.isinf(yb[1]) and np.isinf(yh[1])
    assert np.isinf(yh[2]) and yb[2] == float(torch.tensor(1.0e5).bfloat16().float()) + 1.0


def test_bad_arguments(ops):
    x = torch.zeros(4, 8, device=dev)
    with pytest.raises(ValueError):
        ops.linear16_forward(x, torch.zeros(3, 8, device=dev), dtype="int8")
    with pytest.raises(ValueError):
        ops.linear16_forward(x, torch.zeros(3, 7, device=dev))
    with pytest.raises(ValueError):
        ops.linear16_forward(x, torch.zeros(3, 8, device=dev), out=torch.zeros(4, 4, device=dev))
    assert ops.linear16_forward(x[:0], torch.zeros(3, 8, device=dev)).shape == (0, 3)
