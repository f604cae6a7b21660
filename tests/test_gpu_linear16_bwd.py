"""dlrm_linear16_dgrad / dlrm_linear16_wgrad (the 16-bit MFMA Linear's backward) against exact
references, in the pattern of test_gpu_linear16.py.

  dgrad  dX = mask > 0 ? r16(dY) r16(W) : 0          reduction over N, W's ROW index
  wgrad  C  = r16(dY)^T r16(X)  or  C - fl(lr * ..)   reduction over M, both operands' ROW index

Integer and one-hot operands make the result independent of the summation order (and of the
wgrad's batch split), so tests 1, 2 and 4 compare bitwise; only test 3 has a bound, the
fp32-accumulation bound of exact_inputs.gemm_close with the reduction depth.  Operands sit in
NaN-padded buffers, outputs in sentinel-padded buffers with guard rows."""
import numpy as np
import pytest
import torch

from exact_inputs import (SENTINEL, exact_bound_ok, full_mantissa, gemm_close, int_matrix,
                          one_hot_rows, padded, pads_intact, truncate_mantissa)

pytestmark = pytest.mark.gpu

dev = "cuda:0"
NAN = float("nan")
TILES = [0, 128128, 128064, 64064, 32064]  # 0 = the planner
SPLITS = [0, 1, 3]                         # DLRM_TUNE_LINEAR16_WGRAD_SPLIT; 0 = the planner
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
MANT = {"bf16": 7, "fp16": 10}
# (M, N, K): each dimension takes a 1, a value that is no multiple of 4, and one that spans
# more than one 64-step and more than one tile with a tail
SHAPES = [(1, 1, 1), (3, 1, 256), (256, 3, 1), (33, 17, 13), (13, 33, 17), (64, 64, 64),
          (130, 129, 33), (33, 130, 129), (70, 36, 480), (257, 130, 96), (96, 257, 130)]
LR = 0.25


@pytest.fixture(scope="module")
def ops():
    from dlrm_hip import ops as _ops
    assert tuple(TILES[1:]) == tuple(_ops.LINEAR16_DGRAD_TILES) == tuple(_ops.LINEAR16_WGRAD_TILES)
    return _ops


def _gen(seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _pad4(n):
    return (n + 3) // 4 * 4


def _aligned(t):
    """``t`` in a NaN-padded buffer whose row stride is a multiple of 4 (16-byte loads)."""
    return padded(t, 2, _pad4(t.shape[1] + 1) - t.shape[1], NAN)


def _guarded(t):
    """``t`` one element into a NaN-filled flat buffer with an odd row stride: neither the
    base nor the stride allows 16-byte loads."""
    r, c = t.shape
    ld = c + 1 if (c + 1) % 2 else c + 2
    flat = torch.full((1 + (r + 2) * ld,), NAN, device=t.device)
    view = flat[1:1 + r * ld].view(r, ld)[:, :c]
    view.copy_(t)
    return view


def _bits(t):
    return t.contiguous().view(torch.int32)


class IntCase:
    """Integer operands of one shape in both layouts, built once and only read."""

    def __init__(self, M, N, K):
        g = _gen(17 * M + 5 * N + K)
        self.M, self.N, self.K = M, N, K
        self.dy = int_matrix((M, N), -4, 4, g)
        self.w = int_matrix((N, K), -4, 4, g)
        self.x = int_matrix((M, K), -4, 4, g)
        self.c0 = int_matrix((N, K), -8, 8, g, nonzero=False)
        # the mask: positives, negatives, both zeros and one NaN
        mask = int_matrix((M, K), -2, 2, g, nonzero=False)
        flat = mask.view(-1)
        flat[::5] = 0.0
        flat[1::7] = -0.0
        flat[flat.numel() // 2] = NAN
        self.mask = mask
        self.layouts = {
            "aligned": {k: _aligned(getattr(self, k)) for k in ("dy", "w", "x", "mask")},
            "guarded": {k: _guarded(getattr(self, k)) for k in ("dy", "w", "x", "mask")},
        }
        self.dx = (self.dy.double() @ self.w.double()).float()
        self.dx_masked = torch.where(self.mask > 0, self.dx, torch.zeros_like(self.dx))
        self.gw = (self.dy.double().t() @ self.x.double()).float()
        self.sgd = (self.c0.double() - LR * self.gw.double()).float()
        self.exact = exact_bound_ok(self.dy.abs(), self.w.abs()) and \
            exact_bound_ok(self.dy.abs().t(), self.x.abs(), extra=8)


_CASES = {}


def _case(shape):
    if shape not in _CASES:
        _CASES[shape] = IntCase(*shape)
    return _CASES[shape]


def test_alignment_of_the_two_layouts():
    c = _case((70, 36, 480))
    for k, t in c.layouts["aligned"].items():
        assert t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 and t.stride(0) > t.shape[1], k
    for k, t in c.layouts["guarded"].items():
        assert t.data_ptr() % 16 != 0 and t.stride(0) % 2 == 1, k
    m = c.mask
    assert bool((m > 0).any()) and bool((m < 0).any()) and bool(torch.isnan(m).any())
    z = _bits(m)[m == 0]
    assert bool((z == 0).any()) and bool((z != 0).any())  # +0.0 and -0.0


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_dgrad_integer_exact(ops, dt, tile):
    """1. Integer operands: bitwise the fp64 reference for every shape, load path and mask;
    nothing outside dX[0:M][0:K] is written."""
    for shape in SHAPES:
        c = _case(shape)
        assert c.exact
        for t in (c.dy, c.w):
            assert torch.equal(t.to(DTYPES[dt]).float(), t)
        for path, lay in c.layouts.items():
            for masked in (False, True):
                out = padded(torch.zeros(c.M, c.K, device=dev), 2, 3, SENTINEL)
                with ops.tuning(linear16_dgrad_tile=tile):
                    ops.linear16_dgrad(lay["dy"], lay["w"], lay["mask"] if masked else None,
                                       out=out, dtype=dt)
                what = (shape, path, masked)
                assert torch.equal(out, c.dx_masked if masked else c.dx), what
                assert pads_intact(out), what


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_wgrad_integer_exact(ops, dt, tile):
    """1. The same for the weight gradient, STORE and SGD (integer C in [-8, 8], lr = 0.25:
    every value is a small multiple of 1/4), with the planner's split and forced ones."""
    for shape in SHAPES:
        c = _case(shape)
        assert c.exact
        for path, lay in c.layouts.items():
            for split in SPLITS:
                for lr in (None, LR):
                    start = torch.zeros_like(c.c0) if lr is None else c.c0
                    out = padded(start, 2, 3, SENTINEL)
                    with ops.tuning(linear16_wgrad_tile=tile, linear16_wgrad_split=split):
                        ops.linear16_wgrad(lay["dy"], lay["x"], out, lr=lr, dtype=dt)
                    what = (shape, path, split, lr)
                    assert torch.equal(out, c.gw if lr is None else c.sgd), what
                    assert pads_intact(out), what


def _alternatives(a, b, dt):
    """Products of a truncated / an unrounded operand pair, as fp32."""
    t = (truncate_mantissa(a, MANT[dt]).double() * truncate_mantissa(b, MANT[dt]).double()).float()
    u = (a.double() * b.to(DTYPES[dt]).double()).float()
    return t, u


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_rounding_mode(ops, dt, tile):
    """2. A one-hot operand along the reduction against full-mantissa values: every output is
    ONE product r16(a) r16(b), exact in fp32; truncation or an unrounded operand differs."""
    tdt = DTYPES[dt]
    for (M, N, K) in ((33, 96, 40), (5, 13, 3), (96, 33, 70)):
        g = _gen(100 * M + K)
        # dgrad: one nonzero per row of dY
        dy, w = one_hot_rows(M, N, g), full_mantissa((N, K), g)
        n_of = dy.abs().argmax(1)
        a, b = dy[torch.arange(M, device=dev), n_of][:, None].expand(M, K), w[n_of]
        want = (a.to(tdt).double() * b.to(tdt).double()).float()
        with ops.tuning(linear16_dgrad_tile=tile):
            got = ops.linear16_dgrad(padded(dy, 2, 3, NAN), padded(w, 2, 3, NAN), dtype=dt)
        assert torch.equal(got, want), (M, N, K)
        for alt in _alternatives(a.contiguous(), b.contiguous(), dt):
            assert not torch.equal(alt, want)
        # wgrad: exactly one nonzero per column of dY
        dy, x = one_hot_rows(N, M, g).t().contiguous(), full_mantissa((M, K), g)
        m_of = dy.abs().argmax(0)
        a, b = dy[m_of, torch.arange(N, device=dev)][:, None].expand(N, K), x[m_of]
        want = (a.to(tdt).double() * b.to(tdt).double()).float()
        for split in (0, 2):
            out = torch.empty(N, K, device=dev)
            with ops.tuning(linear16_wgrad_tile=tile, linear16_wgrad_split=split):
                ops.linear16_wgrad(padded(dy, 2, 3, NAN), padded(x, 2, 3, NAN), out, dtype=dt)
            assert torch.equal(out, want), (M, N, K, split)
        for alt in _alternatives(a.contiguous(), b.contiguous(), dt):
            assert not torch.equal(alt, want)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_random_operands(ops, dt, tile):
    """3. Random operands vs fp64 of the ROUNDED operands: the 16-bit products are exact in
    fp32, what remains is an fp32 accumulation over the reduction depth (gemm_close)."""
    M, N, K = 300, 257, 130
    g = _gen(3)
    tdt = DTYPES[dt]
    dy = torch.randn(M, N, generator=g, device=dev) * 0.1
    w = torch.randn(N, K, generator=g, device=dev) * 0.05
    x = torch.randn(M, K, generator=g, device=dev)
    c0 = torch.randn(N, K, generator=g, device=dev)
    dyr, wr, xr = dy.to(tdt).double(), w.to(tdt).double(), x.to(tdt).double()
    with ops.tuning(linear16_dgrad_tile=tile):
        dx = ops.linear16_dgrad(dy, w, dtype=dt)
    ok, worst = gemm_close(dx.cpu().numpy(), (dyr @ wr).cpu().numpy(),
                           (dyr.abs() @ wr.abs()).cpu().numpy(), N)
    print(f"linear16_dgrad {dt} tile {tile}: worst |err| / tol = {worst:.4f}")
    assert ok, worst
    for lr in (None, 0.3):
        C = torch.empty(N, K, device=dev) if lr is None else c0.clone()
        with ops.tuning(linear16_wgrad_tile=tile):
            ops.linear16_wgrad(dy, x, C, lr=lr, dtype=dt)
        acc, absacc = dyr.t() @ xr, dyr.abs().t() @ xr.abs()
        if lr is None:
            ref, absprod = acc, absacc
        else:  # lr * acc and the subtraction each round once more: inside 1e-5 max(1, |ref|)
            ref, absprod = c0.double() - float(np.float32(lr)) * acc, \
                c0.double().abs() + lr * absacc
        ok, worst = gemm_close(C.cpu().numpy(), ref.cpu().numpy(), absprod.cpu().numpy(), M)
        print(f"linear16_wgrad {dt} tile {tile} lr {lr}: worst |err| / tol = {worst:.4f}")
        assert ok, worst


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_isolation_and_determinism(ops, dt, tile):
    """4. A NaN in one row / column of an operand poisons exactly the outputs that depend on
    it (and none where the mask is <= 0); two calls give equal bits."""
    M, N, K = 130, 129, 96
    g = _gen(4)
    dy = torch.randn(M, N, generator=g, device=dev)
    w = torch.randn(N, K, generator=g, device=dev)
    x = torch.randn(M, K, generator=g, device=dev)
    c0 = torch.randn(N, K, generator=g, device=dev)
    mask = torch.randn(M, K, generator=g, device=dev)
    rows = lambda n, i: torch.arange(n, device=dev) != i  # noqa: E731
    dyn, wn, xn = dy.clone(), w.clone(), x.clone()
    dyn[77, 41], wn[100, 50], xn[77, 50] = NAN, NAN, NAN

    with ops.tuning(linear16_dgrad_tile=tile):
        for mk in (None, mask):
            d0 = ops.linear16_dgrad(dy, w, mk, dtype=dt)
            d1 = ops.linear16_dgrad(dy, w, mk, dtype=dt)
            dr = ops.linear16_dgrad(dyn, w, mk, dtype=dt)
            dc = ops.linear16_dgrad(dy, wn, mk, dtype=dt)
            assert torch.equal(_bits(d0), _bits(d1)) and not bool(torch.isnan(d0).any())
            live = torch.ones_like(d0, dtype=torch.bool) if mk is None else mk > 0
            assert torch.equal(torch.isnan(dr[77]), live[77])
            assert torch.equal(torch.isnan(dc[:, 50]), live[:, 50])
            assert torch.equal(_bits(dr[rows(M, 77)]), _bits(d0[rows(M, 77)]))
            assert torch.equal(_bits(dc[:, rows(K, 50)]), _bits(d0[:, rows(K, 50)]))
            if mk is not None:
                assert bool((d0[~live] == 0).all()) and bool((dr[~live] == 0).all())

    for split in (0, 2):
        with ops.tuning(linear16_wgrad_tile=tile, linear16_wgrad_split=split):
            for lr in (None, 0.3):
                run = lambda a, b: ops.linear16_wgrad(a, b, c0.clone(), lr=lr, dtype=dt)  # noqa: E731
                c_0, c_1 = run(dy, x), run(dy, x)
                cr, cc = run(dyn, x), run(dy, xn)
                assert torch.equal(_bits(c_0), _bits(c_1)) and not bool(torch.isnan(c_0).any())
                assert bool(torch.isnan(cr[41]).all()) and bool(torch.isnan(cc[:, 50]).all())
                assert torch.equal(_bits(cr[rows(N, 41)]), _bits(c_0[rows(N, 41)]))
                assert torch.equal(_bits(cc[:, rows(K, 50)]), _bits(c_0[:, rows(K, 50)]))


def test_inf_and_fp16_overflow(ops):
    """5. Inf propagates; an fp16 operand above 65504 rounds to Inf, bf16 keeps it."""
    big = float(torch.tensor(1.0e5).bfloat16().float())
    dy = torch.tensor([[1.0, 2.0], [float("inf"), 1.0], [1.0e5, 1.0]], device=dev)
    w = torch.tensor([[1.0], [1.0]], device=dev)
    db = ops.linear16_dgrad(dy, w, dtype="bf16").cpu().numpy().ravel()
    dh = ops.linear16_dgrad(dy, w, dtype="fp16").cpu().numpy().ravel()
    assert db[0] == dh[0] == 3.0 and np.isinf(db[1]) and np.isinf(dh[1])
    assert np.isinf(dh[2]) and db[2] == big + 1.0
    x = torch.tensor([[1.0], [1.0], [1.0]], device=dev)
    g = torch.tensor([[1.0, 1.0, 1.0e5], [2.0, float("inf"), 1.0], [0.0, 0.0, 0.0]], device=dev)
    cb = ops.linear16_wgrad(g, x, torch.empty(3, 1, device=dev), dtype="bf16").cpu().numpy().ravel()
    ch = ops.linear16_wgrad(g, x, torch.empty(3, 1, device=dev), dtype="fp16").cpu().numpy().ravel()
    assert cb[0] == ch[0] == 3.0 and np.isinf(cb[1]) and np.isinf(ch[1])
    assert np.isinf(ch[2]) and cb[2] == big + 1.0


def test_empty_reduction(ops):
    """M == 0: STORE writes zeros, SGD leaves C alone; N == 0: dgrad writes zeros."""
    c = torch.full((3, 5), 2.0, device=dev)
    g0, x0 = torch.zeros(0, 3, device=dev), torch.zeros(0, 5, device=dev)
    assert bool((ops.linear16_wgrad(g0, x0, c.clone(), lr=0.5) == 2.0).all())
    assert bool((ops.linear16_wgrad(g0, x0, c.clone()) == 0.0).all())
    dx = ops.linear16_dgrad(torch.zeros(4, 0, device=dev), torch.zeros(0, 5, device=dev),
                            out=torch.full((4, 5), SENTINEL, device=dev))
    assert bool((dx == 0.0).all())


def test_bad_arguments(ops):
    from dlrm_hip import _lib
    g, w, x = (torch.zeros(s, device=dev) for s in ((4, 3), (3, 8), (4, 8)))
    with pytest.raises(ValueError):
        ops.linear16_dgrad(g, w, dtype="int8")
    with pytest.raises(ValueError):
        ops.linear16_dgrad(g, torch.zeros(2, 8, device=dev))
    with pytest.raises(ValueError):
        ops.linear16_dgrad(g, w, mask=torch.zeros(4, 7, device=dev))
    with pytest.raises(ValueError):
        ops.linear16_dgrad(g, w, out=torch.zeros(4, 4, device=dev))
    with pytest.raises(ValueError):
        ops.linear16_dgrad(g.t(), torch.zeros(4, 8, device=dev))  # rows not contiguous
    with pytest.raises(ValueError):
        ops.linear16_wgrad(g, x, torch.zeros(3, 8, device=dev), dtype="int8")
    with pytest.raises(ValueError):
        ops.linear16_wgrad(g, torch.zeros(5, 8, device=dev), torch.zeros(3, 8, device=dev))
    with pytest.raises(ValueError):
        ops.linear16_wgrad(g, x, torch.zeros(8, 3, device=dev))
    # a forced split needs a workspace; one that is too small is refused on both levels
    G, X, C = (torch.zeros(s, device=dev) for s in ((256, 3), (256, 8), (3, 8)))
    with ops.tuning(linear16_wgrad_split=2):
        need = ops.linear16_wgrad_workspace_size(256, 3, 8)
        assert need == 2 * 3 * 8 * 4
        with pytest.raises(ValueError):
            ops.linear16_wgrad(G, X, C, workspace=torch.zeros(need // 4 - 1, device=dev))
        ops.linear16_wgrad(G, X, C, workspace=torch.zeros(need // 4, device=dev))
        with pytest.raises(_lib.DLRMHipError):
            _lib.call("dlrm_linear16_wgrad", 0, 256, 3, 8, ops._p(G), 3, ops._p(X), 8, 0, 0.0,
                      ops._p(C), 8, None, 0, None)
    with ops.tuning(linear16_wgrad_split=1):
        assert ops.linear16_wgrad_workspace_size(256, 3, 8) == 0
    for bad in ((5, 256, 3, 8, 3, 8, 0, 8), (0, 256, 3, 8, 3, 8, 7, 8), (0, -1, 3, 8, 3, 8, 0, 8),
                (0, 256, 3, 8, 2, 8, 0, 8), (0, 256, 3, 8, 3, 7, 0, 8), (0, 256, 3, 8, 3, 8, 0, 7)):
        ty, M, N, K, ldg, ldx, mode, ldc = bad
        with pytest.raises(_lib.DLRMHipError):
            _lib.call("dlrm_linear16_wgrad", ty, M, N, K, ops._p(G), ldg, ops._p(X), ldx, mode,
                      0.0, ops._p(C), ldc, None, 0, None)
    with pytest.raises(_lib.DLRMHipError):
        _lib.call("dlrm_linear16_dgrad", 0, 4, 3, 8, ops._p(g), 3, ops._p(w), 8, None, 0, None, 8,
                  None)
    for tile_key in ("linear16_dgrad_tile", "linear16_wgrad_tile"):
        with ops.tuning(**{tile_key: 64032}):  # not one of these kernels' tiles
            with pytest.raises(_lib.DLRMHipError):
                ops.linear16_dgrad(g, w) if "dgrad" in tile_key else \
                    ops.linear16_wgrad(g, x, torch.zeros(3, 8, device=dev))
    assert ops.linear16_dgrad(g[:0], w).shape == (0, 8)
