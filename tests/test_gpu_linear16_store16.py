"""The 16-bit Linear kernels on operands that are ALREADY 16-bit in memory (dlrm_linear16_*_fmt,
reached through ops.linear16_forward / _dgrad / _wgrad on bf16 / fp16 tensors) against the
fp32-operand kernels on the same values widened to fp32: the MFMA sees the same operand bits
in the same order, so fp32 outputs compare with torch.equal and a 16-bit output equals the
fp32 one cast once.  One case per kernel is also held to an fp64 product of the widened
operands under the fp32-accumulation bound the linear16 tests use (exact_inputs.gemm_close).

Reduction depths 1, 63, 64, 65, 130 (a tail step; a split that ends mid-step) where the
reduction operand may have any depth (wgrad's batch, an fp32 X / dY); a 16-bit operand whose
reduction runs along its rows moves whole 8-element chunks, so its depths are 8, 64, 72, 136.
Output extents 8 and 72 (one chunk; a last chunk at the 64-wide tile's edge), M = 1, every
leading dimension larger than the extent with NaN in every operand pad, outputs in
sentinel-padded buffers with guard rows."""
import ctypes

import pytest
import torch

from exact_inputs import SENTINEL, gemm_close, padded
from linear16_ref import DTYPES

pytestmark = pytest.mark.gpu

dev = "cuda:0"
NAN = float("nan")
TILES = [0, 128128, 128064, 64064, 32064]  # 0 = the planner
DEPTHS = [1, 63, 64, 65, 130]
DEPTHS8 = [8, 64, 72, 136]
LR = 0.25


@pytest.fixture(scope="module")
def ops():
    from dlrm_hip import ops as _ops
    return _ops


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator(device=dev).manual_seed(seed), device=dev)


def _in(t, dtype=None):
    """``t`` (cast to ``dtype``) in a NaN-padded buffer: two pad rows, a row stride that is a
    multiple of 8 and larger than the width."""
    t = t if dtype is None else t.to(dtype)
    return padded(t, 2, 16 - t.shape[1] % 8, NAN)


def _out(M, N, dtype):
    return padded(torch.zeros((M, N), dtype=dtype, device=dev), 2, 8, SENTINEL)


def pads_intact(view):
    """exact_inputs.pads_intact for a buffer of any element size: everything outside the view
    (pad columns, guard rows) still holds SENTINEL bitwise.  (The shared helper views a 0-dim
    fill value as int32, which a 2-byte type does not allow.)"""
    buf, (r, c) = view._base, view.shape
    as_int = torch.int32 if buf.element_size() == 4 else torch.int16
    fill = torch.full((1,), SENTINEL, dtype=buf.dtype, device=buf.device).view(as_int)
    return all(bool((part.contiguous().view(as_int) == fill).all())
               for part in (buf[:r, c:], buf[r:]))


def _wide(t):
    return _in(t.float())


def _mask(M, K, seed):
    m = _rand((M, K), seed)
    flat = m.view(-1)
    flat[::5] = 0.0
    flat[1::7] = -0.0
    flat[flat.numel() // 2] = NAN
    return m


# (x16, y16) / (dy16, dx16) / (dy16, x16): the built combinations, the mixed ones included
FORMATS = [(True, True), (True, False), (False, True)]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_forward_matches_the_fp32_operand_kernel(ops, dt, tile):
    T = DTYPES[dt]
    with ops.tuning(linear16_tile=tile):
        for x16, y16 in FORMATS:
            for (M, N), K in zip([(1, 8), (33, 72), (70, 8), (5, 72), (130, 136)],
                                 DEPTHS8 + [72] if x16 else DEPTHS):
                x, w, b = _rand((M, K), K), _in(_rand((N, K), N + K)), _rand((N,), 3)
                xin = _in(x, T) if x16 else _in(x)
                got = ops.linear16_forward(xin, w, b, relu=True, dtype=dt,
                                           out=_out(M, N, T if y16 else torch.float32))
                ref = ops.linear16_forward(_wide(xin), w, b, relu=True, dtype=dt)
                assert torch.equal(got, ref.to(T) if y16 else ref), (x16, y16, M, N, K)
                assert pads_intact(got)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_dgrad_matches_the_fp32_operand_kernel(ops, dt, tile):
    T = DTYPES[dt]
    with ops.tuning(linear16_dgrad_tile=tile):
        for dy16, dx16 in FORMATS:
            for (M, K), N in zip([(1, 8), (33, 72), (70, 8), (5, 72), (130, 136)],
                                 DEPTHS8 + [72] if dy16 else DEPTHS):
                dy, w = _rand((M, N), N), _in(_rand((N, K), N + K))
                gin = _in(dy, T) if dy16 else _in(dy)
                # the mask is of dX's format: zeros of both signs, negatives and a NaN
                mask = _in(_mask(M, K, 7), T if dx16 else None)
                for m in (mask, None):
                    got = ops.linear16_dgrad(gin, w, m, dtype=dt,
                                             out=_out(M, K, T if dx16 else torch.float32))
                    ref = ops.linear16_dgrad(_wide(gin), w, None if m is None else _wide(m),
                                             dtype=dt)
                    assert torch.equal(got, ref.to(T) if dx16 else ref), (dy16, dx16, M, N, K)
                    assert pads_intact(got)
                    assert m is None or bool((got[torch.isnan(m)] == 0).all())


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_wgrad_matches_the_fp32_operand_kernel(ops, dt, tile, split):
    """K = 9 and 73: [inp | 1], the constant-1 column inside the chunk that crosses the extent
    (NaN behind it)."""
    T = DTYPES[dt]
    with ops.tuning(linear16_wgrad_tile=tile, linear16_wgrad_split=split):
        for dy16, x16 in FORMATS:
            for M, (N, K) in zip(DEPTHS, [(8, 9), (72, 73), (8, 72), (72, 8), (40, 129)]):
                dy, x = _rand((M, N), M + N), _rand((M, K), M + K)
                x[:, K - 1] = 1.0
                gin = _in(dy, T) if dy16 else _in(dy)
                xin = _in(x, T) if x16 else _in(x)
                c0 = _rand((N, K), 11)
                # store, SGD at a host rate, SGD at a device rate (the _fmt_dev entry point)
                for lr in (None, LR, torch.tensor([LR], device=dev)):
                    got = ops.linear16_wgrad(gin, xin, padded(c0, 2, 3, SENTINEL), lr=lr, dtype=dt)
                    ref = ops.linear16_wgrad(_wide(gin), _wide(xin), c0.clone(), lr=lr, dtype=dt)
                    assert torch.equal(got, ref), (dy16, x16, M, N, K, lr)
                    assert lr is None or not torch.equal(got, c0)
                    assert pads_intact(got)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_against_fp64_products(ops, dt):
    """One case per kernel: the fp64 product of the stored operands (the 16-bit values and the
    fp32 weights rounded as the kernel rounds them) under |err| <= 1e-5 max(1, |ref|) +
    2 depth 2^-24 (|A| |B|)."""
    T = DTYPES[dt]
    M, N, K = 130, 72, 136
    x, dy, w = _rand((M, K), 1).to(T), _rand((M, N), 2).to(T), _rand((N, K), 3)
    x64, dy64, w64 = x.double(), dy.double(), w.to(T).double()
    cases = [
        (ops.linear16_forward(_in(x), _in(w), dtype=dt), x64 @ w64.t(),
         x64.abs() @ w64.abs().t(), K),
        (ops.linear16_dgrad(_in(dy), _in(w), dtype=dt), dy64 @ w64, dy64.abs() @ w64.abs(), N),
        (ops.linear16_wgrad(_in(dy), _in(x), torch.zeros((N, K), device=dev), dtype=dt),
         dy64.t() @ x64, dy64.abs().t() @ x64.abs(), M),
    ]
    for got, ref, absprod, depth in cases:
        assert got.dtype == torch.float32
        ok, worst = gemm_close(got.cpu(), ref.cpu(), absprod.cpu(), depth)
        assert ok, worst


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_refusals_write_nothing(ops, dt):
    from dlrm_hip import _lib
    T = DTYPES[dt]
    M, N, K = 16, 8, 16
    x, w = _in(_rand((M, K), 1), T), _in(_rand((N, K), 2))
    out = _out(M, N, T)
    kind = ops.MLP16_TYPES[dt]
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731

    def fwd(xp, xk, ldx, yk):
        _lib.call("dlrm_linear16_forward_fmt", kind, M, N, K, xp, xk, ldx, ptr(w), w.stride(0),
                  None, 0, 0, ptr(out), yk, out.stride(0), ops._stream(x.device))

    for args, status in (((ptr(x, 2), 1, x.stride(0), 1), "SHAPE"),       # a misaligned base
                         ((ptr(x), 1, x.stride(0) - 4, 1), "SHAPE"),      # ld % 8 != 0
                         ((ptr(w), 0, w.stride(0), 0), "UNSUPPORTED")):   # fp32 to fp32
        with pytest.raises(_lib.DLRMHipError, match=status):
            fwd(*args)
    # the same through ops: a view one element into the buffer, a stride of 12, and a 16-bit
    # mask beside an fp32 dX (no kernel is built for it)
    flat = x._base.view(-1)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.linear16_forward(flat[1:1 + M * 24].view(M, 24)[:, :K], w, out=out, dtype=dt)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.linear16_forward(flat[:M * 12].view(M, 12)[:, :8], w[:, :8], out=out, dtype=dt)
    dx = padded(torch.zeros((M, K), device=dev), 2, 4, SENTINEL)
    g = _in(_rand((M, N), 3), T)
    with pytest.raises(_lib.DLRMHipError, match="UNSUPPORTED"):
        ops.linear16_dgrad(g, w, mask=x, out=dx, dtype=dt)
    # wgrad (dY = g, X = x, C = dx): the library's own checks
    for gp, ldg, xk, status in ((ptr(g, 2), g.stride(0), 1, "SHAPE"),
                                (ptr(g), g.stride(0) - 4, 1, "SHAPE"),
                                (ptr(dx), dx.stride(0), 0, "UNSUPPORTED")):  # fp32 dY, fp32 X
        with pytest.raises(_lib.DLRMHipError, match=status):
            _lib.call("dlrm_linear16_wgrad_fmt", kind, M, N, K, gp, xk, ldg,
                      ptr(dx) if xk == 0 else ptr(x), xk, dx.stride(0) if xk == 0 else x.stride(0),
                      0, 0.0, ptr(dx), dx.stride(0), None, 0, ops._stream(x.device))
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and pads_intact(out) and bool((dx == 0).all()) and pads_intact(dx)
