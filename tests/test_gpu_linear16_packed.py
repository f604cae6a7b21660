"""dlrm_linear16_pack / dlrm_linear16_forward_packed (16-bit MLP operands in memory) against
dlrm_linear16_forward, bit for bit (torch.equal, finite inputs), and against the fp64 product.
Operands are views into NaN-padded buffers that start past the buffer's base, outputs views into
sentinel-padded ones: a read past K or a write outside [:M, :N] shows."""
import numpy as np
import pytest
import torch

from dlrm_hip import ops
from exact_inputs import SENTINEL, full_mantissa, gemm_close, int_matrix, padded

pytestmark = pytest.mark.gpu

dev = "cuda:0"
NAN = float("nan")
TILES = list(ops.LINEAR16_TILES)  # DLRM_TUNE_LINEAR16_TILE values: the four tiles
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
MANT = {"bf16": (7, -126), "fp16": (10, -14)}  # stored mantissa bits, smallest normal exponent
# (M, N, K): one chunk | tails in every tile, partial third k-step | one step, odd N | fp32 X only
SHAPES = [(1, 8, 8), (33, 72, 136), (70, 130, 64), (32, 64, 13)]


def _offset_view(t, ld, off):
    r, c = t.shape
    flat = torch.full((off + (r + 2) * ld,), NAN, dtype=t.dtype, device=t.device)
    view = flat[off:off + r * ld].view(r, ld)[:, :c]
    view.copy_(t)
    return view


def _x_layouts(x, xk, dt):
    """fp32 with 16-byte loads and with element loads, or r16(x) 16 bytes into its buffer."""
    K = x.shape[1]
    if xk == "fp32":
        return [padded(x, 2, (K + 4) // 4 * 4 - K, NAN), _offset_view(x, K + 1, 1)]
    return [_offset_view(x.to(DTYPES[dt]), K + 8, 8)]


def _out(M, N, yk, dt):
    dtype, pad = (torch.float32, 3) if yk == "fp32" else (DTYPES[dt], 8 - N % 8)
    return padded(torch.zeros(M, N, dtype=dtype, device=dev), 2, pad, SENTINEL)


def _only_wrote(Y, want):
    exp = torch.full_like(Y._base, SENTINEL)
    exp[:Y.shape[0], :Y.shape[1]] = want
    return torch.equal(Y._base, exp)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_pack(dt):
    """W.to(dtype) bit for bit, zero past K: contiguous, NaN-padded and unaligned sources."""
    for (_, N, K) in SHAPES:
        g = torch.Generator(device=dev).manual_seed(N + K)
        W = full_mantissa((N, K), g) * 0.37 - 0.5
        Wv = padded(W, 2, (K + 4) // 4 * 4 - K, NAN)
        for src in (W, Wv, _offset_view(W, K + 1, 1)):
            p = ops.linear16_pack(src, dt)
            assert p.wp.shape == (N, max((K + 63) // 64 * 64, 64)) and (p.N, p.K) == (N, K)
            assert torch.equal(p.wp[:, :K].view(torch.int16), W.to(DTYPES[dt]).view(torch.int16))
            assert not bool(p.wp[:, K:].view(torch.int16).any())


@pytest.mark.parametrize("yk", ["fp32", "16"])
@pytest.mark.parametrize("xk", ["fp32", "16"])
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_bit_equal_exact_and_close(dt, tile, xk, yk):
    """Integer operands: the packed forward equals ops.linear16_forward on the fp32 operands
    under the same tile, bias and ReLU (cast to the dtype for a 16-bit Y) and the fp64 product
    exactly; only Y[:M, :N] is written.  Full-mantissa operands: still bit for bit, and within
    gemm_close's fp32-accumulation bound of the fp64 product of the ROUNDED operands - plus, for
    a 16-bit Y, one rounding of the result: half an ulp of the dtype at that value, 2^(e-8) for
    bf16 and 2^(e-11) for fp16 with 2^e <= |y| < 2^(e+1).  That is 2^-9 / 2^-12 relative to the
    top of the binade only; relative to |y| a correct nearest-even rounding reaches 2^-8 / 2^-11
    (measured on MI355X with the flat relative 2^-9: worst |err| / tol 1.50 at (1, 8, 8) bf16,
    the bit-equality holding), so the half ulp is taken per binade."""
    worst_all = 0.0
    for (M, N, K) in SHAPES:
        if xk == "16" and K % 8:
            continue
        g = torch.Generator(device=dev).manual_seed(17 * M + 5 * N + K)
        x, w = int_matrix((M, K), -4, 4, g), int_matrix((N, K), -4, 4, g)
        b = int_matrix((N,), -8, 8, g, nonzero=False)
        W = padded(w, 2, (K + 4) // 4 * 4 - K, NAN)
        W._base[:N, K] = b
        packed = ops.linear16_pack(W, dt)
        acc = x.double() @ w.double().t()
        for xv in _x_layouts(x, xk, dt):
            for bias, relu in ((W._base[:N, K], True), (None, False), (b.clone(), False)):
                ref = acc + (b.double() if bias is not None else 0.0)
                ref = (torch.relu(ref) if relu else ref).float()
                Y = _out(M, N, yk, dt)
                with ops.tuning(linear16_tile=tile):
                    base = ops.linear16_forward(x, w, bias, relu=relu, dtype=dt)
                    ops.linear16_forward_packed(xv, packed, bias, relu=relu, out=Y)
                assert torch.equal(base, ref), (M, N, K, relu)
                assert _only_wrote(Y, ref.to(Y.dtype)), (M, N, K, xv.stride(0), relu)
        g = torch.Generator(device=dev).manual_seed(3 * M + N + 7 * K)
        x = full_mantissa((M, K), g) - 1.5
        w = (full_mantissa((N, K), g) - 1.5) * 0.25
        b = full_mantissa((N,), g) - 1.5
        packed = ops.linear16_pack(w, dt)
        xr, wr = x.to(DTYPES[dt]).double(), w.to(DTYPES[dt]).double()
        ref = (xr @ wr.t() + b.double()).cpu().numpy()
        absprod = (xr.abs() @ wr.abs().t() + b.double().abs()).cpu().numpy()
        for xv in _x_layouts(x, xk, dt):
            Y = _out(M, N, yk, dt)
            with ops.tuning(linear16_tile=tile):
                base = ops.linear16_forward(x, w, b, dtype=dt)
                ops.linear16_forward_packed(xv, packed, b, out=Y)
            assert _only_wrote(Y, base.to(Y.dtype)), (M, N, K)
            got = Y.double().cpu().numpy()
            if yk == "fp32":
                ok, worst = gemm_close(got, ref, absprod, K)
            else:  # gemm_close's bound on the fp32 y, then |r16(y) - y| <= u |y|
                tol = 1e-5 * np.maximum(1.0, np.abs(ref)) + 2.0 * K * 2.0 ** -24 * absprod
                bits, emin = MANT[dt]
                e = np.floor(np.log2(np.maximum(np.abs(ref) + tol, 2.0 ** emin)))
                tol = tol + np.exp2(e - bits - 1)
                worst = float((np.abs(got - ref) / tol).max())
                ok = worst <= 1.0
            worst_all = max(worst_all, worst)
            assert ok, ((M, N, K), worst)
    print(f"linear16_packed {dt} tile {tile} x {xk} y {yk}: worst |err| / tol = {worst_all:.4f}")


def test_bad_arguments():
    from dlrm_hip._lib import DLRMHipError
    bf, z = torch.bfloat16, lambda *s, **kw: torch.zeros(*s, device=dev, **kw)
    packed = ops.linear16_pack(z(3, 16), "bf16")
    x = z(4, 16)
    for call in (
            lambda: ops.linear16_pack(z(3, 16), "int8"),
            lambda: ops.linear16_pack(z(3, 24), "bf16", out=packed),  # another K
            lambda: ops.Linear16Weights(z(3, 32, dtype=bf), 3, 16, "bf16"),  # ldwp % 64
            lambda: ops.linear16_forward_packed(x, z(3, 16)),  # not packed
            lambda: ops.linear16_forward_packed(z(4, 24), packed),  # K mismatch
            lambda: ops.linear16_forward_packed(x.half(), packed),  # fp16 x, bf16 weights
            lambda: ops.linear16_forward_packed(z(4, 17, dtype=bf)[:, 1:], packed),  # alignment
            lambda: ops.linear16_forward_packed(z(4, 20, dtype=bf)[:, :16], packed),  # ldx % 8
            lambda: ops.linear16_forward_packed(z(4, 12, dtype=bf),
                                                ops.linear16_pack(z(3, 12), "bf16")),  # K % 8
            lambda: ops.linear16_forward_packed(x, packed, out=z(4, 4)),
            lambda: ops.linear16_forward_packed(x, packed, out=z(4, 3, dtype=bf)),  # ldy % 8
            lambda: ops.linear16_forward_packed(x, packed, out_dtype=torch.float16)):
        with pytest.raises(ValueError):
            call()
    assert ops.linear16_forward_packed(x[:0], packed).shape == (0, 3)
    y = ops.linear16_forward_packed(x.to(bf), packed, out_dtype=bf)
    assert y.dtype == bf and y.shape == (4, 3) and y.stride(0) == 8 and not bool(y.any())
    Y, p, st = z(4, 8), ops._p, ops._stream(torch.device(dev))
    good = [0, 4, 3, 16, p(x), 0, 16, p(packed.wp), 64, None, 0, 0, p(Y), 0, 8, st]
    ops._lib.call("dlrm_linear16_forward_packed", *good)
    for change in ({0: 2}, {5: 2}, {13: 7}, {8: 32}, {8: 96}, {14: 2}, {5: 1, 6: 20},
                   {5: 1, 3: 12}, {13: 1, 14: 4},
                   {5: 1, 4: ops.ctypes.c_void_p(x.data_ptr() + 2)}):
        args = list(good)
        for pos, bad in change.items():
            args[pos] = bad
        with pytest.raises(DLRMHipError):
            ops._lib.call("dlrm_linear16_forward_packed", *args)
    with pytest.raises(DLRMHipError):
        ops._lib.call("dlrm_linear16_pack", 0, 3, 16, p(x), 16, p(packed.wp), 48, st)
