"""The row-wise 8- and 4-bit packing rule on the host (no GPU): tests/exact_rowsq.pack_rows,
the specification of dlrm_rows_quantize, is bitwise torch's two CPU packers; the exact tables
of tests/exact_rowsq satisfy their own claims; and the argument checks of the new entry points
that need no device."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import exact_rowsq as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = [4, 16, 20, 64, 128, 200, 512]
ROWS = 20000


def _torch_pack(w, bits):
    t = torch.from_numpy(w)
    if bits == 8:
        return torch.ops.quantized.embedding_bag_byte_prepack(t).numpy()
    return torch.ops.quantized.embedding_bag_4bit_prepack(t).numpy()


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("D", DIMS)
def test_pack_rows_is_torchs_packer_bitwise(D, bits):
    gen = np.random.default_rng(1000 * bits + D)
    for name, w in Q.families(ROWS, D, gen, bits).items():
        got, want = Q.pack_rows(w, bits), _torch_pack(w, bits)
        assert got.shape == want.shape == (ROWS, Q.row_bytes(bits, D)), name
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (name, bad.size, bad[:5])


@pytest.mark.parametrize("bits", [8, 4])
def test_ties_round_to_even(bits):
    """The tie family really lands on .5: every level but the extremes is the even neighbour."""
    gen = np.random.default_rng(bits)
    D = 64
    w = Q.tie_table(bits, 500, D, gen)
    q, scale, bias = Q.decode(Q.pack_rows(w, bits), bits, D)
    assert (scale == Q.F32(Q.STEP[bits])).all()
    lvl = (w.astype(np.float64) - bias[:, None].astype(np.float64)) / Q.STEP[bits]
    tie = lvl != np.floor(lvl)
    assert tie.any() and (lvl[tie] - np.floor(lvl[tie]) == 0.5).all()
    assert (q[tie] % 2 == 0).all()
    assert (np.abs(q[tie] - lvl[tie]) == 0.5).all()
    assert (q[~tie] == lvl[~tie]).all()


def _fma_exact(a, b, c):
    """fp32 fma by rational arithmetic: one rounding, to the nearest fp32 (ties to even)."""
    v = Fraction(float(a)) * int(b) + Fraction(float(c))
    lo = np.float32(float(v))  # fp64 first: only a starting point, corrected below
    cands = {float(lo), float(np.nextafter(lo, np.float32(np.inf))),
             float(np.nextafter(lo, np.float32(-np.inf)))}
    best = min(cands, key=lambda x: (abs(Fraction(x) - v),
                                     int(np.float32(x).view(np.int32)) & 1))
    return np.float32(best)


def test_dequant_rounds_once():
    """fma32 against rational arithmetic, on fields chosen so that scale * q + bias needs more
    than 53 bits (where a plain fp64 sum followed by a cast could round twice)."""
    gen = np.random.default_rng(5)
    scale = (gen.standard_normal(4000) * 10.0 ** gen.uniform(-8, 2, 4000)).astype(np.float32)
    bias = (gen.standard_normal(4000) * 10.0 ** gen.uniform(-8, 2, 4000)).astype(np.float32)
    q = gen.integers(0, 256, 4000)
    got = Q.fma32(scale, q, bias)
    want = np.array([_fma_exact(a, b, c) for a, b, c in zip(scale, q, bias)], dtype=np.float32)
    assert (got.view(np.int32) == want.view(np.int32)).all()
    # a built double-rounding trap: p + c = 1 + 2^-24 + 2^-60 must round UP to 1 + 2^-23
    a = np.array([1.0], dtype=np.float32)
    c = np.array([2.0 ** -24 + 2.0 ** -60], dtype=np.float64)
    assert Q.fma32(a, np.array([1]), c)[0] == np.float32(1.0 + 2.0 ** -23)


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("D", [4, 16, 64, 200])
def test_exact_table_quantises_without_error(bits, D):
    gen = np.random.default_rng(D + bits)
    w = Q.exact_table(bits, 3000, D, gen)
    packed = Q.pack_rows(w, bits)
    q, scale, bias = Q.decode(packed, bits, D)
    assert (scale == Q.F32(Q.STEP[bits])).all() and (bias == w.min(axis=1)).all()
    assert q.min(axis=1).max() == 0 and q.max(axis=1).min() == Q.TOP[bits]
    back = Q.dequant(packed, bits, D)
    assert (back.view(np.int32) == w.view(np.int32)).all()
    assert (packed == _torch_pack(w, bits)).all()
    # bag sums of 8 rows: the same bits in two orders, in the lookup's formula
    # acc = fma(scale, q, acc + bias), and equal to the fp64 sum
    bags = gen.integers(0, 3000, size=(500, 8))
    fwd = np.zeros((500, D), dtype=np.float32)
    rev = np.zeros((500, D), dtype=np.float32)
    kern = np.zeros((500, D), dtype=np.float32)
    for l in range(8):
        fwd = fwd + w[bags[:, l]]
        rev = rev + w[bags[:, 7 - l]]
        r = bags[:, l]
        kern = Q.fma32(scale[r, None], q[r], (kern + bias[r, None]).astype(np.float32))
    f64 = w[bags].astype(np.float64).sum(axis=1)
    assert (fwd.view(np.int32) == rev.view(np.int32)).all()
    assert (fwd.astype(np.float64) == f64).all()
    assert (kern.view(np.int32) == fwd.view(np.int32)).all()


# ------------------------------------------------------------ the ABI and its checks --
def test_abi_v17_symbols():
    from dlrm_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()
    assert int(re.search(r"#define\s+DLRM_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 17
    assert _lib.ABI_VERSION >= 17 and _lib.load().dlrm_abi_version() == _lib.ABI_VERSION
    for name, nargs in (("dlrm_rows_quantize", 8), ("dlrm_interact_dot_forward_gather_rows", 15)):
        assert name in hdr and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)
    abi = open(os.path.join(ROOT, "dlrm-yx_amd", "csrc", "abi.cpp")).read()
    assert "&dlrm_rows_quantize" in abi and "&dlrm_interact_dot_forward_gather_rows" in abi


def test_rows_quantize_host_argument_checks():
    """The C entry points validate before they touch the device."""
    import ctypes
    from dlrm_hip import _lib, ops
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    INVALID, UNSUPPORTED = 1, 3
    q8, q4 = ops.ROWS_Q8, ops.ROWS_Q4
    call = lib.dlrm_rows_quantize
    assert call(p, ops.ROWS_F32, 0, 16, q8, p, 24, None) == 0  # rows == 0 launches nothing
    assert call(p, ops.ROWS_F32, 0, 16, q4, p, 12, None) == 0
    assert call(p, ops.ROWS_Q8, 1, 16, q8, p, 24, None) == INVALID  # source format
    assert call(p, ops.ROWS_F32, 1, 16, ops.ROWS_F16, p, 32, None) == INVALID  # destination
    assert call(p, ops.ROWS_F32, 1, 16, q8, p, 32, None) == INVALID  # row pitch
    assert call(p, ops.ROWS_F32, 1, 18, q8, p, 26, None) == UNSUPPORTED  # D % 4
    assert call(p, ops.ROWS_F32, 1, 516, q8, p, 524, None) == UNSUPPORTED  # D > 512
    assert call(p, ops.ROWS_F32, -1, 16, q8, p, 24, None) == INVALID
    g = lib.dlrm_interact_dot_forward_gather_rows
    for fmt in (ops.ROWS_F32, ops.ROWS_F16, 99):
        assert g(4, 3, 16, p, 16, p, fmt, 24, p, p, 0, p, 32, None, None) == UNSUPPORTED
    assert g(4, 3, 16, p, 16, p, q8, 32, p, p, 0, p, 32, None, None) == INVALID  # row pitch
    assert g(4, 3, 16, p, 16, p, q4, 24, p, p, 0, p, 32, None, None) == INVALID
    assert g(4, 3, 20, p, 20, p, q8, 28, p, p, 0, p, 32, None, None) == UNSUPPORTED  # D
    off = ctypes.c_void_p(p.value + 4)
    assert g(4, 3, 16, p, 16, off, q8, 24, p, p, 0, p, 32, None, None) == INVALID  # alignment
    assert g(0, 3, 16, p, 16, p, q8, 24, p, p, 0, p, 32, None, None) == 0  # B == 0


def test_python_argument_checks():
    from dlrm_hip import ops
    w = torch.zeros(3, 16)
    for bits in (0, 16, 32, "8"):
        with pytest.raises(ValueError):
            ops.rows_quantize(w, bits)
    with pytest.raises(ValueError):
        ops.rows_quantize(w.double(), 8)
    with pytest.raises(ValueError):
        ops.rows_quantize(w.to(torch.bfloat16), 4)
    with pytest.raises(ValueError):
        ops.rows_quantize(w[:, :8], 8)  # not contiguous
    with pytest.raises(ValueError):
        ops.rows_quantize(w, 8)  # a CPU tensor
    assert ops.tbe_row_bytes(ops.ROWS_Q8, 128) == Q.row_bytes(8, 128) == 136
    assert ops.tbe_row_bytes(ops.ROWS_Q4, 128) == Q.row_bytes(4, 128) == 68
