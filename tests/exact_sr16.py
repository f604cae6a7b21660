"""Host restatement (numpy) of the fp16 tables' stochastic rounding (include/dlrm_hip.h, ABI
v16): splitmix64, the counter-based 16-bit draw r16(seed, step, row, column) and the rounding
sr16(v, r16).  Written from the definition - floor, ulp and fraction in float64, where every
quantity of an fp32 input is exact - not from the bit trick the kernel uses; the CPU tests
prove the two agree.  tests/test_exact_sr16_cpu.py proves this file, the GPU tests compare
the kernels with it bitwise."""
import numpy as np

_M = (1 << 64) - 1


def splitmix64(z):
    """uint64 array (or int) -> uint64 array; arithmetic wraps."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sr_key(seed, step):
    return splitmix64(splitmix64(np.uint64(int(seed) & _M)) ^ np.uint64(int(step) & _M))


def r16(seed, step, rows, D):
    """The draws of the GLOBAL rows ``rows`` (any ints < 2^64): uint32 [len(rows), D]."""
    rows = np.asarray([int(r) & _M for r in np.asarray(rows, dtype=object).reshape(-1)],
                      dtype=np.uint64)
    C = np.uint64((D + 3) // 4)
    d = np.arange(D, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ctr = rows[:, None] * C + (d // np.uint64(4))[None, :]
    word = splitmix64(sr_key(seed, step) ^ ctr)
    return ((word >> (np.uint64(16) * (d % np.uint64(4)))[None, :]) & np.uint64(0xFFFF)).astype(
        np.uint32)


def sr16(v, r):
    """fp32 array v, draws r (integers 0..65535, broadcast) -> fp16 array, by the definition:
    ulp = 2^(max(floor(log2 |v|), -14) - 10), t = floor(|v| / ulp) * ulp, frac = (|v| - t) / ulp,
    |result| = t + ulp if r < frac * 65536 else t (65536 stored as Inf), v's sign kept; NaN and
    +-Inf as the nearest-even conversion."""
    v = np.asarray(v, dtype=np.float32)
    r = np.broadcast_to(np.asarray(r), v.shape).astype(np.float64)
    fin = np.isfinite(v)
    a = np.abs(np.where(fin, v, np.float32(1.0))).astype(np.float64)
    a_f = np.where(fin, a, 1.0)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(a_f > 0, a_f, 1.0)))
    # log2 of an fp32 in float64 can only be off at exact powers of two' neighbours: fix up
    e = np.where(np.ldexp(1.0, e.astype(np.int64)) > a_f, e - 1, e)
    e = np.where(np.ldexp(1.0, (e + 1).astype(np.int64)) <= a_f, e + 1, e)
    e = np.where(a_f > 0, e, -14.0)
    ulp = np.ldexp(1.0, (np.maximum(e, -14.0) - 10).astype(np.int64))
    q = a_f / ulp                      # exact: a power-of-two scaling
    t = np.floor(q)
    frac = q - t                       # exact
    mag = (t + (r < frac * 65536.0)) * ulp
    mag = np.where(a_f >= 65536.0, np.inf, mag)
    with np.errstate(over="ignore"):
        h = mag.astype(np.float16)     # exact: on the fp16 grid, or 65536 / inf -> inf
    assert np.array_equal(np.where(np.isinf(h), np.inf, h.astype(np.float64)),
                          np.where(mag >= 65536.0, np.inf, mag))
    hb = h.view(np.uint16) | (np.signbit(v).astype(np.uint16) << np.uint16(15))
    with np.errstate(over="ignore", invalid="ignore"):
        ne = v.astype(np.float16).view(np.uint16)
    return np.where(fin, hb, ne).astype(np.uint16).view(np.float16)


def sr16_table(v, seed, step, first_row=0):
    """sr16 of a whole [rows, D] fp32 table whose row 0 is global row ``first_row``."""
    v = np.asarray(v, dtype=np.float32)
    rows = np.arange(v.shape[0], dtype=np.uint64) + np.uint64(first_row)
    return sr16(v, r16(seed, step, rows, v.shape[1]))


def sr16_bit_trick(v, r):
    """The normal-range shortcut: bits(v) + (0x1fff - (r >> 3)), low 13 bits cleared, read
    as fp32 (valid for 2^-14 <= |v| < 65536)."""
    v = np.asarray(v, dtype=np.float32)
    b = v.view(np.uint32)
    r = np.broadcast_to(np.asarray(r), v.shape).astype(np.uint32)
    x = (b + (np.uint32(0x1FFF) - (r >> np.uint32(3)))) & np.uint32(0xFFFFE000)
    with np.errstate(over="ignore"):
        return x.view(np.float32).astype(np.float16)
