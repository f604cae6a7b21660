"""Host restatement of the row-wise 8- and 4-bit packing rule (dlrm_rows_quantize, DESIGN.md
§20), its exact dequantiser, and tables that quantise without error.

pack_rows is the specification: tests/test_exact_rowsq_cpu.py proves it bitwise equal to
torch.ops.quantized.embedding_bag_byte_prepack / embedding_bag_4bit_prepack, and the device
kernel is compared bitwise with it.  Every operation is a numpy fp32 operation, so it rounds
once, as the kernel's does."""
import numpy as np

F32 = np.float32
STEP = {8: 2.0 ** -6, 4: 2.0 ** -3}  # exact_table's level step per width
TOP = {8: 255, 4: 15}


def row_bytes(bits, D):
    return D + 8 if bits == 8 else D // 2 + 4


def pack_rows(w, bits):
    """[rows, D] fp32 -> uint8 [rows, row_bytes]: the packing rule, in fp32, one rounding per
    operation.  D % 4 == 0 (the kernel's contract; the 4-bit layout needs D even)."""
    w = np.ascontiguousarray(w, dtype=F32)
    rows, D = w.shape
    assert bits in (4, 8) and D % 4 == 0
    out = np.empty((rows, row_bytes(bits, D)), dtype=np.uint8)
    if rows == 0:
        return out
    mn, mx = w.min(axis=1), w.max(axis=1)
    if bits == 8:
        rng = mx - mn
        scale = rng / F32(255.0)
        inv = F32(255.0) / (rng + F32(1e-8))
        q = np.rint((w - mn[:, None]) * inv[:, None])
        out[:, :D] = np.clip(q, 0, 255).astype(np.uint8)
        out[:, D:D + 4] = scale.astype(F32).view(np.uint8).reshape(rows, 4)
        out[:, D + 4:] = mn.astype(F32).view(np.uint8).reshape(rows, 4)
        return out
    mnh = mn.astype(np.float16).astype(F32)
    rng = mx - mnh
    scale = (rng / F32(15.0)).astype(np.float16).astype(F32)
    scale[scale == 0] = 1
    with np.errstate(divide="ignore"):
        inv = F32(1.0) / scale
    bad = np.isinf(inv)
    scale[bad] = 1
    inv[bad] = 1
    q = np.clip(np.rint((w - mnh[:, None]) * inv[:, None]), 0, 15).astype(np.uint8)
    out[:, :D // 2] = q[:, 0::2] | (q[:, 1::2] << 4)
    out[:, D // 2:D // 2 + 2] = scale.astype(np.float16).view(np.uint8).reshape(rows, 2)
    out[:, D // 2 + 2:] = mnh.astype(np.float16).view(np.uint8).reshape(rows, 2)
    return out


def decode(packed, bits, D):
    """The fields of packed rows: levels uint8 [rows, D], scale and bias fp32 [rows]."""
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    rows = packed.shape[0]
    assert packed.shape[1] == row_bytes(bits, D)
    if bits == 8:
        q = packed[:, :D]
        sb = packed[:, D:].copy().view(F32).reshape(rows, 2)
        return q, sb[:, 0].copy(), sb[:, 1].copy()
    b = packed[:, :D // 2]
    q = np.empty((rows, D), dtype=np.uint8)
    q[:, 0::2] = b & 0xF
    q[:, 1::2] = b >> 4
    sb = packed[:, D // 2:].copy().view(np.float16).reshape(rows, 2).astype(F32)
    return q, sb[:, 0].copy(), sb[:, 1].copy()


def fma32(a, b, c):
    """fp32 fma(a, b, c) with ONE rounding, for fp32 a, c and small integer b (a * b is then
    exact in fp64).  The fp64 sum is rounded to odd (TwoSum gives the exact error; an inexact
    sum with an even last bit moves one ulp towards the error), and a round-to-odd 53-bit value
    rounds to nearest-even fp32 as the exact value does: no double rounding.  The same holds
    for any b whose product with a is exact in fp64: an fp16 value widened to fp32 (a 24-bit
    times an 11-bit significand: 35 bits, the F16 lookup of exact_rows_lookup.py) or another
    fp32 value (48 bits)."""
    p = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
    c = np.broadcast_to(np.asarray(c, dtype=np.float64), p.shape)
    s = p + c
    cc = s - p
    e = (p - (s - cc)) + (c - cc)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def dequant(packed, bits, D):
    """fp32 [rows, D]: fma(scale, q, bias) per element, computed exactly (one rounding): the
    value the lookup and the gather kernels form."""
    q, scale, bias = decode(packed, bits, D)
    return fma32(scale[:, None], q, bias[:, None])


def exact_table(bits, rows, D, gen):
    """An fp32 [rows, D] table that quantises without error: per row mn = k * step (|k| <= 64,
    exact in fp16), entries mn + j * step at random levels j, the minimum (level 0) and the
    maximum (level 255 | 15) both present.  scale = step and inv = 1 / step are then exact
    powers of two, dequant(pack_rows(w)) == w bit for bit, and sums of up to 8 rows are exact
    in fp32 in any order."""
    step, top = STEP[bits], TOP[bits]
    k = gen.integers(-64, 65, size=(rows, 1))
    j = gen.integers(0, top + 1, size=(rows, D))
    pos = np.argsort(gen.random((rows, D)), axis=1)[:, :2]  # two distinct columns per row
    j[np.arange(rows), pos[:, 0]] = 0
    j[np.arange(rows), pos[:, 1]] = top
    return ((k + j) * step).astype(F32)


def tie_table(bits, rows, D, gen):
    """exact_table with every entry but the row's minimum and maximum moved half a step up
    (level j + 1/2, j < top): (x - mn) * inv lands exactly on .5, so the rounding mode of the
    level shows."""
    step, top = STEP[bits], TOP[bits]
    w = exact_table(bits, rows, D, gen)
    mn, mx = w.min(axis=1, keepdims=True), w.max(axis=1, keepdims=True)
    j = gen.integers(0, top, size=(rows, D))
    t = (mn.astype(np.float64) + (j + 0.5) * step).astype(F32)
    first_min = np.argmax(w == mn, axis=1)
    first_max = np.argmax(w == mx, axis=1)
    t[np.arange(rows), first_min] = mn[:, 0]
    t[np.arange(rows), first_max] = mx[:, 0]
    return t


def families(rows, D, gen, bits):
    """The row families of the packer tests, name -> fp32 [rows, D]."""
    half = gen.uniform(-0.05, 0.05, (rows, D)).astype(F32)
    half[gen.random((rows, D)) < 0.5] = 0
    return {
        "uniform": gen.uniform(-0.05, 0.05, (rows, D)).astype(F32),
        "normal": (gen.standard_normal((rows, D))
                   * 10.0 ** gen.uniform(-6, 3, (rows, 1))).astype(F32),
        "constant": np.repeat(gen.standard_normal((rows, 1)).astype(F32), D, axis=1),
        "zero": np.zeros((rows, D), dtype=F32),
        "half_zero": half,
        "ties": tie_table(bits, rows, D, gen),
    }
