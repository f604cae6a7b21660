"""Host restatement of the pooled lookup over packed rows (dlrm_tbe_forward_rows, csrc/
tbe_rows.hip) and the cases that hold the kernel to it bit for bit.

The rule, per bag, over its VALID lookups in bag order (w = per-sample weight, or 1):
    Q8 / Q4 rows:  ws = fp32(w * scale);  wb = fp32(w * bias)
                   acc = fma(ws, q, fp32(acc + wb))         (one fused multiply-add, one add)
    F16 rows:      acc = fma(w, float(v), acc)
An index below 0 or past its table is dropped (and raises TBE_ERR_INDEX); an empty bag gives
zeros.  Every operation is a numpy fp32 operation or exact_rowsq.fma32, so it rounds once, as
the kernel's does.  tests/test_exact_rows_lookup_cpu.py proves the rule bitwise equal to
torch.ops.quantized.embedding_bag_byte_rowwise_offsets / embedding_bag_4bit_rowwise_offsets,
and shows that the cases below tell it apart from a reversed order and from a contracted
fma(w, bias, acc).

Plain helper module (no GPU needed), like exact_rowsq.py and exact_tbe.py."""
import numpy as np
import torch

import exact_rowsq as Q
import exact_tbe as E

F32 = np.float32
F16, Q8, Q4 = 1, 2, 3  # ops.ROWS_F16 / ROWS_Q8 / ROWS_Q4
FMTS = {"f16": F16, "q8": Q8, "q4": Q4}
BITS = {Q8: 8, Q4: 4}
ROWS = [40, 1, 7]  # rows per table of the general case
VARIANTS = (None, "reversed", "fma_bias")  # the rule, and two rules a kernel could follow instead


def lane_geom(nchunks, min_lpb=4):
    """(LPB, MAXV) of tbe_dispatch.hpp's lane_geom: the power of two >= nchunks, at least
    min_lpb (4: the packed-row lookup's smallest instantiation) and at most 64; chunks per
    lane above that."""
    lpb = min_lpb
    while lpb < nchunks and lpb < 64:
        lpb <<= 1
    return lpb, -(-nchunks // lpb)


def lookup_bag_lengths(D):
    """The bag lengths of a case at embedding dimension D, ascending: empty, one lookup, one
    under / exactly / one over a lane group (the l0 loop's second trip starts at LPB + 1),
    9 (= 4k + 1: one row of a batch of four), 4 LPB + 1 (a fifth trip of one lookup), 130."""
    lpb = lane_geom(D // 4)[0]
    return sorted({0, 1, lpb - 1, lpb, lpb + 1, 9, 4 * lpb + 1, 130})


def min_row_bytes(fmt, D):
    return 2 * D if fmt == F16 else Q.row_bytes(BITS[fmt], D)


def nan_row(fmt, D):
    """A row of 0xFF bytes: NaN scale and bias (Q8: fp32, Q4: fp16), NaN halves (F16)."""
    if fmt == F16:
        return np.full(D, 0xFFFF, dtype=np.uint16).view(np.float16)
    return np.full(Q.row_bytes(BITS[fmt], D), 0xFF, dtype=np.uint8)


def pack_table(w, fmt):
    """fp32 [rows, D] -> the table as the kernel reads it at the tight pitch: uint8
    [rows, row_bytes] (Q8 / Q4, exact_rowsq.pack_rows) or float16 [rows, D]."""
    if fmt == F16:
        return np.ascontiguousarray(w, dtype=F32).astype(np.float16)
    return Q.pack_rows(w, BITS[fmt])


def family_rows(rows, D, fmt, gen):
    """fp32 [rows, D]: exact_rowsq's normal, uniform and half_zero families, row i from family
    i mod 3."""
    fam = Q.families(rows, D, gen, BITS.get(fmt, 8))
    w = np.empty((rows, D), dtype=F32)
    for k, name in enumerate(("normal", "uniform", "half_zero")):
        w[k::3] = fam[name][k::3]
    return w


def make_psw(n, gen):
    """Per-sample weights: full 24-bit mantissas at exponents -3 .. 2 with random signs; every
    7th an exact 0, every 11th -1, and one subnormal."""
    m = gen.integers(1 << 23, 1 << 24, n).astype(np.float64) * 2.0 ** -23
    w = (m * 2.0 ** gen.integers(-3, 3, n) * gen.choice([-1.0, 1.0], n)).astype(F32)
    w[3::7] = 0
    w[5::11] = -1
    if n > 1:
        w[n // 2] = F32(3 * 2.0 ** -140)
        assert 0 < w[n // 2] < np.finfo(F32).tiny
    return w


def case_seed(fmt, D):
    """The seed of the general case of (format, D): the GPU tests compare the kernel on the
    very data on which the CPU tests show the rules apart."""
    return 1000 * fmt + D


def lookup_case(D, fmt, seed, invalid=False, pair=E.IDX_PAIRS[0], nan_rows=True, rows=ROWS,
                lengths=None, tables=None):
    """(case, table, psw).  Three tables of 40, 1 and 7 rows; the bag lengths
    lookup_bag_lengths(D) in one table and reversed in the next (``lengths``: another list).
    The rows come from family_rows, packed by pack_table (``tables``: fp32 rows to pack
    instead, one array per table).  With ``nan_rows`` every table of at least 2 rows has its
    row 0, every fifth row and every row that no index names set to 0xFF bytes, and the
    indices name only the others: the kernel reads row 0 for every inactive slot and must
    drop it by selection, so a NaN in an output shows a row multiplied by zero instead.
    ``invalid``: an index one past the table inside the longest bag of table 0 (past the
    first lane group at every D) and a -1 inside the longest bag of the last table."""
    gen = np.random.default_rng(seed)
    lens = list(lookup_bag_lengths(D) if lengths is None else lengths)
    per_table = [lens if t % 2 == 0 else lens[::-1] for t in range(len(rows))]
    pools = [np.array([r for r in range(n) if n == 1 or not nan_rows or (r and r % 5)])
             for n in rows]
    c0 = E.bags_csr("pool", [p.size for p in pools], per_table, seed)
    idx = np.concatenate([pools[t][c0.indices[c0.table == t]] for t in range(len(rows))])
    if invalid:
        B = len(lens)
        long0 = int(np.argmax(c0.bag_len[:B]))  # table 0
        idx[c0.offsets[long0] + c0.bag_len[long0] // 2 + 5] = rows[0]
        last = (len(rows) - 1) * B
        longl = last + int(np.argmax(c0.bag_len[last:]))
        idx[c0.offsets[longl] + c0.bag_len[longl] - 2] = -1
    case = E.Case(f"rows{D}", rows, len(lens), idx, c0.offsets, pair[0], pair[1])
    assert case.flag == (E.ERR_INDEX if invalid else 0)
    parts = [family_rows(n, D, fmt, gen) for n in rows] if tables is None else tables
    table = np.concatenate([pack_table(w, fmt) for w in parts])
    if nan_rows:
        named = np.zeros(case.total_rows, dtype=bool)
        named[case.row[case.valid]] = True
        for t, n in enumerate(rows):
            if n >= 2:
                sl = slice(case.row_base[t], case.row_base[t + 1])
                table[sl][~named[sl]] = nan_row(fmt, D)
                assert not named[case.row_base[t]]
    return case, table, make_psw(case.N, gen)


def ref_lookup(case, fmt, D, table, psw=None, variant=None):
    """fp32 [B, T, D]: the rule of this module's docstring on ``table`` (tight pitch: uint8
    [rows, row_bytes] or float16 [rows, D]).  Vectorised over bags and D, a loop over the
    position inside the bag.  ``variant``: None, or one of the rules the CPU tests must be
    able to tell from it: 'reversed' (the bag's lookups last to first), 'fma_bias'
    (acc + w*bias contracted into fma(w, bias, acc))."""
    assert variant in VARIANTS
    if fmt == F16:
        val = np.asarray(table, dtype=np.float16).astype(F32)  # exact
        assert val.shape == (case.total_rows, D)
        scale = bias = None
    else:
        val, scale, bias = Q.decode(table, BITS[fmt], D)
        assert val.shape == (case.total_rows, D)
    nb = case.T * case.B
    acc = np.zeros((nb, D), dtype=F32)
    w_all = np.ones(case.N, dtype=F32) if psw is None else np.asarray(psw, dtype=F32)
    lens, start = case.bag_len, case.offsets[:-1]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for p in range(int(lens.max()) if nb else 0):
            bags = np.flatnonzero(lens > p)
            pos = start[bags] + (lens[bags] - 1 - p if variant == "reversed" else p)
            ok = case.valid[pos]
            bags, pos = bags[ok], pos[ok]
            r, w = case.row[pos], w_all[pos]
            if fmt == F16:
                acc[bags] = Q.fma32(w[:, None], val[r], acc[bags])
                continue
            ws, wb = w * scale[r], w * bias[r]
            assert ws.dtype == wb.dtype == F32
            if variant == "fma_bias":
                inner = Q.fma32(w[:, None], np.repeat(bias[r, None], D, axis=1), acc[bags])
            else:
                inner = acc[bags] + wb[:, None]
            assert inner.dtype == F32
            acc[bags] = Q.fma32(ws[:, None], val[r], inner)
    return np.ascontiguousarray(acc.reshape(case.T, case.B, D).transpose(1, 0, 2))


def grid_stride_case(D, fmt, B, seed, rows=64):
    """(case, table, psw) of one table and B bags of 0, 1 or 2 lookups: more bags than the
    8192 capped workgroups hold, so every wave takes a second trip of its grid-stride loop.
    No NaN rows (every row is named at these sizes); weighted."""
    gen = np.random.default_rng(seed)
    lens = gen.integers(0, 3, B)
    lens[0], lens[-1], lens[-2] = 0, 2, 1
    off = np.concatenate([[0], np.cumsum(lens)])
    idx = gen.integers(0, rows, int(off[-1]))
    case = E.Case(f"stride{D}", [rows], B, idx, off, torch.int32, torch.int32)
    table = pack_table(family_rows(rows, D, fmt, gen), fmt)
    return case, table, make_psw(case.N, gen)
