"""CPU proofs of tests/exact_rows_lookup.py (no GPU): the rule ref_lookup states is bitwise
torch's two quantized lookups, it is the fp64 sum where every sum is exact, the cases hold
what they promise, and their data tell the rule apart from the rules a kernel could follow
instead (a reversed order, a contracted fma(w, bias, acc))."""
import numpy as np
import pytest
import torch

import exact_rows_lookup as R
import exact_rowsq as Q
import exact_tbe as E

DIMS = [4, 16, 20, 64, 128, 200, 260, 512]
GPU_DIMS = [4, 16, 20, 64, 128, 200, 256, 260, 512]  # test_gpu_rows_exact.py


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _torch_lookup(case, fmt, table, psw):
    """torch's op per table -> fp32 [B, T, D]."""
    op = (torch.ops.quantized.embedding_bag_byte_rowwise_offsets if fmt == R.Q8
          else torch.ops.quantized.embedding_bag_4bit_rowwise_offsets)
    outs = []
    for t in range(case.T):
        a, e = case.offsets[t * case.B], case.offsets[(t + 1) * case.B]
        w = torch.from_numpy(table[case.row_base[t]:case.row_base[t + 1]].copy())
        idx = torch.from_numpy(case.indices[a:e].copy())
        off = torch.from_numpy(case.offsets[t * case.B:(t + 1) * case.B] - a)
        pw = None if psw is None else torch.from_numpy(psw[a:e].copy())
        outs.append(op(w, idx, off, False, 0, False, pw, None, False).numpy())
    return np.stack(outs, axis=1)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("fmt", ["q8", "q4"])
@pytest.mark.parametrize("D", DIMS)
def test_ref_lookup_is_torchs_op_bitwise(D, fmt, weighted):
    """Rows without the NaN rows and indices all valid: torch has neither convention."""
    f = R.FMTS[fmt]
    case, table, psw = R.lookup_case(D, f, seed=100 + D, nan_rows=False)
    psw = psw if weighted else None
    got = R.ref_lookup(case, f, D, table, psw)
    want = _torch_lookup(case, f, table, psw)
    assert got.shape == want.shape == (case.B, case.T, D)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, (len(bad), bad[:3], [int(case.bag_len[t * case.B + b])
                                                for b, t, _ in bad[:3]])


@pytest.mark.parametrize("fmt", ["q8", "q4"])
@pytest.mark.parametrize("D", [16, 64, 200])
def test_exact_tables_give_the_fp64_sum(D, fmt):
    """exact_rowsq.exact_table rows, bags of 8 lookups or fewer: every partial sum is exact in
    fp32, so the rule gives the fp64 sum of the dequantised rows, whatever the order."""
    f = R.FMTS[fmt]
    gen = np.random.default_rng(D)
    tables = [Q.exact_table(R.BITS[f], n, D, gen) for n in R.ROWS]
    case, table, _ = R.lookup_case(D, f, seed=D, lengths=[0, 1, 2, 3, 5, 8, 7, 4],
                                   tables=tables)
    assert case.bag_len.max() == 8
    deq = Q.dequant(table, R.BITS[f], D).astype(np.float64)
    want = np.zeros((case.T * case.B, D))
    np.add.at(want, case.bag, deq[case.row])
    assert np.isfinite(want).all()  # no 0xFF row is named
    want = want.reshape(case.T, case.B, D).transpose(1, 0, 2)
    for variant in (None, "reversed"):
        got = R.ref_lookup(case, f, D, table, variant=variant)
        assert (got.astype(np.float64) == want).all(), variant


@pytest.mark.parametrize("fmt", ["f16", "q8", "q4"])
@pytest.mark.parametrize("D", GPU_DIMS)
def test_the_cases_tell_the_rules_apart(D, fmt):
    """On the general case's own data a reversed order changes bits, weighted or not, and on
    the weighted quantized case so does fma(w, bias, acc) in place of the separate add: a
    kernel following either rule cannot pass the bitwise comparison."""
    f = R.FMTS[fmt]
    for invalid in (False, True):
        case, table, psw = R.lookup_case(D, f, seed=R.case_seed(f, D), invalid=invalid)
        for w in (None, psw):
            ref = R.ref_lookup(case, f, D, table, w)
            assert np.isfinite(ref).all()  # the 0xFF rows are never summed
            rev = R.ref_lookup(case, f, D, table, w, variant="reversed")
            differ = (_bits(ref) != _bits(rev)).any(axis=2)  # [B, T]
            # bags of 0 or 1 lookups have one order only.  Weighted, at least three in four
            # of the bags of 3 or more show the order; unweighted fewer can (the bags of the
            # 1-row table sum one row, and sums of a few fp16 values are often exact)
            lens = case.bag_len.reshape(case.T, case.B).T
            assert not differ[lens <= 1].any()
            assert differ[lens >= 3].mean() >= (0.75 if w is not None else 0.1), \
                (invalid, w is not None, differ[lens >= 3].mean())
        if f != R.F16:
            con = R.ref_lookup(case, f, D, table, psw, variant="fma_bias")
            ref = R.ref_lookup(case, f, D, table, psw)
            differ = (_bits(ref) != _bits(con)).any(axis=2)
            assert differ[lens >= 3].mean() >= 0.5, (invalid, differ[lens >= 3].mean())
            # unweighted, fma(1, bias, acc) IS the add: only the weighted case can show it
            con1 = R.ref_lookup(case, f, D, table, None, variant="fma_bias")
            assert (_bits(con1) == _bits(R.ref_lookup(case, f, D, table, None))).all()


def test_lane_geometry_and_bag_lengths():
    from dlrm_hip import ops
    assert (R.F16, R.Q8, R.Q4) == (ops.ROWS_F16, ops.ROWS_Q8, ops.ROWS_Q4)
    assert E.ERR_INDEX == ops.TBE_ERR_INDEX
    want = {4: (4, 1), 16: (4, 1), 20: (8, 1), 64: (16, 1), 128: (32, 1), 200: (64, 1),
            256: (64, 1), 260: (64, 2), 512: (64, 2)}
    assert sorted(want) == GPU_DIMS
    for D, geom in want.items():
        assert R.lane_geom(D // 4) == geom
        lpb = geom[0]
        assert R.lookup_bag_lengths(D) == sorted({0, 1, lpb - 1, lpb, lpb + 1, 9, 4 * lpb + 1, 130})
    for D in range(4, 516, 4):  # the fp32 lookup's lane group, but for the floor of 4 lanes
        assert (R.lane_geom(D // 4)[0] == E.dispatch(D)[1]) == (D not in (4, 8)), D
        assert R.lane_geom(D // 4)[1] <= 2
    assert R.lane_geom(1, 1) == (1, 1) and R.lane_geom(129) == (64, 3)


@pytest.mark.parametrize("fmt", ["f16", "q8", "q4"])
def test_case_holds_what_it_promises(fmt):
    f, D = R.FMTS[fmt], 20
    case, table, psw = R.lookup_case(D, f, seed=1, invalid=True)
    assert case.rows == R.ROWS and case.B == len(R.lookup_bag_lengths(D))
    for t in range(case.T):  # the lengths, reversed in every other table
        lens = case.bag_len[t * case.B:(t + 1) * case.B].tolist()
        assert lens == (R.lookup_bag_lengths(D) if t % 2 == 0 else R.lookup_bag_lengths(D)[::-1])
    raw = table.view(np.uint16 if f == R.F16 else np.uint8)
    full = 0xFFFF if f == R.F16 else 0xFF
    for t in (0, 2):
        assert (raw[case.row_base[t]] == full).all() and (raw[case.row_base[t] + 5] == full).all()
    assert not (raw[case.row_base[1]] == full).all()  # the 1-row table's row is a real one
    named = np.unique(case.row[case.valid])
    assert not (raw[named] == full).all(axis=1).any()
    # the two invalid indices: one past table 0, -1 in the last table, both deep in a long bag
    bad = np.flatnonzero((case.bag >= 0) & ~case.valid)
    assert case.indices[bad].tolist() == [40, -1] and case.table[bad].tolist() == [0, 2]
    for p in bad:
        assert case.bag_len[case.bag[p]] >= 130 and p - case.offsets[case.bag[p]] > 64
    assert case.flag == E.ERR_INDEX
    # dropped means: the result of the batch without them
    keep = np.ones(case.N, dtype=bool)
    keep[bad] = False
    off = case.offsets - np.concatenate([[0], np.cumsum(~keep)])[case.offsets]
    clean = E.Case("clean", case.rows, case.B, case.indices[keep], off)
    assert clean.flag == 0
    for w in (None, psw):
        a = R.ref_lookup(case, f, D, table, w)
        b = R.ref_lookup(clean, f, D, table, None if w is None else w[keep])
        assert (_bits(a) == _bits(b)).all()
    assert (psw == 0).sum() > 5 and (psw == -1).sum() > 5
    assert ((psw != 0) & (np.abs(psw) < np.finfo(np.float32).tiny)).sum() == 1
    m = np.abs(psw[(psw != 0) & (np.abs(psw) >= 0.125)]).view(np.int32) & 0xFF
    assert np.unique(m).size > 100  # full mantissas: the low byte takes every value


def test_grid_stride_case():
    case, table, psw = R.grid_stride_case(4, R.Q8, 8192 * 4 * 16 + 5, seed=2)
    assert case.T == 1 and case.B > 8192 * 4 * (64 // R.lane_geom(1)[0])
    assert set(np.unique(case.bag_len)) == {0, 1, 2} and case.flag == 0
    out = R.ref_lookup(case, R.Q8, 4, table, psw)
    assert out.shape == (case.B, 1, 4) and np.isfinite(out).all()
    assert (out[case.bag_len == 0] == 0).all()
