"""dlrm_tbe_forward_rows (the pooled lookup over F16 / Q8 / Q4 rows, csrc/tbe_rows.hip) held
BIT FOR BIT to the rule its file header states, restated on the host by
tests/exact_rows_lookup.ref_lookup (itself bitwise torch's two quantized lookups:
tests/test_exact_rows_lookup_cpu.py):

    acc = fma(w*scale, q, acc + w*bias)   per valid lookup, in bag order  (F16: fma(w, v, acc))

There is no tolerance in this file.  The bag lengths straddle every lane group (so the l0
loop takes a second and a fifth trip), the per-sample weights carry full mantissas, zeros,
-1 and a subnormal, row 0 of every table and every unnamed row are 0xFF bytes (NaN scale,
bias or halves: a row multiplied by zero instead of dropped shows as NaN), the output sits in
a sentinel buffer with a padded batch stride and the error flag must hold exactly the expected
bits.  DESIGN.md ("Exact-arithmetic coverage of the embedding side") says which case reaches
which LPB / MAXV rung."""
import functools

import numpy as np
import pytest
import torch

import exact_rows_lookup as R
import exact_tbe as E
from exact_inputs import SENTINEL, padded, pads_intact

pytestmark = pytest.mark.gpu

dev = "cuda:0"
FMTS = ["f16", "q8", "q4"]
# LPB 4, 4, 8, 16, 32, a ragged 64 (50 chunks), a full 64, MAXV = 2 with a ragged second
# chunk (65 chunks) and with a full one
DIMS = [4, 16, 20, 64, 128, 200, 256, 260, 512]


@pytest.fixture(scope="module")
def ops():
    from dlrm_hip import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def _case(fmt, D, invalid, pair):
    """(case, table, psw) of (format, D): built once, shared, never changed."""
    return R.lookup_case(D, R.FMTS[fmt], seed=R.case_seed(R.FMTS[fmt], D), invalid=invalid,
                         pair=E.IDX_PAIRS[pair])


@functools.lru_cache(maxsize=None)
def _ref(fmt, D, invalid, pair, weighted):
    case, table, psw = _case(fmt, D, invalid, pair)
    ref = R.ref_lookup(case, R.FMTS[fmt], D, table, psw if weighted else None)
    assert np.isfinite(ref).all()
    return torch.from_numpy(ref)


def _dev_table(table, pitch=None):
    """The table on the device; ``pitch`` (bytes): as a strided view of a 0xFF-filled buffer
    of that row pitch."""
    t = torch.from_numpy(table)
    if pitch is None:
        return t.to(dev)
    per = pitch // t.element_size()
    assert per * t.element_size() == pitch and per > t.shape[1]
    buf = torch.full((t.shape[0] + 1, pitch), 0xFF, dtype=torch.uint8, device=dev)
    view = buf.view(t.dtype)[:t.shape[0], :t.shape[1]]
    view.copy_(t)
    assert view.stride(0) == per
    return view


def _lookup(ops, case, fmt, D, W, psw, weighted):
    """One launch into a sentinel buffer (out_batch_stride = T*D + 4, two guard rows):
    (fp32 [B, T, D] on the host, the error flag)."""
    idx, off, rb = case.device_csr(dev)
    out = padded(torch.full((case.B, case.T * D), SENTINEL, device=dev), 2, 4, SENTINEL)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.tbe_forward_rows(W, R.FMTS[fmt], D, rb, case.T, case.B, idx, off,
                         per_sample_weights=torch.from_numpy(psw).to(dev) if weighted else None,
                         out=out, out_batch_stride=case.T * D + 4, error_flag=err)
    torch.cuda.synchronize()
    assert pads_intact(out), "the lookup wrote outside its [B, T*D] view"
    return out.cpu().reshape(case.B, case.T, D), int(err.item())


def _where(case, got, ref):
    """The first differing bag, placed for the reader."""
    bad = np.argwhere((got.view(torch.int32) != ref.view(torch.int32)).any(2).numpy())
    if bad.size == 0:
        return "equal"
    b, t = (int(x) for x in bad[0])
    n = int(case.bag_len[t * case.B + b])
    d = int(np.flatnonzero((got[b, t].view(torch.int32) != ref[b, t].view(torch.int32)).numpy())[0])
    return (f"{len(bad)} bags differ; first: sample {b} table {t} ({n} lookups), column {d}: "
            f"got {got[b, t, d].item()!r} ref {ref[b, t, d].item()!r}")


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("fmt", FMTS)
def test_lookup_is_the_rule(ops, fmt, D):
    """Unweighted and weighted, without and with invalid indices (one past the table and -1,
    each deep inside a long bag), the four index / offset dtype pairs in turn."""
    n = 0
    for weighted in (False, True):
        for invalid in (False, True):
            pair = n % 4
            n += 1
            case, table, psw = _case(fmt, D, invalid, pair)
            ref = _ref(fmt, D, invalid, pair, weighted)
            got, flag = _lookup(ops, case, fmt, D, _dev_table(table), psw, weighted)
            what = (fmt, D, weighted, invalid, E.IDX_PAIRS[pair])
            assert E.bits_equal(got, ref), (what, _where(case, got, ref))
            assert flag == case.flag == (ops.TBE_ERR_INDEX if invalid else 0), what


@pytest.mark.parametrize("fmt", FMTS)
def test_lookup_row_pitch(ops, fmt):
    """A row pitch above the minimum (the rows a strided view of a 0xFF-filled buffer): the
    bits of the tight-pitch run, and the rule's."""
    for D in (64, {"f16": 20, "q8": 200, "q4": 260}[fmt]):
        pitch = {"q8": D + 12, "q4": D // 2 + 6, "f16": 2 * (D + 4)}[fmt]
        assert pitch > R.min_row_bytes(R.FMTS[fmt], D)
        case, table, psw = _case(fmt, D, True, 3)
        W = _dev_table(table, pitch)
        assert (W.stride(0) * W.element_size(), W.shape[1] * W.element_size()) == \
            (pitch, R.min_row_bytes(R.FMTS[fmt], D))
        for weighted in (False, True):
            tight, f0 = _lookup(ops, case, fmt, D, _dev_table(table), psw, weighted)
            wide, f1 = _lookup(ops, case, fmt, D, W, psw, weighted)
            ref = _ref(fmt, D, True, 3, weighted)
            assert E.bits_equal(wide, tight), (D, weighted, _where(case, wide, tight))
            assert E.bits_equal(wide, ref), (D, weighted, _where(case, wide, ref))
            assert f0 == f1 == ops.TBE_ERR_INDEX


@pytest.mark.parametrize("fmt,D,B", [("q8", 4, 8192 * 4 * 16 + 5), ("q4", 256, 8192 * 4 + 5)])
def test_lookup_grid_stride(ops, fmt, D, B):
    """More bags than the 8192 capped workgroups hold (4 waves of 64 / LPB bags each), so the
    grid-stride loop takes a second trip: every bag against the rule."""
    f = R.FMTS[fmt]
    assert B == 8192 * 4 * (64 // R.lane_geom(D // 4)[0]) + 5
    case, table, psw = R.grid_stride_case(D, f, B, seed=D)
    ref = torch.from_numpy(R.ref_lookup(case, f, D, table, psw))
    got, flag = _lookup(ops, case, fmt, D, _dev_table(table), psw, True)
    assert E.bits_equal(got, ref), _where(case, got, ref)
    assert flag == 0


@pytest.mark.parametrize("fmt", FMTS)
def test_lookup_is_deterministic(ops, fmt):
    D = 128
    case, table, psw = _case(fmt, D, True, 0)
    W = _dev_table(table)
    a, _ = _lookup(ops, case, fmt, D, W, psw, True)
    b, _ = _lookup(ops, case, fmt, D, W, psw, True)
    assert E.bits_equal(a, b)
