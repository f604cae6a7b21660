"""Host refusals of the embedding entry points, through dlrm_hip._lib.call with fake non-null
pointers: every case here returns from the library before any HIP call, so it runs without a
GPU.  Table-driven: one argument order per entry point, one set of valid values, and each case
changes the one or two values its refusal is about.  Asserted: the status code, and that the
message carries the entry point's own name."""
import ctypes

import pytest

from dlrm_hip import _lib

INVALID_ARG, UNSUPPORTED, WORKSPACE = 1, 3, 4
PTR = 0x10000  # fake device pointer, 64 KiB aligned; never dereferenced on the host
ROLE_MAGIC = 0x7B3E0001  # tbe_bwd_roles.hpp kRoleMagic

_CSR = "D row_base T B indices index_bits offsets offset_bits N total_rows psw"
_TAIL = "mx ws ws_bytes err presorted stream"
_UPD = _CSR + " grad gbs "
BACKWARD = {
    "dlrm_tbe_backward_sgd": "weights " + _UPD + "lr " + _TAIL,
    "dlrm_tbe_backward_sgd_dev": "weights " + _UPD + "lr_dev " + _TAIL,
    "dlrm_tbe_backward_sgd_f16": "weights " + _UPD + "lr " + _TAIL,
    "dlrm_tbe_backward_sgd_f16_dev": "weights " + _UPD + "lr_dev " + _TAIL,
    "dlrm_tbe_backward_sgd_f16_sr": "weights " + _UPD + "lr lr_null sr_state " + _TAIL,
    "dlrm_tbe_backward_rowwise_adagrad": "weights momentum " + _UPD + "lr eps " + _TAIL,
    "dlrm_tbe_backward_rowwise_adagrad_dev": "weights momentum " + _UPD + "lr_dev eps " + _TAIL,
    "dlrm_tbe_backward_adagrad": "weights momentum " + _UPD + "lr lr_null eps " + _TAIL,
    "dlrm_tbe_backward_dense": "weights " + _UPD + _TAIL,
    "dlrm_tbe_backward_sort": _CSR + " mx ws ws_bytes err stream",
    "dlrm_tbe_backward_defer": "mode weights momentum " + _UPD + "lr eps "
                               + _TAIL.replace("stream", "role stream"),
    "dlrm_tbe_backward_defer_dev": "mode weights momentum " + _UPD + "lr_dev eps "
                                   + _TAIL.replace("stream", "role stream"),
}
DEFER = ("dlrm_tbe_backward_defer", "dlrm_tbe_backward_defer_dev")


def _valid(D=8, T=2, B=3, N=6, total_rows=100):
    need = _lib.query("dlrm_tbe_backward_workspace_size", N, total_rows, D)
    return dict(weights=PTR, momentum=PTR, D=D, row_base=PTR, T=T, B=B, indices=PTR,
                index_bits=32, offsets=PTR, offset_bits=64, N=N, total_rows=total_rows, psw=None,
                grad=PTR, gbs=T * D, lr=0.1, lr_dev=PTR, lr_null=None, sr_state=PTR, eps=1e-8,
                mx=0, ws=PTR, ws_bytes=need, err=None, presorted=0, stream=None, mode=1)


def _role():
    """A role that reads as live (every word the magic, so dlrm_role_blocks != 0)."""
    role = _lib.LaunchRole()
    ctypes.memmove(ctypes.byref(role), (ctypes.c_uint32 * 64)(*([ROLE_MAGIC] * 64)), 256)
    assert _lib.query("dlrm_role_blocks", ctypes.byref(role)) != 0
    return role


def _call(name, order, **change):
    vals = _valid(**{k: change.pop(k) for k in ("D", "N", "total_rows") if k in change})
    role = _role()
    vals["role"] = ctypes.byref(role)
    vals.update(change)
    _lib.call(name, *[vals[k] for k in order.split()])
    return role


def _refused(name, order, code, *words, **change):
    with pytest.raises(_lib.DLRMHipError) as e:
        _call(name, order, **change)
    assert e.value.code == code, str(e.value)
    msg = str(e.value).split(": ", 2)[2]  # "<fn> failed (status n): <STATUS>: <library message>"
    for w in (name,) + words:
        assert w in msg, (w, msg)


# Refusals every backward entry point shares (bwd_dispatch and the workspace check).
SHARED = [
    ("index_bits", INVALID_ARG, ("index_bits must be 32 or 64",), dict(index_bits=16)),
    ("offset_bits", INVALID_ARG, ("offset_bits must be 32 or 64",), dict(offset_bits=8)),
    ("presorted", INVALID_ARG, ("bad presorted 3",), dict(presorted=3)),
    ("grad_stride", INVALID_ARG, ("grad_batch_stride < T*D",), dict(gbs=15)),
    ("rows_2^32-1", UNSUPPORTED, ("rows in one call",), dict(total_rows=2**32 - 1)),
    ("workspace", WORKSPACE, ("workspace",), "one byte short"),
    ("null_row_base", INVALID_ARG, ("null pointer",), dict(row_base=None)),
]


@pytest.mark.parametrize("name", list(BACKWARD))
@pytest.mark.parametrize("case", SHARED, ids=[c[0] for c in SHARED])
def test_backward_shared_refusals(name, case):
    _, code, words, change = case
    order = BACKWARD[name]
    if change == "one byte short":
        change = dict(ws_bytes=_valid()["ws_bytes"] - 1)
    if not set(change) <= set(order.split()) | {"total_rows"}:
        return  # dlrm_tbe_backward_sort takes no gradient and no presorted
    _refused(name, order, code, *words, **change)


# Each entry point's own checks (the ones it makes before the shared ones).
OWN = [
    ("dlrm_tbe_backward_sgd", "null pointer", dict(weights=None)),
    ("dlrm_tbe_backward_sgd_dev", "null lr_dev", dict(lr_dev=None)),
    ("dlrm_tbe_backward_sgd_f16", "null pointer", dict(grad=None)),
    ("dlrm_tbe_backward_sgd_f16_dev", "null lr_dev", dict(lr_dev=None)),
    ("dlrm_tbe_backward_sgd_f16_sr", "sr_state must be an 8-byte aligned", dict(sr_state=None)),
    ("dlrm_tbe_backward_sgd_f16_sr", "sr_state must be an 8-byte aligned",
     dict(sr_state=PTR + 4)),
    ("dlrm_tbe_backward_rowwise_adagrad", "null momentum", dict(momentum=None)),
    ("dlrm_tbe_backward_rowwise_adagrad_dev", "null momentum or lr_dev", dict(momentum=None)),
    ("dlrm_tbe_backward_rowwise_adagrad_dev", "null momentum or lr_dev", dict(lr_dev=None)),
    ("dlrm_tbe_backward_adagrad", "null state_sum", dict(momentum=None)),
    ("dlrm_tbe_backward_dense", "null pointer", dict(weights=None)),
    ("dlrm_tbe_backward_sort", "null pointer", dict(indices=None)),
    ("dlrm_tbe_backward_defer", "null role", dict(role=None)),
    ("dlrm_tbe_backward_defer", "mode must be 0 (sgd) or 1 (rowwise adagrad)", dict(mode=2)),
    ("dlrm_tbe_backward_defer", "rowwise adagrad needs momentum", dict(momentum=None)),
    ("dlrm_tbe_backward_defer_dev", "null lr_dev", dict(lr_dev=None)),
    ("dlrm_tbe_backward_defer_dev", "null role", dict(role=None)),
    ("dlrm_tbe_backward_defer_dev", "mode must be 0 (sgd) or 1 (rowwise adagrad)",
     dict(mode=-1)),
    ("dlrm_tbe_backward_defer_dev", "rowwise adagrad needs momentum", dict(momentum=None)),
]


@pytest.mark.parametrize("name,word,change", OWN,
                         ids=[f"{n[9:]}-{next(iter(c))}" for n, _, c in OWN])
def test_backward_own_checks(name, word, change):
    _refused(name, BACKWARD[name], INVALID_ARG, word, **change)


@pytest.mark.parametrize("name", list(BACKWARD))
def test_no_lookups_is_ok(name):
    """N == 0 returns OK with no workspace at all; a deferred call leaves an empty role."""
    role = _call(name, BACKWARD[name], N=0, indices=None, offsets=None, ws=None, ws_bytes=0)
    if name in DEFER:
        assert _lib.query("dlrm_role_blocks", ctypes.byref(role)) == 0


@pytest.mark.parametrize("name", DEFER)
def test_a_refused_deferred_call_leaves_an_empty_role(name):
    role = _role()
    vals = dict(_valid(), role=ctypes.byref(role), index_bits=16)
    with pytest.raises(_lib.DLRMHipError):
        _lib.call(name, *[vals[k] for k in BACKWARD[name].split()])
    assert _lib.query("dlrm_role_blocks", ctypes.byref(role)) == 0


@pytest.mark.parametrize("name", [n for n in BACKWARD if n != "dlrm_tbe_backward_sort"])
def test_d_2052_is_refused_before_the_sort(name):
    """D = 2052 is 513 float4 chunks, nine per lane of a 64-lane group: the update's kernels
    hold at most eight.  The geometry is computed before the first launch, so the refusal
    needs no device; the workspace is correctly sized."""
    _refused(name, BACKWARD[name], UNSUPPORTED, "D=2052 too large", D=2052)


# ------------------------------------------------- the other embedding entry points --
FORWARD = "weights D row_base T B indices index_bits offsets offset_bits psw out obs err stream"
ROWS = ("weights fmt row_bytes D row_base T B indices index_bits offsets offset_bits psw out "
        "obs err stream")
PRESORT = ("weights D row_base T B indices index_bits offsets offset_bits psw out obs N "
           "total_rows mx ws ws_bytes err bottom stream")
PSW_GRAD = ("weights D row_base T B indices index_bits offsets offset_bits N grad gbs gpsw "
            "stream")
QR_EXPAND = ("T B indices index_bits offsets offset_bits src kind coll mx pidx poff cap err "
             "stream")
QUANTIZE = "src src_fmt rows D dst_fmt dst dst_row_bytes stream"
F32, F16, Q8, Q4 = 0, 1, 2, 3

OTHERS = [
    ("dlrm_tbe_forward", FORWARD, INVALID_ARG, "index_bits must be 32|64", dict(index_bits=0)),
    ("dlrm_tbe_forward", FORWARD, INVALID_ARG, "offset_bits must be 32|64",
     dict(offset_bits=16)),
    ("dlrm_tbe_forward", FORWARD, INVALID_ARG, "out_batch_stride < T*D", dict(obs=15)),
    ("dlrm_tbe_forward", FORWARD, INVALID_ARG, "null pointer", dict(out=None)),
    ("dlrm_tbe_forward", FORWARD, INVALID_ARG, "bad sizes", dict(T=0)),
    # (this message names the entry point without its prefix)
    ("tbe_forward", FORWARD, UNSUPPORTED, "D=2052 too large", dict(D=2052, obs=2 * 2052)),
    ("dlrm_tbe_forward_rows", ROWS, INVALID_ARG, "index_bits must be 32|64",
     dict(index_bits=8)),
    ("dlrm_tbe_forward_rows", ROWS, INVALID_ARG, "offset_bits must be 32|64",
     dict(offset_bits=0)),
    ("dlrm_tbe_forward_rows", ROWS, INVALID_ARG, "bad row format 0", dict(fmt=F32)),
    ("dlrm_tbe_forward_rows", ROWS, INVALID_ARG, "row_bytes 15 < 16", dict(row_bytes=15)),
    ("dlrm_tbe_forward_rows", ROWS, INVALID_ARG, "out_batch_stride < T*D", dict(obs=15)),
    ("dlrm_tbe_forward_rows", ROWS, UNSUPPORTED, "multiple of 4 and <= 512 (D=516)",
     dict(D=516, row_bytes=524, obs=2 * 516)),
    ("dlrm_tbe_forward_rows", ROWS, UNSUPPORTED, "multiple of 4 and <= 512 (D=6)",
     dict(D=6, obs=12)),
    ("dlrm_tbe_forward_rows", ROWS, UNSUPPORTED, "misaligned rows or output",
     dict(weights=PTR + 2)),
    ("dlrm_tbe_forward_presort", PRESORT, UNSUPPORTED, "out = NULL needs the per-table sort",
     dict(out=None, mx=0)),
    ("dlrm_tbe_forward_presort", PRESORT, UNSUPPORTED, "out = NULL needs the per-table sort",
     dict(out=None, mx=4097)),
    ("dlrm_tbe_forward_presort", PRESORT, INVALID_ARG, "index_bits must be 32|64",
     dict(index_bits=16)),
    ("dlrm_tbe_forward_presort", PRESORT, INVALID_ARG, "offset_bits must be 32|64",
     dict(offset_bits=16)),
    ("dlrm_tbe_forward_presort", PRESORT, INVALID_ARG, "out_batch_stride < T*D", dict(obs=15)),
    ("dlrm_tbe_forward_presort", PRESORT, INVALID_ARG, "null workspace", dict(ws=None)),
    ("dlrm_tbe_forward_presort", PRESORT, WORKSPACE, "workspace", "one byte short"),
    ("dlrm_tbe_forward_presort", PRESORT, UNSUPPORTED, "D=2052 too large",
     dict(D=2052, obs=2 * 2052)),
    # no sort and no bottom MLP: the plain lookup's checks, under the lookup's name
    ("dlrm_tbe_forward", PRESORT, INVALID_ARG, "index_bits must be 32|64",
     dict(mx=0, index_bits=16)),
    ("dlrm_tbe_psw_grad", PSW_GRAD, INVALID_ARG, "bad index_bits", dict(index_bits=16)),
    ("dlrm_tbe_psw_grad", PSW_GRAD, INVALID_ARG, "bad offset_bits", dict(offset_bits=16)),
    ("dlrm_tbe_psw_grad", PSW_GRAD, INVALID_ARG, "grad_batch_stride < T*D", dict(gbs=15)),
    ("dlrm_tbe_psw_grad", PSW_GRAD, INVALID_ARG, "null pointer", dict(gpsw=None)),
    ("dlrm_qr_expand_csr", QR_EXPAND, INVALID_ARG, "bad index_bits", dict(index_bits=16)),
    ("dlrm_qr_expand_csr", QR_EXPAND, INVALID_ARG, "bad offset_bits", dict(offset_bits=16)),
    ("dlrm_qr_expand_csr", QR_EXPAND, INVALID_ARG, "null pointer", dict(coll=None)),
    ("dlrm_qr_expand_csr", QR_EXPAND, INVALID_ARG, "bad sizes", dict(cap=-1)),
    ("dlrm_rows_quantize", QUANTIZE, INVALID_ARG, "source format 2 is not F32 | F16",
     dict(src_fmt=Q8)),
    ("dlrm_rows_quantize", QUANTIZE, INVALID_ARG, "destination format 1 is not Q8 | Q4",
     dict(dst_fmt=F16)),
    ("dlrm_rows_quantize", QUANTIZE, UNSUPPORTED, "multiple of 4 and <= 512 (D=516)",
     dict(D=516, dst_row_bytes=524)),
    ("dlrm_rows_quantize", QUANTIZE, INVALID_ARG, "dst_row_bytes 15 != 16",
     dict(dst_row_bytes=15)),
    ("dlrm_rows_quantize", QUANTIZE, INVALID_ARG, "null pointer", dict(dst=None)),
    ("dlrm_rows_quantize", QUANTIZE, UNSUPPORTED, "misaligned source or destination",
     dict(src=PTR + 8)),
]


def _other_valid():
    v = _valid()
    v.update(out=PTR, obs=16, fmt=Q8, row_bytes=16, mx=10, bottom=None, gpsw=PTR, src=PTR,
             kind=PTR, coll=PTR, pidx=PTR, poff=PTR, cap=64, src_fmt=F32, dst_fmt=Q8, dst=PTR,
             dst_row_bytes=16, rows=5)
    return v


@pytest.mark.parametrize("name,order,code,word,change", OTHERS,
                         ids=[f"{o[0]}-{o[3][:24].replace(' ', '_')}-{i}"
                              for i, o in enumerate(OTHERS)])
def test_other_entry_points(name, order, code, word, change):
    vals = _other_valid()
    if change == "one byte short":
        change = dict(ws_bytes=vals["ws_bytes"] - 1)
    if "D" in change:
        vals["ws_bytes"] = _lib.query("dlrm_tbe_backward_workspace_size", vals["N"],
                                      vals["total_rows"], change["D"])
    vals.update(change)
    entry = {FORWARD: "dlrm_tbe_forward", ROWS: "dlrm_tbe_forward_rows",
             PRESORT: "dlrm_tbe_forward_presort", PSW_GRAD: "dlrm_tbe_psw_grad",
             QR_EXPAND: "dlrm_qr_expand_csr", QUANTIZE: "dlrm_rows_quantize"}[order]
    with pytest.raises(_lib.DLRMHipError) as e:
        _lib.call(entry, *[vals[k] for k in order.split()])
    assert e.value.code == code, str(e.value)
    msg = str(e.value).split(": ", 2)[2]
    assert name in msg and word in msg, msg


def test_empty_calls_are_ok():
    v = _other_valid()
    for order, entry, change in (
            (PSW_GRAD, "dlrm_tbe_psw_grad", dict(N=0, indices=None, gpsw=None)),
            (ROWS, "dlrm_tbe_forward_rows", dict(B=0)),
            (QUANTIZE, "dlrm_rows_quantize", dict(rows=0, src=None, dst=None))):
        vals = dict(v, **change)
        _lib.call(entry, *[vals[k] for k in order.split()])
