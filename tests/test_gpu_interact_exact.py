"""Exact-arithmetic tests of every branch of the dot interaction's launch ladder (csrc/
interact.hip): each kernel against the fp64 reference of tests/exact_interact.py, bit for bit
(torch.equal), on integer cases and on full-mantissa cases, at every template the library
instantiates, every output / gradient / feature layout, every waves-per-workgroup class of
the runtime-D kernels, the elementwise kernels, every grid-stride cap, the gather modes with
invalid indices, the cat interaction, and the refusals.  Inputs sit in NaN-filled buffers,
outputs in sentinel-filled ones with guard rows; the whole buffer outside the view must keep
its fill.  Which kernel a shape runs is asserted with exact_interact's restatement of the
ladder; test_exact_interact_cpu.py proves the cases and the plans on the CPU."""
import functools

import pytest
import torch

import exact_interact as X
from exact_inputs import SENTINEL

pytestmark = pytest.mark.gpu

dev = "cuda:0"
NAN = float("nan")
BITS = {3: 8, 4: 4}  # gather mode -> width of the packed levels


@pytest.fixture(scope="module")
def ops():
    from dlrm_hip import ops as _ops
    return _ops


class Buf:
    """A [rows, width] view (row stride ld) that starts ``off`` floats into a flat buffer
    filled with ``fill``, with two guard rows behind it; ``data`` is copied into the view."""

    def __init__(self, rows, width, ld, off=0, fill=SENTINEL, data=None, dtype=torch.float32):
        self.geom = ((rows, width), (ld, 1), off)
        self.fill = fill
        self.flat = torch.full((off + (rows + 2) * ld + 4,), fill, dtype=dtype, device=dev)
        self.view = self.flat.as_strided(*self.geom)
        if data is not None:
            self.view.copy_(data)

    def untouched(self):
        """Everything outside the view still holds the fill, bitwise."""
        c = self.flat.clone()
        c.as_strided(*self.geom).fill_(self.fill)
        want = torch.full_like(c, self.fill)
        return torch.equal(c.view(torch.int32), want.view(torch.int32))


def _pad4(n):
    return (n + 3) // 4 * 4


def row_layout(width, kind):
    """(ld, off) of an output or grad_out row layout: 'vec' 16-byte-aligned rows (the float4
    path; its scalar tail runs when width % 4 != 0), 'odd' an odd row stride, 'off1' the base
    one float off."""
    return {"vec": (_pad4(width) + 4, 0), "odd": ((width + 4) | 1, 0),
            "off1": (_pad4(width) + 4, 1)}[kind]


def _features(case, kind, fill=NAN, data=True):
    """(x, ly, buffers) in a feature layout: 'btd' [B, T, D] with a padded batch stride,
    'list' one tensor per feature with pairwise different batch strides (list_strides),
    'off1' the 'btd' layout one float off (not 16-byte aligned).  ``data`` False: empty
    gradient buffers of that layout."""
    B, F, D = case.B, case.F, case.D
    T = F - 1
    off = 1 if kind == "off1" else 0
    if kind == "list":
        bufs = [Buf(B, D, s, 0, fill) for s in X.list_strides(F, D)]
        if data:
            bufs[0].view.copy_(case.x)
            for t in range(T):
                bufs[t + 1].view.copy_(case.ly[:, t])
        return bufs[0].view, [b.view for b in bufs[1:]], bufs
    bx = Buf(B, D, D + 4, off, fill, case.x if data else None)
    if T == 0:
        return bx.view, [], [bx]
    bl = Buf(B, T * D, T * D + 4, off, fill, case.ly.reshape(B, T * D) if data else None)
    return bx.view, bl.view.view(B, T, D), [bx, bl]


@functools.lru_cache(maxsize=None)
def _ref(case, relu_x):
    return {k: v.to(dev) for k, v in X.reference(case, relu_x).items()}


def _first_diff(got, ref):
    bad = (got != ref).nonzero()
    if bad.numel() == 0:
        return None
    i = tuple(bad[0].tolist())
    return i, float(got[i]), float(ref[i]), int(bad.shape[0])


def _check(buf, ref, what):
    assert torch.equal(buf.view, ref), (what, _first_diff(buf.view, ref))
    assert buf.untouched(), (what, "wrote outside its rows")


def _check_grads(case, relu_x, gx, gly, gbufs, what):
    ref = _ref(case, relu_x)
    assert torch.equal(gx, ref["gx"]), (what, "gx", _first_diff(gx, ref["gx"]))
    if case.F > 1:
        g = torch.stack(list(gly), 1) if isinstance(gly, (list, tuple)) else gly
        assert torch.equal(g, ref["gly"]), (what, "gly", _first_diff(g, ref["gly"]))
    for b in gbufs:
        assert b.untouched(), (what, "wrote outside its rows")


def run_pooled(ops, case, relu_x, fwd=X.FWD_FORCED, bwd=X.BWD_FORCED, out="vec", feat="btd",
               grad=None, what=()):
    """The pooled entry points under each forced version, against the reference."""
    x, ly, _ = _features(case, feat)
    ld, off = row_layout(case.width, out)
    for v in fwd:
        o = Buf(case.B, case.width, ld, off)
        with ops.tuning(interact_fwd=v):
            ops.interact_forward("dot", x, ly, case.self_int, out=o.view)
        _check(o, _ref(case, relu_x)["R"], (what, "fwd", v))
    dR = Buf(case.B, case.width, ld, off, NAN, case.dR)
    for v in bwd:
        gx, gly, gbufs = _features(case, grad or feat, SENTINEL, data=False)
        with ops.tuning(interact_bwd=v):
            ops.interact_backward("dot", x, ly, dR.view, case.self_int, grad_x=gx, grad_ly=gly,
                                  relu_x=relu_x)
        _check_grads(case, relu_x, gx, gly, gbufs, (what, "bwd", v))


def _table(case, mode):
    """The table as gather mode ``mode`` reads it, NaN (0xFF bytes) behind its last row."""
    rows, D = case.W.shape
    if mode == 1:
        return Buf(rows, D, D, 0, NAN, case.W).view
    if mode == 2:
        w16 = case.W.half()
        assert torch.equal(w16.float(), case.W)
        return Buf(rows, D, D, 0, NAN, w16, dtype=torch.float16).view
    packed = torch.from_numpy(X.pack_int_rows(case.W, BITS[mode]))
    buf = torch.full((rows + 2, packed.shape[1]), 0xFF, dtype=torch.uint8, device=dev)
    buf[:rows] = packed.to(dev)
    return buf[:rows]


def run_gather(ops, case, relu_x, mode, fwd=X.FWD_FORCED, bwd=X.BWD_FORCED, out="vec", what=()):
    """The gather entry points of ``mode`` (1 fp32, 2 fp16, 3 Q8, 4 Q4 rows; the backward for 1
    and 2) under each forced version; x_bstride = D + 4; the flag is exactly the case's."""
    B, D, T = case.B, case.D, case.F - 1
    x = Buf(B, D, D + 4, 0, NAN, case.x).view
    W = _table(case, mode)
    rb = torch.from_numpy(case.row_base).to(dev)
    idx = case.idx.to(torch.int32).reshape(-1).to(dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ld, off = row_layout(case.width, out)
    for v in fwd:
        o = Buf(B, case.width, ld, off)
        err.zero_()
        with ops.tuning(interact_fwd=v):
            if mode >= 3:
                ops.interact_forward_gather_rows(x, W, ops.ROWS_Q8 if mode == 3 else ops.ROWS_Q4,
                                                 D, rb, idx, case.self_int, out=o.view,
                                                 error_flag=err)
            else:
                ops.interact_forward_gather(x, W, rb, idx, case.self_int, out=o.view,
                                            error_flag=err)
        _check(o, _ref(case, relu_x)["R"], (what, "gather fwd", mode, v))
        assert int(err.item()) == case.flag, (what, "flag", mode, v)
    if mode > 2:
        return
    dR = Buf(B, case.width, ld, off, NAN, case.dR)
    for v in bwd:
        gx = Buf(B, D, D + 4)
        gl = Buf(B, T * D, T * D + 4)
        with ops.tuning(interact_bwd=v):
            ops.interact_backward_gather(x, W, rb, idx, dR.view, case.self_int, grad_x=gx.view,
                                         grad_ly=gl.view.view(B, T, D), relu_x=relu_x)
        _check_grads(case, relu_x, gx.view, gl.view.view(B, T, D), (gx, gl),
                     (what, "gather bwd", mode, v))


# ------------------------------------------------------------------ 1. staged --
@pytest.mark.parametrize("entry", X.staged_plan(), ids=lambda e: "D%d-F%d-s%d-B%d-r%d-g%d" % e)
def test_staged_every_template(ops, entry):
    """Every (kernel version, D, GATHER) interact.hip instantiates (the plan's coverage is
    asserted in test_exact_interact_cpu.py): the pooled entry points under every forced forward
    (4 / 5 / 0) and backward (3 / 4 / 5 / 0) version, and the entry's gather mode next to them."""
    D, F, self_int, B, relu_x, gather = entry
    assert X.fwd_kernel(B, F, D)[0] in ("v4", "v5") and X.bwd_kernel(B, F, D)[0] != "mfma"
    run_pooled(ops, X.int_case(B, F, D, self_int), relu_x, what=entry)
    if gather:
        run_gather(ops, X.gather_case(B, F, D, self_int), relu_x, gather, what=entry)


def test_staged_plan_is_complete():
    assert X.templates_of(X.staged_plan()) == X.instantiated_templates()


# ----------------------------------------------------------------- 2. layouts --
@pytest.mark.parametrize("D", X.STAGED_D)
def test_output_and_grad_out_layouts(ops, D):
    """R and grad_out rows in the four layouts, under every staged version: 16-byte-aligned
    rows whose width has a tail of width % 4 floats (the loop behind the float4 loop), the same
    without a tail, an odd row stride, and a base one float off (both scalar paths)."""
    for shape, layouts in (("tail", X.OUT_LAYOUTS), ("no tail", ("vec",))):
        F, self_int = X.LAYOUT_SHAPES[shape]
        case = X.int_case(5, F, D, self_int)
        assert (case.width % 4 != 0) == (shape == "tail")
        for k, out in enumerate(layouts):
            run_pooled(ops, case, k % 2 == 0, out=out, what=(shape, out))
            if out != "vec" or shape == "tail":
                g = X.gather_case(5, F, D, self_int)
                run_gather(ops, g, k % 2 == 1, 1 + k % 2, out=out, what=(shape, out))


# --------------------------------------------------------- 3. feature layouts --
@pytest.mark.parametrize("D", X.STAGED_D)
def test_feature_and_gradient_layouts(ops, D):
    """[B, T, D] with a padded batch stride is every other test's layout; here a list whose
    tensors have pairwise different batch strides (features and gradient rows), features one
    float off (the runtime-D kernels), and aligned features with gradient rows one float off
    (the fall-through to the runtime-D backward plus relu_mask_kernel)."""
    for F, self_int, B in ((9, False, 5), (32, True, 3), (1, True, 3)):
        case = X.int_case(B, F, D, self_int)
        strides = X.list_strides(F, D)
        assert len(set(strides)) == F and min(strides) == strides[0] == D
        for relu_x in (True, False):
            run_pooled(ops, case, relu_x, feat="list", what=("list", F, relu_x))
            assert X.fwd_kernel(B, F, D, aligned=False)[0] == "mfma"
            run_pooled(ops, case, relu_x, fwd=(0,), bwd=(0,), feat="off1",
                       what=("features off1", F, relu_x))
            assert X.bwd_kernel(B, F, D, grads_aligned=False)[0] == "mfma"
            run_pooled(ops, case, relu_x, fwd=(), bwd=(0, 3), feat="btd", grad="off1",
                       what=("gradient rows off1", F, relu_x))


# --------------------------------------------------------------- 4. runtime-D --
@pytest.mark.parametrize("D", X.RUNTIME_D)
def test_runtime_d_every_wave_class(ops, D):
    """The runtime-D MFMA kernels at 4, 2 and 1 waves per workgroup and their fall-through to
    the elementwise kernels at 0 (F = 32), odd D (the k < D guard), D > 64 (a second trip of
    the lane loops); the classes are asserted over RUNTIME_D in test_exact_interact_cpu.py."""
    assert {X.fwd_waves(32, d) for d in X.RUNTIME_D} == {4, 2, 1, 0}
    assert {X.bwd_waves(32, d) for d in X.RUNTIME_D} == {4, 2, 1, 0}
    for F in (X.RUNTIME_SMALL_F, 32):
        assert X.fwd_kernel(3, F, D)[0] == ("mfma" if X.fwd_waves(F, D) else "generic")
        for k, B in enumerate((1, 3, 5)):
            case = X.int_case(B, F, D, (k + F) % 2 == 0)
            run_pooled(ops, case, k != 1, fwd=(0,), bwd=(0,), what=(F, B))


# ------------------------------------------------------------- 5. elementwise --
@pytest.mark.parametrize("F", X.ELEMENTWISE_F)
def test_elementwise_kernels(ops, F):
    """F > 32: pair_of's float sqrt and its correction loops at every triangular boundary up
    to p = 2079 (F = 64 with the diagonal)."""
    for self_int in (False, True):
        for D in (1, 8):
            assert X.fwd_kernel(3, F, D)[0] == X.bwd_kernel(3, F, D)[0] == "generic"
            run_pooled(ops, X.int_case(3, F, D, self_int), D == 8, fwd=(0,), bwd=(0,),
                       feat="list" if D == 8 else "btd", what=(F, self_int, D))


def _refused(ops, fn, bufs, what):
    from dlrm_hip._lib import DLRMHipError
    with pytest.raises(DLRMHipError):
        fn()
    torch.cuda.synchronize()
    for b in bufs:
        c = b.flat.view(torch.int32)
        assert torch.equal(c, torch.full_like(b.flat, b.fill).view(torch.int32)), what


def test_f65_is_refused(ops):
    B, F, D = 2, X.K_MAX_F + 1, 8
    feats = [Buf(B, D, D, 0, NAN, torch.ones(B, D)) for _ in range(F)]
    x, ly = feats[0].view, [b.view for b in feats[1:]]
    w = D + X.npairs(F, False)
    o, dR = Buf(B, w, w + 4), Buf(B, w, w + 4, 0, NAN, torch.ones(B, w))
    grads = [Buf(B, D, D) for _ in range(F)]
    _refused(ops, lambda: ops.interact_forward("dot", x, ly, False, out=o.view), [o], "fwd")
    _refused(ops, lambda: ops.interact_backward(
        "dot", x, ly, dR.view, False, grad_x=grads[0].view,
        grad_ly=[g.view for g in grads[1:]]), grads, "bwd")


# -------------------------------------------------------------------- 6. caps --
@pytest.mark.parametrize("what,side,forced,B,D", X.CAP_CASES, ids=[c[0] for c in X.CAP_CASES])
def test_grid_stride_caps(ops, what, side, forced, B, D):
    """Each grid cap crossed at the smallest shape (F = 2): some workgroup takes a second trip
    of its grid-stride loop, and the last group of four is partly filled."""
    kern = (X.fwd_kernel if side == "fwd" else X.bwd_kernel)(B, 2, D, forced)
    assert X.crosses_cap(kern) and B % 4 != 0, kern
    case = X.int_case(B, 2, D, False)
    run_pooled(ops, case, True, fwd=(forced,) if side == "fwd" else (),
               bwd=(forced,) if side == "bwd" else (), what=what)


@pytest.mark.parametrize("B", [X.V5_MAX_BATCH, X.V5_MAX_BATCH + 1])
def test_v5_batch_edge_unforced(ops, B):
    assert X.fwd_kernel(B, 2, 64)[0] == ("v5" if B <= X.V5_MAX_BATCH else "v4")
    assert X.bwd_kernel(B, 2, 64)[0] == ("v5" if B <= X.V5_MAX_BATCH else "v3")
    run_pooled(ops, X.int_case(B, 2, 64, True), True, fwd=(0,), bwd=(0,), what=B)


# ------------------------------------------------------------------ 7. gather --
@pytest.mark.parametrize("D", X.STAGED_D)
def test_gather_invalid_indices(ops, D):
    """An index of -1 or of ``rows`` (one past its table), in feature 1 or F - 1, in sample 0
    or in the last sample of a partly filled group of four: the forward's flag is exactly
    ERR_INDEX, R and every gradient are the zero-row reference's; fp32 and fp16 rows forward
    and backward, Q8 and Q4 rows forward.  Without an invalid index the flag stays 0 (asserted
    by run_gather against case.flag)."""
    B, F = 6, 9
    n = 0
    for value in (-1, "rows"):
        for f in (1, F - 1):
            for b in (0, B - 1):
                case = X.gather_case(B, F, D, n % 2 == 1, invalid=((value, f, b),))
                assert case.flag == X.ERR_INDEX and B % 4 != 0
                assert not bool(case.ly[b, f - 1].any())
                for mode in (1, 2, 3, 4):
                    run_gather(ops, case, n % 2 == 0, mode, what=(value, f, b))
                n += 1
    clean = X.gather_case(B, F, D, True)
    assert clean.flag == 0
    for mode in (1, 2, 3, 4):
        run_gather(ops, clean, True, mode, what="clean")


# ----------------------------------------------------------- 8. full mantissa --
def _run_fm(ops, kind, B, F, D, self_int, fwd, bwd, gather=False, what=()):
    case = X.fm_case(kind, B, F, D, self_int)
    fwd = fwd if kind == "fm_fwd" else ()
    bwd = () if kind == "fm_fwd" else bwd
    for relu_x in (True, False) if bwd else (False,):
        if gather:
            run_gather(ops, X.as_gather(case), relu_x, 1, fwd=fwd, bwd=bwd, what=(what, kind))
        else:
            run_pooled(ops, case, relu_x, fwd=fwd, bwd=bwd, what=(what, kind))


@pytest.mark.parametrize("kind", sorted(X.FM_OPERANDS))
@pytest.mark.parametrize("D", X.STAGED_D)
def test_full_mantissa_staged(ops, D, kind):
    """Every output one fp32 product of full-mantissa operands (exact_interact.fm_case): a
    bf16 or xf32 MFMA body, or a truncated operand, changes it.  Every staged version at every
    D, pooled and through the fp32 gather."""
    for F, self_int in ((9, True), (min(32, D), False)):
        _run_fm(ops, kind, 5, F, D, self_int, X.FWD_FORCED, X.BWD_FORCED, what=F)
        _run_fm(ops, kind, 5, F, D, not self_int, X.FWD_FORCED, X.BWD_FORCED, gather=True, what=F)


@pytest.mark.parametrize("kind", sorted(X.FM_OPERANDS))
@pytest.mark.parametrize("F,D", [(9, 13), (32, 100), (41, 64)])
def test_full_mantissa_runtime_d_and_elementwise(ops, F, D, kind):
    assert X.fwd_kernel(5, F, D)[0] == X.bwd_kernel(5, F, D)[0] == (
        "generic" if F > 32 else "mfma")
    for self_int in (False, True):
        _run_fm(ops, kind, 5, F, D, self_int, (0,), (0,), what=(F, D))


# --------------------------------------------------------------------- 9. cat --
def _cat_values(B, F, D):
    g = torch.Generator()
    g.manual_seed(B * 1000 + F * 10 + D)
    v = X.signed_fm((B, F, D), g)
    flat, n = v.view(-1), B * F * D
    flat[torch.tensor([0, n // 3, n // 2, n - 1])] = torch.tensor(
        [NAN, -0.0, 2.0 ** -140, -2.0 ** -149])
    return v


@pytest.mark.parametrize("F", [1, 27])
@pytest.mark.parametrize("D", [1, 5, 128])
def test_cat_forward_and_backward_are_copies(ops, F, D):
    """The cat interaction moves bits: full-mantissa values with a NaN, a -0.0 and denormals,
    compared as int32; strided ([B, T, D], padded batch stride) and list layouts."""
    B = 5
    v = _cat_values(B, F, D)
    assert bool(v.isnan().any()) and bool(((v != 0) & (v.abs() < 2.0 ** -126)).any())
    case = X.Case("cat", False, v[:, 0].contiguous(), v[:, 1:].contiguous(), None)
    R_ref = X.cat_ref(case.x, case.ly).to(dev)
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    for feat in ("btd", "list"):
        x, ly, _ = _features(case, feat)
        o = Buf(B, F * D, F * D + 3)
        ops.interact_forward("cat", x, ly, out=o.view)
        assert torch.equal(bits(o.view), bits(R_ref)), feat
        assert o.untouched(), feat
        dR = Buf(B, F * D, F * D + 3, 1, NAN, R_ref)
        gx, gly, gbufs = _features(case, feat, SENTINEL, data=False)
        ops.interact_backward("cat", x, ly, dR.view, grad_x=gx, grad_ly=gly)
        assert torch.equal(bits(gx), bits(case.x.to(dev))), feat
        if F > 1:
            g = torch.stack(list(gly), 1) if isinstance(gly, list) else gly
            assert torch.equal(bits(g), bits(case.ly.to(dev))), feat
        for b in gbufs:
            assert b.untouched(), feat


# --------------------------------------------------------------- 10. refusals --
def test_refusals_write_nothing(ops):
    case = X.gather_case(5, 9, 16, False)
    B, F, D, T = case.B, case.F, case.D, case.F - 1
    x, ly, _ = _features(case, "btd")
    rb = torch.from_numpy(case.row_base).to(dev)
    idx = case.idx.to(torch.int32).reshape(-1).to(dev)
    W = _table(case, 1)
    dR = Buf(B, case.width, case.width + 4, 0, NAN, case.dR)

    # ld_out one short of the width (rows overlap; nothing may be written)
    short = Buf(B, case.width, case.width + 4)
    view = short.flat.as_strided((B, case.width), (case.width - 1, 1))
    _refused(ops, lambda: ops.interact_forward("dot", x, ly, False, out=view), [short], "ld_out")
    _refused(ops, lambda: ops.interact_forward_gather(x, W, rb, idx, False, out=view), [short],
             "gather ld_out")

    def gather_fwd(xx, WW, rbb, idxx, width):
        o = Buf(xx.shape[0], width, width + 4)
        _refused(ops, lambda: ops.interact_forward_gather(xx, WW, rbb, idxx, False, out=o.view),
                 [o], "gather fwd")

    def gather_bwd(xx, WW, rbb, idxx, dRv, goff=0):
        b, d, t = xx.shape[0], xx.shape[1], rbb.numel() - 1
        gx, gl = Buf(b, d, d + 4, goff), Buf(b, t * d, t * d + 4, goff)
        _refused(ops, lambda: ops.interact_backward_gather(
            xx, WW, rbb, idxx, dRv, False, grad_x=gx.view, grad_ly=gl.view.view(b, t, d)),
            [gx, gl], "gather bwd")

    # D = 8: not a staged width
    c8 = X.gather_case(5, 9, 8, False)
    x8 = Buf(5, 8, 12, 0, NAN, c8.x).view
    i8 = c8.idx.to(torch.int32).reshape(-1).to(dev)
    rb8 = torch.from_numpy(c8.row_base).to(dev)
    dR8 = Buf(5, c8.width, c8.width + 4, 0, NAN, c8.dR)
    gather_fwd(x8, _table(c8, 1), rb8, i8, c8.width)
    gather_bwd(x8, _table(c8, 1), rb8, i8, dR8.view)
    # F = 33: past the gather kernels' 32 rows
    c33 = X.gather_case(2, 33, 16, False)
    x33 = Buf(2, 16, 20, 0, NAN, c33.x).view
    i33 = c33.idx.to(torch.int32).reshape(-1).to(dev)
    rb33 = torch.from_numpy(c33.row_base).to(dev)
    dR33 = Buf(2, c33.width, c33.width + 4, 0, NAN, c33.dR)
    gather_fwd(x33, _table(c33, 1), rb33, i33, c33.width)
    gather_bwd(x33, _table(c33, 1), rb33, i33, dR33.view)
    # a table one float off, and gradient rows one float off
    Wm = Buf(case.W.shape[0], D, D, 1, NAN, case.W).view
    gather_fwd(x, Wm, rb, idx, case.width)
    gather_bwd(x, Wm, rb, idx, dR.view)
    gather_bwd(x, W, rb, idx, dR.view, goff=1)
