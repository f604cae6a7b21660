"""Exact-arithmetic cases for the feature interaction (csrc/interact.hip): builders, the fp64
reference, the bug models a case must be able to show, and a restatement of the host's launch
ladder, so that a test can say which kernel a shape runs.

Reference (DLRM_Net.interact_features):
    forward   T = [x, ly] (F x D per sample), Z = T T^T, R = [x, Z[row-major lower triangle]]
              (strict, or with the diagonal under self interaction);
    backward  dT = (G + G^T) T with G the lower-triangular scatter of dR[D:], dR[:D] added to
              feature 0, ReLU'(x) as (x > 0) applied to it when relu_x is set;
    gather    feature f >= 1 of sample b is row row_base[f-1] + idx[f-1][b] of W; an index
              outside its table makes the row zero (its gradient row is what the formula gives
              for a zero row) and raises ERR_INDEX.
Everything is computed in float64 and rounded to fp32 once.  Two families of cases make that
the only correct fp32 answer (exact_inputs.py):
  * integers in [-3, 3]: the sum of |terms| of every output is below 2^24, so every partial
    sum in any order is exact;
  * full-mantissa: every output is ONE product of two fp32 values (or an exact zero), so a
    truncated or bf16-rounded operand changes it.
Plain helper module (no GPU needed), like exact_tbe.py and exact_head.py; proved in
tests/test_exact_interact_cpu.py."""
import dataclasses
import functools

import numpy as np
import torch

import exact_rowsq as Q
from exact_inputs import SENTINEL, full_mantissa, int_matrix, truncate_mantissa

ERR_INDEX = 1  # DLRM_TBE_ERR_INDEX
F64 = np.float64


def npairs(F, self_int):
    return F * (F + 1) // 2 if self_int else F * (F - 1) // 2


def tril(F, self_int):
    """(i, j) of the row-major lower triangle, as numpy index arrays."""
    li, lj = np.tril_indices(F, 0 if self_int else -1)
    return li, lj


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    kind: str            # "int" | "fm_fwd" | "fm_bwd_a" | "fm_bwd_b"
    self_int: bool
    x: torch.Tensor      # [B, D] fp32
    ly: torch.Tensor     # [B, F - 1, D] fp32
    dR: torch.Tensor     # [B, D + pairs] fp32 (zeros for fm_fwd: forward only)
    # gather cases: ly is the looked-up rows, invalid ones zero
    W: torch.Tensor = None         # [total rows, D] fp32
    rows: tuple = None             # rows per table
    idx: torch.Tensor = None       # [F - 1, B] int64, as given (invalid ones included)

    @property
    def B(self):
        return self.x.shape[0]

    @property
    def D(self):
        return self.x.shape[1]

    @property
    def F(self):
        return self.ly.shape[1] + 1

    @property
    def width(self):
        return self.D + npairs(self.F, self.self_int)

    @property
    def T64(self):
        return np.concatenate([self.x.numpy()[:, None, :], self.ly.numpy()], 1).astype(F64)

    @property
    def row_base(self):
        return np.concatenate([[0], np.cumsum(self.rows)]).astype(np.int64)

    @property
    def valid(self):
        return (self.idx >= 0) & (self.idx < torch.tensor(self.rows)[:, None])

    @property
    def flag(self):
        return 0 if bool(self.valid.all()) else ERR_INDEX


# ------------------------------------------------------------------ reference --
def _ident(a):
    return a


def _zgram(T, A=_ident, Bop=_ident):
    return np.einsum("bid,bjd->bij", A(T), Bop(T))


def _scatter(dRp, F, self_int):
    """S = G + G^T [B, F, F] (the diagonal, present under self interaction, counts twice)."""
    li, lj = tril(F, self_int)
    G = np.zeros((dRp.shape[0], F, F), dtype=F64)
    G[:, li, lj] = dRp
    return G + G.transpose(0, 2, 1)


def _round32(a64, exact):
    a32 = a64.astype(np.float32)
    if exact:
        assert np.array_equal(a32.astype(F64), a64), "not exact in fp32"
    return torch.from_numpy(a32)


def forward_ref(case, A=_ident, Bop=_ident):
    """R [B, width] fp32.  ``A`` / ``Bop``: a transformation of the left / right operand of
    T T^T (identity in the reference; a reduced-precision model otherwise)."""
    T = case.T64
    li, lj = tril(case.F, case.self_int)
    Z = _zgram(T, A, Bop)
    return _round32(np.concatenate([T[:, 0], Z[:, li, lj]], 1),
                    case.kind == "int" and A is _ident and Bop is _ident)


def backward_ref(case, relu_x, Sop=_ident, Top=_ident):
    """(grad_x [B, D], grad_ly [B, F-1, D]) fp32; ``Sop`` / ``Top`` as in forward_ref."""
    T, D = case.T64, case.D
    dR = case.dR.numpy().astype(F64)
    S = _scatter(dR[:, D:], case.F, case.self_int)
    dT = np.einsum("bik,bkd->bid", Sop(S), Top(T))
    dT[:, 0] += dR[:, :D]
    if relu_x:
        dT[:, 0] = np.where(case.x.numpy() > 0, dT[:, 0], 0.0)
    exact = case.kind == "int" and Sop is _ident and Top is _ident
    return _round32(dT[:, 0], exact), _round32(dT[:, 1:], exact)


def formula(x, ly, dR, self_int, relu_x, dtype=torch.float64):
    """The same formulas in torch, in ``dtype``: (R, grad_x, grad_ly).  In float64 it is the
    reference above on every case of this module; in float32 it is the arithmetic of the
    reference implementation's bmm and of its autograd (dT = G T + G^T T, two products), which
    the golden fixtures record (test_exact_interact_cpu.py asserts both)."""
    B, D = x.shape
    T = torch.cat([x[:, None, :], ly], 1).to(dtype)
    F = T.shape[1]
    li, lj = (torch.from_numpy(a) for a in tril(F, self_int))
    Z = torch.bmm(T, T.transpose(1, 2))
    R = torch.cat([T[:, 0], Z[:, li, lj]], 1)
    G = torch.zeros(B, F, F, dtype=dtype)
    G[:, li, lj] = dR[:, D:].to(dtype)
    dT = torch.bmm(G, T) + torch.bmm(G.transpose(1, 2), T)
    dT[:, 0] += dR[:, :D].to(dtype)
    if relu_x:
        dT[:, 0] = torch.where(x > 0, dT[:, 0], torch.zeros((), dtype=dtype))
    return R, dT[:, 0], dT[:, 1:]


def cat_ref(x, ly):
    """The cat interaction: R = [x, ly_1, ..., ly_{F-1}] (copies: compare as bits)."""
    return torch.cat([x[:, None, :], ly], 1).reshape(x.shape[0], -1)


def cat_backward_ref(dR, F, D):
    g = dR.reshape(dR.shape[0], F, D)
    return g[:, 0], g[:, 1:]


def terms_ok(case):
    """exact_inputs' criterion on the case's own data.  Integers: the sum of |terms| of every
    output is below 2^24 (quantum 1).  Full-mantissa: every output has at most one non-zero
    term, and dR[:D] is zero wherever the product part of feature 0's gradient is not."""
    T, D = case.T64, case.D
    dR = case.dR.numpy().astype(F64)
    S = _scatter(dR[:, D:], case.F, case.self_int)
    if case.kind == "int":
        for a in (T, dR):
            assert np.array_equal(a, np.rint(a))
        fwd = np.abs(_zgram(np.abs(T))).max(initial=0)
        bwd = np.einsum("bik,bkd->bid", np.abs(S), np.abs(T))
        bwd[:, 0] += np.abs(dR[:, :D])
        return max(fwd, bwd.max(initial=0)) < 2 ** 24
    nzT, nzS = (T != 0).astype(F64), (S != 0).astype(F64)
    if case.kind == "fm_fwd":
        return _zgram(nzT).max() <= 1
    n = np.einsum("bik,bkd->bid", nzS, nzT)
    return n.max() <= 1 and not ((n[:, 0] != 0) & (dR[:, :D] != 0)).any()


# ------------------------------------------------------------------- builders --
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))
    return g


def _finish_int(x, ly, self_int, g, **gather):
    """The integer case over x and ly: x gets a zero, a -0.0 and a negative per sample (D = 1:
    in turn), dR is non-zero in every pair, and dR[:D] is raised by one wherever feature 0's
    unmasked gradient would vanish at such a position - so the mask models are visible."""
    B, D = x.shape
    F = ly.shape[1] + 1
    x = x.clone()
    specials, b = torch.tensor([0.0, -0.0, -2.0]), torch.arange(B)
    if D >= 3:
        for k in range(3):
            x[b, (b + k) % D] = specials[k]
    else:
        x[:, 0] = specials[b % 3]
    if D >= 4:
        x[0, D - 1] = 3.0  # the last column of feature 0 (sample 0's specials sit in 0 .. 2)
    dR = int_matrix((B, D + npairs(F, self_int)), -3, 3, g, nonzero=True)
    case = Case("int", self_int, x, ly, dR, **gather)
    gx, _ = backward_ref(case, False)
    dR[:, :D] += ((gx == 0) & ~(x > 0)).float()
    case = Case("int", self_int, x, ly, dR, **gather)
    check_int_case(case)
    return case


def check_int_case(case):
    """The properties every integer case has (asserted by the builders)."""
    x, ly, dR, B, F, D = case.x, case.ly, case.dR, case.B, case.F, case.D
    assert terms_ok(case)
    gx, _ = backward_ref(case, False)
    special = ~(x > 0)
    assert bool((x == 0).any()) and bool(torch.signbit(x[x == 0]).any() or (B < 2 and D < 3))
    assert bool((x < 0).any()) or (B < 3 and D < 3)
    assert bool((gx[special] != 0).all()), "upstream gradient vanishes at a masked position"
    T = torch.cat([x[:, None], ly], 1)
    assert bool((T[:, F - 1] != 0).any()) and bool((T[:, :, D - 1] != 0).any())
    assert bool((T[B - 1] != 0).any()) and bool((dR[B - 1] != 0).any())
    assert bool((dR[:, D:] != 0).all())  # every pair, the diagonal ones included


@functools.lru_cache(maxsize=None)
def int_case(B, F, D, self_int, seed=0):
    g = _gen(1, B, F, D, self_int, seed)
    x = int_matrix((B, D), -3, 3, g, nonzero=False)
    ly = int_matrix((B, F - 1, D), -3, 3, g, nonzero=True)
    return _finish_int(x, ly, self_int, g)


@functools.lru_cache(maxsize=None)
def gather_case(B, F, D, self_int, invalid=(), seed=0):
    """An integer case whose features 1.. are rows of F - 1 tables, one of them of a single row;
    the last row of the last table is looked up by the last sample.  ``invalid``: tuples
    (value, feature, sample) with value -1 or "rows" (one past the table)."""
    g = _gen(2, B, F, D, self_int, seed)
    T = F - 1
    rows = [int(r) for r in torch.randint(2, 40, (T,), generator=g)]
    rows[T // 2] = 1
    rb = np.concatenate([[0], np.cumsum(rows)])
    W = int_matrix((int(rb[-1]), D), -3, 3, g, nonzero=True)
    idx = torch.stack([torch.randint(0, n, (B,), generator=g) for n in rows])
    idx[T - 1, B - 1] = rows[T - 1] - 1
    for value, f, b in invalid:
        idx[f - 1, b] = rows[f - 1] if value == "rows" else value
    ok = (idx >= 0) & (idx < torch.tensor(rows)[:, None])
    glob = torch.from_numpy(rb[:-1])[:, None] + idx.clamp(min=0)
    ly = torch.where(ok[:, :, None], W[torch.where(ok, glob, torch.zeros_like(glob))],
                     torch.zeros(()))
    x = int_matrix((B, D), -3, 3, g, nonzero=False)
    return _finish_int(x, ly.transpose(0, 1).contiguous(), self_int, g, W=W, rows=tuple(rows),
                       idx=idx)


def as_gather(case):
    """The case as a lookup: table t holds feature t + 1's B rows, sample b looks up row b."""
    B, T, D = case.ly.shape
    return dataclasses.replace(case, W=case.ly.transpose(0, 1).reshape(T * B, D).contiguous(),
                               rows=(B,) * T, idx=torch.arange(B).repeat(T, 1))


def pack_int_rows(W, bits):
    """uint8 [rows, row_bytes]: integer rows in [-3, 3] as Q8 | Q4 rows with scale 1 and bias
    -3 (levels 0 .. 6), so fma(scale, q, bias) gives W back exactly."""
    w = W.numpy()
    rows, D = w.shape
    q = (w + 3).astype(np.uint8)
    assert np.array_equal(q.astype(np.float32) - 3, w) and q.max(initial=0) <= 6
    out = np.empty((rows, Q.row_bytes(bits, D)), dtype=np.uint8)
    sb = np.array([1.0, -3.0], dtype=np.float32 if bits == 8 else np.float16).view(np.uint8)
    if bits == 8:
        out[:, :D] = q
        out[:, D:] = sb
    else:
        out[:, :D // 2] = q[:, 0::2] | (q[:, 1::2] << 4)
        out[:, D // 2:] = sb
    assert np.array_equal(Q.dequant(out, bits, D), w)
    return out


def signed_fm(shape, g):
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return full_mantissa(shape, g) * sign * 2.0 ** torch.randint(-2, 3, shape, generator=g)


def _pow2(shape, g):
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return sign * 2.0 ** torch.randint(-2, 3, shape, generator=g)


# which operand of the product carries the full mantissas, per kind
FM_OPERANDS = {"fm_fwd": ("A", "B"), "fm_bwd_a": ("S",), "fm_bwd_b": ("T",)}


@functools.lru_cache(maxsize=None)
def fm_case(kind, B, F, D, self_int, seed=0):
    """Full-mantissa cases: every output one fp32 product, rounded once.
    fm_fwd    each feature row has one non-zero value, in column 0, D/2 or D-1 (features share
              columns): Z[i][j] = fl(v_i v_j) or 0, the diagonal fl(v_i^2).  Forward only.
    fm_bwd_a  dR's pair part is full-mantissa and T is one +-2^e per row in distinct columns
              (F <= D): dT[i][c_k] = S[i][k] * +-2^e.
    fm_bwd_b  one pair of dR per sample is +-2^e (the pairs in turn, the last one first) and T
              is full-mantissa: dT[i] = g T[j], dT[j] = g T[i].
    In both backward kinds dR[:D] is full-mantissa where the product part of feature 0's
    gradient is zero, and zero elsewhere."""
    g = _gen(3, sorted(FM_OPERANDS).index(kind), B, F, D, self_int, seed)
    P = npairs(F, self_int)
    dR = torch.zeros(B, D + P)
    if kind == "fm_fwd":
        cols = torch.tensor(sorted({0, D // 2, D - 1}))
        col = cols[torch.randint(0, len(cols), (B, F), generator=g)]
        col[:, F - 1] = D - 1
        T = torch.zeros(B, F, D)
        T.scatter_(2, col[:, :, None], signed_fm((B, F, 1), g))
    elif kind == "fm_bwd_a":
        assert F <= D
        col = torch.stack([torch.randperm(D, generator=g)[:F] for _ in range(B)])
        T = torch.zeros(B, F, D)
        T.scatter_(2, col[:, :, None], _pow2((B, F, 1), g))
        dR[:, D:] = signed_fm((B, P), g)
        free = torch.ones(B, D, dtype=torch.bool)
        free.scatter_(1, col[:, 0 if self_int else 1:], False)
        dR[:, :D] = signed_fm((B, D), g) * free
    else:
        assert P >= 1
        T = signed_fm((B, F, D), g)
        li, lj = tril(F, self_int)
        p = (P - 1 - torch.arange(B)) % P
        dR[torch.arange(B), D + p] = _pow2((B,), g)
        touches0 = torch.from_numpy((li == 0) | (lj == 0))[p]
        dR[:, :D] = signed_fm((B, D), g) * ~touches0[:, None]
    case = Case(kind, self_int, T[:, 0].contiguous(), T[:, 1:].contiguous(), dR)
    assert terms_ok(case)
    for alt in reduced_precision_results(case).values():
        assert not _same(alt, reference(case, relu_x=False)), (kind, B, F, D, self_int)
    return case


def reference(case, relu_x=True):
    """{"R", "gx", "gly"} of the case; the backward full-mantissa kinds have no "R" (their
    dense T makes the forward inexact: they are backward cases only)."""
    gx, gly = backward_ref(case, relu_x)
    out = {"R": forward_ref(case), "gx": gx, "gly": gly}
    if case.kind.startswith("fm_bwd"):
        del out["R"]
    return out


def _same(a, b):
    keys = set(a) & set(b)
    assert keys
    return all(np.array_equal(a[k].numpy().view(np.int32), b[k].numpy().view(np.int32))
               for k in keys)


def _np_op(fn):
    return lambda a: fn(torch.from_numpy(a.astype(np.float32))).numpy().astype(F64)


REDUCED = {"trunc10": _np_op(lambda t: truncate_mantissa(t, 10)),
           "trunc7": _np_op(lambda t: truncate_mantissa(t, 7)),
           "bf16": _np_op(lambda t: t.bfloat16().float())}


def reduced_precision_results(case):
    """{(model, operand): outputs}: the case computed with one operand of its product cut to
    10 or 7 mantissa bits or rounded to bf16 - on each operand that carries full mantissas
    (FM_OPERANDS).  A full-mantissa case differs from every one of them."""
    out = {}
    for name, op in REDUCED.items():
        for which in FM_OPERANDS[case.kind]:
            if which in "AB":
                R = forward_ref(case, **{"A" if which == "A" else "Bop": op})
                out[name, which] = {"R": R}
            else:
                gx, gly = backward_ref(case, False, **{"Sop" if which == "S" else "Top": op})
                out[name, which] = {"gx": gx, "gly": gly}
    return out


# ----------------------------------------------------------------- bug models --
# Each model maps (case, relu_x) to the outputs a kernel with that bug would write, and says
# which cases it can affect; test_exact_interact_cpu.py asserts that it changes bits on every
# such case.  Outputs that the bug leaves unwritten hold SENTINEL.
def pair_of(p, self_int):
    """(i, j) of pair p (interact.hip's pair_of, in exact integer arithmetic)."""
    i = 0 if self_int else 1
    while npairs(i + 1, self_int) <= p:  # the pairs of rows 0 .. i
        i += 1
    return i, p - (i * (i + 1) // 2 if self_int else i * (i - 1) // 2)


def _from_parts(case, relu_x, T=None, Tprod=None, S=None, dx=None, mask=None, R_pairs=None):
    """The formulas with parts replaced: T (what is copied to R[:D]), Tprod (the operand of
    the products), S, dx (= dR[:D]) and the ReLU mask."""
    D = case.D
    T = case.T64 if T is None else T
    Tprod = T if Tprod is None else Tprod
    dR = case.dR.numpy().astype(F64)
    li, lj = tril(case.F, case.self_int)
    Z = _zgram(Tprod)
    pairs = Z[:, li, lj] if R_pairs is None else R_pairs(Z)
    S = _scatter(dR[:, D:], case.F, case.self_int) if S is None else S
    dT = np.einsum("bik,bkd->bid", S, Tprod)
    dT[:, 0] += dR[:, :D] if dx is None else dx
    if mask is None:
        mask = case.x.numpy() > 0 if relu_x else np.ones((case.B, D), dtype=bool)
    dT[:, 0] = np.where(mask, dT[:, 0], 0.0)
    return {"R": _round32(np.concatenate([T[:, 0], pairs], 1), False),
            "gx": _round32(dT[:, 0], False), "gly": _round32(dT[:, 1:], False)}


def bug_row_dropped(case, relu_x):
    T = case.T64.copy()
    T[:, case.F - 1] = 0
    out = _from_parts(case, relu_x, T=case.T64, Tprod=T)
    if case.F >= 2:
        out["gly"][:, -1] = 0  # the row's own gradient is never formed either
    return out


def bug_col_dropped(case, relu_x):
    T = case.T64.copy()
    T[:, :, case.D - 1] = 0
    return _from_parts(case, relu_x, T=case.T64, Tprod=T)


def bug_diag_once(case, relu_x):
    S = _scatter(case.dR.numpy().astype(F64)[:, case.D:], case.F, case.self_int)
    i = np.arange(case.F)
    S[:, i, i] *= 0.5
    return _from_parts(case, relu_x, S=S)


def bug_wrong_triangle(case, relu_x):
    """The strict triangle under self interaction, and the reverse: pair p is read from, and
    its gradient scattered to, the other triangle's p-th cell (cells past it: zero)."""
    F, D, P = case.F, case.D, npairs(case.F, case.self_int)
    li, lj = tril(F, not case.self_int)
    n = min(P, li.size)
    dRp = case.dR.numpy().astype(F64)[:, D:]
    G = np.zeros((case.B, F, F), dtype=F64)
    G[:, li[:n], lj[:n]] = dRp[:, :n]

    def pairs(Z):
        out = np.zeros((case.B, P), dtype=F64)
        out[:, :n] = Z[:, li[:n], lj[:n]]
        return out
    return _from_parts(case, relu_x, S=G + G.transpose(0, 2, 1), R_pairs=pairs)


def bug_pair_of_off_by_one(case, relu_x):
    """pair_of one row short at every triangular number p > 0 (the float sqrt rounding down
    with no correction loop): pair p = tri(i) resolves to (i - 1, p - tri(i - 1))."""
    F, D, P = case.F, case.D, npairs(case.F, case.self_int)
    cells = []
    for p in range(P):
        i, j = pair_of(p, case.self_int)
        if j == 0 and p > 0:
            i, j = i - 1, p - (i * (i - 1) // 2 if case.self_int else (i - 1) * (i - 2) // 2)
        cells.append((i, j))
    ci = np.array([c[0] for c in cells], dtype=np.int64)
    cj = np.array([c[1] for c in cells], dtype=np.int64)
    dRp = case.dR.numpy().astype(F64)[:, D:]
    G = np.zeros((case.B, F, F), dtype=F64)
    for p in range(P):  # the last writer wins, as in LDS
        G[:, ci[p], cj[p]] = dRp[:, p]
    S = G + G.transpose(0, 2, 1)
    return _from_parts(case, relu_x, S=S, R_pairs=lambda Z: Z[:, ci, cj])


def bug_mask_ge(case, relu_x):
    return _from_parts(case, relu_x, mask=(case.x.numpy() >= 0) if relu_x else None)


def bug_dx_not_added(case, relu_x):
    return _from_parts(case, relu_x, dx=np.zeros((case.B, case.D)))


def bug_relu_when_off(case, relu_x):
    return _from_parts(case, True)


def bug_tail_unwritten(case, relu_x):
    """The last width % 4 floats of a row neither written (R) nor read (dR)."""
    w4 = case.width // 4 * 4
    dR = case.dR.clone()
    dR[:, w4:] = 0
    out = reference(dataclasses.replace(case, dR=dR), relu_x)
    out["R"][:, w4:] = SENTINEL
    return out


def bug_partial_group_dropped(case, relu_x):
    out = {k: v.clone() for k, v in reference(case, relu_x).items()}
    for v in out.values():
        v[case.B // 4 * 4:] = SENTINEL
    return out


def list_strides(F, D):
    """Pairwise different batch strides, feature 0's the smallest (D, D + 4, D + 8, ...)."""
    return [D + 4 * f for f in range(F)]


def bug_bs0_everywhere(case, relu_x):
    """Feature f's row of sample b read at b * bs[0] inside feature f's own buffer, the
    buffers being those of the list layout (list_strides; row b of a buffer starts at
    b * stride, NaN between rows)."""
    B, F, D = case.B, case.F, case.D
    T = case.T64
    wrong = T.copy()
    for f, bs in enumerate(list_strides(F, D)):
        buf = np.full(B * bs, np.nan)
        for b in range(B):
            buf[b * bs:b * bs + D] = T[b, f]
        for b in range(B):
            wrong[b, f] = buf[b * D:b * D + D]
    with np.errstate(invalid="ignore"):
        return _from_parts(case, relu_x, T=wrong)


def bug_invalid_not_zeroed(case, relu_x):
    """An invalid index read as row 0 of its table instead of as a zero row."""
    rb = torch.from_numpy(case.row_base[:-1])[:, None]
    ly = case.ly.clone()
    bad = ~case.valid
    ly.transpose(0, 1)[bad] = case.W[(rb + torch.zeros_like(case.idx))[bad]]
    return reference(dataclasses.replace(case, ly=ly), relu_x)


# name -> (model, the cases it can affect, the outputs it can change)
BUG_MODELS = {
    "row_dropped": (bug_row_dropped, lambda c, r: c.F >= 2),
    "col_dropped": (bug_col_dropped, lambda c, r: npairs(c.F, c.self_int) >= 1),
    "diag_once": (bug_diag_once, lambda c, r: c.self_int),
    "wrong_triangle": (bug_wrong_triangle, lambda c, r: c.F >= 2),
    "pair_of_off_by_one": (bug_pair_of_off_by_one,
                           lambda c, r: c.F >= 3),  # F = 2: no such p, or the mirror cell
    "mask_ge": (bug_mask_ge, lambda c, r: r),
    "dx_not_added": (bug_dx_not_added, lambda c, r: not r or bool((c.x > 0).any())),
    "relu_when_off": (bug_relu_when_off, lambda c, r: not r),
    "tail_unwritten": (bug_tail_unwritten, lambda c, r: c.width % 4 != 0),
    "partial_group_dropped": (bug_partial_group_dropped, lambda c, r: c.B % 4 != 0),
    "bs0_everywhere": (bug_bs0_everywhere, lambda c, r: c.F >= 2 and c.B >= 2),
    "invalid_not_zeroed": (bug_invalid_not_zeroed, lambda c, r: c.idx is not None and c.flag),
}


# ---------------------------------------------------------- dispatch formulas --
# A RESTATEMENT of csrc/interact.hip's host code (waves_for, fwd_version, bwd_version, the
# grid sizes of the launches): keep it in step with that file.  The tests use it only to
# assert which class a shape falls in, never to compute an expected value.
K_MAX_F = 64
STAGED_D = (16, 32, 64, 128)
V5_MAX_BATCH = 1024
CAP_STAGED = 8192    # workgroups of 4 waves: v4 forward, v3 and v4 backward
CAP_V5 = 16384       # v5_grid: a workgroup per sample
CAP_RUNTIME = 4096   # grid_for: the runtime-D MFMA kernels
LDS_BYTES = 64 * 1024


def waves_for(per_wave_bytes):
    for w in (4, 2, 1):
        if per_wave_bytes * w <= LDS_BYTES:
            return w
    return 0


def fwd_waves(F, D):
    return waves_for(F * (D + 1) * 4)


def bwd_waves(F, D):
    return waves_for((F * (D + 1) + 32 * 33) * 4)


def fwd_version(D, B, forced=0):
    if forced == 4:
        return 4
    if forced == 5:
        return 5 if D >= 64 else 4
    return 5 if D >= 64 and B <= V5_MAX_BATCH else 4


def bwd_version(D, B, forced=0):
    if forced in (3, 4):
        return forced
    if forced == 5:
        return 5 if D >= 64 else 4
    if D <= 32:
        return 4
    return 5 if B <= V5_MAX_BATCH else 3


def fwd_kernel(B, F, D, forced=0, aligned=True):
    """("v4" | "v5" | "mfma" | "generic", workgroups launched, units a workgroup takes per
    trip of its grid-stride loop, units in all); the elementwise kernel has no such loop."""
    if F <= 32 and D in STAGED_D and aligned:
        if fwd_version(D, B, forced) == 5:
            return "v5", min(B, CAP_V5), 1, B
        return "v4", min(-(-B // 4), CAP_STAGED), 4, B
    w = fwd_waves(F, D)
    if F <= 32 and w:
        return "mfma", min(-(-B // w), CAP_RUNTIME), w, B
    return "generic", None, None, B


def bwd_kernel(B, F, D, forced=0, aligned=True, grads_aligned=True):
    if F <= 32 and D in STAGED_D and aligned and grads_aligned:
        v = bwd_version(D, B, forced)
        if v == 5:
            return "v5", min(B, CAP_V5), 1, B
        if v == 4:
            nblk = D // 32 if D > 32 else 1  # a unit: a 32-column block of a sample
            return "v4", min(-(-B * nblk // 4), CAP_STAGED), 4, B * nblk
        return "v3", min(-(-B // 4), CAP_STAGED), 4, B
    w = bwd_waves(F, D)
    if F <= 32 and w:
        return "mfma", min(-(-B // w), CAP_RUNTIME), w, B
    return "generic", None, None, B


def crosses_cap(kernel):
    """True when the launch is capped: some workgroup takes a second trip of its loop."""
    name, grid, per, units = kernel
    return per is not None and units > grid * per


def instantiated_templates():
    """Every (kernel, D, GATHER) interact.hip instantiates: the forward kernels take every
    gather mode (0 pooled, 1 fp32, 2 fp16, 3 Q8, 4 Q4), the backward ones 0, 1 and 2; v5
    exists for D = 64 and 128."""
    out = set()
    for D in STAGED_D:
        out |= {("fwd_v4", D, g) for g in range(5)}
        out |= {(k, D, g) for k in ("bwd_v3", "bwd_v4") for g in range(3)}
        if D >= 64:
            out |= {("fwd_v5", D, g) for g in range(5)}
            out |= {("bwd_v5", D, g) for g in range(3)}
    return out


FWD_FORCED = (4, 5, 0)
BWD_FORCED = (3, 4, 5, 0)
STAGED_F = (1, 2, 3, 9, 17, 27, 31, 32)
STAGED_B = (1, 3, 5, 9)


def staged_plan():
    """The trimmed cross product of the staged test: entries (D, F, self_int, B, relu_x,
    gather) - every entry runs under every forced forward and backward version; ``gather``
    (0: none) is the mode run next to the pooled entry points.  F = 1 and F = 32 take both
    self modes at every D."""
    plan = []
    for di, D in enumerate(STAGED_D):
        for k, F in enumerate(STAGED_F):
            for self_int in ((False, True) if F in (1, 32) else ((k + di) % 2 == 1,)):
                B = STAGED_B[(k + di) % 4]
                relu_x = (k // 2 + di + self_int) % 2 == 0
                gather = 0 if F == 1 else 1 + k % 4
                plan.append((D, F, self_int, B, relu_x, gather))
    return plan


def templates_of(plan):
    """The templates a staged plan runs, by the restated ladder."""
    out = set()
    for D, F, self_int, B, relu_x, gather in plan:
        for g in {0, gather} if F >= 2 else {0}:
            for v in FWD_FORCED:
                out.add(("fwd_" + fwd_kernel(B, F, D, v)[0], D, g))
            if g <= 2:
                for v in BWD_FORCED:
                    out.add(("bwd_" + bwd_kernel(B, F, D, v)[0], D, g))
    return out


RUNTIME_D = (1, 4, 5, 13, 65, 100, 200, 300, 500, 520)
RUNTIME_SMALL_F = 7
ELEMENTWISE_F = (33, 41, 64)
OUT_LAYOUTS = ("vec", "odd", "off1")  # "vec" at a width with and without a tail
LAYOUT_SHAPES = {"tail": (27, False), "no tail": (9, False)}  # (F, self): width % 4 = 3 | 0
# (what, forward or backward, forced version, B, D): the caps of interact.hip, each crossed at
# the smallest shape (F = 2)
CAP_CASES = (("v4 forward", "fwd", 4, 32773, 16), ("v3 backward", "bwd", 3, 32773, 16),
             ("v4 backward", "bwd", 4, 8195, 128), ("v5 forward", "fwd", 5, 16387, 64),
             ("v5 backward", "bwd", 5, 16387, 64), ("runtime-D forward", "fwd", 0, 16389, 4),
             ("runtime-D backward", "bwd", 0, 16389, 4))
