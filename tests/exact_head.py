"""Inputs and CPU references for the exact-arithmetic tests of the step's tail: the fused head
(dlrm_head_step, its deferred finalize, dlrm_head_predict, dlrm_head_forward_backward), the
bias-gradient column sums, the dense optimizers and the device RNG fills.

The head's per-row math goes through expf / logf, which are not correctly rounded, so the
anchor rows use the three logits whose sigmoid follows from IEEE arithmetic alone:
    z = 0    expf(-0) = 1                      p = 0.5
    z = 24   1 + expf(-24) rounds to 1          p = 1
    z = -100 expf(100) overflows to inf         p = 0
With integer X and w, dz is then a dyadic number and every product and partial sum of the
weight gradient is exact in any order (head_case asserts the condition), so the kernel must
equal the reference BIT FOR BIT.  Rows with integer z in [-16, 16] ("general") check the
transcendental part under a measured ulp bound and everything after it bitwise.

Plain helper module (numpy / torch on the CPU, no GPU import), proved in
test_exact_head_cpu.py."""
from dataclasses import dataclass
from fractions import Fraction

import numpy as np
import torch

f32, f64 = np.float32, np.float64

# both sides of every DLRM_HEAD_NC_DISPATCH edge (NC 2 | 4 | 5 | 8 | 12 | 17 | 24 | 32)
HEAD_KS = [1, 2, 63, 64, 65, 128, 129, 256, 257, 320, 321, 512, 513, 768, 769, 1088, 1089,
           1536, 1537, 2048]
HEAD_MS = [1, 3, 4, 5, 37, 64, 257, 1023]  # fl(fl(1/M) * M) == 1 for each
# (M, K) of the anchor cases: every K at M = 5 and 257, every M at K = 2, 65, 321
HEAD_SHAPES = sorted({(M, K) for M in (5, 257) for K in HEAD_KS} |
                     {(M, K) for M in HEAD_MS for K in (2, 65, 321)})
ANCHOR_P = {0: 0.5, 24: 1.0, -100: 0.0}
MSE_TARGETS = [0.0, 0.25, 0.5, 0.75, 1.0]


def head_nc(K):
    """The NC instantiation DLRM_HEAD_NC_DISPATCH picks for K columns."""
    nc = -(-K // 64)
    return next(v for v in (2, 4, 5, 8, 12, 17, 24, 32) if nc <= v)


def inv_m_exact(M):
    """fl(fl(1/M) * M) == 1 in float32: grad_scale = M / 8 then cancels the kernel's 1/M."""
    return f32(f32(1) / f32(M)) * f32(M) == f32(1)


@dataclass
class HeadCase:
    M: int
    K: int
    loss: str
    kind: str          # "anchor" | "saturated" | "general"
    X: torch.Tensor    # [M, K] integers in [-1, 3] (column K-2 carries the logit), X[:, K-1] = 1
    w: torch.Tensor    # [K] integers in [-2, 2], w[K-2] = 1, w[K-1] the folded bias
    t: torch.Tensor    # [M] targets
    z: np.ndarray      # [M] the exact logits (int64)
    grad_scale: float


def head_case(M, K, loss, kind="anchor", seed=0, grad_scale=None):
    """Rows whose dot product is exactly the chosen logit.  anchor: z = 0 on the rows that
    matter to a row or block bug (m % 4 == 3, the last row) and on every third row before
    the last 4-row block, 24 / -100 elsewhere; saturated: only 24 / -100; general: integers
    in [-16, 16]."""
    assert K > 1 or kind == "anchor", "K = 1 has w = 0: every logit is 0"
    g = torch.Generator().manual_seed(1000 * M + K + 7 * seed + (loss == "bce"))
    w = torch.randint(-2, 3, (K,), generator=g).double()
    X = torch.randint(-1, 4, (M, K), generator=g).double()
    X[:, K - 1] = 1.0
    m = np.arange(M)
    if kind == "general":
        z = torch.randint(-16, 17, (M,), generator=g).numpy()
    elif kind == "saturated":
        z = np.where(m % 2 == 0, 24, -100)
    else:
        z = np.where(m % 2 == 0, 24, -100)
        z[(m % 4 == 3) | (m == M - 1) | ((m % 3 == 0) & (m < (M - 1) // 4 * 4))] = 0
    if K == 1:
        w[:] = 0.0
        z = np.zeros(M, dtype=np.int64)
    else:
        if w[K - 1] == 0:
            w[K - 1] = -1.0  # a bias that counts
        w[K - 2] = 1.0
        if K >= 3:  # a zero and a negative input under a nonzero weight on the last row
            w[0], X[M - 1, 0] = 2.0, 0.0
        if K >= 4:
            w[1], X[M - 1, 1] = -1.0, -1.0
        X[:, K - 2] = 0.0
        X[:, K - 2] = torch.from_numpy(z.astype(np.float64)) - X @ w
    z = z.astype(np.int64)
    assert np.array_equal((X @ w).numpy(), z.astype(np.float64))
    key = torch.from_numpy((m % 4 == 3) | (m == M - 1))
    if loss == "bce":
        t = torch.randint(0, 2, (M,), generator=g).double()
        t[key] = 0.0  # the rows a bug model drops pull one way: their sum cannot cancel
    else:
        t = torch.tensor(MSE_TARGETS, dtype=torch.float64)[torch.randint(0, 5, (M,), generator=g)]
        t[key & (t >= 0.5)] = 0.25
    if grad_scale is None:
        assert inv_m_exact(M), M
        grad_scale = M * 2.0 ** -3
    c = HeadCase(M, K, loss, kind, X.float(), w.float(), t.float(), z, float(grad_scale))
    if kind != "general" and float(grad_scale) == M * 2.0 ** -3:
        ok, why = head_exact_ok(c)
        assert ok, why
    return c


def anchor_prob(z):
    return np.array([ANCHOR_P[int(v)] for v in z], dtype=f32)


def head_row_ref(p, t, loss, lo, gscale, M):
    """float32 restatement of head_row_math given p = sigmoid(z), one operation per rounding:
    (pc, dz, pass).  numpy keeps float32 op float32 in float32."""
    p, t = np.asarray(p, dtype=f32), np.asarray(t, dtype=f32)
    invM = f32(1) / f32(M)
    pc, passed = p.copy(), np.ones(p.shape, dtype=bool)
    if 0.0 < lo < 0.5:
        lo32 = f32(lo)
        hi = f32(1) - lo32
        passed = (p >= lo32) & (p <= hi)
        pc = np.minimum(np.maximum(p, lo32), hi)
    with np.errstate(over="ignore", invalid="ignore"):
        if loss == "bce":
            den = np.maximum((f32(1) - pc) * pc, f32(1e-12))
            dp = (pc - t) / den * invM
        else:
            dp = f32(2) * (pc - t) * invM
        dp = dp * f32(gscale)
        dp = np.where(passed, dp, f32(0))
        dz = dp * (f32(1) - p) * p
    assert pc.dtype == f32 and dz.dtype == f32
    return pc, dz, passed


def row_loss64(pc, t, loss):
    """The row loss at the (clamped) probability, in float64; 1 - pc is the kernel's float32
    difference, and the logs are clamped at -100 as torch's BCELoss does."""
    pc = np.asarray(pc, dtype=f32)
    t = np.asarray(t, dtype=f64)
    if loss == "mse":
        d = pc.astype(f64) - t
        return d * d
    with np.errstate(divide="ignore"):
        lp = np.maximum(np.log(pc.astype(f64)), -100.0)
        l1p = np.maximum(np.log((f32(1) - pc).astype(f64)), -100.0)
    return -(t * lp + (1.0 - t) * l1p)


def head_reference(c, p=None, lo=0.0, grad_scale=None, model=None):
    """Everything dlrm_head_step writes, from p = sigmoid(z) (the anchors' exact values when
    None): prob, dz, dX (masked / unmasked), dw, loss and the per-row loss.  The reduced
    outputs are float64 sums (exact for the anchor cases).  ``model`` applies one bug model
    (test_exact_head_cpu.py proves each changes the result)."""
    M, K = c.M, c.K
    gs = c.grad_scale if grad_scale is None else grad_scale
    X, w, t = c.X.numpy(), c.w.numpy(), c.t.numpy()
    z = c.z.astype(f64)
    Meff = M
    if model == "m_rounded_up":
        Meff = -(-M // 4) * 4
    if model == "grad_scale_ignored":
        gs = 1.0
    if model == "col_skipped" and K % 64 == 1:
        z = z - w[K - 1] * X[:, K - 1]
        p = None
    if model == "pad_included":
        z = z + np.nan
    if p is None:
        anchors = all(v in ANCHOR_P for v in np.unique(z))
        p = anchor_prob(z) if anchors else sigmoid64(z).astype(f32)
    pc, dz, _ = head_row_ref(p, t, c.loss, lo, gs, Meff)
    dXu = (dz[:, None].astype(f64) * w[None, :].astype(f64)).astype(f32)  # fl(dz * w)
    mask = (X >= 0) if model == "mask_ge" else (X > 0)
    dXm = np.where(mask, dXu, f32(0))
    rows = np.ones(M, dtype=bool)
    if model == "row_dropped":
        rows[np.arange(M) % 4 == 3] = False
    if model == "block_dropped":
        rows[(M - 1) // 4 * 4:] = False
    dw64 = (dz[rows, None].astype(f64) * X[rows].astype(f64)).sum(0)
    if model == "col_skipped" and K % 64 == 1:
        dw64[K - 1] = 0.0
        dXu[:, K - 1] = dXm[:, K - 1] = 0.0
    rl = row_loss64(pc, t, c.loss)
    loss = (f32(rl.sum()) / f32(M)).astype(f32)
    return dict(prob=pc, dz=dz, dXm=dXm, dXu=dXu, dw64=dw64, dw=dw64.astype(f32),
                row_loss=rl, loss=np.array([loss], dtype=f32))


HEAD_MODELS = ["row_dropped", "block_dropped", "m_rounded_up", "mask_ge", "col_skipped",
               "pad_included", "grad_scale_ignored"]


def model_applies(model, M, K):
    """Whether a bug model can change anything at this shape."""
    return {"row_dropped": M >= 4, "m_rounded_up": M % 4 != 0, "mask_ge": K >= 3,
            "col_skipped": K % 64 == 1}.get(model, True)


def head_exact_ok(c, lo=0.0):
    """The anchor condition: dz dyadic (a multiple of 2^-6: 2^-5 or 2^-6 for MSE, 2^-4 for
    BCE, 0 on the saturated rows) and max_k sum_m |dz_m x_mk| * 2^6 < 2^24, so every partial
    sum of dw is a multiple of 2^-6 below 2^18 - exact in float32 in any order - and the row
    losses sum exactly."""
    r = head_reference(c, lo=lo)
    dz = r["dz"].astype(f64)
    if not np.array_equal(dz * 64, np.round(dz * 64)):
        return False, "dz is not a multiple of 2^-6"
    s = (np.abs(dz)[:, None] * np.abs(c.X.numpy().astype(f64))).sum(0).max()
    if not s * 64 < 2 ** 24:
        return False, f"sum |dz x| = {s} too large"
    if c.loss == "mse" or (c.kind == "saturated" and lo == 0.0):
        rl = r["row_loss"]
        if not (np.array_equal(rl * 16, np.round(rl * 16)) and rl.sum() * 16 < 2 ** 24):
            return False, "row losses do not sum exactly"
    return True, ""


def ref_sgd_w(w, dw64, lr):
    """fmaf(-lr, s, w) with a dyadic lr: the float64 value is exact, one rounding."""
    return (np.asarray(w, dtype=f64) - lr * dw64).astype(f32)


# ------------------------------------------------------------------ ulp measures ----
def ulp_error(got, ref64):
    """|got - ref| in units of the float32 ulp of ref (ref in float64)."""
    ref64 = np.asarray(ref64, dtype=f64)
    ulp = np.spacing(np.abs(ref64).astype(f32)).astype(f64)
    return np.abs(np.asarray(got, dtype=f64) - ref64) / ulp


def sigmoid64(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, dtype=f64)))


SWEEP_Z = np.arange(-200, 49) * 0.5  # every half-integer z in [-100, 24]


# ------------------------------------------------------------------------ colsum ----
COLSUM_MS = [0, 1, 63, 64, 65, 129, 1025]
COLSUM_NS = [1, 255, 256, 257, 300]
COLSUM_SCALES = [1.0, -1.0, 0.5, -0.5, 2.0]


def colsum_case(M, N, scaled, seed=0):
    """Y: integers in [-4, 4] (no zeros); scale (when asked for): dyadic values, one per row."""
    g = torch.Generator().manual_seed(100 * M + N + seed)
    Y = torch.randint(-4, 4, (M, N), generator=g)
    Y = torch.where(Y >= 0, Y + 1, Y).float()
    scale = None
    if scaled:
        scale = torch.tensor(COLSUM_SCALES)[torch.randint(0, 5, (M,), generator=g)]
    return Y, scale


def ref_colsum(Y, scale, alpha=1.0, out0=None, param0=None, lr=0.0, model=None):
    """(out, sgd_param) of dlrm_colsum_f32 in float64 (exact: integers times dyadic factors):
    out = [out0 +] alpha * s, param = param0 - lr * s with s the scaled column sum."""
    Y64 = Y.numpy().astype(f64)
    if scale is not None:
        Y64 = Y64 * scale.numpy().astype(f64)[:, None]
    rows = np.ones(Y64.shape[0], dtype=bool)
    if model == "chunk_row_dropped":
        rows[np.arange(Y64.shape[0]) % 64 == 63] = False
    s = Y64[rows].sum(0)
    a = 1.0 if model == "alpha_ignored" and out0 is not None else alpha
    out = a * s + (0.0 if out0 is None else out0.numpy().astype(f64))
    assert np.abs(out).max(initial=0) < 2 ** 24 and np.array_equal(out * 4, np.round(out * 4))
    param = None
    if param0 is not None:
        param = (param0.numpy().astype(f64) - lr * s).astype(f32)
    return out.astype(f32), param


# -------------------------------------------------------------- dense optimizers ----
OPT_NS = [0, 1, 255, 256, 257, 4194304 + 3]  # the last crosses the 16384-workgroup cap


def sgd_case(n, seed=0):
    g = torch.Generator().manual_seed(n + seed)
    return (torch.randint(-8, 9, (n,), generator=g).float(),
            torch.randint(-8, 9, (n,), generator=g).float())


def ref_sgd(p, g, lr):
    return torch.from_numpy((p.numpy().astype(f64) - lr * g.numpy().astype(f64)).astype(f32))


def adagrad_case(n, seed=0):
    """p: integers in [-8, 8]; g: nonzero integers in [-64, 64]; state_sum = r^2 - g^2 with an
    integer r in (|g|, 4096), so g^2 + state_sum is the perfect square r^2 (when the gradient
    is not rescaled) and sqrtf is exact."""
    gen = torch.Generator().manual_seed(n + 11 + seed)
    p = torch.randint(-8, 9, (n,), generator=gen).float()
    g = torch.randint(-64, 64, (n,), generator=gen)
    g = torch.where(g >= 0, g + 1, g)
    r = g.abs() + torch.randint(1, 4000, (n,), generator=gen)
    ss = (r * r - g * g).float()
    assert n == 0 or int(r.max()) < 4096
    return p, g.float(), ss


def round_sum_f32(a, b):
    """fl32(a + b) for float64 arrays whose exact sum may not fit float64 (an fma's single
    rounding: a the exact product, b the addend).  h + e = a + b exactly (two-sum); rounding h
    is right unless h sits exactly halfway between two float32 values, where e breaks the tie."""
    a, b = np.asarray(a, dtype=f64), np.asarray(b, dtype=f64)
    h = a + b
    bb = h - a
    e = (a - (h - bb)) + (b - bb)
    r = h.astype(f32)
    up, dn = np.nextafter(r, f32(np.inf)), np.nextafter(r, f32(-np.inf))
    r64 = r.astype(f64)
    tie_up = (h == (r64 + up.astype(f64)) / 2) & (e > 0)
    tie_dn = (h == (r64 + dn.astype(f64)) / 2) & (e < 0)
    return np.where(tie_up, up, np.where(tie_dn, dn, r)).astype(f32)


def ref_adagrad_dense(p, g, ss, clr, eps, gs=1.0):
    """float32 emulation of adagrad_kernel, one operation per rounding:
        gj = fl(g * gs); s = fma(gj, gj, ss); p = fma(-clr, fl(gj / fl(sqrt(s) + eps)), p).
    The products gj * gj and clr * u are exact in float64 (48 bits; clr a power of two); each
    fma's one rounding is round_sum_f32's (ref_adagrad_fraction is the proof).  Returns
    (p, state_sum)."""
    assert np.frexp(f32(clr))[0] == 0.5
    gj = (g.numpy().astype(f32) * f32(gs)).astype(f32)
    s = round_sum_f32(gj.astype(f64) * gj.astype(f64), ss.numpy().astype(f64))
    den = np.sqrt(s) + f32(eps)
    u = gj / den
    assert den.dtype == f32 and u.dtype == f32
    pn = round_sum_f32(-f64(f32(clr)) * u.astype(f64), p.numpy().astype(f64))
    return torch.from_numpy(pn), torch.from_numpy(s)


def _round_f32(fr):
    """A Fraction rounded once to float32, to nearest even, in integer arithmetic."""
    if fr == 0:
        return f32(0)
    sign, a = (-1, -fr) if fr < 0 else (1, fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    q = Fraction(2) ** (max(e, -126) - 23)  # the float32 spacing at a
    k, rem = divmod(a, q)
    k = int(k)
    if rem * 2 > q or (rem * 2 == q and k % 2):
        k += 1
    return f32(sign * float(k * q))


def ref_adagrad_fraction(p, g, ss, clr, eps, gs=1.0):
    """The same with both fmas in fractions.Fraction (exact), rounded once each.  For small n."""
    gj = (g.numpy().astype(f32) * f32(gs)).astype(f32)
    P, S = [], []
    for i in range(len(gj)):
        s = _round_f32(Fraction(float(gj[i])) ** 2 + Fraction(float(ss[i])))
        u = gj[i] / (np.sqrt(s) + f32(eps))
        assert u.dtype == f32
        pn = _round_f32(Fraction(float(p[i])) - Fraction(float(f32(clr))) * Fraction(float(u)))
        S.append(s)
        P.append(pn)
    return torch.tensor(np.array(P, dtype=f32)), torch.tensor(np.array(S, dtype=f32))


# ------------------------------------------------------------------- fill streams ----
_C1, _C2, _C3 = (np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9),
                 np.uint64(0x94D049BB133111EB))
FILL_NS = [1, 257, 4194304 + 3]
FILL_SEEDS = [1234, 2 ** 63 + 5]


def splitmix64(z):
    """splitmix64's output function on a uint64 array (wrapping arithmetic)."""
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64)) + _C1
    z = (z ^ (z >> np.uint64(30))) * _C2
    z = (z ^ (z >> np.uint64(27))) * _C3
    return z ^ (z >> np.uint64(31))


def fill_stream(n, seed, first=0):
    """The 64-bit words of elements [first, first + n) of the seed's stream."""
    key = splitmix64(np.uint64(seed & (2 ** 64 - 1)))[0]
    j = np.arange(n, dtype=np.uint64) + np.uint64(first)
    return splitmix64(key ^ j)


def ref_uniform_fill(n, lo, hi, seed, first=0):
    """uniform_fill_kernel: u = (x >> 40) * 2^-24 (exact), out = lo + (hi - lo) * u.  For a
    power-of-two width the product is exact, so the one rounding is the add's whether or not
    the compiler contracts it into an fma."""
    width = f32(f32(hi) - f32(lo))
    assert np.frexp(width)[0] == 0.5, "width must be a power of two"
    u = (fill_stream(n, seed, first) >> np.uint64(40)).astype(f32) * f32(2.0 ** -24)
    return torch.from_numpy((f32(lo) + width * u).astype(f32))


def mulhi64(x, hi):
    """(x * hi) >> 64 for a uint64 array x and a Python int hi < 2^64, by 32-bit limbs."""
    m32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    x0, x1 = x & m32, x >> s32
    h0, h1 = np.uint64(hi & 0xFFFFFFFF), np.uint64(hi >> 32)
    t = x0 * h0
    t = x1 * h0 + (t >> s32)
    w1, w2 = t & m32, t >> s32
    w1 = x0 * h1 + w1
    return x1 * h1 + w2 + (w1 >> s32)


def ref_uniform_int(n, hi, seed, exact_python=False):
    """uniform_int_kernel: floor(x * hi / 2^64) as int64 (exact_python: in Python integers)."""
    x = fill_stream(n, seed)
    if exact_python:
        return torch.tensor([(int(v) * hi) >> 64 for v in x], dtype=torch.int64)
    return torch.from_numpy(mulhi64(x, hi).astype(np.int64))


# --------------------------------------------------------------------- QR / CSR ----
def qr_split_values(c):
    """Indices around the places where the float32 quotient and integer division part."""
    v = [0, 1, c - 1, c, c + 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 1]
    for k in (2 ** 24 // c + 3, 2 ** 27 // c + 1, (2 ** 31 - 1) // c - 1):
        v += [k * c - 1, k * c, k * c + 1]
    return sorted({x for x in v if 0 <= x <= 2 ** 31 - 1})


def ref_csr(table_offsets, table_nnz):
    out, base = [], 0
    for o, n in zip(table_offsets, table_nnz):
        out.append(o.long() + base)
        base += int(n)
    return torch.cat(out + [torch.tensor([base])])
