"""Exact-arithmetic cases and references for the embedding side (lookup, sorted backward with
the fused optimizers, per-sample-weight and expanded gradients).

The backward sorts the lookups by (row, position), so its summation order is fixed; with
integer-valued operands every order gives the same bits anyway, the Kahan compensation is
identically zero, and - division and square root being the correctly rounded IEEE ones - SGD,
dense accumulation, fp16 SGD and row-wise Adagrad can all be required to equal a CPU reference
bit for bit.  This module builds

  * run-structured CSR batches (run_csr): the caller gives, per table, the lookups per distinct
    row in row order, so where every run falls against the 16- and 64-lookup block edges of the
    sorted array is known on the host (alignment_classes names what a sorted array contains);
  * integer operands (make_operands) with the conditions under which fp32 is exact
    (exact_conditions_ok: conditions of a test, not tolerances);
  * the references, on the touched rows only (a 1.1 M-row case stays small);
  * models of kernel bugs on the lookup list (BUG_MODELS), each of which must change a result.

Plain helper module (no GPU needed), like exact_inputs.py; proved in test_exact_tbe_cpu.py."""
import numpy as np
import torch

from exact_inputs import int_matrix

ERR_INDEX, ERR_TABLE_CAP = 1, 2  # ops.TBE_ERR_INDEX / TBE_ERR_TABLE_CAP
CH, LONG_CH = 16, 64              # sorted lookups per block (tbe_bwd_roles.hpp CH / kLongCH)
SEG_CAP, RANK_SORT_MAX = 4096, 512  # per-table LDS sort: lookups per table, rank-sort limit


def dispatch(D, aligned=True):
    """(VW, LPB, MAXV) of the kernel launch_fwd / launch_bwd choose (MAXV: chunks per lane,
    rounded up to the instantiated 1, 2, 4 or 8); MAXV > 8 is refused."""
    vw = 4 if (aligned and D % 4 == 0) else 1
    nchunks = D // vw
    lpb = 1
    while lpb < nchunks and lpb < 64:
        lpb <<= 1
    maxv = -(-nchunks // lpb)
    return vw, lpb, 1 << (maxv - 1).bit_length()


def digit_class(total_rows):
    """(digit bits, passes) of the device-wide sort over ``total_rows`` (tiled_digit_bits)."""
    bits = max(1, int(total_rows).bit_length())  # keys in [0, total_rows]
    db = 10 if (bits + 9) // 10 < (bits + 7) // 8 else 8
    return db, -(-bits // db)


class Case:
    """One table-batched CSR batch and everything the host knows about it.  Per lookup:
    ``table`` and ``bag`` (t*B + b; -1 outside every bag), ``row`` (global row; -1 when the
    index is out of range or the lookup is outside every bag) and ``valid``.  ``runs``: the
    (start, length, global row) of every run of the array sorted by (row, position), the
    invalid and outside lookups after the last run."""

    def __init__(self, name, rows, B, indices, offsets, idx_dtype=torch.int32,
                 off_dtype=torch.int32, runs_spec=None):
        self.name, self.rows, self.B, self.T = name, list(rows), int(B), len(rows)
        self.indices = np.asarray(indices, dtype=np.int64)
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.idx_dtype, self.off_dtype = idx_dtype, off_dtype
        self.row_base = np.concatenate([[0], np.cumsum(self.rows)]).astype(np.int64)
        self.total_rows = int(self.row_base[-1])
        self.N = N = self.indices.size
        nb = self.T * self.B
        assert self.offsets.size == nb + 1 and (np.diff(self.offsets) >= 0).all()
        assert 0 <= self.offsets[0] and self.offsets[-1] <= N
        pos = np.arange(N)
        bag = np.searchsorted(self.offsets, pos, side="right") - 1
        inside = (pos >= self.offsets[0]) & (pos < self.offsets[-1])
        self.bag = np.where(inside, bag, -1)
        self.table = np.where(inside, np.minimum(bag, nb - 1) // self.B, -1)
        nrows_of = np.asarray(self.rows + [0])[self.table]
        self.valid = inside & (self.indices >= 0) & (self.indices < nrows_of)
        self.row = np.where(self.valid, self.row_base[self.table] + self.indices, -1)
        self.flag = ERR_INDEX if (inside & ~self.valid).any() else 0
        self.bag_len = np.diff(self.offsets)
        self.table_lookups = [int(self.offsets[(t + 1) * B] - self.offsets[t * B])
                              for t in range(self.T)]
        self.max_table = max(self.table_lookups)
        self.keys = np.where(self.valid, self.row, self.total_rows)  # sentinel = total_rows
        self.runs = runs_of(np.sort(self.keys, kind="stable"), self.total_rows)
        self.runs_spec = runs_spec

    def device_csr(self, dev):
        return (torch.from_numpy(self.indices).to(self.idx_dtype).to(dev),
                torch.from_numpy(self.offsets).to(self.off_dtype).to(dev),
                torch.from_numpy(self.row_base).to(dev))

    def sorted_keys(self, variant="global"):
        """The sorted key array as a sort variant leaves it.  'global' (device-wide): every
        sentinel after the last run.  'per_table' (LDS and tiled sorts): the lookups outside
        every bag stay where they are, each table's invalid lookups end its own range."""
        if variant == "global":
            return np.sort(self.keys, kind="stable")
        out = np.full(self.N, self.total_rows, dtype=np.int64)
        for t in range(self.T):
            a, e = self.offsets[t * self.B], self.offsets[(t + 1) * self.B]
            out[a:e] = np.sort(self.keys[a:e], kind="stable")
        return out

    def with_dtypes(self, idx_dtype, off_dtype):
        return Case(self.name, self.rows, self.B, self.indices, self.offsets, idx_dtype,
                    off_dtype, self.runs_spec)


def runs_of(sorted_keys, sentinel):
    """(start, length, key) of every run of equal non-sentinel keys."""
    k = np.asarray(sorted_keys)
    if k.size == 0:
        return np.zeros((0, 3), dtype=np.int64)
    starts = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    lens = np.diff(np.concatenate([starts, [k.size]]))
    keep = k[starts] != sentinel
    return np.stack([starts[keep], lens[keep], k[starts][keep]], 1).astype(np.int64)


def _bag_cuts(n, B, rng, empty_ends):
    """Offsets (B + 1) of B bags over n lookups: variable lengths, empty bags among them -
    the first and the last bag of the table too when ``empty_ends`` (B >= 3)."""
    if B >= 3 and empty_ends:
        inner = np.sort(rng.integers(0, n + 1, B - 3))
        if B >= 5 and n > 0:
            inner[len(inner) // 2] = inner[len(inner) // 2 - 1]  # an empty bag in the middle
            inner = np.sort(inner)
        return np.concatenate([[0, 0], inner, [n, n]])
    return np.concatenate([[0], np.sort(rng.integers(0, n + 1, B - 1)), [n]])


def run_csr(name, tables, B, seed, lead=0, trail=0, invalid=(), idx_dtype=torch.int32,
            off_dtype=torch.int32, empty_ends=True):
    """Run-structured CSR.  ``tables``: per table (nrows, run_lengths): lookups per distinct
    row, in row order (fewer runs than rows: a sorted random subset of the rows is used, the
    others stay untouched; no runs: a table without lookups).  Each table's lookups are dealt
    to its B bags at random positions, bag lengths variable with empty bags.  ``lead`` /
    ``trail``: lookups before offsets[0] / after offsets[T*B] (outside every bag; their
    indices look valid).  ``invalid``: (table, position in the table's lookups, value) -
    out-of-range or negative indices inserted there (extra lookups: the runs stay as given)."""
    rng = np.random.default_rng(seed)
    rows = [int(n) for n, _ in tables]
    idx, off, spec, base, start = [], [lead], [], 0, 0
    for t, (nrows, runs) in enumerate(tables):
        runs = [int(r) for r in runs]
        assert len(runs) <= nrows and all(r > 0 for r in runs)
        which = np.sort(rng.choice(nrows, len(runs), replace=False)) if runs else np.zeros(0, int)
        li = rng.permutation(np.repeat(which, runs)).tolist()
        for tt, p, v in sorted(x for x in invalid if x[0] == t):
            assert v < 0 or v >= nrows
            li.insert(min(p, len(li)), v)
        for r, n in zip(which, runs):
            spec.append((start, n, base + int(r)))
            start += n
        cuts = _bag_cuts(len(li), B, rng, empty_ends)
        off.extend((off[-1] - cuts[0] + cuts[1:]).tolist())
        idx.extend(li)
        base += nrows
    indices = [1 % rows[0]] * lead + idx + [0] * trail
    return Case(name, rows, B, indices, off, idx_dtype, off_dtype,
                np.asarray(spec, dtype=np.int64).reshape(-1, 3))


def bags_csr(name, rows, bag_lengths, seed, invalid=(), idx_dtype=torch.int32,
             off_dtype=torch.int32, distinct=False):
    """CSR with the given bag lengths (one list per table, each of B entries), uniformly
    random valid indices (``distinct``: no row twice in a table, so every bag of length 1
    reads a row of its own); ``invalid``: (position in the index array, value)."""
    rng = np.random.default_rng(seed)
    B = len(bag_lengths[0])
    idx, off = [], [0]
    for nrows, lens in zip(rows, bag_lengths):
        assert len(lens) == B
        n = int(sum(lens))
        idx.extend((rng.permutation(nrows)[:n] if distinct else rng.integers(0, nrows, n)).tolist())
        off.extend((off[-1] + np.cumsum(lens)).tolist())
    for p, v in invalid:
        idx[p] = v
    return Case(name, rows, B, idx, off, idx_dtype, off_dtype)


# ------------------------------------------------------------- block alignment ----
ALIGN_CLASSES = ("one_block_at_edge", "k_blocks_edge_to_edge", "mid_to_edge", "edge_to_mid",
                 "mid_to_mid_3_blocks", "single_first_of_block", "single_last_of_block",
                 "end_and_start_in_one_block", "long_run", "run_then_sentinel")


def alignment_classes(sorted_keys, sentinel, ch, lpb):
    """Which of ALIGN_CLASSES the runs of a sorted key array show against blocks of ``ch``
    lookups; ``lpb``: 'long_run' spans more than max(lpb, 16) + 2 blocks (the combine's
    kend probe then takes a second round and its partial loads a second batch)."""
    k = np.asarray(sorted_keys)
    runs = runs_of(k, sentinel)
    got = set()
    multi_end_blocks, multi_start_blocks = set(), set()
    for s, n, _ in runs:
        e = s + n  # [s, e)
        b0, b1 = s // ch, (e - 1) // ch
        nblk = b1 - b0 + 1
        s_edge, e_edge = s % ch == 0, (e % ch == 0 or e == k.size)
        if n == ch and s_edge:
            got.add("one_block_at_edge")
        if s_edge and e % ch == 0 and n >= 2 * ch:
            got.add("k_blocks_edge_to_edge")
        if not s_edge and e % ch == 0 and nblk >= 1 and n > 1:
            got.add("mid_to_edge")
        if s_edge and not e_edge and nblk >= 2:
            got.add("edge_to_mid")
        if not s_edge and not e_edge and nblk >= 3:
            got.add("mid_to_mid_3_blocks")
        if n == 1 and s % ch == 0:
            got.add("single_first_of_block")
        if n == 1 and s % ch == ch - 1:
            got.add("single_last_of_block")
        if nblk > max(lpb, 16) + 2:
            got.add("long_run")
        if nblk >= 2:
            multi_start_blocks.add(b0)
            multi_end_blocks.add(b1)
        if e < k.size and k[e] == sentinel:
            got.add("run_then_sentinel")
    if multi_end_blocks & multi_start_blocks:
        got.add("end_and_start_in_one_block")
    return got


def structure_runs():
    """Run lengths (in sorted order) holding every class of ALIGN_CLASSES at blocks of 64
    and of 16 lookups: the list starts at a multiple of 64."""
    runs = []
    pos = lambda: sum(runs)  # noqa: E731

    def to(ch, r):  # length-1 runs up to position = r (mod ch)
        while pos() % ch != r:
            runs.append(1)

    for ch in (64, 16):
        to(ch, 0)
        runs.append(ch)            # one block, edge to edge
        runs.append(3 * ch)        # k blocks, edge to edge
        runs.append(1)             # a single lookup first in its block ...
        runs.append(ch - 1)        # ... then mid-block to the edge
        runs.append(ch + 5)        # edge to mid-block (2 blocks)
        runs.append(3 * ch + 2)    # mid to mid over 4 blocks, starting where the last ended
        to(ch, ch - 1)
        runs.append(1)             # a single lookup last in its block
    to(64, 0)
    runs.append(36 * 64)           # > max(LPB, 16) + 2 blocks at either block length
    runs.append(7)                 # the last valid run: ends mid-block, sentinels follow
    return runs


# -------------------------------------------------------------------- operands ----
class Operands:
    """Integer operands of one (case, D): grad_out G [B, T, D], per-sample weights psw [N]
    (or None), and on the touched rows ``urows`` (sorted global rows): W0u, the dense
    accumulator acc0u and the momentum mom0u."""


def _separate_neighbours(G, vals):
    """No bag's gradient row equals that of the bag before it or of the same sample in the
    table before it (a gradient read from the neighbour must show): component 0 cycles
    through ``vals`` until it differs."""
    B, T, _ = G.shape
    for b in range(B):
        for t in range(T):
            for _ in range(len(vals)):
                same_b = b > 0 and torch.equal(G[b, t], G[b - 1, t])
                same_t = t > 0 and torch.equal(G[b, t], G[b, t - 1])
                if not (same_b or same_t):
                    break
                G[b, t, 0] = vals[(vals.index(float(G[b, t, 0])) + 1) % len(vals)]
    return G


def _balance_long_runs(case, G, psw, min_run=512):
    """A row with hundreds of lookups in B <= 64 bags takes every bag's gradient row many
    times over, and the square of its coalesced gradient would leave the integers fp32
    holds (condition 3).  For each table's longest run (from ``min_run`` lookups), the
    signs of components 1.. of the table's gradient rows are chosen bag by bag so that the
    row's running sum stays small; component 0 keeps its random sign."""
    w = np.ones(case.N) if psw is None else psw.numpy().astype(np.float64)
    for t in range(case.T):
        mine = case.runs[(case.runs[:, 2] >= case.row_base[t]) &
                         (case.runs[:, 2] < case.row_base[t + 1])]
        if mine.size == 0 or mine[:, 1].max() < min_run:
            continue
        row = mine[np.argmax(mine[:, 1]), 2]
        coef = np.zeros(case.B)
        hit = case.row == row
        np.add.at(coef, case.bag[hit] % case.B, w[hit])
        s = torch.zeros(G.shape[2] - 1, dtype=torch.float64)
        for b in range(case.B):
            v = coef[b] * G[b, t, 1:].abs().double()
            plus = (s + v).abs() <= (s - v).abs()
            G[b, t, 1:] = torch.where(plus, G[b, t, 1:].abs(), -G[b, t, 1:].abs())
            s = torch.where(plus, s + v, s - v)
    return G


def make_operands(case, D, weighted, seed, gmax=8, lr=2.0 ** -4, eps=2.0 ** -10):
    gen = torch.Generator().manual_seed(seed)
    o = Operands()
    o.D, o.lr, o.eps, o.gmax = D, float(lr), float(eps), gmax
    vals = [float(v) for v in range(-gmax, gmax + 1) if v != 0]
    o.psw = int_matrix((case.N,), -3, 3, gen) if weighted else None
    o.G = _balance_long_runs(case, int_matrix((case.B, case.T, D), -gmax, gmax, gen), o.psw)
    o.G = _separate_neighbours(o.G, vals)
    o.urows = np.unique(case.row[case.valid])
    n = o.urows.size
    o.W0u = int_matrix((n, D), -64, 64, gen, nonzero=False)
    o.acc0u = int_matrix((n, D), -64, 64, gen)
    o.mom0u = int_matrix((n,), 0, 8, gen, nonzero=False)
    return o


def operands_for(case, D, weighted, seed, adagrad=True, zero_row=None, **kw):
    """make_operands with the largest gradient range of [-8, 8], [-4, 4], [-2, 2], [-1, 1]
    under which the exactness conditions hold (long runs at a large D need a small one for
    Adagrad's sum of squares); ``zero_row``: cancel_row on that global row.  No range
    fitting is a bug in the case."""
    msg = ""
    for gmax in (8, 4, 2, 1):
        o = make_operands(case, D, weighted, seed, gmax=gmax, **kw)
        if zero_row is not None:
            cancel_row(case, o, zero_row)
        ok, msg = exact_conditions_ok(case, o, adagrad,
                                      () if zero_row is None else (zero_row,))
        if ok:
            return o
    raise AssertionError(f"{case.name} D={D}: {msg}")


def lookup_values(case, o):
    """Per lookup: its weight (1 unweighted) and the grad_out row of its bag (zeros outside
    every bag), fp64."""
    w = np.ones(case.N) if o.psw is None else o.psw.numpy().astype(np.float64)
    g = np.zeros((case.N, o.D))
    ins = case.bag >= 0
    t, b = case.bag[ins] // case.B, case.bag[ins] % case.B
    g[ins] = o.G.numpy().astype(np.float64)[b, t]
    return w, g


def coalesce(urows, rows, values):
    """fp64 index_add of ``values`` [n, D] into the rows ``rows`` (global), laid out on
    ``urows``; rows outside urows raise."""
    slot = np.searchsorted(urows, rows)
    assert (slot < urows.size).all() and (urows[slot] == rows).all()
    out = torch.zeros(urows.size, values.shape[1], dtype=torch.float64)
    out.index_add_(0, torch.from_numpy(slot), torch.from_numpy(np.ascontiguousarray(values)))
    return out


def coalesced_grad(case, o, absolute=False):
    """gsum[urows]: sum over the valid lookups of weight * grad_out row (``absolute``: of
    |weight| * |grad_out row|, the bound of every partial sum)."""
    w, g = lookup_values(case, o)
    v = case.valid
    vals = (np.abs(w[v, None]) * np.abs(g[v])) if absolute else w[v, None] * g[v]
    return coalesce(o.urows, case.row[v], vals)


def exact_conditions_ok(case, o, adagrad=True, zero_rows=()):
    """The conditions under which every fp32 operation of the backward is exact (Adagrad:
    up to its five roundings), checked on the data: (ok, message).
      1. sum over a run of |w_l| |g| < 2^24 (every partial sum is a representable integer);
      2. (|W0| + lr max|gsum|) / min(lr, 1) < 2^24 (w - lr g is a representable multiple of lr);
      3. Adagrad: sum_d gsum^2 < 2^24 on every touched row;
      4. neighbouring bags (and the same sample's bags of neighbouring tables) have different
         gradient rows, and a touched row's coalesced gradient is zero exactly where
         ``zero_rows`` (global rows) says so."""
    lim = 2.0 ** 24
    gs, ga = coalesced_grad(case, o), coalesced_grad(case, o, absolute=True)
    if ga.numel() and float(ga.max()) >= lim:
        return False, f"run sum bound {float(ga.max())} >= 2^24"
    wmax = max(float(o.W0u.abs().max()) if o.W0u.numel() else 0.0,
               float(o.acc0u.abs().max()) if o.acc0u.numel() else 0.0)
    gmx = float(ga.max()) if ga.numel() else 0.0
    if (wmax + o.lr * gmx) / min(o.lr, 1.0) >= lim or wmax + gmx >= lim:
        return False, f"update bound (|W0| {wmax}, |gsum| {gmx}, lr {o.lr}) >= 2^24"
    if adagrad and gs.numel() and float((gs ** 2).sum(1).max()) >= lim:
        return False, f"Adagrad sum of squares {float((gs ** 2).sum(1).max())} >= 2^24"
    G = o.G
    if case.B > 1 and bool((G[1:] == G[:-1]).all(2).any()):
        return False, "two neighbouring bags have the same gradient row"
    if case.T > 1 and bool((G[:, 1:] == G[:, :-1]).all(2).any()):
        return False, "a sample's gradient rows of two neighbouring tables are equal"
    zero = (gs == 0).all(1).numpy()
    want = np.isin(o.urows, np.asarray(list(zero_rows), dtype=np.int64))
    if (zero != want).any():
        return False, f"coalesced gradient zero on rows {o.urows[zero].tolist()}, " \
                      f"meant {sorted(zero_rows)}"
    return True, ""


def cancel_row(case, o, row):
    """Make the coalesced gradient of global ``row`` cancel: it must have exactly two
    lookups, in different bags; the second bag's gradient row becomes minus the first's
    (and the two per-sample weights equal)."""
    p = np.flatnonzero(case.row == row)
    assert p.size == 2 and case.bag[p[0]] != case.bag[p[1]], (row, p)
    (t0, b0), (t1, b1) = [(case.bag[q] // case.B, case.bag[q] % case.B) for q in p]
    o.G[b1, t1] = -o.G[b0, t0]
    if o.psw is not None:
        o.psw[p[1]] = o.psw[p[0]]


# ------------------------------------------------------------------ references ----
def ref_sgd(W0u, gsum, lr):
    return (W0u.double() - lr * gsum).float()


def ref_sgd_f16(W0u_half, gsum, lr):
    """The exact value (representable in fp32 under condition 2) rounded once to fp16."""
    return (W0u_half.double() - lr * gsum).float().half()


def ref_dense(acc0u, gsum):
    return (acc0u.double() + gsum).float()


def ref_adagrad(W0u, mom0u, gsum, D, lr, eps):
    """numpy float32 emulation of finalize_row, one operation per rounding; returns (W, mom)."""
    f32 = np.float32
    g = gsum.numpy()
    sq = (g * g).sum(1)  # exact integer (condition 3)
    assert (sq < 2.0 ** 24).all()
    mean = sq.astype(f32) / f32(D)
    mnew = mom0u.numpy().astype(f32) + mean
    denom = np.sqrt(mnew) + f32(eps)
    assert mnew.dtype == f32 and denom.dtype == f32
    with np.errstate(invalid="ignore", divide="ignore"):
        u = g.astype(f32) / denom[:, None]
    assert u.dtype == f32
    w = (W0u.numpy().astype(np.float64) - lr * u.astype(np.float64)).astype(f32)
    return torch.from_numpy(w), torch.from_numpy(mnew)


def ref_forward(case, o, Wu):
    """Pooled sums [B, T, D] over the valid lookups, fp64 -> fp32; ``Wu``: rows on o.urows."""
    w = np.ones(case.N) if o.psw is None else o.psw.numpy().astype(np.float64)
    v = case.valid
    slot = np.searchsorted(o.urows, case.row[v])
    vals = w[v, None] * Wu.numpy().astype(np.float64)[slot]
    out = torch.zeros(case.T * case.B, Wu.shape[1], dtype=torch.float64)
    out.index_add_(0, torch.from_numpy(case.bag[v]), torch.from_numpy(vals))
    return out.view(case.T, case.B, -1).permute(1, 0, 2).contiguous().float()


def ref_psw_grad(case, o, Wu):
    """Per lookup <grad_out row of its bag, its weight row>; 0 for invalid / outside lookups."""
    _, g = lookup_values(case, o)
    v = case.valid
    out = np.zeros(case.N)
    slot = np.searchsorted(o.urows, case.row[v])
    out[v] = (g[v] * Wu.numpy().astype(np.float64)[slot]).sum(1)
    return torch.from_numpy(out).float()


def ref_expand_grad(case, o):
    """Per lookup weight * grad_out row of its bag; zeros outside every bag (the kernel does
    not see the indices: an out-of-range lookup inside a bag gets its bag's row)."""
    w, g = lookup_values(case, o)
    return torch.from_numpy(w[:, None] * g).float()


def bits_equal(a, b):
    """Bitwise equality of two fp32 (int32 view) or fp16 (int16 view) tensors: NaN rows and
    signed zeros compare as stored."""
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    bits = lambda x: x.contiguous().view(it)  # noqa: E731
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def untouched_intact(before, after, urows):
    """Every row outside ``urows`` keeps its bits."""
    keep = torch.ones(before.shape[0], dtype=torch.bool, device=before.device)
    keep[torch.as_tensor(urows, device=before.device)] = False
    return bits_equal(before[keep], after[keep])


# ------------------------------------------------------------------ bug models ----
class Lookups:
    """The valid lookups of a case in sorted order, as a kernel's block pass sees them:
    row, weight, gradient row and sorted position; the models below edit this list."""

    def __init__(self, case, o):
        w, g = lookup_values(case, o)
        order = np.argsort(case.keys, kind="stable")
        order = order[case.valid[order]]
        self.case, self.o = case, o
        self.p, self.row, self.w, self.g = order, case.row[order], w[order], g[order]
        self.spos = np.arange(order.size)  # valid lookups come first in the sorted array

    def gsum(self):
        return coalesce(self.o.urows, self.row, self.w[:, None] * self.g)

    def keep(self, mask):
        self.p, self.row, self.w, self.g, self.spos = (x[mask] for x in
                                                      (self.p, self.row, self.w, self.g, self.spos))
        return self


def _run_end_mask(lk):
    return np.concatenate([lk.row[1:] != lk.row[:-1], [True]])


def _drop(lk, i):
    m = np.ones(lk.row.size, dtype=bool)
    m[i] = False
    return lk.keep(m)


def bug_drop_block_first(lk, ch=CH):
    return _drop(lk, np.flatnonzero(lk.spos % ch == 0)[-1])


def bug_drop_block_last(lk, ch=CH):
    return _drop(lk, np.flatnonzero(lk.spos % ch == ch - 1)[0])


def bug_drop_run_end(lk, ch=CH):
    ends = np.flatnonzero(_run_end_mask(lk))
    return _drop(lk, ends[len(ends) // 2])


def bug_apply_twice(lk, ch=CH):
    i = lk.row.size // 2
    for name in ("p", "row", "w", "spos"):
        setattr(lk, name, np.insert(getattr(lk, name), i, getattr(lk, name)[i]))
    lk.g = np.insert(lk.g, i, lk.g[i], axis=0)
    return lk


def _regrad(lk, i, bag):
    B = lk.case.B
    lk.g[i] = lk.o.G.numpy().astype(np.float64)[bag % B, bag // B]
    return lk


def bug_neighbour_bag(lk, ch=CH):
    i = lk.row.size // 3
    bag = lk.case.bag[lk.p[i]]
    b = bag % lk.case.B
    return _regrad(lk, i, bag + 1 if b + 1 < lk.case.B else bag - 1)


def bug_neighbour_table(lk, ch=CH):
    i = lk.row.size // 3
    bag, B, T = lk.case.bag[lk.p[i]], lk.case.B, lk.case.T
    return _regrad(lk, i, bag + B if bag // B + 1 < T else bag - B)


def bug_ignore_weight(lk, ch=CH):
    i = int(np.flatnonzero(lk.w != 1.0)[0])
    lk.w[i] = 1.0
    return lk


def bug_omit_last_partial(lk, ch=CH):
    """The partial sum of the last block of a run crossing a block edge is never added."""
    ends = np.flatnonzero(_run_end_mask(lk))
    starts = np.concatenate([[0], ends[:-1] + 1])
    for s, e in zip(starts, ends):
        if lk.spos[s] // ch != lk.spos[e] // ch:
            return lk.keep(~((lk.row == lk.row[s]) & (lk.spos // ch == lk.spos[e] // ch)))
    raise AssertionError("no run crosses a block edge")


def bug_invalid_to_last_row(lk, ch=CH):
    """An out-of-range lookup clamped to its table's last row instead of being skipped."""
    c = lk.case
    p = int(np.flatnonzero((c.bag >= 0) & ~c.valid)[0])
    t = c.table[p]
    w, g = lookup_values(c, lk.o)
    lk.row = np.append(lk.row, c.row_base[t + 1] - 1)
    lk.w, lk.g = np.append(lk.w, w[p]), np.vstack([lk.g, g[p][None]])
    lk.p, lk.spos = np.append(lk.p, p), np.append(lk.spos, lk.spos[-1] + 1)
    return lk


BUG_MODELS = {"drop_block_first": bug_drop_block_first, "drop_block_last": bug_drop_block_last,
              "drop_run_end": bug_drop_run_end, "apply_twice": bug_apply_twice,
              "neighbour_bag": bug_neighbour_bag, "neighbour_table": bug_neighbour_table,
              "ignore_weight": bug_ignore_weight, "omit_last_partial": bug_omit_last_partial,
              "invalid_to_last_row": bug_invalid_to_last_row}


# ----------------------------------------------------------------- named cases ----
IDX_PAIRS = [(torch.int32, torch.int32), (torch.int32, torch.int64),
             (torch.int64, torch.int32), (torch.int64, torch.int64)]


def skewed_case():
    """Backward dispatch on D: tables of 1, 3 and 40 rows, a few hundred lookups each, so
    every D sees runs over many blocks; two invalid indices, lookups outside the bags."""
    return run_csr("skewed", [(1, [150]), (3, [90, 1, 120]), (40, [7, 1, 33, 2, 64, 16, 5, 1,
                                                                      20, 48, 3, 9])],
                   B=24, seed=11, lead=2, trail=3, invalid=[(1, 5, 3), (2, 40, -1)])


def structure_case():
    """Backward run structure: a 1-row table whose run is the whole table (64 lookups: the
    next table starts at a block edge), the structure_runs() list, then the invalid indices
    (last table) and lookups outside every bag, so sentinels follow the last run in every
    sort variant.  N is no multiple of 16."""
    runs = structure_runs()
    rows2 = len(runs) + 5
    last = runs[-1]
    c = run_csr("structure", [(1, [64]), (rows2, runs[:-1]), (2, [last, 2])], B=64, seed=12,
                trail=3, invalid=[(2, 4, 6), (2, 0, -2)])
    return c


def small_n_cases():
    """N = 1, N < 16 and N a multiple of both block lengths."""
    return [run_csr("n1", [(2, [1])], B=1, seed=13, empty_ends=False),
            run_csr("n7", [(3, [4, 3])], B=3, seed=14, empty_ends=False),
            run_csr("n128", [(1, [40]), (9, [30, 1, 17, 20, 20])], B=8, seed=15)]


def cancel_case():
    """A touched row whose two lookups cancel (cancel_row on the operands), between runs."""
    return run_csr("cancel", [(5, [3, 2, 4]), (4, [20, 5])], B=6, seed=16, empty_ends=False)


def sort_case(kind, idx_dtype=torch.int32, off_dtype=torch.int32):
    """Variable-length batches for the sort variants: empty bags, one empty table,
    offsets[0] > 0, trailing lookups and invalid indices.  kind: 'rank' (tables <= 512
    lookups), 'radix' (a table of 513..4096), 'tiled' (a table of 4097..8192 beside a small
    and an empty table), 'tiled10' (two tables of two tiles and 12 680 lookups in all: at
    D = 128 the workspace then holds the tiled sort's 10-bit histograms), or 'rows<n>'
    (about n rows in all, for the device-wide sort)."""
    rng = np.random.default_rng(len(kind) + 100)

    def runs(n_runs, total):
        r = np.ones(n_runs, dtype=np.int64)
        extra = rng.integers(0, n_runs, total - n_runs)
        np.add.at(r, extra // 3 * 3 % n_runs, 1)  # skewed: a third of the rows take it all
        return r.tolist()

    kw = dict(B=32, seed=17, lead=3, trail=5, idx_dtype=idx_dtype, off_dtype=off_dtype)
    if kind == "rank":
        tabs = [(50, runs(30, 300)), (7, []), (200, runs(90, 500))]
        inv = [(0, 17, 50), (2, 100, -1)]
    elif kind == "radix":
        tabs = [(300, runs(200, 513)), (7, []), (1000, runs(400, 3000))]
        inv = [(0, 17, 10 ** 6), (2, 100, -1)]
    elif kind == "tiled":
        tabs = [(90, runs(60, 200)), (5, []), (3000, runs(900, 4200))]
        inv = [(0, 17, 90), (2, 4100, -7)]
    elif kind == "tiled10":
        tabs = [(90, runs(80, 4489)), (5, []), (3000, runs(1500, 8179))]
        inv = [(0, 17, 90), (2, 4100, -7)]
    else:
        n = int(kind[4:])
        a, b = n // 3, n - n // 3 - 4
        tabs = [(a, runs(min(a, 60), 200)), (4, []), (b, runs(min(b, 150), 400))]
        inv = [(0, 17, a), (2, 100, -1)]
    return run_csr("sort_" + kind, tabs, invalid=inv, **kw)


GLOBAL_ROW_CLASSES = {200: (8, 1), 600: (10, 1), 5000: (8, 2), 70000: (10, 2),
                      1100000: (8, 3)}
