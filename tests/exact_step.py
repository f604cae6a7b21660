"""An exact DLRM and the fp64 reference of ONE WHOLE training step on it (plain helper module:
numpy / torch on the CPU, no GPU import; proved in test_exact_step_cpu.py, used against the
engine in test_gpu_exact_step.py).

The model follows linear16_ref.tiny_exact_model - tables, X and the non-head weights are small
integers, a non-head weight row holds a few +-1 - at sizes that reach the trainer's fused paths
(D = 16, a 13 -> 32 -> 16 bottom chain, a three-layer top MLP, B a power of two).  Only the head
differs: its weights are multiples of 2 B >= 128 over integer activations, so every logit is 0
or at least 128 in magnitude - the anchors of exact_head.py, where sigmoid follows from IEEE
arithmetic alone (p = 0.5, 1, 0).  dz is then 0 or +-1/(2 B) (BCE; +-1/(4 B) for MSE), the
head's input gradient an integer (or a dyadic fraction), and every value of the backward a
multiple of one power of two.

Exactness is exact_inputs.py's criterion, checked on the data by Ledger for EVERY reduction of
the step (forward GEMMs with the folded bias, interaction, dgrad, wgrad, bias sums, interaction
backward, coalesced row gradients): with the terms in units of their common quantum 2^-k, the
sum of their magnitudes stays below 2^24, so every partial sum in any order is a representable
fp32 value.  The averaging and W-rank factors are powers of two.  With power-of-two learning
rates every updated value is checked to be representable, so an fp32 step - whatever its
summation order, fusion or contraction - equals this reference BIT FOR BIT.  Adagrad's square
root and division are correctly rounded IEEE operations: the row-wise rule is
exact_tbe.ref_adagrad (finalize_row), the element-wise one exact_adagrad.ref_adagrad_elem, the
dense one exact_head.ref_adagrad_dense, each applied to the exact gradients.

The magnitudes are small enough for the 16-bit paths too: every operand of an MLP GEMM below
the head is at most 107 quanta (exact in bf16), and every table value, before and after the
SGD update, is exact in fp16; build() asserts both."""
import functools
from dataclasses import dataclass, field

import numpy as np
import torch

import exact_adagrad as A
import exact_head as H
import exact_tbe as E
import oracle as O

f32, f64 = np.float32, np.float64
LIM = 2.0 ** 24
D = 16
ROWS = [64, 48, 40]
BOT = [13, 32, 16]
TOP_HIDDEN = [32, 16]
QR_C, QR_THRESHOLD = 4, 50       # table 0 (64 rows) becomes 16 quotient + 4 remainder rows
LR, EMB_LR = 2.0 ** -3, 2.0 ** -5  # powers of two, and different: a swapped rate shows
EPS = 2.0 ** -10
DI2 = [0, 1, 0]  # the two-rank allocation: rank-major feature order [0, 2, 1]
ORDER2 = [0, 2, 1]
SENTINEL = 5.0  # the last row of every table (of the quotient table under QR): never indexed

# name -> (B, lookups per bag, arch_interaction_itself, QR operation, loss, model seed, W); the
# seeds are the ones, of 0..59, whose model passes build()'s assertions with the most rows and
# weights updated
VARIANTS = {
    "onehot": (64, 1, False, None, "bce", 38, 1),
    "multihot": (64, 3, False, None, "bce", 37, 1),
    "itself": (128, 1, True, None, "bce", 0, 1),
    "qr_mult": (64, 1, False, "mult", "bce", 10, 1),
    "qr_add": (64, 1, False, "add", "bce", 59, 1),
    "mse": (64, 1, False, None, "mse", 38, 1),
    # two ranks (oracle.distributed_step): the rank-major feature order is part of the model
    "two_ranks": (64, 1, False, None, "bce", 5, 2),
    "two_ranks_multihot": (128, 3, False, None, "bce", 14, 2),
    "two_ranks_qr": (64, 1, False, "mult", "bce", 10, 2),
    # a bottom MLP whose widest layer has 64 rows: the split chains (bottom_parts 2 and 4)
    "wide": (64, 1, False, None, "bce", 3, 1),
}
BOT_OF = {"wide": [13, 64, 64, 16]}
BUG_MODELS = ["emb_rate_x1.25", "sample_dropped", "table_not_updated", "inv_b_plus_1",
              "bias_grad_dropped", "relu_x_omitted", "diag_twice", "dense_not_averaged",
              "emb_without_w", "remainder_dropped"]


def bug_applies(bug, variant):
    """Whether a bug model can change anything on this variant."""
    itself, qr, W = VARIANTS[variant][2], VARIANTS[variant][3], VARIANTS[variant][6]
    return {"diag_twice": itself, "dense_not_averaged": W > 1, "emb_without_w": W > 1,
            "remainder_dropped": qr is not None}.get(bug, True)


def num_int(itself):
    F = len(ROWS) + 1
    return D + (F * (F + 1) // 2 if itself else F * (F - 1) // 2)


def quantum(a):
    """The largest power of two that divides every element of ``a`` (1 for all zeros)."""
    nz = np.asarray(a, dtype=f64).ravel()
    nz = nz[nz != 0]
    if nz.size == 0:
        return 1.0
    for k in range(-40, 80):
        s = nz * 2.0 ** k
        if np.array_equal(s, np.round(s)):
            return 2.0 ** -k
    raise AssertionError("no dyadic quantum")


class Ledger:
    """Runs the step's reductions in fp64 and asserts the criterion for each: sum of |terms| in
    units of the operands' quanta < 2^24.  worst[name] keeps the largest figure seen."""

    def __init__(self, check=True):
        self.worst, self.check = {}, check  # check=False: a bug model's run (1 / (B + 1) ...)
        self.operand = 0.0

    def note(self, name, v):
        v = float(v)
        assert not self.check or v < LIM, f"{name}: sum of |terms| = {v} quanta >= 2^24"
        self.worst[name] = max(self.worst.get(name, 0.0), v)

    def mm(self, name, a, b):
        if not name.startswith("head"):  # an MLP GEMM below the head: its operands, in quanta
            self.operand = max(self.operand, float(np.abs(a).max(initial=0) / quantum(a)),
                               float(np.abs(b).max(initial=0) / quantum(b)))
        self.note(name, (np.abs(a) @ np.abs(b)).max(initial=0) / (quantum(a) * quantum(b)))
        return a @ b

    def sum0(self, name, a):
        self.note(name, np.abs(a).sum(0).max(initial=0) / quantum(a))
        return a.sum(0)


@dataclass
class Model:
    """The parameters as fp64 arrays.  tables[t]: [rows, D], or a (quotient, remainder) pair."""
    tables: list
    bot: list   # [(W [N, K], b [N])]
    top: list
    itself: bool = False
    qr_op: str = None
    loss: str = "bce"


@dataclass
class Case:
    name: str
    model: Model
    X: np.ndarray       # [B, 13] float32
    lS_o: np.ndarray    # [T, B] int64
    lS_i: list          # T x int64
    T: np.ndarray       # [B, 1] float32
    B: int = 0
    L: int = 1
    W: int = 1
    order: list = None  # the features' order in the interaction (None: the tables')
    ledger: dict = field(default_factory=dict)
    operand: float = 0.0  # the largest operand of an MLP GEMM below the head, in its quantum


def _aug(h):
    return np.concatenate([h, np.ones((h.shape[0], 1))], axis=1)


def _pool(tab, idx, off, B):
    ends = list(off[1:]) + [len(idx)]
    out = np.zeros((B, tab.shape[1]))
    for b in range(B):
        for l in range(int(off[b]), int(ends[b])):
            out[b] += tab[idx[l]]
    return out


def _split(idx):
    return idx // QR_C, idx % QR_C


def _pairs(F, itself):
    li, lj = torch.tril_indices(F, F, offset=0 if itself else -1)
    return list(zip(li.tolist(), lj.tolist()))


def forward64(m, X, lS_o, lS_i, order=None, led=None):
    """The forward in fp64 with every reduction checked: a dict of the activations."""
    led = led or Ledger()
    B = X.shape[0]
    T = len(m.tables)
    order = list(range(T)) if order is None else list(order)
    acts = [X.astype(f64)]
    for W, b in m.bot:  # the bias rides as the last k-term, as in the engine's folded layout
        acts.append(np.maximum(led.mm("bottom forward", _aug(acts[-1]), np.c_[W, b].T), 0.0))
    x = acts[-1]
    pooled, parts = [], []
    for t in range(T):
        idx, off = np.asarray(lS_i[t]), np.asarray(lS_o[t])
        if isinstance(m.tables[t], tuple):
            q, r = _split(idx)
            eq, er = _pool(m.tables[t][0], q, off, B), _pool(m.tables[t][1], r, off, B)
            parts.append((eq, er))
            pooled.append(eq * er if m.qr_op == "mult" else eq + er)
        else:
            parts.append(None)
            pooled.append(_pool(m.tables[t], idx, off, B))
    for t in range(T):  # the pooled sums: |rows| summed over a bag, in the tables' quantum
        idx, off = np.asarray(lS_i[t]), np.asarray(lS_o[t])
        for tab, ix in (zip(m.tables[t], _split(idx)) if isinstance(m.tables[t], tuple)
                        else [(m.tables[t], idx)]):
            led.note("pooled lookup", _pool(np.abs(tab), ix, off, B).max() / quantum(tab))
    feats = np.stack([x] + [pooled[t] for t in order], axis=1)  # [B, F, D]
    F = feats.shape[1]
    Z = np.einsum("bid,bjd->bij", feats, feats)
    led.note("interaction", np.einsum("bid,bjd->bij", np.abs(feats), np.abs(feats)).max())
    pairs = _pairs(F, m.itself)
    R = np.concatenate([x, np.stack([Z[:, i, j] for i, j in pairs], axis=1)], axis=1)
    tacts = [R]
    for W, b in m.top[:-1]:
        tacts.append(np.maximum(led.mm("top forward", _aug(tacts[-1]), np.c_[W, b].T), 0.0))
    wh, bh = m.top[-1]
    z = led.mm("head", _aug(tacts[-1]), np.c_[wh, bh].T).ravel()
    return dict(acts=acts, x=x, pooled=pooled, parts=parts, feats=feats, pairs=pairs,
                tacts=tacts, z=z, order=order)


def anchor_prob(z):
    """exact_head's anchors for logits that are 0 or at least 128 in magnitude: expf(-128)
    vanishes beside 1 and expf(128) overflows, as at 24 and -100."""
    z = np.asarray(z)
    assert np.all((z == 0) | (np.abs(z) >= 128)) and np.array_equal(z, np.round(z))
    return H.anchor_prob(np.where(z == 0, 0, np.where(z > 0, 24, -100)))


def grads64(m, c, bug=None, led=None):
    """Forward, loss and every gradient of one step on Case ``c`` at its world size W (the
    oracle.distributed_step semantics: a rank's loss is the mean over its B / W rows, dense
    gradients are averaged over the ranks, embedding gradients summed), in fp64.  ``bug``
    applies one of BUG_MODELS' gradient-side models."""
    led = led or Ledger()
    B, T, W = c.B, len(m.tables), c.W
    fw = forward64(m, c.X, c.lS_o, c.lS_i, c.order, led)
    p = anchor_prob(fw["z"])
    t = c.T.ravel().astype(f32)
    Bl = B // W
    pc, dz, _ = H.head_row_ref(p, t, m.loss, 0.0, 1.0, Bl + 1 if bug == "inv_b_plus_1" else Bl)
    rl = H.row_loss64(pc, t, m.loss)
    loss = np.array([f32(rl[s * Bl:(s + 1) * Bl].sum()) / f32(Bl) for s in range(W)], dtype=f32)
    dz = dz.astype(f64)
    dense_scale = 1.0 if bug == "dense_not_averaged" else 1.0 / W
    n_bot = len(m.bot)

    def layer_bwd(name, g, inp, Wl, first):
        """(dW, db, d inp before its ReLU mask) for the gradient g at the layer's output."""
        dW = led.mm(name + " wgrad", g.T, inp)
        db = led.sum0(name + " bias sum", g)
        return dW, db, (None if first else led.mm(name + " dgrad", g, Wl))

    gd = [None] * (n_bot + len(m.top))
    g = dz[:, None]
    for li in range(len(m.top) - 1, -1, -1):
        inp = fw["tacts"][li]
        dW, db, dinp = layer_bwd("head" if li == len(m.top) - 1 else "top", g, inp,
                                 m.top[li][0], False)
        gd[n_bot + li] = [dW, db]
        g = dinp * (inp > 0) if li > 0 else dinp  # the interaction's output has no ReLU
    dR = g
    feats, pairs, F = fw["feats"], fw["pairs"], fw["feats"].shape[1]
    dF = np.zeros_like(feats)
    dFabs = np.zeros_like(feats)
    for k, (i, j) in enumerate(pairs):
        gz = dR[:, D + k][:, None]
        mult = 2.0 if bug == "diag_twice" and i == j else 1.0
        for a, b in ((i, j), (j, i)):  # d(f_i . f_j): f_j to i and f_i to j (twice f_i at i = j)
            dF[:, a] += mult * gz * feats[:, b]
            dFabs[:, a] += mult * np.abs(gz) * np.abs(feats[:, b])
    dx = dR[:, :D] + dF[:, 0]
    led.note("interaction backward", (dFabs[:, 0] + np.abs(dR[:, :D])).max()
             / (quantum(dR) * quantum(feats)))
    led.note("interaction backward", dFabs.max() / (quantum(dR) * quantum(feats)))
    g = dx if bug == "relu_x_omitted" else dx * (fw["x"] > 0)
    for li in range(n_bot - 1, -1, -1):
        inp = fw["acts"][li]
        dW, db, dinp = layer_bwd("bottom", g, inp, m.bot[li][0], li == 0)
        gd[li] = [dW, db]
        if li > 0:
            g = dinp * (inp > 0)
    for pair in gd:
        pair[0], pair[1] = pair[0] * dense_scale, pair[1] * dense_scale
    if bug == "bias_grad_dropped":
        gd[n_bot][1] = np.zeros_like(gd[n_bot][1])  # the widest layer: the top MLP's first
    # ---- embedding gradients: the per-bag gradient scattered onto the rows it pooled
    emb_scale = 1.0 / W if bug == "emb_without_w" else 1.0
    gt = []
    for t in range(T):
        dE = dF[:, 1 + fw["order"].index(t)] * emb_scale
        idx, off = np.asarray(c.lS_i[t]), np.asarray(c.lS_o[t])
        bag = np.searchsorted(off, np.arange(len(idx)), side="right") - 1
        keep = np.ones(len(idx), dtype=bool)
        if bug == "sample_dropped" and t == 0:
            keep[_multiply_touched_lookup(idx, bag, dE, isinstance(m.tables[t], tuple))] = False

        def scatter(rows, vals, n):
            out, mag = np.zeros((n, D)), np.zeros((n, D))
            np.add.at(out, rows[keep], vals[bag][keep])
            np.add.at(mag, rows[keep], np.abs(vals[bag][keep]))
            led.note("coalesced row gradient", mag.max(initial=0) / quantum(vals))
            return out
        if isinstance(m.tables[t], tuple):
            q, r = _split(idx)
            eq, er = fw["parts"][t]
            dq, dr = (dE * er, dE * eq) if m.qr_op == "mult" else (dE, dE)
            gq = scatter(q, dq, m.tables[t][0].shape[0])
            gr = scatter(r, dr, m.tables[t][1].shape[0])
            gt.append((gq, np.zeros_like(gr) if bug == "remainder_dropped" else gr))
        else:
            gt.append(scatter(idx, dE, m.tables[t].shape[0]))
    return dict(fw=fw, prob=pc, dz=dz.astype(f32), loss=loss, row_loss=rl, dense=gd, tables=gt)


def _multiply_touched_lookup(idx, bag, dE, qr):
    """A lookup of a row (a quotient row under QR) that several bags name, whose own gradient
    is not zero: dropping it changes that row's coalesced gradient."""
    rows = idx // QR_C if qr else idx
    live = np.abs(dE[bag]).sum(1) > 0
    for i in np.flatnonzero(live):
        if (rows[bag != bag[i]] == rows[i]).any():
            return i
    raise AssertionError("no multiply-touched row with a live gradient")


def _representable(name, v, check=True):
    assert not check or np.array_equal(v.astype(f32).astype(f64), v), \
        f"{name}: an updated value is inexact"
    return v.astype(f32)


def _flat(tables):
    return [x for t in tables for x in (t if isinstance(t, tuple) else (t,))]


def apply_update(m, g, optimizer="sgd", lr=LR, emb_lr=EMB_LR, bug=None):
    """The parameters after the update, float32: dict(dense=[(W, b)], tables=[flat physical
    tables], state=...).  sgd: the fp64 value, checked representable.  rwsadagrad / adagrad: the
    float32 emulations on the exact gradients, from zero state; their gradients must also
    square exactly."""
    if bug == "emb_rate_x1.25":
        emb_lr = emb_lr * 1.25
    tabs, gtabs = _flat(m.tables), _flat(g["tables"])
    skip = 1 if bug == "table_not_updated" else -1
    out = dict(dense=[], tables=[], dense_sum=[], momentum=[], table_sum=[])
    for (Wl, b), (dW, db) in zip(m.bot + m.top, g["dense"]):
        if optimizer == "sgd":
            out["dense"].append((_representable("dense W", Wl - lr * dW, bug is None),
                                 _representable("dense b", b - lr * db, bug is None)))
            continue
        new, sums = [], []
        for p, gp in ((Wl, dW), (b, db)):
            assert np.abs(gp).max(initial=0) / quantum(gp) < 4096, "a dense g^2 is inexact"
            pn, s = H.ref_adagrad_dense(torch.from_numpy(p.astype(f32)),
                                        torch.from_numpy(gp.astype(f32)),
                                        torch.zeros(p.shape), lr, EPS)
            new.append(pn.numpy()), sums.append(s.numpy())
        out["dense"].append(tuple(new)), out["dense_sum"].append(tuple(sums))
    for k, (tab, gt) in enumerate(zip(tabs, gtabs)):
        if k == skip:
            gt = np.zeros_like(gt)
        if optimizer == "sgd":
            out["tables"].append(_representable("table", tab - emb_lr * gt, bug is None))
        elif optimizer == "rwsadagrad":
            w, mom = E.ref_adagrad(torch.from_numpy(tab.astype(f32)), torch.zeros(tab.shape[0]),
                                   torch.from_numpy(gt), D, emb_lr, EPS)
            out["tables"].append(w.numpy()), out["momentum"].append(mom.numpy())
        else:
            w, s = A.ref_adagrad_elem(torch.from_numpy(tab.astype(f32)), torch.zeros(tab.shape),
                                      torch.from_numpy(gt), emb_lr, EPS)
            out["tables"].append(w.numpy()), out["table_sum"].append(s.numpy())
    return out


def reference(c, optimizer="sgd", lr=LR, emb_lr=EMB_LR, bug=None):
    """Everything one step leaves behind: prob, dz, loss (one per rank), the updated
    parameters and the optimizer state.  Asserts the exactness criterion on the way."""
    led = Ledger(check=bug is None)
    g = grads64(c.model, c, bug, led)
    out = apply_update(c.model, g, optimizer, lr, emb_lr, bug)
    out.update(prob=g["prob"], dz=g["dz"], loss=g["loss"], row_loss=g["row_loss"],
               grads=g, ledger=led.worst, operand=led.operand)
    return out


def loss_is_exact(c):
    """exact_head's rule: MSE row losses (0, 1/4, 1) sum exactly; BCE rows at z = 0 carry
    log 2 through logf, so the BCE mean is compared under the head test's ulp bound."""
    return c.model.loss == "mse"


# ------------------------------------------------------------------------ builder ----
def _sparse_rows(rng, N, K, nnz):
    Wl = np.zeros((N, K))
    for n in range(N):
        cols = rng.choice(K, size=min(nnz, K), replace=False)
        Wl[n, cols] = rng.choice([-1.0, 1.0], size=cols.size)
    return Wl


def _head_weights(rng, A_last, t, scale):
    """scale x a sparse +-1 vector over the last hidden layer, chosen so that all three logit
    classes occur with both targets and as many z = 0 rows as possible have a live input."""
    K = A_last.shape[1]
    best, best_score = None, -1
    for _ in range(4000):
        v = np.zeros(K)
        cols = rng.choice(K, size=rng.choice([2, 3, 4]), replace=False)
        v[cols] = rng.choice([-1.0, 1.0], size=cols.size)
        z = A_last @ v
        cls = [(z == 0), (z > 0), (z < 0)]
        if not all((k & (t == tv)).sum() >= 2 for k in cls for tv in (0, 1)):
            continue
        live = cls[0] & ((A_last * np.abs(v)) > 0).any(1)
        score = min((live & (t == 0)).sum(), (live & (t == 1)).sum())
        if score > best_score:
            best, best_score = v, score
    assert best is not None and best_score >= 2, "no head with live anchor rows"
    return scale * best


@functools.lru_cache(maxsize=None)
def build(name):
    """The Case of VARIANTS[name] (built once, only read).  Asserts what the tests rely on: the
    anchor classes, a nonzero update of every parameter tensor, rows that repeat within a bag
    and across bags, untouched sentinel rows, and (through reference()) exactness."""
    return _build(name, VARIANTS[name][5])


def _build(name, seed):
    B, L, itself, qr_op, loss, _, W = VARIANTS[name]
    order = ORDER2 if W == 2 else None
    rng = np.random.RandomState(4200 + seed)
    tables = []
    for n in ROWS:
        tab = rng.randint(-1, 2, size=(n, D)).astype(f64) * (rng.rand(n, D) < 0.6) + 0.0
        tab[n - 1] = SENTINEL
        tables.append(tab)
    if qr_op is not None:
        nq = -(-ROWS[0] // QR_C)
        tq = rng.randint(-1, 2, size=(nq, D)).astype(f64)
        tq[nq - 1] = SENTINEL
        tr = rng.randint(1, 3, size=(QR_C, D)).astype(f64) * rng.choice([-1.0, 1.0], (QR_C, D))
        tables[0] = (tq, tr)
    ln_bot = BOT_OF.get(name, BOT)
    bot = [(_sparse_rows(rng, ln_bot[i + 1], ln_bot[i], 3),
            rng.randint(-1, 2, size=ln_bot[i + 1]).astype(f64)) for i in range(len(ln_bot) - 1)]
    widths = [num_int(itself)] + TOP_HIDDEN
    top = [(_sparse_rows(rng, widths[i + 1], widths[i], 3),
            rng.randint(0, 2, size=widths[i + 1]).astype(f64)) for i in range(len(widths) - 1)]
    X = rng.randint(0, 3, size=(B, BOT[0])).astype(f32)
    lS_o = np.array([np.arange(B) * L for _ in ROWS], dtype=np.int64)
    lS_i = []
    for n in ROWS:
        hi = (n - 1) - ((n - 1) % QR_C if qr_op is not None and n > QR_THRESHOLD else 0)
        idx = rng.randint(0, hi, size=(B, L))
        idx[1::4] = idx[0::4]  # the same rows in neighbouring samples: rows named by two bags
        if L > 1:
            idx[::3, 1] = idx[::3, 0]  # a row twice within a bag
        lS_i.append(idx.ravel().astype(np.int64))
    T = rng.randint(0, 2, size=(B, 1)).astype(f32)
    m = Model(tables, bot, top + [(np.zeros((1, TOP_HIDDEN[-1])), np.zeros(1))], itself, qr_op,
              loss)
    fw = forward64(m, X, lS_o, lS_i, order)
    m.top[-1] = (_head_weights(rng, fw["tacts"][-1], T.ravel(), 2.0 * B)[None, :], np.zeros(1))
    c = Case(name, m, X, lS_o, lS_i, T, B, L, W, order)
    r = reference(c)
    c.ledger, c.operand = r["ledger"], r["operand"]
    # 16-bit operands: an integer multiple <= 256 of a power of two is exact in bf16 (8
    # significand bits), so mlp_precision="bf16" - fp32 accumulation - gives the same bits; and
    # every table value before and after the SGD update is exact in fp16 (emb_precision="fp16")
    assert c.operand <= 256, "an MLP operand is inexact in bf16"
    for t in _flat(m.tables) + r["tables"]:
        assert np.array_equal(t.astype(np.float16).astype(f64), t), \
            "a table value is inexact in fp16"
    z = r["grads"]["fw"]["z"]
    for s in range(W):  # on every rank
        sl = slice(s * B // W, (s + 1) * B // W)
        for k in ((z == 0), (z >= 128), (z <= -128)):
            assert all((k[sl] & (T.ravel()[sl] == tv)).any() for tv in (0, 1)), \
                "an anchor class is missing"
    assert set(np.unique(np.abs(r["dz"]))) <= {0.0, W / (2 * B), W / (4 * B)}
    for v in _flat(m.tables) + [x for pair in m.bot + m.top for x in pair]:
        assert not np.signbit(v[v == 0]).any(), "a parameter holds -0: 0 - lr * 0 is +0"
    for dW, db in r["grads"]["dense"]:
        assert dW.any() and db.any(), "a dense tensor has no update"
    for gt, tab in zip(_flat(r["grads"]["tables"]), _flat(m.tables)):
        assert (gt != 0).any(1).sum() >= 4, "a table has (almost) no update"
        assert not gt[tab[:, 0] == SENTINEL].any(), "a sentinel row has a gradient"
    return c


def ln_bot(c):
    return [BOT[0]] + [Wl.shape[0] for Wl, _ in c.model.bot]


def ln_top(c):
    return [num_int(c.model.itself)] + TOP_HIDDEN + [1]


def flat_index(c):
    """Per logical table, the positions of its physical tables in reference()'s flat lists."""
    out, k = [], 0
    for t in c.model.tables:
        n = 2 if isinstance(t, tuple) else 1
        out.append(list(range(k, k + n)))
        k += n
    return out


def to_oracle(c):
    """A fresh oracle.OracleDLRM holding the Case's parameters (float32: all exact)."""
    m = c.model
    plain = [t[0] if isinstance(t, tuple) else t for t in m.tables]
    ref = O.OracleDLRM(D, ROWS, ln_bot(c), ln_top(c), arch_interaction_itself=m.itself,
                       loss_function=m.loss, rng=np.random.RandomState(0),
                       tables=[np.zeros((n, D), dtype=f32) for n in ROWS])
    for k, t in enumerate(m.tables):
        if isinstance(t, tuple):
            ref.emb_l[k] = O.QREmbeddingBagOracle(ROWS[k], D, QR_C, m.qr_op,
                                                  weight_q=t[0].astype(f32),
                                                  weight_r=t[1].astype(f32))
        else:
            ref.emb_l[k].weight.data = torch.tensor(plain[k].astype(f32))
    lin = [x for seq in (ref.bot_l, ref.top_l) for x in seq if isinstance(x, torch.nn.Linear)]
    for x, (Wl, b) in zip(lin, m.bot + m.top):
        x.weight.data = torch.tensor(Wl.astype(f32))
        x.bias.data = torch.tensor(b.astype(f32))
    return ref


def oracle_state(ref):
    """(dense [(W, b)], flat physical tables) of an oracle, float32 numpy."""
    lin = [x for seq in (ref.bot_l, ref.top_l) for x in seq if isinstance(x, torch.nn.Linear)]
    dense = [(x.weight.detach().numpy(), x.bias.detach().numpy()) for x in lin]
    tabs = []
    for e in ref.emb_l:
        tabs += [e.weight_q.detach().numpy(), e.weight_r.detach().numpy()] \
            if hasattr(e, "weight_q") else [e.weight.detach().numpy()]
    return dense, tabs


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.dtype == b.dtype == f32 and a.shape == b.shape
            and np.array_equal(a.view(np.int32), b.view(np.int32)))


def state_equal(ref_out, dense, tables):
    """Names of the tensors of (dense, tables) that differ in any bit from a reference()."""
    bad = []
    for i, ((W0, b0), (W1, b1)) in enumerate(zip(ref_out["dense"], dense)):
        bad += [f"W{i}"] * (not bits_equal(W0, W1)) + [f"b{i}"] * (not bits_equal(b0, b1))
    for k, (t0, t1) in enumerate(zip(ref_out["tables"], tables)):
        bad += [f"table{k}"] * (not bits_equal(t0, t1))
    return bad
