"""Exact-arithmetic reference for the element-wise Adagrad mode of the embedding backward
(tbe_backward("adagrad"), MODE_ADAGRAD_ELEM of csrc/tbe_bwd_roles.hpp), and the fp32 / fp64
twin that conditions the engine's trajectory tests.

The cases, operands and coalesced gradients are exact_tbe's; this module adds the start state
(integer-valued, >= 0, some of it 0) and the reference of the rule

    s = fmaf(g, g, S);  S = s;  W = fmaf(-lr, g / (sqrtf(s) + eps), W)

With an integer g and an integer S, S + g^2 is an integer below 2^24: the first fma is exact.
sqrt, + eps and the division are correctly rounded IEEE operations, emulated one numpy float32
operation each.  With lr a power of two lr * u is exact, so the second fma rounds W - lr * u
once, as the fp64 difference rounded to fp32 does.  The same conditions make torch.optim.Adagrad
on the CPU - whatever its operation order or contraction - give the same bits, which
test_exact_adagrad_cpu.py proves for its sparse and its dense form.

Plain helper module (no GPU needed), like exact_tbe.py."""
import copy
import math

import numpy as np
import torch


def start_state(o):
    """S0 on the touched rows: |acc0u| (integers in [1, 64]) with every fifth element 0 (an
    accumulator that is still at its initial value)."""
    S = o.acc0u.abs().clone()
    S.view(-1)[::5] = 0.0
    return S


def ref_adagrad_elem(W0u, S0u, gsum, lr, eps):
    """numpy float32 emulation of the element-wise rule, one operation per rounding; returns
    (W, S).  Asserts its own exactness conditions."""
    f32 = np.float32
    m, e = math.frexp(lr)
    assert m == 0.5 and lr > 0, f"lr {lr} is no power of two"
    g64 = gsum.numpy().astype(np.float64)
    S0 = S0u.numpy().astype(np.float64)
    assert (S0 >= 0).all() and (S0 == np.round(S0)).all() and (g64 == np.round(g64)).all()
    s64 = S0 + g64 * g64
    assert s64.size == 0 or s64.max() < 2.0 ** 24, "S0 + g^2 leaves the integers fp32 holds"
    s = s64.astype(f32)  # exact
    g = g64.astype(f32)  # exact (condition 1 of exact_tbe)
    denom = np.sqrt(s) + f32(eps)
    assert s.dtype == f32 and denom.dtype == f32
    with np.errstate(invalid="ignore", divide="ignore"):
        u = g / denom
    assert u.dtype == f32
    w = (W0u.numpy().astype(np.float64) - lr * u.astype(np.float64)).astype(f32)
    return torch.from_numpy(w), torch.from_numpy(s)


def table_csr(case, t):
    """Table t's valid lookups as an nn.EmbeddingBag input: (table-local indices, offsets of
    its B bags, positions of those lookups in the case)."""
    sel = np.flatnonzero(case.valid & (case.table == t))
    bag = case.bag[sel] - t * case.B
    assert (np.diff(bag) >= 0).all()
    off = np.searchsorted(bag, np.arange(case.B), side="left")
    return case.indices[sel], off, sel


# ------------------------------------------------------------ the conditioning twin ----
# The trajectory tests compare the engine with an fp32 CPU oracle through conftest.fp32_close
# (1e-5 * max(1, |ref|)).  Element-wise Adagrad's first steps are lr * g / (|g| + eps): an
# element with |g| near eps amplifies rounding by lr / eps, so at small eps the fp32 oracle
# alone leaves that tolerance.  The twin steps an fp64 copy of the oracle beside it; a case is
# well conditioned when the two stay within TWIN_BOUND = 1e-6, a tenth of the tolerance, on
# everything the trajectory tests compare: every step's Z and loss, every parameter and every
# Adagrad sum after the last step.
TWIN_BOUND = 1e-6
TRAJ = dict(D=32, B=256, rows=[3, 5000, 150, 201, 2000, 64, 1000, 7], bot=[13, 64, 32],
            top=[64, 1], lr=0.01, steps=3, qr_collisions=4, qr_threshold=200)
# case -> (lookups per bag, QR operation or None)
TRAJ_CASES = {"plain_onehot": (1, None), "plain_multihot": (3, None), "qr_mult": (1, "mult"),
              "qr_add": (1, "add")}
# adagrad_eps of each case: 1e-4 unless the twin needs more (raised by decades until the
# oracle alone stays within TWIN_BOUND on all of Z, loss, parameters and sums;
# test_exact_adagrad_cpu.py asserts these values do).  No case needs more.
TRAJ_EPS = {"plain_onehot": 1e-4, "plain_multihot": 1e-4, "qr_mult": 1e-4, "qr_add": 1e-4}
# Scale of the QR tables' initial values (a power of two: exact).  QREmbeddingBag draws both
# tables from U[sqrt(1/n), 1), which suits "mult" (a product below 1).  Under "add" a feature
# reaches 2 and the 32-wide dot products 128: the head saturates, the fp32 BCE of predictions
# within 1e-5 of 1 differs from its fp64 copy by 3.2e-5 (three times fp32_close's tolerance) and
# Adagrad sums near 100 by 1.4e-6 - fp32's own rounding, which no eps cures (eps = 1e-1 leaves
# 3.3e-6 / 1.1e-6).  So the remedy is in the case's data: the scale is halved until the twin
# holds all three figures (1: 8.6e-7 / 3.2e-5 / 1.4e-6 for Z and parameters / loss / sums;
# 1/2: 3.1e-7 / 8.8e-8 / 1.35e-6; 1/4: 1.7e-7 / 1.2e-7 / 9.5e-8).
TRAJ_QR_SCALE = {"qr_mult": 1.0, "qr_add": 0.25}


def traj_ln_top():
    F = len(TRAJ["rows"]) + 1
    return [TRAJ["D"] + F * (F - 1) // 2] + TRAJ["top"]


def traj_model(O, name):
    """The oracle of a trajectory case (test_qr_step_vs_oracle's shape and seeds)."""
    _, op = TRAJ_CASES[name]
    np.random.seed(11)
    ref = O.OracleDLRM(TRAJ["D"], TRAJ["rows"], TRAJ["bot"], traj_ln_top(), loss_function="bce")
    if op is not None:
        torch.manual_seed(5)
        for k, n in enumerate(TRAJ["rows"]):
            if n > TRAJ["qr_threshold"]:
                e = O.QREmbeddingBagOracle(n, TRAJ["D"], TRAJ["qr_collisions"], op)
                with torch.no_grad():
                    e.weight_q.mul_(TRAJ_QR_SCALE[name])
                    e.weight_r.mul_(TRAJ_QR_SCALE[name])
                ref.emb_l[k] = e
    return ref


def traj_batches(name):
    """steps x (X, lS_o, lS_i, T) as numpy arrays."""
    L, _ = TRAJ_CASES[name]
    rng = np.random.RandomState(3)
    rows, B = TRAJ["rows"], TRAJ["B"]
    out = []
    for _ in range(TRAJ["steps"]):
        X = np.log1p(rng.rand(B, TRAJ["bot"][0]).astype(np.float32))
        lS_o = np.array([np.arange(B) * L for _ in rows], dtype=np.int64)
        lS_i = [rng.randint(0, n, size=B * L).astype(np.int64) for n in rows]
        T = np.round(rng.rand(B, 1).astype(np.float32))
        out.append((X, lS_o, lS_i, T))
    return out


def oracle_step(model, opt, X, lS_o, lS_i, T, dtype=torch.float32):
    Z = model(torch.tensor(X).to(dtype), torch.tensor(lS_o), [torch.tensor(i) for i in lS_i])
    Er = model.loss_fn(Z, torch.tensor(T).to(dtype))
    opt.zero_grad()
    Er.backward()
    opt.step()
    return Z.detach(), Er.detach()


def rel_diff(a, b):
    """max |a - b| / max(1, |b|): fp32_close's measure."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) if a.size else 0.0


# The two-rank case: the small model, seeds and batches of tests/test_gpu_dist.py's two-rank test
TWO_RANKS = dict(W=2, sharder="greedy", lr=0.01, eps=1e-4, steps=3, B=12)
TWO_RANKS_CFG = dict(m_spa=8, ln_emb=[300, 40, 1000, 7, 120], ln_bot=[13, 32, 8],
                     ln_top=[23, 16, 1])


def two_ranks_setup(O):
    """(model, device_indices, batches) of the two-rank case."""
    c = TWO_RANKS_CFG
    di = O.shard(c["ln_emb"], TWO_RANKS["W"], TWO_RANKS["sharder"])
    np.random.seed(77)
    ref = O.OracleDLRM(c["m_spa"], c["ln_emb"], c["ln_bot"], c["ln_top"], loss_function="bce")
    rng = np.random.RandomState(8)
    np.random.seed(99)
    batches = []
    for _ in range(TWO_RANKS["steps"]):
        X, lS_o, lS_i = O.generate_uniform_input_batch(13, c["ln_emb"], TWO_RANKS["B"], 5, False)
        T = torch.tensor(rng.randint(0, 2, size=(TWO_RANKS["B"], 1)).astype(np.float32))
        batches.append((torch.log(X + 1), torch.stack(lS_o), lS_i, T))
    return ref, di, batches


def twin_spread(O, name, eps):
    """The fp32 oracle against its fp64 copy over the case's steps, as rel_diff: (the worst of
    every step's Z and every parameter after the last step; the worst loss; the worst Adagrad
    sum).  All three are bounded by TWIN_BOUND.  ``name``: a key of TRAJ_CASES, or
    "two_ranks"."""
    dist = name == "two_ranks"
    if dist:
        ref, di, batches = two_ranks_setup(O)
        lr = TWO_RANKS["lr"]
    else:
        ref, batches, lr = traj_model(O, name), traj_batches(name), TRAJ["lr"]
    ref64 = copy.deepcopy(ref).double()
    o32 = torch.optim.Adagrad(ref.parameters(), lr=lr, eps=eps)
    o64 = torch.optim.Adagrad(ref64.parameters(), lr=lr, eps=eps)
    worst = loss = sums = 0.0
    for X, lS_o, lS_i, T in batches:
        if dist:
            W = TWO_RANKS["W"]
            Zs, Es = O.distributed_step(ref, W, di, X, lS_o, lS_i, T, lr, optimizer=o32)
            Z64, E64 = O.distributed_step(ref64, W, di, X.double(), lS_o, lS_i, T.double(), lr,
                                          optimizer=o64)
            Z, Er, Z64, E64 = (torch.cat([v.reshape(-1) for v in x]) for x in (Zs, Es, Z64, E64))
        else:
            Z, Er = oracle_step(ref, o32, X, lS_o, lS_i, T)
            Z64, E64 = oracle_step(ref64, o64, X, lS_o, lS_i, T, torch.float64)
        worst = max(worst, rel_diff(Z.numpy(), Z64.numpy()))
        loss = max(loss, rel_diff(Er.numpy(), E64.numpy()))
    for p, p64 in zip(ref.parameters(), ref64.parameters()):
        worst = max(worst, rel_diff(p.detach().numpy(), p64.detach().numpy()))
        sums = max(sums, rel_diff(o32.state[p]["sum"].numpy(), o64.state[p64]["sum"].numpy()))
    return worst, loss, sums
