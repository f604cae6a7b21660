"""CPU references for the 16-bit MLP inference path (plain helper module, no GPU needed, like
eval_ref.py and exact_inputs.py).

  * forward(): an oracle.OracleDLRM forward in fp64 with the input and the weight of every
    Linear below the head rounded through a 16-bit type (the fp32 value, as the kernel sees
    it, rounded to nearest-even by torch's cast); the head's K -> 1 layer, the biases, the
    activations, the lookup and the interaction stay unrounded, as on the device.
  * tiny_exact_model(): a DLRM whose whole forward is small-integer arithmetic, so the fp32
    path and the 16-bit paths must agree bit for bit."""
import numpy as np
import torch

import oracle as O

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
# integers up to this magnitude are exact in the type (8 / 11 significand bits)
EXACT_INT = {"bf16": 256, "fp16": 2048}


def r16(t, dt):
    """fp64 tensor -> its fp32 value -> RNE to ``dt`` -> fp64 (dt None: unchanged)."""
    return t if dt is None else t.float().to(DTYPES[dt]).double()


def _mlp(seq, h, dt, head, record):
    mods = list(seq)
    linears = [m for m in mods if isinstance(m, torch.nn.Linear)]
    for i, m in enumerate(mods):
        if isinstance(m, torch.nn.Linear):
            if record is not None:
                record.append(h.clone())
            rounded = None if (head and m is linears[-1]) else dt
            h = r16(h, rounded) @ r16(m.weight.detach().double(), rounded).t() \
                + m.bias.detach().double()
        elif isinstance(m, torch.nn.ReLU):
            h = torch.relu(h)
        elif isinstance(m, torch.nn.Sigmoid):
            h = torch.sigmoid(h)
        else:
            raise TypeError(type(m))
    return h


def forward(ref, X, lS_o, lS_i, dt=None, record=None):
    """prob [B] (fp64 numpy) of OracleDLRM ``ref``; ``record`` (a list) receives the input of
    every Linear, bottom MLP first."""
    with torch.no_grad():
        x = _mlp(ref.bot_l, torch.as_tensor(X).double(), dt, False, record)
        ly = [y.double() for y in ref.apply_emb(torch.as_tensor(lS_o),
                                                [torch.as_tensor(i) for i in lS_i])]
        z = O.interact(x, ly, ref.op, ref.itself)
        p = _mlp(ref.top_l, z, dt, True, record)
        if 0.0 < ref.loss_threshold < 1.0:
            p = torch.clamp(p, min=ref.loss_threshold, max=1.0 - ref.loss_threshold)
    return p.numpy().ravel()


TINY = dict(D=4, rows=[8, 8, 8], bot=[4, 8, 4], B=37)
TINY_SEEDS = (3, 8)


def tiny_ln_top(itself=False):
    F = len(TINY["rows"]) + 1
    return [TINY["D"] + (F * (F + 1) // 2 if itself else F * (F - 1) // 2), 8, 4, 1]


def tiny_exact_model(seed, itself=False):
    """(OracleDLRM, X, lS_o, lS_i, T): tables in {-1, 0, 1}, every non-head weight row with at
    most 2 nonzeros from {-1, 1}, biases in {-1, 0, 1}, X in {0, 1, 2}, one lookup per bag;
    the head's weights are multiples of 1/8.  Bounds: bottom activations <= 5, 11; dot terms
    <= 4 * 11 = 44 (self terms <= 4 * 121 = 484); top activations <= 2 * 44 + 1 = 89 (itself:
    969), then <= 2 * 89 + 1 = 179 (itself: 1939)."""
    rng = np.random.RandomState(1000 + seed)
    D, rows, bot, B = TINY["D"], TINY["rows"], TINY["bot"], TINY["B"]
    ln_top = tiny_ln_top(itself)
    tables = [rng.randint(-1, 2, size=(n, D)).astype(np.float32) for n in rows]
    ref = O.OracleDLRM(D, rows, bot, ln_top, arch_interaction_itself=itself, loss_function="bce",
                       rng=np.random.RandomState(seed), tables=tables)
    linears = [m for seq in (ref.bot_l, ref.top_l) for m in seq if isinstance(m, torch.nn.Linear)]
    for m in linears:
        N, K = m.weight.shape
        W = np.zeros((N, K), dtype=np.float32)
        if m is linears[-1]:
            W[:] = rng.randint(-8, 9, size=(N, K)) / 8.0
        else:
            for n in range(N):
                cols = rng.choice(K, size=min(2, K), replace=False)
                W[n, cols] = rng.choice([-1.0, 1.0], size=cols.size)
        m.weight.data = torch.tensor(W)
        m.bias.data = torch.tensor(rng.randint(-1, 2, size=N).astype(np.float32))
    X = rng.randint(0, 3, size=(B, bot[0])).astype(np.float32)
    lS_o = np.array([np.arange(B) for _ in rows], dtype=np.int64)
    lS_i = [rng.randint(0, n, size=B).astype(np.int64) for n in rows]
    T = np.round(rng.rand(B, 1)).astype(np.float32)
    return ref, X, lS_o, lS_i, T


def bump_weights(ref):
    """Add 1.0 to entry [0, 0] of every MLP weight matrix of the oracle (the test does the same
    in place on the device); returns the number of matrices."""
    n = 0
    with torch.no_grad():
        for seq in (ref.bot_l, ref.top_l):
            for m in seq:
                if isinstance(m, torch.nn.Linear):
                    m.weight[0, 0] += 1.0
                    n += 1
    return n


def linear_inputs_exact(ref, X, lS_o, lS_i, dt):
    """True when every non-head Linear input of the fp64 forward is an integer of magnitude
    <= EXACT_INT[dt], i.e. exact in ``dt`` (so is every weight: small integers), and the
    largest magnitude seen."""
    rec = []
    forward(ref, X, lS_o, lS_i, None, rec)
    worst, ok = 0.0, True
    for h in rec[:-1]:  # the last one is the head's input (fp32 on the device)
        worst = max(worst, float(h.abs().max()))
        ok = ok and bool((h == h.round()).all()) and bool((r16(h, dt) == h).all())
    return ok and worst <= EXACT_INT[dt], worst
