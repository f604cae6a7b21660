"""dlrm_linear16_bwd_group (the 16-bit Linear backward as one grouped launch, ABI v22) against
fp64 references computed with torch on the CPU.

  dgrad  dX = mask > 0 ? dY W : 0        wgrad  C = dY^T X   or   C - lr dY^T X

Integer operands in [-4, 4] (exact in bf16 and fp16, every partial sum far below 2^24) and
lr = 0.5 on an integer C make every result exact and independent of the summation order, so the
comparison is torch.equal.  Every launch runs twice on the same workspace (a ticket that is
not reset or a stale partial fails the second run); outputs sit in sentinel-padded buffers
with guard rows."""
import pytest
import torch

from exact_inputs import SENTINEL, gemm_close, int_matrix, padded, pads_intact

pytestmark = pytest.mark.gpu

dev = "cuda:0"
NAN = float("nan")
LR = 0.5
# (kind, M, N, K): the dgrads take a 1, a non-multiple of 4 and a value past a tile edge and
# a 64-deep step in every dimension; M = 130 is three reduction steps, the last one short;
# M = 64 * 32 + 1 reaches many splits under the planner
GROUPS = {
    "dgrad": [("d", 33, 70, 65)],
    "wgrad": [("w", 130, 70, 65)],
    "pair": [("d", 33, 70, 65), ("w", 130, 70, 65)],
    "four": [("d", 1, 65, 70), ("w", 64 * 32 + 1, 33, 1), ("d", 70, 1, 33), ("w", 130, 3, 129)],
}
# (group, forced wgrad split; 0 = the planner)
RUNS = [("dgrad", 0), ("wgrad", 1), ("wgrad", 2), ("wgrad", 3), ("pair", 2), ("pair", 3),
        ("four", 0)]
# forced (dgrad tile, wgrad tile); 0 = the planner: both kinds in every class, mixed classes
TILES = [(0, 0), (128128, 32064), (32064, 128128), (128064, 64064), (64064, 128064)]
_REFS = {}


@pytest.fixture(scope="module")
def ops():
    from dlrm_hip import ops as _ops
    return _ops


def _reference(group):
    """Operands and fp64 results of a group, built once on the CPU and only read."""
    if group not in _REFS:
        gen = torch.Generator().manual_seed(11)
        out = []
        for kind, M, N, K in GROUPS[group]:
            dy = int_matrix((M, N), -4, 4, gen)
            if kind == "d":
                w, mask = int_matrix((N, K), -4, 4, gen), int_matrix((M, K), -1, 1, gen, False)
                ref = torch.where(mask > 0, dy.double() @ w.double(), 0.0)
                out.append(dict(kind=kind, dy=dy, b=w, mask=mask, c0=None, ref=ref))
            else:
                x, c0 = int_matrix((M, K), -4, 4, gen), int_matrix((N, K), -4, 4, gen)
                out.append(dict(kind=kind, dy=dy, b=x, mask=None, c0=c0,
                                ref=c0.double() - LR * (dy.double().t() @ x.double())))
        _REFS[group] = out
    return _REFS[group]


def _operand(t, aligned):
    """``t`` on the device in a NaN-padded buffer: row stride a multiple of 4 on a 16-byte
    base, or one float into a flat buffer with an odd row stride (element loads)."""
    t = t.to(dev)
    r, c = t.shape
    if aligned:
        return padded(t, 2, (c + 4) // 4 * 4 - c, NAN)
    ld = c + 1 if (c + 1) % 2 else c + 2
    flat = torch.full((1 + (r + 2) * ld,), NAN, device=dev)
    view = flat[1:1 + r * ld].view(r, ld)[:, :c]
    view.copy_(t)
    return view


def _problems(ops, ref, aligned):
    """The device problems of a reference group: (structs, outputs, tensors kept alive)."""
    probs, outs, keep = [], [], []
    for p in ref:
        dy, b = _operand(p["dy"], aligned), _operand(p["b"], aligned)
        rows, cols = p["ref"].shape
        out = padded(torch.full((rows, cols), SENTINEL, device=dev), 2, 3, SENTINEL)
        if p["kind"] == "d":
            mask = padded(p["mask"].to(dev), 1, 1, NAN)
            probs.append(ops.dgrad16_problem(dy, b, mask, out))
            keep.append(mask)
        else:
            probs.append(ops.wgrad16_problem(dy, b, out, LR))
        outs.append(out)
        keep += [dy, b]
    return probs, outs, keep


@pytest.mark.parametrize("tiles", TILES)
@pytest.mark.parametrize("group,split", RUNS)
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_exact_groups_and_replay(ops, dt, aligned, group, split, tiles):
    ref = _reference(group)
    probs, outs, keep = _problems(ops, ref, aligned)
    with ops.tuning(linear16_dgrad_tile=tiles[0], linear16_wgrad_tile=tiles[1],
                    linear16_wgrad_split=split):
        need = ops.linear16_bwd_group_workspace_size(probs, dt)
        assert (need > 0) == (group != "dgrad" and split != 1)
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        for replay in range(2):
            for p, out in zip(ref, outs):  # the same starting C, sentinels where dX goes
                out.copy_(torch.full_like(out, SENTINEL) if p["c0"] is None else p["c0"].to(dev))
            ops.linear16_bwd_group(probs, dt, ws)
            for i, (p, out) in enumerate(zip(ref, outs)):
                assert torch.equal(out.cpu().double(), p["ref"]), (replay, i)
                assert pads_intact(out), (replay, i)


def test_random_operands_match_the_per_layer_launches(ops):
    """bf16, random normal operands, the dgrad beside a split wgrad (STORE and SGD): within the
    fp32-accumulation bound over the reduction depth (gemm_close, as test_gpu_linear16_bwd) of
    fp64 products of the rounded operands, and bitwise linear16_dgrad / linear16_wgrad under
    the same forced tile and split."""
    gen = torch.Generator().manual_seed(5)
    (_, M, N, K), (_, Mw, Nw, Kw) = GROUPS["pair"]
    dy, w = torch.randn(M, N, generator=gen) * 0.1, torch.randn(N, K, generator=gen) * 0.05
    mask = torch.randn(M, K, generator=gen)
    dyw, x = torch.randn(Mw, Nw, generator=gen) * 0.1, torch.randn(Mw, Kw, generator=gen)
    c0 = torch.randn(Nw, Kw, generator=gen)
    r = lambda t: t.to(torch.bfloat16).double()  # noqa: E731
    acc, absacc = r(dyw).t() @ r(x), r(dyw).abs().t() @ r(x).abs()
    dyd, wd, maskd, dywd, xd = (t.to(dev) for t in (dy, w, mask, dyw, x))
    for lr in (None, 0.3):
        dx, C, dx1, C1 = (torch.empty(M, K, device=dev), c0.to(dev), torch.empty(M, K, device=dev),
                          c0.to(dev))
        with ops.tuning(linear16_dgrad_tile=64064, linear16_wgrad_tile=32064,
                        linear16_wgrad_split=3):
            probs = [ops.dgrad16_problem(dyd, wd, maskd, dx), ops.wgrad16_problem(dywd, xd, C, lr)]
            ws = torch.zeros(ops.linear16_bwd_group_workspace_size(probs), dtype=torch.uint8,
                             device=dev)
            ops.linear16_bwd_group(probs, "bf16", ws)
            ops.linear16_dgrad(dyd, wd, maskd, out=dx1)
            ops.linear16_wgrad(dywd, xd, C1, lr=lr)
        assert torch.equal(dx, dx1) and torch.equal(C, C1)
        ok, worst = gemm_close(dx.cpu().numpy(), torch.where(mask > 0, r(dy) @ r(w), 0.0).numpy(),
                               (r(dy).abs() @ r(w).abs()).numpy(), N)
        assert ok, worst
        want, absprod = (acc, absacc) if lr is None else \
            (c0.double() - float(torch.tensor(lr, dtype=torch.float32)) * acc,
             c0.double().abs() + lr * absacc)
        ok, worst = gemm_close(C.cpu().numpy(), want.numpy(), absprod.numpy(), Mw)
        assert ok, worst


@pytest.mark.parametrize("what,code", [("n0", 1), ("n5", 1), ("short", 4), ("tile", 1)])
def test_refusals_write_nothing(ops, what, code):
    from dlrm_hip._lib import DLRMHipError
    probs, outs, keep = _problems(ops, _reference("pair"), True)
    with ops.tuning(linear16_wgrad_split=2):
        need = ops.linear16_bwd_group_workspace_size(probs)
    ws = torch.zeros(need - (what == "short"), dtype=torch.uint8, device=dev)
    sent = {"n0": [], "n5": probs + probs + probs[:1]}.get(what, probs)
    with ops.tuning(linear16_wgrad_split=2, linear16_wgrad_tile=64032 if what == "tile" else 0):
        with pytest.raises(DLRMHipError) as e:
            ops.linear16_bwd_group(sent, "bf16", ws)
    assert e.value.code == code
    torch.cuda.synchronize()
    for out in outs:
        assert bool((out._base == SENTINEL).all())
    assert not ws.any()
