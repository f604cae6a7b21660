"""Row-wise Adagrad on fp16 rows (dlrm_tbe_backward_rowwise_adagrad_f16), BITWISE:
exact_tbe.ref_adagrad (numpy fp32) on integer, half-representable operands gives the fp32 row v
and the momentum; the host rounds v with .half() or with exact_sr16's sr16 and the draw of
(seed, step, global row, column).  D: one per lane class of exact_tbe.dispatch."""
import functools

import numpy as np
import pytest
import torch

import exact_sr16 as X
import exact_tbe as E

pytestmark = pytest.mark.gpu
dev = "cuda:0"
SEED, STEP = 77, 3
D_LANES = [4, 6, 8, 16, 32, 64, 128, 256, 260, 1024]  # 6: scalar lanes; 260, 1024: chunks per lane
CASES = ([("skewed", D, False, "device_wide") for D in D_LANES]
         + [("structure", D, offset, sort) for D in (16, 260) for offset in (False, True)
            for sort in ("per_table", "device_wide")]  # one reference: draws ignore sort and width
         + [(name, 16, False, "device_wide") for name in ("n1", "n7", "n128", "cancel", "long")])


@functools.lru_cache(maxsize=None)
def _reference(name, D):
    """Case, operands, ref_adagrad's (v, momentum) on the touched rows, the cancelling row."""
    named = {"skewed": E.skewed_case, "structure": E.structure_case, "cancel": E.cancel_case,
             # >= kLongChN lookups: 64-lookup blocks, most 13-lookup runs cross an edge
             "long": lambda: E.run_csr("long", [(21000, [13] * 20165)], B=64, seed=21)}
    c = named[name]() if name in named else {c.name: c for c in E.small_n_cases()}[name]
    zero = int(c.runs_spec[c.runs_spec[:, 1] == 2][0, 2]) if name == "cancel" else None
    o = E.operands_for(c, D, False, seed=D, adagrad=True, zero_row=zero)
    return (c, o, zero) + E.ref_adagrad(o.W0u, o.mom0u, E.coalesced_grad(c, o), D, o.lr, o.eps)


def _buffers(c, o, offset=False):
    """NaN everywhere but the touched rows; ``offset``: rows 2 bytes off 8-byte alignment."""
    R, u = c.total_rows, torch.from_numpy(o.urows).to(dev)
    flat = torch.full((R * o.D + 8,), float("nan"), dtype=torch.float16, device=dev)
    W = flat[int(offset):int(offset) + R * o.D].view(R, o.D)
    assert (W.data_ptr() % 8 != 0) == bool(offset)
    W[u] = o.W0u.half().to(dev)
    mom = torch.full((R,), float("nan"), device=dev)
    mom[u] = o.mom0u.to(dev)
    return W, mom, u, c.device_csr(dev), o.G.reshape(c.B, -1).to(dev)


def _update(name, D, sr, offset=False, sort="device_wide", step=STEP, lr_dev=False):
    from dlrm_hip import ops
    c, o, zero, v, m = _reference(name, D)
    W, mom, u, (idx, off, rb), G = _buffers(c, o, offset)
    W0, mom0 = W.clone(), mom.clone()
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.tbe_backward("rowwise_adagrad", W, rb, c.T, c.B, idx, off, G, eps=o.eps, momentum=mom,
                     lr=torch.tensor([o.lr], device=dev) if lr_dev else o.lr, error_flag=err,
                     max_lookups_per_table=c.max_table if sort == "per_table" else 0,
                     sr_state=ops.sr_state(SEED, step, device=dev) if sr else None)
    torch.cuda.synchronize()
    want = torch.from_numpy(X.sr16(v.numpy(), X.r16(SEED, step, o.urows, D))) if sr else v.half()
    got = W[u].cpu()
    bad = (got.view(torch.int16) != want.view(torch.int16)).any(1).nonzero().flatten()[:3].tolist()
    assert not bad, (name, D, [(int(o.urows[i]), got[i, :4], want[i, :4]) for i in bad])
    assert E.bits_equal(mom[u].cpu(), m) and int(err.item()) == c.flag
    assert E.untouched_intact(W0, W, o.urows) and E.untouched_intact(mom0, mom, o.urows)
    if zero is not None:  # a cancelled gradient: v is the old half, stored unchanged by either
        k = int(np.searchsorted(o.urows, zero))  # store, and the momentum keeps its bits
        assert E.bits_equal(got[k], o.W0u[k].half()) and E.bits_equal(m[k:k + 1], o.mom0u[k:k + 1])
    return got


@pytest.mark.parametrize("sr", [False, True], ids=["nearest", "stochastic"])
@pytest.mark.parametrize("name,D,offset,sort", CASES)
def test_update_is_the_reference_rounded(name, D, offset, sort, sr):
    assert len({E.dispatch(d)[1:] + (d % 4 == 0,) for d in D_LANES}) == len(D_LANES)
    c = _reference(name, D)[0]
    assert c.max_table <= E.SEG_CAP or sort != "per_table"
    assert (c.N >= 1 << 18) == (name == "long")
    _update(name, D, sr, offset, sort)


def test_steps_draw_differently_and_rates_agree():
    a, b = _update("structure", 16, True), _update("structure", 16, True, step=STEP + 1)
    assert not E.bits_equal(a, b)
    for sr in (False, True):  # a device rate: the same reference, so the same bits
        _update("structure", 16, sr, lr_dev=True)


def test_captured_update_and_tick_replayed_twice():
    from dlrm_hip import ops
    c, o = _reference("structure", 16)[:2]
    W, mom, _, (idx, off, rb), G = _buffers(c, o)
    st = ops.sr_state(SEED, STEP, device=dev)
    ws = torch.empty(ops.tbe_backward_workspace_size(c.N, c.total_rows, 16), dtype=torch.uint8,
                     device=dev)
    start = (W.clone(), mom.clone(), st.clone())

    def body():
        ops.tbe_backward("rowwise_adagrad", W, rb, c.T, c.B, idx, off, G, lr=o.lr, eps=o.eps,
                         momentum=mom, workspace=ws, sr_state=st)
        ops.sr_tick(st)

    def twice(fn):
        for dst, src in zip((W, mom, st), start):
            dst.copy_(src)
        fn(), fn()
        torch.cuda.synchronize()
        return W.clone(), mom.clone(), ops.sr_state_values(st)

    eager = twice(body)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        body()
    replayed = twice(graph.replay)
    assert eager[2] == replayed[2] == (SEED, STEP + 2)
    assert E.bits_equal(eager[0], replayed[0]) and E.bits_equal(eager[1], replayed[1])
