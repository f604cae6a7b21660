"""dlrm_mlp_chain16_forward (the bottom MLP of a 16-bit build as one bf16 / fp16 MFMA launch)
against plain fp64 torch on the CPU and, bit for bit, against dlrm_linear16_forward applied
layer by layer; then DLRMTrainer.fuse_bottom16 on against off."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda:0"
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
DTS = sorted(DT)
# (rows; K_0 -> N_0 -> ...): C3's widths, a partial third row block; four layers, every later K
# off the 32-k block, N < 16; one row and column, the largest K_0; element loads inside a row
SHAPES = [(33, [13, 512, 256, 128]), (17, [4, 40, 24, 17, 3]), (1, [512, 1]), (16, [37, 20])]
NAN, SENT = float("nan"), -777.0


def _random(rows, widths, seed):
    g = torch.Generator().manual_seed(seed)
    Ws = [torch.randn(n, k, generator=g) / k ** 0.5 for k, n in zip(widths, widths[1:])]
    return torch.randn(rows, widths[0], generator=g), Ws, [torch.randn(len(W), generator=g) for W in Ws]


def _integer(rows, widths, seed):
    """X and bias in {-1, 0, 1}; each W row has at most 3 non-zeros in {-1, 1}, one of them in
    the last column: every value is exact in both types and |Y_l| <= 4, 13, 40, 121."""
    g = torch.Generator().manual_seed(seed)
    Ws = []
    for k, n in zip(widths, widths[1:]):
        pos = torch.randint(0, k, (n, 3), generator=g)
        pos[:, 0] = k - 1
        sign = torch.randint(0, 2, (n, 3), generator=g) * 2.0 - 1.0
        Ws.append(torch.zeros(n, k).scatter_(1, pos, sign))
    bs = [torch.randint(-1, 2, (len(W),), generator=g).float() for W in Ws]
    return torch.randint(-1, 2, (rows, widths[0]), generator=g).float(), Ws, bs


def _views(X, Ws, bs, off=0, fold=False):
    """Device views inside wider buffers.  Inputs: NaN around every row; W's column K holds a
    non-zero "bias" as in the trainer's layout (with ``fold`` the layer's own, a strided view).
    Outputs: SENT in pad columns and guard rows.  ``off`` = 1: X and W off the 16-byte boundary."""
    rows = X.shape[0]
    xb = torch.full((rows, X.shape[1] + 5), NAN, device=dev)
    xb[:, off:off + X.shape[1]] = X.to(dev)
    ws, bv, ybs = [], [], []
    for W, b in zip(Ws, bs):
        n, k = W.shape
        wb = torch.full((n, (k + off + 4) // 4 * 4 + 4), NAN, device=dev)
        wb[:, off:off + k] = W.to(dev)
        wb[:, off + k] = b.to(dev) if fold else 7.0
        ws.append(wb[:, off:off + k])
        bv.append(wb[:, off + k] if fold else b.to(dev))
        ybs.append(torch.full((rows + 2, n + 3), SENT, device=dev))
    return xb[:, off:off + X.shape[1]], ws, bv, ybs


def _y(yb):
    return yb[1:-1, 1:-2]


def _run(dt, x, ws, bv, ys):
    from dlrm_hip import ops
    chain = ops.mlp_chain16(x, list(zip(ws, bv, ys)), dtype=dt)
    assert ops.mlp_chain16_supported(chain)
    ops.mlp_chain16_forward(chain)
    torch.cuda.synchronize()


def _pads_intact(yb):
    rest = yb.clone()
    _y(rest).fill_(SENT)
    return bool((rest == SENT).all())


@pytest.mark.parametrize("rows,widths", SHAPES)
@pytest.mark.parametrize("dt", DTS)
def test_exact_integers(dt, rows, widths):
    X, Ws, bs = _integer(rows, widths, seed=rows)
    x, ws, bv, ybs = _views(X, Ws, bs)
    _run(dt, x, ws, bv, [_y(yb) for yb in ybs])
    h = X.double()
    for l, (W, b, yb) in enumerate(zip(Ws, bs, ybs)):
        h = torch.relu(h @ W.double().t() + b.double())
        assert h.abs().max() <= (4, 13, 40, 121)[l]  # exact in bf16 (integers below 256)
        assert torch.equal(_y(yb).cpu(), h.float()), l
        assert _pads_intact(yb), l


@pytest.mark.parametrize("rows,widths", SHAPES[:2])
@pytest.mark.parametrize("dt", DTS)
def test_full_mantissa_is_linear16_layer_by_layer(dt, rows, widths):
    from dlrm_hip import ops
    X, Ws, bs = _random(rows, widths, seed=100 + rows)
    x, ws, bv, ybs = _views(X, Ws, bs, fold=True)
    _run(dt, x, ws, bv, [_y(yb) for yb in ybs])
    h = inp = x
    for l, (w, b, yb) in enumerate(zip(ws, bv, ybs)):
        h = ops.linear16_forward(h, w, b, relu=True, dtype=dt)
        got = _y(yb)
        assert torch.equal(got, h) and _pads_intact(yb), l
        # the fp64 product of the rounded operands, from the device's own Y_{l-1}
        a, w16 = inp.cpu().to(DT[dt]).double(), w.cpu().to(DT[dt]).double()
        ref = torch.relu(a @ w16.t() + b.cpu().double())
        tol = 1e-5 * ref.abs().clamp(min=1.0) + 2 * w.shape[1] * 2.0 ** -24 * (a.abs() @ w16.abs().t())
        err = (got.cpu().double() - ref).abs()
        print(f"chain16 {dt} {rows}x{widths} layer {l}: worst err / tol {(err / tol).max():.3f}")
        assert (err <= tol).all(), l
        inp = got


def test_intermediates_none_nan_row_and_no_rows():
    rows, widths = SHAPES[0]
    X, Ws, bs = _random(rows, widths, seed=5)
    X[7, 3] = NAN
    x, ws, bv, ybs = _views(X, Ws, bs)
    _run("bf16", x, ws, bv, [_y(yb) for yb in ybs])
    for yb in ybs:  # the NaN reaches every output of row 7 and nothing else
        bad = torch.isnan(_y(yb))
        assert bad[7].all() and int(bad.sum()) == bad.shape[1]
    x2, ws2, bv2, ybs2 = _views(X, Ws, bs)
    _run("bf16", x2, ws2, bv2, [None, None, _y(ybs2[2])])
    assert torch.equal(_y(ybs2[2]).nan_to_num(-1.0), _y(ybs[2]).nan_to_num(-1.0))  # last Y unchanged
    assert all(bool((yb == SENT).all()) for yb in ybs2[:2])  # intermediates untouched
    x0, ws0, bv0, ybs0 = _views(X[:0], Ws, bs)
    _run("bf16", x0, ws0, bv0, [_y(yb) for yb in ybs0])
    assert all(bool((yb == SENT).all()) for yb in ybs0)


@pytest.mark.parametrize("dt", DTS)
def test_unaligned_bases_give_the_same_bits(dt):
    rows, widths = 17, [45, 40, 24]
    X, Ws, bs = _random(rows, widths, seed=9)
    outs = []
    for off in (0, 1):
        x, ws, bv, ybs = _views(X, Ws, bs, off=off, fold=True)
        assert x.data_ptr() % 16 == 4 * off and ws[0].data_ptr() % 16 == 4 * off
        _run(dt, x, ws, bv, [_y(yb) for yb in ybs])
        assert all(_pads_intact(yb) for yb in ybs)
        outs.append([_y(yb).clone() for yb in ybs])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("widths", [[8, 513], [8, 8, 8, 8, 8, 8]])
def test_unsupported_shapes_are_refused(widths):
    from dlrm_hip import _lib, ops
    x, ws, bv, ybs = _views(*_random(4, widths, seed=1))
    chain = ops.mlp_chain16(x, list(zip(ws, bv, [_y(yb) for yb in ybs])))
    assert not ops.mlp_chain16_supported(chain)
    with pytest.raises(_lib.DLRMHipError) as e:
        ops.mlp_chain16_forward(chain)
    assert e.value.code == 3  # DLRM_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------- engine --
@pytest.mark.parametrize("dt", DTS)
def test_engine_predict_on_equals_off(dt):
    import test_gpu_train16 as T
    _, _, tr = T._make("c3_small")
    batch = tr.make_batch(*T._batches("c3_small", 1)[0])
    probs = []
    for on in (False, True):
        tr.fuse_bottom16 = on
        eager = tr.predict(batch, precision=dt).clone()
        assert tr.bottom16_fused is on
        torch.cuda.synchronize()
        run = tr.capture_predict(batch, precision=dt)
        for _ in range(3):
            run()
        probs += [eager, tr._predict_bufs(tr._buffers(batch.X.shape[0], batch.X.shape[0]))["prob"].clone()]
    assert all(torch.equal(p, probs[0]) for p in probs) and len(torch.unique(probs[0])) > 4
    tr.predict(batch)  # fp32: the 16-bit chain does not apply
    assert tr.bottom16_fused is False
    tr.quantize_mlp(8)
    tr.predict(batch, mlp_bits=8)
    assert tr.bottom16_fused is False
    tr.check_errors()


def test_engine_bf16_step_on_equals_off_and_wide_bottom_falls_back():
    import test_gpu_train16 as T
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    raw = T._batches("c3_small", 1)[0]
    out = []
    for on in (False, True):
        _, _, tr = T._make("c3_small", mlp_precision="bf16")
        tr.fuse_bottom16 = on
        prob, loss = tr.step(tr.make_batch(*raw))
        tr.check_errors()
        assert tr.bottom16_fused is on
        out.append([prob.clone(), loss.clone()] + T._state(tr))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    cfg = TrainerConfig(m_spa=8, ln_emb=[50, 60], ln_bot=[13, 528, 8], ln_top=[8 + 3, 16, 1],
                        loss_function="bce", mlp_precision="bf16")
    tr = DLRMTrainer(cfg, device=dev)
    tr.fuse_bottom16 = True
    g = torch.Generator().manual_seed(0)
    tr.step(tr.make_batch(torch.rand(32, 13, generator=g), torch.arange(32).repeat(2, 1),
                          [torch.randint(0, 50, (32,), generator=g) for _ in range(2)],
                          torch.rand(32, 1, generator=g).round()))
    tr.check_errors()
    assert tr.bottom16_fused is False
