"""The int8 dynamic-quantized Linear's arithmetic as an exact rule in numpy.

It is torch.quantization.quantize_dynamic(model, {nn.Linear}, torch.qint8) on the fbgemm
engine, bit for bit (tests/test_exact_mlp8_cpu.py proves that on the CPU), and what
dlrm_linear8_pack / dlrm_linear8_range / dlrm_linear8_forward compute, bit for bit
(tests/test_gpu_linear8.py).  "fl" is one fp32 rounding; everything else is fp64 or exact
integer arithmetic.

  weights (static, per tensor, symmetric):
      lo = min(min W, 0), hi = max(max W, 0)
      s_w = max(fl(max(-lo, hi) / 127.5), FLT_EPSILON)
      wq  = clamp(rint(fl(W * fl(1 / s_w))), -128, 127)
  activations (dynamic, per tensor, per call, 7-bit range): qparams(), codes()
      xq = clamp(rint(fma(x, inv, zp)), 0, 255),  d = xq - zp
  output:
      acc = sum_k d[m][k] * wq[n][k]                       (exact, int32)
      y   = fma(float(acc), fl(s_x * s_w), bias[n])         (one rounding)
"""
import numpy as np

F32 = np.float32
FLT_EPSILON = F32(np.finfo(np.float32).eps)
SMALL_SCALE = F32(6.1e-5)
QMAX = 127  # reduce_range: activations use 7 of the 8 bits


def pack(W):
    """W [N, K] fp32 -> (wq int8 [N, K], s_w fp32)."""
    W = np.ascontiguousarray(W, dtype=F32)
    lo = min(float(W.min()) if W.size else 0.0, 0.0)
    hi = max(float(W.max()) if W.size else 0.0, 0.0)
    with np.errstate(all="ignore"):
        s_w = max(F32(F32(max(-lo, hi)) / F32(127.5)), FLT_EPSILON)
        inv = F32(F32(1.0) / s_w)
        q = np.rint((W * inv).astype(F32))  # fp32 product, one rounding
    return np.clip(q, -128, 127).astype(np.int8), F32(s_w)


def qparams(x):
    """(s_x fp32, inv fp32, zp int) of the tensor x: torch's ChooseQuantizationParams with
    qmin = 0, qmax = 127."""
    x = np.asarray(x, dtype=F32)
    mn = F32(min(float(x.min()) if x.size else 0.0, 0.0))
    mx = F32(max(float(x.max()) if x.size else 0.0, 0.0))
    with np.errstate(all="ignore"):
        scale = (float(mx) - float(mn)) / QMAX
        fs = F32(scale)
        if fs == 0 or np.isinf(F32(1.0) / fs):
            scale = 0.1
        mnd, mxd = float(mn), float(mx)
        if scale < float(SMALL_SCALE):
            # the range is stretched to the smallest scale before the zero point is chosen
            if mn == 0:
                mxd = float(F32(SMALL_SCALE * F32(QMAX)))
            elif mx == 0:
                mnd = -float(F32(SMALL_SCALE * F32(QMAX)))
            else:
                amp = float(SMALL_SCALE) / scale
                mnd, mxd = mnd * amp, mxd * amp
            scale = float(SMALL_SCALE)
        z_min = 0.0 - mnd / scale
        z_max = QMAX - mxd / scale
        z = z_min if abs(mnd / scale) < QMAX + abs(mxd / scale) else z_max
        zp = 0 if z < 0 else QMAX if z > QMAX else int(np.rint(z))
        s_x = F32(scale)
        inv = F32(F32(1.0) / s_x)
    return s_x, inv, zp


def codes(x, inv, zp):
    """d = xq - zp (int32) of x under (inv, zp): the fma rounds once to fp32."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(all="ignore"):
        t = (x.astype(np.float64) * float(inv) + float(zp)).astype(F32)  # exact in fp64, then fl
        xq = np.clip(np.rint(t), 0, 255).astype(np.int32)
    return xq - np.int32(zp)


def _fma32(a, b, c):
    """fl(a * b + c) for fp32 a, b, c with |a| < 2^31 an integer-valued float: a * b is
    exact in fp64 (24 + 24 bits); the sum of two doubles rounded to fp64 and then to fp32
    could round twice, so the sum is formed exactly (two-sum) and rounded once."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # s + err == p + c exactly
    y = s.astype(F32)
    # s is within half an fp64 ulp of the true sum; that only matters when s sits exactly on
    # an fp32 rounding boundary (a midpoint), where err decides the direction
    yd = y.astype(np.float64)
    up = np.nextafter(y, F32(np.inf)).astype(np.float64)
    dn = np.nextafter(y, F32(-np.inf)).astype(np.float64)
    with np.errstate(all="ignore"):
        tie_up = (s == (yd + up) / 2) & np.isfinite(up)
        tie_dn = (s == (yd + dn) / 2) & np.isfinite(dn)
    y = np.where(tie_up & (err > 0), up.astype(F32), y)
    y = np.where(tie_dn & (err < 0), dn.astype(F32), y)
    return y.astype(F32)


def layer_packed(x, wq, s_w, bias=None, relu=False, want=None):
    """One quantized Linear on packed weights: x [M, K] fp32 -> y [M, N] fp32.  ``want``: a
    dict that receives s_x, zp and d."""
    x = np.asarray(x, dtype=F32)
    s_x, inv, zp = qparams(x)
    d = codes(x, inv, zp)
    if want is not None:
        want.update(s_x=s_x, inv=inv, zp=zp, d=d)
    acc = d.astype(np.int64) @ wq.astype(np.int64).T
    assert np.abs(acc).max(initial=0) < 2 ** 31
    a = acc.astype(np.int32).astype(F32)  # round-to-nearest-even above 2^24
    s = F32(s_x * F32(s_w))
    with np.errstate(all="ignore"):
        if bias is None:
            y = (a.astype(np.float64) * float(s)).astype(F32)
        else:
            y = _fma32(a, np.full((), s, F32), np.asarray(bias, dtype=F32)[None, :])
    if relu:
        y = np.where(y > 0, y, F32(0))  # -0 -> +0
    return y.astype(F32)


def layer(x, W, bias=None, relu=False, want=None):
    wq, s_w = pack(W)
    return layer_packed(x, wq, s_w, bias, relu, want)


CLASSES = ("randn", "relu", "zero", "tiny_pos", "tiny_mixed", "tiny_neg", "all_neg", "huge",
           "subnormal", "pm1", "half", "saturating")


def make_input(cls, M, K, gen):
    """x [M, K] fp32 of one input class of the issue's table."""
    if cls == "randn":
        x = gen.standard_normal((M, K))
    elif cls == "relu":
        x = np.maximum(gen.standard_normal((M, K)), 0)
    elif cls == "zero":
        x = np.zeros((M, K))
    elif cls == "tiny_pos":  # range < 6.1e-5 * 127: the scale floor and the stretched range
        x = gen.random((M, K)) * 1e-4
    elif cls == "tiny_mixed":
        x = (gen.random((M, K)) - 0.3) * 1e-4
    elif cls == "tiny_neg":
        x = -gen.random((M, K)) * 1e-4
    elif cls == "all_neg":
        x = -1 - gen.random((M, K))
    elif cls == "huge":
        x = gen.standard_normal((M, K)) * 1e30
    elif cls == "subnormal":
        x = gen.standard_normal((M, K)) * 1e-41
    elif cls == "pm1":  # x * inv + zp == 127.5 exactly: the code 128
        x = gen.integers(0, 2, (M, K)) * 2.0 - 1
    elif cls == "half":  # scale exactly 0.25 on an asymmetric range: ties in the codes
        x = np.clip(gen.integers(-20, 108, (M, K)) * 0.25, -5.0, 26.75)
        x.flat[0] = -5.0
        x.flat[-1] = 26.75
    elif cls == "saturating":  # |d| = 127 against |wq| = 127 (with saturating weights)
        x = gen.integers(0, 2, (M, K)) * 3.0
    else:
        raise KeyError(cls)
    return np.ascontiguousarray(x, dtype=F32)


def make_weights(cls, N, K, gen):
    """(W [N, K], bias [N]) to go with an input class."""
    if cls == "saturating":
        return (np.sign(gen.standard_normal((N, K))) * 2.0).astype(F32), \
            gen.integers(-2, 3, N).astype(F32)
    if cls in ("pm1", "half"):
        return gen.integers(-3, 4, (N, K)).astype(F32), gen.integers(-2, 3, N).astype(F32)
    return (gen.standard_normal((N, K)) / np.sqrt(K)).astype(F32), \
        gen.standard_normal(N).astype(F32)


def stack(x, layers):
    """layers: (W, bias | None, relu) triples applied in order."""
    for W, b, relu in layers:
        x = layer(x, W, b, relu)
    return x
