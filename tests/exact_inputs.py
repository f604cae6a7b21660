"""Inputs for which fp32 arithmetic is exact, so a kernel's result must equal the fp64
reference bit for bit - in any summation order, split or tile - and no tolerance is needed.

Two families:
  * integer-valued operands (int_matrix): while exact_bound_ok() holds, every product and
    every partial sum is an integer below 2^24, hence representable; a dropped, doubled or
    NaN-polluted k-term changes the result.
  * one nonzero per row of one operand (one_hot_rows) against a dense full-mantissa operand
    (full_mantissa): each output is ONE correctly rounded product fl(a * b) plus exact
    zeros, so reduced operand precision (a TF32-like body, a lost split-operand term)
    changes essentially every element.

Plain helper module (no GPU needed), like eval_ref.py and relu_align.py; the generators are
proved in test_exact_inputs_cpu.py."""
import numpy as np
import torch

SENTINEL = -7.0  # output pad / guard fill, as elsewhere in the suite


def int_matrix(shape, lo, hi, gen, nonzero=True, device=None):
    """Integer-valued fp32 tensor, entries uniform in [lo, hi]; nonzero=True never returns
    0 (so every k-term of a product counts).  Generated on ``gen``'s device (a CPU or a
    GPU torch.Generator), then moved to ``device`` when one is given."""
    if nonzero and lo <= 0 <= hi:
        v = torch.randint(lo, hi, shape, generator=gen, device=gen.device)
        v = torch.where(v >= 0, v + 1, v)  # hi - lo values, 0 skipped
    else:
        v = torch.randint(lo, hi + 1, shape, generator=gen, device=gen.device)
    v = v.to(torch.float32)
    return v if device is None else v.to(device)


def _mantissas(shape, gen):
    m = torch.randint(1 << 23, 1 << 24, shape, generator=gen, device=gen.device)  # 24 bits
    return m.to(torch.float32) * 2.0 ** -23  # exact: in [1, 2), no denormals


def full_mantissa(shape, gen, device=None):
    """Dense fp32 tensor of values m * 2^-23, m a random integer in [2^23, 2^24)."""
    v = _mantissas(shape, gen)
    return v if device is None else v.to(device)


def one_hot_rows(M, K, gen, device=None):
    """[M, K] fp32 with exactly one nonzero per row, at a random k, a full_mantissa value."""
    out = torch.zeros(M, K, device=gen.device)
    k = torch.randint(0, K, (M,), generator=gen, device=gen.device)
    out[torch.arange(M, device=gen.device), k] = _mantissas((M,), gen)
    return out if device is None else out.to(device)


def padded(t, pad_rows, pad_cols, fill):
    """A view holding ``t`` inside a larger [rows + pad_rows, cols + pad_cols] buffer filled
    with ``fill`` (stride(0) > shape[1]); the pads sit after the last row / column.  Use
    fill = NaN for operands, SENTINEL for outputs.  ``view._base`` is the whole buffer."""
    r, c = t.shape
    buf = torch.full((r + pad_rows, c + pad_cols), fill, dtype=t.dtype, device=t.device)
    view = buf[:r, :c]
    view.copy_(t)
    return view


def pads_intact(view, fill=SENTINEL):
    """True when everything of ``view``'s buffer outside the view still holds ``fill``
    bitwise (pad columns and guard rows)."""
    buf = view._base
    r, c = view.shape
    f = torch.full((), fill, dtype=buf.dtype, device=buf.device)
    bits = lambda x: x.contiguous().view(torch.int32)  # noqa: E731
    return bool((bits(buf[:r, c:]) == bits(f)).all()) and bool((bits(buf[r:]) == bits(f)).all())


def exact_bound_ok(absA, absB, extra=0):
    """max(|A| @ |B|) + extra < 2^24: every partial sum of A @ B, in any order, is then an
    integer fp32 holds exactly (integer-valued operands).  A condition of a test, not a
    tolerance.  ``extra`` bounds whatever an epilogue adds (|bias|, |old C|)."""
    if absA.numel() == 0 or absB.numel() == 0:
        return extra < 2 ** 24
    return float((absA.double() @ absB.double()).max()) + extra < 2 ** 24


def truncate_mantissa(x, bits):
    """fp32 values with the stored mantissa cut to ``bits`` bits (toward zero): a model of
    a reduced-precision operand path (10: TF32, 7: bf16)."""
    drop = 23 - bits
    mask = torch.tensor(-(1 << drop), dtype=torch.int32)
    return (x.contiguous().view(torch.int32) & mask).view(torch.float32)


def fma_chain(A, B, order):
    """A @ B accumulated as a chain of fp32 fused multiply-adds over k in ``order``: float64
    holds each a*b of fp32 operands exactly, and for the inputs of this module acc + a*b is
    either exact in float64 too (integers) or a lone product (one-hot), so the one rounding
    to fp32 per step is fmaf's."""
    A64, B64 = A.numpy().astype(np.float64), B.numpy().astype(np.float64)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.float32)
    for k in order:
        acc = (acc.astype(np.float64) + np.outer(A64[:, k], B64[k])).astype(np.float32)
    return torch.from_numpy(acc)


def gemm_close(C, ref, absprod, K):
    """A copy of test_gpu_kernels.gemm_close's formula (that module imports the GPU-side
    oracle, so the CPU self-test takes the formula from here): |C - ref| <=
    1e-5*max(1,|ref|) + 2*K*2^-24*(|A||B|).  Returns (ok, worst |err| / tol)."""
    C, ref, absprod = (np.asarray(x, dtype=np.float64) for x in (C, ref, absprod))
    tol = 1e-5 * np.maximum(1.0, np.abs(ref)) + 2.0 * K * 2.0 ** -24 * absprod
    err = np.abs(C - ref)
    return bool((err <= tol).all()), float((err / tol).max())
