"""The exact-arithmetic input generators (tests/exact_inputs.py) do what they promise, and
the comparisons built on them fail for the right reasons - shown here on the CPU, with
models of the kernel bugs they are meant to catch (a dropped k-term, reduced operand
precision, a pad that reaches the sum)."""
import numpy as np
import torch

import exact_inputs as X

M, N, K = 130, 70, 2048


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_int_matrix_range_and_nonzero():
    g = _gen(0)
    a = X.int_matrix((200, 300), -4, 4, g)
    assert a.dtype == torch.float32 and torch.equal(a, a.round())
    assert a.min() == -4 and a.max() == 4 and not (a == 0).any()
    assert sorted(a.unique().tolist()) == [-4, -3, -2, -1, 1, 2, 3, 4]
    b = X.int_matrix((200, 300), -2, 2, g, nonzero=False)
    assert sorted(b.unique().tolist()) == [-2, -1, 0, 1, 2]
    c = X.int_matrix((50, 50), 1, 3, g)  # a range without 0
    assert sorted(c.unique().tolist()) == [1, 2, 3]


def test_full_mantissa_and_one_hot_values():
    g = _gen(1)
    d = X.full_mantissa((64, 96), g)
    assert d.dtype == torch.float32 and d.min() >= 1.0 and d.max() < 2.0
    m = d.double() * 2.0 ** 23
    assert torch.equal(m, m.round())  # m * 2^-23 with integer m
    # the low mantissa bits are in use (a 10-bit truncation moves nearly every value)
    assert (X.truncate_mantissa(d, 10) != d).float().mean() > 0.99
    h = X.one_hot_rows(M, K, g)
    assert h.shape == (M, K) and ((h != 0).sum(1) == 1).all()
    nz = h[h != 0]
    assert nz.min() >= 1.0 and nz.max() < 2.0
    assert len(set(h.nonzero()[:, 1].tolist())) > M // 2  # random k, not one column


def test_padded_views_and_pad_check():
    t = torch.arange(12, dtype=torch.float32).view(3, 4)
    v = X.padded(t, 2, 4, float("nan"))
    assert v.shape == (3, 4) and v.stride() == (8, 1) and torch.equal(v, t)
    assert v._base.shape == (5, 8) and v.data_ptr() == v._base.data_ptr()
    assert torch.isnan(v._base[:, 4:]).all() and torch.isnan(v._base[3:]).all()
    c = X.padded(torch.zeros(3, 4), 2, 4, X.SENTINEL)
    assert X.pads_intact(c)
    c.fill_(1.0)
    assert X.pads_intact(c)  # writes inside the view do not count
    c._base[1, 5] = 0.0
    assert not X.pads_intact(c)  # a pad column
    c._base[1, 5] = X.SENTINEL
    c._base[4, 0] = 7.0
    assert not X.pads_intact(c)  # a guard row
    c._base[4, 0] = X.SENTINEL
    assert X.pads_intact(c)


def test_exact_bound_ok_is_the_2_pow_24_condition():
    a = torch.full((1, 4), 2.0 ** 11)
    b = torch.full((4, 1), 2.0 ** 10)
    assert X.exact_bound_ok(a, b)  # 4 * 2^21 = 2^23
    assert not X.exact_bound_ok(a, b, extra=2 ** 23)
    assert not X.exact_bound_ok(a * 2, b)  # 2^24 itself is outside
    assert X.exact_bound_ok(torch.zeros(3, 0), torch.zeros(0, 5), extra=8)


def test_integer_products_are_exact_in_any_order_and_split():
    """Integer operands in [-4, 4] at K = 2048: fp32 fmaf chains in random k-orders, and 2,
    5 and 16 split partial sums added afterwards, all equal the fp64 product bitwise; a
    dropped or doubled k-term, or one NaN pad element reaching the sum, does not."""
    g = _gen(2)
    A = X.int_matrix((M, K), -4, 4, g)
    B = X.int_matrix((K, N), -4, 4, g)
    assert X.exact_bound_ok(A.abs(), B.abs())
    ref = (A.double() @ B.double()).float()
    assert torch.equal(ref.double(), A.double() @ B.double())  # the cast loses nothing
    rng = np.random.RandomState(0)
    for _ in range(3):
        assert torch.equal(X.fma_chain(A, B, rng.permutation(K)), ref)
    for s in (2, 5, 16):
        chunk = -(-K // s)
        parts = [X.fma_chain(A[:, k0:k0 + chunk], B[k0:k0 + chunk], range(min(chunk, K - k0)))
                 for k0 in range(0, K, chunk)]
        assert len(parts) == s
        tot = parts[0]
        for p in parts[1:]:
            tot = tot + p  # fp32 adds, in split order
        assert torch.equal(tot, ref)
    # the bugs the comparison is for: every output element changes
    order = list(range(K))
    dropped = X.fma_chain(A, B, order[:777] + order[778:])
    assert (dropped != ref).all()
    doubled = X.fma_chain(A, B, order + [5])
    assert (doubled != ref).all()
    Ap = X.padded(A, 2, 4, float("nan"))
    leak = Ap._base[:M, :K + 1].double() @ torch.cat([B.double(), torch.zeros(1, N, dtype=torch.float64)])
    assert torch.isnan(leak).all()  # a pad column read, even times a masked-to-zero B row


def test_one_hot_product_is_one_rounding_and_sees_lost_mantissa_bits():
    """A one-hot (per row) times a dense full-mantissa B: the fp32 fmaf chain equals the
    fp64 product rounded once; operands truncated to 10 (TF32) or 7 (bf16) mantissa bits
    change more than 99 % of the outputs.  The same with the roles swapped."""
    g = _gen(3)
    A = X.one_hot_rows(M, K, g)
    B = X.full_mantissa((K, N), g)
    ref = (A.double() @ B.double()).float()
    assert (ref.double() != A.double() @ B.double()).float().mean() > 0.9  # rounding happens
    assert torch.equal(X.fma_chain(A, B, range(K)), ref)
    assert torch.equal(X.fma_chain(A, B, np.random.RandomState(1).permutation(K)), ref)
    for bits in (10, 7):
        for ta, tb in ((True, True), (True, False), (False, True)):
            At = X.truncate_mantissa(A, bits) if ta else A
            Bt = X.truncate_mantissa(B, bits) if tb else B
            got = (At.double() @ Bt.double()).float()
            assert (got != ref).float().mean() > 0.99, (bits, ta, tb)
    A2 = X.full_mantissa((M, K), g)
    B2 = X.one_hot_rows(N, K, g).t().contiguous()  # one nonzero per column
    ref2 = (A2.double() @ B2.double()).float()
    assert torch.equal(X.fma_chain(A2, B2, range(K)), ref2)
    got = (X.truncate_mantissa(A2, 10).double() @ B2.double()).float()
    assert (got != ref2).float().mean() > 0.99


def test_gemm_close_tolerance_admits_a_10_bit_mantissa_product():
    """The gap the exact tests close: with randn operands at K = 2048 a product of operands
    truncated to a TF32-like 10-bit mantissa stays INSIDE gemm_close's tolerance (formula
    copied into exact_inputs.gemm_close from test_gpu_kernels.gemm_close), so the
    tolerance tests cannot see a reduced-precision GEMM body; the one-hot test above can."""
    g = _gen(4)
    A = torch.randn(M, K, generator=g)
    B = torch.randn(K, N, generator=g)
    ref = A.double() @ B.double()
    ap = A.double().abs() @ B.double().abs()
    trunc = X.truncate_mantissa(A, 10).double() @ X.truncate_mantissa(B, 10).double()
    ok, worst = X.gemm_close(trunc.numpy(), ref.numpy(), ap.numpy(), K)
    assert ok and 0.05 < worst < 1.0, worst
    assert (trunc.float() != ref.float()).float().mean() > 0.99  # yet it is not the product
