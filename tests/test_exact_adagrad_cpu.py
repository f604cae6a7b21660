"""CPU proofs for the element-wise Adagrad mode: exact_adagrad.ref_adagrad_elem equals
torch.optim.Adagrad bit for bit (its sparse form on an nn.EmbeddingBag(sparse=True), its dense
form on the coalesced gradient); the fp32 / fp64 twin that conditions the engine's trajectory
tests; optim.Adagrad's argument checks; the C ABI at v19."""
import os
import re

import numpy as np
import pytest
import torch

import exact_adagrad as A
import exact_tbe as E
from conftest import ROOT

CASES = {"skewed": E.skewed_case, "structure": E.structure_case, "cancel": E.cancel_case}
CASES.update({c.name: (lambda c=c: c) for c in E.small_n_cases()})


def _setup(name, D, weighted):
    c = CASES[name]()
    zero = int(c.runs_spec[c.runs_spec[:, 1] == 2][0, 2]) if name == "cancel" else None
    o = E.operands_for(c, D, weighted, seed=D + 7 * weighted, zero_row=zero)
    return c, o, E.coalesced_grad(c, o), A.start_state(o)


def _full(c, o, vals, fill):
    out = torch.full((c.total_rows, vals.shape[1]), fill, dtype=torch.float32)
    out[torch.from_numpy(o.urows)] = vals
    return out


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name,D", [("skewed", 1), ("skewed", 5), ("skewed", 16), ("cancel", 16),
                                    ("n1", 16), ("n7", 128), ("n128", 16), ("structure", 16)])
def test_reference_equals_torch_adagrad_sparse_and_dense(name, D, weighted):
    c, o, gsum, S0 = _setup(name, D, weighted)
    assert bool((S0 == 0).any()) and bool((S0 > 0).any()) and bool((S0 >= 0).all())
    Wref, Sref = A.ref_adagrad_elem(o.W0u, S0, gsum, o.lr, o.eps)
    u = torch.from_numpy(o.urows)
    # dense form: the whole table, the coalesced gradient (zero on the untouched rows)
    W = torch.nn.Parameter(_full(c, o, o.W0u, 3.0))
    opt = torch.optim.Adagrad([W], lr=o.lr, eps=o.eps)
    opt.state[W]["sum"].copy_(_full(c, o, S0, 2.0))
    W.grad = _full(c, o, gsum.float(), 0.0)
    opt.step()
    assert E.bits_equal(W.detach()[u], Wref) and E.bits_equal(opt.state[W]["sum"][u], Sref)
    keep = torch.ones(c.total_rows, dtype=torch.bool)
    keep[u] = False
    assert bool((W.detach()[keep] == 3.0).all()) and bool((opt.state[W]["sum"][keep] == 2.0).all())
    # sparse form: one EmbeddingBag(sparse=True) per table on the same lookups
    for t in range(c.T):
        idx, off, sel = A.table_csr(c, t)
        if idx.size == 0:
            continue
        lo, hi = int(c.row_base[t]), int(c.row_base[t + 1])
        emb = torch.nn.EmbeddingBag(hi - lo, D, mode="sum", sparse=True)
        emb.weight.data = _full(c, o, o.W0u, 3.0)[lo:hi].clone()
        opt = torch.optim.Adagrad(emb.parameters(), lr=o.lr, eps=o.eps)
        opt.state[emb.weight]["sum"].copy_(_full(c, o, S0, 2.0)[lo:hi])
        psw = None if o.psw is None else o.psw[torch.from_numpy(sel)]
        out = emb(torch.from_numpy(idx), torch.from_numpy(off), per_sample_weights=psw)
        (out * o.G[:, t]).sum().backward()
        assert emb.weight.grad.is_sparse
        opt.step()
        mine = (o.urows >= lo) & (o.urows < hi)
        k = torch.from_numpy(o.urows[mine] - lo)
        m = torch.from_numpy(mine)
        assert E.bits_equal(emb.weight.detach()[k], Wref[m]), (name, D, t)
        assert E.bits_equal(opt.state[emb.weight]["sum"][k], Sref[m]), (name, D, t)


def test_reference_rounds_and_holds_a_cancelled_row():
    """The reference does round (the test is no integer identity), and a row whose gradient
    cancels keeps W and S."""
    c, o, gsum, S0 = _setup("cancel", 16, False)
    W, S = A.ref_adagrad_elem(o.W0u, S0, gsum, o.lr, o.eps)
    exact = o.W0u.double() - o.lr * gsum / (S.double().sqrt() + o.eps)
    assert not torch.equal(W.double(), exact)
    k = int(np.searchsorted(o.urows, int(c.runs_spec[c.runs_spec[:, 1] == 2][0, 2])))
    assert not gsum[k].any() and torch.equal(W[k], o.W0u[k]) and torch.equal(S[k], S0[k])


def test_reference_asserts_its_conditions():
    c, o, gsum, S0 = _setup("n7", 16, False)
    with pytest.raises(AssertionError):
        A.ref_adagrad_elem(o.W0u, S0, gsum, 0.05, o.eps)  # lr no power of two
    with pytest.raises(AssertionError):
        A.ref_adagrad_elem(o.W0u, S0 + 2.0 ** 24, gsum, o.lr, o.eps)
    with pytest.raises(AssertionError):
        A.ref_adagrad_elem(o.W0u, S0 + 0.5, gsum, o.lr, o.eps)


@pytest.mark.parametrize("name", sorted(A.TRAJ_CASES) + ["two_ranks"])
def test_trajectory_cases_are_well_conditioned(name):
    """The fp32 oracle against its fp64 copy over every trajectory case of
    test_gpu_trainer_adagrad.py (the two-rank case included) at the case's adagrad_eps:
    everything those tests compare - every step's Z and loss, every parameter and every Adagrad
    sum after the last step - within TWIN_BOUND (1e-6), a tenth of fp32_close's tolerance."""
    import oracle as O
    eps = A.TWO_RANKS["eps"] if name == "two_ranks" else A.TRAJ_EPS[name]
    spread, loss, sums = A.twin_spread(O, name, eps)
    print(f"{name}: eps {eps:g}, fp32 vs fp64 oracle: Z and parameters "
          f"{spread:.3e}, loss {loss:.3e}, Adagrad sums {sums:.3e}")
    assert spread <= A.TWIN_BOUND, (name, "Z and parameters", spread)
    assert loss <= A.TWIN_BOUND, (name, "loss", loss)
    assert sums <= A.TWIN_BOUND, (name, "Adagrad sums", sums)


def test_default_eps_is_ill_conditioned_for_a_tolerance():
    """Why the trajectories do not run at the default eps = 1e-10: there the fp32 oracle
    alone leaves fp32_close's 1e-5 (the bitwise tests cover that eps instead)."""
    import oracle as O
    assert A.twin_spread(O, "plain_multihot", 1e-10)[0] > 1e-5


# ------------------------------------------------------------------ optim.Adagrad ----
def test_optim_adagrad_argument_checks():
    from dlrm_hip import optim
    p = torch.nn.Parameter(torch.zeros(4, 8))
    for kw in (dict(lr=-1.0), dict(lr_decay=-0.1), dict(weight_decay=-0.1),
               dict(initial_accumulator_value=-1.0), dict(eps=-1e-3)):
        with pytest.raises(ValueError):
            optim.Adagrad([p], **kw)
    opt = optim.Adagrad([p], lr=0.5, lr_decay=0.1, weight_decay=0.0,
                        initial_accumulator_value=0.25, eps=1e-8)
    ref = torch.optim.Adagrad([p], lr=0.5, lr_decay=0.1, initial_accumulator_value=0.25,
                              eps=1e-8)
    assert set(opt.state[p]) == set(ref.state[p]) == {"sum", "step"}
    assert torch.equal(opt.state[p]["sum"], ref.state[p]["sum"])
    a, b = opt.state[p]["step"], ref.state[p]["step"]  # state_dicts swap between the classes
    assert type(a) is type(b) and a.dtype == b.dtype and a.device == b.device and a == b
    for k in ("lr", "lr_decay", "weight_decay", "initial_accumulator_value", "eps"):
        assert opt.param_groups[0][k] == ref.param_groups[0][k]
    # weight_decay with a sparse gradient: torch's RuntimeError, before any kernel runs
    opt = optim.Adagrad([p], weight_decay=0.1)
    p.grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.ones(1, 8), (4, 8))
    with pytest.raises(RuntimeError, match="weight_decay option is not compatible with sparse"):
        opt.step()


def test_trainer_config_refuses_fp16_tables_with_adagrad():
    from dlrm_hip.trainer import TrainerConfig
    kw = dict(m_spa=8, ln_emb=[10, 10], ln_bot=[13, 8], ln_top=[11, 1])
    with pytest.raises(NotImplementedError, match="DESIGN.md §22"):
        TrainerConfig(**kw, optimizer="adagrad", emb_precision="fp16")
    assert TrainerConfig(**kw, optimizer="adagrad").optimizer == "adagrad"


# ------------------------------------------------------------------------- ABI ----
_CTYPE = {"float*": "P", "const float*": "P", "const int64_t*": "P", "const void*": "P",
          "void*": "P", "int32_t*": "P", "dlrm_stream_t": "P", "int64_t": "c_int64",
          "int32_t": "c_int32", "float": "c_float", "size_t": "c_size_t"}


def _prototype(name):
    txt = open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/dlrm_hip.h"
    return [" ".join(a.split()[:-1]) for a in m.group(1).split(",")]


def test_abi_v19_declares_and_binds_the_adagrad_entry_point():
    import ctypes
    from dlrm_hip import _lib
    hdr = open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()
    assert int(re.search(r"#define\s+DLRM_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 19
    assert _lib.ABI_VERSION >= 19
    names = {"P": ctypes.c_void_p, "c_int64": ctypes.c_int64, "c_int32": ctypes.c_int32,
             "c_float": ctypes.c_float, "c_size_t": ctypes.c_size_t}
    args = _prototype("dlrm_tbe_backward_adagrad")
    res, sig = _lib.SIGNATURES["dlrm_tbe_backward_adagrad"]
    assert res is ctypes.c_int32
    assert [names[_CTYPE[a]] for a in args] == sig
    # the argument list of dlrm_tbe_backward_rowwise_adagrad up to grad_batch_stride, then
    # lr, lr_dev, eps and the common tail
    rws = _prototype("dlrm_tbe_backward_rowwise_adagrad")
    assert args[:15] == rws[:15]
    assert args[15:18] == ["float", "const float*", "float"] and args[18:] == rws[17:]
    lib = _lib.load()
    assert hasattr(lib, "dlrm_tbe_backward_adagrad")
    with pytest.raises(_lib.DLRMHipError) as e:  # a null state_sum is INVALID_ARG
        _lib.call("dlrm_tbe_backward_adagrad", None, None, 16, None, 1, 1, None, 32, None, 32,
                  0, 4, None, None, 16, 0.1, None, 1e-10, 0, None, 0, None, 0, None)
    assert e.value.code == 1 and "state_sum" in str(e.value)
