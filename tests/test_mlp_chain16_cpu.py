"""Host side of the 16-bit bottom-MLP chain (no GPU): ops.mlp_chain16's refusals, which run
before the library is loaded, and dlrm_mlp_chain16's argument checks, which run before the
first HIP call."""
import ctypes

import pytest
import torch


def _layers(widths=(13, 32, 8), rows=4):
    X = torch.zeros(rows, widths[0])
    return X, [[torch.zeros(n, k), torch.zeros(n), torch.zeros(rows, n)]
               for k, n in zip(widths, widths[1:])]


@pytest.mark.parametrize("what,match", [
    ("dtype", "dtype"), ("last_y", "last layer's Y"), ("bias", "bias"), ("width", "wide"),
    ("cpu", "device tensors")])
def test_ops_refusals(what, match):
    from dlrm_hip import ops
    X, layers = _layers()
    dtype = "int8" if what == "dtype" else "bf16"
    if what == "last_y":
        layers[-1][2] = None
    elif what == "bias":
        layers[0][1] = torch.zeros(31)
    elif what == "width":
        layers[1][0] = torch.zeros(8, 33)
    with pytest.raises(ValueError, match=match):
        ops.mlp_chain16(X, layers, dtype=dtype)


def test_abi_argument_checks_without_a_device():
    from dlrm_hip import _lib
    lib = _lib.load()
    OK, INVALID, SHAPE, UNSUPPORTED = 0, 1, 2, 3

    def status(**kw):
        c = _lib.MlpChain16(type=0, layers=2, rows=0, X=4096, ldx=13, in_width=13)
        for l, (k, n) in enumerate(((13, 32), (32, 8))):
            c.out_width[l], c.W[l], c.ldw[l], c.Y[l], c.ldy[l] = n, 4096, k, 4096, n
        for name, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, name)[v[0]] = v[1]
            else:
                setattr(c, name, v)
        rc = lib.dlrm_mlp_chain16_forward(ctypes.byref(c), None)
        assert bool(lib.dlrm_mlp_chain16_supported(ctypes.byref(c))) == (rc == OK)
        return rc

    assert status() == OK  # rows = 0: nothing to launch
    assert status(type=2) == INVALID and status(rows=-1) == INVALID
    assert status(layers=0) == UNSUPPORTED and status(layers=5) == UNSUPPORTED
    assert status(in_width=513, ldx=513) == UNSUPPORTED and status(in_width=0) == UNSUPPORTED
    assert status(out_width=(1, 513), ldy=(1, 513)) == UNSUPPORTED
    assert b"out_width[1] = 513" in lib.dlrm_last_error()
    assert status(ldx=12) == SHAPE and status(ldw=(1, 31)) == SHAPE and status(ldy=(0, 31)) == SHAPE
    # a null required pointer (with rows to work on; refused before any launch)
    assert status(rows=4, X=None) == INVALID and status(rows=4, W=(1, None)) == INVALID
    assert status(rows=4, Y=(1, None)) == INVALID
