"""dlrm_interact_dot_forward_pool (ABI v20): the argument refusals, which need no GPU (every
check precedes the first HIP call; null pointers are enough)."""
import pytest

from dlrm_hip import _lib

F32, Q8 = 0, 2


def _call(B=4, F=3, D=16, fmt=F32, row_bytes=64):
    _lib.call("dlrm_interact_dot_forward_pool", B, F, D, None, D, None, fmt, row_bytes, None,
              None, None, 0, None, 64, None, 0, None, None)


@pytest.mark.parametrize("kw,status", [
    (dict(F=1), "INVALID_ARG"), (dict(F=33), "INVALID_ARG"), (dict(D=48), "UNSUPPORTED"),
    (dict(fmt=7), "UNSUPPORTED"), (dict(row_bytes=32), "INVALID_ARG"),
    (dict(fmt=Q8, row_bytes=16), "INVALID_ARG"), (dict(), "INVALID_ARG")])  # (): null pointers
def test_refusals(kw, status):
    with pytest.raises(_lib.DLRMHipError, match=status):
        _call(**kw)


def test_empty_batch_launches_nothing():
    _call(B=0)
    _call(B=0, fmt=Q8, row_bytes=24)
