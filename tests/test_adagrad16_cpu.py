"""fp16 rows under row-wise Adagrad, the parts that need no GPU: the header's
prototype against the ctypes one, the entry point's host refusals, TrainerConfig.emb_optimizer."""
import ctypes
import os
import re

import pytest

from dlrm_hip import _lib
from dlrm_hip.trainer import DLRMTrainer, TrainerConfig

NAME = "dlrm_tbe_backward_rowwise_adagrad_f16"
INVALID_ARG, UNSUPPORTED = 1, 3
PTR = 0x10000  # fake device pointer: these calls return before any HIP call


def test_header_prototype_matches_the_binding():
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "dlrm_hip.h")) as f:
        args = re.search(r"int " + NAME + r"\((.*?)\);", f.read(), re.S).group(1).split(",")
    types = [re.sub(r"\s*\w+$", "", a.strip().replace("const ", "")) for a in args]
    want = [ctypes.c_void_p if "*" in t or t == "dlrm_stream_t" else
            getattr(ctypes, "c_" + (t if t == "size_t" else t.replace("_t", ""))) for t in types]
    assert _lib.SIGNATURES[NAME] == (ctypes.c_int32, want)
    assert _lib.ABI_VERSION == 23 == _lib.load().dlrm_abi_version()


def _call(D=8, **change):
    v = dict(weights=PTR, momentum=PTR, D=D, row_base=PTR, T=2, B=3, indices=PTR, index_bits=32,
             offsets=PTR, offset_bits=64, N=6, total_rows=100, psw=None, grad=PTR, gbs=2 * D,
             lr=0.1, lr_dev=None, eps=1e-8, sr_state=None, mx=0, ws=PTR,
             ws_bytes=_lib.query("dlrm_tbe_backward_workspace_size", 6, 100, D), err=None,
             presorted=0, stream=None)
    v.update(change)
    _lib.call(NAME, *v.values())


@pytest.mark.parametrize("code,word,change", [
    (INVALID_ARG, "null pointer", dict(weights=None)),
    (INVALID_ARG, "null momentum", dict(momentum=None)),
    (INVALID_ARG, "8-byte aligned", dict(sr_state=PTR + 4)),
    (UNSUPPORTED, "D=2052 too large", dict(D=2052))])
def test_host_refusals_are_the_siblings(code, word, change):
    with pytest.raises(_lib.DLRMHipError) as e:
        _call(**change)
    assert e.value.code == code and NAME in str(e.value) and word in str(e.value)
    for sr in (None, PTR):  # no lookups: OK under either store
        _call(N=0, indices=None, offsets=None, ws=None, ws_bytes=0, sr_state=sr)


def _cfg(m_spa=16, **kw):
    return TrainerConfig(m_spa=m_spa, ln_emb=[40, 30], ln_bot=[13, m_spa], ln_top=[m_spa + 3, 1],
                         **kw)


def test_emb_optimizer_validation():
    assert _cfg().emb_optimizer is None and _cfg(optimizer="rwsadagrad").emb_opt == "rwsadagrad"
    assert _cfg(optimizer="rwsadagrad", emb_optimizer="sgd").emb_opt == "sgd"
    for kw in (dict(emb_optimizer="adagrad"), dict(emb_optimizer="adam"),
               dict(optimizer="adagrad", emb_optimizer="sgd"),
               dict(optimizer="adagrad", emb_optimizer="rwsadagrad", emb_precision="fp16")):
        with pytest.raises(ValueError):
            _cfg(**kw)
    for dense in ("sgd", "rwsadagrad"):  # the new capability is a valid configuration
        _cfg(emb_precision="fp16", optimizer=dense, emb_optimizer="rwsadagrad",
             emb_rounding="stochastic", mlp_precision="bf16", device_lr=True)


@pytest.mark.parametrize("emb_opt,section", [(None, "§18"), ("rwsadagrad", "§26")])
def test_fp16_refusals_name_their_section(emb_opt, section):
    """emb_optimizer=None is the old behaviour in every respect: the §18 refusals stay."""
    cases = [dict(qr_flag=True), dict(m_spa=18), dict(m_spa=516)]
    for kw in cases + ([dict(optimizer="rwsadagrad")] if emb_opt is None else []):
        with pytest.raises(NotImplementedError, match=section):
            _cfg(emb_precision="fp16", emb_optimizer=emb_opt, **kw)
    with pytest.raises(NotImplementedError, match="§22"):  # element-wise Adagrad: fp32 tables
        _cfg(emb_precision="fp16", optimizer="adagrad")
    with pytest.raises(NotImplementedError, match=section):  # refused before any device work
        DLRMTrainer(_cfg(emb_precision="fp16", emb_optimizer=emb_opt), device="cpu",
                    world_size=2)
