"""Host side of the fp16 embedding tables (TrainerConfig.emb_precision = "fp16", ABI v15), no
GPU: the version in the header, the binding and the built library, the new entry points'
signatures against the header's prototypes, and the config field with its refusals."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

P = ctypes.c_void_p
NEW = {  # entry point -> (source file, number of arguments)
    "dlrm_interact_dot_forward_gather_f16": ("interact.hip", 13),
    "dlrm_interact_dot_backward_gather_f16": ("interact.hip", 15),
    "dlrm_tbe_backward_sgd_f16_dev": ("tbe_bwd.hip", 21),
}


def _header():
    return open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()


def _proto(hdr, name):
    text = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"(int|size_t) " + name + r"\((.*?)\);", text, flags=re.S)
    assert m, f"{name}: no prototype in the header"
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
             "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64}
    args = [a.strip() for a in m.group(2).split(",")]
    return [P if "*" in a or a.startswith("dlrm_stream_t") else ctype[a.split()[0]]
            for a in args]


def test_abi_version_is_15_everywhere():
    from dlrm_hip import _lib
    hdr = _header()
    assert int(re.search(r"#define\s+DLRM_ABI_VERSION\s+(\d+)", hdr).group(1)) >= 15
    assert re.search(r"^ \* 15:", hdr, flags=re.M)  # the version history line
    assert _lib.ABI_VERSION >= 15
    assert _lib.load().dlrm_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("name", sorted(NEW))
def test_new_entry_points_match_the_header(name):
    from dlrm_hip import _lib
    src_file, nargs = NEW[name]
    want = _proto(_header(), name)
    res, sig = _lib.SIGNATURES[name]
    assert res is ctypes.c_int32 and sig == want and len(sig) == nargs
    assert hasattr(_lib.load(), name)
    src = open(os.path.join(ROOT, "dlrm-yx_amd", "csrc", src_file)).read()
    assert f'extern "C" int {name}(' in src


def test_f16_entry_points_take_their_fp32_siblings_arguments():
    """The fp16 gathers take the fp32 gathers' argument lists, the device-rate fp16 update the
    device-rate fp32 update's (a `void*` row buffer where those take `float*`)."""
    from dlrm_hip import _lib
    for f16, f32 in (("dlrm_interact_dot_forward_gather_f16", "dlrm_interact_dot_forward_gather"),
                     ("dlrm_interact_dot_backward_gather_f16",
                      "dlrm_interact_dot_backward_gather"),
                     ("dlrm_tbe_backward_sgd_f16_dev", "dlrm_tbe_backward_sgd_dev")):
        assert _lib.SIGNATURES[f16] == _lib.SIGNATURES[f32]


def test_uniform_fill_at_binding():
    from dlrm_hip import _lib
    res, sig = _lib.SIGNATURES["dlrm_uniform_fill_at"]
    assert res is ctypes.c_int32 and sig == _proto(_header(), "dlrm_uniform_fill_at")
    assert hasattr(_lib.load(), "dlrm_uniform_fill_at")


KW = dict(m_spa=4, ln_emb=[8], ln_bot=[4, 4], ln_top=[5, 1])


def test_emb_precision_field():
    from dlrm_hip.trainer import TrainerConfig
    assert TrainerConfig(**KW).emb_precision == "fp32"
    assert TrainerConfig(**KW, emb_precision="fp16").emb_precision == "fp16"
    both = TrainerConfig(**KW, emb_precision="fp16", mlp_precision="bf16", device_lr=True)
    assert (both.emb_precision, both.mlp_precision, both.lr_mode) == ("fp16", "bf16", "device")


@pytest.mark.parametrize("bad", ["bf16", "int8", "fp8", "half", ""])
def test_unknown_emb_precision_is_a_value_error(bad):
    from dlrm_hip.trainer import TrainerConfig
    with pytest.raises(ValueError):
        TrainerConfig(**KW, emb_precision=bad)


def test_fp16_refuses_what_it_cannot_run():
    from dlrm_hip.trainer import TrainerConfig
    for extra in (dict(optimizer="rwsadagrad"), dict(qr_flag=True)):
        with pytest.raises(NotImplementedError) as e:
            TrainerConfig(**KW, emb_precision="fp16", **extra)
        assert "DESIGN.md §18" in str(e.value)
        TrainerConfig(**KW, **extra)  # fp32 tables keep both
    wide = dict(KW, m_spa=516, ln_bot=[4, 516], ln_top=[517, 1])
    with pytest.raises(NotImplementedError) as e:
        TrainerConfig(**wide, emb_precision="fp16")
    assert "DESIGN.md §18" in str(e.value)
    odd = dict(KW, m_spa=6, ln_bot=[4, 6], ln_top=[7, 1])
    with pytest.raises(NotImplementedError):
        TrainerConfig(**odd, emb_precision="fp16")
