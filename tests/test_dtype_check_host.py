"""CPU-only: every entry point of include/eyegaze_hip.h that takes an `int dtype` validates it FIRST, through the one shared check
(csrc/common.h: eg_dtype_check).  Each is called with a bad dtype and every other argument zero: were its dtype check missing or
late, the call would be refused for its null pointers instead and the message would not match.  Nothing is launched."""
import ctypes as C
import re
from pathlib import Path

import pytest

from eyegaze_multimodal_amd import _lib as L

REPO = Path(__file__).resolve().parent.parent
PREDICATES = {"eg_attn_block_ok"}       # answers 0 / 1 for a dtype instead of failing
# the entry points that eg_dtype_check is asked to hold to bf16 / fp16 (f32_ok = false)
ONLY_16 = {"eg_gemm_tn_grouped256", "eg_token_grad_tail", "eg_heads_fwd", "eg_classifier_ce_bwd_fused", "eg_heads_bwd_chain",
           "eg_heads_bwd_pool", "eg_conv2d_wgrad_flat", "eg_conv2d_flat"}


def dtype_entry_points():
    """{name: index of its `int dtype` parameter} of every declared function that has one"""
    text = (REPO / "include" / "eyegaze_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for name, params in re.findall(r"\b(?:int|int64_t|const char\*)\s+(eg_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        params = [" ".join(p.split()) for p in params.split(",")]
        if "int dtype" in params and name not in PREDICATES:
            out[name] = params.index("int dtype")
    return out


ENTRY_POINTS = dtype_entry_points()


def zeros(name, dtype):
    """the argument list of `name`: the dtype, and zero for everything else (null pointers, sizes 0, rowmap(0))"""
    types = L.SIGNATURES[name]
    assert types[ENTRY_POINTS[name]] is C.c_int, name
    args = [L.rowmap(0) if t is L.RowMap else 0.0 if t is C.c_float else None if issubclass(t, C._Pointer) else 0 for t in types]
    args[ENTRY_POINTS[name]] = dtype
    return args


def test_the_header_scan_finds_the_entry_points():
    assert len(ENTRY_POINTS) >= 43 and ONLY_16 <= set(ENTRY_POINTS)
    assert {"eg_window_pack", "eg_pack_table_ex_check", "eg_layernorm_bwd", "eg_attention_long_bwd", "eg_conv2d_flat"} <= set(ENTRY_POINTS)
    assert set(ENTRY_POINTS) <= set(L.SIGNATURES)


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_a_bad_dtype_is_reported_before_anything_else(name):
    with pytest.raises(L.EgError, match="dtype 7"):
        L.call(name, *zeros(name, 7))


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_fp32_is_refused_exactly_where_only_16_bit_kernels_exist(name):
    """EG_F32 with zeros: the 16-bit-only entry points say so; every other one accepts the dtype and goes on to refuse the zeros (so
    a new 16-bit-only entry point has to be listed in ONLY_16)."""
    with pytest.raises(L.EgError) as e:
        L.call(name, *zeros(name, L.EG_F32))
    if name in ONLY_16:
        assert "bf16 / fp16 only" in str(e.value)
    else:
        assert "dtype" not in str(e.value)
