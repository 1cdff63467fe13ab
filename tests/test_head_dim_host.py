"""CPU-only: the head-width rule of the engine (engine.attention_head_dim: d_model / num_heads is 32 or 64) and the host-side
refusals of eg_attention_dk_fwd / _bwd / _probs.  The entry points are called with fake non-null pointers and arguments that the
host check refuses, so nothing is launched and nothing is dereferenced."""
from types import SimpleNamespace

import pytest

from eyegaze_multimodal_amd import _lib as L
from eyegaze_multimodal_amd.engine import attention_head_dim

F = 0x1000      # a non-null pointer that is never followed


def cfg(d, H):
    return SimpleNamespace(d_model=d, num_heads=H)


@pytest.mark.parametrize("d,H,want", [(128, 2, 64), (256, 4, 64), (512, 8, 64), (256, 8, 32)])
def test_head_dim_of_supported_configs(d, H, want):
    assert attention_head_dim(cfg(d, H)) == want


@pytest.mark.parametrize("d,H", [(256, 16), (256, 2), (100, 3)])
def test_other_head_dims_are_refused_naming_both_widths(d, H):
    with pytest.raises(L.EgError) as e:
        attention_head_dim(cfg(d, H))
    assert "32" in str(e.value) and "64" in str(e.value) and f"{d}/{H}" in str(e.value)


def fwd(NB=2, S=16, H=2, hd=64, kv=0, dtype=L.EG_BF16, p=0.0, st=0):
    return L.call("eg_attention_dk_fwd", F, F, F, NB, S, H, hd, kv, dtype, p, 3, st, 0)


def bwd(NB=2, S=16, H=2, hd=64, kv=0, dtype=L.EG_BF16, p=0.0, st=0, cap=None):
    return L.call("eg_attention_dk_bwd", F, F, F, F, F, NB, S, H, hd, kv, dtype, p, 3, st, F, NB * H * S if cap is None else cap, 0)


def probs(NB=2, S=16, H=2, hd=64, kv=0, dtype=L.EG_BF16, **_):
    return L.call("eg_attention_dk_probs", F, F, F, NB, S, H, hd, kv, dtype, 0)


ENTRIES = [fwd, bwd, probs]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("hd", [16, 128, 0, 48])
def test_head_dims_other_than_32_and_64_are_refused(entry, hd):
    with pytest.raises(L.EgError) as e:
        entry(hd=hd)
    assert "32" in str(e.value) and "64" in str(e.value) and f"head_dim={hd}" in str(e.value)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("hd", [32, 64])
def test_sequence_limit(entry, hd):
    with pytest.raises(L.EgError, match="2048"):
        entry(S=2049, hd=hd)


@pytest.mark.parametrize("hd", [32, 64])
def test_backward_scratch_capacity(hd):
    with pytest.raises(L.EgError, match="scratch"):
        bwd(NB=2, S=16, H=2, hd=hd, cap=2 * 2 * 16 - 1)


@pytest.mark.parametrize("entry", ENTRIES)
def test_kv_shift_equal_to_nb(entry):
    with pytest.raises(L.EgError, match="kv_shift"):
        entry(NB=2, kv=2)


@pytest.mark.parametrize("entry", [fwd, bwd])
def test_dropout_without_a_state(entry):
    with pytest.raises(L.EgError, match="step state"):
        entry(p=0.1, st=0)


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_dtype_comes_first(entry):
    with pytest.raises(L.EgError, match="dtype 7"):
        entry(dtype=7, hd=16, S=4096)
