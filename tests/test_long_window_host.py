"""Host-only length checks of the HIP path (engine.sequence_length) at the reference's window lengths, and the CPU replica of the
long attention core's 64-bit dropout index (tests/dropout64.py) against the 32-bit one below 2^32.  No GPU needed."""
import copy
import json

import numpy as np
import pytest

from eyegaze_multimodal_amd import _lib as L
from eyegaze_multimodal_amd import train_art as TA
from eyegaze_multimodal_amd.engine import ATTN_LONG_MAX_S, sequence_length
from tests.dropout64 import attn_element_index, hip_keep_mask64
from tests.helpers import GOLDEN, hip_keep_mask


def model_cfg(name, window):
    fx = json.loads((GOLDEN / "reference_configs.json").read_text())
    cfg = copy.deepcopy(next(e["config"] for e in fx["entries"] if e["name"] == name))
    cfg["data"]["window_size"] = window
    return TA.build_model(cfg, compute_dtype="bf16").cfg


@pytest.mark.parametrize("name,window,S", [("A2_plus_spectrogram", 2048, 161), ("A1_baseline_temporal_only", 8192, 513),
                                           ("A5_full_model", 2048, 203), ("A1_baseline_temporal_only", 4096, 257),
                                           ("A2_plus_spectrogram", 4096, 289), ("A5_full_model", 1024, 139)])
def test_long_windows_pass_the_length_checks(name, window, S):
    assert sequence_length(model_cfg(name, window), window) == S


def test_sequence_past_the_attention_limit_is_refused_naming_it():
    assert ATTN_LONG_MAX_S == 2048
    cfg = model_cfg("A1_baseline_temporal_only", 32768)          # S = 1 + 32768 / 16 = 2049, max_len 8192
    with pytest.raises(L.EgError, match="limit of 2048"):
        sequence_length(cfg, 32768)


def test_ibs_window_limit_is_refused_with_its_own_message():
    cfg = model_cfg("A5_full_model", 4096)                       # S = 331 would run; the synchrony kernels stop at T = 2048
    with pytest.raises(L.EgError, match="IBS"):
        sequence_length(cfg, 4096)


def test_positional_table_limit_still_applies():
    cfg = model_cfg("A1_baseline_temporal_only", 1024)           # max_len = 256
    with pytest.raises(L.EgError, match="max_len 256"):
        sequence_length(cfg, 8192)


def test_64_bit_mask_equals_the_32_bit_mask_below_2_to_the_32():
    rng = np.random.default_rng(0)
    idx = np.concatenate([rng.integers(0, 1 << 32, 200_000, dtype=np.uint64),
                          np.arange((1 << 32) - 64, 1 << 32, dtype=np.uint64), np.arange(64, dtype=np.uint64),
                          np.arange((1 << 31) - 32, (1 << 31) + 32, dtype=np.uint64)])
    for seed, site, p in [(0x1234_5678_9ABC, 16, 0.1), (7, 31, 0.25)]:
        assert (hip_keep_mask64(seed, site, idx, p) == hip_keep_mask(seed, site, idx.astype(np.uint32), p)).all()


def test_64_bit_mask_does_not_wrap():
    """above 2^32 the mask is not a copy of the one 2^32 elements earlier (what a wrapping 32-bit index would draw)"""
    idx = attn_element_index(200, 8, 2048)[:, :64].reshape(-1)
    assert int(idx.min()) >= 1 << 32
    hi = hip_keep_mask64(9, 16, idx, 0.25)
    lo = hip_keep_mask64(9, 16, idx - np.uint64(1 << 32), 0.25)
    assert 0.7 < hi.mean() < 0.8 and (hi != lo).mean() > 0.3
