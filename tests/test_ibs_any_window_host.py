"""Host-only checks of synchrony (IBS) tokens at any window length in [64, 2048]: the model-level length check, the C entry points'
bound (refused before any launch, so no GPU is needed) and the spectrum size against the fp32 band predicate of torch.fft."""
import copy
import json

import numpy as np
import pytest
import torch

from eyegaze_multimodal_amd import _lib as L
from eyegaze_multimodal_amd import train_art as TA
from eyegaze_multimodal_amd.engine import sequence_length
from eyegaze_multimodal_amd.tokens import ROBUST_BANDS, SCALAR_BANDS
from tests.helpers import GOLDEN


def model_cfg(name, window, fs=256):
    fx = json.loads((GOLDEN / "reference_configs.json").read_text())
    cfg = copy.deepcopy(next(e["config"] for e in fx["entries"] if e["name"] == name))
    cfg["data"]["window_size"] = window
    cfg["data"]["sampling_rate"] = fs
    return TA.build_model(cfg, compute_dtype="bf16").cfg


@pytest.mark.parametrize("name,window,fs,S", [("A5_full_model", 1000, 250, 138), ("A5_full_model", 2000, 256, 200),
                                              ("A3_plus_ibs_scalar", 1000, 250, 65), ("A3_plus_ibs_scalar", 1125, 250, 73),
                                              ("A5_full_model", 1021, 256, 139)])
def test_ibs_windows_that_are_not_powers_of_two_pass_the_length_checks(name, window, fs, S):
    assert sequence_length(model_cfg(name, window, fs), window) == S


def test_ibs_window_past_2048_is_still_refused_naming_ibs():
    cfg = model_cfg("A5_full_model", 4096)
    with pytest.raises(L.EgError, match="IBS"):
        sequence_length(cfg, 4096)


@pytest.mark.parametrize("T", [63, 2049])
def test_c_entry_points_refuse_windows_outside_64_to_2048(T):
    """fake pointers: the call is refused on the host before any launch"""
    import ctypes as C
    fake = 0x1000
    lo = (C.c_float * 6)(*[b[0] for b in ROBUST_BANDS])
    hi = (C.c_float * 6)(*[b[1] for b in ROBUST_BANDS])
    with pytest.raises(L.EgError, match=f"T={T}"):
        L.call("eg_ibs_analytic", fake, fake, fake, fake, fake, 8, T, 256.0, 8, C.addressof(lo), C.addressof(hi), 6, 0)
    with pytest.raises(L.EgError, match=f"T={T}"):
        L.call("eg_ibs_pairs", fake, fake, fake, fake, fake, 1, 4, T, 256.0, 8, C.addressof(lo), C.addressof(hi), 6, 0)


@pytest.mark.parametrize("fs", [128, 200, 250, 256, 500, 512])
def test_nbin_covers_every_bin_the_fp32_band_predicate_admits(fs):
    from eyegaze_multimodal_amd.tokens import nbin_for
    hi = max(b[1] for b in ROBUST_BANDS + SCALAR_BANDS)
    for T in range(64, 2049):
        n = nbin_for(T, fs, hi)
        freqs = torch.fft.rfftfreq(T, d=1.0 / fs)                # the oracle's band test (float32)
        admitted = torch.nonzero(freqs <= hi).flatten()
        assert int(admitted.max()) + 1 <= n <= T // 2 + 1, (T, fs, n)     # may keep one bin past the band: it is never read
        # the kernels' predicate: float(k) * float32(fs / T), the same fp32 frequencies
        k = np.arange(T // 2 + 1, dtype=np.float32)
        assert np.array_equal(k * (np.float32(fs) / np.float32(T)), freqs.numpy()), (T, fs)
        if T & (T - 1) == 0:                                       # unchanged wherever it was accepted before
            assert n == min(T // 2 + 1, int(hi * T / fs) + 1)
