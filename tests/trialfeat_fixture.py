"""TEST INFRASTRUCTURE -- the trial-features fixture (tests/golden/trial_features.npz) and its restatement, loaded and
computed once for every test module that needs them."""
from pathlib import Path

import numpy as np

from tests import trialfeat_ref as T

Z = np.load(Path(__file__).resolve().parent / "golden" / "trial_features.npz")
FS = int(Z["sampling_rate"])
TRIALS = [tuple(int(v) for v in row) for row in Z["trials"]]            # (C, L1, L2)
KEYS = ("time_domain", "freq_domain", "freq_bins", "bands_energy", "intra_con", "inter_con")
_restated = {}


def raw(t):
    return Z[f"raw/{t}/0"], Z[f"raw/{t}/1"]


def reference(t):
    return {k: Z[f"ref/{t}/{k}"] for k in KEYS if f"ref/{t}/{k}" in Z.files}


def _restate(t):
    if t not in _restated:
        cache = {}
        _restated[t] = {False: T.trial_features_ref(*raw(t), fs=FS, cache=cache),
                        True: T.trial_features_ref(*raw(t), fs=FS, sums32=True, cache=cache), "sides": cache["sides"], "z": cache["z"]}
    return _restated[t]


def restated(t, sums32=False):
    """both variants of the restatement per trial, computed once for every test that needs them (the filters are Python loops)"""
    return _restate(t)[sums32]


def band_sides(t):
    """[band][player] -> (band signal, amplitude, cos, sin), float32, of the restatement"""
    return _restate(t)["sides"]


def analytic_signals(t):
    """[band][player] -> the restatement's float64 analytic signal"""
    return _restate(t)["z"]
