"""TEST INFRASTRUCTURE -- the entropy fixture (tests/golden/entropy.npz) and what both test modules compute from it
once: the restatement's float32 filtered rows (the filters are Python loops)."""
from pathlib import Path

import numpy as np

from tests import entropy_ref as ER

Z = np.load(Path(__file__).resolve().parent / "golden" / "entropy.npz")
FS = float(Z["sampling_rate"])
EEG_NAMES = [str(n) for n in Z["eeg/names"]]
IMAGE_NAMES = [str(n) for n in Z["image/names"]]
TOL_SPECTRAL = float(Z["tolerance/spectral"])
TOL_SPATIAL = float(Z["tolerance/spatial"])
TABLE_COLUMNS = ["pair_id", "player", "trial_idx", "condition", "spatial_entropy", "mean_entropy"]
_filtered = {}


def raw(name):
    return Z[f"eeg/{name}/raw"]


def reference_entropy(name):
    return Z[f"eeg/{name}/entropy"]


def filtered(name):
    """the restatement's band-passed rows of a recording, rounded to float32 as the device stores them"""
    if name not in _filtered:
        _filtered[name] = ER.filtered_ref(raw(name), FS)
    return _filtered[name]


def image(name):
    return Z[f"image/{name}/pixels"]


def image_entropy(name, normalize=True):
    return float(Z[f"image/{name}/entropy" if normalize else f"image/{name}/entropy_raw"])


def _py(v):
    return v.item() if isinstance(v, np.generic) else v


def table_rows(prefix="table", columns=TABLE_COLUMNS):
    cols = [Z[f"{prefix}/{c}"] for c in columns]
    return [{c: (str(v) if isinstance(v, np.str_) else _py(v)) for c, v in zip(columns, row)} for row in zip(*cols)]
