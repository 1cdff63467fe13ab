"""Loader of the head-width-64 fixtures (tests/golden/hd64_*.npz, written by tests/make_golden_hd64.py).  A fixture that would
pass the file-size limit is stored in two parts (<name>.npz and <name>_gen_eeg.npz); this reads them back as one, with the
interface of tests.helpers.load_golden so that the oracle's check functions run on it unchanged."""
import ast

import numpy as np

from oracle.dual_eeg_oracle import ModelCfg, synthetic_state_dict
from tests.helpers import GOLDEN, WEIGHT_SEED

HD64_CONFIGS = ["hd64_xattn", "hd64_full"]


class Parts:
    """the entries of several .npz files under one `files` list and one [] lookup"""

    def __init__(self, paths):
        self._z = [np.load(p, allow_pickle=False) for p in paths]
        self.files = [k for z in self._z for k in z.files]

    def __getitem__(self, key):
        for z in self._z:
            if key in z.files:
                return z[key]
        raise KeyError(key)


def load_hd64(name):
    assert name in HD64_CONFIGS
    paths = [GOLDEN / f"{name}.npz"]
    if (GOLDEN / f"{name}_gen_eeg.npz").exists():
        paths.append(GOLDEN / f"{name}_gen_eeg.npz")
    z = Parts(paths)
    kw = ast.literal_eval(str(z["cfg_json"]))
    cfg = ModelCfg(**kw)
    sd = synthetic_state_dict(cfg, WEIGHT_SEED)
    assert list(sd.keys()) == [str(k) for k in z["state_keys"]]
    return z, kw, cfg, sd
