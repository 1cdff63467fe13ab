"""
TEST INFRASTRUCTURE -- fixtures at attention head width 64 (d_model 128 with 2 heads), written by the reference through
oracle/make_golden.py, imported unchanged (so it runs only where the reference is mounted, as that module says).  B = 4.
The names carry no `tiny` prefix on purpose: with it run_config stores every gradient tensor and the files grow to 4-5 MB.

Usage:  python tests/make_golden_hd64.py
"""
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from oracle import make_golden as G  # noqa: E402

BASE = dict(in_channels=8, max_len=256, num_classes=3, d_model=128, num_layers=2, num_heads=2, d_ff=256)
CONFIGS = {
    "hd64_xattn": dict(BASE, use_spectrogram=False, use_ibs=False, use_cross_attention=True),     # S = 65
    "hd64_full": dict(BASE, use_spectrogram=True, use_ibs=True, use_robust_ibs=True),             # S = 115
}

FILE_LIMIT = 1 << 20     # no committed file is larger than 1 MiB


def split_if_large(path: Path):
    """A fixture above the file limit is rewritten as two: its `gen_eeg/` entries move to <name>_gen_eeg.npz, everything else stays.
    Nothing is dropped or altered; tests/hd64_golden.py reads the parts back as one fixture."""
    if path.stat().st_size <= FILE_LIMIT:
        return
    z = np.load(path, allow_pickle=False)
    part = {k: z[k] for k in z.files if k.startswith("gen_eeg/")}
    rest = {k: z[k] for k in z.files if not k.startswith("gen_eeg/")}
    np.savez_compressed(path, **rest)
    other = path.with_name(path.stem + "_gen_eeg.npz")
    np.savez_compressed(other, **part)
    for p in (path, other):
        assert p.stat().st_size <= FILE_LIMIT, (p, p.stat().st_size)
        print(f"  {p.name}: {p.stat().st_size / 1e6:.2f} MB")


if __name__ == "__main__":
    torch.set_num_threads(8)
    torch.manual_seed(0)
    G.B = 4
    model_mod, gen_mod, _ = G.load_reference()
    out_dir = REPO / "tests" / "golden"
    for name, kw in CONFIGS.items():
        G.run_config(name, kw, model_mod, gen_mod, out_dir)
        split_if_large(out_dir / f"{name}.npz")
