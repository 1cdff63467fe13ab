"""
TEST INFRASTRUCTURE -- the fixture of the entropy analysis, written by the reference's own classes:
5_Metrics/entropy_calculators.py (SpectralEntropyCalculator, SpatialEntropyCalculator) and compute_summary_statistics of
7_Analysis/python_scripts/analyze_entropy.py, loaded by path and imported unchanged, so this runs only where the reference tree
(oracle.make_golden.REF), scipy, pandas, PIL and tqdm exist.  No reference source is copied; the file holds numbers and names only.
(The script imports its plotting module, which imports seaborn; where that is absent a stand-in module takes its name -- nothing
here plots.)

EEG rows, raw-like uV signals from make_golden_trial_features.raw_pair's recipe, at lengths chosen for a reason:
  256        one Welch segment
  257
  383        still one segment: the tail is dropped
  384        exactly two segments
  777
  3250       the dataset's trial length, at C = 3
and special rows: a 500-sample trial scaled by 1e-4 and a 1000-sample trial scaled by 1e-6 (the only rows on which a missing eps
or a wrong fs shows), a pure 10 Hz sine, an all-zero row and a constant 1234.5 row (both log2(129)).

Images, uint8: RGB 37 x 53, grey 64 x 64, channel-first (3, 40, 24), the (3, 5, 3) array the reference transposes, a constant 8 x 8
(exactly 6 bits), the script's focused 224 x 224 x 3 image (zeros with one 24 x 24 patch); and one float64 50 x 60 x 3.

Summaries: about 40 made-up entropies over 3 pairs x 2 players x 3 conditions with a group of one (its std is NaN).

Stored besides the inputs and the reference's outputs: the coefficients of (0.5, 50) at 250 Hz, of a band whose upper edge falls
between 0.99 and 0.999 of Nyquist and of a band below the 0.001 clamp; `restatement_err/spectral`, the largest distance of
tests/entropy_ref from the reference WHEN THE FILTERED SIGNAL IS ROUNDED TO FLOAT32 as the device's row store rounds it
(`restatement_err/spectral64`: with a float64 signal), `tolerance/spectral` twice the former, `restatement_err/spatial`.

Usage:  python tests/make_golden_entropy.py
"""
import importlib.util
import sys
from pathlib import Path
from unittest import mock

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from oracle.make_golden import REF  # noqa: E402
from tests import entropy_ref as ER  # noqa: E402
from tests.make_golden_trial_features import raw_pair  # noqa: E402

FS = 250.0
SEED = 20241020
EEG_LENGTHS = [(2, 256), (2, 257), (2, 383), (2, 384), (2, 777), (3, 3250)]          # (C, L)
COEF_BANDS = {"default": (0.5, 50.0), "upper": (0.5, 124.5), "lower": (0.1, 50.0)}    # 124.5 / 125 = 0.996; 0.1 / 125 < 0.001
FILE_LIMIT = 400_000
SPECTRAL_TOLERANCE_LIMIT = 1e-6      # anything looser could hide a symmetric window (3.9e-3), a missing bin doubling or mean removal
SPATIAL_GATE = 1e-10                 # derived in DESIGN.md §8n, not measured


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    calc = load("ref_entropy_calculators", REF / "5_Metrics" / "entropy_calculators.py")
    try:
        import seaborn  # noqa: F401
    except ImportError:
        sys.modules["seaborn"] = mock.MagicMock()
    script = load("ref_analyze_entropy", REF / "7_Analysis" / "python_scripts" / "analyze_entropy.py")
    return calc, script


def eeg_recordings(rng):
    """name -> (C, L) float32"""
    recs = {}
    for C, L in EEG_LENGTHS:
        recs[f"len{L}"] = raw_pair(rng, C, L, L)[0]
    recs["scaled_1e-4"] = (raw_pair(rng, 2, 500, 500)[0].astype(np.float64) * 1e-4).astype(np.float32)
    recs["scaled_1e-6"] = (raw_pair(rng, 2, 1000, 1000)[0].astype(np.float64) * 1e-6).astype(np.float32)
    t = np.arange(1024) / FS
    recs["special"] = np.stack([np.sin(2 * np.pi * 10.0 * t), np.zeros(1024), np.full(1024, 1234.5)]).astype(np.float32)
    return recs


def images(rng):
    focused = np.zeros((224, 224, 3), np.uint8)
    focused[100:124, 100:124] = 255
    return {"rgb_37x53": rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), "grey_64x64": rng.integers(0, 256, (64, 64), dtype=np.uint8),
            "planar_3x40x24": rng.integers(0, 256, (3, 40, 24), dtype=np.uint8), "planar_3x5x3": rng.integers(0, 256, (3, 5, 3), dtype=np.uint8),
            "constant_8x8": np.full((8, 8), 77, np.uint8), "focused_224": focused, "f64_50x60x3": rng.random((50, 60, 3))}


def summary_table(rng):
    rows = []
    for pair in (12, 13, 14):
        for player in ("playerA", "playerB"):
            for cond, n in (("Single", 3), ("Competition", 2), ("Cooperation", 2)):
                if (pair, player, cond) == (14, "playerB", "Cooperation"):
                    n = 1                                                     # the group of one: its std is NaN
                for k in range(n):
                    rows.append((pair, player, k + 1, cond, float(rng.normal(4.5, 0.4)), float(rng.normal(6.5, 0.2))))
    order = rng.permutation(len(rows))
    return [rows[i] for i in order]                                           # shuffled: the summary's order is the sort's


def build():
    import pandas as pd
    from scipy import signal
    calc, script = load_reference()
    from eyegaze_multimodal_amd import entropy as E
    assert list(calc.STANDARD_32_CHANNELS) == E.STANDARD_32_CHANNELS
    rng = np.random.default_rng(SEED)
    out = {"sampling_rate": np.float64(FS), "seed": np.int64(SEED)}
    for name, (lo, hi) in COEF_BANDS.items():
        b, a = signal.butter(4, [max(lo / (FS / 2), 0.001), min(hi / (FS / 2), 0.999)], btype="band")      # _design_bandpass_filter
        out[f"coef/{name}/band"], out[f"coef/{name}/b"], out[f"coef/{name}/a"] = np.asarray([lo, hi], np.float64), b, a
    spectral = calc.SpectralEntropyCalculator(sampling_rate=FS)
    assert np.array_equal(spectral._b, out["coef/default/b"]) and np.array_equal(spectral._a, out["coef/default/a"])
    recs = eeg_recordings(rng)
    out["eeg/names"] = np.asarray(list(recs))
    err32 = err64 = 0.0
    for name, x in recs.items():
        ref = spectral.compute(x)
        assert ref.dtype == np.float64
        out[f"eeg/{name}/raw"], out[f"eeg/{name}/entropy"] = x, ref
        d32 = float(np.abs(ER.spectral_entropy_ref(x, FS) - ref).max())
        d64 = float(np.abs(ER.spectral_entropy_ref(x, FS, round32=False) - ref).max())
        print(f"eeg {name} {x.shape}: entropy {ref.min():.4f} .. {ref.max():.4f}, restatement {d32:.1e} (float64 signal {d64:.1e})")
        err32, err64 = max(err32, d32), max(err64, d64)
    special = out["eeg/special/entropy"]
    assert abs(special[1] - np.log2(129)) < 1e-9 and abs(special[2] - np.log2(129)) < 1e-9, special
    out["restatement_err/spectral"], out["restatement_err/spectral64"] = np.float64(err32), np.float64(err64)
    out["tolerance/spectral"] = np.float64(2 * err32)
    assert 0 < out["tolerance/spectral"] <= SPECTRAL_TOLERANCE_LIMIT, out["tolerance/spectral"]
    spatial = calc.SpatialEntropyCalculator()
    raw_spatial = calc.SpatialEntropyCalculator(normalize_input=False)
    imgs = images(rng)
    out["image/names"] = np.asarray(list(imgs))
    err = 0.0
    for name, im in imgs.items():
        ref, ref_raw = float(spatial.compute(im)), float(raw_spatial.compute(im))
        out[f"image/{name}/pixels"], out[f"image/{name}/entropy"], out[f"image/{name}/entropy_raw"] = im, np.float64(ref), np.float64(ref_raw)
        d = max(abs(ER.spatial_entropy_ref(im) - ref), abs(ER.spatial_entropy_ref(im, normalize=False) - ref_raw))
        print(f"image {name} {im.shape} {im.dtype}: entropy {ref:.6f} (raw {ref_raw:.6f}), restatement {d:.1e}")
        err = max(err, d)
    assert out["image/constant_8x8/entropy"] == 6.0
    out["restatement_err/spatial"] = np.float64(err)
    assert err <= SPATIAL_GATE / 100, err
    out["tolerance/spatial"] = np.float64(SPATIAL_GATE)
    rows = summary_table(rng)
    cols = ["pair_id", "player", "trial_idx", "condition", "spatial_entropy", "mean_entropy"]
    df = pd.DataFrame(rows, columns=cols)
    for c in cols:
        out[f"table/{c}"] = df[c].to_numpy() if df[c].dtype != object else df[c].to_numpy().astype(str)
    for value in ("spatial_entropy", "mean_entropy"):
        s = script.compute_summary_statistics(df, value_col=value)
        assert list(s.columns) == ["pair_id", "player", "condition", "mean", "std", "min", "max", "n_trials"]
        assert int(s["std"].isna().sum()) == 1
        for c in s.columns:
            out[f"summary/{value}/{c}"] = s[c].to_numpy() if s[c].dtype != object else s[c].to_numpy().astype(str)
    # the script's merge (:773-791): gaze rows without the last five trials, EEG rows without the first five
    keys = ["pair_id", "player", "trial_idx", "condition"]
    merged = pd.merge(df[keys + ["spatial_entropy"]].iloc[:-5], df[keys + ["mean_entropy"]].iloc[5:], on=keys, how="inner")
    merged = merged.rename(columns={"spatial_entropy": "gaze_entropy", "mean_entropy": "eeg_entropy"})
    for c in merged.columns:
        out[f"merge/{c}"] = merged[c].to_numpy() if merged[c].dtype != object else merged[c].to_numpy().astype(str)
    return out


if __name__ == "__main__":
    out = build()
    path = REPO / "tests" / "golden" / "entropy.npz"
    np.savez_compressed(path, **out)
    assert path.stat().st_size < FILE_LIMIT, path.stat().st_size
    print(f"{path.name}: {path.stat().st_size / 1e3:.0f} kB")
    for k in sorted(out):
        if k.startswith(("restatement_err", "tolerance/")):
            print(f"  {k} = {float(out[k]):.3e}")
