"""
TEST INFRASTRUCTURE -- the fixture of the trial features, written by the reference's own extractor:
2_Preprocessing/scripts/extract_eeg_features.py, loaded by path and imported unchanged, so this runs only where the reference
tree (oracle.make_golden.REF), scipy, pandas, tqdm and joblib exist.  No reference source is copied.  Each trial goes through the
body of process_trial (:794-835) function by function -- process_trial itself reads CSV files and refuses trials below 500 samples.

Raw-like pairs (a per-channel offset of thousands, a random walk, a component both players share so that the inter-brain values
are not all near zero, tones at 6, 10 and 20 Hz with per-channel phases, noise) at lengths chosen for a reason:
  256          the minimum: one coherence segment, one Welch segment
  257 | 300    odd (the other Hilbert weight branch); the alignment cuts the partner
  500          the script's own minimum at 250 Hz
  777          3 * 7 * 37: odd with a large prime factor
  1000
all at C = 6 (masked edges of the pair tiles), and 3250 = 2 * 5^3 * 13, the reference's trial length, at C = 3 for the file size (at C = 2 the common-average reference leaves two rows that are each other's negative).

Stored: the raw inputs, every output (time_domain only for the two shortest trials), the band coefficients, per PLI entry the
number of samples with |Im P| < 1e-4 in the float64 restatement (`near`), and per output the largest distance of both variants
of tests/trialfeat_ref from the reference (`restatement_err64/<name>`, `restatement_err32/<name>`); `tolerance/<name>` is twice
the larger of the two.

Usage:  python tests/make_golden_trial_features.py
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from oracle.make_golden import REF  # noqa: E402
from tests import trialfeat_ref as T  # noqa: E402

FS = 250
TRIALS = [(6, 256, 256), (6, 257, 300), (6, 500, 500), (6, 777, 777), (6, 1000, 1000), (3, 3250, 3250)]      # (C, L1, L2)
STORE_TIME = (0, 1)
COEF_BANDS = {"delta": (0.5, 4), "theta": (4, 7), "alpha": (8, 12), "beta": (12, 28), "gamma": (28, 50), "pre": (0.5, 50.0),
              "clamped": (0.1, 4)}                                    # 0.1 / 125 < 0.001: the script's lower clamp
FILE_LIMIT = 400_000
TOLERANCE_LIMIT = 1e-3               # values live in [-1, 1]: anything looser hides a wrong bin or band
NEAR_LIMIT = 0.02                    # 2 near / L: the PLI rule must not be able to hide a wrong PLI


def raw_pair(rng, C, L1, L2):
    n = max(L1, L2)
    t = np.arange(n) / FS
    shared = np.cumsum(rng.normal(0.0, 1.5, n)) + 12.0 * np.sin(2 * np.pi * 10.0 * t + rng.uniform(0, 2 * np.pi)) + rng.normal(0.0, 6.0, n)
    out = []
    for L in (L1, L2):
        x = rng.uniform(-4000.0, 4000.0, (C, 1)) + np.cumsum(rng.normal(0.0, 2.0, (C, n)), axis=1) + rng.normal(0.0, 5.0, (C, n))
        for f, amp in ((6.0, 15.0), (10.0, 20.0), (20.0, 10.0)):
            x = x + amp * rng.uniform(0.5, 1.0, (C, 1)) * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi, (C, 1)))
        x = x + rng.uniform(0.4, 1.0, (C, 1)) * shared
        out.append(x[:, :L].astype(np.float32))
    return out


def load_extractor():
    path = REF / "2_Preprocessing" / "scripts" / "extract_eeg_features.py"
    spec = importlib.util.spec_from_file_location("ref_extract_eeg_features", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.SCIPY_AVAILABLE
    return mod


def reference_features(P, eeg1, eeg2):
    """process_trial :794-835"""
    n = min(eeg1.shape[1], eeg2.shape[1])
    p1, p2 = P.preprocess_eeg(eeg1[:, :n], FS), P.preprocess_eeg(eeg2[:, :n], FS)
    freqs, psd1 = P.compute_psd(p1, FS)
    _, psd2 = P.compute_psd(p2, FS)
    bands = P.FREQUENCY_BANDS
    f = {"time_domain": np.stack([p1, p2]), "freq_domain": np.stack([psd1, psd2]), "freq_bins": freqs,
         "bands_energy": np.stack([P.compute_band_energy(psd1, freqs, bands), P.compute_band_energy(psd2, freqs, bands)]),
         "intra_con": np.stack([P.compute_intra_connectivity(p1, bands, FS), P.compute_intra_connectivity(p2, bands, FS)]),
         "inter_con": P.compute_inter_connectivity(p1, p2, bands, FS)}
    assert all(v.dtype == np.float32 for v in f.values())
    return f


def build(seed):
    """the fixture's dict, or None when this seed breaks one of the generator's own conditions"""
    from scipy import signal
    from eyegaze_multimodal_amd import features as F
    P = load_extractor()
    assert list(P.FREQUENCY_BANDS.items()) == list(F.FREQUENCY_BANDS.items()) and P.METRIC_NAMES == F.METRIC_NAMES
    rng = np.random.default_rng(seed)
    out = {"trials": np.asarray(TRIALS, np.int64), "sampling_rate": np.int64(FS), "near_delta": np.float64(T.NEAR_DELTA)}
    for name, (lo, hi) in COEF_BANDS.items():
        b, a = signal.butter(4, [max(lo / (FS / 2), 0.001), min(hi / (FS / 2), 0.99)], btype="band")     # bandpass_filter :170-175
        out[f"coef/{name}/band"], out[f"coef/{name}/b"], out[f"coef/{name}/a"] = np.asarray([lo, hi], np.float64), b, a
    err = {64: {}, 32: {}}
    pli = []
    for t, (C, L1, L2) in enumerate(TRIALS):
        raw = raw_pair(rng, C, L1, L2)
        ref = reference_features(P, *raw)
        L = min(L1, L2)
        out[f"raw/{t}/0"], out[f"raw/{t}/1"] = raw
        for k, v in ref.items():
            if k != "time_domain" or t in STORE_TIME:
                out[f"ref/{t}/{k}"] = v
        cache = {}
        r64 = T.trial_features_ref(*raw, fs=FS, cache=cache)
        r32 = T.trial_features_ref(*raw, fs=FS, sums32=True, cache=cache)
        near = r64["near"].copy()
        d = np.arange(C)
        near[:2, :, d, d] = 0                                          # intra diagonals are exact, not counted
        out[f"near/{t}"] = near.astype(np.int32)
        if 2.0 * near.max() / L > NEAR_LIMIT:
            print(f"seed {seed}: trial {t} has an entry with {near.max()} near samples of {L}")
            return None
        for bits, r in ((64, r64), (32, r32)):
            for name, v in T.distances(r, ref).items():
                err[bits][name] = max(err[bits].get(name, 0.0), v)
            assert T.intra_diagonals_exact(r)
        pli.append((r64, ref, near, L))
        print(f"trial {t} (C={C}, L={L}): " + ", ".join(f"{k} {v:.1e}" for k, v in T.distances(r64, ref).items()))
    for bits in (64, 32):
        for name, v in err[bits].items():
            out[f"restatement_err{bits}/{name}"] = np.float64(v)
    for name in err[64]:
        tol = 2.0 * max(err[64][name], err[32][name])
        out[f"tolerance/{name}"] = np.float64(tol)
        if name != "time_domain" and tol >= TOLERANCE_LIMIT:
            print(f"seed {seed}: tolerance/{name} = {tol:.3e}")
            return None
    slack = max(float(out[f"tolerance/{n}"]) for n in ("pearson", "power_corr", "plv", "wpli"))
    out["tolerance/pli_slack"] = np.float64(slack)
    for r64, ref, near, L in pli:                                       # the reference itself meets the PLI rule
        if T.pli_excess(ref, r64, near, slack, L) > 0:
            print(f"seed {seed}: the reference's PLI is outside the rule")
            return None
    return out


if __name__ == "__main__":
    for seed in range(20240901, 20240911):
        out = build(seed)
        if out is not None:
            break
    else:
        raise SystemExit("no seed met the generator's conditions")
    out["seed"] = np.int64(seed)
    path = REPO / "tests" / "golden" / "trial_features.npz"
    np.savez_compressed(path, **out)
    assert path.stat().st_size <= FILE_LIMIT, path.stat().st_size
    print(f"{path.name}: {path.stat().st_size / 1e3:.0f} kB, seed {seed}")
    for k in sorted(out):
        if k.startswith(("restatement_err", "tolerance/")):
            print(f"  {k} = {float(out[k]):.3e}")
