"""
TEST INFRASTRUCTURE -- the fixture of the recording preprocessing, written by the reference's own pipeline:
2_Preprocessing/scripts/preprocess_eeg_windows.py, loaded by path and imported unchanged, so this runs only where the reference
tree (oracle.make_golden.REF), scipy, pandas and tqdm exist.  No reference source is copied.

Six pairs of C = 6 raw-like recordings (a per-channel offset of thousands, a random walk, 10 Hz and 50 Hz tones, noise) whose
per-player lengths sit at the edges of the kernels: 28 (the shortest scipy accepts at 9 coefficients), 63 / 64 / 65 (a time
tile), 257 / 299 / 300 and 1000; four pairs hold two lengths.  Both filter settings -- (0.5, 50, 250), the script's default, and
(1, 45, 256), the YAML's -- store the reference's b, a, scipy's lfilter_zi, bandpass_filter's and preprocess_eeg's outputs per
recording and the windows extract_windows gives after the pair's alignment; `filt_restatement_err` is the largest
|tests/recprep_ref.filtfilt_ref - bandpass_filter| this generator measured.

Usage:  python tests/make_golden_recording_preprocess.py
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from oracle.make_golden import REF  # noqa: E402
from tests import recprep_ref as R  # noqa: E402

C = 6
PAIR_LENGTHS = [(28, 29), (63, 63), (64, 65), (65, 64), (300, 257), (1000, 299)]
SETTINGS = {"s250": (0.5, 50.0, 250), "s256": (1.0, 45.0, 256)}          # (filter_low, filter_high, sampling_rate)
WINDOW, STRIDE = 128, 64
FILE_LIMIT = 400_000


def raw_like(rng, L, fs=250.0):
    t = np.arange(L) / fs
    off = rng.uniform(-4000.0, 4000.0, size=(C, 1))
    walk = np.cumsum(rng.normal(0.0, 2.0, size=(C, L)), axis=1)
    tones = 20.0 * np.sin(2 * np.pi * 10.0 * t + rng.uniform(0, 2 * np.pi, (C, 1))) + \
        15.0 * np.sin(2 * np.pi * 50.0 * t + rng.uniform(0, 2 * np.pi, (C, 1)))
    return (off + walk + tones + rng.normal(0.0, 5.0, size=(C, L))).astype(np.float32)


def load_pipeline():
    path = REF / "2_Preprocessing" / "scripts" / "preprocess_eeg_windows.py"
    spec = importlib.util.spec_from_file_location("ref_preprocess_eeg_windows", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.SCIPY_AVAILABLE
    return mod


if __name__ == "__main__":
    from scipy import signal
    P = load_pipeline()
    rng = np.random.default_rng(20240611)
    out = {"pair_lengths": np.asarray(PAIR_LENGTHS, np.int64), "window": np.int64(WINDOW), "stride": np.int64(STRIDE)}
    recs = [[raw_like(rng, L) for L in pair] for pair in PAIR_LENGTHS]
    for p, pair in enumerate(recs):
        for w, x in enumerate(pair):
            out[f"raw/{p}/{w}"] = x
    for tag, (lo, hi, fs) in SETTINGS.items():
        b, a = signal.butter(4, [lo / (fs / 2), min(hi / (fs / 2), 0.99)], btype="band")     # bandpass_filter's own call (:119-124)
        zi = signal.lfilter_zi(b, a)
        out[f"{tag}/setting"] = np.asarray([lo, hi, fs], np.float64)
        out[f"{tag}/b"], out[f"{tag}/a"], out[f"{tag}/zi"] = b, a, zi
        err = 0.0
        for p, pair in enumerate(recs):
            done = []
            for w, x in enumerate(pair):
                filt = P.bandpass_filter(x.copy(), lo, hi, fs)
                full = P.preprocess_eeg(x.copy(), sampling_rate=fs, low_freq=lo, high_freq=hi)
                assert filt.dtype == np.float32 and full.dtype == np.float32 and filt.shape == x.shape
                assert not np.array_equal(filt, x), "bandpass_filter swallowed an exception and returned its input"
                err = max(err, float(np.abs(R.filtfilt_ref(b, a, zi, x) - filt.astype(np.float64)).max()))
                out[f"{tag}/filt/{p}/{w}"], out[f"{tag}/final/{p}/{w}"] = filt, full
                done.append(full)
            n = min(d.shape[1] for d in done)                                               # process_single_sample :252-259
            wins = [P.extract_windows(d[:, :n], WINDOW, STRIDE) for d in done]
            assert len(wins[0]) == len(wins[1])
            if wins[0]:
                out[f"{tag}/windows/{p}"] = np.stack([np.stack(wins[0]), np.stack(wins[1])], axis=1)     # [nwin, 2, C, W]
        out[f"{tag}/filt_restatement_err"] = np.float64(err)
        print(f"{tag}: filt_restatement_err = {err:.3e}, |filt| up to "
              f"{max(float(np.abs(v).max()) for k, v in out.items() if k.startswith(tag + '/filt/')):.1f}")
    out["filt_restatement_err"] = np.float64(max(out[f"{t}/filt_restatement_err"] for t in SETTINGS))
    path = REPO / "tests" / "golden" / "recording_preprocess.npz"
    np.savez_compressed(path, **out)
    assert path.stat().st_size <= FILE_LIMIT, path.stat().st_size
    print(f"{path.name}: {path.stat().st_size / 1e3:.0f} kB, filt_restatement_err = {float(out['filt_restatement_err']):.3e}")
