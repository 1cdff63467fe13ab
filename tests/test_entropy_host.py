"""CPU tests of the entropy analysis: the numpy restatement against the reference's own outputs
(tests/golden/entropy.npz), the calculator's coefficients, the layout rule, the file name patterns, summaries, merge and CSV writers,
and the host-side refusals of both entry points and of both calls."""
import csv
import ctypes
import math
from pathlib import Path

import numpy as np
import pytest

from eyegaze_multimodal_amd import entropy as E
from eyegaze_multimodal_amd import features as F
from eyegaze_multimodal_amd.filters import butter_bandpass
from tests import entropy_ref as ER
from tests.entropy_fixture import (EEG_NAMES, FS, IMAGE_NAMES, TOL_SPATIAL, TOL_SPECTRAL, Z, filtered, image, image_entropy, raw,
                                   reference_entropy, table_rows)

GOLDEN = Path(__file__).resolve().parent / "golden"


# ---------------------------------------------------------------------------------------------------------------
# restatement and fixture
# ---------------------------------------------------------------------------------------------------------------
def test_restatement_meets_the_reference_within_the_stored_distances():
    worst = 0.0
    for name in EEG_NAMES:
        d = float(np.abs(ER.spectral_entropy_of_rows(filtered(name), FS) - reference_entropy(name)).max())
        worst = max(worst, d)
        assert d <= float(Z["restatement_err/spectral"]) * (1 + 1e-6) + 1e-13, (name, d)
    print(f"spectral restatement: {worst:.2e} (stored {float(Z['restatement_err/spectral']):.2e})")
    for name in IMAGE_NAMES:
        for normalize in (True, False):
            d = abs(ER.spatial_entropy_ref(image(name), normalize) - image_entropy(name, normalize))
            assert d <= max(float(Z["restatement_err/spatial"]), 1e-14), (name, normalize, d)


def test_generator_assertions_hold_on_load():
    assert (GOLDEN / "entropy.npz").stat().st_size < 400_000
    assert 0 < TOL_SPECTRAL <= 1e-6 and TOL_SPECTRAL == 2 * float(Z["restatement_err/spectral"])
    assert float(Z["restatement_err/spectral64"]) < 1e-12                # the whole distance is the one rounding to float32
    assert TOL_SPATIAL == 1e-10 and float(Z["restatement_err/spatial"]) <= 1e-12
    special = reference_entropy("special")
    assert abs(special[1] - math.log2(129)) < 1e-9 and abs(special[2] - math.log2(129)) < 1e-9       # all-zero and constant rows
    assert special[0] < 2.0                                                                          # the 10 Hz sine: concentrated
    assert image_entropy("constant_8x8") == 6.0
    assert [tuple(raw(n).shape) for n in EEG_NAMES[:6]] == [(2, 256), (2, 257), (2, 383), (2, 384), (2, 777), (3, 3250)]
    assert all(raw(n).dtype == np.float32 and reference_entropy(n).dtype == np.float64 for n in EEG_NAMES)
    assert image("f64_50x60x3").dtype == np.float64 and all(image(n).dtype == np.uint8 for n in IMAGE_NAMES if not n.startswith("f64"))
    assert int(np.isnan(Z["summary/spatial_entropy/std"]).sum()) == 1
    # the fixture holds numbers and names only
    assert all(Z[k].dtype.kind in "fiuU" for k in Z.files)


def test_wrong_variants_are_outside_the_tolerance():
    """what the tolerance must not hide: eps left out and a wrong fs show on the scaled rows; a symmetric window on the raw ones"""
    rows = filtered("scaled_1e-6")
    ref = reference_entropy("scaled_1e-6")
    assert np.abs(ER.spectral_entropy_of_rows(rows, FS, eps=0.0) - ref).max() > 1.0
    assert np.abs(ER.spectral_entropy_of_rows(rows, 256.0) - ref).max() > 100 * TOL_SPECTRAL
    rows = filtered("len777").astype(np.float64)
    n = np.arange(256)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * n / 255)                                                      # symmetric Hann
    seg = np.stack([rows[:, 128 * s:128 * s + 256] for s in range((777 - 256) // 128 + 1)], axis=1)
    p = np.abs(np.fft.rfft((seg - seg.mean(axis=2, keepdims=True)) * w, axis=2)) ** 2 / (FS * (w ** 2).sum())
    p[:, :, 1:-1] *= 2
    assert np.abs(ER.shannon_bits(p.mean(axis=1)) - reference_entropy("len777")).max() > 1e-3


# ---------------------------------------------------------------------------------------------------------------
# coefficients
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "upper", "lower"])
def test_coefficients_are_scipys_bit_for_bit(name):
    lo, hi = Z[f"coef/{name}/band"]
    b, a = E.entropy_band_coefficients(float(lo), float(hi), FS)
    assert np.array_equal(b, Z[f"coef/{name}/b"]) and np.array_equal(a, Z[f"coef/{name}/a"])


def test_the_upper_band_tells_the_two_clamps_apart():
    lo, hi = (float(v) for v in Z["coef/upper/band"])
    assert 0.99 < hi / (FS / 2) < 0.999
    assert not np.array_equal(butter_bandpass(4, lo, hi, FS)[1], Z["coef/upper/a"])                  # the default clamps at 0.99


def test_butter_bandpass_default_is_unchanged():
    T = np.load(GOLDEN / "trial_features.npz")
    names = sorted({k.split("/")[1] for k in T.files if k.startswith("coef/")})
    assert len(names) >= 6
    for name in names:
        lo, hi = T[f"coef/{name}/band"]
        b, a = F.band_coefficients(float(lo), float(hi), int(T["sampling_rate"]))
        assert np.array_equal(b, T[f"coef/{name}/b"]) and np.array_equal(a, T[f"coef/{name}/a"]), name
    b0, a0 = butter_bandpass(4, 0.5, 50.0, 250.0)
    b1, a1 = butter_bandpass(4, 0.5, 50.0, 250.0, high_clamp=0.99)
    assert np.array_equal(b0, b1) and np.array_equal(a0, a1)


# ---------------------------------------------------------------------------------------------------------------
# layout rule
# ---------------------------------------------------------------------------------------------------------------
def test_layout_follows_the_reference_rule_in_its_order():
    assert E.image_layout((64, 64)) == E.GREY
    assert E.image_layout((3, 40, 24)) == E.PLANAR
    assert E.image_layout((3, 5, 3)) == E.PLANAR                          # shape[0] == 3 is asked first: the reference transposes it
    assert E.image_layout((3, 3, 3)) == E.PLANAR
    assert E.image_layout((37, 53, 3)) == E.INTERLEAVED
    with pytest.raises(ValueError, match="Expected 3 channels, got 4"):   # an RGBA image
        E.image_layout((20, 30, 4))
    with pytest.raises(ValueError, match="Expected 2D or 3D array, got 4D"):
        E.image_layout((2, 20, 30, 3))
    # and the (3, 5, 3) array's entropy is the transposed one's: the fixture's value
    assert abs(ER.spatial_entropy_ref(image("planar_3x5x3")) - image_entropy("planar_3x5x3")) < 1e-13


def test_spatial_entropy_refuses_what_it_does_not_serve():
    with pytest.raises(ValueError, match="Expected 3 channels, got 4"):
        E.spatial_entropy([np.zeros((8, 8, 4), np.uint8)], device="cpu")
    with pytest.raises(ValueError, match="float32 images are not served.*pairwise"):
        E.spatial_entropy([np.zeros((8, 8), np.float32)], device="cpu")
    with pytest.raises(ValueError, match="share one dtype"):
        E.spatial_entropy([np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.float64)], device="cpu")
    with pytest.raises(ValueError, match="share one dtype"):
        E.spatial_entropy([np.zeros((8, 8), np.uint16)], device="cpu")
    with pytest.raises(ValueError, match="0 pixels"):
        E.spatial_entropy([np.zeros((0, 8), np.uint8)], device="cpu")


# ---------------------------------------------------------------------------------------------------------------
# file names
# ---------------------------------------------------------------------------------------------------------------
def test_file_name_patterns():
    assert E.parse_eeg_filename("Pair-12-A-Single-EYE_trial03_player.csv") == {"pair_id": 12, "condition": "Single", "trial_idx": 3,
                                                                               "player": "A_player"}
    assert E.parse_eeg_filename("Pair-12-B-Single-EYE_trial40_observer.csv")["player"] == "B_observer"
    assert E.parse_eeg_filename("Pair-7-Comp-EYE_trial2_playerB.csv") == {"pair_id": 7, "condition": "Competition", "trial_idx": 2,
                                                                          "player": "playerB"}
    assert E.parse_eeg_filename("Pair-33-Coop-EYE_trial19_playerA.csv") == {"pair_id": 33, "condition": "Cooperation", "trial_idx": 19,
                                                                            "player": "playerA"}
    assert E.parse_gaze_filename("Pair-7-Comp-EYE_trial2_playerB.jpg") == E.parse_eeg_filename("Pair-7-Comp-EYE_trial2_playerB.csv")
    assert E.parse_gaze_filename("Pair-12-A-Single-EYE_trial03_player.png")["condition"] == "Single"
    for bad in ("Pair-12-C-Single-EYE_trial03_player.csv", "Pair-12-A-Single-EYE_trial03_playerA.csv", "Pair-x-Comp-EYE_trial2_playerB.csv",
                "Pair-7-Comp-EYE_trial2_playerC.csv", "Pair-7-Comp-EYE_trial_playerB.csv", "pair-7-Comp-EYE_trial2_playerB.csv",
                "Pair-7-Coop-EEG_trial2_playerB.csv", "Pair-7-Coop-EYE_trial2_playerB.txt", "xPair-7-Coop-EYE_trial2_playerB.csv"):
        assert E.parse_eeg_filename(bad) is None, bad
    assert E.parse_gaze_filename("Pair-7-Comp-EYE_trial2_playerB.bmp") is None


def test_scans_are_sorted_by_name_and_keep_matching_files_only(tmp_path):
    names = ["Pair-9-Coop-EYE_trial2_playerB", "Pair-10-Comp-EYE_trial1_playerA", "Pair-10-A-Single-EYE_trial1_player", "notes"]
    for n in names:
        (tmp_path / f"{n}.csv").write_text("0\n")
        (tmp_path / f"{n}.png").write_bytes(b"")
    (tmp_path / "Pair-9-Coop-EYE_trial3_playerB.jpg").write_bytes(b"")
    eeg = E.scan_eeg_files(tmp_path)
    assert [f["filename"] for f in eeg] == sorted(f"{n}.csv" for n in names[:3])
    assert all(Path(f["filepath"]).exists() for f in eeg)
    gaze = E.scan_gaze_files(tmp_path)
    assert [f["filename"] for f in gaze] == sorted([f"{n}.png" for n in names[:3]] + ["Pair-9-Coop-EYE_trial3_playerB.jpg"])
    with pytest.raises(FileNotFoundError, match="EEG directory not found"):
        E.scan_eeg_files(tmp_path / "nowhere")


# ---------------------------------------------------------------------------------------------------------------
# summaries, merge, CSV writers
# ---------------------------------------------------------------------------------------------------------------
SUMMARY = ["pair_id", "player", "condition", "mean", "std", "min", "max", "n_trials"]


@pytest.mark.parametrize("value", ["spatial_entropy", "mean_entropy"])
def test_summary_statistics_match_the_reference(value):
    got = E.summary_statistics(table_rows(), value)
    ref = table_rows(f"summary/{value}", SUMMARY)
    assert len(got) == len(ref) == 18
    assert [list(g) for g in got] == [SUMMARY] * len(got)
    for g, r in zip(got, ref):
        assert (g["pair_id"], g["player"], g["condition"], g["n_trials"]) == (r["pair_id"], r["player"], r["condition"], r["n_trials"])
        assert g["min"] == r["min"] and g["max"] == r["max"]
        assert abs(g["mean"] - r["mean"]) <= 4 * np.spacing(abs(r["mean"]))
        if r["n_trials"] == 1:
            assert math.isnan(g["std"]) and math.isnan(r["std"])
        else:
            assert abs(g["std"] - r["std"]) <= 1e-13, (g, r)
    keys = [(g["pair_id"], g["player"], g["condition"]) for g in got]
    assert keys == sorted(keys)


def test_cross_modality_is_the_scripts_inner_merge():
    rows = table_rows()
    got = E.cross_modality(rows[:-5], rows[5:])
    cols = ["pair_id", "player", "trial_idx", "condition", "gaze_entropy", "eeg_entropy"]
    ref = table_rows("merge", cols)
    assert len(ref) == len(rows) - 10
    assert [list(g) for g in got] == [cols] * len(got)
    assert got == ref


def read_csv(path):
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    return rows[0], rows[1:]


def test_csv_writers_produce_the_scripts_files(tmp_path):
    rows = table_rows()
    gaze = [{k: r[k] for k in (*E.MERGE_KEYS, "spatial_entropy")} for r in rows[:-5]]
    eeg = []
    for r in rows[5:]:
        channels = np.linspace(r["mean_entropy"] - 0.1, r["mean_entropy"] + 0.1, 32)
        eeg.append({**{k: r[k] for k in E.MERGE_KEYS}, "mean_entropy": r["mean_entropy"], **dict(zip(E.STANDARD_32_CHANNELS, map(float, channels)))})
    written = E.write_results(tmp_path / "out", gaze, eeg)
    assert written == ["gaze_entropy_raw.csv", "gaze_entropy_summary.csv", "eeg_entropy_raw_corrected.csv", "eeg_entropy_summary.csv",
                       "cross_modality_entropy.csv"]
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(written)
    head, body = read_csv(tmp_path / "out" / "gaze_entropy_raw.csv")
    assert head == ["pair_id", "player", "trial_idx", "condition", "spatial_entropy"] and len(body) == len(gaze)
    assert [float(b[4]) for b in body] == [g["spatial_entropy"] for g in gaze]                       # shortest round-trip floats
    head, body = read_csv(tmp_path / "out" / "eeg_entropy_raw_corrected.csv")
    assert head == ["pair_id", "player", "trial_idx", "condition", "mean_entropy", *E.STANDARD_32_CHANNELS] and len(body) == len(eeg)
    assert E.STANDARD_32_CHANNELS[:3] == ["Fp1", "Fz", "F3"] and E.STANDARD_32_CHANNELS[-1] == "Fp2" and len(E.STANDARD_32_CHANNELS) == 32
    for name, value in (("gaze_entropy_summary.csv", "spatial_entropy"), ("eeg_entropy_summary.csv", "mean_entropy")):
        head, body = read_csv(tmp_path / "out" / name)
        assert head == SUMMARY
        want = E.summary_statistics(gaze if value == "spatial_entropy" else eeg, value)
        assert len(body) == len(want)
        for b, w in zip(body, want):
            assert b[:3] == [str(w["pair_id"]), w["player"], w["condition"]] and int(b[7]) == w["n_trials"]
            assert b[4] == ("" if math.isnan(w["std"]) else repr(w["std"]))                          # NaN is an empty cell, as pandas writes it
    assert any(b[4] == "" for b in read_csv(tmp_path / "out" / "gaze_entropy_summary.csv")[1])
    head, body = read_csv(tmp_path / "out" / "cross_modality_entropy.csv")
    assert head == ["pair_id", "player", "trial_idx", "condition", "gaze_entropy", "eeg_entropy"] and len(body) == len(rows) - 10
    # one modality alone writes its two files and no merge
    assert E.write_results(tmp_path / "gaze_only", gaze, None) == ["gaze_entropy_raw.csv", "gaze_entropy_summary.csv"]
    assert E.write_results(tmp_path / "none", [], []) == []


# ---------------------------------------------------------------------------------------------------------------
# refusals, reached without a GPU: every check runs before any launch
# ---------------------------------------------------------------------------------------------------------------
FAKE = 0x1000          # never dereferenced


def rows_desc(L, n_rows=4, C=2, max_len=1000, data=FAKE):
    return L.RecordingRowsDesc(data, FAKE, FAKE, FAKE, n_rows, C, max_len, 0)


def test_spectral_entropy_entry_point_refuses_on_the_host():
    from eyegaze_multimodal_amd import _lib as L
    call = lambda d, fs=250.0, eps=1e-10, psd=0, out=FAKE: L.call("eg_trial_spectral_entropy", ctypes.byref(d), fs, eps, psd, out, 0)
    with pytest.raises(L.EgError, match="null pointer"):
        call(rows_desc(L, data=0))
    with pytest.raises(L.EgError, match="null pointer"):
        call(rows_desc(L), out=0)
    with pytest.raises(L.EgError, match="n_rows=0 must be > 0"):
        call(rows_desc(L, n_rows=0))
    with pytest.raises(L.EgError, match="C=0 must be > 0"):
        call(rows_desc(L, C=0))
    with pytest.raises(L.EgError, match="n_rows=5 is no multiple of C=2"):
        call(rows_desc(L, n_rows=5))
    for bad in (255, 65537):
        with pytest.raises(L.EgError, match=f"max_len={bad} outside"):
            call(rows_desc(L, max_len=bad))
    with pytest.raises(L.EgError, match="fs=0 must be > 0"):
        call(rows_desc(L), fs=0.0)
    with pytest.raises(L.EgError, match="eps=-1e-10 must be >= 0"):
        call(rows_desc(L), eps=-1e-10)
    # eg_trial_welch still insists on pairs of players; the entropy entry point does not
    with pytest.raises(L.EgError, match="no multiple of 2 C"):
        L.call("eg_trial_welch", ctypes.byref(rows_desc(L, n_rows=3, C=1)), 250.0, None, None, 0, FAKE, FAKE, 0, 0)


def image_desc(L, n_images=2, max_pix=100, elem=0, data=FAKE, off=FAKE):
    return L.ImageBatchDesc(data, off, FAKE, FAKE, n_images, max_pix, elem, 1)


def test_image_entropy_entry_point_refuses_on_the_host():
    from eyegaze_multimodal_amd import _lib as L
    call = lambda d, eps=1e-10, ws=FAKE, cap=1 << 40, out=FAKE: L.call("eg_image_entropy", ctypes.byref(d), eps, ws, cap, out, 0)
    for kw in ({"data": 0}, {"off": 0}):
        with pytest.raises(L.EgError, match="null pointer"):
            call(image_desc(L, **kw))
    with pytest.raises(L.EgError, match="null pointer"):
        call(image_desc(L), ws=0)
    with pytest.raises(L.EgError, match="null pointer"):
        call(image_desc(L), out=0)
    with pytest.raises(L.EgError, match="n_images=0 must be > 0"):
        call(image_desc(L, n_images=0))
    for bad in (0, (1 << 24) + 1):
        with pytest.raises(L.EgError, match=f"max_pix={bad} outside"):
            call(image_desc(L, max_pix=bad))
    with pytest.raises(L.EgError, match="elem=2 is neither"):
        call(image_desc(L, elem=2))
    with pytest.raises(L.EgError, match="eps=-1 must be >= 0"):
        call(image_desc(L), eps=-1.0)
    chunk = L.IMAGE_ENTROPY_CHUNK
    assert chunk == 8192
    assert L.image_entropy_workspace_doubles(3, chunk) == 12 and L.image_entropy_workspace_doubles(3, chunk + 1) == 24
    assert L.image_entropy_workspace_doubles(1, 1 << 24) == 4 * 2048
    assert L.image_entropy_workspace_doubles(0, 10) == -1 and L.image_entropy_workspace_doubles(1, 0) == -1
    assert L.image_entropy_workspace_doubles(1, (1 << 24) + 1) == -1
    with pytest.raises(L.EgError, match="need 24 workspace doubles, the workspace's capacity is 23"):
        call(image_desc(L, n_images=3, max_pix=chunk + 1), cap=23)


def test_spectral_entropy_refuses_lengths_and_settings_it_does_not_serve():
    for n in (128, 255, 65537):
        with pytest.raises(ValueError, match=f"{n} samples, served are 256 to 65536"):
            E.spectral_entropy([np.zeros((2, 300), np.float32), np.zeros((2, n), np.float32)], device="cpu")
    with pytest.raises(ValueError, match="needs \\(C, L\\) recordings"):
        E.spectral_entropy([np.zeros(300, np.float32)], device="cpu")
    with pytest.raises(ValueError, match="nperseg = 128"):
        E.spectral_entropy([np.zeros((2, 300), np.float32)], nperseg=128, device="cpu")
    with pytest.raises(ValueError, match="more than 17"):
        E.spectral_entropy([np.zeros((2, 300), np.float32)], filter_order=9, device="cpu")
    assert E.spectral_entropy([], device="cpu") == []
