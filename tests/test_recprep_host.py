"""CPU tests of the recording preprocessing's host side: the scipy-free filter design and the sequential float64
restatement (tests/recprep_ref.py) against the reference's own pipeline (tests/golden/recording_preprocess.npz, written by
tests/make_golden_recording_preprocess.py), and every refusal that happens before a launch.  No GPU."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest

from eyegaze_multimodal_amd import _lib as L
from eyegaze_multimodal_amd import filters
from tests import recprep_ref as R

Z = np.load(Path(__file__).resolve().parent / "golden" / "recording_preprocess.npz")
TAGS = ("s250", "s256")
PAIRS = [tuple(int(v) for v in p) for p in Z["pair_lengths"]]
TOL = dict(atol=5e-6, rtol=0)      # the data path's tolerance (tests/test_gpu_data.py)


def setting(tag):
    lo, hi, fs = (float(v) for v in Z[f"{tag}/setting"])
    return lo, hi, fs


def recordings():
    """(pair, player) of every recording of the fixture, in storage order"""
    return [(p, w) for p in range(len(PAIRS)) for w in range(2)]


def test_fixture_covers_the_stated_lengths():
    flat = [n for p in PAIRS for n in p]
    assert {28, 63, 64, 65, 300, 1000} <= set(flat) and sum(a != b for a, b in PAIRS) >= 2
    assert all(Z[f"raw/{p}/{w}"].shape == (6, PAIRS[p][w]) and Z[f"raw/{p}/{w}"].dtype == np.float32 for p, w in recordings())
    assert max(min(p) for p in PAIRS) >= 128 + 2 * 64                  # three windows of 128 at stride 64
    assert float(np.abs(Z["raw/0/0"]).max()) > 1000.0                  # raw-like: an offset of thousands
    assert 0 < float(Z["filt_restatement_err"]) < 1e-4


@pytest.mark.parametrize("tag", TAGS)
def test_filter_design_matches_the_reference_coefficients(tag):
    lo, hi, fs = setting(tag)
    b, a = filters.butter_bandpass(4, lo, hi, fs)
    assert b.dtype == a.dtype == np.float64 and len(b) == len(a) == 9 and a[0] == 1.0
    np.testing.assert_allclose(b, Z[f"{tag}/b"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(a, Z[f"{tag}/a"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(filters.lfilter_zi(b, a), Z[f"{tag}/zi"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(filters.lfilter_zi(Z[f"{tag}/b"], Z[f"{tag}/a"]), Z[f"{tag}/zi"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("tag", TAGS)
def test_filter_design_matches_scipy_where_it_imports(tag):
    signal = pytest.importorskip("scipy.signal")
    lo, hi, fs = setting(tag)
    for order in (1, 2, 4, 8):
        b, a = filters.butter_bandpass(order, lo, hi, fs)
        bs, as_ = signal.butter(order, [lo / (fs / 2), min(hi / (fs / 2), 0.99)], btype="band")
        np.testing.assert_allclose(b, bs, rtol=1e-13, atol=0)
        np.testing.assert_allclose(a, as_, rtol=1e-13, atol=0)
        np.testing.assert_allclose(filters.lfilter_zi(b, a), signal.lfilter_zi(bs, as_), rtol=1e-13, atol=0)


def test_high_edge_is_clamped_as_the_reference_clamps_it():
    b, a = filters.butter_bandpass(4, 0.5, 200.0, 250.0)              # 200 Hz is beyond Nyquist: min(1.6, 0.99)
    b2, a2 = filters.butter_bandpass(4, 0.5, 0.99 * 125.0, 250.0)
    assert np.array_equal(b, b2) and np.array_equal(a, a2)


@pytest.mark.parametrize("kw", [dict(low_hz=0.0), dict(low_hz=-1.0), dict(low_hz=60.0), dict(low_hz=50.0), dict(order=0), dict(order=9),
                                dict(order=2.5)])
def test_filter_design_refusals(kw):
    args = dict(order=4, low_hz=0.5, high_hz=50.0, fs=250.0)
    args.update(kw)
    with pytest.raises(ValueError):
        filters.butter_bandpass(**args)


@pytest.fixture(scope="module")
def restated():
    """tag -> {(pair, player): (filtered float64, final float32)} by the restatement with the PACKAGE's coefficients, once"""
    out = {}
    for tag in TAGS:
        b, a = filters.butter_bandpass(4, *setting(tag))
        zi = filters.lfilter_zi(b, a)
        out[tag] = {}
        for p, w in recordings():
            f = R.filtfilt_ref(b, a, zi, Z[f"raw/{p}/{w}"])
            out[tag][p, w] = (f, R.car_zscore_ref(f.astype(np.float32)))
    return out


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_final_output_matches_the_reference(restated, tag):
    for p, w in recordings():
        np.testing.assert_allclose(restated[tag][p, w][1], Z[f"{tag}/final/{p}/{w}"], err_msg=f"pair {p} player {w}", **TOL)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_filter_stage_matches_the_reference(restated, tag):
    tol = float(Z["filt_restatement_err"])                              # measured by the generator, held as measured
    for p, w in recordings():
        np.testing.assert_allclose(restated[tag][p, w][0], Z[f"{tag}/filt/{p}/{w}"].astype(np.float64), atol=tol, rtol=0,
                                   err_msg=f"pair {p} player {w}")


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_windows_are_cut_after_alignment(tag):
    for p, (la, lb) in enumerate(PAIRS):
        n = min(la, lb)
        if n < 128:
            assert f"{tag}/windows/{p}" not in Z.files
            continue
        wins = Z[f"{tag}/windows/{p}"]
        assert wins.shape == ((n - 128) // 64 + 1, 2, 6, 128)
        for j in range(wins.shape[0]):
            for w in range(2):
                assert np.array_equal(wins[j, w], Z[f"{tag}/final/{p}/{w}"][:, 64 * j:64 * j + 128])


# ---------------------------------------------------------------------------------------------------------------
# host refusals of the three entry points: nothing below is dereferenced or launched
# ---------------------------------------------------------------------------------------------------------------
FAKE = 0x1000


def dbl(v):
    return (ctypes.c_double * len(v))(*v)


def filt_args(**over):
    d = dict(data=FAKE, row_off=FAKE, row_len=FAKE, ws_off=FAKE, n_rows=72, C=6, max_len=1000, b=[0.1] * 9, a=[1.0] + [0.1] * 8,
             zi=[0.0] * 8, ncoef=9, ws=FAKE, need=5000, cap=5000)
    d.update(over)
    desc = L.RecordingRowsDesc(d["data"], d["row_off"], d["row_len"], d["ws_off"], d["n_rows"], d["C"], d["max_len"], 0)
    arr = lambda v: None if v is None else dbl(v)
    return (ctypes.byref(desc), arr(d["b"]), arr(d["a"]), arr(d["zi"]), d["ncoef"], d["ws"], d["need"], d["cap"], 0)


@pytest.mark.parametrize("over,match", [
    (dict(data=0), "null pointer"), (dict(row_off=0), "null pointer"), (dict(row_len=0), "null pointer"), (dict(ws_off=0), "null pointer"),
    (dict(b=None), "null pointer"), (dict(a=None), "null pointer"), (dict(zi=None), "null pointer"), (dict(ws=0), "null pointer"),
    (dict(n_rows=0), "n_rows=0"), (dict(n_rows=-3), "n_rows=-3"), (dict(C=0), "C=0"), (dict(C=-1), "C=-1"),
    (dict(ncoef=1), "ncoef=1 outside"), (dict(ncoef=18, b=[0.1] * 18, a=[1.0] + [0.1] * 17, zi=[0.0] * 17), "ncoef=18 outside"),
    (dict(a=[2.0] + [0.1] * 8), "must be 1"),
    (dict(cap=4999), "need 5000 workspace doubles, the workspace's capacity is 4999"), (dict(need=0), "workspace"),
])
def test_filtfilt_host_checks(over, match):
    with pytest.raises(L.EgError, match=match):
        L.call("eg_recording_filtfilt", *filt_args(**over))


@pytest.mark.parametrize("over,match", [
    (dict(data=0), "null pointer"), (dict(row_off=0), "null pointer"), (dict(row_len=0), "null pointer"),
    (dict(n_rows=0), "n_rows=0"), (dict(C=0), "C=0"), (dict(n_rows=71), "no multiple of C=6"),
])
def test_car_zscore_host_checks(over, match):
    d = dict(data=FAKE, row_off=FAKE, row_len=FAKE, n_rows=72, C=6)
    d.update(over)
    desc = L.RecordingRowsDesc(d["data"], d["row_off"], d["row_len"], 0, d["n_rows"], d["C"], 1000, 0)
    with pytest.raises(L.EgError, match=match):
        L.call("eg_recording_car_zscore", ctypes.byref(desc), 0)


@pytest.mark.parametrize("over,match", [
    (dict(data=0), "null pointer"), (dict(pair_off=0), "null pointer"), (dict(pair_len=0), "null pointer"),
    (dict(win_pair=0), "null pointer"), (dict(win_start=0), "null pointer"), (dict(order=0), "null pointer"),
    (dict(eeg1=0), "null pointer"), (dict(eeg2=0), "null pointer"),
    (dict(n=0), "bad shape"), (dict(C=0), "bad shape"), (dict(T=-1), "bad shape"), (dict(n_pairs=0), "empty tables"),
    (dict(T=16385), "16384"),
    (dict(first=-1), "outside the order"), (dict(first=7), "outside the order"), (dict(n=11), "outside the order"),
    (dict(win_label=0), "no win_label"),
])
def test_window_cut_host_checks(over, match):
    """eg_window_gather's refusals (tests/test_resident_host.py), without the mode"""
    from tests.test_resident_host import gather_args
    args = gather_args(**over)
    with pytest.raises(L.EgError, match="eg_window_cut: .*" + match):
        L.call("eg_window_cut", *args[:8], args[9])


def test_rows_descriptor_mirrors_the_header():
    import re
    from tests.test_capi_symbols import REPO
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "eyegaze_hip.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct eg_recording_rows_desc \{(.*?)\} eg_recording_rows_desc;", text, flags=re.S).group(1)
    names = [w for w in re.findall(r"\w+", body) if w not in ("const", "float", "int64_t", "int32_t")]
    assert names == [f[0] for f in L.RecordingRowsDesc._fields_]
    assert ctypes.sizeof(L.RecordingRowsDesc) == 4 * 8 + 4 * 4
    for name in ("eg_recording_filtfilt", "eg_recording_car_zscore", "eg_window_cut"):
        m = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m and len(m.group(1).split(",")) == len(L.SIGNATURES[name]), name


# ---------------------------------------------------------------------------------------------------------------
# the wrappers' refusals
# ---------------------------------------------------------------------------------------------------------------
PREP = {"sampling_rate": 250, "filter_low": 0.5, "filter_high": 50.0}


def test_preprocess_recordings_refuses_a_row_not_longer_than_the_padding():
    from eyegaze_multimodal_amd.data import preprocess_recordings
    x = np.zeros((6, 27), np.float32)
    with pytest.raises(ValueError, match="27 samples"):
        preprocess_recordings([np.zeros((6, 100), np.float32), x], device="cpu", **PREP)
    with pytest.raises(ValueError, match="one channel count"):
        preprocess_recordings([np.zeros((6, 100), np.float32), np.zeros((5, 100), np.float32)], device="cpu", **PREP)


@pytest.mark.parametrize("bad", [dict(filter_low=0.0), dict(filter_low=60.0), dict(filter_low=-2.0)])
def test_preprocess_recordings_refuses_a_bad_band(bad):
    from eyegaze_multimodal_amd.data import preprocess_recordings
    with pytest.raises(ValueError, match="butter_bandpass"):
        preprocess_recordings([np.zeros((6, 100), np.float32)], device="cpu", **{**PREP, **bad})


def test_row_tables_and_their_validation():
    from eyegaze_multimodal_amd.data import recording_row_tables, validate_recording_rows
    off, ln, wso, floats, need = recording_row_tables([28, 100], 3, 27)
    assert off.tolist() == [0, 28, 56, 84, 184, 284] and ln.tolist() == [28] * 3 + [100] * 3 and ln.dtype == np.int32
    assert wso.tolist() == [0, 82, 164, 246, 400, 554] and floats == 384 and need == 3 * 82 + 3 * 154
    validate_recording_rows(off, ln, 3, 27, floats)
    with pytest.raises(ValueError, match="covers floats"):
        validate_recording_rows(off, ln, 3, 27, floats - 1)
    bad = off.copy()
    bad[4] -= 1
    with pytest.raises(ValueError, match="overlaps"):
        validate_recording_rows(bad, ln, 3, 27, floats)
    bad = ln.copy()
    bad[5] = 101                                                       # the last row: longer without touching a neighbour
    with pytest.raises(ValueError, match="different lengths"):
        validate_recording_rows(off, bad, 3, 27, floats + 1)
    with pytest.raises(ValueError, match="padding of 28"):
        validate_recording_rows(off, ln, 3, 28, floats)


def test_resident_windows_refuses_to_normalise_a_preprocessed_store_twice(tmp_path):
    from eyegaze_multimodal_amd.data import ResidentWindows, build_recording_store
    from tests.test_data_host import FILES, ITEMS, LABEL2ID, STRIDE, W
    index = build_recording_store(ITEMS, None, LABEL2ID, tmp_path, W, STRIDE, recordings=FILES)
    assert "preprocessed" not in index
    index["preprocessed"] = {**PREP, "order": 4}
    (tmp_path / "index.json").write_text(json.dumps(index))
    with pytest.raises(ValueError, match="a second time"):
        ResidentWindows(tmp_path, 4, "cpu", preprocessing=True)


def test_store_builder_refuses_an_incomplete_mapping(tmp_path):
    from eyegaze_multimodal_amd.data import build_recording_store
    from tests.test_data_host import FILES, ITEMS, LABEL2ID, STRIDE, W
    with pytest.raises(ValueError, match="filter_high"):
        build_recording_store(ITEMS, None, LABEL2ID, tmp_path, W, STRIDE, recordings=FILES,
                              recording_preprocessing={"sampling_rate": 250, "filter_low": 0.5})


def test_train_config_needs_resident_for_recording_preprocessing():
    from eyegaze_multimodal_amd import train_art as TA
    data = {"recording_preprocessing": True, "sampling_rate": 256, "filter_low": 1.0, "filter_high": 45.0}
    cfg = {"data": dict(data), "training": {"output_dir": "run", "per_device_train_batch_size": 4, "per_device_eval_batch_size": 4}}
    with pytest.raises(ValueError, match="needs data.resident"):
        TA.recording_preprocessing_of(cfg)
    cfg["data"]["random_seed"] = 0
    with pytest.raises(ValueError, match="needs data.resident"):
        TA.window_loaders(cfg, "cpu", 0, 1)
    cfg["data"]["resident"] = True
    assert TA.recording_preprocessing_of(cfg) == {"sampling_rate": 256.0, "filter_low": 1.0, "filter_high": 45.0}
    assert TA.store_dir(cfg).name == "recording_store_preprocessed"
    cfg["data"]["recording_preprocessing"] = False
    assert TA.recording_preprocessing_of(cfg) is None and TA.store_dir(cfg).name == "recording_store"
    del cfg["data"]["filter_high"]
    cfg["data"]["recording_preprocessing"] = True
    with pytest.raises(ValueError, match="filter_high"):
        TA.recording_preprocessing_of(cfg)


def test_predict_recording_refuses_a_mapping_with_a_missing_key():
    from eyegaze_multimodal_amd.predict import predict_recording
    rec = np.zeros((8, 2048), np.float32)
    with pytest.raises(ValueError, match="sampling_rate"):
        predict_recording(None, rec, rec, recording_preprocessing={"filter_low": 1.0, "filter_high": 45.0})
    with pytest.raises(ValueError, match="twice"):
        predict_recording(None, rec, rec, preprocessing=True, recording_preprocessing=PREP)
