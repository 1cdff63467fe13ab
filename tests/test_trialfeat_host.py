"""CPU-only tests of the trial features: the numpy restatement against the reference's outputs
(tests/golden/trial_features.npz, written by tests/make_golden_trial_features.py), the band coefficients with the script's lower
clamp, and the host-side refusals of the new entry points and of extract_trial_features."""
import ctypes
import numpy as np
import pytest

from eyegaze_multimodal_amd import _lib as L
from eyegaze_multimodal_amd import features as F
from tests import trialfeat_ref as T

from tests.trialfeat_fixture import FS, TRIALS, Z, raw, reference, restated  # noqa: E402


def test_fixture_shapes_and_conditions():
    assert [t[1:] for t in TRIALS] == [(256, 256), (257, 300), (500, 500), (777, 777), (1000, 1000), (3250, 3250)]
    assert float(Z["near_delta"]) == T.NEAR_DELTA
    for t, (C, L1, L2) in enumerate(TRIALS):
        n, ref = min(L1, L2), reference(t)
        assert raw(t)[0].shape == (C, L1) and raw(t)[1].shape == (C, L2)
        assert ref["freq_domain"].shape == (2, C, 129) and ref["bands_energy"].shape == (2, C, 5)
        assert ref["intra_con"].shape == (2, 7, 5, C, C) and ref["inter_con"].shape == (7, 5, C, C)
        assert ("time_domain" in ref) == (t < 2) and (t >= 2 or ref["time_domain"].shape == (2, C, n))
        assert np.array_equal(ref["freq_bins"], F.frequency_bins(FS))
        assert Z[f"near/{t}"].shape == (3, 5, C, C) and 2.0 * Z[f"near/{t}"].max() / n <= 0.02
    for k in Z.files:
        if k.startswith("tolerance/"):
            assert float(Z[k]) < 1e-3, k


@pytest.mark.parametrize("sums32", [False, True])
@pytest.mark.parametrize("t", range(len(TRIALS)))
def test_restatement_matches_the_reference_within_the_recorded_errors(t, sums32):
    got, ref = restated(t, sums32), reference(t)
    for name, d in T.distances(got, ref).items():
        assert d <= float(Z[f"restatement_err{32 if sums32 else 64}/{name}"]), (name, d)
    assert T.intra_diagonals_exact(got) and T.intra_diagonals_exact(ref)
    if not sums32:
        near = got["near"].copy()
        d = np.arange(TRIALS[t][0])
        near[:2, :, d, d] = 0
        assert np.array_equal(near, Z[f"near/{t}"])
        assert T.pli_excess(ref, got, Z[f"near/{t}"], float(Z["tolerance/pli_slack"]), min(TRIALS[t][1:])) <= 0


def test_band_coefficients_with_the_lower_clamp():
    names = [k.split("/")[1] for k in Z.files if k.startswith("coef/") and k.endswith("/band")]
    assert set(names) == {"delta", "theta", "alpha", "beta", "gamma", "pre", "clamped"}
    for name in names:
        lo, hi = Z[f"coef/{name}/band"]
        b, a = F.band_coefficients(float(lo), float(hi), FS)
        assert np.array_equal(b, Z[f"coef/{name}/b"]) and np.array_equal(a, Z[f"coef/{name}/a"]), name
    lo, hi = Z["coef/clamped/band"]
    assert lo / (FS / 2) < 0.001                                         # the clamp is what this band tests
    assert not np.array_equal(Z["coef/clamped/a"], Z["coef/delta/a"])


def test_band_bins_follow_the_float32_axis():
    k0, k1 = F.band_bins(F.FREQUENCY_BANDS, FS)
    f = F.frequency_bins(FS)
    for (lo, hi), a, b in zip(F.FREQUENCY_BANDS.values(), k0, k1):
        mask = (f >= lo) & (f <= hi)
        assert mask.sum() == b - a + 1 and mask[a:b + 1].all()
    assert F.band_bins({"none": (0.1, 0.2)}, FS) == ([0], [-1])


# ---------------------------------------------------------------------------------------------------------------
# host refusals: nothing below is dereferenced or launched
# ---------------------------------------------------------------------------------------------------------------
FAKE = 0x1000
DESC = dict(data=FAKE, row_off=FAKE, row_len=FAKE, ws_off=FAKE, n_rows=24, C=6, max_len=1000)
DESC_CASES = [(dict(data=0), "null pointer"), (dict(row_off=0), "null pointer"), (dict(row_len=0), "null pointer"),
              (dict(n_rows=0), "n_rows=0"), (dict(C=0), "C=0"), (dict(C=-2), "C=-2"), (dict(n_rows=18), "no multiple of 2 C=12"),
              (dict(max_len=255), "max_len=255 outside"), (dict(max_len=65537), "max_len=65537 outside")]


def desc_of(over):
    d = {**DESC, **{k: v for k, v in over.items() if k in DESC}}
    return L.RecordingRowsDesc(d["data"], d["row_off"], d["row_len"], d["ws_off"], d["n_rows"], d["C"], d["max_len"], 0)


def i32(v):
    return (ctypes.c_int32 * len(v))(*v)


@pytest.mark.parametrize("over,match", DESC_CASES + [
    (dict(psd=0), "null pointer"), (dict(energy=0), "null pointer"), (dict(k0=None), "null pointer"), (dict(fs=0.0), "fs=0"),
    (dict(nbands=9), "nbands=9 outside"), (dict(k1=[3, 129]), "bins \\[2, 129\\]"), (dict(k0=[-1, 2]), "bins \\[-1, 3\\]")])
def test_welch_host_checks(over, match):
    a = dict(fs=250.0, k0=[1, 2], k1=[3, 4], nbands=2, psd=FAKE, energy=FAKE, flag=0)
    a.update({k: v for k, v in over.items() if k in a})
    arr = lambda v: None if v is None else i32(v)
    with pytest.raises(L.EgError, match="eg_trial_welch: .*" + match):
        L.call("eg_trial_welch", ctypes.byref(desc_of(over)), a["fs"], arr(a["k0"]), arr(a["k1"]), a["nbands"], a["psd"], a["energy"], a["flag"], 0)


@pytest.mark.parametrize("over,match", DESC_CASES + [
    (dict(ws_off=0), "null pointer"), (dict(chirp=0), "null pointer"), (dict(amp=0), "null pointer"), (dict(cs=0), "null pointer"),
    (dict(sn=0), "null pointer"), (dict(ws=0), "null pointer"),
    (dict(cap=99999), "need 100000 workspace doubles .* capacity is 99999"), (dict(need=2048), "at least 3584")])
def test_analytic_host_checks(over, match):
    a = dict(chirp=FAKE, amp=FAKE, cs=FAKE, sn=FAKE, ws=FAKE, need=100000, cap=100000)
    a.update({k: v for k, v in over.items() if k in a})
    with pytest.raises(L.EgError, match="eg_trial_analytic: .*" + match):
        L.call("eg_trial_analytic", ctypes.byref(desc_of(over)), a["chirp"], a["amp"], a["cs"], a["sn"], a["ws"], a["need"], a["cap"], 0)


@pytest.mark.parametrize("over,match", DESC_CASES + [
    (dict(ws_off=0), "null pointer"), (dict(chirp=0), "null pointer"), (dict(ws=0), "null pointer"),
    (dict(cap=99999), "need 100000 workspace doubles .* capacity is 99999"), (dict(need=2048), "at least 3584")])
def test_analytic_tables_host_checks(over, match):
    a = dict(chirp=FAKE, ws=FAKE, need=100000, cap=100000)
    a.update({k: v for k, v in over.items() if k in a})
    with pytest.raises(L.EgError, match="eg_trial_analytic_tables: .*" + match):
        L.call("eg_trial_analytic_tables", ctypes.byref(desc_of(over)), a["chirp"], a["ws"], a["need"], a["cap"], 0)


@pytest.mark.parametrize("over,match", DESC_CASES + [
    (dict(amp=0), "null pointer"), (dict(cs=0), "null pointer"), (dict(sn=0), "null pointer"), (dict(ws=0), "null pointer"),
    (dict(con=0), "null pointer"), (dict(band=5), "band=5 outside"), (dict(band=-1), "band=-1 outside"), (dict(nbands=0), "nbands=0 outside"),
    (dict(nbands=9), "nbands=9 outside"), (dict(cap=5279), "need 5280 workspace floats, the workspace's capacity is 5279")])
def test_pairs_host_checks(over, match):
    assert L.trial_pairs_workspace_floats(24, 6, 1000) == 4 * 24 + 2 * 3 * 4 * 6 * 36 == 5280
    a = dict(amp=FAKE, cs=FAKE, sn=FAKE, ws=FAKE, cap=5280, con=FAKE, band=0, nbands=5)
    a.update({k: v for k, v in over.items() if k in a})
    with pytest.raises(L.EgError, match="eg_trial_pairs: .*" + match):
        L.call("eg_trial_pairs", ctypes.byref(desc_of(over)), a["amp"], a["cs"], a["sn"], a["ws"], a["cap"], a["con"], a["band"], a["nbands"], 0)


@pytest.mark.parametrize("over,match", DESC_CASES + [
    (dict(ws=0), "null pointer"), (dict(con=0), "null pointer"), (dict(band=5), "band=5 outside"), (dict(nbands=0), "nbands=0 outside"),
    (dict(cap=21671), "need 21672 workspace floats, the workspace's capacity is 21671")])
def test_coherence_host_checks(over, match):
    assert L.trial_coherence_workspace_floats(24, 1000) == 24 * 129 * (1 + 2 * 3) == 21672
    a = dict(ws=FAKE, cap=21672, con=FAKE, band=0, nbands=5)
    a.update({k: v for k, v in over.items() if k in a})
    with pytest.raises(L.EgError, match="eg_trial_coherence: .*" + match):
        L.call("eg_trial_coherence", ctypes.byref(desc_of(over)), a["ws"], a["cap"], a["con"], a["band"], a["nbands"], 0)


@pytest.mark.parametrize("over,match", [(dict(data=0), "null pointer"), (dict(row_off=0), "null pointer"), (dict(row_len=0), "null pointer"),
                                        (dict(n_rows=0), "n_rows=0"), (dict(C=0), "C=0"), (dict(n_rows=23), "no multiple of C=6")])
def test_car_host_checks(over, match):
    with pytest.raises(L.EgError, match="eg_recording_car: .*" + match):
        L.call("eg_recording_car", ctypes.byref(desc_of(over)), 0)


def test_filtfilt_exact_refuses_what_filtfilt_refuses():
    from tests.test_recprep_host import filt_args
    cases = [(dict(data=0), "null pointer"), (dict(ws_off=0), "null pointer"), (dict(b=None), "null pointer"), (dict(ws=0), "null pointer"),
             (dict(n_rows=0), "n_rows=0"), (dict(C=0), "C=0"), (dict(ncoef=1), "ncoef=1 outside"), (dict(a=[2.0] + [0.1] * 8), "must be 1"),
             (dict(cap=4999), "need 5000 workspace doubles, the workspace's capacity is 4999")]
    for over, match in cases:
        with pytest.raises(L.EgError, match="eg_recording_filtfilt_exact: .*" + match):
            L.call("eg_recording_filtfilt_exact", *filt_args(**over))


def test_workspace_helpers_refuse_bad_shapes():
    assert L.trial_analytic_twiddle_doubles(256) == 512 and L.trial_analytic_twiddle_doubles(3250) == 8192
    assert L.trial_analytic_twiddle_doubles(65536) == 131072
    assert L.trial_analytic_twiddle_doubles(255) == -1 and L.trial_analytic_twiddle_doubles(65537) == -1
    assert L.trial_pairs_workspace_floats(18, 6, 1000) == -1 and L.trial_pairs_workspace_floats(24, 6, 100) == -1
    assert L.trial_coherence_workspace_floats(0, 1000) == -1 and L.trial_coherence_workspace_floats(24, 70000) == -1


def test_analytic_tables_layout():
    rows, chirp, need = F.analytic_tables([256, 5000], 3)
    tw = 16384                                                            # 2 * 5000 - 1 -> M = 16384
    assert chirp.tolist() == [tw, tw + 2 * 512 + 2 * 256]
    first = tw + 2 * 512 + 2 * 256 + 2 * 16384 + 2 * 5000
    assert rows[:6].tolist() == [first] * 6                               # M = 512 transforms in LDS: no doubles of its own
    assert rows[6:].tolist() == [first + 2 * 16384 * i for i in range(6)] and need == first + 6 * 2 * 16384
    assert all(v % 2 == 0 for v in rows.tolist() + chirp.tolist())        # complex doubles stay 16-byte aligned


# ---------------------------------------------------------------------------------------------------------------
# the wrapper's refusals (before anything touches a device)
# ---------------------------------------------------------------------------------------------------------------
def test_extract_trial_features_refuses_lengths_and_channel_counts():
    z = lambda c, n: np.zeros((c, n), np.float32)
    with pytest.raises(ValueError, match="common length of 255 samples"):
        F.extract_trial_features([(z(6, 300), z(6, 300)), (z(6, 255), z(6, 400))], device="cpu")
    with pytest.raises(ValueError, match="common length of 65537 samples"):
        F.extract_trial_features([(z(2, 65537), z(2, 65537))], device="cpu")
    with pytest.raises(ValueError, match="trial 1 has 6 and 5 channels"):
        F.extract_trial_features([(z(6, 300), z(6, 300)), (z(6, 300), z(5, 300))], device="cpu")
    with pytest.raises(ValueError, match="trial 1 has 4 and 4 channels"):
        F.extract_trial_features([(z(6, 300), z(6, 300)), (z(4, 300), z(4, 300))], device="cpu")
    with pytest.raises(ValueError, match=r"\(C, L\) recordings"):
        F.extract_trial_features([(np.zeros(300, np.float32), z(6, 300))], device="cpu")
    with pytest.raises(ValueError, match="9 bands"):
        F.extract_trial_features([(z(6, 300), z(6, 300))], bands={str(i): (1.0 + i, 2.0 + i) for i in range(9)}, device="cpu")
    assert F.extract_trial_features([], device="cpu") == []


def test_header_declares_what_the_binding_binds():
    import re
    from tests.test_capi_symbols import REPO
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "eyegaze_hip.h").read_text(), flags=re.S)
    for name in ("eg_recording_car", "eg_recording_filtfilt_exact", "eg_trial_welch", "eg_trial_analytic_tables", "eg_trial_analytic", "eg_trial_pairs", "eg_trial_coherence",
                 "eg_trial_analytic_twiddle_doubles", "eg_trial_pairs_workspace_floats", "eg_trial_coherence_workspace_floats"):
        m = re.search(r"(?:int|int64_t)\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m and len(m.group(1).split(",")) == len(L.SIGNATURES[name]), name
    assert "trialfeat.hip" in __import__("eyegaze_multimodal_amd.build", fromlist=["SOURCES"]).SOURCES
