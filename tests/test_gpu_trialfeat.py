"""GPU tests of the trial features against the reference extractor's own outputs
(tests/golden/trial_features.npz) and the numpy restatement (tests/trialfeat_ref.py): every entry point alone on the fixture's
rows with sentinels around every row and workspace, extract_trial_features batched and one by one, full tiles at C = 32, the
transform that does not fit LDS, and the command line.

Tolerances are the fixture's: per continuous output twice the larger distance of the restatement's two variants from the
reference (the device contracts multiply-adds and orders its sums unlike both).  Where a test compares with the restatement on
identical inputs the same figures apply: device and restatement are then two correct evaluations that differ in rounding only."""
import ctypes
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd import features as F  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from tests import trialfeat_ref as T  # noqa: E402
from tests.trialfeat_fixture import FS, TRIALS, Z, analytic_signals, band_sides, raw, reference, restated  # noqa: E402

DEV = "cuda"
C = 6
C6 = [t for t, tr in enumerate(TRIALS) if tr[0] == C]                  # the five trials of six channels
SENTINEL = 12345.0
GAP = 5                                                                 # sentinel floats behind every row
GUARD = 64                                                              # sentinel elements behind every workspace and output
TOL = {k.split("/")[1]: float(Z[k]) for k in Z.files if k.startswith("tolerance/")}
BANDS = list(F.FREQUENCY_BANDS)
IDX = F.METRIC_NAMES.index


def stream():
    return torch.cuda.current_stream().cuda_stream


class Rows:
    """the C = 6 trials' 60 rows in one store with GAP sentinel floats behind every row"""

    def __init__(self, source, trials=C6, Cn=C):
        """source(trial, player) -> (Cn, L) float32"""
        recs = [np.asarray(source(t, w), np.float32) for t in trials for w in (0, 1)]
        self.lengths = [recs[2 * i].shape[1] for i in range(len(trials))]
        lens = np.repeat([r.shape[1] for r in recs], Cn).astype(np.int64)
        self.Cn, self.n_rows, self.max_len = Cn, len(lens), int(lens.max())
        self.row_off = np.concatenate([[0], np.cumsum(lens + GAP)])[:-1]
        self.row_len = lens.astype(np.int32)
        self.floats = int((lens + GAP).sum())
        host = np.full(self.floats, SENTINEL, np.float32)
        self.is_row = np.zeros(self.floats, bool)
        for r, x in enumerate(row for q in recs for row in q):
            host[self.row_off[r]:self.row_off[r] + len(x)] = x
            self.is_row[self.row_off[r]:self.row_off[r] + len(x)] = True
        self.host = host
        self.data = torch.from_numpy(host).to(DEV)
        an_off, chirp_off, self.an_need = F.analytic_tables(self.lengths, Cn)
        self.tabs = [torch.from_numpy(t).to(DEV) for t in (self.row_off, self.row_len, an_off, chirp_off)]
        self.desc = L.RecordingRowsDesc(ptr(self.data), ptr(self.tabs[0]), ptr(self.tabs[1]), ptr(self.tabs[2]), self.n_rows, Cn,
                                        self.max_len, 0)

    def plane(self):
        return torch.full((self.floats,), SENTINEL, dtype=torch.float32, device=DEV)

    def rows_of(self, flat, i):
        """(2, Cn, L) of trial i from a flat host image"""
        r0 = 2 * self.Cn * i
        return np.stack([flat[self.row_off[r]:self.row_off[r] + self.row_len[r]] for r in range(r0, r0 + 2 * self.Cn)]).reshape(
            2, self.Cn, -1)

    def untouched(self, flat):
        return bool((flat[~self.is_row] == np.float32(SENTINEL)).all())

    def analytic(self):
        amp, cs, sn = self.plane(), self.plane(), self.plane()
        ws = torch.full((self.an_need + GUARD,), -7.0, dtype=torch.float64, device=DEV)
        call("eg_trial_analytic_tables", ctypes.byref(self.desc), ptr(self.tabs[3]), ptr(ws), self.an_need, self.an_need, stream())
        call("eg_trial_analytic", ctypes.byref(self.desc), ptr(self.tabs[3]), ptr(amp), ptr(cs), ptr(sn), ptr(ws), self.an_need, self.an_need,
             stream())
        return amp, cs, sn, ws

    def con(self, nb=5):
        return torch.full((len(self.lengths) * 3 * 7 * nb * self.Cn * self.Cn + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)

    def con_view(self, con, nb=5):
        return con[:-GUARD].view(len(self.lengths), 3, 7, nb, self.Cn, self.Cn).cpu().numpy()


def band_rows(bi, part):
    """the restatement's float32 rows of band bi: part 0 the band signal, 1 amplitude, 2 cos, 3 sin"""
    return lambda t, w: band_sides(t)[bi][w][part]


def test_car_is_the_stated_pass_bit_for_bit():
    """eg_recording_car against the CAR arithmetic eg_recording_car_zscore states (channel sum in float32 in channel order), and
    against the first launch of eg_recording_car_zscore itself: z-scoring the CAR output by hand gives that entry point's bits."""
    rows = Rows(lambda t, w: raw(t)[w][:, :min(TRIALS[t][1:])])
    call("eg_recording_car", ctypes.byref(rows.desc), stream())
    got = rows.data.cpu().numpy()
    assert rows.untouched(got)
    for i, t in enumerate(C6):
        for w in (0, 1):
            assert np.array_equal(rows.rows_of(got, i)[w], T.car_ref(raw(t)[w][:, :min(TRIALS[t][1:])]))
    both = Rows(lambda t, w: raw(t)[w][:, :min(TRIALS[t][1:])])
    call("eg_recording_car_zscore", ctypes.byref(both.desc), stream())
    z = both.data.cpu().numpy()
    for i in range(len(C6)):
        v = rows.rows_of(got, i).reshape(2 * C, -1)
        v64 = v.astype(np.float64)
        mean = v64.sum(axis=1, keepdims=True) / v.shape[1]
        std = np.sqrt(((v64 - mean) ** 2).sum(axis=1, keepdims=True) / v.shape[1])
        np.testing.assert_allclose(both.rows_of(z, i).reshape(2 * C, -1), (v - mean.astype(np.float32)) / (std.astype(np.float32) + np.float32(1e-8)),
                                   rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("band", ["delta", "gamma"])
def test_filtfilt_exact_gives_the_restatements_bits(band):
    """The uncontracted recurrence performs the restatement's (and scipy's) operations one by one, so the band signal is the
    restatement's bit for bit -- also in the 0.5-4 Hz band, where a contracted recurrence is 1e-4 of the signal away."""
    from eyegaze_multimodal_amd.data import recording_row_tables
    from eyegaze_multimodal_amd.filters import lfilter_zi
    bi = BANDS.index(band)
    rows = Rows(lambda t, w: restated(t)["time_domain"][w])
    b, a = F.band_coefficients(*F.FREQUENCY_BANDS[band], FS)
    _, _, ws_off, _, need = recording_row_tables([x for x in rows.lengths for _ in (0, 1)], C, 27)
    t_ws = torch.from_numpy(ws_off).to(DEV)
    ws = torch.full((need + GUARD,), -7.0, dtype=torch.float64, device=DEV)
    desc = L.RecordingRowsDesc(ptr(rows.data), ptr(rows.tabs[0]), ptr(rows.tabs[1]), ptr(t_ws), rows.n_rows, C, rows.max_len, 0)
    dbl = lambda v: (ctypes.c_double * len(v))(*[float(x) for x in v])
    call("eg_recording_filtfilt_exact", ctypes.byref(desc), dbl(b), dbl(a), dbl(lfilter_zi(b, a)), len(b), ptr(ws), need, need, stream())
    got = rows.data.cpu().numpy()
    assert rows.untouched(got) and (ws[need:] == -7.0).all()
    for i, t in enumerate(C6):
        for w in (0, 1):
            assert np.array_equal(rows.rows_of(got, i)[w], band_sides(t)[bi][w][0]), (t, w)


def test_welch_matches_the_reference_psd_and_band_energy():
    rows = Rows(lambda t, w: restated(t)["time_domain"][w])
    psd = torch.full((rows.n_rows * 129 + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    energy = torch.full((rows.n_rows * 5 + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    flag = torch.zeros(1 + GUARD, dtype=torch.int32, device=DEV)
    k0, k1 = F.band_bins(F.FREQUENCY_BANDS, FS)
    i32 = lambda v: (ctypes.c_int32 * len(v))(*v)
    call("eg_trial_welch", ctypes.byref(rows.desc), float(FS), i32(k0), i32(k1), 5, ptr(psd), ptr(energy), ptr(flag), stream())
    assert rows.untouched(rows.data.cpu().numpy()) and np.array_equal(rows.data.cpu().numpy(), rows.host)
    assert (psd[-GUARD:] == SENTINEL).all() and (energy[-GUARD:] == SENTINEL).all() and int(flag.abs().sum()) == 0
    p, e = psd[:-GUARD].view(-1, 2, C, 129).cpu().numpy(), energy[:-GUARD].view(-1, 2, C, 5).cpu().numpy()
    for i, t in enumerate(C6):
        d = T.distances({**reference(t), "freq_domain": p[i], "bands_energy": e[i]}, reference(t))
        print(f"trial {t}: PSD {d['freq_domain']:.2e} (tolerance {TOL['freq_domain']:.2e}), band energy {d['bands_energy']:.2e} "
              f"(tolerance {TOL['bands_energy']:.2e})")
        assert d["freq_domain"] <= TOL["freq_domain"] and d["bands_energy"] <= TOL["bands_energy"], (t, d)


@pytest.mark.parametrize("band", ["delta", "beta"])
def test_analytic_signal_matches_the_float64_restatement(band):
    """Amplitude and unit phasor against numpy's float64 FFT.  Bounds: the amplitude is one rounding to float32 of a float64 value
    that agrees with numpy's to ~1e-13 relative, so one float32 spacing at the row's largest amplitude; a phasor component is a
    float32 rounding of a value in [-1, 1] (6e-8) plus the float64 error of z divided by |z| (1e-13 max|z| / |z|)."""
    bi = BANDS.index(band)
    rows = Rows(band_rows(bi, 0))
    amp, cs, sn, ws = rows.analytic()
    assert np.array_equal(rows.data.cpu().numpy(), rows.host)                                          # the band signal is only read
    a, c, s, w = amp.cpu().numpy(), cs.cpu().numpy(), sn.cpu().numpy(), ws.cpu().numpy()
    assert rows.untouched(a) and rows.untouched(c) and rows.untouched(s) and (w[rows.an_need:] == -7.0).all()
    for i, t in enumerate(C6):
        for pl in (0, 1):
            z = analytic_signals(t)[bi][pl]
            mag = np.abs(z)
            assert np.abs(rows.rows_of(a, i)[pl] - mag).max() <= np.spacing(np.float32(mag.max()))
            bound = 1.2e-7 + 1e-12 * mag.max() / mag
            assert (np.abs(rows.rows_of(c, i)[pl] - z.real / mag) <= bound).all() and (np.abs(rows.rows_of(s, i)[pl] - z.imag / mag) <= bound).all()


def test_analytic_signal_beyond_the_lds_transform():
    """L = 4097 (M = 16384 > 8192) runs in workspace doubles, next to a trial of 300 that runs in LDS, in one call; and an all-zero
    row gives amplitude 0 and the phasor (1, 0)."""
    rng = np.random.default_rng(7)
    recs = {(0, 0): rng.normal(0, 10, (1, 4097)), (0, 1): rng.normal(0, 10, (1, 4097)), (1, 0): rng.normal(0, 10, (1, 300)),
            (1, 1): np.zeros((1, 300))}
    rows = Rows(lambda t, w: recs[(t, w)], trials=[0, 1], Cn=1)
    amp, cs, sn, ws = rows.analytic()
    a, c, s, w = amp.cpu().numpy(), cs.cpu().numpy(), sn.cpu().numpy(), ws.cpu().numpy()
    assert rows.untouched(a) and rows.untouched(c) and rows.untouched(s) and (w[rows.an_need:] == -7.0).all()
    for (t, pl), x in recs.items():
        _, _, _, z = T.analytic_ref(x.astype(np.float32))
        mag = np.abs(z[0])
        ga, gc, gs = (rows.rows_of(v, t)[pl][0] for v in (a, c, s))
        if not mag.any():
            assert (ga == 0).all() and (gc == 1).all() and (gs == 0).all()
            continue
        assert np.abs(ga - mag).max() <= np.spacing(np.float32(mag.max()))
        bound = 1.2e-7 + 1e-12 * mag.max() / mag
        assert (np.abs(gc - z[0].real / mag) <= bound).all() and (np.abs(gs - z[0].imag / mag) <= bound).all()


def check_connectivity(got, ref, near, L_, metrics, what):
    """got, ref (3, 7, nb, C, C); the fixture's tolerances per metric, phase_diff as the complex mean, PLI by the near rule"""
    worst = {}
    for name in metrics:
        if name in T.CONTINUOUS:
            worst[name] = float(np.abs(got[:, IDX(name)] - ref[:, IDX(name)]).max())
    if "phase_diff" in metrics:
        mean = lambda c: c[:, IDX("plv")] * np.exp(1j * c[:, IDX("phase_diff")])
        worst["phase_diff"] = float(np.abs(mean(got) - mean(ref)).max())
    print(what + ": " + ", ".join(f"{k} {v:.2e} (tolerance {TOL[k]:.2e})" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= TOL[name], (what, name, v, TOL[name])
    if "pli" in metrics:
        d = np.abs(got[:, IDX("pli")].astype(np.float64) - ref[:, IDX("pli")])
        excess = float(((d - TOL["pli_slack"]) * L_ / 2 - near).max())
        print(f"{what}: PLI excess {excess:.2e} samples, up to {int(near.max())} near samples")
        assert excess <= 0, (what, excess)


PAIR_METRICS = ["pearson", "power_corr", "plv", "pli", "wpli", "phase_diff"]


def run_pairs_and_coherence(bi):
    rows = Rows(band_rows(bi, 0))
    planes = []
    for part in (1, 2, 3):
        src = Rows(band_rows(bi, part))
        planes.append(src.data)
    pair_need, coh_need = L.trial_pairs_workspace_floats(rows.n_rows, C, rows.max_len), L.trial_coherence_workspace_floats(rows.n_rows, rows.max_len)
    pws = torch.full((pair_need + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    cws = torch.full((coh_need + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    con = rows.con()
    call("eg_trial_pairs", ctypes.byref(rows.desc), ptr(planes[0]), ptr(planes[1]), ptr(planes[2]), ptr(pws), pair_need, ptr(con), bi, 5, stream())
    call("eg_trial_coherence", ctypes.byref(rows.desc), ptr(cws), coh_need, ptr(con), bi, 5, stream())
    return rows, planes, pws, cws, con


@pytest.mark.parametrize("band", ["theta", "gamma"])
def test_pairs_and_coherence_match_the_restatement_and_stay_in_bounds(band):
    bi = BANDS.index(band)
    runs = []
    for _ in range(2):
        rows, planes, pws, cws, con = run_pairs_and_coherence(bi)
        assert np.array_equal(rows.data.cpu().numpy(), rows.host)                                      # inputs are only read
        assert (pws[-GUARD:] == SENTINEL).all() and (cws[-GUARD:] == SENTINEL).all() and (con[-GUARD:] == SENTINEL).all()
        got = rows.con_view(con)
        other = [b for b in range(5) if b != bi]
        assert (got[:, :, :, other] == np.float32(SENTINEL)).all()                                      # only this band's entries are written
        runs.append(got[:, :, :, bi].copy())
    assert runs[0].tobytes() == runs[1].tobytes()                                                       # no atomics: bit-reproducible
    for i, t in enumerate(C6):
        ref = T.stack_con(restated(t))[:, :, bi:bi + 1]
        check_connectivity(runs[0][i][:, :, None], ref, Z[f"near/{t}"][:, bi:bi + 1], min(TRIALS[t][1:]), F.METRIC_NAMES, f"trial {t} {band}")
        d = np.arange(C)
        for name in ("pli", "wpli", "phase_diff"):
            assert (runs[0][i][:2, IDX(name)][:, d, d] == 0).all(), name


def features_close_to_reference(got, t, what):
    ref = reference(t)
    Cn, n = TRIALS[t][0], min(TRIALS[t][1:])
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert g["time_domain"].shape == (2, Cn, n) and g["freq_domain"].shape == (2, Cn, 129) and g["freq_bins"].shape == (129,)
    assert g["bands_energy"].shape == (2, Cn, 5) and g["intra_con"].shape == (2, 7, 5, Cn, Cn) and g["inter_con"].shape == (7, 5, Cn, Cn)
    assert all(v.dtype == np.float32 for v in g.values()) and all(v.is_cuda and v.is_contiguous() for v in got.values())
    assert np.array_equal(g["freq_bins"], ref["freq_bins"])
    if "time_domain" in ref:
        # the uncontracted filter performs scipy's operations one by one and the CAR pass is the reference's arithmetic, so the
        # preprocessed signals are the reference's bit for bit
        assert np.array_equal(g["time_domain"], ref["time_domain"])
    d = T.distances(g, ref)
    print(f"{what}: PSD {d['freq_domain']:.2e} ({TOL['freq_domain']:.2e}), band energy {d['bands_energy']:.2e} ({TOL['bands_energy']:.2e})")
    assert d["freq_domain"] <= TOL["freq_domain"] and d["bands_energy"] <= TOL["bands_energy"], (what, d)
    check_connectivity(T.stack_con(g), T.stack_con(ref), Z[f"near/{t}"], n, F.METRIC_NAMES, what)
    assert T.intra_diagonals_exact(g)


def same_bytes(a, b):
    return all(a[k].shape == b[k].shape and a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in a)


def test_extract_trial_features_ragged_call_matches_the_reference():
    """All C = 6 trials in ONE ragged call (device tensors and numpy arrays mixed), the C = 3 trial of 3250 samples in a second one
    -- a call has one C -- against the reference's outputs; every trial alone gives the batched call's bytes."""
    pairs = [raw(t) for t in C6]
    pairs[1] = tuple(torch.from_numpy(x).to(DEV) for x in pairs[1])
    out = F.extract_trial_features(pairs, FS, device=DEV)
    assert len(out) == len(C6)
    for o, t in zip(out, C6):
        features_close_to_reference(o, t, f"trial {t}")
    for o, t in zip(out, C6):
        assert same_bytes(o, F.extract_trial_features([raw(t)], FS, device=DEV)[0]), t
    assert same_bytes(out[0], F.extract_trial_features(pairs, FS, device=DEV)[0])
    long_ = len(TRIALS) - 1
    features_close_to_reference(F.extract_trial_features([raw(long_)], FS, device=DEV)[0], long_, "trial of 3250")


def test_batches_do_not_change_the_bytes(monkeypatch):
    pairs = [raw(t) for t in C6]
    whole = F.extract_trial_features(pairs, FS, device=DEV)
    monkeypatch.setattr(F, "FEATURE_BATCH_BYTES", 1)                        # every trial its own batch, still one sync
    split = F.extract_trial_features(pairs, FS, device=DEV)
    assert all(same_bytes(a, b) for a, b in zip(whole, split))


def test_full_tiles_at_32_channels_match_the_restatement():
    """C = 32 (full 32 x 32 pair tiles, the workload's channel count), L = 512 (two splits) against tests/trialfeat_ref.  The
    fixture's tolerances apply: L sits between its 500 and 777, and device and restatement differ in rounding only."""
    rng = np.random.default_rng(11)
    t = np.arange(512) / FS
    shared = np.cumsum(rng.normal(0, 1.5, 512)) + rng.normal(0, 6.0, 512)
    recs = []
    for _ in (0, 1):
        x = rng.uniform(-4000, 4000, (32, 1)) + np.cumsum(rng.normal(0, 2.0, (32, 512)), axis=1) + rng.normal(0, 5.0, (32, 512))
        for f, amp in ((6.0, 15.0), (10.0, 20.0), (20.0, 10.0)):
            x = x + amp * rng.uniform(0.5, 1.0, (32, 1)) * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi, (32, 1)))
        recs.append((x + rng.uniform(0.4, 1.0, (32, 1)) * shared).astype(np.float32))
    ref = T.trial_features_ref(*recs, fs=FS)
    got = {k: v.cpu().numpy() for k, v in F.extract_trial_features([tuple(recs)], FS, device=DEV)[0].items()}
    near = ref["near"].copy()
    d = np.arange(32)
    near[:2, :, d, d] = 0
    assert np.array_equal(got["time_domain"], ref["time_domain"])                       # same operations, one by one: the same bits
    dist = T.distances(got, ref)
    assert dist["freq_domain"] <= TOL["freq_domain"] and dist["bands_energy"] <= TOL["bands_energy"], dist
    check_connectivity(T.stack_con(got), T.stack_con(ref), near, 512, F.METRIC_NAMES, "C = 32")
    assert T.intra_diagonals_exact(got)


def test_non_finite_input_is_refused():
    x = raw(0)
    bad = x[1].copy()
    bad[3, 100] = np.nan
    with pytest.raises(ValueError, match="NaN or Inf"):
        F.extract_trial_features([x, (x[0], bad)], FS, device=DEV)
    bad[3, 100] = np.inf
    with pytest.raises(ValueError, match="NaN or Inf"):
        F.extract_trial_features([(bad, x[0])], FS, device=DEV)


def test_command_line_writes_the_scripts_files(tmp_path):
    eeg, out = tmp_path / "eeg", tmp_path / "features"
    eeg.mkdir()
    meta = []
    for t, cls in ((2, "Cooperation"), (1, "Single"), (3, "Comp")):
        for w in (0, 1):
            np.savetxt(eeg / f"t{t}p{w}.csv", raw(t)[w], delimiter=",", fmt="%.9e")
        meta.append({"player1": f"t{t}p0", "player2": f"t{t}p1", "class": cls, "pair": 10 + t})
    meta.append({"player1": "t2p0", "player2": "nobody", "class": "Single", "pair": 1})
    bad = raw(3)[0].copy()
    bad[2, 40] = np.nan                                                  # one bad trial costs its own file, not its batch's
    np.savetxt(eeg / "nanp0.csv", bad, delimiter=",", fmt="%.9e")
    meta.insert(1, {"player1": "nanp0", "player2": "t3p1", "class": "Coop", "pair": 2})
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    argv = ["--metadata", str(tmp_path / "meta.json"), "--eeg-dir", str(eeg), "--output-dir", str(out)]
    assert F.main(argv) == 0
    results = {r["trial_id"]: r for r in F.run_extraction(meta, eeg, tmp_path / "again")}
    assert {k: r["status"] for k, r in results.items()} == {"t2p0_t2p1": "success", "nanp0_t3p1": "error", "t1p0_t1p1": "error",
                                                            "t3p0_t3p1": "success", "t2p0_nobody": "error"}
    assert "NaN or Inf" in results["nanp0_t3p1"]["error"] and "too short" in results["t1p0_t1p1"]["error"]
    assert "not found" in results["t2p0_nobody"]["error"]
    assert sorted(p.name for p in out.glob("*.npy")) == ["t2p0_t2p1.npy", "t3p0_t3p1.npy"]      # 257 samples: below the script's two seconds
    for t, cls, idx in ((2, "Cooperation", 2), (3, "Comp", 1)):
        f = np.load(out / f"t{t}p0_t{t}p1.npy", allow_pickle=True).item()
        assert list(f) == ["time_domain", "freq_domain", "freq_bins", "bands_energy", "intra_con", "inter_con", "metadata"]
        n = min(TRIALS[t][1:])
        assert f["metadata"] == {"player1": f"t{t}p0", "player2": f"t{t}p1", "class": cls, "class_idx": idx, "pair": 10 + t, "timepoints": n,
                                 "sampling_rate": 250, "bands": BANDS, "metrics": F.METRIC_NAMES}
        assert all(isinstance(f[k], np.ndarray) and f[k].dtype == np.float32 for k in f if k != "metadata")
        assert f["time_domain"].shape == (2, C, n) and f["intra_con"].shape == (2, 7, 5, C, C) and f["inter_con"].shape == (7, 5, C, C)
        ref = reference(t)
        assert np.array_equal(f["freq_bins"], ref["freq_bins"]) and f["freq_domain"].shape == ref["freq_domain"].shape
        assert np.abs(f["inter_con"][IDX("pearson")] - ref["inter_con"][IDX("pearson")]).max() <= TOL["pearson"]
    stamps = {p.name: p.stat().st_mtime_ns for p in out.glob("*.npy")}
    (out / "t3p0_t3p1.npy").unlink()
    assert F.main(argv + ["--resume"]) == 0
    assert (out / "t3p0_t3p1.npy").exists()                                                         # the missing one is written again
    assert (out / "t2p0_t2p1.npy").stat().st_mtime_ns == stamps["t2p0_t2p1.npy"]                    # the existing one is not touched
