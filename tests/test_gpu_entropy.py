"""GPU tests of the entropy analysis against the reference's own outputs (tests/golden/entropy.npz) and the numpy
restatement (tests/entropy_ref.py): both entry points alone with sentinels behind every row, workspace and output, the two calls
batched and one by one, and the command line.

Tolerances: the spectral entropy within the fixture's tolerance/spectral of the reference (twice the restatement's own distance,
all of it the one rounding of the filtered signal to float32) and within 1e-10 of the restatement on identical float32 rows (two
fp64 evaluations that differ in rounding only); the spatial entropy within 1e-10 bits (derived in DESIGN.md §8n)."""
import csv
import ctypes
import logging
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd import entropy as E  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from tests import entropy_ref as ER  # noqa: E402
from tests.entropy_fixture import (EEG_NAMES, FS, IMAGE_NAMES, TOL_SPATIAL, TOL_SPECTRAL, filtered, image, image_entropy, raw,  # noqa: E402
                                   reference_entropy)

DEV = "cuda"
SENTINEL = 12345.0
GAP = 5                 # sentinel floats behind every row
GUARD = 64              # sentinel elements behind every workspace and output
SAME_ROWS = 1e-10       # device against restatement on identical rows


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------
# eg_trial_spectral_entropy
# ---------------------------------------------------------------------------------------------------------------
class Rows:
    """single channel rows (C = 1) in one store with GAP sentinel floats behind every row"""

    def __init__(self, rows, max_len=None):
        lens = np.asarray([len(r) for r in rows], np.int64)
        self.n_rows, self.max_len = len(rows), int(max_len or lens.max())
        self.row_off = np.concatenate([[0], np.cumsum(lens + GAP)])[:-1]
        self.host = np.full(int((lens + GAP).sum()), SENTINEL, np.float32)
        for off, r in zip(self.row_off, rows):
            self.host[off:off + len(r)] = r
        self.data = torch.from_numpy(self.host).to(DEV)
        self.tabs = [torch.from_numpy(self.row_off).to(DEV), torch.from_numpy(lens.astype(np.int32)).to(DEV)]
        self.desc = L.RecordingRowsDesc(ptr(self.data), ptr(self.tabs[0]), ptr(self.tabs[1]), 0, self.n_rows, 1, self.max_len, 0)

    def entropy(self, with_psd=True, fs=FS):
        """-> (entropy [n_rows] f64, psd [n_rows, 129] f32 or None), the sentinels behind both checked"""
        out = torch.full((self.n_rows + GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
        psd = torch.full((self.n_rows * 129 + GUARD,), SENTINEL, dtype=torch.float32, device=DEV) if with_psd else None
        call("eg_trial_spectral_entropy", ctypes.byref(self.desc), fs, E.EPS, ptr(psd), ptr(out), stream())
        assert self.data.cpu().numpy().tobytes() == self.host.tobytes()                                # inputs are only read (bytes: rows may hold NaN)
        assert (out[self.n_rows:] == SENTINEL).all() and (psd is None or (psd[-GUARD:] == SENTINEL).all())
        return out[:self.n_rows].cpu().numpy(), None if psd is None else psd[:-GUARD].view(self.n_rows, 129).cpu().numpy()


def fixture_rows():
    """every channel of every fixture recording, band-passed by the restatement: (rows, reference entropies)"""
    return [r for n in EEG_NAMES for r in filtered(n)], np.concatenate([reference_entropy(n) for n in EEG_NAMES])


def test_spectral_entry_point_matches_reference_and_restatement():
    rows, ref = fixture_rows()
    store = Rows(rows)
    got, psd = store.entropy()
    restated = np.concatenate([ER.spectral_entropy_of_rows(filtered(n), FS) for n in EEG_NAMES])
    d_ref, d_same = np.abs(got - ref), np.abs(got - restated)
    print(f"spectral entropy: {d_ref.max():.2e} from the reference (tolerance {TOL_SPECTRAL:.2e}), {d_same.max():.2e} from the restatement")
    assert got.dtype == np.float64 and d_ref.max() <= TOL_SPECTRAL and d_same.max() <= SAME_ROWS
    zero = sum(len(filtered(n)) for n in EEG_NAMES[:EEG_NAMES.index("special")]) + 1
    assert not rows[zero].any() and abs(got[zero] - math.log2(129)) <= 1e-12                         # the all-zero row
    assert abs(got[zero + 1] - math.log2(129)) <= 1e-9                                               # the constant row, as the reference
    # the optional PSD is eg_trial_welch's, byte for byte; without it the entropies are the same bytes
    assert store.n_rows % 2 == 0
    welch = torch.full((store.n_rows * 129 + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    energy = torch.full((store.n_rows + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    k = (ctypes.c_int32 * 1)(0)
    call("eg_trial_welch", ctypes.byref(store.desc), FS, k, k, 1, ptr(welch), ptr(energy), 0, stream())
    assert welch[:-GUARD].cpu().numpy().tobytes() == psd.tobytes()
    again, none = store.entropy(with_psd=False)
    assert none is None and again.tobytes() == got.tobytes()


def test_spectral_entry_point_odd_row_count_skipped_row_and_non_finite_rows():
    rows, _ = fixture_rows()
    clean, _ = Rows(rows).entropy()
    # five rows, C = 1: eg_trial_welch would refuse them; the third is shorter than a segment and is skipped
    five = [rows[0], rows[1], rows[4][:200], rows[2], rows[10]]
    store = Rows(five)
    got, psd = store.entropy()
    assert got[2] == SENTINEL and (psd[2] == np.float32(SENTINEL)).all()
    assert got[[0, 1, 3, 4]].tobytes() == clean[[0, 1, 2, 10]].tobytes()                             # a row's bytes do not depend on the batch
    # a row longer than max_len is skipped too
    got, _ = Rows(five, max_len=len(rows[2])).entropy()
    assert got[4] == SENTINEL and got[2] == SENTINEL and got[[0, 1, 3]].tobytes() == clean[[0, 1, 2]].tobytes()
    # NaN and Inf: that row's entropy is NaN, no other row moves
    bad = [r.copy() for r in rows]
    bad[1][100] = np.nan
    bad[12][300] = np.inf
    got, _ = Rows(bad).entropy()
    assert np.isnan(got[1]) and np.isnan(got[12])
    keep = np.ones(len(rows), bool)
    keep[[1, 12]] = False
    assert got[keep].tobytes() == clean[keep].tobytes()


# ---------------------------------------------------------------------------------------------------------------
# spectral_entropy
# ---------------------------------------------------------------------------------------------------------------
def recordings():
    recs = [raw(n) for n in EEG_NAMES]
    recs[2] = torch.from_numpy(recs[2]).to(DEV)                          # device tensors and numpy arrays mixed
    return recs


def as_bytes(tensors):
    return [t.cpu().numpy().tobytes() for t in tensors]


def test_spectral_entropy_ragged_call_matches_the_reference(monkeypatch):
    recs = recordings()
    assert len({r.shape[0] for r in recs}) > 1 and len({r.shape[1] for r in recs}) > 1               # ragged in channels AND length
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                              # a synchronising torch call inside raises
    try:
        out = E.spectral_entropy(recs, FS, device=DEV)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(out) == len(recs)
    worst = 0.0
    for o, n in zip(out, EEG_NAMES):
        assert o.is_cuda and o.dtype == torch.float64 and tuple(o.shape) == (raw(n).shape[0],)
        worst = max(worst, float(np.abs(o.cpu().numpy() - reference_entropy(n)).max()))
    print(f"spectral_entropy: {worst:.2e} from the reference (tolerance {TOL_SPECTRAL:.2e})")
    assert worst <= TOL_SPECTRAL
    whole = as_bytes(out)
    for i, r in enumerate(recs):                                         # every recording alone gives the batched call's bytes
        assert as_bytes(E.spectral_entropy([r], FS, device=DEV)) == [whole[i]], EEG_NAMES[i]
    monkeypatch.setattr(E, "ENTROPY_BATCH_BYTES", 1)                     # every recording its own batch
    assert as_bytes(E.spectral_entropy(recs, FS, device=DEV)) == whole


def test_spectral_entropy_without_the_filter_matches_the_restatement():
    names = ["len383", "len3250"]
    out = E.spectral_entropy([raw(n) for n in names], FS, apply_filter=False, device=DEV)
    for o, n in zip(out, names):
        assert np.abs(o.cpu().numpy() - ER.spectral_entropy_ref(raw(n), FS, apply_filter=False)).max() <= SAME_ROWS


# ---------------------------------------------------------------------------------------------------------------
# eg_image_entropy
# ---------------------------------------------------------------------------------------------------------------
def run_images(images, normalize=True, max_pix=None, layouts=None, shift=0):
    """eg_image_entropy on one batch: images 16-byte aligned (+ shift elements) with a sentinel gap between them, sentinels behind
    workspace and output -> entropy [n] f64"""
    elem = 0 if images[0].dtype == np.uint8 else 1
    align = 16 if elem == 0 else 2
    lay = [E.image_layout(im.shape) for im in images] if layouts is None else layouts
    npix = [im.size // (1 if E.image_layout(im.shape) == E.GREY else 3) for im in images]
    off, at = [], 0
    for im in images:
        off.append(at + shift)
        at += -(-(im.size + shift) // align) * align + align
    host = np.full(at, 171, images[0].dtype)
    for im, o in zip(images, off):
        host[o:o + im.size] = np.ascontiguousarray(im).reshape(-1)
    data = torch.from_numpy(host).to(DEV)
    tabs = [torch.tensor(off, dtype=torch.int64, device=DEV), torch.tensor(npix, dtype=torch.int32, device=DEV),
            torch.tensor(lay, dtype=torch.int32, device=DEV)]
    n, max_pix = len(images), max_pix or max(npix)
    need = L.image_entropy_workspace_doubles(n, max_pix)
    ws = torch.full((need + GUARD,), -7.0, dtype=torch.float64, device=DEV)
    out = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    desc = L.ImageBatchDesc(ptr(data), ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), n, max_pix, elem, int(normalize))
    call("eg_image_entropy", ctypes.byref(desc), E.EPS, ptr(ws), need, ptr(out), stream())
    assert data.cpu().numpy().tobytes() == host.tobytes()                                           # inputs are only read
    assert (ws[need:] == -7.0).all() and (out[n:] == SENTINEL).all()
    return out[:n].cpu().numpy()


U8_NAMES = [n for n in IMAGE_NAMES if image(n).dtype == np.uint8]


@pytest.mark.parametrize("normalize", [True, False])
def test_image_entry_point_matches_the_reference(normalize):
    imgs = [image(n) for n in U8_NAMES]
    assert len(imgs) == 6
    got = run_images(imgs, normalize)
    ref = np.asarray([image_entropy(n, normalize) for n in U8_NAMES])
    print(f"spatial entropy (normalize={normalize}): {np.abs(got - ref).max():.2e} from the reference (gate {TOL_SPATIAL:.0e})")
    assert np.abs(got - ref).max() <= TOL_SPATIAL
    if normalize:
        assert abs(got[U8_NAMES.index("constant_8x8")] - 6.0) <= TOL_SPATIAL
    assert run_images(imgs, normalize).tobytes() == got.tobytes()                                    # two runs: the same bytes
    for i, im in enumerate(imgs):                                                                    # alone: the batch's bytes
        assert run_images([im], normalize).tobytes() == got[i:i + 1].tobytes(), U8_NAMES[i]


def test_image_entry_point_float64_elements():
    rng = np.random.default_rng(5)
    imgs = [image("f64_50x60x3"), rng.random((33, 47)) * 3.0 - 1.0, rng.random((3, 21, 35))]
    for normalize in (True, False):
        got = run_images(imgs, normalize)
        want = np.asarray([ER.spatial_entropy_ref(im, normalize) for im in imgs])
        assert np.abs(got - want).max() <= TOL_SPATIAL
        assert abs(got[0] - image_entropy("f64_50x60x3", normalize)) <= TOL_SPATIAL
        assert run_images(imgs[:1], normalize).tobytes() == got[:1].tobytes()


def test_image_entry_point_many_chunks_ragged_tail_and_tiny_images():
    """301 x 517 = 155617 pixels: 19 chunks of 8192, the last of 8161 pixels that ends in a group of one pixel; in all three
    layouts, next to a 1 x 1 image and a one-chunk image"""
    rng = np.random.default_rng(6)
    big = rng.integers(0, 256, (301, 517, 3), dtype=np.uint8)
    imgs = [big, np.full((1, 1), 9, np.uint8), rng.integers(0, 256, (64, 100), dtype=np.uint8), rng.integers(0, 256, (301, 517), dtype=np.uint8),
            np.ascontiguousarray(big.transpose(2, 0, 1)), np.full((1, 1, 3), 200, np.uint8)]
    assert 301 * 517 > 18 * L.IMAGE_ENTROPY_CHUNK and (301 * 517) % 16 == 1
    for normalize in (True, False):
        got = run_images(imgs, normalize)
        want = np.asarray([ER.spatial_entropy_ref(im, normalize) for im in imgs])
        print(f"many chunks (normalize={normalize}): {np.abs(got - want).max():.2e} from the restatement")
        assert np.abs(got - want).max() <= TOL_SPATIAL
        assert abs(got[0] - got[4]) <= TOL_SPATIAL                                                   # interleaved and planar: one image
        assert run_images(imgs[:1], normalize).tobytes() == got[:1].tobytes()
        assert run_images(imgs[::-1], normalize)[::-1].tobytes() == got.tobytes()                    # any batch: the same bytes
    # images that do not start on a 16-byte boundary take the narrow loads and are still right
    got = run_images(imgs, True, shift=1)
    assert np.abs(got - np.asarray([ER.spatial_entropy_ref(im) for im in imgs])).max() <= TOL_SPATIAL


def test_image_entry_point_skips_what_it_cannot_serve():
    imgs = [image("grey_64x64"), image("focused_224"), image("rgb_37x53")]
    whole = run_images(imgs)
    got = run_images(imgs, max_pix=64 * 64)                                                          # the 224 x 224 image is beyond max_pix
    assert got[1] == SENTINEL and got[[0, 2]].tobytes() == whole[[0, 2]].tobytes()
    got = run_images(imgs, layouts=[0, 1, 7])                                                        # a layout outside {0, 1, 2}
    assert got[2] == SENTINEL and got[[0, 1]].tobytes() == whole[[0, 1]].tobytes()


def test_spatial_entropy_call(monkeypatch):
    imgs = [image(n) for n in U8_NAMES]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = E.spatial_entropy(imgs, device=DEV)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (len(imgs),)
    got = out.cpu().numpy()
    assert np.abs(got - np.asarray([image_entropy(n) for n in U8_NAMES])).max() <= TOL_SPATIAL
    assert got.tobytes() == run_images(imgs).tobytes()
    raw_ = E.spatial_entropy(imgs, normalize_input=False, device=DEV).cpu().numpy()
    assert np.abs(raw_ - np.asarray([image_entropy(n, False) for n in U8_NAMES])).max() <= TOL_SPATIAL
    f64 = E.spatial_entropy([image("f64_50x60x3")], device=DEV).cpu().numpy()
    assert abs(f64[0] - image_entropy("f64_50x60x3")) <= TOL_SPATIAL
    monkeypatch.setattr(E, "ENTROPY_BATCH_BYTES", 1)                     # every image its own batch
    assert E.spatial_entropy(imgs, device=DEV).cpu().numpy().tobytes() == got.tobytes()


# ---------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------
def read_csv(path):
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    return rows[0], rows[1:]


def test_command_line_writes_the_scripts_files(tmp_path, caplog):
    from PIL import Image
    eeg, gaze, out = tmp_path / "eeg", tmp_path / "gaze", tmp_path / "out"
    eeg.mkdir(), gaze.mkdir()
    # a channel's entropy does not depend on the other channels: 32-channel files tiled from the fixture's two-channel trials
    trials = [("Pair-12-Comp-EYE_trial1_playerA", "len777", "rgb_37x53"), ("Pair-12-Coop-EYE_trial2_playerB", "len384", "grey_64x64"),
              ("Pair-12-A-Single-EYE_trial3_player", "len257", "focused_224")]
    for stem, rec, img in trials:
        np.savetxt(eeg / f"{stem}.csv", np.tile(raw(rec), (16, 1)), delimiter=",", fmt="%.9e")
        Image.fromarray(image(img)).save(gaze / f"{stem}.png")
    Image.fromarray(np.zeros((10, 12, 4), np.uint8)).save(gaze / "Pair-13-Comp-EYE_trial1_playerA.png")
    np.savetxt(eeg / "Pair-13-Comp-EYE_trial1_playerA.csv", np.tile(raw("len777"), (16, 1))[:31], delimiter=",", fmt="%.9e")
    np.savetxt(eeg / "Pair-13-Coop-EYE_trial1_playerA.csv", np.tile(raw("len256"), (16, 1))[:, :200], delimiter=",", fmt="%.9e")
    np.savetxt(eeg / "notes.csv", np.zeros((2, 2)), delimiter=",")
    with caplog.at_level(logging.WARNING):
        assert E.main(["--modality", "both", "--eeg-path", str(eeg), "--gaze-path", str(gaze), "--output-dir", str(out)]) == 0
    skipped = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING and r.name == E.log.name]
    assert len(skipped) == 3, skipped
    assert any("Pair-13-Comp-EYE_trial1_playerA.png" in m and "Expected 3 channels, got 4" in m for m in skipped)
    assert any("Pair-13-Comp-EYE_trial1_playerA.csv has 31 channels, expected 32" in m for m in skipped)
    assert any("Pair-13-Coop-EYE_trial1_playerA.csv" in m and "200 samples" in m for m in skipped)
    assert sorted(p.name for p in out.iterdir()) == ["cross_modality_entropy.csv", "eeg_entropy_raw_corrected.csv", "eeg_entropy_summary.csv",
                                                     "gaze_entropy_raw.csv", "gaze_entropy_summary.csv"]
    by_name = sorted(trials)                                             # files are taken in the order of their names
    head, body = read_csv(out / "gaze_entropy_raw.csv")
    assert head == ["pair_id", "player", "trial_idx", "condition", "spatial_entropy"] and len(body) == 3
    for b, (stem, _, img) in zip(body, by_name):
        meta = E.parse_eeg_filename(stem + ".csv")
        assert b[:4] == [str(meta["pair_id"]), meta["player"], str(meta["trial_idx"]), meta["condition"]]
        assert abs(float(b[4]) - image_entropy(img)) <= TOL_SPATIAL
    head, body = read_csv(out / "eeg_entropy_raw_corrected.csv")
    assert head == ["pair_id", "player", "trial_idx", "condition", "mean_entropy", *E.STANDARD_32_CHANNELS] and len(body) == 3
    for b, (stem, rec, _) in zip(body, by_name):
        meta = E.parse_eeg_filename(stem + ".csv")
        assert b[:4] == [str(meta["pair_id"]), meta["player"], str(meta["trial_idx"]), meta["condition"]]
        want = np.tile(reference_entropy(rec), 16)
        assert np.abs(np.asarray(b[5:], np.float64) - want).max() <= TOL_SPECTRAL
        assert abs(float(b[4]) - want.mean()) <= TOL_SPECTRAL
    for name in ("gaze_entropy_summary.csv", "eeg_entropy_summary.csv"):
        head, body = read_csv(out / name)
        assert head == ["pair_id", "player", "condition", "mean", "std", "min", "max", "n_trials"]
        assert [b[:3] for b in body] == [["12", "A_player", "Single"], ["12", "playerA", "Competition"], ["12", "playerB", "Cooperation"]]
        assert all(b[4] == "" and b[7] == "1" for b in body)                                         # one trial each: the std is NaN
    head, body = read_csv(out / "cross_modality_entropy.csv")
    assert head == ["pair_id", "player", "trial_idx", "condition", "gaze_entropy", "eeg_entropy"] and len(body) == 3
    # one modality alone
    assert E.main(["--modality", "gaze", "--gaze-path", str(gaze), "--output-dir", str(tmp_path / "gaze_only")]) == 0
    assert sorted(p.name for p in (tmp_path / "gaze_only").iterdir()) == ["gaze_entropy_raw.csv", "gaze_entropy_summary.csv"]
