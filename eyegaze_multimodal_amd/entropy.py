"""Entropy analysis on the device: what the reference's 7_Analysis/python_scripts/analyze_entropy.py computes with
5_Metrics/entropy_calculators.py -- the spectral entropy of every EEG channel of a trial, the spatial entropy of every gaze
heat-map image, per-subject summaries and the gaze / EEG merge -- each modality as ONE ragged call with one host sync.

    python -m eyegaze_multimodal_amd.entropy --modality gaze|eeg|both [--eeg-path DIR] [--gaze-path DIR] --output-dir OUT

writes the script's CSV files.  There is no CPU path for the entropies: eg_recording_filtfilt_exact, eg_trial_spectral_entropy and
eg_image_entropy of libeyegaze_hip.so compute them; summaries and the merge are a few thousand doubles in numpy on the host."""
from __future__ import annotations

import argparse
import csv
import ctypes
import logging
import math
import re
import sys
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .filters import butter_bandpass, lfilter_zi

# the 32 electrode names of the raw EEG table, in the reference's order (entropy_calculators.py:468-473)
STANDARD_32_CHANNELS = ["Fp1", "Fz", "F3", "F7", "FT9", "FC5", "FC1", "C3", "T7", "TP9", "CP5", "CP1", "Pz", "P3", "P7", "O1",
                        "Oz", "O2", "P4", "P8", "TP10", "CP6", "CP2", "Cz", "C4", "T8", "FT10", "FC6", "FC2", "F4", "F8", "Fp2"]
MERGE_KEYS = ("pair_id", "player", "trial_idx", "condition")
EPS = 1e-10                             # _normalize_to_probability's eps (:45), absolute
MIN_LEN, MAX_LEN = 256, 65536           # EG_TRIAL_MIN_LEN, EG_TRIAL_MAX_LEN
NPERSEG = 256
MAX_PIX = 1 << 24                       # eg_image_entropy's largest image
ENTROPY_BATCH_BYTES = 1 << 30           # device bytes (inputs, workspaces) per batch of either call
GREY, INTERLEAVED, PLANAR = 0, 1, 2     # eg_image_batch_desc's layouts

log = logging.getLogger(__name__)


def entropy_band_coefficients(low_hz: float, high_hz: float, fs: float, order: int = 4):
    """(b, a) of SpectralEntropyCalculator._design_bandpass_filter (:267-276): butter(order, [max(low / nyq, 0.001),
    min(high / nyq, 0.999)], 'band').  The lower clamp is handed over as the frequency that divides back to 0.001 exactly
    (features.band_coefficients' way), the upper one is filters.butter_bandpass' high_clamp."""
    nyq = fs / 2
    if low_hz / nyq < 0.001:
        low_hz = 0.001 * nyq
        for cand in (low_hz, np.nextafter(low_hz, np.inf), np.nextafter(low_hz, -np.inf)):
            if cand / nyq == 0.001:
                low_hz = float(cand)
                break
    return butter_bandpass(order, low_hz, high_hz, fs, high_clamp=0.999)


def _upload(host: torch.Tensor, dev) -> torch.Tensor:
    """host -> device without a host sync: through pinned memory, asynchronously on the current stream"""
    if dev.type != "cuda":
        return host.to(dev)
    return host.pin_memory().to(dev, non_blocking=True)


def _dbl(v):
    return (ctypes.c_double * len(v))(*[float(x) for x in v])


# ---------------------------------------------------------------------------------------------------------------
# spectral entropy
# ---------------------------------------------------------------------------------------------------------------
def _as_recording(r, i: int) -> torch.Tensor:
    t = r.detach().to(torch.float32) if torch.is_tensor(r) else torch.from_numpy(np.ascontiguousarray(r, dtype=np.float32))
    if t.dim() != 2 or t.shape[0] < 1:
        raise ValueError(f"spectral_entropy needs (C, L) recordings, recording {i} is {tuple(t.shape)}")
    if not MIN_LEN <= int(t.shape[1]) <= MAX_LEN:
        raise ValueError(f"spectral_entropy: recording {i} has {int(t.shape[1])} samples, served are {MIN_LEN} to {MAX_LEN}")
    return t.contiguous()


def _spectral_batch(recs: List[torch.Tensor], fs: float, coef, dev) -> List[torch.Tensor]:
    """one batch on the current stream of `dev`, no host sync: every channel is a row, so the descriptor's C is 1"""
    from . import _lib as L
    from .data import recording_row_tables, validate_recording_rows
    lengths = [int(r.shape[1]) for r in recs for _ in range(int(r.shape[0]))]
    pad = 3 * len(coef[0]) if coef else 0
    row_off, row_len, ws_off, floats, ws_need = recording_row_tables(lengths, 1, pad)
    validate_recording_rows(row_off, row_len, 1, pad, floats)
    if all(r.device.type == "cpu" for r in recs):
        data = _upload(torch.cat([r.reshape(-1) for r in recs]), dev)                   # joined on the host: ONE upload
    else:                                                                               # device recordings are joined on the device
        data = torch.cat([(_upload(r, dev) if r.device.type == "cpu" else r.to(dev)).reshape(-1) for r in recs])
    tabs = np.concatenate([row_off, ws_off, row_len.astype(np.int64)])                 # the three tables travel as one
    t_tabs = _upload(torch.from_numpy(tabs), dev)
    n = len(lengths)
    t_off, t_ws, t_len = t_tabs[:n], t_tabs[n:2 * n], t_tabs[2 * n:].to(torch.int32)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    desc = L.RecordingRowsDesc(L.ptr(data), L.ptr(t_off), L.ptr(t_len), L.ptr(t_ws), n, 1, max(lengths), 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if coef:
        b, a = coef
        ws = torch.empty(ws_need, dtype=torch.float64, device=dev)
        L.call("eg_recording_filtfilt_exact", ctypes.byref(desc), _dbl(b), _dbl(a), _dbl(lfilter_zi(b, a)), len(b), L.ptr(ws), ws_need,
               int(ws.numel()), stream)
    L.call("eg_trial_spectral_entropy", ctypes.byref(desc), float(fs), EPS, 0, L.ptr(out), stream)
    res, at = [], 0
    for r in recs:
        res.append(out[at:at + int(r.shape[0])])
        at += int(r.shape[0])
    return res


def spectral_entropy(recordings, sampling_rate: float = 250.0, filter_low: float = 0.5, filter_high: float = 50.0, filter_order: int = 4,
                     apply_filter: bool = True, device="cuda", nperseg: int = NPERSEG) -> List[torch.Tensor]:
    """SpectralEntropyCalculator.compute (:346-381) for every recording of `recordings` -- (C_i, L_i) float32 arrays or tensors,
    lengths AND channel counts ragged -- as a list of float64 device tensors (C_i,), in bits: zero-phase Butterworth band-pass
    with the calculator's coefficients (eg_recording_filtfilt_exact, scipy's bits), Welch PSD, Shannon entropy of the PSD
    (eg_trial_spectral_entropy).  No common-average reference and no z-score: the calculator has neither.  Recordings run in
    batches of at most ENTROPY_BATCH_BYTES device bytes on the current stream; the function does not sync -- the copy-back of
    the results is the caller's one sync.  A NaN or Inf in a channel makes that channel's entropy NaN.
    ValueError: a recording that is not (C, L), L outside [256, 65536] (below 256 the reference shortens the segment, at
    L <= 128 it raises; neither is restated), nperseg != 256, an order with more than 17 coefficients, a bad band."""
    from . import _lib as L
    if nperseg != NPERSEG:
        raise ValueError(f"spectral_entropy: nperseg = {nperseg}, served is {NPERSEG} alone")
    fs = float(sampling_rate)
    coef = entropy_band_coefficients(filter_low, filter_high, fs, filter_order) if apply_filter else None
    recs = [_as_recording(r, i) for i, r in enumerate(recordings)]
    if not recs:
        return []
    L.lib()
    dev = torch.device(device)
    ncoef = len(coef[0]) if coef else 0
    cost = lambda r: int(r.shape[0]) * (4 * int(r.shape[1]) + 8 * (int(r.shape[1]) + 6 * ncoef) + 32)
    out, batch, used = [], [], 0
    for r in recs:
        if batch and used + cost(r) > ENTROPY_BATCH_BYTES:
            out += _spectral_batch(batch, fs, coef, dev)
            batch, used = [], 0
        batch.append(r)
        used += cost(r)
    return out + _spectral_batch(batch, fs, coef, dev)


# ---------------------------------------------------------------------------------------------------------------
# spatial entropy
# ---------------------------------------------------------------------------------------------------------------
def image_layout(shape) -> int:
    """_to_grayscale's rule in its order (:125-143): 2-D is grey; 3-D with shape[0] == 3 is channel-first -- also a (3, W, 3)
    array, which the reference transposes; otherwise shape[2] == 3 is pixel-interleaved; anything else raises its text"""
    if len(shape) == 2:
        return GREY
    if len(shape) == 3:
        if shape[0] == 3:                               # transposed to (H, W, 3): its last axis is always 3
            return PLANAR
        if shape[2] == 3:
            return INTERLEAVED
        raise ValueError(f"Expected 3 channels, got {shape[2]}")
    raise ValueError(f"Expected 2D or 3D array, got {len(shape)}D")


def _spatial_batch(images: List[np.ndarray], layouts: List[int], elem: int, normalize: bool, dev, out: torch.Tensor) -> None:
    from . import _lib as L
    align = 16 if elem == 0 else 2                      # elements per 16 bytes
    npix = [im.size // (1 if lay == GREY else 3) for im, lay in zip(images, layouts)]
    off, at = [], 0
    for im in images:
        off.append(at)
        at += -(-im.size // align) * align
    host = np.zeros(at, dtype=np.uint8 if elem == 0 else np.float64)
    for im, o in zip(images, off):
        host[o:o + im.size] = im.reshape(-1)
    data = _upload(torch.from_numpy(host), dev)                                        # ONE upload
    n, max_pix = len(images), max(npix)
    tabs = _upload(torch.from_numpy(np.concatenate([np.asarray(off, np.int64), np.asarray(npix, np.int64), np.asarray(layouts, np.int64)])), dev)
    t_off, t_npix, t_lay = tabs[:n], tabs[n:2 * n].to(torch.int32), tabs[2 * n:].to(torch.int32)
    need = L.image_entropy_workspace_doubles(n, max_pix)
    ws = torch.empty(need, dtype=torch.float64, device=dev)
    desc = L.ImageBatchDesc(L.ptr(data), L.ptr(t_off), L.ptr(t_npix), L.ptr(t_lay), n, max_pix, elem, int(bool(normalize)))
    L.call("eg_image_entropy", ctypes.byref(desc), EPS, L.ptr(ws), need, L.ptr(out), torch.cuda.current_stream(dev).cuda_stream)


def spatial_entropy(images, normalize_input: bool = True, device="cuda") -> torch.Tensor:
    """SpatialEntropyCalculator.compute (:145-180) for every image of `images` -- numpy arrays, uint8 or float64, one dtype per
    call, any sizes: (H, W) grey, (3, H, W) channel-first or (H, W, 3) RGB by the reference's rule (image_layout) -- as one
    float64 device tensor (N,), in bits.  One join, one upload and one eg_image_entropy call per batch of at most
    ENTROPY_BATCH_BYTES device bytes; the function does not sync.
    ValueError: the reference's own refusals with its text (an RGBA image has 4 channels), mixed or other dtypes -- float32
    among them: the reference computes a float32 image entirely in float32 with numpy's pairwise sums, which is not restated --
    an empty image or one beyond 2^24 pixels."""
    from . import _lib as L
    arrs = [np.asarray(im) for im in images]
    if not arrs:
        return torch.empty(0, dtype=torch.float64, device=device)
    dtypes = {a.dtype for a in arrs}
    if np.dtype(np.float32) in dtypes:
        raise ValueError("spatial_entropy: float32 images are not served: the reference computes them entirely in float32 with numpy's "
                         "pairwise sums, which is not restated; pass uint8 or float64")
    if len(dtypes) != 1 or next(iter(dtypes)) not in (np.dtype(np.uint8), np.dtype(np.float64)):
        raise ValueError(f"spatial_entropy: images must share one dtype, uint8 or float64, got {sorted(str(d) for d in dtypes)}")
    elem = 0 if arrs[0].dtype == np.uint8 else 1
    layouts = [image_layout(a.shape) for a in arrs]
    for i, (a, lay) in enumerate(zip(arrs, layouts)):
        n = a.size // (1 if lay == GREY else 3)
        if not 1 <= n <= MAX_PIX:
            raise ValueError(f"spatial_entropy: image {i} has {n} pixels, served are 1 to {MAX_PIX}")
    arrs = [np.ascontiguousarray(a) for a in arrs]
    L.lib()
    dev = torch.device(device)
    out = torch.empty(len(arrs), dtype=torch.float64, device=dev)
    chunk, size = L.IMAGE_ENTROPY_CHUNK, arrs[0].dtype.itemsize
    # a batch's device bytes: the padded images, 24 of tables and 8 of output per image, 32 of workspace per image and chunk of
    # the batch's largest image
    first, data, biggest = 0, 0, 0
    for i, a in enumerate(arrs):
        mine, chunks = a.size * size + 48, -(-(a.size // (1 if layouts[i] == GREY else 3)) // chunk)
        if i > first and data + mine + 32 * (i - first + 1) * max(biggest, chunks) > ENTROPY_BATCH_BYTES:
            _spatial_batch(arrs[first:i], layouts[first:i], elem, normalize_input, dev, out[first:i])
            first, data, biggest = i, 0, 0
        data, biggest = data + mine, max(biggest, chunks)
    _spatial_batch(arrs[first:], layouts[first:], elem, normalize_input, dev, out[first:])
    return out


# ---------------------------------------------------------------------------------------------------------------
# summaries and the merge: numpy on the host, from the arrays that were copied back once
# ---------------------------------------------------------------------------------------------------------------
def summary_statistics(rows: Sequence[Dict], value_col: str, group_cols=("pair_id", "player", "condition")) -> List[Dict]:
    """compute_summary_statistics (analyze_entropy.py:537-570): per group of `group_cols`, in sorted key order, mean, sample std
    (ddof = 1: NaN for one trial), min, max and n_trials of `value_col`; NaN values are left out, as pandas leaves them out"""
    groups: Dict[tuple, List[float]] = {}
    for r in rows:
        groups.setdefault(tuple(r[c] for c in group_cols), []).append(float(r[value_col]))
    out = []
    for key in sorted(groups):
        v = np.asarray(groups[key], np.float64)
        v = v[~np.isnan(v)]
        n = len(v)
        rec = dict(zip(group_cols, key))
        rec.update({"mean": float(v.mean()) if n else math.nan, "std": float(v.std(ddof=1)) if n > 1 else math.nan,
                    "min": float(v.min()) if n else math.nan, "max": float(v.max()) if n else math.nan, "n_trials": n})
        out.append(rec)
    return out


def cross_modality(gaze_rows: Sequence[Dict], eeg_rows: Sequence[Dict]) -> List[Dict]:
    """the script's inner merge on pair_id, player, trial_idx, condition (:773-791), in the gaze rows' order, the columns renamed
    gaze_entropy and eeg_entropy"""
    by_key: Dict[tuple, List[Dict]] = {}
    for r in eeg_rows:
        by_key.setdefault(tuple(r[k] for k in MERGE_KEYS), []).append(r)
    out = []
    for g in gaze_rows:
        key = tuple(g[k] for k in MERGE_KEYS)
        for e in by_key.get(key, ()):
            rec = dict(zip(MERGE_KEYS, key))
            rec.update({"gaze_entropy": g["spatial_entropy"], "eeg_entropy": e["mean_entropy"]})
            out.append(rec)
    return out


# ---------------------------------------------------------------------------------------------------------------
# the script's files
# ---------------------------------------------------------------------------------------------------------------
_SINGLE = re.compile(r"Pair-(\d+)-([AB])-Single-EYE_trial(\d+)_(player|observer)\.csv")
_DUAL = {"Competition": re.compile(r"Pair-(\d+)-Comp-EYE_trial(\d+)_(playerA|playerB)\.csv"),
         "Cooperation": re.compile(r"Pair-(\d+)-Coop-EYE_trial(\d+)_(playerA|playerB)\.csv")}


def parse_eeg_filename(filename: str) -> Optional[Dict]:
    """{pair_id, condition, trial_idx, player} of the script's three file name patterns (:110-162), None for any other name;
    like the script's re.match, anchored at the start only"""
    m = _SINGLE.match(filename)
    if m:
        pair_id, ab, trial_idx, role = m.groups()
        return {"pair_id": int(pair_id), "condition": "Single", "trial_idx": int(trial_idx), "player": f"{ab}_{role}"}
    for condition, pattern in _DUAL.items():
        m = pattern.match(filename)
        if m:
            pair_id, trial_idx, player = m.groups()
            return {"pair_id": int(pair_id), "condition": condition, "trial_idx": int(trial_idx), "player": player}
    return None


def parse_gaze_filename(filename: str) -> Optional[Dict]:
    """the same patterns with a .jpg or .png extension (:165-179)"""
    return parse_eeg_filename(filename.replace(".jpg", ".csv").replace(".png", ".csv"))


def _scan(directory, patterns, parse, what) -> List[Dict]:
    path = Path(directory)
    if not path.exists():
        raise FileNotFoundError(f"{what} directory not found: {directory}")
    files = []
    for f in sorted((f for p in patterns for f in path.glob(p)), key=lambda f: f.name):
        meta = parse(f.name)
        if meta is not None:
            files.append({**meta, "filepath": str(f), "filename": f.name})
    return files


def scan_eeg_files(eeg_dir) -> List[Dict]:
    return _scan(eeg_dir, ("*.csv",), parse_eeg_filename, "EEG")


def scan_gaze_files(gaze_dir) -> List[Dict]:
    return _scan(gaze_dir, ("*.jpg", "*.png"), parse_gaze_filename, "Gaze")


def load_gaze_image(path) -> np.ndarray:
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("the gaze heat maps load through Pillow (PIL), which is not installed") from e
    with Image.open(path) as img:
        return np.array(img)


def gaze_entropy_rows(files: Sequence[Dict], device="cuda") -> List[Dict]:
    """analyze_gaze_entropy (:409-461): the raw gaze table's rows.  A file that cannot be served (an RGBA or 16-bit image) is
    logged and left out while the run goes on; the rest is one spatial_entropy call and one copy-back."""
    kept, images = [], []
    for f in files:
        try:
            img = load_gaze_image(f["filepath"])
            if img.dtype != np.uint8:
                raise ValueError(f"pixels of type {img.dtype}, served is uint8")
            image_layout(img.shape)
        except (ValueError, OSError) as e:
            log.warning("Error processing %s: %s", f["filename"], e)
            continue
        kept.append(f)
        images.append(img)
    if not kept:
        return []
    values = spatial_entropy(images, device=device).cpu().numpy()                      # the one sync
    return [{"pair_id": f["pair_id"], "player": f["player"], "trial_idx": f["trial_idx"], "condition": f["condition"],
             "spatial_entropy": float(v)} for f, v in zip(kept, values)]


def eeg_entropy_rows(files: Sequence[Dict], sampling_rate: float = 250.0, filter_low: float = 0.5, filter_high: float = 50.0,
                     n_channels: int = 32, device="cuda") -> List[Dict]:
    """analyze_eeg_entropy (:464-534): the raw EEG table's rows -- mean_entropy, then one column per channel under the names of
    STANDARD_32_CHANNELS.  A file whose channel count is not `n_channels` or whose length is not served is logged and left out."""
    from .data import load_recording
    kept, recs = [], []
    for f in files:
        rec, _ = load_recording(f["filepath"])
        if rec.shape[0] != n_channels:
            log.warning("Warning: %s has %d channels, expected %d", f["filename"], rec.shape[0], n_channels)
            continue
        if not MIN_LEN <= rec.shape[1] <= MAX_LEN:
            log.warning("Error processing %s: %d samples, served are %d to %d", f["filename"], rec.shape[1], MIN_LEN, MAX_LEN)
            continue
        kept.append(f)
        recs.append(rec)
    if not kept:
        return []
    out = spectral_entropy(recs, sampling_rate, filter_low, filter_high, device=device)
    values = torch.cat(out).cpu().numpy().reshape(len(kept), n_channels)               # the one sync
    rows = []
    for f, v in zip(kept, values):
        row = {"pair_id": f["pair_id"], "player": f["player"], "trial_idx": f["trial_idx"], "condition": f["condition"],
               "mean_entropy": float(v.mean())}
        row.update({name: float(x) for name, x in zip(STANDARD_32_CHANNELS, v)})
        rows.append(row)
    return rows


def _cell(v) -> str:
    if isinstance(v, (float, np.floating)):
        return "" if math.isnan(v) else repr(float(v))
    return str(v)


def write_csv(path, rows: Sequence[Dict], columns: Sequence[str]) -> None:
    """pandas' to_csv(index=False) of such a table: a header, shortest round-trip floats, an empty cell for NaN"""
    with open(path, "w", newline="", encoding="utf-8") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow(columns)
        for r in rows:
            w.writerow([_cell(r[c]) for c in columns])


SUMMARY_COLUMNS = ["pair_id", "player", "condition", "mean", "std", "min", "max", "n_trials"]


def write_results(output_dir, gaze_rows: Optional[Sequence[Dict]] = None, eeg_rows: Optional[Sequence[Dict]] = None) -> List[str]:
    """the script's step 2 and its merged table (:635-661, :803-806), file names and column orders as there; returns the names
    written.  An empty table writes nothing, as there."""
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    written = []

    def put(name, rows, columns):
        write_csv(out / name, rows, columns)
        written.append(name)

    if gaze_rows:
        put("gaze_entropy_raw.csv", gaze_rows, [*MERGE_KEYS, "spatial_entropy"])
        put("gaze_entropy_summary.csv", summary_statistics(gaze_rows, "spatial_entropy"), SUMMARY_COLUMNS)
    if eeg_rows:
        channels = [c for c in STANDARD_32_CHANNELS if c in eeg_rows[0]]
        put("eeg_entropy_raw_corrected.csv", eeg_rows, [*MERGE_KEYS, "mean_entropy", *channels])
        put("eeg_entropy_summary.csv", summary_statistics(eeg_rows, "mean_entropy"), SUMMARY_COLUMNS)
    if gaze_rows and eeg_rows:
        merged = cross_modality(gaze_rows, eeg_rows)
        if merged:
            put("cross_modality_entropy.csv", merged, [*MERGE_KEYS, "gaze_entropy", "eeg_entropy"])
    return written


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="Entropy analysis on the device (analyze_entropy.py's CSV outputs)")
    ap.add_argument("--modality", required=True, choices=["gaze", "eeg", "both"])
    ap.add_argument("--eeg-path", help="directory of the Pair-*-EYE_trial*_*.csv recordings")
    ap.add_argument("--gaze-path", help="directory of the heat maps under the same names, .jpg or .png")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--sampling-rate", type=float, default=250.0)
    ap.add_argument("--filter-low", type=float, default=0.5)
    ap.add_argument("--filter-high", type=float, default=50.0)
    ap.add_argument("--n-channels", type=int, default=32)
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    gaze_rows = eeg_rows = None
    if args.modality in ("gaze", "both"):
        if not args.gaze_path:
            ap.error("--gaze-path is required for this modality")
        files = scan_gaze_files(args.gaze_path)
        log.info("Found %d Gaze image files", len(files))
        gaze_rows = gaze_entropy_rows(files, args.device)
        log.info("Computed entropy for %d Gaze trials", len(gaze_rows))
    if args.modality in ("eeg", "both"):
        if not args.eeg_path:
            ap.error("--eeg-path is required for this modality")
        files = scan_eeg_files(args.eeg_path)
        log.info("Found %d EEG CSV files", len(files))
        eeg_rows = eeg_entropy_rows(files, args.sampling_rate, args.filter_low, args.filter_high, args.n_channels, args.device)
        log.info("Computed entropy for %d EEG trials", len(eeg_rows))
    for name in write_results(args.output_dir, gaze_rows, eeg_rows):
        log.info("Saved: %s", Path(args.output_dir) / name)
    return 0


if __name__ == "__main__":
    sys.exit(main())
