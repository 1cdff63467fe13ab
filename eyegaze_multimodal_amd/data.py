"""Synthetic window generators for throughput and accuracy runs.  Real EEG CSVs are absent
from the reference tree; the reference's own synthesiser is 1_Data/processed/two_EEG_fusion.py:31-49
(sine mixture + Gaussian noise).  `synth_windows` restates that recipe and makes it class-conditional so that
validation accuracy is learnable: stream 2 shares a class-dependent fraction of stream 1's components."""
from __future__ import annotations

import numpy as np
import torch


def zscore_window(x: np.ndarray) -> np.ndarray:
    """per-window global z-score, population std (1_Data/processed/dual_eeg_dataset.py:201-202)"""
    return ((x - x.mean()) / (x.std() + 1e-8)).astype(np.float32)


def _sines(rng, C, T, fs, ncomp):
    t = np.arange(T, dtype=np.float32) / fs
    f = rng.uniform(1.0, 40.0, size=(C, ncomp, 1)).astype(np.float32)
    a = rng.uniform(0.1, 1.0, size=(C, ncomp, 1)).astype(np.float32)
    p = rng.uniform(0.0, 2 * np.pi, size=(C, ncomp, 1)).astype(np.float32)
    return (a * np.sin(2 * np.pi * f * t + p)).sum(1).astype(np.float32)


def synth_windows(n: int, C: int = 8, T: int = 1024, num_classes: int = 3, fs: float = 256.0, noise_std: float = 0.1,
                  seed: int = 0):
    """Returns eeg1, eeg2 [n,C,T] f32 (z-scored per window) and labels [n] i64.
    class c: stream 2 = coupling[c] * (stream 1 delayed by lag[c]) + (1-coupling[c]) * independent mixture, and both
    streams carry a class-specific rhythm (6 / 11 / 20 / 31 / 43 Hz, random phase per window) on half of the channels."""
    rng = np.random.default_rng(seed)
    coupling = np.linspace(0.0, 0.9, num_classes)
    lags = [0, 7, 19, 3, 11][:num_classes]
    marker = [6.0, 11.0, 20.0, 31.0, 43.0][:num_classes]
    tt = np.arange(T, dtype=np.float32) / fs
    x1 = np.zeros((n, C, T), np.float32)
    x2 = np.zeros((n, C, T), np.float32)
    y = rng.integers(0, num_classes, size=n)
    for i in range(n):
        a = _sines(rng, C, T, fs, 3) + rng.normal(0, noise_std, (C, T)).astype(np.float32)
        b = _sines(rng, C, T, fs, 3) + rng.normal(0, noise_std, (C, T)).astype(np.float32)
        c = int(y[i])
        m = (0.8 * np.sin(2 * np.pi * marker[c] * tt + rng.uniform(0, 2 * np.pi))).astype(np.float32)
        a[::2] += m
        b[1::2] += m
        x1[i] = zscore_window(a)
        x2[i] = zscore_window(coupling[c] * np.roll(a, lags[c], axis=1) + (1 - coupling[c]) * b)
    return torch.from_numpy(x1), torch.from_numpy(x2), torch.from_numpy(y.astype(np.int64))


def randn_windows(B: int, C: int, T: int, seed: int, num_classes: int = 3, device="cpu"):
    """Throughput-run batch: randn(seed) + per-window z-score, labels cyclic."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, B, C, T, generator=g)
    x = (x - x.mean(dim=(2, 3), keepdim=True)) / (x.std(dim=(2, 3), unbiased=False, keepdim=True) + 1e-8)
    labels = torch.arange(B) % num_classes
    return x[0].contiguous().to(device), x[1].contiguous().to(device), labels.to(device)


# ------------------------------------------------------------------------------------------------------
# Windowed shards.  The reference's DualEEGDataset re-reads BOTH full CSV recordings for every
# window it returns (1_Data/processed/dual_eeg_dataset.py:176-183); here each recording is read once, cut into the
# same windows (same enumeration order as `_prepare_windows`, :62-120) and stored raw as `[n, 2, C, T]` f32 `.npy`
# shards.  Batches are gathered from memory-mapped shards into pinned staging memory, copied to the device on a
# side stream, and normalised there by `eg_window_normalize` (the reference normalises on the host, :194-202).
# ------------------------------------------------------------------------------------------------------
import json  # noqa: E402
from pathlib import Path  # noqa: E402
from typing import Dict, Iterable, List, Optional, Sequence  # noqa: E402


def orient_recording(eeg: np.ndarray):
    """file contents -> ((C, T) f32, columns in the file).  Rows are channels unless there are more rows than columns
    (dual_eeg_dataset.py:132-139).  The column count AS STORED is what the reference's window enumeration uses
    (:86-92 reads one row and takes its width), so a transposed file yields no windows there — kept."""
    ncols = int(eeg.shape[1])
    if eeg.shape[0] > eeg.shape[1]:
        eeg = eeg.T
    return np.ascontiguousarray(eeg, dtype=np.float32), ncols


def load_recording(path):
    import pandas as pd
    return orient_recording(pd.read_csv(path, header=None).values)


def kept_pairs(items: Sequence[Dict], eeg_base_path, window_size: int, stride: int,
               recordings: Optional[Dict[str, np.ndarray]] = None):
    """The reference's window enumeration (`_prepare_windows`, dual_eeg_dataset.py:62-120), pair by pair: yields
    (idx, item, a, b, nwin) for every item of `items` that has windows -- a, b the two (C, len) recordings with the channels
    truncated to the pair's minimum, nwin = (min_len - W) // stride + 1 windows starting at i * stride.  Items with a missing
    file or `min_len < W` are skipped (min_len from the column counts as stored, see orient_recording); a pair whose channel
    count differs from the earlier ones raises ValueError.  Both the shard builder and the recording store walk this."""
    base = Path(eeg_base_path) if eeg_base_path is not None else None
    cache: Dict[str, np.ndarray] = {}

    def get(name):
        if recordings is not None:
            return orient_recording(recordings[name]) if name in recordings else None
        if name not in cache:
            p = base / f"{name}.csv"
            cache[name] = load_recording(p) if p.exists() else None
        return cache[name]

    C_all = None
    for idx, item in enumerate(items):
        ra, rb = get(item["player1"]), get(item["player2"])
        if ra is None or rb is None:
            continue
        (a, na), (b, nb_) = ra, rb
        min_len = min(na, nb_)
        if min_len < window_size:
            continue
        C = min(a.shape[0], b.shape[0])
        if C_all is None:
            C_all = C
        elif C != C_all:
            raise ValueError(f"item {idx}: {C} channels, earlier items have {C_all}")
        yield idx, item, a[:C], b[:C], (min_len - window_size) // stride + 1
        if recordings is None:
            cache.clear()


def _window_meta(idx: int, item: Dict, s: int, e: int) -> Dict:
    return {"dataset_idx": idx, "start": s, "end": e, "player1": item["player1"], "player2": item["player2"], "class": item["class"]}


def build_window_shards(items: Sequence[Dict], eeg_base_path, label2id: Dict[str, int], out_dir, window_size: int = 1024,
                        stride: int = 256, shard_windows: int = 4096, recordings: Optional[Dict[str, np.ndarray]] = None) -> Dict:
    """Cut every (player1, player2) pair of `items` into sliding windows and write shards + index.

    items        sequence of {'player1': name, 'player2': name, 'class': label} (the reference's metadata rows)
    recordings   optional name -> 2-D array holding a file's contents, instead of `<eeg_base_path>/<name>.csv`
    Window enumeration = the reference's (kept_pairs): per item in order, `(min_len - W) // stride + 1` windows starting at
    `i * stride`, items with a missing file or `min_len < W` skipped; channels truncated to the pair's minimum."""
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    meta: List[Dict] = []
    labels: List[int] = []
    shards: List[Dict] = []
    buf: List[np.ndarray] = []
    C_all = None

    def flush():
        if not buf:
            return
        arr = np.stack(buf)
        name = f"windows_{len(shards):05d}.npy"
        np.save(out / name, arr)
        shards.append({"file": name, "count": int(arr.shape[0])})
        buf.clear()

    for idx, item, a, b, nwin in kept_pairs(items, eeg_base_path, window_size, stride, recordings):
        C_all = a.shape[0]
        for w in range(nwin):
            s, e = w * stride, w * stride + window_size
            buf.append(np.stack([a[:, s:e], b[:, s:e]]))
            meta.append(_window_meta(idx, item, s, e))
            labels.append(int(label2id[item["class"]]))
            if len(buf) == shard_windows:
                flush()
    flush()
    np.save(out / "labels.npy", np.asarray(labels, dtype=np.int64))
    index = {"window_size": window_size, "stride": stride, "channels": C_all, "count": len(meta), "shards": shards,
             "windows": meta, "label2id": label2id}
    (out / "index.json").write_text(json.dumps(index))
    return index


class WindowShards:
    """Per-rank batch iterator over windowed shards; yields dicts shaped like the reference's `collate_fn` output
    (dual_eeg_dataset.py:236-248): {'eeg1','eeg2': f32 [B,C,T] on `device`, 'labels': i64 [B], 'dataset_idx': list}.

    preprocessing=False -> per-window z-score (yaml default, :201-202); True -> CAR + per-channel z-score (:142-168; the
    reference's band-pass step there is a TODO that does nothing).  Rank r of `world` takes indices r::world of each
    epoch's (optionally shuffled) order, as `ddp.shard_indices` does for the synthetic runs."""

    def __init__(self, root, batch_size: int, device, rank: int = 0, world: int = 1, shuffle: bool = False, seed: int = 0,
                 preprocessing: bool = False, drop_last: bool = False):
        from . import _lib as L
        L.lib()  # the normalisation has no CPU fallback
        self.root = Path(root)
        self.index = json.loads((self.root / "index.json").read_text())
        self.labels = torch.from_numpy(np.load(self.root / "labels.npy"))
        self.maps = [np.load(self.root / s["file"], mmap_mode="r") for s in self.index["shards"]]
        counts = np.array([s["count"] for s in self.index["shards"]], dtype=np.int64)
        self.starts = np.concatenate([[0], np.cumsum(counts)])
        self.n, self.C, self.T = int(self.index["count"]), int(self.index["channels"]), int(self.index["window_size"])
        self.B, self.device, self.rank, self.world = batch_size, torch.device(device), rank, world
        self.shuffle, self.seed, self.mode, self.drop_last = shuffle, seed, 1 if preprocessing else 0, drop_last
        self.epoch = 0
        # double-buffered pinned staging + device raw buffers; copies run on their own stream
        self.pinned = [torch.empty(batch_size, 2, self.C, self.T, dtype=torch.float32).pin_memory() for _ in range(2)]
        self.raw = [torch.empty(batch_size, 2, self.C, self.T, dtype=torch.float32, device=self.device) for _ in range(2)]
        self.copy_stream = torch.cuda.Stream(self.device)
        self.copied = [torch.cuda.Event() for _ in range(2)]
        self.consumed = [torch.cuda.Event() for _ in range(2)]

    def set_epoch(self, epoch: int):
        self.epoch = epoch

    def _order(self) -> np.ndarray:
        return epoch_order(self.n, self.shuffle, self.seed, self.epoch, self.rank, self.world)

    def __len__(self):
        if self.drop_last:      # the same count on every rank (a DDP step needs all of them)
            return (self.n // self.world) // self.B
        m = len(range(self.rank, self.n, self.world))
        return (m + self.B - 1) // self.B

    def _gather(self, ids: np.ndarray, slot: int):
        dst = self.pinned[slot].numpy()
        which = np.searchsorted(self.starts, ids, side="right") - 1
        for j, (i, s) in enumerate(zip(ids, which)):
            dst[j] = self.maps[s][i - self.starts[s]]

    def _stage(self, ids: np.ndarray, slot: int):
        self.consumed[slot].synchronize()          # the normalise kernel that last read raw[slot] has finished
        self._gather(ids, slot)
        with torch.cuda.stream(self.copy_stream):
            self.raw[slot][: len(ids)].copy_(self.pinned[slot][: len(ids)], non_blocking=True)
            self.copied[slot].record(self.copy_stream)

    def __iter__(self):
        from ._lib import call, ptr
        order = self._order()
        nb = len(self)
        chunks = [order[i * self.B:(i + 1) * self.B] for i in range(nb)]
        if not chunks:
            return
        self._stage(chunks[0], 0)
        for k, ids in enumerate(chunks):
            slot = k & 1
            if k + 1 < nb:
                self._stage(chunks[k + 1], slot ^ 1)      # host gather + H2D of the next batch overlap this batch's compute
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(self.copied[slot])
            n = len(ids)
            eeg1 = torch.empty(n, self.C, self.T, dtype=torch.float32, device=self.device)
            eeg2 = torch.empty_like(eeg1)
            call("eg_window_normalize", ptr(self.raw[slot]), ptr(eeg1), ptr(eeg2), n, self.C, self.T, self.mode, cur.cuda_stream)
            self.consumed[slot].record(cur)
            yield {"eeg1": eeg1, "eeg2": eeg2, "labels": self.labels[ids].to(self.device, non_blocking=True),
                   "dataset_idx": [self.index["windows"][int(i)]["dataset_idx"] for i in ids]}


# ------------------------------------------------------------------------------------------------------
# Device-resident recordings.  The shards above store every sample window_size / stride times and every batch
# crosses the host.  The recording store keeps each kept pair ONCE -- only the samples its windows cover, `[2][C][len]` f32 at a
# float offset of one flat `store.npy` -- plus a window table (pair, start).  ResidentWindows uploads store and tables once and
# cuts + normalises every batch on the device with one `eg_window_gather` launch: nothing of a batch crosses the host.
# ------------------------------------------------------------------------------------------------------
PREPROCESS_ORDER = 4            # the reference's Butterworth order (preprocess_eeg_windows.py:101)
PREPROCESS_KEYS = ("sampling_rate", "filter_low", "filter_high")


def recording_preprocessing_args(mapping) -> Dict:
    """{sampling_rate, filter_low, filter_high} of a `recording_preprocessing` mapping as floats; ValueError names a missing key"""
    missing = [k for k in PREPROCESS_KEYS if not hasattr(mapping, "keys") or k not in mapping]
    if missing:
        raise ValueError(f"recording_preprocessing needs {list(PREPROCESS_KEYS)}; missing {missing}")
    return {k: float(mapping[k]) for k in PREPROCESS_KEYS}


def recording_row_tables(lengths: Sequence[int], C: int, pad: int):
    """Recordings of `lengths` samples, each [C][length] f32, back to back -> (row_off i64, row_len i32, ws_off i64, floats,
    workspace doubles): eg_recording_filtfilt's tables, rows in storage order, row r's extended forward output at ws_off[r]."""
    ln = np.repeat(np.asarray(lengths, dtype=np.int64), C)
    row_off = np.concatenate([[0], np.cumsum(ln)])
    ws_off = np.concatenate([[0], np.cumsum(ln + 2 * pad)])
    return row_off[:-1].copy(), ln.astype(np.int32), ws_off[:-1].copy(), int(row_off[-1]), int(ws_off[-1])


def validate_recording_rows(row_off, row_len, C: int, pad: int, data_floats: int) -> None:
    """The only bounds check the recording kernels get (they trust their tables): every row inside the `data_floats` floats, rows
    in ascending order without overlap, every row longer than the filter's padding (where scipy raises the reference swallows the
    exception and goes on with the unfiltered signal; here it is a ValueError), one length inside each group of C rows."""
    off, ln = np.asarray(row_off, dtype=np.int64), np.asarray(row_len, dtype=np.int64)
    if C < 1 or len(off) < 1 or len(off) != len(ln) or len(off) % C:
        raise ValueError(f"recording rows: {len(off)} offsets, {len(ln)} lengths, C={C}")
    if ln.min() <= pad:
        r = int(np.argmin(ln))
        raise ValueError(f"recording rows: row {r} has {ln[r]} samples, the zero-phase filter needs more than its padding of {pad}")
    if (ln + 2 * pad).max() >= 2 ** 31:
        raise ValueError("recording rows: a row's padded length does not fit int32")
    end = off + ln
    if off[0] < 0 or (end > data_floats).any():
        r = int(np.argmax((end > data_floats) | (off < 0)))
        raise ValueError(f"recording rows: row {r} covers floats [{off[r]}, {end[r]}) of {data_floats}")
    if (off[1:] < end[:-1]).any():
        r = int(np.argmax(off[1:] < end[:-1]))
        raise ValueError(f"recording rows: row {r + 1} at float {off[r + 1]} overlaps row {r}, which ends at {end[r]}")
    g = ln.reshape(-1, C)
    if (g != g[:, :1]).any():
        raise ValueError(f"recording rows: group {int(np.argmax((g != g[:, :1]).any(axis=1)))} holds rows of different lengths")


def preprocess_recordings(recs, sampling_rate: float, filter_low: float, filter_high: float, order: int = PREPROCESS_ORDER,
                          device="cuda") -> List[torch.Tensor]:
    """The reference's recording-level preprocessing (preprocess_eeg, preprocess_eeg_windows.py:145-172) on the device: recs is a
    list of (C, L) arrays or tensors (one C, any lengths); returns f32 device tensors of the same shapes, views of one buffer --
    zero-phase Butterworth band-pass [filter_low, filter_high] Hz (filters.butter_bandpass, eg_recording_filtfilt), common-average
    reference over the C channels given, per-channel z-score over the whole recording (eg_recording_car_zscore).  One upload, two
    entry-point calls on the current stream, no host sync of its own.  ValueError: a bad band, a recording not longer than the
    filter's padding (3 * (2 * order + 1) samples), recordings of different channel counts."""
    import ctypes
    from . import _lib as L
    from .filters import butter_bandpass, lfilter_zi
    b, a = butter_bandpass(order, filter_low, filter_high, sampling_rate)
    zi = lfilter_zi(b, a)
    ncoef, pad = len(b), 3 * len(b)
    ts = [r.detach().to(torch.float32) if torch.is_tensor(r) else torch.from_numpy(np.ascontiguousarray(r, dtype=np.float32)) for r in recs]
    if not ts or any(t.dim() != 2 for t in ts) or len({int(t.shape[0]) for t in ts}) != 1:
        raise ValueError(f"preprocess_recordings needs (C, L) recordings of one channel count, got {[tuple(t.shape) for t in ts]}")
    C, lengths = int(ts[0].shape[0]), [int(t.shape[1]) for t in ts]
    row_off, row_len, ws_off, floats, ws_need = recording_row_tables(lengths, C, pad)
    validate_recording_rows(row_off, row_len, C, pad, floats)
    L.lib()
    dev = torch.device(device)
    data = torch.cat([t.reshape(-1) for t in ts]).to(dev)              # the one upload (host recordings); a fresh buffer either way
    tabs = [torch.from_numpy(x).to(dev) for x in (row_off, row_len, ws_off)]
    ws = torch.empty(ws_need, dtype=torch.float64, device=dev)
    desc = L.RecordingRowsDesc(L.ptr(data), L.ptr(tabs[0]), L.ptr(tabs[1]), L.ptr(tabs[2]), len(row_len), C, max(lengths), 0)
    dbl = lambda v: (ctypes.c_double * len(v))(*[float(x) for x in v])
    stream = torch.cuda.current_stream(dev).cuda_stream             # (tables and workspace are allocated and freed on this stream)
    L.call("eg_recording_filtfilt", ctypes.byref(desc), dbl(b), dbl(a), dbl(zi), ncoef, L.ptr(ws), ws_need, int(ws.numel()), stream)
    L.call("eg_recording_car_zscore", ctypes.byref(desc), stream)
    starts = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64) * C)])
    return [data[int(starts[i]):int(starts[i + 1])].view(C, lengths[i]) for i in range(len(ts))]


PREPROCESS_BATCH_BYTES = 256 << 20      # recording bytes per device batch of the store builder (the fp64 workspace is twice that)


def _preprocessed_pairs(pairs, prep: Dict, device):
    """kept_pairs' tuples with a, b replaced by their preprocessed WHOLE recordings (host arrays), in batches of bounded bytes"""
    batch, nbytes = [], 0

    def flush():
        out = preprocess_recordings([r for _, _, a, b, _ in batch for r in (a, b)], device=device, **prep)
        host = [t.cpu().numpy() for t in out]
        for j, (idx, item, _, _, nwin) in enumerate(batch):
            yield idx, item, host[2 * j], host[2 * j + 1], nwin
        batch.clear()

    for tup in pairs:
        batch.append(tup)
        nbytes += 4 * (tup[2].size + tup[3].size)
        if nbytes >= PREPROCESS_BATCH_BYTES:
            yield from flush()
            nbytes = 0
    if batch:
        yield from flush()


def build_recording_store(items: Sequence[Dict], eeg_base_path, label2id: Dict[str, int], out_dir, window_size: int = 1024,
                          stride: int = 256, recordings: Optional[Dict[str, np.ndarray]] = None, recording_preprocessing=None,
                          device="cuda") -> Dict:
    """`build_window_shards`' arguments, skipping rules and window order (kept_pairs), written as a recording store:
      store.npy   flat f32; pair p at float offset off[p] as [2][C][len[p]], len[p] = (nwin - 1) * stride + window_size
      labels.npy  i64 per window, as the shards'
      index.json  the shard index's keys (without `shards`) + `pairs` [{offset, length, dataset_idx}] + `window_pair` [count]
    recording_preprocessing = {sampling_rate, filter_low, filter_high}: each kept pair's two recordings go WHOLE through
    preprocess_recordings on `device` -- before they are cut to the common length, the reference's order
    (preprocess_eeg_windows.py:239-255) -- in batches of bounded device bytes; the layout is the same and index.json gains
    `preprocessed` {the three values, order}.  The common-average reference runs over the channels the store keeps (the pair's
    minimum), not over load_eeg_csv's zero-padded 32.  None (the default) writes what this function always wrote."""
    prep = recording_preprocessing_args(recording_preprocessing) if recording_preprocessing is not None else None
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    meta: List[Dict] = []
    labels: List[int] = []
    pairs: List[Dict] = []
    window_pair: List[int] = []
    C_all, total = None, 0
    walk = kept_pairs(items, eeg_base_path, window_size, stride, recordings)
    if prep is not None:
        walk = _preprocessed_pairs(walk, prep, device)
    tmp = out / "store.f32.partial"                     # the total is known only after the walk: raw first, .npy after
    with open(tmp, "wb") as f:
        for idx, item, a, b, nwin in walk:
            C_all = a.shape[0]
            length = (nwin - 1) * stride + window_size
            np.stack([a[:, :length], b[:, :length]]).astype(np.float32, copy=False).tofile(f)
            for w in range(nwin):
                meta.append(_window_meta(idx, item, w * stride, w * stride + window_size))
                labels.append(int(label2id[item["class"]]))
                window_pair.append(len(pairs))
            pairs.append({"offset": total, "length": length, "dataset_idx": idx})
            total += 2 * C_all * length
    store = np.lib.format.open_memmap(out / "store.npy", mode="w+", dtype=np.float32, shape=(total,))
    if total:
        raw = np.memmap(tmp, dtype=np.float32, mode="r", shape=(total,))
        for i in range(0, total, 1 << 24):
            store[i:i + (1 << 24)] = raw[i:i + (1 << 24)]
        del raw
    store.flush()
    del store
    tmp.unlink()
    np.save(out / "labels.npy", np.asarray(labels, dtype=np.int64))
    index = {"window_size": window_size, "stride": stride, "channels": C_all, "count": len(meta), "windows": meta,
             "label2id": label2id, "pairs": pairs, "window_pair": window_pair}
    if prep is not None:
        index["preprocessed"] = {**prep, "order": PREPROCESS_ORDER}
    (out / "index.json").write_text(json.dumps(index))
    return index


def store_tables(index: Dict):
    """index -> (pair_off [P], pair_len [P], win_pair [N], win_start [N]), int64 host arrays in eg_window_gather's table order"""
    return (np.asarray([p["offset"] for p in index["pairs"]], dtype=np.int64),
            np.asarray([p["length"] for p in index["pairs"]], dtype=np.int64),
            np.asarray(index["window_pair"], dtype=np.int64),
            np.asarray([w["start"] for w in index["windows"]], dtype=np.int64))


def validate_store(index: Dict, store_floats: int) -> None:
    """Raises ValueError unless every window lies inside its pair (0 <= start, start + T <= len[pair]), every pair inside the
    store's `store_floats` floats, and the pairs' offsets are non-decreasing without overlap.  This is the only bounds check the
    gather gets: the kernel trusts its tables."""
    C, T = int(index["channels"] or 0), int(index["window_size"])
    off, ln, wp, ws = store_tables(index)
    if C < 1 or T < 1:
        raise ValueError(f"recording store: channels={C} window_size={T}")
    if not (len(wp) == len(ws) == int(index["count"])):
        raise ValueError(f"recording store: {len(ws)} windows, {len(wp)} pair numbers, count {index['count']}")
    if len(ln) and (ln.min() < 0 or ln.max() >= 2 ** 31):
        raise ValueError("recording store: a pair's length does not fit int32")
    end = off + 2 * C * ln
    if len(off) and (off[0] < 0 or end[-1] > store_floats or (end > store_floats).any()):
        p = int(np.argmax((end > store_floats) | (off < 0)))
        raise ValueError(f"recording store: pair {p} covers floats [{off[p]}, {end[p]}) of a store of {store_floats}")
    if (off[1:] < end[:-1]).any():
        p = int(np.argmax(off[1:] < end[:-1]))
        raise ValueError(f"recording store: pair {p + 1} at float {off[p + 1]} overlaps pair {p}, which ends at {end[p]}")
    if len(wp) and (wp.min() < 0 or wp.max() >= len(ln)):
        raise ValueError(f"recording store: a window names a pair outside [0, {len(ln)})")
    bad = (ws < 0) | (ws + T > ln[wp]) if len(wp) else np.zeros(0, bool)
    if bad.any():
        w = int(np.argmax(bad))
        raise ValueError(f"recording store: window {w} covers samples [{ws[w]}, {ws[w] + T}) of pair {wp[w]}, which has {ln[wp[w]]}")


def epoch_order(n: int, shuffle: bool, seed: int, epoch: int, rank: int, world: int) -> np.ndarray:
    """Both loaders' `_order`: the epoch's (optionally shuffled) window order, rank r of world taking r::world"""
    idx = np.arange(n)
    if shuffle:
        idx = np.random.default_rng(seed + epoch).permutation(n)
    return idx[rank::world]


class DeviceRecordings:
    """A recording store in device memory with its window tables, and the launch that cuts batches out of it.
    data: flat f32 device tensor; the tables are host arrays (store_tables' order), validated by the caller."""

    def __init__(self, data: torch.Tensor, pair_off, pair_len, win_pair, win_start, win_label, C: int, T: int):
        from . import _lib as L
        L.lib()
        dev = data.device
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        self.data, self.C, self.T, self.device = data, int(C), int(T), dev
        self.pair_off, self.pair_len = up(pair_off, np.int64), up(pair_len, np.int32)
        self.win_pair, self.win_start = up(win_pair, np.int32), up(win_start, np.int32)
        self.win_label = up(win_label, np.int64) if win_label is not None else None
        self.n_windows = int(self.win_pair.numel())
        self.desc = L.WindowGatherDesc(L.ptr(data), L.ptr(self.pair_off), L.ptr(self.pair_len), L.ptr(self.win_pair),
                                       L.ptr(self.win_start), L.ptr(self.win_label), int(self.pair_off.numel()), self.n_windows,
                                       self.C, self.T)

    def gather(self, order: torch.Tensor, first: int, n: int, mode: int):
        """windows order[first : first + n] (order: i32 device tensor of window numbers) -> eeg1, eeg2 [n, C, T] f32 normalised in
        `mode` (0, 1: eg_window_gather; 2: as stored, eg_window_cut), labels [n] i64 or None: one launch on the current stream, no
        copy, no sync"""
        import ctypes
        from ._lib import call, ptr
        eeg1 = torch.empty(n, self.C, self.T, dtype=torch.float32, device=self.device)
        eeg2 = torch.empty_like(eeg1)
        labels = torch.empty(n, dtype=torch.int64, device=self.device) if self.win_label is not None else None
        if mode == 2:
            call("eg_window_cut", ctypes.byref(self.desc), ptr(order), int(order.numel()), int(first), int(n), ptr(eeg1), ptr(eeg2),
                 ptr(labels), torch.cuda.current_stream(self.device).cuda_stream)
            return eeg1, eeg2, labels
        call("eg_window_gather", ctypes.byref(self.desc), ptr(order), int(order.numel()), int(first), int(n), ptr(eeg1), ptr(eeg2),
             ptr(labels), int(mode), torch.cuda.current_stream(self.device).cuda_stream)
        return eeg1, eeg2, labels


class ResidentWindows:
    """WindowShards' interface over a recording store that lives in device memory: same constructor, same batches (bit for
    bit), same order, `__len__` and `set_epoch`.  Construction validates the index, uploads the store (in bounded chunks) and
    the tables once; an epoch uploads this rank's order (int32) once; a batch is ONE eg_window_gather launch on the current
    stream -- no host gather, no H2D copy, no event, no sync.  Build it once per run and iterate it every epoch.  With
    world > 1 every rank holds the whole store and takes its rank::world share.  There is no fallback: a store that does not
    fit raises EgError.  A store whose index carries `preprocessed` (build_recording_store(recording_preprocessing=...)) is cut
    as stored (eg_window_cut); asking for preprocessing=True on top of it raises ValueError."""
    UPLOAD_CHUNK = 1 << 24      # floats per staged upload (64 MiB)

    def __init__(self, root, batch_size: int, device, rank: int = 0, world: int = 1, shuffle: bool = False, seed: int = 0,
                 preprocessing: bool = False, drop_last: bool = False):
        from ._lib import EgError
        self.root = Path(root)
        self.index = json.loads((self.root / "index.json").read_text())
        self.preprocessed = self.index.get("preprocessed")
        if self.preprocessed and preprocessing:
            raise ValueError(f"{self.root}: the store's recordings were preprocessed whole ({self.preprocessed}); "
                             "preprocessing=True would normalise its windows a second time")
        labels = np.load(self.root / "labels.npy")
        host = np.load(self.root / "store.npy", mmap_mode="r")
        validate_store(self.index, int(host.shape[0]))
        self.n, self.C, self.T = int(self.index["count"]), int(self.index["channels"]), int(self.index["window_size"])
        if labels.shape[0] != self.n:
            raise ValueError(f"{self.root}: {labels.shape[0]} labels for {self.n} windows")
        self.B, self.device, self.rank, self.world = batch_size, torch.device(device), rank, world
        self.shuffle, self.seed, self.mode, self.drop_last = shuffle, seed, 1 if preprocessing else 0, drop_last
        if self.preprocessed:
            self.mode = 2                               # cut as stored: the z-score was taken over the whole recording
        self.epoch = 0
        self.dataset_idx = np.asarray([w["dataset_idx"] for w in self.index["windows"]], dtype=np.int64)
        need = 4 * int(host.shape[0])
        try:
            data = torch.empty(int(host.shape[0]), dtype=torch.float32, device=self.device)
        except torch.OutOfMemoryError as e:
            free = torch.cuda.mem_get_info(self.device)[0]
            raise EgError(f"ResidentWindows: the recording store needs {need} bytes of device memory, {free} are free "
                          "(there is no fallback: use WindowShards)") from e
        stage = torch.empty(min(self.UPLOAD_CHUNK, max(1, int(host.shape[0]))), dtype=torch.float32).pin_memory()
        for i in range(0, int(host.shape[0]), self.UPLOAD_CHUNK):
            m = min(self.UPLOAD_CHUNK, int(host.shape[0]) - i)
            stage.numpy()[:m] = host[i:i + m]
            data[i:i + m].copy_(stage[:m])              # synchronous: `stage` is free again when it returns
        off, ln, wp, ws = store_tables(self.index)
        self.store = DeviceRecordings(data, off, ln, wp, ws, labels, self.C, self.T)
        self._order_dev = None

    def set_epoch(self, epoch: int):
        self.epoch = epoch

    def _order(self) -> np.ndarray:
        return epoch_order(self.n, self.shuffle, self.seed, self.epoch, self.rank, self.world)

    __len__ = WindowShards.__len__

    def __iter__(self):
        order = self._order()
        nb = len(self)
        if nb == 0:
            return
        # the epoch's one upload; kept on the object so that the last launch's table outlives the generator
        self._order_dev = order_dev = torch.from_numpy(order.astype(np.int32)).to(self.device)
        didx = self.dataset_idx[order].tolist()
        for k in range(nb):
            first = k * self.B
            n = min(self.B, len(order) - first)
            eeg1, eeg2, labels = self.store.gather(order_dev, first, n, self.mode)
            yield {"eeg1": eeg1, "eeg2": eeg2, "labels": labels, "dataset_idx": didx[first:first + n]}
