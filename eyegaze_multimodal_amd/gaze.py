"""Gaze heat-map images on the device: the image half of the reference's MultimodalDataset
(1_Data/processed/multimodal_dataset.py:67-83, :151-154) -- Resize, RandomHorizontalFlip, ColorJitter(brightness, contrast), ToTensor,
Normalize -- without a batch ever crossing the host.  Every image is decoded once on the host (Pillow), resized once on the device
into a uint8 store (eg_gaze_resize: Pillow's bytes) and kept there; a training batch is ONE eg_gaze_batch launch that gathers,
flips, jitters, normalises and writes the [B, F, W] fp32 images ImageEngine.forward takes, addressed by the window order that
eg_window_gather takes.  ResidentMultimodal pairs it with data.ResidentWindows: two launches per batch.

There is no CPU path: both entry points live in libeyegaze_hip.so."""
from __future__ import annotations

import ctypes
import dataclasses
import functools
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .engine import scramble_seed

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # multimodal_dataset.py:74-75
MAX_SIDE, MIN_OUT, MAX_OUT = 4096, 8, 512      # EG_GAZE_MAX_SIDE, EG_GAZE_MIN_OUT, EG_GAZE_MAX_OUT
PRECISION_BITS = 22                            # Pillow's fixed point for 8-bit samples
RESIZE_BATCH_BYTES = 256 << 20                 # device bytes (images, intermediates) per eg_gaze_resize call


# ---------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resize_tables(in_size: int, out_size: int) -> np.ndarray:
    """One axis of Pillow's antialiased bilinear resample, in -> out, as eg_gaze_resize reads it: int32 words [0] ksize,
    [1 .. out] xmin, [1 + out .. 2 out] count, then k [out][ksize] -- the triangle filter over a support of max(in / out, 1) source
    pixels around (xx + 0.5) in / out, normalised by its sequential sum, rounded to 22-bit fixed point.  fp64 throughout, as the
    library computes it.  Cached per (in, out); the array is read-only."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resize_tables: sizes must be >= 1 (got {in_size} -> {out_size})")
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = fscale
    ksize = 2 * int(math.ceil(support)) + 1
    xx = np.arange(out_size, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0.0).astype(np.int64)
    xmax = np.minimum(np.trunc(center + support + 0.5), float(in_size)).astype(np.int64)
    count = xmax - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs((x + xmin[:, None] - center[:, None] + 0.5) / fscale))
    w[x >= count[:, None]] = 0.0
    ww = np.zeros(out_size, np.float64)
    for t in range(ksize):                     # the sequential sum, tap by tap (trailing zeros add nothing)
        ww += w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.trunc(0.5 + w * float(1 << PRECISION_BITS)).astype(np.int32)        # (no weight of this filter is negative)
    tab = np.concatenate([[ksize], xmin, count, k.reshape(-1)]).astype(np.int32)
    tab.setflags(write=False)
    return tab


def validate_resize_tables(tab, in_size: int, out_size: int) -> None:
    """The only bounds check eg_gaze_resize's taps get (the kernel trusts its tables): ValueError unless the table has resize_tables'
    shape for in -> out, 0 <= xmin, count >= 1, xmin + count <= in and count <= ksize for every output."""
    tab = np.asarray(tab)
    if tab.ndim != 1 or tab.size < 1 + 2 * out_size:
        raise ValueError(f"resize table {in_size} -> {out_size}: {tab.size} words, too short for its xmin and count")
    ksize = int(tab[0])
    want = 2 * int(math.ceil(max(in_size / out_size, 1.0))) + 1
    if ksize != want or tab.size != 1 + 2 * out_size + out_size * ksize:
        raise ValueError(f"resize table {in_size} -> {out_size}: ksize {ksize} in {tab.size} words, expected ksize {want}")
    xmin, count = tab[1:1 + out_size].astype(np.int64), tab[1 + out_size:1 + 2 * out_size].astype(np.int64)
    bad = (xmin < 0) | (count < 1) | (xmin + count > in_size) | (count > ksize)
    if bad.any():
        xx = int(np.argmax(bad))
        raise ValueError(f"resize table {in_size} -> {out_size}: output {xx} reads [{xmin[xx]}, {xmin[xx]} + {count[xx]}) of {in_size} "
                         f"source pixels with ksize {ksize}")


def normalise_table(mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD) -> torch.Tensor:
    """[3, 256] f32 (host): ToTensor followed by Normalize(mean, std) of every uint8 value, in the operations torchvision runs --
    float32(v) / 255, minus the float32 mean, divided by the float32 std -- so the table is their result, not an approximation"""
    if len(mean) != 3 or len(std) != 3 or any(float(s) == 0.0 for s in std):
        raise ValueError(f"normalise_table needs three means and three non-zero stds (got {mean!r}, {std!r})")
    v = torch.arange(256, dtype=torch.float32).div(255)
    m, s = torch.as_tensor(mean, dtype=torch.float32), torch.as_tensor(std, dtype=torch.float32)
    return v[None, :].sub(m[:, None]).div(s[:, None]).contiguous()


@dataclasses.dataclass(frozen=True)
class GazeAugmentation:
    """The reference's training transforms on the resized image (multimodal_dataset.py:71-72): RandomHorizontalFlip(hflip_prob) and
    ColorJitter(brightness, contrast) -- factors uniform in [1 - x, 1 + x], the two in a random order -- drawn per image and player
    on the device (eg_gaze_batch).  Refuses what the C entry point refuses.  The YAML form is `training.image_augmentation:` with
    these three keys; absent means none (from_config)."""
    hflip_prob: float = 0.5
    brightness: float = 0.2
    contrast: float = 0.2

    def __post_init__(self):
        for name in ("hflip_prob", "brightness", "contrast"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"{name} must be a finite number (got {v!r})")
        if not 0.0 <= self.hflip_prob <= 1.0:
            raise ValueError(f"hflip_prob must lie in [0, 1] (got {self.hflip_prob!r})")
        for name in ("brightness", "contrast"):
            if not 0.0 <= getattr(self, name) < 1.0:
                raise ValueError(f"{name} must lie in [0, 1) (got {getattr(self, name)!r})")

    @property
    def enabled(self) -> bool:
        return bool(self.hflip_prob or self.brightness or self.contrast)

    @classmethod
    def from_config(cls, config: Dict) -> Optional["GazeAugmentation"]:
        """config['training']['image_augmentation'] -> an instance, None when the key is absent or null; unknown keys are a ValueError"""
        m = (config.get("training") or {}).get("image_augmentation")
        if m is None:
            return None
        if not hasattr(m, "keys"):
            raise ValueError(f"training.image_augmentation must be a mapping of hflip_prob / brightness / contrast (got {m!r})")
        extra = sorted(set(m) - {"hflip_prob", "brightness", "contrast"})
        if extra:
            raise ValueError(f"training.image_augmentation: unknown keys {extra}")
        return cls(**{k: m[k] for k in m})


def _upload(host: torch.Tensor, dev) -> torch.Tensor:
    """host -> device without a host sync: through pinned memory, asynchronously on the current stream"""
    if dev.type != "cuda":
        return host.to(dev)
    return host.pin_memory().to(dev, non_blocking=True)


def _size(size) -> Tuple[int, int]:
    F, W = (int(size), int(size)) if isinstance(size, (int, np.integer)) else (int(size[0]), int(size[1]))
    if not (MIN_OUT <= F <= MAX_OUT and MIN_OUT <= W <= MAX_OUT):
        raise ValueError(f"GazeImageStore: size {F}x{W}, served are {MIN_OUT} to {MAX_OUT} per side")
    return F, W


def load_rgb(path) -> np.ndarray:
    """Image.open(path).convert('RGB') as a (h, w, 3) uint8 array (multimodal_dataset.py:153)"""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("the gaze heat maps load through Pillow (PIL), which is not installed") from e
    with Image.open(path) as img:
        return np.asarray(img.convert("RGB"), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# the store
# ---------------------------------------------------------------------------------------------------------------
class GazeImageStore:
    """N gaze images resized to (F, W) and resident in device memory as uint8 [N, F, W, 3]: `data`.  Build it once per run
    (from_arrays / from_files); batch() cuts training batches out of it."""

    def __init__(self, data: torch.Tensor, norm: Optional[torch.Tensor] = None):
        if data.dtype != torch.uint8 or data.dim() != 4 or data.shape[3] != 3 or not data.is_contiguous():
            raise ValueError(f"GazeImageStore needs a contiguous uint8 [N, F, W, 3] tensor (got {data.dtype} {tuple(data.shape)})")
        self.data, self.device = data, data.device
        self.n, self.F, self.W = int(data.shape[0]), int(data.shape[1]), int(data.shape[2])
        _size((self.F, self.W))
        self.norm = (normalise_table() if norm is None else norm).to(device=self.device, dtype=torch.float32).contiguous()

    def __len__(self) -> int:
        return self.n

    @classmethod
    def from_arrays(cls, images: Sequence[np.ndarray], size, device="cuda", mean=IMAGENET_MEAN, std=IMAGENET_STD) -> "GazeImageStore":
        """images: (h, w, 3) uint8 arrays of any sizes; size: an int or (F, W).  One upload and one eg_gaze_resize call per batch
        of at most RESIZE_BATCH_BYTES device bytes, on the current stream, no sync.  ValueError: an image that is not (h, w, 3)
        uint8 or has a side outside [1, 4096], a size outside [8, 512]."""
        from . import _lib as L
        F, W = _size(size)
        arrs = []
        for i, im in enumerate(images):
            a = np.asarray(im)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"GazeImageStore: image {i} is {a.dtype} {a.shape}, served is uint8 (h, w, 3)")
            if not (1 <= a.shape[0] <= MAX_SIDE and 1 <= a.shape[1] <= MAX_SIDE):
                raise ValueError(f"GazeImageStore: image {i} is {a.shape[0]}x{a.shape[1]}, served are sides of 1 to {MAX_SIDE}")
            arrs.append(np.ascontiguousarray(a))
        L.lib()
        dev = torch.device(device)
        data = torch.empty(len(arrs), F, W, 3, dtype=torch.uint8, device=dev)
        first, used = 0, 0
        for i, a in enumerate(arrs):
            mine = a.size + 3 * W * a.shape[0] + 64
            if i > first and used + mine > RESIZE_BATCH_BYTES:
                _resize_batch(arrs[first:i], F, W, dev, data[first:i])
                first, used = i, 0
            used += mine
        if arrs:
            _resize_batch(arrs[first:], F, W, dev, data[first:])
        return cls(data, normalise_table(mean, std))

    @classmethod
    def from_files(cls, paths: Sequence, size, device="cuda", mean=IMAGENET_MEAN, std=IMAGENET_STD) -> "GazeImageStore":
        """from_arrays over Image.open(p).convert('RGB') of every path (decoding is the host's: JPEG needs Pillow)"""
        return cls.from_arrays([load_rgb(p) for p in paths], size, device, mean, std)

    def batch(self, pair_img: torch.Tensor, win_pair: torch.Tensor, order: torch.Tensor, first: int, n: int,
              augmentation: Optional[GazeAugmentation] = None, seed: int = 0, rgb: bool = False, _factors: Optional[torch.Tensor] = None):
        """Samples order[first : first + n] of eg_window_gather's addressing -- pair_img [n_pairs, 2] i32 (store index of player 1's
        and player 2's image of every pair), win_pair [n_windows] i32, order i32, all device tensors -- as img1, img2 [n, F, W] f32
        (and rgb1, rgb2 [n, 3, F, W] f32 with rgb=True): ONE eg_gaze_batch launch on the current stream, no copy, no sync.
        augmentation None (or with everything 0) gives the evaluation transform; otherwise sample j, player pl draws from counter
        2 (first + j) + pl of the 64-bit `seed`, whose halves travel as seed_lo / seed_hi.  The index tables are trusted as
        eg_window_gather trusts its own; validate_pair_img checks pair_img once.
        _factors is TEST-ONLY: a [2 n, 4] f32 device tensor of (flip, fb, fc, brightness first) per image 2 j + pl that replaces the
        draws, for parity against Pillow at given factors."""
        from ._lib import call, ptr
        for name, t in (("pair_img", pair_img), ("win_pair", win_pair), ("order", order)):
            if t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"GazeImageStore.batch: {name} must be a contiguous int32 tensor on {self.device}")
        if _factors is not None and (_factors.dtype != torch.float32 or tuple(_factors.shape) != (2 * n, 4) or _factors.device != self.device
                                     or not _factors.is_contiguous()):
            raise ValueError(f"GazeImageStore.batch: _factors must be a contiguous f32 [{2 * n}, 4] tensor on {self.device}")
        aug = augmentation if augmentation is not None and augmentation.enabled else None
        f32 = dict(dtype=torch.float32, device=self.device)
        img1, img2 = torch.empty(n, self.F, self.W, **f32), torch.empty(n, self.F, self.W, **f32)
        rgb1 = torch.empty(n, 3, self.F, self.W, **f32) if rgb else None
        rgb2 = torch.empty(n, 3, self.F, self.W, **f32) if rgb else None
        seed = int(seed) & ((1 << 64) - 1)
        stream = torch.cuda.current_stream(self.device).cuda_stream if self.device.type == "cuda" else 0
        call("eg_gaze_batch", ptr(self.data), self.n, self.F, self.W, ptr(pair_img), ptr(win_pair), ptr(order), int(order.numel()),
             int(first), int(n), ptr(self.norm), seed & 0xFFFFFFFF, seed >> 32, float(aug.hflip_prob) if aug else 0.0,
             float(aug.brightness) if aug else 0.0, float(aug.contrast) if aug else 0.0, ptr(_factors), ptr(img1), ptr(img2), ptr(rgb1),
             ptr(rgb2), stream)
        return (img1, img2, rgb1, rgb2) if rgb else (img1, img2)


def validate_pair_img(pair_img, n_pairs: int, n_images: int) -> np.ndarray:
    """pair_img as an int32 [n_pairs, 2] host array; ValueError unless it has that shape and every entry names an image of the store.
    With data.validate_store (win_pair < n_pairs) this is the bounds check eg_gaze_batch's gather gets."""
    a = np.asarray(pair_img)
    if a.ndim != 2 or a.shape != (n_pairs, 2) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"pair_img must be an integer [{n_pairs}, 2] array (got {a.dtype} {a.shape})")
    if a.size and (a.min() < 0 or a.max() >= n_images):
        p = int(np.argmax(((a < 0) | (a >= n_images)).any(axis=1)))
        raise ValueError(f"pair_img: pair {p} names images {a[p].tolist()} of a store of {n_images}")
    return np.ascontiguousarray(a, dtype=np.int32)


def _resize_batch(arrs: List[np.ndarray], F: int, W: int, dev, out: torch.Tensor) -> None:
    """one ragged eg_gaze_resize call: out [len(arrs), F, W, 3] uint8 (a slice of the store)"""
    from . import _lib as L
    n = len(arrs)
    off, mid_off, at, mid = [], [], 0, 0
    for a in arrs:
        off.append(at)
        mid_off.append(mid)
        at += -(-a.size // 16) * 16
        mid += -(-(3 * W * a.shape[0]) // 16) * 16
    host = np.zeros(at, dtype=np.uint8)
    for a, o in zip(arrs, off):
        host[o:o + a.size] = a.reshape(-1)
    hs, ws = [a.shape[0] for a in arrs], [a.shape[1] for a in arrs]
    words, where, parts = 0, {}, []
    for key in [(w, W) for w in ws] + [(h, F) for h in hs]:
        if key not in where:
            tab = resize_tables(*key)
            validate_resize_tables(tab, *key)
            where[key] = words
            parts.append(tab)
            words += tab.size
    htab, vtab = [where[(w, W)] for w in ws], [where[(h, F)] for h in hs]
    sum_h = int(sum(hs))
    need = L.gaze_resize_workspace_bytes(n, sum_h, W)
    if need < 0 or mid > need:
        raise L.EgError(f"eg_gaze_resize_workspace_bytes({n}, {sum_h}, {W}) = {need}, the intermediates take {mid}")
    data = _upload(torch.from_numpy(host), dev)                                          # ONE upload of the pixels
    tabs = _upload(torch.from_numpy(np.concatenate(parts)), dev)
    meta = _upload(torch.from_numpy(np.concatenate([off, mid_off, htab, vtab, hs, ws]).astype(np.int64)), dev)
    t_h, t_w = meta[4 * n:5 * n].to(torch.int32), meta[5 * n:].to(torch.int32)
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    desc = L.GazeResizeDesc(L.ptr(data), L.ptr(meta), L.ptr(t_h), L.ptr(t_w), L.ptr(meta) + 8 * n, L.ptr(tabs), L.ptr(meta) + 16 * n,
                            L.ptr(meta) + 24 * n, sum_h, n, max(hs), F, W)
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
    L.call("eg_gaze_resize", ctypes.byref(desc), L.ptr(work), need, L.ptr(out), stream)


# ---------------------------------------------------------------------------------------------------------------
# the loader
# ---------------------------------------------------------------------------------------------------------------
def batch_seed(seed: int, epoch: int, batch: int, rank: int) -> int:
    """The 64-bit augmentation seed of one batch: splitmix64 (engine.scramble_seed) folded over (seed, epoch, batch, rank), so that no
    two batches, epochs or ranks of a run share their draws and a re-run repeats them"""
    s = scramble_seed(int(seed) & ((1 << 64) - 1))
    for v in (epoch, batch, rank):
        s = scramble_seed(s ^ (int(v) & ((1 << 64) - 1)))
    return s


class ResidentMultimodal:
    """The multimodal loader: data.ResidentWindows (EEG) and a GazeImageStore (images) walked in ResidentWindows' order.  Per batch
    two launches over the same order_dev, first, n -- eg_window_gather (or eg_window_cut) and eg_gaze_batch -- and no other host
    work; yields (img1, img2, eeg1, eeg2, labels), the tuple MultimodalTrainer.train_step and evaluate take.
    pair_img [n_pairs, 2]: the store index of player 1's and player 2's image of every pair of the recording store, in its pair
    order.  augmentation None is the evaluation transform; otherwise batch k of an epoch draws from batch_seed(eeg.seed, epoch, k,
    rank).  __len__ and set_epoch are ResidentWindows'."""

    def __init__(self, eeg, images: GazeImageStore, pair_img, augmentation: Optional[GazeAugmentation] = None):
        if images.device != eeg.device and (images.device.type, images.device.index or 0) != (eeg.device.type, eeg.device.index or 0):
            raise ValueError(f"ResidentMultimodal: the recordings live on {eeg.device}, the images on {images.device}")
        self.eeg, self.images, self.augmentation = eeg, images, augmentation
        host = validate_pair_img(pair_img, int(eeg.store.pair_off.numel()), len(images))
        self.pair_img = torch.from_numpy(host).to(images.device)

    def __len__(self) -> int:
        return len(self.eeg)

    def set_epoch(self, epoch: int) -> None:
        self.eeg.set_epoch(epoch)

    def __iter__(self):
        eeg = self.eeg
        order = eeg._order()
        nb = len(eeg)
        if nb == 0:
            return
        eeg._order_dev = order_dev = torch.from_numpy(order.astype(np.int32)).to(eeg.device)      # the epoch's one upload
        for k in range(nb):
            first = k * eeg.B
            n = min(eeg.B, len(order) - first)
            eeg1, eeg2, labels = eeg.store.gather(order_dev, first, n, eeg.mode)
            img1, img2 = self.images.batch(self.pair_img, eeg.store.win_pair, order_dev, first, n, self.augmentation,
                                           batch_seed(eeg.seed, eeg.epoch, k, eeg.rank))
            yield img1, img2, eeg1, eeg2, labels
