"""Gaze error and mechanism analysis on the device: the reference's ErrorAnalyzer and MechanismAnalyzer
(6_Utils/error_analysis.py) and step 4 of 7_Analysis/python_scripts/analyze_gaze.py over a trained multimodal model and the
device-resident image store (gaze.GazeImageStore).

The reference computes its spatial table one sample at a time: compute_gaze_distance and compute_gaze_overlap run about fifteen
small torch reductions and six .item() calls per sample.  Here the whole table is ONE eg_gaze_pair_stats call -- two memory-bound
walks over the uint8 store -- computed once per pair and gathered per sample on the device; eg_row_cosine is
compute_feature_correlation's arithmetic.  There is no CPU path for either: both live in libeyegaze_hip.so.  The host statistics
(pair accuracy summaries, class statistics, ANOVA and t-tests) are plain numpy restatements of the reference's outputs, key for
key; their p-values come from the regularised incomplete beta function below, so neither scipy nor pandas is imported."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import gaze as G

DEFAULT_CLASS_NAMES = ["Single", "Competition", "Cooperation"]                # error_analysis.py:30
PAIR_FIELDS = ("distance", "overlap", "cy_a", "cx_a", "cy_b", "cx_b", "inter", "union", "na", "nb", "total_a", "total_b",
               "abs_total_a", "abs_total_b")                                  # the columns of eg_gaze_pair_stats' rows
_INT_FIELDS = ("inter", "union", "na", "nb")


# ---------------------------------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------------------------------
def raw_table() -> torch.Tensor:
    """[3, 256] f32 (host): ToTensor alone, float32(v) / 255 in every channel"""
    return torch.arange(256, dtype=torch.float32).div(255).repeat(3, 1).contiguous()


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0


def _pair_tensor(store: G.GazeImageStore, pair_img) -> torch.Tensor:
    """pair_img as an int32 [n_pairs, 2] tensor on the store's device.  A host array is checked by gaze.validate_pair_img and
    uploaded; a tensor that already lives on the device is taken as it is, without the download a check would cost (it is
    ResidentMultimodal.pair_img, checked when the loader was built) -- the kernel skips a pair that names no image, and its row
    stays NaN."""
    if isinstance(pair_img, torch.Tensor) and pair_img.device.type != "cpu":
        if (pair_img.dtype != torch.int32 or pair_img.device != store.device or pair_img.dim() != 2 or pair_img.shape[1] != 2
                or pair_img.shape[0] == 0 or not pair_img.is_contiguous()):
            raise ValueError(f"pair_img on a device must be a contiguous int32 [n_pairs, 2] tensor on {store.device}, n_pairs > 0")
        return pair_img
    host = pair_img.numpy() if isinstance(pair_img, torch.Tensor) else np.asarray(pair_img)
    if host.ndim != 2 or host.shape[0] == 0:
        raise ValueError(f"pair_img must be an integer [n_pairs, 2] array, n_pairs > 0 (got shape {host.shape})")
    return G._upload(torch.from_numpy(G.validate_pair_img(host, host.shape[0], len(store))), store.device)


def spatial_statistics(store: G.GazeImageStore, pair_img, normalised: bool = True, threshold: float = 0.1) -> Dict[str, torch.Tensor]:
    """compute_gaze_distance and compute_gaze_overlap (error_analysis.py:277-358) of every pair of pair_img [n_pairs, 2] (store
    numbers of the two players' images) in ONE eg_gaze_pair_stats call on the current stream, no sync.  normalised=True reads the
    store's own table (what the dataloader yields: ToTensor + Normalize), False the table float32(v) / 255 (ToTensor alone).
    -> device tensors [n_pairs]: distance, overlap, cy_a, cx_a, cy_b, cx_b (f64), inter, union, na, nb (i64), total = [n_pairs, 2]
    f64 (sum of the grey image, the denominator of the centre) and abs_total likewise (sum |g|: abs_total / |total| is the
    centre's condition number).
    On normalised tensors total is usually negative, and the reference then returns its literal default centre (112, 112) whatever
    the image size is: both images of such a pair give distance 0.  The raw table gives the meaningful centre of mass."""
    from . import _lib as L
    if not math.isfinite(float(threshold)):
        raise ValueError(f"threshold must be finite (got {threshold!r})")
    dev = store.device
    pairs = _pair_tensor(store, pair_img)
    n_pairs = int(pairs.shape[0])
    table = store.norm if normalised else raw_table().to(dev)
    need = L.gaze_pair_stats_workspace_bytes(len(store))
    work = torch.empty(need // 8, dtype=torch.float64, device=dev)
    out = torch.full((n_pairs, L.GAZE_PAIR_FIELDS), float("nan"), dtype=torch.float64, device=dev)
    L.call("eg_gaze_pair_stats", L.ptr(store.data), len(store), store.F, store.W, L.ptr(pairs), n_pairs, L.ptr(table), float(threshold),
           L.ptr(work), need, L.ptr(out), _stream(dev))
    res = {name: out[:, i] for i, name in enumerate(PAIR_FIELDS[:6])}
    res.update({name: out[:, 6 + i].to(torch.int64) for i, name in enumerate(_INT_FIELDS)})       # counts <= 2^18: exact in f64
    res["total"], res["abs_total"] = out[:, 10:12], out[:, 12:14]
    return res


def _names(labels: np.ndarray, class_names: Optional[Sequence[str]]) -> List[str]:
    names = list(class_names or DEFAULT_CLASS_NAMES)
    return [names[int(l)] for l in labels]


def spatial_sensitivity(store: G.GazeImageStore, pair_img, win_pair, predictions, labels, class_names: Optional[Sequence[str]] = None,
                        normalised: bool = True, threshold: float = 0.1) -> Dict[str, np.ndarray]:
    """analyze_spatial_sensitivity's DataFrame (error_analysis.py:360-412) as a dict of its columns, one row per sample: distance,
    overlap, correct, label, label_name.  Sample i shows the images of pair win_pair[i]; the table is computed once per pair
    (spatial_statistics) and gathered through win_pair on the device; ONE host copy at the end.  predictions and labels: [n]
    integers (device tensors or arrays)."""
    dev = store.device
    st = spatial_statistics(store, pair_img, normalised, threshold)
    wp = torch.as_tensor(win_pair, device=dev).to(torch.int64)
    n_pairs = int(st["distance"].shape[0])
    pred, lab = torch.as_tensor(predictions, device=dev).to(torch.int64), torch.as_tensor(labels, device=dev).to(torch.int64)
    if not (wp.dim() == 1 and pred.shape == wp.shape and lab.shape == wp.shape):
        raise ValueError(f"win_pair, predictions and labels must be [n] (got {tuple(wp.shape)}, {tuple(pred.shape)}, {tuple(lab.shape)})")
    both = torch.stack([st["distance"][wp.clamp(0, n_pairs - 1)], st["overlap"][wp.clamp(0, n_pairs - 1)], (pred == lab).double(),
                        lab.double(), wp.double()])
    host = both.cpu().numpy()                                                  # the one copy (and the one sync)
    if host.shape[1] and (host[4].min() < 0 or host[4].max() >= n_pairs):
        raise ValueError(f"win_pair names pair {int(host[4].max() if host[4].max() >= n_pairs else host[4].min())} of {n_pairs}")
    label = host[3].astype(np.int64)
    return {"distance": host[0], "overlap": host[1], "correct": host[2].astype(np.int64), "label": label,
            "label_name": np.asarray(_names(label, class_names))}


def row_cosine(f1: torch.Tensor, f2: torch.Tensor) -> torch.Tensor:
    """[N] f32 on the device: the cosine of every row pair of two [N, D] arrays (eg_row_cosine: fp64 sums, F.normalize's clamp);
    no sync"""
    from . import _lib as L
    if f1.dim() != 2 or f1.shape != f2.shape or f1.device != f2.device:
        raise ValueError(f"row_cosine needs two [N, D] tensors on one device (got {tuple(f1.shape)}, {tuple(f2.shape)})")
    a, b = f1.detach().float().contiguous(), f2.detach().float().contiguous()
    out = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    L.call("eg_row_cosine", L.ptr(a), L.ptr(b), int(a.shape[0]), int(a.shape[1]), L.ptr(out), _stream(a.device))
    return out


def feature_correlation(f1: torch.Tensor, f2: torch.Tensor, labels, class_names: Optional[Sequence[str]] = None) -> Dict[str, np.ndarray]:
    """compute_feature_correlation (error_analysis.py:414-469) on two [N, D] feature arrays, as the columns of
    save_correlation_analysis_csv: similarity, label, label_name"""
    sim = row_cosine(f1, f2)
    label = torch.as_tensor(labels).detach().cpu().numpy().astype(np.int64)
    if label.shape != (sim.shape[0],):
        raise ValueError(f"labels must be [{sim.shape[0]}] (got {label.shape})")
    return {"similarity": sim.cpu().numpy(), "label": label, "label_name": np.asarray(_names(label, class_names))}


def image_feature_correlation(image_engine, labels, class_names: Optional[Sequence[str]] = None) -> Dict[str, np.ndarray]:
    """feature_correlation over the two players' pooled features of ImageEngine's LAST forward (its `feat` buffer, [2 B, d] in image
    order (sample, player)): the image branch's counterpart of the reference's cls1 / cls2"""
    feat = image_engine.a["feat"]
    pair = feat.view(feat.shape[0] // 2, 2, feat.shape[1])
    return feature_correlation(pair[:, 0], pair[:, 1], labels, class_names)


@torch.no_grad()
def predict_multimodal(trainer, batches) -> Dict[str, np.ndarray]:
    """One walk over (img1, img2, eeg1, eeg2, labels) batches in eval mode, as MultimodalTrainer.evaluate walks them (the same
    engines, the same fusion call) -> y_true [n], y_pred [n] (argmax of the fused logits), y_prob [n, K] (their softmax) and alpha.
    Everything stays on the device until the walk is over; one copy each at the end."""
    m = trainer.model
    m.eval()
    yt, yp, pr, al = [], [], [], []
    for img1, img2, eeg1, eeg2, labels in batches:
        B, _, T = eeg1.shape
        eeg, img = trainer._engines(B, T, img1.shape[-2], img1.shape[-1])
        z_img = img.forward(img1.contiguous().float(), img2.contiguous().float(), train=False).clone()
        eeg.forward(eeg1.contiguous().float(), eeg2.contiguous().float(), labels, train=False)
        fused, alpha, _ = m.fusion(z_img, eeg.a["logits"].clone())
        yt.append(labels.to(torch.int64))
        yp.append(fused.argmax(-1))
        pr.append(torch.softmax(fused.float(), dim=-1))
        al.append(alpha.float().reshape(B, -1))
    if not yt:
        raise ValueError("predict_multimodal: no batches")
    return {"y_true": torch.cat(yt).cpu().numpy(), "y_pred": torch.cat(yp).cpu().numpy(), "y_prob": torch.cat(pr).cpu().numpy(),
            "alpha": torch.cat(al).cpu().numpy()}


def pair_performance(pair_ids: torch.Tensor, y_true: torch.Tensor, y_pred: torch.Tensor) -> Dict[str, np.ndarray]:
    """analyze_pair_performance (error_analysis.py:59-83) from device tensors: per pair id the number of correct samples, the
    number of samples and their ratio, counted with torch.bincount on integers (integer sums are order-free) -> pair_id,
    correct_count, total_count, accuracy for the ids that occur, sorted by accuracy ascending with pair_id as the tie-break.
    The reference's sort_values('accuracy') uses an unstable sort and leaves the order of equal accuracies undefined; the
    tie-break here makes the table a function of its input."""
    ids = torch.as_tensor(pair_ids).to(torch.int64)
    yt, yp = torch.as_tensor(y_true, device=ids.device).to(torch.int64), torch.as_tensor(y_pred, device=ids.device).to(torch.int64)
    if ids.dim() != 1 or ids.numel() == 0 or yt.shape != ids.shape or yp.shape != ids.shape:
        raise ValueError(f"pair_performance needs three [n] tensors, n > 0 (got {tuple(ids.shape)}, {tuple(yt.shape)}, {tuple(yp.shape)})")
    uniq, inv = torch.unique(ids, return_inverse=True)                         # ids need not be small or non-negative
    total = torch.bincount(inv, minlength=uniq.numel())
    correct = torch.bincount(inv[yt == yp], minlength=uniq.numel())
    host = torch.stack([uniq, correct, total]).cpu().numpy()
    acc = host[1] / host[2]                                                    # fp64 quotient of two integers: pandas' mean of booleans
    order = np.lexsort((host[0], acc))
    return {"pair_id": host[0][order], "correct_count": host[1][order], "total_count": host[2][order], "accuracy": acc[order]}


# ---------------------------------------------------------------------------------------------------------------
# host statistics: numpy restatements of the reference's outputs, key for key
# ---------------------------------------------------------------------------------------------------------------
def hard_pairs(stats: Dict[str, np.ndarray], percentile: float = 20) -> List[int]:
    """identify_hard_pairs: the pair ids whose accuracy is at or below the percentile, in the table's order"""
    acc = np.asarray(stats["accuracy"], np.float64)
    thr = np.percentile(acc, percentile)
    return [int(p) for p in np.asarray(stats["pair_id"])[acc <= thr]]


def pair_statistics(stats: Dict[str, np.ndarray]) -> Dict[str, float]:
    """compute_pair_statistics; std is pandas' (ddof = 1; nan for a single pair)"""
    acc = np.asarray(stats["accuracy"], np.float64)
    return {"mean_accuracy": float(acc.mean()), "std_accuracy": float(acc.std(ddof=1)) if acc.size > 1 else float("nan"),
            "min_accuracy": float(acc.min()), "max_accuracy": float(acc.max()), "n_pairs": int(acc.size),
            "hard_pairs_count": len(hard_pairs(stats))}


def error_distribution(y_true, y_pred, class_names: Optional[Sequence[str]] = None) -> Dict[str, np.ndarray]:
    """analyze_error_distribution: one row per misclassified sample"""
    names = list(class_names or DEFAULT_CLASS_NAMES)
    yt, yp = np.asarray(y_true).astype(np.int64), np.asarray(y_pred).astype(np.int64)
    idx = np.flatnonzero(yt != yp)
    tn, pn = [names[t] for t in yt[idx]], [names[p] for p in yp[idx]]
    return {"sample_idx": idx, "true_label": yt[idx], "true_name": np.asarray(tn, dtype=str), "pred_label": yp[idx],
            "pred_name": np.asarray(pn, dtype=str), "confusion_type": np.asarray([f"{t}_as_{p}" for t, p in zip(tn, pn)], dtype=str)}


def confusion_analysis(y_true, y_pred, class_names: Optional[Sequence[str]] = None) -> Dict[str, np.ndarray]:
    """compute_confusion_analysis: every (true, predicted) pair of distinct classes whose true class occurs, with its count and
    its percentage of the true class, by count descending (ties in the reference's row order: a stable sort)"""
    names = list(class_names or DEFAULT_CLASS_NAMES)
    yt, yp = np.asarray(y_true), np.asarray(y_pred)
    rows = []
    for i, tn in enumerate(names):
        tc = int((yt == i).sum())
        for j, pn in enumerate(names):
            if i != j and tc > 0:
                c = int(((yt == i) & (yp == j)).sum())
                rows.append((tn, pn, c, c / tc * 100))
    rows.sort(key=lambda r: -r[2])
    return {"true_class": np.asarray([r[0] for r in rows], dtype=str), "pred_class": np.asarray([r[1] for r in rows], dtype=str),
            "count": np.asarray([r[2] for r in rows], np.int64), "percentage": np.asarray([r[3] for r in rows], np.float64)}


def class_statistics(values, labels, class_names: Optional[Sequence[str]] = None) -> Dict[str, np.ndarray]:
    """compute_class_statistics: per class that occurs n_samples, mean, std (numpy's, ddof = 0), min, max, median, q25, q75"""
    names = list(class_names or DEFAULT_CLASS_NAMES)
    v, l = np.asarray(values), np.asarray(labels)
    keys = ("class", "n_samples", "mean", "std", "min", "max", "median", "q25", "q75")
    rows = []
    for i, name in enumerate(names):
        c = v[l == i]
        if c.size:
            rows.append((name, c.size, c.mean(), c.std(), c.min(), c.max(), np.median(c), np.percentile(c, 25), np.percentile(c, 75)))
    out = {k: np.asarray([r[j] for r in rows], dtype=(str if j == 0 else np.int64 if j == 1 else np.float64)) for j, k in enumerate(keys)}
    return out


def betainc(a: float, b: float, x: float) -> float:
    """The regularised incomplete beta function I_x(a, b) in fp64: the continued fraction of DLMF 8.17.22 evaluated by the modified
    Lentz algorithm, on x or through I_x(a, b) = 1 - I_{1-x}(b, a) on whichever side converges fast (x < (a + 1) / (a + b + 2))."""
    if not (a > 0 and b > 0) or not (0.0 <= x <= 1.0):
        return float("nan")
    if x == 0.0 or x == 1.0:
        return x
    if x > (a + 1.0) / (a + b + 2.0):
        return 1.0 - betainc(b, a, 1.0 - x)
    front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x)) / a
    tiny = 1e-300
    c, d = 1.0, 1.0 - (a + b) * x / (a + 1.0)
    d = 1.0 / (d if abs(d) > tiny else tiny)
    f = d
    for m in range(1, 1000):
        num = m * (b - m) * x / ((a + 2 * m - 1.0) * (a + 2 * m))
        d = 1.0 + num * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + num / c
        c = c if abs(c) > tiny else tiny
        f *= d * c
        num = -(a + m) * (a + b + m) * x / ((a + 2 * m) * (a + 2 * m + 1.0))
        d = 1.0 + num * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + num / c
        c = c if abs(c) > tiny else tiny
        delta = d * c
        f *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return front * f


def f_oneway(*groups):
    """One-way ANOVA: (F, p) with p = I_{d2 / (d2 + d1 F)}(d2 / 2, d1 / 2), the upper tail of the F distribution.  The sums of
    squares are taken about the grand mean, as scipy.stats.f_oneway takes them."""
    gs = [np.asarray(g, np.float64) for g in groups]
    alld = np.concatenate(gs)
    n, k = alld.size, len(gs)
    alld = alld - alld.mean()
    off, parts = 0, []
    for g in gs:
        parts.append(alld[off:off + g.size])
        off += g.size
    corr = alld.sum() ** 2 / n
    sstot = (alld * alld).sum() - corr
    ssbn = sum(p.sum() ** 2 / p.size for p in parts) - corr
    sswn = sstot - ssbn
    d1, d2 = k - 1, n - k
    if d2 <= 0 or sswn == 0:
        return (float("inf") if ssbn > 0 else float("nan")), (0.0 if ssbn > 0 else float("nan"))
    F = (ssbn / d1) / (sswn / d2)
    return float(F), betainc(d2 / 2.0, d1 / 2.0, d2 / (d2 + d1 * F))


def ttest_ind(a, b):
    """Student's two-sided t-test with pooled variance: (t, p), p = I_{df / (df + t^2)}(df / 2, 1 / 2)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n1, n2 = a.size, b.size
    df = n1 + n2 - 2
    if df <= 0:
        return float("nan"), float("nan")
    v1 = a.var(ddof=1) if n1 > 1 else 0.0
    v2 = b.var(ddof=1) if n2 > 1 else 0.0
    svar = ((n1 - 1) * v1 + (n2 - 1) * v2) / df
    den = math.sqrt(svar * (1.0 / n1 + 1.0 / n2))
    if den == 0:
        return float("nan"), float("nan")
    t = float((a.mean() - b.mean()) / den)
    return t, betainc(df / 2.0, 0.5, df / (df + t * t))


def statistical_tests_by_class(values, labels, class_names: Optional[Sequence[str]] = None) -> Dict[str, np.ndarray]:
    """statistical_tests_by_class (error_analysis.py:471-557) with the reference's choices: one-way ANOVA over the classes that
    occur with eta squared, then the pairwise pooled-variance two-sided t-tests (0, 1), (0, 2), (1, 2) with Cohen's d on np.var
    (ddof = 0) and Bonferroni's alpha = 0.05 / 3; the same `comparison` and `effect_size` strings.  Fewer than two classes with
    data: no rows."""
    names = list(class_names or DEFAULT_CLASS_NAMES)
    v, l = np.asarray(values, np.float64), np.asarray(labels)
    groups = {name: v[l == i] for i, name in enumerate(names)}
    rows = []
    if sum(g.size > 0 for g in groups.values()) >= 2:
        gv = [groups[n] for n in names if groups[n].size > 0]
        F, p = f_oneway(*gv)
        gm = v.mean()
        ssb = sum(g.size * (g.mean() - gm) ** 2 for g in gv)
        sst = ((v - gm) ** 2).sum()
        eta = ssb / sst if sst > 0 else 0
        rows.append(("ANOVA (all classes)", F, p, bool(p < 0.05), f"eta^2 = {eta:.3f}"))
        comparisons = [(0, 1), (0, 2), (1, 2)]
        alpha = 0.05 / len(comparisons)
        for i, j in comparisons:
            if i >= len(names) or j >= len(names):
                continue
            gi, gj = groups[names[i]], groups[names[j]]
            if gi.size == 0 or gj.size == 0:
                continue
            t, p = ttest_ind(gi, gj)
            pooled = np.sqrt((np.var(gi) + np.var(gj)) / 2)
            d = (np.mean(gi) - np.mean(gj)) / pooled if pooled > 0 else 0.0
            rows.append((f"{names[i]} vs {names[j]}", t, p, bool(p < alpha), f"Cohen's d = {d:.3f}"))
    return {"comparison": np.asarray([r[0] for r in rows], dtype=str), "statistic": np.asarray([r[1] for r in rows], np.float64),
            "p_value": np.asarray([r[2] for r in rows], np.float64), "significant": np.asarray([r[3] for r in rows], bool),
            "effect_size": np.asarray([r[4] for r in rows], dtype=str)}


# ---------------------------------------------------------------------------------------------------------------
# python -m eyegaze_multimodal_amd.gaze_analysis --config YAML --checkpoint CKPT --output-dir OUT [--raw]
# ---------------------------------------------------------------------------------------------------------------
def write_csv(path, columns: Dict[str, Sequence]) -> None:
    """a dict of equally long columns as a CSV file (what DataFrame.to_csv(index=False) writes of them)"""
    import csv
    keys = list(columns)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(keys)
        for row in zip(*[np.asarray(columns[k]).tolist() for k in keys]):
            w.writerow(row)


def main(argv=None):
    import argparse
    from pathlib import Path
    from .train_art import load_config
    from .train_multimodal_fuzzy_fusion import build_from_config, build_loaders
    ap = argparse.ArgumentParser(description="Per-sample and per-pair analysis tables of a trained multimodal model (MI355X HIP)")
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--checkpoint", type=str, required=True, help="best_model.pt of train_multimodal_fuzzy_fusion")
    ap.add_argument("--output-dir", type=str, required=True)
    ap.add_argument("--raw", action="store_true", help="spatial table on ToTensor-only images (v / 255) instead of the normalised ones")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("gaze_analysis (HIP) needs an MI355X: there is no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    out = Path(args.output_dir)
    out.mkdir(parents=True, exist_ok=True)
    ck = torch.load(args.checkpoint, map_location="cpu", weights_only=False)      # checkpoint_dict's keys, written by the trainer
    config = load_config(args.config)
    _, val_ld, images = build_loaders(config, device, out)
    run = dict(config, training=dict(config["training"], steps_per_epoch=1), data=dict(config["data"]))
    run["data"].setdefault("num_classes", (config.get("model") or {}).get("num_classes", 3))
    trainer = build_from_config(run, device)
    trainer.model.load_state_dict(ck["model_state_dict"])
    names = list(config["data"].get("class_names") or DEFAULT_CLASS_NAMES)
    pred = predict_multimodal(trainer, val_ld)
    win_pair = val_ld.eeg.store.win_pair[val_ld.eeg._order_dev.to(torch.int64)]   # the pair of every sample, in the walk's order
    yt, yp, prob = pred["y_true"], pred["y_pred"], pred["y_prob"]
    cols = {"true_label": yt, "true_label_name": _names(yt, names), "pred_label": yp, "pred_label_name": _names(yp, names),
            "correct": yt == yp, "confidence": prob.max(axis=1)}
    cols.update({f"prob_{n}": prob[:, i] for i, n in enumerate(names)})
    cols.update(alpha=pred["alpha"].mean(axis=1), pair_id=win_pair.cpu().numpy())
    write_csv(out / "predictions.csv", cols)
    write_csv(out / "pair_stats.csv", pair_performance(win_pair, torch.from_numpy(yt).to(device), torch.from_numpy(yp).to(device)))
    spatial = spatial_sensitivity(images, val_ld.pair_img, win_pair, yp, yt, names, normalised=not args.raw)
    write_csv(out / "spatial_analysis.csv", spatial)
    cs, ts = {}, {}
    for metric in ("distance", "overlap"):
        for k, v in class_statistics(spatial[metric], spatial["label"], names).items():
            cs.setdefault(k, []).extend(v.tolist())
        for k, v in statistical_tests_by_class(spatial[metric], spatial["label"], names).items():
            ts.setdefault(k, []).extend(v.tolist())
        cs.setdefault("metric", []).extend([metric] * (len(cs["class"]) - len(cs.get("metric", []))))
        ts.setdefault("metric", []).extend([metric] * (len(ts["comparison"]) - len(ts.get("metric", []))))
    write_csv(out / "class_statistics.csv", cs)
    write_csv(out / "statistical_tests.csv", ts)
    return out


if __name__ == "__main__":
    main()
