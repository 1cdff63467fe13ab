"""
TEST INFRASTRUCTURE -- the fixture of the gaze pair analysis, written by the reference's own analyzers: its
6_Utils/error_analysis.py is loaded by path and ITS compute_gaze_distance, compute_gaze_overlap, statistical_tests_by_class,
compute_class_statistics, analyze_pair_performance, identify_hard_pairs, compute_pair_statistics, analyze_error_distribution and
compute_confusion_analysis are called; the cosine is torch's F.normalize on both arrays and the sum of products, the lines of its
compute_feature_correlation.  Runs only where the reference, torch, pandas and scipy are; the file holds pixels and numbers only.

Images (tests/gazepair_ref.py draws them): per (F, W) of SIZES six seeded images -- blob, noise, blob, noise, blob, blob -- an
all-zero and a constant one; PAIRS names them, among them a pair (a, a) and images shared by several pairs.  Every image is used as
the normalised tensor (ToTensor + Normalize, what the dataloader yields) and as the raw one (ToTensor alone).  Of one 224 x 224
pair only the reference's outputs are stored: its images come from the seed.
The centre of mass is a nested function of compute_gaze_distance; its values are read off the .item() calls it makes while
compute_gaze_distance(img, img) runs (four calls: cy, cx, cy, cx; none: the default branch).  The mask counts behind an IoU are
read off the three .sum() calls of compute_gaze_overlap in the same way.  Nothing of the reference is restated here.

Conditions, asserted here: every image on the centre-of-mass branch has S >= 1 and sum |g| / |S| <= 16, every image on the default
branch S <= -1 or S == 0 (gazepair_ref.well_conditioned, S exact) -- then the fp32 decision total < 1e-8 cannot differ from the
fp64 one.  The seeded images of a size are redrawn from the next seed until they hold.

Usage:  python tests/make_golden_gaze_pairs.py /path/to/reference
"""
import importlib.util
import sys
from pathlib import Path
from unittest import mock

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import gazepair_ref as R  # noqa: E402

SEED = 20261021
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILE_LIMIT = 600_000
STAT_CASES = [(90, (0.0, 0.3, 1.0), 1.0), (45, (0.0, 0.0, 0.05), 1.0), (200, (5.0, 5.5, 3.0), 2.0), (31, (0.0, 4.0, 8.0), 0.5),
              (60, (1.0, 1.2, None), 1.0)]                                    # (n, class means, sigma); None: the class is absent


def load_reference(root: Path):
    spec = importlib.util.spec_from_file_location("reference_error_analysis", root / "6_Utils" / "error_analysis.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tensors(img: np.ndarray):
    """(F, W, 3) uint8 -> the normalised and the raw (3, F, W) f32 tensors, in torch's own operations"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)      # ToTensor
    mean, std = torch.as_tensor(MEAN, dtype=torch.float32), torch.as_tensor(STD, dtype=torch.float32)
    return {"norm": t.sub(mean[:, None, None]).div(std[:, None, None]), "raw": t}


def centre_of(analyzer, t):
    """the reference's centre of mass of one tensor, read off its own .item() calls; (112, 112) when it makes none"""
    import torch
    seen, item = [], torch.Tensor.item

    def spy(self):
        v = item(self)
        seen.append(v)
        return v

    with mock.patch.object(torch.Tensor, "item", spy):
        d = analyzer.compute_gaze_distance(t, t)
    assert d == 0.0 and len(seen) in (0, 4) and seen[:2] == seen[2:], (d, seen)
    return (seen[0], seen[1], 1) if seen else (112.0, 112.0, 0)


def overlap_of(analyzer, ta, tb):
    """the reference's IoU of one pair and the counts behind it (inter, union, na, nb), read off the three .sum() calls that
    compute_gaze_overlap makes: mask_a * mask_b, mask_a, mask_b"""
    import torch
    seen, total = [], torch.Tensor.sum

    def spy(self, *a, **k):
        v = total(self, *a, **k)
        seen.append(float(v))
        return v

    with mock.patch.object(torch.Tensor, "sum", spy):
        iou = analyzer.compute_gaze_overlap(ta, tb)
    assert len(seen) == 3 and all(v == int(v) for v in seen), seen
    inter, na, nb = (int(v) for v in seen)
    return iou, (inter, na + nb - inter, na, nb)


def ok(store: np.ndarray) -> bool:
    return all(R.well_conditioned(R.image_stats(R.gray(im, tab))) for im in store for tab in R.tables().values())


def conditioned(seed: int, F: int, W: int, n: int):
    """the first seed >= `seed` whose images meet the conditions under both tables"""
    while not ok(R.seeded_images(seed, F, W, n)):
        seed += 1
    return seed


def pair_outputs(analyzer, store: np.ndarray, pairs):
    tens = [tensors(im) for im in store]
    out = {}
    for kind in ("norm", "raw"):
        cen = np.asarray([centre_of(analyzer, t[kind]) for t in tens], np.float64)
        for i, im in enumerate(store):                                         # the branch the reference took is the one S names
            st = R.image_stats(R.gray(im, R.tables()[kind]))
            assert R.well_conditioned(st) and bool(cen[i, 2]) == (st["S"] >= 1e-8), (kind, i, st["S"])
        out[f"{kind}/centres"] = cen
        out[f"{kind}/distance"] = np.asarray([analyzer.compute_gaze_distance(tens[a][kind], tens[b][kind]) for a, b in pairs], np.float64)
        both = [overlap_of(analyzer, tens[a][kind], tens[b][kind]) for a, b in pairs]
        assert all(np.float32(iou) == iou for iou, _ in both)                  # an fp32 quotient (or the literal 0.0)
        out[f"{kind}/overlap"] = np.asarray([iou for iou, _ in both], np.float32)
        out[f"{kind}/counts"] = np.asarray([c for _, c in both], np.int64)      # inter, union, na, nb
    return out


def frame(prefix: str, df, out: dict):
    out[f"{prefix}/columns"] = np.asarray(list(df.columns), dtype=str)
    for c in df.columns:
        a = df[c].to_numpy()
        if a.dtype == object:
            a = a.astype(bool) if all(isinstance(v, (bool, np.bool_)) for v in a) else a.astype(str)
        out[f"{prefix}/{c}"] = a


def statistics(ref, out: dict):
    import pandas as pd
    rng = np.random.default_rng(SEED)
    mech, err = ref.MechanismAnalyzer("early"), ref.ErrorAnalyzer()
    out["stats/n_cases"] = np.int64(len(STAT_CASES))
    for k, (n, means, sigma) in enumerate(STAT_CASES):
        present = [c for c in range(3) if means[c] is not None]
        labels = rng.choice(present, size=n)
        values = np.asarray([means[c] for c in labels]) + sigma * rng.standard_normal(n)
        out[f"stats/{k}/values"], out[f"stats/{k}/labels"] = values, labels.astype(np.int64)
        frame(f"stats/{k}/tests", mech.statistical_tests_by_class(values, labels), out)
        frame(f"stats/{k}/class", mech.compute_class_statistics(values, labels), out)
    n = 300
    y_true = rng.integers(0, 3, n)
    y_pred = y_true.copy()
    wrong = rng.choice(n, 70, replace=False)
    y_pred[wrong] = rng.integers(0, 3, 70)
    pair_ids = rng.integers(1, 14, n)
    pair_ids[pair_ids == 5] = 6                                                # an id that does not occur
    out["perf/y_true"], out["perf/y_pred"], out["perf/pair_ids"] = y_true, y_pred, pair_ids
    df = pd.DataFrame({"pair_id": pair_ids, "true_label": y_true, "pred_label": y_pred, "correct": y_true == y_pred})
    ps = err.analyze_pair_performance(df)
    frame("perf/pair_stats", ps, out)
    out["perf/hard_pairs"] = np.asarray(err.identify_hard_pairs(ps), np.int64)
    out["perf/hard_pairs_50"] = np.asarray(err.identify_hard_pairs(ps, 50), np.int64)
    summary = err.compute_pair_statistics(ps)
    out["perf/summary_keys"] = np.asarray(list(summary), dtype=str)
    out["perf/summary"] = np.asarray([float(v) for v in summary.values()], np.float64)
    frame("perf/errors", err.analyze_error_distribution(y_true, y_pred), out)
    frame("perf/confusion", err.compute_confusion_analysis(y_true, y_pred), out)


def cosines(out: dict):
    import torch
    import torch.nn.functional as F
    for D in R.COSINE_D:
        a, b = R.cosine_inputs(SEED, D)
        c1, c2 = F.normalize(torch.from_numpy(a), dim=-1), F.normalize(torch.from_numpy(b), dim=-1)
        out[f"cosine/{D}"] = (c1 * c2).sum(dim=-1).numpy()


def build(root: Path):
    ref = load_reference(root)
    analyzer = ref.MechanismAnalyzer("early")
    out = {"seed": np.int64(SEED), "sizes": np.asarray(R.SIZES, np.int64), "pairs": np.asarray(R.PAIRS, np.int32),
           "mean": np.asarray(MEAN), "std": np.asarray(STD)}
    seed = SEED
    for F, W in R.SIZES:
        seed = conditioned(seed, F, W, R.N_SEEDED)
        store = R.with_extras(R.seeded_images(seed, F, W))
        assert ok(store)
        out[f"{F}x{W}/seed"], out[f"{F}x{W}/store"] = np.int64(seed), store
        for k, v in pair_outputs(analyzer, store, R.PAIRS).items():
            out[f"{F}x{W}/{k}"] = v
        seed += 1
    F, W = R.BIG
    seed = conditioned(seed, F, W, 2)
    out["big/seed"] = np.int64(seed)
    for k, v in pair_outputs(analyzer, R.seeded_images(seed, F, W, 2), [(0, 1)]).items():
        out[f"big/{k}"] = v
    statistics(ref, out)
    cosines(out)
    return out


if __name__ == "__main__":
    out = build(Path(sys.argv[1]))
    path = REPO / "tests" / "golden" / "gaze_pairs.npz"
    np.savez_compressed(path, **out)
    assert path.stat().st_size < FILE_LIMIT, path.stat().st_size
    taken = sum(int(out[f"{F}x{W}/{k}/centres"][:, 2].sum()) for F, W in R.SIZES for k in ("norm", "raw"))
    print(f"{path.name}: {path.stat().st_size / 1e3:.0f} kB, {len(out)} arrays, {taken} centres of mass taken")
