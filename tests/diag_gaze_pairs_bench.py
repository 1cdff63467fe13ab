"""Diagnostic (manual, GPU box): gaze_analysis.spatial_statistics -- ONE eg_gaze_pair_stats call -- against the reference-style
per-sample loop on device tensors (the torch calls and the .item()s of compute_gaze_distance and compute_gaze_overlap,
6_Utils/error_analysis.py:277-358, sample by sample), and against the byte floor: launch 1 reads the store once, launch 2 reads each
pair's two images again.  2048 pairs over 4096 images at 224 x 224, the reference's image size.  Device events after warm-up;
prints one JSON line.  DESIGN.md §8q quotes it.

Usage:  python tests/diag_gaze_pairs_bench.py [--pairs 2048] [--images 4096] [--size 224] [--reps 20] [--loop-samples 512]"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from eyegaze_multimodal_amd import gaze as G
from eyegaze_multimodal_amd import gaze_analysis as A
from tests import gazepair_ref as R

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12          # bytes / s: the specification, and what a float4 copy reaches on this GPU


def reference_style(img_a: torch.Tensor, img_b: torch.Tensor, threshold: float = 0.1):
    """one sample as the reference computes it, on (3, H, W) device tensors: fifteen small reductions and element-wise
    launches, six host syncs"""
    def centre(t):
        gray = t.mean(dim=0)
        total = gray.sum()
        if total < 1e-8:
            return 112.0, 112.0
        h, w = gray.shape
        ys = torch.arange(h, dtype=torch.float32, device=gray.device).unsqueeze(1)
        xs = torch.arange(w, dtype=torch.float32, device=gray.device).unsqueeze(0)
        return ((gray * ys).sum() / total).item(), ((gray * xs).sum() / total).item()

    (ya, xa), (yb, xb) = centre(img_a), centre(img_b)
    distance = float(np.sqrt((ya - yb) ** 2 + (xa - xb) ** 2))
    ga, gb = img_a.mean(dim=0), img_b.mean(dim=0)
    ga = (ga - ga.min()) / (ga.max() - ga.min() + 1e-8)
    gb = (gb - gb.min()) / (gb.max() - gb.min() + 1e-8)
    ma, mb = (ga > threshold).float(), (gb > threshold).float()
    inter = (ma * mb).sum()
    union = ma.sum() + mb.sum() - inter
    return distance, (0.0 if union < 1e-8 else (inter / union).item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-samples", type=int, default=512, help="samples the per-sample loop is timed on (its time is per sample)")
    ap.add_argument("--raw", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    F = W = args.size
    base = torch.from_numpy(R.seeded_images(11, F, W, 64)).to(dev)                # heat-map blobs and noise
    gen = torch.Generator(device=dev).manual_seed(1)
    idx = torch.randint(0, 64, (args.images,), device=dev, generator=gen)
    shift = torch.randint(0, 24, (args.images, 1, 1, 1), device=dev, generator=gen, dtype=torch.int32)
    data = (base[idx].to(torch.int32) + shift).clamp_(0, 255).to(torch.uint8).contiguous()      # 4096 distinct images
    store = G.GazeImageStore(data)
    pairs = torch.randint(0, args.images, (args.pairs, 2), device=dev, generator=gen, dtype=torch.int32)
    normalised = not args.raw

    for _ in range(3):
        st = A.spatial_statistics(store, pairs, normalised)
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            st = A.spatial_statistics(store, pairs, normalised)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / args.reps)
    ms = float(np.median(times))
    image_bytes = 3 * F * W
    nbytes = args.images * image_bytes + 2 * args.pairs * image_bytes

    # the per-sample loop: the tensors a dataloader would hand over (eg_gaze_batch, outside the timing), then sample by sample
    n = min(args.loop_samples, args.pairs)
    ar = torch.arange(n, dtype=torch.int32, device=dev)
    table = store.norm
    if args.raw:
        store.norm = A.raw_table().to(dev)
    _, _, rgb1, rgb2 = store.batch(pairs[:n].contiguous(), ar, ar, 0, n, rgb=True)
    store.norm = table
    for i in range(8):
        reference_style(rgb1[i], rgb2[i])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    loop = [reference_style(rgb1[i], rgb2[i]) for i in range(n)]
    e1.record()
    torch.cuda.synchronize()
    loop_ms = e0.elapsed_time(e1) / n * args.pairs
    # the two routes agree (the loop's sums are fp32 in torch's order: the bound of tests/gazepair_ref.py is not applied here)
    d, o = st["distance"][:n].cpu().numpy(), st["overlap"][:n].cpu().numpy()
    agree = {"overlap_equal": int(sum(np.float32(o[i]) == np.float32(loop[i][1]) for i in range(n))), "of": n,
             "overlap_max_abs_diff": float(max(abs(o[i] - loop[i][1]) for i in range(n))),
             "distance_max_abs_diff": float(max(abs(d[i] - loop[i][0]) for i in range(n)))}
    print(json.dumps({"pairs": args.pairs, "images": args.images, "size": args.size, "table": "raw" if args.raw else "normalised",
                      "spatial_statistics_ms": round(ms, 4), "spread_ms": [round(min(times), 4), round(max(times), 4)],
                      "bytes": nbytes, "achieved_GBps": round(nbytes / ms / 1e6, 1),
                      "floor_ms_at_8.0TBps": round(nbytes / HBM_PEAK * 1e3, 4), "share_of_floor": round(nbytes / HBM_PEAK * 1e3 / ms, 3),
                      "floor_ms_at_copy_rate_6.29TBps": round(nbytes / HBM_COPY * 1e3, 4),
                      "reference_style_loop_ms": round(loop_ms, 1), "loop_timed_on_samples": n,
                      "speedup": round(loop_ms / ms, 1), "agreement": agree}))


if __name__ == "__main__":
    main()
