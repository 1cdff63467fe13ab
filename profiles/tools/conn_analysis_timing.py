"""Connectivity analyses, hook routes against the fused routes -> profiles/conn_analysis_timing.json.

    timeout 900 python profiles/tools/conn_analysis_timing.py OUT.json [--workloads a5c32 a5] [--runs 2]

Synthetic windows (data.randn_windows), bf16, one GPU, wall clock around a whole analysis that ends in a synchronise; the two sides
of each comparison alternate, `runs` timed runs per side after one warm-up run each:
  (a) frequency sensitivity
      hook   what a tree without frequency_sensitivity offers: seven predict_windows walks, six of them with the reference's
             FrequencyMaskHook (eeg_metrics.py:318-349) registered on ibs_matrix_generator;
      fused  predict.frequency_sensitivity: one walk, one InferenceEngine.forward_band_masks call per batch.
  (b) class means
      hook   the reference's capture hook (eeg_metrics.py:195-198) copies every batch's [B, 6, nfeat, C, C] matrices to the host,
             which keeps all of them and takes compute_mean_ibs_by_class's numpy means;
      fused  predict.connectivity_statistics.
      Also the peak host bytes of both (tracemalloc: numpy's allocations are traced).
Workloads: bench.py's a5c32 (C = 32) and a5 (C = 8) models at B = 256, T = 1024, 512 windows.  The bar of (a): the fused walk is
not slower than the hook walks by more than the spread between the hook side's own runs."""
import argparse
import json
import sys
import time
import tracemalloc
from pathlib import Path

HERE = Path(__file__).resolve()
sys.path.insert(0, str(HERE.parent.parent.parent))

SHAPES = {"a5c32": dict(workload="a5c32", T=1024, B=256, N=512), "a5": dict(workload="a5", T=1024, B=256, N=512)}


def hook_sensitivity(model, x1, x2, y, B, predict_windows, metric):
    out = {}
    for band in (None, 0, 1, 2, 3, 4, 5):
        def mask(m, i, o, band=band):
            o[:, band, :, :, :] = 0
            return o
        h = model.ibs_matrix_generator.register_forward_hook(mask) if band is not None else None
        try:
            out[band] = metric(predict_windows(model, x1, x2, y, batch_size=B)["confusion"])
        finally:
            if h is not None:
                h.remove()
    return out


def hook_class_means(np, model, x1, x2, y, B, names):
    seen = []
    h = model.ibs_matrix_generator.register_forward_hook(lambda m, i, o: seen.append(o.detach().cpu().numpy()))
    try:
        for i in range(0, x1.shape[0], B):
            model.predict(x1[i:i + B], x2[i:i + B])
    finally:
        h.remove()
    matrices, labels = np.concatenate(seen, axis=0), y.cpu().numpy()
    return {n: (matrices[labels == c].mean(axis=0) if (labels == c).any() else np.zeros_like(matrices[0])) for c, n in enumerate(names)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--workloads", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench import WORKLOADS
    from eyegaze_multimodal_amd import DualEEGTransformer
    from eyegaze_multimodal_amd.data import randn_windows
    from eyegaze_multimodal_amd.predict import (BAND_NAMES, CLASS_NAMES, band_metrics_from_confusion, connectivity_statistics,
                                                frequency_sensitivity, predict_windows)
    if not torch.cuda.is_available():
        raise SystemExit("conn_analysis_timing.py measures on the GPU: there is none here")
    dev = torch.device("cuda", 0)
    res = {}
    for name in args.workloads:
        sh = SHAPES[name]
        kw = dict(WORKLOADS[sh["workload"]][0], num_classes=3)
        Cn, T, B, N = kw.pop("in_channels", 8), sh["T"], sh["B"], sh["N"]
        torch.manual_seed(42)
        model = DualEEGTransformer(in_channels=Cn, max_len=T // 4, compute_dtype="bf16", **kw).to(dev).eval()
        x1, x2, y = randn_windows(N, Cn, T, seed=1234, num_classes=3, device=dev)
        sides = {"sens_hook": lambda: hook_sensitivity(model, x1, x2, y, B, predict_windows, band_metrics_from_confusion),
                 "sens_fused": lambda: frequency_sensitivity(model, x1, x2, y, batch_size=B),
                 "means_hook": lambda: hook_class_means(np, model, x1, x2, y, B, CLASS_NAMES),
                 "means_fused": lambda: connectivity_statistics(model, x1, x2, y, batch_size=B)}
        out, host_peak, ms = {}, {}, {k: [] for k in sides}
        for k, fn in sides.items():                             # warm-up run: code objects, engines, buffers; and the host peak
            torch.cuda.synchronize()
            tracemalloc.start()
            out[k] = fn()
            torch.cuda.synchronize()
            host_peak[k] = tracemalloc.get_traced_memory()[1]
            tracemalloc.stop()
        for _ in range(args.runs):
            for k, fn in sides.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[k].append(round((time.perf_counter() - t0) * 1e3, 3))
        fused = out["sens_fused"]
        same = (fused["baseline"] == out["sens_hook"][None]
                and all(fused["sensitivity"][n] == out["sens_hook"][b] for b, n in enumerate(BAND_NAMES)))
        diff = max(float(np.abs(out["means_hook"][n] - out["means_fused"]["class_mean"][n]).max()) for n in CLASS_NAMES)
        best = {k: min(v) for k, v in ms.items()}
        rec = {"model": sh["workload"], "C": Cn, "T": T, "B": B, "windows": N, "dtype": "bf16", "ms": ms,
               "sensitivity_hook_over_fused": round(best["sens_hook"] / best["sens_fused"], 3),
               "sensitivity_hook_spread_ms": round(max(ms["sens_hook"]) - min(ms["sens_hook"]), 3),
               "sensitivity_fused_not_slower": bool(min(ms["sens_fused"]) <= min(ms["sens_hook"]) + max(ms["sens_hook"]) - min(ms["sens_hook"])),
               "sensitivity_metrics_equal": bool(same),
               "means_hook_over_fused": round(best["means_hook"] / best["means_fused"], 3),
               "means_host_peak_bytes": {"hook": host_peak["means_hook"], "fused": host_peak["means_fused"]},
               "means_max_abs_diff": diff}
        res[name] = rec
        print(json.dumps({name: rec}), flush=True)
        del model, sides, out
        torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
