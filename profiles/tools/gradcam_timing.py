"""Grad-CAM class means, the hook route against the device route -> profiles/gradcam_timing.json.

    timeout 900 python profiles/tools/gradcam_timing.py OUT.json [--runs 3] [--batch 128] [--windows 512] [--device-only]

bench.py's a5c32 model (C = 32), T = 1024, bf16, synthetic windows (data.randn_windows), one GPU; wall clock around a whole
analysis that ends in a synchronise; the two routes alternate, `runs` timed runs per route after one warm-up run each (which also
warms every engine shape):
  hook    the reference's compute_gradcam_batch algorithm (tests/gradcam_ref.py: gradcam_ref over hook_runner) through the hook
          contract of the HIP model: the whole training backward per batch, conv-2 a second time without its ReLU, four fp32
          [B*C, 64, Hp, Wp] tensors per batch copied to the host;
  device  predict.gradcam_statistics: eval forward, the backward cut at conv-2's output gradient, one eg_gradcam_accumulate.
Also the peak device memory of each route (torch.cuda.max_memory_allocated over a run of its own) and the largest difference of
the class means.  --device-only: two runs of the device route and nothing else (the subject of a rocprofv3 --kernel-trace run)."""
import argparse
import json
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve()
sys.path.insert(0, str(HERE.parent.parent.parent))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--windows", type=int, default=512)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench import WORKLOADS
    from eyegaze_multimodal_amd import DualEEGTransformer
    from eyegaze_multimodal_amd.data import randn_windows
    from eyegaze_multimodal_amd.predict import CLASS_NAMES, gradcam_statistics
    from tests.gradcam_ref import gradcam_ref, hook_runner
    if not torch.cuda.is_available():
        raise SystemExit("gradcam_timing.py measures on the GPU: there is none here")
    dev = torch.device("cuda", 0)
    kw = dict(WORKLOADS["a5c32"][0], num_classes=3)
    Cn, T, B, N = kw.pop("in_channels", 8), 1024, args.batch, args.windows
    torch.manual_seed(42)
    model = DualEEGTransformer(in_channels=Cn, max_len=T // 4, compute_dtype="bf16", **kw).to(dev).eval()
    x1, x2, y = randn_windows(N, Cn, T, seed=1234, num_classes=3, device=dev)
    sides = {"hook": lambda: gradcam_ref(hook_runner(model), x1, x2, y.cpu(), B, max_samples=None, names=CLASS_NAMES),
             "device": lambda: gradcam_statistics(model, x1, x2, y, batch_size=B, max_samples=None)}
    if args.device_only:
        for _ in range(2):
            sides["device"]()
            torch.cuda.synchronize()
        return
    out, peak, ms = {}, {}, {k: [] for k in sides}
    for k, fn in sides.items():                             # warm-up run: code objects, engines, buffers; and the device peak
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out[k] = fn()
        torch.cuda.synchronize()
        peak[k] = {"max_memory_allocated": torch.cuda.max_memory_allocated(), "allocated_before": base}
    for _ in range(args.runs):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append(round((time.perf_counter() - t0) * 1e3, 3))
    top = max(float(m.max()) for m in out["hook"]["class_mean"].values())
    diff = max(float(np.abs(out["hook"]["class_mean"][n] - out["device"]["class_mean"][n]).max()) for n in CLASS_NAMES)
    spread = {k: round(max(v) - min(v), 3) for k, v in ms.items()}
    rec = {"model": "a5c32", "C": Cn, "T": T, "B": B, "windows": N, "dtype": "bf16", "ms": ms, "spread_ms": spread,
           "hook_over_device": round(min(ms["hook"]) / min(ms["device"]), 3),
           "device_faster_by_more_than_the_spread": bool(min(ms["hook"]) - max(ms["device"]) > max(spread.values())),
           "peak_device_bytes": peak, "class_counts_equal": out["hook"]["class_count"] == out["device"]["class_count"],
           "class_mean_max_abs_diff_over_max": diff / top, "class_mean_max": top}
    print(json.dumps(rec), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
