"""Attention statistics, hook route against eg_attention_stats -> profiles/attn_stats_parent_vs_change.json.

    timeout 600 python profiles/tools/attn_stats_bench.py OUT.json [--only stats] [--workloads a5 long]

Synthetic windows (data.randn_windows), bf16, HIP events around a whole walk of the windows that ends in a synchronise; the two
routes alternate, three repeats after one warm-up walk each:
  (a) hook   what a tree without attention_statistics offers: a forward hook on cross_attn.cross_attn.dropout copies both
             directions' [B, H, S, S] probabilities to the host (eg_attention*_probs writes them), and the host takes the mean over
             heads and directions, the batch sum and every sample's diagonal, as eeg_metrics.py:503-545 does;
  (b) stats  predict.attention_statistics.
Workloads: a5 = bench.py's a5 model at B = 128 (256 windows); long = the cfg3 model at T = 8192 (S = 513), B = 16 (32 windows), where
the hook route's probabilities still fit.  Also: peak device memory of each route above what is resident before it
(torch.cuda.max_memory_allocated), the largest difference between the two routes' results, and the new kernel's arithmetic.
--only stats runs route (b) alone, for a kernel trace in a run of its own."""
import argparse
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve()
sys.path.insert(0, str(HERE.parent.parent.parent))

SHAPES = {"a5": dict(workload="a5", T=1024, B=128, N=256), "long": dict(workload="cfg3", T=8192, B=16, N=32)}


def hook_route(torch, np, model, x1, x2, labels, B):
    seen = []
    h = model.cross_attn.cross_attn.dropout.register_forward_hook(lambda m, i, o: seen.append(i[0].detach().cpu()))
    total, diags, count = None, [], 0
    try:
        for i in range(0, x1.shape[0], B):
            seen.clear()
            model.predict(x1[i:i + B], x2[i:i + B])
            avg = (seen[0].mean(dim=1) + seen[1].mean(dim=1)) / 2.0
            total = avg.sum(dim=0) if total is None else total + avg.sum(dim=0)
            count += avg.shape[0]
            diags += [torch.diagonal(avg[j]).numpy() for j in range(avg.shape[0])]
    finally:
        h.remove()
    return (total / count).numpy(), np.stack(diags)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--only", default=None, choices=[None, "stats"])
    ap.add_argument("--workloads", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench import WORKLOADS
    from eyegaze_multimodal_amd import DualEEGTransformer
    from eyegaze_multimodal_amd.data import randn_windows
    from eyegaze_multimodal_amd.predict import attention_statistics
    if not torch.cuda.is_available():
        raise SystemExit("attn_stats_bench.py measures on the GPU: there is none here")
    dev = torch.device("cuda", 0)
    res = {}
    for name in args.workloads:
        sh = SHAPES[name]
        kw = dict(WORKLOADS[sh["workload"]][0], num_classes=3)
        Cn, T, B, N = kw.pop("in_channels", 8), sh["T"], sh["B"], sh["N"]
        torch.manual_seed(42)
        model = DualEEGTransformer(in_channels=Cn, max_len=T // 4, compute_dtype="bf16", **kw).to(dev).eval()
        x1, x2, y = randn_windows(N, Cn, T, seed=1234, num_classes=3, device=dev)
        routes = {"stats": lambda: attention_statistics(model, x1, x2, y, batch_size=B, max_samples=None)}
        if args.only is None:
            routes["hook"] = lambda: hook_route(torch, np, model, x1, x2, y, B)
        for i in range(0, N, B):                                # the engines of both batch shapes exist before any peak is taken
            model.predict(x1[i:i + B], x2[i:i + B])
        out, peak, ms = {}, {}, {k: [] for k in routes}
        for k, fn in routes.items():                            # warm-up walk: code objects, the route's own buffers; and the peak
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out[k] = fn()
            torch.cuda.synchronize()
            peak[k] = int(torch.cuda.max_memory_allocated() - base)
        for _ in range(args.repeats):
            for k, fn in routes.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ms[k].append(round(a.elapsed_time(b), 3))
        eng = model.inference_engine(B, T, dev)
        S, H, DK, NB = eng.S, model.cfg.num_heads, eng.head_dim, 2 * B
        rec = {"model": sh["workload"], "T": T, "B": B, "windows": N, "S": S, "H": H, "head_dim": DK, "dtype": "bf16",
               "ms_per_walk": ms, "peak_bytes": peak, "probabilities_bytes_per_batch": NB * H * S * S * 4,
               "stats_kernel_per_batch": {"flops": 2 * NB * H * S * S * DK, "exponentials": NB * H * S * S}}
        if "hook" in routes:
            best = {k: min(v) for k, v in ms.items()}
            rec["speedup_hook_over_stats"] = round(best["hook"] / best["stats"], 2)
            rec["max_abs_diff"] = {"mean_map": float(np.abs(out["hook"][0] - out["stats"]["mean_map"]).max()),
                                   "diagonals": float(np.abs(out["hook"][1] - out["stats"]["diagonals"]).max())}
        res[name] = rec
        print(json.dumps({name: rec}), flush=True)
        del model, routes, out
        torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
