"""Exact t-SNE on the device -> profiles/tsne_timing.json.

    timeout 600 python profiles/tools/tsne_timing.py OUT.json [--sizes 2048 8192] [--dim 768] [--iters 200] [--runs 5]

Per N (three Gaussian clusters in `dim` dimensions), by HIP events after a warm-up, five runs each, every run listed:
  stages       eg_tsne_sqdist, eg_tsne_affinities, eg_tsne_joint, one call each
  iteration    `iters` iterations of eg_tsne_gradient + eg_tsne_update without stats, per iteration; and eg_tsne_gradient alone
               with stats (the 50th iteration's)
  stream       a device-to-device copy of the N x N float32 matrix (read + write) and the time to read N^2 * 4 bytes once at that
               copy's rate: the floor of an iteration, which streams P once
  tsne         embedding.tsne at 1000 iterations from the PCA init by wall clock, the final sync included (N <= 4096 only)"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve()
sys.path.insert(0, str(HERE.parent.parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from eyegaze_multimodal_amd import _lib as L
    from eyegaze_multimodal_amd import embedding as E
    from eyegaze_multimodal_amd._lib import call, ptr
    if not torch.cuda.is_available():
        raise SystemExit("tsne_timing.py measures on the GPU: there is none here")
    st = torch.cuda.current_stream().cuda_stream

    def timed(fn, runs=args.runs):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return {"median_ms": statistics.median(out), "runs_ms": out}

    result = {"device": torch.cuda.get_device_name(0), "dim": args.dim, "iters": args.iters, "sizes": {}}
    for N in args.sizes:
        rng = np.random.default_rng(N)
        centres = 3.0 * rng.standard_normal((3, args.dim))
        X = torch.from_numpy((centres[rng.integers(0, 3, N)] + rng.standard_normal((N, args.dim))).astype(np.float32)).cuda()
        dist, cond, P = (torch.empty(N, N, device="cuda") for _ in range(3))
        beta, steps = torch.empty(N, device="cuda", dtype=torch.float64), torch.empty(N, device="cuda", dtype=torch.int32)
        ws = torch.empty(L.tsne_workspace_bytes(N), dtype=torch.uint8, device="cuda")
        r = {}
        r["sqdist"] = timed(lambda: call("eg_tsne_sqdist", ptr(X), N, args.dim, ptr(dist), st))
        r["affinities"] = timed(lambda: call("eg_tsne_affinities", ptr(dist), N, 30.0, ptr(cond), ptr(beta), ptr(steps), st))
        r["affinities"]["max_steps"] = int(steps.max())
        r["joint"] = timed(lambda: call("eg_tsne_joint", ptr(cond), N, ptr(ws), ws.numel(), ptr(P), st))
        r["copy_n2_f32"] = timed(lambda: cond.copy_(P))
        rate = 2 * 4.0 * N * N / (r["copy_n2_f32"]["median_ms"] * 1e-3)
        r["copy_bytes_per_s"] = rate
        r["stream_p_once_ms"] = 4.0 * N * N / rate * 1e3
        d = E.Descent(P, E.pca_init(X))
        lr = max(N / 12.0 / 4.0, 50.0)

        def iterations():
            for _ in range(args.iters):
                d.step(12.0, 0.5, lr, False)
        it = timed(iterations)
        r["iteration"] = {"median_ms": it["median_ms"] / args.iters, "runs_ms": [v / args.iters for v in it["runs_ms"]]}
        r["gradient_only"] = timed(lambda: call("eg_tsne_gradient", ptr(d.Y), ptr(P), 1.0, N, ptr(ws), ws.numel(), ptr(d.grad), 0, st))
        r["gradient_with_kl"] = timed(lambda: call("eg_tsne_gradient", ptr(d.Y), ptr(P), 1.0, N, ptr(ws), ws.numel(), ptr(d.grad),
                                                   ptr(d.stats), st))
        r["update_only"] = timed(lambda: call("eg_tsne_update", ptr(d.Y), ptr(d.update), ptr(d.gains), ptr(d.grad), N, 0.5, lr, 0.01, 0, st))
        if N <= 4096:
            walls = []
            for _ in range(3):
                torch.cuda.synchronize()
                t = time.perf_counter()
                Y, kl, n_iter = E.tsne(X, max_iter=1000)
                Y.cpu()
                walls.append(time.perf_counter() - t)
            r["tsne_1000"] = {"wall_s": walls, "kl_divergence": kl, "n_iter": n_iter}
        result["sizes"][str(N)] = r
        print(N, json.dumps(r), flush=True)
        del dist, cond, P, d
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
