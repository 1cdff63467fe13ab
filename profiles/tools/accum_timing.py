"""Gradient accumulation timings on the bench workload (cfg3, bf16, B = 256 by default) -> profiles/accum_timing.json.

  python profiles/tools/accum_timing.py OUT.json            loops (fwd+bwd alone, k = 1 step, k = 4 group) + kernels in a hot loop
  python profiles/tools/accum_timing.py --trace-run         the k = 4 loop alone, to be run under `rocprofv3 --kernel-trace --stats`
  python profiles/tools/accum_timing.py --from-trace DIR    per-kernel averages of that trace (accumulate, adamw, sqnorm)
Wall times are host clocks around a synchronised region of many steps; kernel times are HIP events (hot loop: the 27 MB buffers
then sit in the Infinity Cache) and the profiler's kernel trace (inside real steps: the buffers come from HBM)."""
import csv
import glob
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))


def setup(B=256, dtype="bf16", workload="cfg3"):
    import torch
    from bench import WORKLOADS
    from eyegaze_multimodal_amd import DualEEGTransformer, HipAdamW
    from eyegaze_multimodal_amd.data import randn_windows
    dev = torch.device("cuda", 0)
    kw, _ = WORKLOADS[workload]
    kw = dict(kw, num_classes=3)
    C = kw.pop("in_channels", 8)
    torch.manual_seed(42)
    model = DualEEGTransformer(in_channels=C, max_len=256, compute_dtype=dtype, **kw).to(dev)
    model.train()
    eng = model.engine(B, 1024, dev)
    opt = HipAdamW(model, lr=1e-4, weight_decay=0.01)
    x = randn_windows(B, C, 1024, seed=1234, num_classes=3, device=dev)
    return torch, model, eng, opt, x, torch.ones(1, device=dev)


def loops(out_path, steps=60, warmup=12, rounds=3):
    torch, model, eng, opt, (x1, x2, y), one = setup()
    ibs = one if model.cfg.use_ibs else None
    K = 4

    def fwd_bwd(i):
        opt.begin_step(eng, seed=1000 + i, advance=(i == 0))
        eng.forward(x1, x2, y, train=True)
        eng.backward(gloss=one, gloss_ibs=ibs)

    def k1(i):
        opt.begin_step(eng, seed=1000 + i)
        eng.forward(x1, x2, y, train=True)
        eng.backward(gloss=one, gloss_ibs=ibs)
        opt.step(eng)

    def k4(i):                                        # one MICRO-step per call; every 4th ends in the optimiser step
        j = i % K
        opt.begin_step(eng, seed=1000 + i, grad_scale=1.0 / (j + 1), advance=(j == 0))
        eng.forward(x1, x2, y, train=True)
        eng.backward(gloss=one, gloss_ibs=ibs)
        eng.accumulate(first=(j == 0), norm=(j == K - 1))
        if j == K - 1:
            opt.step(eng, accumulated=True, norm_ready=True)

    def timed(fn):
        for i in range(warmup):
            fn(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            fn(warmup + i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    k1(0)
    res = {"fwd_bwd_ms": [], "k1_step_ms": [], "k4_micro_step_ms": []}
    for _ in range(rounds):                           # interleaved: drift hits every version alike
        res["fwd_bwd_ms"].append(timed(fwd_bwd))
        res["k1_step_ms"].append(timed(k1))
        res["k4_micro_step_ms"].append(timed(k4))
    # kernels alone, hot loop, HIP events
    from eyegaze_multimodal_amd._lib import call, ptr
    fp = model._flat
    n = fp.total
    acc, g, part = fp.accumulator(), fp.grad, eng.g["sqpart"]
    g.normal_()
    m, v = torch.zeros_like(g), torch.zeros_like(g)
    st = eng.st_ptr
    kernels = {
        "accumulate_first": (lambda: call("eg_grad_accumulate", ptr(acc), ptr(g), n, 1, 0, 0, 0), 8),
        "accumulate_add": (lambda: call("eg_grad_accumulate", ptr(acc), ptr(g), n, 0, 0, 0, 0), 12),
        "accumulate_add_norm": (lambda: call("eg_grad_accumulate", ptr(acc), ptr(g), n, 0, ptr(part), 1024, 0), 12),
        "grad_sqnorm": (lambda: call("eg_grad_sqnorm", ptr(g), n, ptr(part), 1024, 0), 4),
        "adamw": (lambda: call("eg_adamw", ptr(fp.flat), ptr(g), ptr(m), ptr(v), n, 0.9, 0.999, 1e-8, 0.01, st, 0), 28),
    }
    hot = {}
    with torch.cuda.stream(torch.cuda.default_stream()):
        for name, (fn, bpe) in kernels.items():
            for _ in range(10):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(100):
                fn()
            b.record()
            torch.cuda.synchronize()
            us = a.elapsed_time(b) * 10.0
            hot[name] = {"us": round(us, 2), "bytes_per_element": bpe, "TB_per_s": round(n * bpe / us / 1e6, 3)}
    res.update(elements=n, hot_loop_kernels=hot, workload="cfg3 bf16 B=256 T=1024", steps=steps, rounds=rounds)
    Path(out_path).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


def trace_run(groups=10):
    torch, model, eng, opt, (x1, x2, y), one = setup()
    for i in range(4 * groups):
        j = i % 4
        opt.begin_step(eng, seed=1000 + i, grad_scale=1.0 / (j + 1), advance=(j == 0))
        eng.forward(x1, x2, y, train=True)
        eng.backward(gloss=one)
        eng.accumulate(first=(j == 0), norm=(j == 3))
        if j == 3:
            opt.step(eng, accumulated=True, norm_ready=True)
    torch.cuda.synchronize()
    print(model._flat.total)


def from_trace(d, n):
    f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
    agg = {}
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"]
        for key in ("grad_accumulate_kernel<true, false>", "grad_accumulate_kernel<false, false>",
                    "grad_accumulate_kernel<false, true>", "adamw_kernel", "sqnorm_partial_kernel"):
            if key in name:
                agg.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    bpe = {"grad_accumulate_kernel<true, false>": 8, "grad_accumulate_kernel<false, false>": 12,
           "grad_accumulate_kernel<false, true>": 12, "adamw_kernel": 28, "sqnorm_partial_kernel": 4}
    out = {}
    for k, v in agg.items():
        v = sorted(v)
        med = v[len(v) // 2]
        out[k] = {"launches": len(v), "median_us": round(med, 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2),
                  "TB_per_s_at_median": round(n * bpe[k] / med / 1e6, 3)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if "--trace-run" in sys.argv:
        trace_run()
    elif "--from-trace" in sys.argv:
        i = sys.argv.index("--from-trace")
        from_trace(sys.argv[i + 1], int(sys.argv[i + 2]))
    else:
        loops(sys.argv[1] if len(sys.argv) > 1 else "accum_timing.json")
