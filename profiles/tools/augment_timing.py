"""Window augmentation timings (eg_window_augment) -> profiles/augment_timing.json.

    python profiles/tools/augment_timing.py OUT.json

For cfg3 (B = 256, C = 8, T = 1024) and a5c32 (C = 32), bf16:
  kernels   eg_window_augment alone with the lab recipe (noise 0.05, channel dropout 0.2, 2 masks of <= 50 samples) and with
            noise only, and eg_window_normalize at the same shape as the yardstick: HIP events around 200 back-to-back launches
            (hot loop: the working set, 34 MB at C = 8 and 134 MB at C = 32, fits the 256 MiB Infinity Cache), bytes = one read
            and one write of both players' windows;
  steps     ms per training step (forward + backward + clip + AdamW, eager) over 100 steps after 20 warm-up, with and without
            the recipe, the two versions alternating over 3 rounds so that drift hits both alike.
A run that finds no GPU fails."""
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))

RECIPE = dict(gaussian_noise_std=0.05, channel_dropout_prob=0.2, time_mask_max_length=50, time_mask_num=2)


def kernels(torch, eng, x1, x2, reps=200, warm=20):
    from eyegaze_multimodal_amd._lib import call, ptr
    B, C, T = x1.shape
    o1, o2 = torch.empty_like(x1), torch.empty_like(x2)
    raw = torch.randn(B, 2, C, T, device=x1.device)
    st = eng.st_ptr
    launches = {
        "augment_recipe": lambda: call("eg_window_augment", ptr(x1), ptr(x2), ptr(o1), ptr(o2), B, C, T, 0.05, 0.2, 2, 50, st, 0),
        "augment_noise_only": lambda: call("eg_window_augment", ptr(x1), ptr(x2), ptr(o1), ptr(o2), B, C, T, 0.05, 0.0, 0, 0, st, 0),
        "augment_masks_only": lambda: call("eg_window_augment", ptr(x1), ptr(x2), ptr(o1), ptr(o2), B, C, T, 0.0, 0.2, 2, 50, st, 0),
        "window_normalize": lambda: call("eg_window_normalize", ptr(raw), ptr(o1), ptr(o2), B, C, T, 0, 0),
    }
    nbytes = 2 * 2 * B * C * T * 4          # both players, one read + one write (the masks-only launch reads less: see the row)
    out = {}
    with torch.cuda.stream(torch.cuda.default_stream()):
        for name, fn in launches.items():
            for _ in range(warm):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            us = a.elapsed_time(b) * 1e3 / reps
            out[name] = {"us": round(us, 2), "bytes": nbytes, "TB_per_s": round(nbytes / us / 1e6, 3)}
    return out


def steps(torch, model, eng, opt, x1, x2, y, one, n=100, warm=20, rounds=3):
    from eyegaze_multimodal_amd import WindowAugmentation
    ibs = one if model.cfg.use_ibs else None
    count = [0]

    def run(k):
        for _ in range(k):
            count[0] += 1
            opt.begin_step(eng, seed=1000 + count[0])
            eng.forward(x1, x2, y, train=True)
            eng.backward(gloss=one, gloss_ibs=ibs)
            opt.step(eng)

    def timed(aug):
        model.augmentation = aug
        run(warm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    res = {"off_ms": [], "recipe_ms": []}
    for _ in range(rounds):
        res["off_ms"].append(round(timed(None), 4))
        res["recipe_ms"].append(round(timed(WindowAugmentation(**RECIPE)), 4))
    model.augmentation = None
    res["off_ms_median"], res["recipe_ms_median"] = sorted(res["off_ms"])[rounds // 2], sorted(res["recipe_ms"])[rounds // 2]
    res["delta_percent_of_step"] = round(100.0 * (res["recipe_ms_median"] - res["off_ms_median"]) / res["off_ms_median"], 3)
    return res


def main(out_path):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("augment_timing.py measures on the GPU; none found")
    from profiles.tools.accum_timing import setup
    res = {"recipe": RECIPE, "dtype": "bf16", "B": 256, "T": 1024, "steps": 100, "warmup": 20, "rounds": 3, "kernel_reps": 200}
    for workload in ("cfg3", "a5c32"):
        torch_, model, eng, opt, (x1, x2, y), one = setup(workload=workload)
        res[workload] = {"shape": list(x1.shape), "kernels": kernels(torch, eng, x1, x2),
                         "steps": steps(torch, model, eng, opt, x1, x2, y, one)}
        print(json.dumps({workload: res[workload]}), flush=True)
        del model, eng, opt
        torch.cuda.empty_cache()
    Path(out_path).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "augment_timing.json")
