"""Entropy analysis on the device -> profiles/entropy_timing.json.

    timeout 900 python profiles/tools/entropy_timing.py OUT.json [--runs 5] [--recordings 1000] [--images 10000]
    python profiles/tools/entropy_timing.py OUT.json --cpu-reference MACHINE [--cpu-recordings 3] [--cpu-images 200]

Device side (one GPU):
  eeg     `recordings` synthetic raw-like recordings of C = 32 x 3250 samples through entropy.spectral_entropy, and one alone
  gaze    `images` synthetic heat maps of 224 x 224 x 3 uint8 through entropy.spatial_entropy, and one alone
five runs after a warm-up, every run listed: the whole call by wall clock (host arrays in, the copy-back of the results as its one
sync) and every entry point by HIP events around its calls, summed over the call.  Each kernel's floor is stated next to it: the
bytes it reads over the HBM rate (the images are read twice: the second pass may be served by the 256 MB last-level cache), and for
the filter the sequential walk of one lane per row.
CPU side (--cpu-reference, where the reference tree and scipy exist): the reference's own compute() loops on the same kind of
input in one thread; stored under cpu_reference/MACHINE.  Both sides merge into the same file."""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve()
sys.path.insert(0, str(HERE.parent.parent.parent))

HBM_BYTES_PER_S = 8.0e12            # MI355X HBM3E
C, SAMPLES, SIDE = 32, 3250, 224


def raw_recordings(rng, n):
    import numpy as np
    t = np.arange(SAMPLES) / 250.0
    out = []
    for _ in range(n):
        x = rng.uniform(-4000, 4000, (C, 1)) + np.cumsum(rng.normal(0, 2.0, (C, SAMPLES)), axis=1) + rng.normal(0, 5.0, (C, SAMPLES))
        for f, amp in ((6.0, 15.0), (10.0, 20.0), (20.0, 10.0)):
            x += amp * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28, (C, 1)))
        out.append(x.astype(np.float32))
    return out


def heat_maps(rng, n):
    import numpy as np
    yy, xx = np.mgrid[:SIDE, :SIDE]
    out = []
    for _ in range(n):
        cy, cx, s = rng.uniform(40, 180), rng.uniform(40, 180), rng.uniform(10, 40)
        blob = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
        img = np.stack([255 * blob, 180 * blob ** 0.5, 60 * (1 - blob)], axis=2) + rng.integers(0, 12, (SIDE, SIDE, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def device_side(args):
    import numpy as np
    import torch
    from eyegaze_multimodal_amd import _lib as L
    from eyegaze_multimodal_amd import entropy as E
    if not torch.cuda.is_available():
        raise SystemExit("entropy_timing.py measures on the GPU: there is none here")
    rng = np.random.default_rng(0)
    events = []
    plain_call = L.call

    def timed_call(name, *a):
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        plain_call(name, *a)
        ev[1].record()
        events.append((name, ev))

    def case(run_call, n_items):
        wall, per_call = [], {}
        for i in range(args.runs + 1):                               # the first run warms the code objects and is dropped
            events.clear()
            L.call = timed_call
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_call()
            dt = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            L.call = plain_call
            if i:
                wall.append(round(dt, 3))
                run = {}
                for name, (e0, e1) in events:
                    run[name] = run.get(name, 0.0) + e0.elapsed_time(e1)
                for name, v in run.items():
                    per_call.setdefault(name, []).append(round(v, 4))
        return {"items": n_items, "whole_call_ms": wall, "whole_call_ms_median": statistics.median(wall),
                "per_item_ms_median": round(statistics.median(wall) / n_items, 5), "entry_point_ms": per_call,
                "entry_point_ms_median": {k: statistics.median(v) for k, v in per_call.items()}}

    def eeg_case(recs):
        rec = case(lambda: torch.cat(E.spectral_entropy(recs, 250.0, device="cuda")).cpu(), len(recs))
        rows = len(recs) * C
        rec["floors_ms"] = {
            "eg_trial_spectral_entropy: f32 rows read once at the HBM rate": round(rows * SAMPLES * 4 / HBM_BYTES_PER_S * 1e3, 4),
            "eg_recording_filtfilt_exact: rows read and written (f32) and the fp64 intermediate written and read, at the HBM rate":
                round(rows * ((SAMPLES * 4 * 2) + (SAMPLES + 54) * 8 * 2) / HBM_BYTES_PER_S * 1e3, 4),
            "eg_recording_filtfilt_exact: steps of one lane's sequential walk (two passes over samples + 54)": 2 * (SAMPLES + 54)}
        return rec

    def gaze_case(imgs):
        rec = case(lambda: E.spatial_entropy(imgs, device="cuda").cpu(), len(imgs))
        nbytes = len(imgs) * SIDE * SIDE * 3
        rec["floors_ms"] = {"eg_image_entropy: uint8 pixels read twice at the HBM rate": round(2 * nbytes / HBM_BYTES_PER_S * 1e3, 4),
                            "eg_image_entropy: uint8 pixels read once at the HBM rate": round(nbytes / HBM_BYTES_PER_S * 1e3, 4)}
        rec["image_bytes"] = nbytes
        return rec

    # the values do not matter to the time: 100 distinct recordings and 200 distinct images, repeated
    base_r, base_i = raw_recordings(rng, min(args.recordings, 100)), heat_maps(rng, min(args.images, 200))
    recs = [base_r[i % len(base_r)] for i in range(args.recordings)]
    imgs = [base_i[i % len(base_i)] for i in range(args.images)]
    return {"C": C, "samples": SAMPLES, "image": [SIDE, SIDE, 3], "runs": args.runs, "device": torch.cuda.get_device_name(0),
            "eeg_many": eeg_case(recs), "eeg_one": eeg_case(recs[:1]), "gaze_many": gaze_case(imgs), "gaze_one": gaze_case(imgs[:1])}


def cpu_side(args):
    import numpy as np
    from tests.make_golden_entropy import load_reference
    calc, _ = load_reference()
    rng = np.random.default_rng(0)
    recs, imgs = raw_recordings(rng, args.cpu_recordings), heat_maps(rng, args.cpu_images)
    spectral, spatial = calc.SpectralEntropyCalculator(sampling_rate=250.0), calc.SpatialEntropyCalculator()
    eeg, gaze = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        for r in recs:
            spectral.compute(r)
        eeg.append(round((time.perf_counter() - t0) / len(recs) * 1e3, 3))
        t0 = time.perf_counter()
        for im in imgs:
            spatial.compute(im)
        gaze.append(round((time.perf_counter() - t0) / len(imgs) * 1e3, 4))
    return {"cpus": len(os.sched_getaffinity(0)), "threads": 1, "recordings": len(recs), "images": len(imgs),
            "spectral_compute_ms_per_recording": eeg, "spatial_compute_ms_per_image": gaze}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--recordings", type=int, default=1000)
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--cpu-reference", metavar="MACHINE", help="time the reference's compute() loops here, under this machine's name")
    ap.add_argument("--cpu-recordings", type=int, default=3)
    ap.add_argument("--cpu-images", type=int, default=200)
    args = ap.parse_args()
    out = Path(args.out)
    rec = json.loads(out.read_text()) if out.exists() else {}
    if args.cpu_reference:
        rec.setdefault("cpu_reference", {})[args.cpu_reference] = cpu_side(args)
    else:
        rec["device"] = device_side(args)
    print(json.dumps(rec), flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
