"""Trial features on the device -> profiles/trialfeat_timing.json.

    timeout 900 python profiles/tools/trialfeat_timing.py OUT.json [--runs 5] [--pairs 300] [--samples 3250]
    python profiles/tools/trialfeat_timing.py OUT.json --cpu-reference MACHINE [--workers N]

Synthetic raw-like trials (offset of thousands, random walk, a component both players share, 6 / 10 / 20 Hz tones, noise), C = 32,
250 Hz, the five bands.  Device side (one GPU): eyegaze_multimodal_amd.features.extract_trial_features on
  many   `pairs` pairs of `samples` samples (the reference's trial length)
  one    one such pair
five runs after a warm-up, every run listed: the whole call by wall clock (host arrays in, its one sync at the end) and every
entry point by HIP events around its calls, summed over the call.  For eg_trial_pairs the two floors it is compared with are
stated: the bytes of the four f32 row images over the HBM rate, and its six f32 MFMAs per four samples over the f32 MFMA rate.
CPU side (--cpu-reference, where the reference tree and scipy exist): the body of the reference's process_trial without file
I/O on one such pair in one thread, and over `workers` joblib workers (default: the CPUs this process may use, so that the
pool is not oversubscribed); stored under cpu_reference/MACHINE.  Both sides merge
into the same file."""
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
MFMA_F32_FLOPS = 157.3e12           # v_mfma_f32_16x16x4_f32 peak


def raw_pairs(rng, n, C, L, fs=250.0):
    import numpy as np
    t = np.arange(L) / fs
    out = []
    for _ in range(n):
        shared = np.cumsum(rng.normal(0, 1.5, L)) + rng.normal(0, 6.0, L)
        pair = []
        for _ in (0, 1):
            x = rng.uniform(-4000, 4000, (C, 1)) + np.cumsum(rng.normal(0, 2.0, (C, L)), axis=1) + rng.normal(0, 5.0, (C, L))
            for f, amp in ((6.0, 15.0), (10.0, 20.0), (20.0, 10.0)):
                x += amp * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28, (C, 1)))
            pair.append((x + rng.uniform(0.4, 1.0, (C, 1)) * shared).astype(np.float32))
        out.append(tuple(pair))
    return out


def device_side(args):
    import numpy as np
    import torch
    from eyegaze_multimodal_amd import _lib as L
    from eyegaze_multimodal_amd import features as F
    if not torch.cuda.is_available():
        raise SystemExit("trialfeat_timing.py measures on the GPU: there is none here")
    C, rng = 32, np.random.default_rng(0)
    events = []
    plain_call = L.call

    def timed_call(name, *a):
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        plain_call(name, *a)
        ev[1].record()
        events.append((name, ev))

    def case(pairs):
        wall, per_call = [], {}
        for i in range(args.runs + 1):                               # the first run warms the code objects and is dropped
            events.clear()
            L.call = timed_call
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = F.extract_trial_features(pairs, 250, device="cuda")
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            L.call = plain_call
            if i:
                wall.append(round(dt, 3))
                run = {}
                for name, (e0, e1) in events:
                    run[name] = run.get(name, 0.0) + e0.elapsed_time(e1)
                for name, v in run.items():
                    per_call.setdefault(name, []).append(round(v, 4))
            del out
        n, Ls = len(pairs), pairs[0][0].shape[1]
        med = {k: statistics.median(v) for k, v in per_call.items()}
        nb = len(F.FREQUENCY_BANDS)
        image_bytes = nb * n * 4 * 2 * C * Ls * 4                    # four f32 planes of 2 C rows, read once per band
        flops = nb * n * 3 * 6 * 2 * C * C * Ls                      # six 16x16x4 MFMAs per four samples and 16 x 16 tile
        floor_hbm, floor_mfma = image_bytes / HBM_BYTES_PER_S * 1e3, flops / MFMA_F32_FLOPS * 1e3
        return {"pairs": n, "samples": Ls, "whole_call_ms": wall, "whole_call_ms_median": statistics.median(wall),
                "per_trial_ms_median": round(statistics.median(wall) / n, 4), "entry_point_ms": per_call, "entry_point_ms_median": med,
                "pairs_floor_ms": {"hbm_bytes_of_four_row_images": round(floor_hbm, 4), "f32_mfma": round(floor_mfma, 4),
                                   "measured_over_hbm_floor": round(med["eg_trial_pairs"] / floor_hbm, 2),
                                   "measured_over_mfma_floor": round(med["eg_trial_pairs"] / floor_mfma, 2),
                                   "note": "eg_trial_pairs' time includes its row statistics and finish launches"}}

    many = raw_pairs(rng, args.pairs, C, args.samples)
    return {"C": C, "runs": args.runs, "device": torch.cuda.get_device_name(0), "many": case(many), "one": case(many[:1])}


def cpu_side(args):
    import numpy as np
    from tests.make_golden_trial_features import load_extractor, reference_features
    P = load_extractor()
    pairs = raw_pairs(np.random.default_rng(0), max(2, args.workers), 32, args.samples)
    one = []
    for _ in range(2):
        t0 = time.perf_counter()
        reference_features(P, *pairs[0])
        one.append(round(time.perf_counter() - t0, 3))
    rec = {"samples": args.samples, "C": 32, "cpus": len(os.sched_getaffinity(0)), "process_trial_body_s_one_thread": one}
    if P.JOBLIB_AVAILABLE and args.workers > 1:
        from joblib import Parallel, delayed
        t0 = time.perf_counter()
        Parallel(n_jobs=args.workers, backend="loky")(delayed(reference_features)(P, *p) for p in pairs)
        dt = time.perf_counter() - t0
        rec[f"joblib_{args.workers}_workers"] = {"trials": len(pairs), "seconds": round(dt, 3), "seconds_per_trial": round(dt / len(pairs), 3)}
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=300)
    ap.add_argument("--samples", type=int, default=3250)
    ap.add_argument("--cpu-reference", metavar="MACHINE", help="time the reference's process_trial body here, under this machine's name")
    ap.add_argument("--workers", type=int, default=len(os.sched_getaffinity(0)))
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
