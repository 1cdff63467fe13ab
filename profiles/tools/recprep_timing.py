"""Recording preprocessing on the device -> profiles/recprep_timing.json.

    timeout 900 python profiles/tools/recprep_timing.py OUT.json [--runs 5] [--pairs 300] [--samples 3250] [--long 921600]

Synthetic raw-like recordings (offset of thousands, random walk, 10 / 50 Hz tones, noise), C = 32, the reference's filter
(0.5-50 Hz at 250 Hz, order 4), one GPU.  Two cases:
  store   `pairs` pairs of `samples` samples (the reference's trial length): data.preprocess_recordings end to end (wall clock,
          host arrays in, a synchronise at the end), and its two entry-point calls on a resident copy timed by HIP events;
          against the sequential float64 numpy restatement (tests/recprep_ref.py, vectorised over all rows) and, where scipy
          imports, scipy.signal.filtfilt + the reference's CAR and z-score in numpy, in one thread and in a pool of the CPUs
          this process may use (at most 16)
  long    one pair of `long` samples (an hour at 256 Hz): one wave per player, the worst case of predict_recording
Every run is listed; the medians are what DESIGN.md quotes."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve()
sys.path.insert(0, str(HERE.parent.parent.parent))


def raw_like(rng, n, C, L, fs=250.0):
    import numpy as np
    t = np.arange(L) / fs
    x = rng.uniform(-4000, 4000, (n, C, 1)) + np.cumsum(rng.normal(0, 2.0, (n, C, L)), axis=2)
    x += 20.0 * np.sin(2 * np.pi * 10.0 * t + rng.uniform(0, 6.28, (n, C, 1))) + 15.0 * np.sin(2 * np.pi * 50.0 * t)
    return (x + rng.normal(0, 5.0, (n, C, L))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=300)
    ap.add_argument("--samples", type=int, default=3250)
    ap.add_argument("--long", type=int, default=921600)
    args = ap.parse_args()
    import numpy as np
    import torch
    from eyegaze_multimodal_amd import _lib as L
    from eyegaze_multimodal_amd import filters
    from eyegaze_multimodal_amd.data import preprocess_recordings, recording_row_tables
    from tests import recprep_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("recprep_timing.py measures on the GPU: there is none here")
    dev = torch.device("cuda", 0)
    C, prep = 32, dict(sampling_rate=250.0, filter_low=0.5, filter_high=50.0)
    b, a = filters.butter_bandpass(4, 0.5, 50.0, 250.0)
    zi = filters.lfilter_zi(b, a)
    pad = 3 * len(b)
    dbl = lambda v: (ctypes.c_double * len(v))(*[float(x) for x in v])
    rng = np.random.default_rng(0)

    def launches(recs, runs):
        """the two entry points on a resident copy, by HIP events: ms per run of each"""
        lengths = [r.shape[1] for r in recs]
        row_off, row_len, ws_off, floats, need = recording_row_tables(lengths, C, pad)
        src = torch.cat([torch.from_numpy(r).reshape(-1) for r in recs]).to(dev)
        tabs = [torch.from_numpy(t).to(dev) for t in (row_off, row_len, ws_off)]
        ws = torch.empty(need, dtype=torch.float64, device=dev)
        ms = {"filtfilt": [], "car_zscore": []}
        stream = torch.cuda.current_stream(dev).cuda_stream
        for i in range(runs + 1):                                  # the first run warms the code objects and is dropped
            data = src.clone()
            desc = L.RecordingRowsDesc(L.ptr(data), L.ptr(tabs[0]), L.ptr(tabs[1]), L.ptr(tabs[2]), len(row_len), C, max(lengths), 0)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            L.call("eg_recording_filtfilt", ctypes.byref(desc), dbl(b), dbl(a), dbl(zi), len(b), L.ptr(ws), need, need, stream)
            ev[1].record()
            L.call("eg_recording_car_zscore", ctypes.byref(desc), stream)
            ev[2].record()
            torch.cuda.synchronize()
            if i:
                ms["filtfilt"].append(round(ev[0].elapsed_time(ev[1]), 4))
                ms["car_zscore"].append(round(ev[1].elapsed_time(ev[2]), 4))
        return ms, data

    rec = {"C": C, "filter": {**prep, "order": 4}, "runs": args.runs, "device": torch.cuda.get_device_name(0)}
    # ---- store: pairs x 2 recordings of `samples`
    x = raw_like(rng, 2 * args.pairs, C, args.samples)
    recs = list(x)
    rows = 2 * args.pairs * C
    ms, dev_out = launches(recs, args.runs)
    wall = []
    for i in range(args.runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = preprocess_recordings(recs, device=dev, **prep)
        torch.cuda.synchronize()
        if i:
            wall.append(round((time.perf_counter() - t0) * 1e3, 3))
    got = torch.stack(out).cpu().numpy()
    store = {"pairs": args.pairs, "samples": args.samples, "rows": rows, "waves": (rows + 63) // 64, "launch_ms": ms,
             "launch_ms_median": {k: statistics.median(v) for k, v in ms.items()}, "end_to_end_ms": wall,
             "end_to_end_ms_median": statistics.median(wall)}
    steps = 2 * (args.samples + 2 * pad)
    store["filtfilt_ns_per_row_step"] = round(store["launch_ms_median"]["filtfilt"] * 1e6 / steps, 2)   # every wave walks `steps` samples
    flat = x.reshape(-1, args.samples)
    t0 = time.perf_counter()
    f64 = R.filtfilt_ref(b, a, zi, flat).astype(np.float32)
    t1 = time.perf_counter()
    fin = np.stack([R.car_zscore_ref(f64[i * C:(i + 1) * C]) for i in range(2 * args.pairs)])
    t2 = time.perf_counter()
    store["numpy_restatement_ms"] = {"filtfilt": round((t1 - t0) * 1e3, 1), "car_zscore": round((t2 - t1) * 1e3, 1)}
    store["max_abs_diff_device_vs_restatement"] = float(np.abs(got - fin).max())
    try:
        from scipy import signal
    except ImportError:
        signal = None
    if signal is not None:
        def ref_one(r):
            f = signal.filtfilt(b, a, r, axis=1).astype(np.float32)
            f = (f - f.mean(axis=0, keepdims=True)).astype(np.float32)
            return ((f - f.mean(axis=1, keepdims=True)) / (f.std(axis=1, keepdims=True) + 1e-8)).astype(np.float32)
        t0 = time.perf_counter()
        sp = np.stack([ref_one(r) for r in recs])
        one = (time.perf_counter() - t0) * 1e3
        ncpu = min(16, len(os.sched_getaffinity(0)))
        from concurrent.futures import ThreadPoolExecutor
        t0 = time.perf_counter()
        with ThreadPoolExecutor(ncpu) as ex:
            list(ex.map(ref_one, recs))
        store["scipy_ms"] = {"one_thread": round(one, 1), f"pool_of_{ncpu}": round((time.perf_counter() - t0) * 1e3, 1)}
        store["max_abs_diff_device_vs_scipy"] = float(np.abs(got - sp).max())
    rec["store"] = store
    del x, recs, out, dev_out
    # ---- long: one pair of `long` samples
    xl = raw_like(rng, 2, C, args.long)
    runs = max(2, min(args.runs, 3))
    ms, _ = launches(list(xl), runs)
    rec["long"] = {"samples": args.long, "rows": 2 * C, "waves": 1, "launch_ms": ms,
                   "launch_ms_median": {k: statistics.median(v) for k, v in ms.items()},
                   "filtfilt_ns_per_row_step": round(statistics.median(ms["filtfilt"]) * 1e6 / (2 * (args.long + 2 * pad)), 2)}
    print(json.dumps(rec), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
