"""HIP-event timing of the synchrony (IBS) kernels per window length (GPU), at the a5c32 shape: B = 256 window pairs, C = 32
channels (nsig = 16 384 signals), the 6 robust bands, fs = 256.  T = 1024 and 2048 run the radix-4 transforms and full 256-step
chunks; T = 1000 and 2000 the mixed-radix plan (4 2 5 5 5, 4 4 5 5 5) and a partial last chunk; T = 1021 (prime) the direct DFT.
    python profiles/tools/ibs_window_timing.py --out profiles/ibs_window_timing.json"""
import argparse
import ctypes as CT
import json
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd.tokens import ROBUST_BANDS, nbin_for  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def case(B, C, T, fs, iters):
    nb, nsig = len(ROBUST_BANDS), 2 * B * C
    lo = (CT.c_float * nb)(*[b[0] for b in ROBUST_BANDS])
    hi = (CT.c_float * nb)(*[b[1] for b in ROBUST_BANDS])
    nbin = nbin_for(T, fs, max(b[1] for b in ROBUST_BANDS))
    g = torch.Generator(device=DEV).manual_seed(T)
    x = torch.randn(nsig, T, device=DEV, generator=g)
    xb, ph = torch.zeros(nb, nsig, T, device=DEV), torch.zeros(nb, nsig, T, device=DEV)
    stats, spec = torch.zeros(nb, nsig, 4, device=DEV), torch.zeros(nsig, nbin, 2, device=DEV)
    conn = torch.zeros(B, nb, 7, C, C, device=DEV)

    def analytic():
        L.call("eg_ibs_analytic", x.data_ptr(), xb.data_ptr(), ph.data_ptr(), stats.data_ptr(), spec.data_ptr(), nsig, T, fs,
               nbin, CT.addressof(lo), CT.addressof(hi), nb, 0)

    def pairs():
        L.call("eg_ibs_pairs", xb.data_ptr(), ph.data_ptr(), stats.data_ptr(), spec.data_ptr(), conn.data_ptr(), B, C, T, fs,
               nbin, CT.addressof(lo), CT.addressof(hi), nb, 0)
    ta = timed(analytic, iters)
    tp = timed(pairs, iters)
    return {"T": T, "pow2": T & (T - 1) == 0, "nbin": nbin, "ibs_analytic_us": round(ta * 1e3, 1),
            "ibs_pairs_us": round(tp * 1e3, 1), "analytic_ns_per_sample": ta * 1e6 / (nsig * T),
            "pairs_ns_per_step": tp * 1e6 / T}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "ibs_window_timing.json"))
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    B, C, fs = 256, 32, 256.0
    res = {"device": torch.cuda.get_device_name(0), "B": B, "C": C, "bands": len(ROBUST_BANDS), "fs": fs, "cases": []}
    for T in (1024, 1000, 2048, 2000, 1021):
        r = case(B, C, T, fs, args.iters if T != 1021 else 3)
        res["cases"].append(r)
        print(json.dumps(r), flush=True)
    by = {c["T"]: c for c in res["cases"]}
    res["ratio_1000_over_1024"] = {k: by[1000][f"{k}_us"] / by[1024][f"{k}_us"] for k in ("ibs_analytic", "ibs_pairs")}
    res["ratio_2000_over_2048"] = {k: by[2000][f"{k}_us"] / by[2048][f"{k}_us"] for k in ("ibs_analytic", "ibs_pairs")}
    res["targets_1000"] = {"ibs_analytic": 1.3, "ibs_pairs": 1.1}
    print(json.dumps({k: res[k] for k in ("ratio_1000_over_1024", "ratio_2000_over_2048")}), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
