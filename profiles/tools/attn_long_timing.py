"""HIP-event timing of the attention cores at long windows (GPU): NB = 256 windows, H = 8 heads, bf16, dropout p in {0, 0.1},
S = 160 (the short kernels, eg_attention_fwd / _bwd) and S = 161, 203, 512, 1024, 2048 (eg_attention_long_fwd / _bwd); then one
A5 training step (C = 32, window 2048 -> S = 203) at B = 128 and the share of it spent in the attention core.
    python profiles/tools/attn_long_timing.py --out profiles/attn_long_timing.json
Scores/s counts the NB * H * S^2 attention scores of one launch."""
import argparse
import copy
import ctypes
import json
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))

from eyegaze_multimodal_amd import HipAdamW, _lib as L  # noqa: E402
from eyegaze_multimodal_amd import train_art as TA  # noqa: E402
from eyegaze_multimodal_amd.data import randn_windows  # noqa: E402
from eyegaze_multimodal_amd.engine import scramble_seed  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, iters, warmup=3):
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


def attention_case(NB, S, H, p, iters, state):
    D = H * 32
    g = torch.Generator(device=DEV).manual_seed(S)
    qkv = torch.randn(NB * S, 3 * D, device=DEV, generator=g).to(torch.bfloat16)
    dctx = torch.randn(NB * S, D, device=DEV, generator=g).to(torch.bfloat16)
    ctx = torch.zeros(NB * S, D, device=DEV, dtype=torch.bfloat16)
    lse = torch.zeros(NB, H, S, device=DEV)
    dqkv = torch.zeros_like(qkv)
    scratch = torch.zeros(NB * H * S, device=DEV)
    st = state.data_ptr() if p > 0 else 0
    args = (NB, S, H, 0, L.EG_BF16, p, 16, st)
    long_ = S > 160
    fwd_name = "eg_attention_long_fwd" if long_ else "eg_attention_fwd"

    def fwd():
        L.call(fwd_name, qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), *args, 0)

    def bwd():
        if long_:
            L.call("eg_attention_long_bwd", qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), *args,
                   scratch.data_ptr(), scratch.numel(), 0)
        else:
            L.call("eg_attention_bwd", qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), *args, 0)
    tf = timed(fwd, iters)
    tb = timed(bwd, iters)
    scores = NB * H * S * S
    return {"S": S, "p": p, "kernel": "long" if long_ else "short", "fwd_ms": round(tf, 4), "bwd_ms": round(tb, 4),
            "fwd_scores_per_s": scores / (tf * 1e-3), "bwd_scores_per_s": scores / (tb * 1e-3),
            "fwd_ns_per_kscore2": tf * 1e6 / (S * S), "bwd_ns_per_kscore2": tb * 1e6 / (S * S)}


def a5_step(B, window, steps):
    fx = json.loads((REPO / "tests" / "golden" / "reference_configs.json").read_text())
    cfg = copy.deepcopy(next(e["config"] for e in fx["entries"] if e["name"] == "A5_full_model"))
    cfg["data"]["window_size"] = window
    model = TA.build_model(cfg, compute_dtype="bf16").to(DEV).train()
    x1, x2, labels = randn_windows(B, 32, window, seed=1, num_classes=3)
    x1, x2, labels = x1.to(DEV), x2.to(DEV), labels.to(DEV)
    eng = model.engine(B, window, DEV)
    opt = HipAdamW(model)
    one = torch.ones(1, device=DEV)

    def step():
        opt.begin_step(eng, seed=3)
        eng.forward(x1, x2, labels, train=True)
        eng.backward(gloss=one, gloss_ibs=one)
        opt.step(eng)
    t = timed(step, steps, warmup=2)
    n_attn = model.cfg.num_layers + (1 if model.cfg.use_cross_attention else 0)
    return eng, t, n_attn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "attn_long_timing.json"))
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    NB, H = 256, 8
    sc = scramble_seed(9)
    st = L.StepState(sc & 0xFFFFFFFF, sc >> 32, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0)
    state = torch.zeros(L.STATE_WORDS, dtype=torch.int32)
    ctypes.memmove(state.data_ptr(), ctypes.addressof(st), ctypes.sizeof(st))
    state = state.to(DEV)
    res = {"device": torch.cuda.get_device_name(0), "NB": NB, "H": H, "dtype": "bf16", "cases": []}
    for p in (0.0, 0.1):
        for S in (160, 161, 203, 512, 1024, 2048):
            r = attention_case(NB, S, H, p, args.iters, state)
            res["cases"].append(r)
            print(json.dumps(r), flush=True)
    by = {(c["S"], c["p"]): c for c in res["cases"]}
    res["switch_ratio_p0"] = {"fwd": by[(161, 0.0)]["fwd_ms"] / by[(160, 0.0)]["fwd_ms"],
                              "bwd": by[(161, 0.0)]["bwd_ms"] / by[(160, 0.0)]["bwd_ms"]}
    res["per_S2_ratio_2048_over_512_p0"] = {k: by[(2048, 0.0)][f"{k}_ns_per_kscore2"] / by[(512, 0.0)][f"{k}_ns_per_kscore2"]
                                            for k in ("fwd", "bwd")}
    eng, t_step, n_attn = a5_step(128, 2048, steps=5)
    S = eng.S
    a = attention_case(2 * 128, S, H, 0.1, args.iters, state)
    attn_ms = n_attn * (a["fwd_ms"] + a["bwd_ms"])
    res["a5_step"] = {"B": 128, "window": 2048, "S": S, "ms_per_step": round(t_step, 3), "samples_per_s": 128 / (t_step * 1e-3),
                      "attention_ms_per_step": round(attn_ms, 3), "attention_share": attn_ms / t_step,
                      "how": f"{n_attn} x (eg_attention_long_fwd + _bwd) at NB = 256, S = {S}, p = 0.1, timed alone"}
    print(json.dumps(res["a5_step"]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
