"""Measurements of the width-templated long attention core (csrc/attention_long.hip) on the GPU.  One mode per process, because
a process binds one build of the library; --tree names the checkout whose package is imported (default: this one), so the same
script measures a parent build and the change side by side.
    dump   sha256 of the bytes eg_attention_long_fwd / _bwd write on seeded inputs: S in {161, 2048}, dropout 0 and 0.25, bf16, fp16 and
           f32.  Equal digests from two builds = byte-identical outputs at head width 32.
    w32    HIP-event times of eg_attention_long_fwd / _bwd: NB = 256, H = 8, bf16, p in {0, 0.1}, S in {139, 203, 512, 2048}.
    w64    the same cases through eg_attention_dk_* with H = 4 heads of width 64 and with H = 8 of width 32 (equal D = 256).
    step   one training step of the reference's default model (A5 flags, C = 32, window 1024, B = 128, bf16) with 8 heads (width 32:
           the short core inside the fused attention block) and with 4 heads (width 64: three launches, the long core).
    python profiles/tools/attn_dk_timing.py MODE [--tree DIR] [--out FILE.json]"""
import argparse
import copy
import ctypes
import hashlib
import json
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[2]
DEV = torch.device("cuda:0")
NB, D = 256, 256
S_LIST, P_LIST = (139, 203, 512, 2048), (0.0, 0.1)


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


def make_state(L, seed):
    from eyegaze_multimodal_amd.engine import scramble_seed
    sc = scramble_seed(seed)
    st = L.StepState(sc & 0xFFFFFFFF, sc >> 32, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0)
    state = torch.zeros(L.STATE_WORDS, dtype=torch.int32)
    ctypes.memmove(state.data_ptr(), ctypes.addressof(st), ctypes.sizeof(st))
    return state.to(DEV)


def buffers(nb, S, H, hd, dt, seed):
    g = torch.Generator().manual_seed(seed)
    Dm = H * hd
    qkv = torch.randn(nb * S, 3 * Dm, generator=g).to(dt).to(DEV)
    dctx = torch.randn(nb * S, Dm, generator=g).to(dt).to(DEV)
    ctx = torch.zeros(nb * S, Dm, device=DEV, dtype=dt)
    lse = torch.zeros(nb, H, S, device=DEV)
    return qkv, dctx, ctx, lse, torch.zeros_like(qkv), torch.zeros(nb * H * S, device=DEV)


def run_core(L, family, nb, S, H, hd, dtype, p, state, bufs):
    """(fwd, bwd) closures over one set of buffers; family "long" = eg_attention_long_*, "dk" = eg_attention_dk_*"""
    qkv, dctx, ctx, lse, dqkv, scratch = bufs
    heads = (H, hd) if family == "dk" else (H,)
    tail = (0, dtype, p, 16, state.data_ptr() if p > 0 else 0)

    def fwd():
        L.call(f"eg_attention_{family}_fwd", qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), nb, S, *heads, *tail, 0)

    def bwd():
        L.call(f"eg_attention_{family}_bwd", qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), nb, S,
               *heads, *tail, scratch.data_ptr(), scratch.numel(), 0)
    return fwd, bwd


def mode_dump(L, args):
    state = make_state(L, 9)
    out = {}
    for name, dtype, dt in (("bf16", L.EG_BF16, torch.bfloat16), ("fp16", L.EG_F16, torch.float16), ("f32", L.EG_F32, torch.float32)):
        for S in (161, 2048):
            nb, H = (8, 4) if S == 161 else (2, 2)
            for p in (0.0, 0.25):
                bufs = buffers(nb, S, H, 32, dt, seed=S)
                fwd, bwd = run_core(L, "long", nb, S, H, 32, dtype, p, state, bufs)
                fwd()
                bwd()
                torch.cuda.synchronize()
                for k, v in (("ctx", bufs[2]), ("lse", bufs[3]), ("dqkv", bufs[4])):
                    raw = v.contiguous().view(torch.uint8).cpu().numpy().tobytes()
                    out[f"{name}/S{S}/p{p}/{k}"] = hashlib.sha256(raw).hexdigest()
    return out


def time_cases(L, family, H, hd, iters):
    state = make_state(L, 9)
    rows = []
    for p in P_LIST:
        for S in S_LIST:
            bufs = buffers(NB, S, H, hd, torch.bfloat16, seed=S)
            fwd, bwd = run_core(L, family, NB, S, H, hd, L.EG_BF16, p, state, bufs)
            n = max(iters, int(iters * 512 * 512 / (S * S)))          # short launches: more of them per window
            rows.append({"family": family, "H": H, "head_dim": hd, "S": S, "p": p, "fwd_ms": round(timed(fwd, n), 4),
                         "bwd_ms": round(timed(bwd, n), 4)})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def mode_step(L, args):
    from eyegaze_multimodal_amd import HipAdamW
    from eyegaze_multimodal_amd import train_art as TA
    from eyegaze_multimodal_amd.data import randn_windows
    fx = json.loads((REPO / "tests" / "golden" / "reference_configs.json").read_text())
    base = next(e["config"] for e in fx["entries"] if e["name"] == "A5_full_model")
    B, window = 128, 1024
    x1, x2, labels = (v.to(DEV) for v in randn_windows(B, 32, window, seed=1, num_classes=3))
    one = torch.ones(1, device=DEV)
    out = {}
    for rep in range(2):
        for heads in (8, 4):
            cfg = copy.deepcopy(base)
            cfg["data"]["window_size"] = window
            cfg["model"]["num_heads"] = heads
            model = TA.build_model(cfg, compute_dtype="bf16").to(DEV).train()
            eng = model.engine(B, window, DEV)
            opt = HipAdamW(model)

            def step():
                opt.begin_step(eng, seed=3)
                eng.forward(x1, x2, labels, train=True)
                eng.backward(gloss=one, gloss_ibs=one)
                opt.step(eng)
            ms = timed(step, args.iters, warmup=3)
            r = out.setdefault(f"heads{heads}", {"S": eng.S, "attn_block": bool(eng.attn_block), "attn_long": bool(eng.attn_long),
                                                 "ms_per_step": []})
            r["ms_per_step"].append(round(ms, 3))
            print(heads, r, flush=True)
            del model, eng, opt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["dump", "w32", "w64", "step"])
    ap.add_argument("--tree", default=str(REPO))
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    from eyegaze_multimodal_amd import _lib as L
    assert Path(L.__file__).resolve().is_relative_to(Path(args.tree).resolve()), L.__file__
    res = {"mode": args.mode, "tree": Path(args.tree).name, "device": torch.cuda.get_device_name(0)}
    if args.mode == "dump":
        res["sha256"] = mode_dump(L, args)
    elif args.mode == "w32":
        res["cases"] = time_cases(L, "long", 8, 32, args.iters)
    elif args.mode == "w64":
        res["cases"] = time_cases(L, "dk", 4, 64, args.iters) + time_cases(L, "dk", 8, 32, args.iters)
    else:
        res["step"] = mode_step(L, args)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
