"""Forward-only route timings -> profiles/infer_timing.json.

  python profiles/tools/infer_timing.py kernels OUT.json
      eg_attn_block_fwd and eg_ffn_chain, lean against keeping form, HIP events around hot loops: NB = 512 windows of S = 65
      (M = 33 280 rows, F = 1024), bf16, p = 0; the two forms alternate, three repeats
  python profiles/tools/infer_timing.py forward --repo TREE --side forward|predict --workload cfg3|a5c32 OUT.json
      one whole forward at B = 256, bf16, from the package in TREE: `forward` = eval-mode DualEEGTransformer.forward under no_grad
      (what a tree without predict offers), `predict` = DualEEGTransformer.predict.  Host clock around a synchronised loop; also the
      peak device memory of the FIRST call above what the model alone holds (torch.cuda.max_memory_allocated)
  python profiles/tools/infer_timing.py merge OUT.json PART.json ...
A job alternates the sides (parent tree, this tree, parent tree, this tree) and merges the parts."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve()


def events_us(torch, fn, reps=50, warm=10):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernels(out):
    sys.path.insert(0, str(HERE.parent.parent.parent))
    import torch
    from eyegaze_multimodal_amd import _lib as L
    from eyegaze_multimodal_amd._lib import call, ptr
    dev, t, D, F, NB, S = "cuda", torch.bfloat16, 256, 1024, 512, 65
    M = NB * S
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s, sc=1.0, dt=t: (torch.randn(*s, generator=g) * sc).to(dt).to(dev)
    # fragment order does not matter to the clock: any finite weights
    x, wqkv, wo, w1, w2 = rnd(M, D, sc=0.5), rnd(3 * D * D, sc=0.08), rnd(D * D, sc=0.06), rnd(F * D, sc=0.1), rnd(D * F, sc=0.05)
    f32 = torch.float32
    bqkv, bo, b1, b2 = rnd(3 * D, sc=0.1, dt=f32), rnd(D, sc=0.1, dt=f32), rnd(F, sc=0.1, dt=f32), rnd(D, sc=0.1, dt=f32)
    gamma, beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    y, qkv, ctx, r1 = torch.zeros(M, D, device=dev, dtype=t), torch.zeros(M, 3 * D, device=dev, dtype=t), torch.zeros(M, D, device=dev, dtype=t), \
        torch.zeros(M, D, device=dev, dtype=t)
    lse, st, H = torch.zeros(NB, 8, S, device=dev), torch.zeros(M, 2, device=dev), torch.zeros(M, F, device=dev, dtype=t)

    def attn(lean):
        d = L.AttnBlockDesc()
        d.x, d.wqkv_frag, d.wo_frag, d.bqkv, d.bo = ptr(x), ptr(wqkv), ptr(wo), ptr(bqkv), ptr(bo)
        d.NB, d.S, d.d_model, d.num_heads, d.dtype = NB, S, D, 8, L.EG_BF16
        d.ln_gamma, d.ln_beta, d.ln_out = ptr(gamma), ptr(beta), ptr(y)
        if not lean:
            d.qkv, d.ctx, d.lse, d.r1, d.ln_stats = ptr(qkv), ptr(ctx), ptr(lse), ptr(r1), ptr(st)
        return lambda: call("eg_attn_block_fwd", C.byref(d), 0)

    def ffn(lean):
        f = L.FfnDesc()
        f.A, f.W1, f.W2, f.bias1, f.bias2, f.residual, f.act1 = ptr(x), ptr(w1), ptr(w2), ptr(b1), ptr(b2), ptr(x), L.ACT_RELU
        f.lda, f.ldg, f.ldr, f.M, f.F, f.dtype = D, F, D, M, F, L.EG_BF16
        f.ln_gamma, f.ln_beta, f.ln_out = ptr(gamma), ptr(beta), ptr(y)
        if not lean:
            f.H, f.C, f.ln_stats, f.ldh, f.ldc = ptr(H), ptr(r1), ptr(st), F, D
        return lambda: call("eg_ffn_chain", C.byref(f), 0)

    es = 2
    res = {"shape": f"NB={NB} S={S} M={M} F={F} bf16 p=0", "us": {}, "algorithmic_MB": {
        "attn_block_keep": round((es * (M * D * 4 + M * 3 * D + 4 * D * D) + 4 * NB * 8 * S + 8 * M) / 1e6, 1),
        "attn_block_lean": round(es * (2 * M * D + 4 * D * D) / 1e6, 1),
        "ffn_chain_keep": round((es * (M * D * 3 + M * F + 2 * F * D) + 8 * M) / 1e6, 1),
        "ffn_chain_lean": round(es * (2 * M * D + 2 * F * D) / 1e6, 1)}}
    with torch.cuda.stream(torch.cuda.default_stream()):
        for _ in range(3):                                  # alternating: drift hits both forms alike
            for name, mk in (("attn_block", attn), ("ffn_chain", ffn)):
                for lean in (False, True):
                    res["us"].setdefault(f"{name}_{'lean' if lean else 'keep'}", []).append(round(events_us(torch, mk(lean)), 2))
    Path(out).write_text(json.dumps({"kernels": res}, indent=1))
    print(json.dumps(res))


def forward(repo, side, workload, out, B=256, iters=30, warm=5):
    sys.path.insert(0, str(Path(repo).resolve()))
    import torch
    from bench import WORKLOADS
    from eyegaze_multimodal_amd import DualEEGTransformer
    from eyegaze_multimodal_amd.data import randn_windows
    dev = torch.device("cuda", 0)
    kw = dict(WORKLOADS[workload][0], num_classes=3)
    Cn = kw.pop("in_channels", 8)
    torch.manual_seed(42)
    model = DualEEGTransformer(in_channels=Cn, max_len=256, compute_dtype="bf16", **kw).to(dev).eval()
    x1, x2, y = randn_windows(B, Cn, 1024, seed=1234, num_classes=3, device=dev)
    run = (lambda: model.predict(x1, x2, y)) if side == "predict" else (lambda: model(x1, x2, y))
    with torch.no_grad():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        logits = run()["logits"].float().cpu()
        peak = torch.cuda.max_memory_allocated() - base
        for _ in range(warm):
            run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            run()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / iters * 1e3
    rec = {"side": side, "workload": workload, "B": B, "ms_per_forward": round(ms, 3), "peak_bytes_first_call": int(peak),
           "logits_checksum": float(logits.double().abs().sum())}
    if side == "predict":
        from eyegaze_multimodal_amd import _lib as L
        from eyegaze_multimodal_amd.engine import inference_workspace_bytes
        rec["inference_workspace_bytes"] = list(inference_workspace_bytes(model.cfg, B, 1024, L.EG_BF16))
    Path(out).write_text(json.dumps({"forward": [rec]}, indent=1))
    print(json.dumps(rec))


def merge(out, parts):
    res = {"forward": []}
    for p in parts:
        d = json.loads(Path(p).read_text())
        res["forward"] += d.get("forward", [])
        if "kernels" in d:
            res["kernels"] = d["kernels"]
        if "bench" in d:
            res["bench"] = d["bench"]
    Path(out).write_text(json.dumps(res, indent=1))
    print(out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["kernels", "forward", "merge"])
    ap.add_argument("out")
    ap.add_argument("parts", nargs="*")
    ap.add_argument("--repo", default=str(HERE.parent.parent.parent))
    ap.add_argument("--side", default="predict", choices=["forward", "predict"])
    ap.add_argument("--workload", default="cfg3", choices=["cfg3", "a5c32"])
    a = ap.parse_args()
    if a.mode == "kernels":
        kernels(a.out)
    elif a.mode == "forward":
        forward(a.repo, a.side, a.workload, a.out)
    else:
        merge(a.out, a.parts)
