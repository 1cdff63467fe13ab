"""The image encoder at 224 x 224 -> profiles/image224_timing.json.

    timeout 600 python profiles/tools/image224_timing.py OUT.json [--runs 7]

One GPU.  Every figure is HIP events around the call(s) alone, inputs already on the device, `runs` runs after two warm-ups, every
run listed, the median quoted:
  conv1     eg_spec_conv1_fwd_banded / _bwd_banded at 224 x 224 with the production band height, nimg = 32 (the reference's batch
            of 16 pairs) and nimg = 512, bf16.  Bytes from the shapes (the images once, the interior of p1 / dp1 once, the partial
            rows once); the share is bytes / time over the measured copy rate of the MI355X (6.29 TB/s, float4 copy).
  routes    the whole-image kernels against the banded ones with band_rows forced to 16, nimg = 32: forward at 120 x 120 (the
            largest square whose whole forward fits 64 KiB of LDS; its whole backward does not), forward and backward at 112 x 112.
            Informational: production routing is eg_spec_conv1_band_rows' and is not chosen by these numbers.
  step      one MultimodalTrainer.train_step at image 224, B = 16, bf16 and fp16, and the image engine's forward + backward alone
            with HIP events around every launch (the per-launch split of the image branch)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))

COPY_BYTES_PER_S = 6.29e12


def timed(fn, runs):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def entry(ms, nbytes=None):
    med = statistics.median(ms)
    out = {"ms": [round(v, 4) for v in ms], "median_ms": round(med, 4)}
    if nbytes is not None:
        out.update(bytes=int(nbytes), TB_per_s=round(nbytes / med / 1e9, 3),
                   share_of_copy_rate=round(nbytes / (med * 1e-3) / COPY_BYTES_PER_S, 3))
    return out


def conv1(L, torch, dev, nimg, F, nfr, band, runs, whole_fwd=False, whole_bwd=False):
    """forward / backward of conv-1 on the banded kernels with `band` pooled rows, and on the whole-image kernels where asked"""
    Hp, Wp = F // 2, nfr // 2
    g = torch.Generator().manual_seed(nimg + F)
    img = torch.randn(nimg, F, nfr, generator=g).to(dev)
    w, b = (torch.randn(32, 9, generator=g) / 3).to(dev), (torch.randn(32, generator=g) * 0.1 - 1.0).to(dev)
    p1 = torch.zeros(nimg, Hp + 2, Wp + 4, 32, dtype=torch.bfloat16, device=dev)
    dp1 = torch.randn(nimg, Hp + 2, Wp, 32, generator=g).to(torch.bfloat16).to(dev)
    nbands = -(-Hp // band)
    part = torch.zeros(nimg * nbands, 320, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    p = L.ptr
    cell = nimg * Hp * Wp * 32 * 2
    out = {"nimg": nimg, "size": [F, nfr], "band_rows": band, "nbands": nbands, "workgroups": nimg * nbands,
           "lds_bytes_fwd": ((2 * band + 2) * (nfr + 2) + 320) * 4}
    out["fwd_banded"] = entry(timed(lambda: L.call("eg_spec_conv1_fwd_banded", p(img), p(w), p(b), p(p1), nimg, F, nfr, band, L.EG_BF16, st),
                                    runs), img.numel() * 4 + cell)
    out["bwd_banded"] = entry(timed(lambda: L.call("eg_spec_conv1_bwd_banded", p(img), p(w), p(b), p(dp1), p(part), nimg, F, nfr, band,
                                                   L.EG_BF16, st), runs), img.numel() * 4 + cell + part.numel() * 4)
    if whole_fwd:
        out["fwd_whole"] = entry(timed(lambda: L.call("eg_spec_conv1_fwd", p(img), p(w), p(b), p(p1), nimg, F, nfr, L.EG_BF16, st), runs),
                                 img.numel() * 4 + cell)
    if whole_bwd:
        out["bwd_whole"] = entry(timed(lambda: L.call("eg_spec_conv1_bwd", p(img), p(w), p(b), p(dp1), p(part), nimg, F, nfr, L.EG_BF16, st),
                                       runs), img.numel() * 4 + cell + nimg * 320 * 4)
    return out


def step(torch, dev, dtype, runs, B=16, size=224):
    from eyegaze_multimodal_amd import DualEEGTransformer, engine as E, image_encoder, tokens
    from eyegaze_multimodal_amd.fuzzy_gating_fusion import FuzzyGatingFusion
    from eyegaze_multimodal_amd.train_multimodal_fuzzy_fusion import MultimodalFusionModel, MultimodalTrainer, synth_multimodal
    torch.manual_seed(3)
    model = MultimodalFusionModel(image_encoder.GazeCNNEncoder(num_classes=3, d_model=256, compute_dtype=dtype),
                                  DualEEGTransformer(in_channels=8, num_classes=3, max_len=256, use_spectrogram=False, use_ibs=False,
                                                     compute_dtype=dtype),
                                  FuzzyGatingFusion(num_classes=3, mode="full"))
    tr = MultimodalTrainer(model, dev)
    img1, img2, x1, x2, y = (t.to(dev) for t in synth_multimodal(B, 8, 1024, size, size, 3, seed=5))
    out = {"B": B, "size": [size, size], "dtype": dtype,
           "train_step": entry(timed(lambda: tr.train_step(img1, img2, x1, x2, y), runs))}
    # the image branch alone, events around every launch
    eng = model.gaze_encoder.engine(B, size, size, dev)
    gl = torch.randn(B, 3, device=dev)
    rows, real = [], E.call

    def probe(name, *args):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        real(name, *args)
        b.record()
        rows.append((name, a, b))
    per = []
    for run in range(2 + runs):
        del rows[:]
        for m in (E, tokens, image_encoder):
            m.call = probe
        try:
            eng.forward(img1, img2, True)
            eng.backward(gl)
        finally:
            for m in (E, tokens, image_encoder):
                m.call = real
        torch.cuda.synchronize()
        if run >= 2:
            per.append([(n, a.elapsed_time(b)) for n, a, b in rows])
    names = [n for n, _ in per[0]]
    med = [statistics.median(r[i][1] for r in per) for i in range(len(names))]
    out["image_branch_launches"] = [{"launch": n, "median_ms": round(v, 4)} for n, v in zip(names, med)]
    out["image_branch_sum_ms"] = round(sum(med), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    import torch
    from eyegaze_multimodal_amd import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("image224_timing.py measures on the GPU: there is none here")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "copy_bytes_per_s": COPY_BYTES_PER_S}
    band = L.spec_conv1_band_rows(224, 224)
    res["conv1_224"] = [conv1(L, torch, dev, n, 224, 224, band, args.runs) for n in (32, 512)]
    res["routes"] = {"note": "informational: production takes the whole-image kernels wherever their backward fits 64 KiB",
                     "120x120": conv1(L, torch, dev, 32, 120, 120, 16, args.runs, whole_fwd=True),
                     "112x112": conv1(L, torch, dev, 32, 112, 112, 16, args.runs, whole_fwd=True, whole_bwd=True)}
    res["step"] = [step(torch, dev, dt, args.runs) for dt in ("bf16", "fp16")]
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
