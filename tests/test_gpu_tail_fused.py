"""The step's small-launch tail on its fused kernels (Engine.fused_tail = True, the default for bf16 / fp16) against the separate
launches it replaces (fused_tail = False) on the same model, inputs and seed.

Everything compared here is required to be BIT-IDENTICAL (torch.equal; byte equality for the packed weights):
  * forward: logits, sloss, loss, cls1, cls2, comb, zf, hcl -- eg_heads_fwd runs gemm_nt_kernel's MFMA shape, operand order and
    ascending K order in one accumulator, rounds to the 16-bit type at the same points, draws SITE_CLS's mask from the same element
    indices, and shares the class-projection / cross-entropy / mean code with eg_classifier_ce_fwd;
  * backward: dz (as left for the encoder), dy1pad, and the gradients of classifier.*, symmetric_fusion.proj.*, pos_embed, cls_token
    -- the in-launch weight gradients keep eg_gemm_tn's two 128-row slabs (one MFMA chain each over ascending 32-row steps, added
    last, as eg_reduce_partials adds them) and its 16-row bias column sums; eg_token_grad_tail keeps eg_batch_rowsum's sixteen
    chains and their combination tree.  No quantity is held to a weaker (float64-bound) comparison;
  * the packed weight buffers conv0, conv1, conv1T, pos: pure data movement."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import DualEEGTransformer  # noqa: E402
from oracle import dual_eeg_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
KW = dict(in_channels=8, num_classes=3, max_len=256, use_spectrogram=False, use_ibs=False, use_cross_attention=True)
T = 1024
PACKED = ("conv0", "conv1", "conv1T", "pos")
FWD = ("logits", "sloss", "loss", "cls1", "cls2", "comb", "zf", "hcl")
GRADS = ("classifier.0.weight", "classifier.0.bias", "classifier.3.weight", "classifier.3.bias", "symmetric_fusion.proj.weight",
         "symmetric_fusion.proj.bias", "pos_embed.pos_embed.weight", "cls_token")


def build(dtype, B, seed=11):
    cfg = O.ModelCfg(**KW)
    model = DualEEGTransformer(**KW, compute_dtype=dtype)
    model.load_state_dict(O.synthetic_state_dict(cfg, seed=7))
    model = model.to(DEV)
    g = torch.Generator().manual_seed(seed + B)
    x1, x2 = torch.randn(B, 8, T, generator=g).to(DEV), torch.randn(B, 8, T, generator=g).to(DEV)
    labels = torch.randint(0, 3, (B,), generator=g).to(DEV)
    ext = dict(glogits=(0.01 * torch.randn(B, 3, generator=g)).to(DEV), gcls1=(0.01 * torch.randn(B, 256, generator=g)).to(DEV),
               gcls2=(0.01 * torch.randn(B, 256, generator=g)).to(DEV))
    return model, model.engine(B, T, DEV), x1, x2, labels, ext


def run(model, eng, fused, x1, x2, labels, train, bwd_kw):
    eng.fused_tail = fused
    fp = model._flat
    for n in PACKED:                      # the packed buffers and the outputs must be WRITTEN by this route, not left over
        eng.w[n].view(torch.int16).fill_(0x7b7b)
    for n in FWD:
        eng.a[n].fill_(7.0)
    fp.grad.fill_(7.0)
    eng.set_state(seed=5, lr=1e-3, step=1)
    eng.forward(x1, x2, labels, train=train)
    out = {n: eng.a[n].clone() for n in FWD}
    out.update({"w." + n: eng.w[n].view(torch.int16).clone() for n in PACKED})
    keep = {}
    eng.backward(on_segment=lambda name: keep.setdefault(name, eng.g["dzA"].clone()) if name == "heads" else None, **bwd_kw)
    torch.cuda.synchronize()
    out["dz"] = keep["heads"]
    out["dy1pad"] = eng.g["dy1pad"].clone()
    for n in GRADS:
        o = fp.offsets[n]
        out["g." + n] = fp.grad[o:o + dict(zip(fp.names, fp.params))[n].numel()].clone()
    return out


def compare(a, b, skip=()):
    for n in a:
        if n in skip:
            continue
        assert torch.equal(a[n], b[n]), (n, float((a[n].float() - b[n].float()).abs().max()))
    assert torch.isfinite(a["logits"]).all()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B", [4, 32, 256])
def test_fused_tail_equals_the_separate_launches(B, dtype):
    model, eng, x1, x2, labels, ext = build(dtype, B)
    one = torch.ones(1, device=DEV)
    # train mode (dropout), labels, loss gradient
    f = run(model, eng, True, x1, x2, labels, True, dict(gloss=one))
    s = run(model, eng, False, x1, x2, labels, True, dict(gloss=one))
    compare(f, s)
    assert 0.02 < float((f["hcl"] == 0).float().mean()) < 1.0 and float(f["g.classifier.0.weight"].abs().max()) > 0
    assert float(f["dy1pad"].float().abs().max()) > 0 and float(f["g.pos_embed.pos_embed.weight"].abs().max()) > 0
    # evaluation mode without labels: logits only, gradients from an external logit gradient
    f = run(model, eng, True, x1, x2, None, False, dict(glogits=ext["glogits"]))
    s = run(model, eng, False, x1, x2, None, False, dict(glogits=ext["glogits"]))
    compare(f, s, skip=("sloss", "loss"))
    assert torch.equal(f["loss"], torch.full_like(f["loss"], 7.0)) and torch.equal(s["loss"], f["loss"])   # untouched without labels
    # evaluation mode with labels
    f = run(model, eng, True, x1, x2, labels, False, dict(gloss=one))
    s = run(model, eng, False, x1, x2, labels, False, dict(gloss=one))
    compare(f, s)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_fused_tail_with_external_gradients(dtype):
    model, eng, x1, x2, labels, ext = build(dtype, 32)
    kw = dict(gloss=torch.full((1,), 0.5, device=DEV), **ext)
    f = run(model, eng, True, x1, x2, labels, True, kw)
    s = run(model, eng, False, x1, x2, labels, True, kw)
    compare(f, s)


def test_the_step_keeps_training_on_the_fused_route():
    """a few optimiser steps on each route from the same start: same parameters, bit for bit"""
    from eyegaze_multimodal_amd import HipAdamW
    finals = []
    for fused in (True, False):
        model, eng, x1, x2, labels, _ = build("bf16", 32)
        eng.fused_tail = fused
        opt = HipAdamW(model)
        for i in range(3):
            opt.begin_step(eng, seed=100 + i)
            eng.forward(x1, x2, labels, train=True)
            eng.backward(gloss=torch.ones(1, device=DEV))
            opt.step(eng)
        torch.cuda.synchronize()
        finals.append((model._flat.flat.clone(), eng.a["loss"].clone()))
    assert torch.equal(finals[0][0], finals[1][0]) and torch.equal(finals[0][1], finals[1][1])
