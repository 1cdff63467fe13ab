"""The image encoder at the reference's image size, 224 x 224 (`data.image_size`), and at the image store's limit 512 x 512: conv-1 on
the banded kernels (csrc/spec.hip), conv-2 on the segmented-row eg_gemm_nt / eg_gemm_tn in every dtype (rows too wide for the
flat-correlation kernels).  d_model 64, B = 2, images from synth_multimodal.  Gates:
  f32   logits against oracle.multimodal_oracle.image_logits within 2e-5, parameter gradients against torch autograd within 1e-3
        relative norm per parameter -- those of tests/test_gpu_multimodal.py::test_image_branch_matches_torch_cnn (at 2 x 224 x 224 the
        oracle's f32 and f64 logits differ by 1e-8 and max |logit| is 0.11: the same room as at 64 x 16);
  bf16  logits finite and within 2e-2 of the f32 device logits relative to max |logit|, the project's 16-bit tolerance;
  step  one MultimodalTrainer.train_step + evaluate against oracle Stepper with the loss / gradient gates of
        test_f32_steps_match_the_cpu_restatement."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd.image_encoder import GazeCNNEncoder  # noqa: E402
from eyegaze_multimodal_amd.train_multimodal_fuzzy_fusion import MultimodalTrainer, synth_multimodal  # noqa: E402
from oracle import dual_eeg_oracle as O  # noqa: E402
from oracle import fuzzy_oracle as FO  # noqa: E402
from oracle.multimodal_oracle import Stepper, image_logits  # noqa: E402
from tests.test_gpu_multimodal import DEV, KW, make  # noqa: E402

B, SIZE = 2, 224


def encoder(dtype, state=None):
    torch.manual_seed(3)
    enc = GazeCNNEncoder(num_classes=3, d_model=64, compute_dtype=dtype)
    if state is not None:
        enc.load_state_dict(state)
    return enc


@functools.lru_cache(maxsize=None)
def f32_case():
    """the f32 engine's logits and gradients at 2 x 224 x 224, with the CPU module they are checked against (shared, never modified)"""
    enc = encoder("f32")
    cpu = copy.deepcopy(enc).eval()
    img1, img2, *_ = synth_multimodal(B, 8, 1024, SIZE, SIZE, 3, seed=1)
    gl = torch.randn(B, 3, generator=torch.Generator().manual_seed(2))
    enc = enc.to(DEV)
    eng = enc.engine(B, SIZE, SIZE, DEV)
    assert eng.sp["band_rows"] == 16 and eng.sp["nbands"] == 7
    logits = eng.forward(img1.to(DEV), img2.to(DEV), train=False).cpu().clone()
    eng.backward(gl.to(DEV))
    torch.cuda.synchronize()
    fp = enc._flat
    grads = {n: fp.grad[fp.offsets[n]: fp.offsets[n] + p.numel()].view(p.shape).cpu().double() for n, p in enc.named_parameters()}
    return dict(cpu=cpu, img1=img1, img2=img2, gl=gl, logits=logits, grads=grads)


def test_f32_logits_and_gradients_match_torch_at_224():
    c = f32_case()
    cpu = copy.deepcopy(c["cpu"])
    with torch.no_grad():
        ref = image_logits(cpu, c["img1"], c["img2"])
    err = float((c["logits"] - ref).abs().max())
    print(f"image 224 f32: max |dlogit| {err:.3e}, max |logit| {float(ref.abs().max()):.3e}")
    assert err < 2e-5
    (image_logits(cpu, c["img1"], c["img2"]) * c["gl"]).sum().backward()
    for n, q in cpu.named_parameters():
        r = q.grad.double()
        rel = float((c["grads"][n] - r).norm() / r.norm().clamp_min(1e-12))
        print(f"  grad {n}: relative error {rel:.3e}")
        assert rel < 1e-3, n


def test_bf16_logits_stay_within_the_16_bit_tolerance_of_f32_at_224():
    """the first 16-bit run of the segmented-row conv-2 route at any size (narrow images take the flat-correlation kernels)"""
    c = f32_case()
    enc = encoder("bf16", c["cpu"].state_dict()).to(DEV)
    eng = enc.engine(B, SIZE, SIZE, DEV)
    got = eng.forward(c["img1"].to(DEV), c["img2"].to(DEV), train=False).cpu()
    assert bool(torch.isfinite(got).all())
    rel = float((got - c["logits"]).abs().max() / c["logits"].abs().max())
    print(f"image 224 bf16: max |dlogit| / max |logit| {rel:.3e}")
    assert rel <= 2e-2, rel


def test_one_trainer_step_and_evaluate_at_224_match_the_cpu_restatement():
    model = make("f32")
    img1, img2, x1, x2, y = synth_multimodal(B, 8, 1024, SIZE, SIZE, 3, seed=5)
    hp = dict(encoder_lr=2e-4, fusion_lr=2e-3, weight_decay=0.01, max_grad_norm=1.0)
    cpu_gaze = copy.deepcopy(model.gaze_encoder)
    eeg_sd = {k: v.clone() for k, v in model.eeg_encoder.state_dict().items()}
    fus_sd = {k: v.clone() for k, v in model.fusion.state_dict().items()}
    ref = Stepper(cpu_gaze, O.ModelCfg(**KW), eeg_sd, fus_sd, "full", hp["encoder_lr"], hp["fusion_lr"], hp["weight_decay"],
                  hp["max_grad_norm"], (0.3, 0.3, 0.1), (0.5, 5.0), warmup_steps=2, total_steps=10)
    tr = MultimodalTrainer(model, DEV, **hp, warmup_steps=2, total_steps=10)
    d = lambda t_: t_.to(DEV)
    out = tr.train_step(d(img1), d(img2), d(x1), d(x2), d(y), dropout=False)
    r = ref.step(img1, img2, x1, x2, y)
    torch.cuda.synchronize()
    print(f"step at 224: loss {float(out['loss']):.6f} vs {float(r['loss']):.6f}")
    assert abs(float(out["loss"]) - float(r["loss"])) < 2e-5, (float(out["loss"]), float(r["loss"]))
    np.testing.assert_allclose(out["alpha"].cpu().numpy(), r["alpha"].numpy(), atol=2e-5)
    np.testing.assert_allclose(out["fused_logits"].cpu().numpy(), r["fused"].numpy(), atol=5e-5)
    efp = model.eeg_encoder._flat
    for n, p in model.eeg_encoder.named_parameters():
        g = efp.grad[efp.offsets[n]: efp.offsets[n] + p.numel()].view(p.shape).cpu().double()
        rr = r["grads"]["eeg"][n].double()
        if float(rr.norm()) < 1e-7:
            continue
        assert float((g - rr).norm() / rr.norm()) < 3e-3, n
    gfp = model.gaze_encoder._flat
    gg = torch.cat([gfp.grad[gfp.offsets[n]: gfp.offsets[n] + p.numel()] for n, p in model.gaze_encoder.named_parameters()]).cpu().double()
    rel = float((gg - r["grads"]["gaze"].double()).norm() / r["grads"]["gaze"].double().norm())
    print(f"  gaze gradient relative error {rel:.3e}")
    assert rel < 3e-3
    st = model.eeg_encoder.engine(B, 1024, DEV).read_state()
    assert abs(st.grad_norm - float(r["norm"])) < 2e-3 * float(r["norm"])
    # evaluate: the fused cross-entropy of the restatement's parameters after its step, no dropout
    ev = tr.evaluate([(d(img1), d(img2), d(x1), d(x2), d(y))])
    with torch.no_grad():
        z_img = image_logits(ref.gaze, img1, img2)
        z_eeg = O.forward(x1, x2, {**ref.eeg, **ref.buf}, ref.cfg, y)["logits"]
        fused, _, _ = FO.fuzzy_forward_torch(z_img, z_eeg, ref.fus, "full")
        want = float(F.cross_entropy(fused, y))
    print(f"  evaluate loss {ev['loss']:.6f} vs {want:.6f}")
    assert abs(ev["loss"] - want) < 2e-5, (ev["loss"], want)
    top = fused.topk(2, -1).values
    if float((top[:, 0] - top[:, 1]).min()) > 1e-3:             # every sample decided far beyond the f32 gate: the same labels
        assert ev["accuracy"] == float((fused.argmax(-1) == y).float().mean())


def test_bf16_forward_and_backward_at_512_are_finite_and_repeatable():
    enc = encoder("bf16").to(DEV)
    img1, img2, *_ = synth_multimodal(B, 8, 1024, 512, 512, 3, seed=1)
    gl = torch.randn(B, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    eng = enc.engine(B, 512, 512, DEV)
    assert eng.sp["band_rows"] == 8 and eng.sp["nbands"] == 32
    runs = []
    for _ in range(2):
        logits = eng.forward(img1.to(DEV), img2.to(DEV), train=True).cpu().clone()
        eng.backward(gl)
        torch.cuda.synchronize()
        runs.append((logits, enc._flat.grad.cpu().clone()))
    assert bool(torch.isfinite(runs[0][0]).all()) and bool(torch.isfinite(runs[0][1]).all())
    assert float(runs[0][1].abs().max()) > 0
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
