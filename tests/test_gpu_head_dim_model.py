"""Whole model at attention head width 64 (d_model / num_heads = 64: every attention call site on eg_attention_dk_*), through
DualEEGTransformer:
  * the two fixtures written by the reference at d_model 128 with 2 heads (tests/golden/hd64_*.npz): eval forward in bf16 and
    fp16, f32 forward and gradients -- the gates of tests/test_gpu_model.py;
  * an f32 train-mode step with the kernels' dropout masks replayed in the oracle;
  * a long window (S = 257) against the oracle;
  * the attention-probability hook, a graph-captured step, and the trainer on d_model 256 with 4 heads."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import DualEEGTransformer, HipAdamW  # noqa: E402
from eyegaze_multimodal_amd.data import randn_windows  # noqa: E402
from oracle import dual_eeg_oracle as O  # noqa: E402
from tests.hd64_golden import HD64_CONFIGS, load_hd64  # noqa: E402
from tests.helpers import WEIGHT_SEED, t  # noqa: E402
from tests.test_gpu_model import _check_token_stages, relerr  # noqa: E402

DEV = "cuda"


def build(name, dtype="bf16", **over):
    z, kw, cfg, sd = load_hd64(name)
    if over:
        kw = dict(kw, **over)
        cfg = O.ModelCfg(**kw)
        sd = O.synthetic_state_dict(cfg, WEIGHT_SEED)
    model = DualEEGTransformer(**kw, compute_dtype=dtype)
    assert list(model.state_dict().keys()) == list(sd.keys())
    model.load_state_dict(sd, strict=True)
    return z, kw, cfg, sd, model.to(DEV)


def the_engine(model):
    eng = next(iter(model._engines.values()))
    assert eng.head_dim == 64 and eng.attn_long and not eng.attn_block and eng._attn_core == "eg_attention_dk"
    return eng


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", HD64_CONFIGS)
@pytest.mark.parametrize("kind", ["randn", "gen_eeg"])
def test_eval_forward_matches_reference(name, kind, dtype):
    """tests/test_gpu_model.py::test_eval_forward_matches_reference's gates.  The reference's smallest top-2 margin on these inputs
    is 0.77, so every sample is decided and argmax must be equal on all of them."""
    z, kw, cfg, sd, model = build(name, dtype)
    model.eval()
    x1, x2, labels = t(z[f"{kind}/eeg1"]).to(DEV), t(z[f"{kind}/eeg2"]).to(DEV), t(z["labels"]).to(DEV)
    with torch.no_grad():
        out = model(x1, x2, labels)
    torch.cuda.synchronize()
    eng = the_engine(model)
    ref_logits = z[f"{kind}/out/logits"]
    got = out["logits"].cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - ref_logits).max()
    NB, S, d = eng.NB, eng.S, cfg.d_model
    e_h1 = relerr(eng.a["h1"].float().cpu().view(NB, eng.T2, d)[:2], z[f"{kind}/stage/h1"])
    e_zn = relerr(eng.a["zn"].float().cpu().view(NB, S, d)[:2], z[f"{kind}/stage/z1"])
    e_zc = relerr(eng.a["zc"].float().cpu().view(NB, S, d)[:2], z[f"{kind}/stage/zc1"])
    print(f"{name} {kind} {dtype}: max|dlogit| {err:.3e}  h1 {e_h1:.3e}  z1 {e_zn:.3e}  zc1 {e_zc:.3e}")
    assert err <= 3e-2, f"logits err {err}"
    top2 = np.sort(ref_logits, -1)
    assert ((top2[:, -1] - top2[:, -2]) > 4e-2).all()
    assert (got.argmax(-1) == z[f"{kind}/out/argmax"]).all()
    assert abs(float(out["loss_ce"]) - float(z[f"{kind}/out/loss_ce"])) < 2e-2
    for k in ("cls1", "cls2", "ibs_token"):
        if k in out:
            assert relerr(out[k].cpu(), z[f"{kind}/out/{k}"]) < 3e-2, k
    if "ibs_logits" in out:
        assert np.abs(out["ibs_logits"].cpu().numpy() - z[f"{kind}/out/ibs_logits"]).max() < 3e-2
        assert abs(float(out["loss_ibs_cls"]) - float(z[f"{kind}/out/loss_ibs_cls"])) < 2e-2
    _check_token_stages(z, kind, cfg, eng, tight=False)
    assert e_h1 < 2e-2 and e_zn < 3e-2 and e_zc < 3e-2


@pytest.mark.parametrize("name", HD64_CONFIGS)
@pytest.mark.parametrize("kind", ["randn", "gen_eeg"])
def test_f32_forward_and_gradients_are_tight(name, kind):
    """tests/test_gpu_model.py::test_f32_forward_and_gradients_are_tight's gates: logits 4e-6, argmax on every sample, gradient
    norms 1e-3 without synchrony tokens and 2e-2 with."""
    z, kw, cfg, sd, model = build(name, "f32")
    model.eval()
    x1, x2, labels = t(z[f"{kind}/eeg1"]).to(DEV), t(z[f"{kind}/eeg2"]).to(DEV), t(z["labels"]).to(DEV)
    out = model(x1, x2, labels)
    loss = out["loss_ce"] + (out["loss_ibs_cls"] if "loss_ibs_cls" in out else 0.0)
    loss.backward()
    torch.cuda.synchronize()
    eng = the_engine(model)
    ltol, gtol = (4e-6, 2e-2) if cfg.use_ibs else (4e-6, 1e-3)
    got = out["logits"].detach().cpu().numpy()
    names = [str(n) for n in z[f"{kind}/grad/names"]]
    params = dict(model.named_parameters())
    gscale = float(z[f"{kind}/grad/global_norm"])
    norm_err = max(abs(float(params[n].grad.norm()) - ref) / max(ref, 1e-3 * gscale) for n, ref in zip(names, z[f"{kind}/grad/norms"]))
    print(f"{name} {kind} f32: max|dlogit| {np.abs(got - z[f'{kind}/out/logits']).max():.3e}  worst gradient-norm error {norm_err:.3e}")
    assert np.abs(got - z[f"{kind}/out/logits"]).max() <= ltol
    assert (got.argmax(-1) == z[f"{kind}/out/argmax"]).all()
    assert abs(float(out["loss_ce"].detach()) - float(z[f"{kind}/out/loss_ce"])) < ltol
    _check_token_stages(z, kind, cfg, eng, tight=True)
    for k in ("cls1", "cls2"):
        np.testing.assert_allclose(out[k].detach().cpu().numpy(), z[f"{kind}/out/{k}"], rtol=10 * ltol, atol=ltol)
    for n, ref in zip(names, z[f"{kind}/grad/norms"]):
        got_n = float(params[n].grad.norm())
        assert abs(got_n - ref) <= 2 * gtol * ref + 1e-6 * gscale, (n, got_n, ref)
    for key in z.files:
        if key.startswith(f"{kind}/grad/full/"):
            n = key.split("/full/")[1]
            ref = torch.from_numpy(z[key]).double()
            g = params[n].grad.cpu().double()
            if float(ref.norm()) < 1e-5 * gscale:  # k_proj.bias: mathematically zero (soft-max shift invariance)
                assert float(g.norm()) < 1e-5 * gscale, n
                continue
            assert float((g - ref).norm() / ref.norm()) < gtol, n


def test_f32_train_step_with_dropout_matches_oracle_with_identical_masks():
    """hd64_xattn, f32, dropout 0.1 at every site; the oracle replays the kernels' masks (the attention index does not depend on the
    head width).  Logits to 2e-4 (tests/test_gpu_model.py's train-mode gate), every parameter gradient to 1e-3 relative."""
    from tests.helpers import hip_dropout_override
    z, kw, cfg, sd, model = build("hd64_xattn", "f32")
    assert cfg.dropout == 0.1
    model.train()
    kind, seed = "gen_eeg", 0x1234_5678_9ABC
    x1c, x2c, labc = t(z[f"{kind}/eeg1"]), t(z[f"{kind}/eeg2"]), t(z["labels"])
    B = x1c.shape[0]
    eng = model.engine(B, x1c.shape[2], torch.device(DEV))
    the_engine(model)
    eng.set_state(seed=seed, lr=0.0, step=1)
    eng.forward(x1c.to(DEV), x2c.to(DEV), labc.to(DEV), train=True)
    eng.backward(gloss=torch.ones(1, device=DEV))
    torch.cuda.synchronize()
    got_logits = eng.a["logits"].cpu().numpy()
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    O.DROPOUT_OVERRIDE = hip_dropout_override(seed, B, cfg.num_layers, O.CTX)
    try:
        out = O.forward(x1c, x2c, params, cfg, labc, train=True)
        out["loss_ce"].backward()
    finally:
        O.DROPOUT_OVERRIDE = None
    ref_logits = out["logits"].detach().numpy()
    assert np.abs(ref_logits - z[f"{kind}/out/logits"]).max() > 1e-3           # the masks were active
    fp = model._flat
    gflat = fp.grad.cpu().double()
    gnorm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params.values() if p.grad is not None)))
    worst, worst_n = 0.0, None
    for n, p in zip(fp.names, fp.params):
        ref = params[n].grad
        if ref is None:
            continue
        g = gflat[fp.offsets[n]: fp.offsets[n] + p.numel()].view(p.shape)
        if float(ref.norm()) < 1e-5 * gnorm:
            assert float(g.norm()) < 1e-4 * gnorm, n
            continue
        rel = float((g - ref.double()).norm() / ref.double().norm())
        if rel > worst:
            worst, worst_n = rel, n
    print(f"hd64_xattn train f32: max|dlogit| {np.abs(got_logits - ref_logits).max():.3e}  worst relative gradient error "
          f"{worst:.3e} ({worst_n})")
    assert np.abs(got_logits - ref_logits).max() <= 2e-4
    assert worst < 1e-3, (worst_n, worst)


# max |dlogit| at S = 257: f32 is tests/test_gpu_long_window.py's gate; the 16-bit gates are 1.5x the largest error measured on the
# MI355X with these seeds (LONG_MEASURED), capped by that file's A1 gates (bf16 1.6e-2, fp16 1.2e-3)
LONG_MEASURED = {"bf16": 6.327e-3, "fp16": 9.093e-4}        # (f32 measured 1.55e-6)
LONG_CAP = {"bf16": 1.6e-2, "fp16": 1.2e-3}
LONG_GATE = {"f32": 1.8e-6, **{k: min(LONG_CAP[k], 1.5 * LONG_MEASURED[k]) for k in LONG_CAP}}     # bf16 9.5e-3, fp16 1.2e-3 (the cap)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "fp16"])
def test_long_window_eval_logits_match_the_oracle(dtype):
    """the hd64_xattn model with max_len 1024 at T = 4096: S = 257 > 160"""
    B, T = 4, 4096
    z, kw, cfg, sd, model = build("hd64_xattn", dtype, max_len=1024)
    model.eval()
    x1, x2, labels = randn_windows(B, cfg.in_channels, T, seed=21, num_classes=cfg.num_classes)
    with torch.no_grad():
        got = model(x1.to(DEV), x2.to(DEV), labels.to(DEV))["logits"].float().cpu().numpy()
        ref = O.forward(x1, x2, sd, cfg, labels)["logits"].numpy()
    eng = the_engine(model)
    assert eng.S == 257
    err = float(np.abs(got - ref).max())
    print(f"hd64_xattn window {T} {dtype}: max|dlogit| = {err:.3e}")
    assert err <= LONG_GATE[dtype], err
    if dtype == "f32":
        assert (got.argmax(-1) == ref.argmax(-1)).all()


def test_attention_probability_hook_at_width_64():
    """[B, 2, S, S] per stream / direction from eg_attention_dk_probs against the oracle's cross-attention probabilities"""
    z, kw, cfg, sd, model = build("hd64_xattn", "bf16")
    model.eval()
    x1, x2 = t(z["gen_eeg/eeg1"]), t(z["gen_eeg/eeg2"])
    seen = []
    h = model.cross_attn.cross_attn.dropout.register_forward_hook(lambda m, i, o: seen.append(i[0].detach().cpu()))
    with torch.no_grad():
        model(x1.to(DEV), x2.to(DEV))
    h.remove()
    the_engine(model)
    st = {}
    with torch.no_grad():
        O.forward(x1, x2, sd, cfg, stages=st)
    assert len(seen) == 2 and tuple(seen[0].shape) == (4, 2, 65, 65)      # direction 1 (q = stream 1), then direction 2
    got = torch.stack(seen).numpy()
    np.testing.assert_allclose(got.sum(-1), 1.0, atol=2e-3)
    print(f"hd64 hook bf16: max|dprob| {np.abs(got - st['xattn_probs'].numpy()).max():.3e}")
    np.testing.assert_allclose(got, st["xattn_probs"].numpy(), atol=2e-2)


def test_captured_step_replays_bit_identically():
    """hd64_xattn, bf16, train mode: a graph-captured training step (graph.py) gives the bits of the eager step."""
    from eyegaze_multimodal_amd.graph import GraphedStep
    z = load_hd64("hd64_xattn")[0]
    x1, x2, labels = t(z["randn/eeg1"]).to(DEV), t(z["randn/eeg2"]).to(DEV), t(z["labels"]).to(DEV)
    one = torch.ones(1, device=DEV)
    runs = []
    for graphed in (False, True):
        _, kw, cfg, sd, model = build("hd64_xattn", "bf16")
        model.train()
        eng = model.engine(x1.shape[0], x1.shape[2], torch.device(DEV))
        the_engine(model)
        opt = HipAdamW(model)
        opt.begin_step(eng, seed=5)              # warm-up step: every buffer exists before a capture
        eng.forward(x1, x2, labels, train=True)
        eng.backward(gloss=one)
        opt.step(eng)
        opt.begin_step(eng, seed=6)
        if graphed:
            GraphedStep(eng, opt, train=True).run(x1, x2, labels)
        else:
            eng.forward(x1, x2, labels, train=True)
            eng.backward(gloss=one)
            opt.step(eng)
        torch.cuda.synchronize()
        runs.append((model._flat.flat.clone(), model._flat.grad.clone(), eng.a["logits"].clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_trainer_steps_with_four_heads_at_d_model_256(tmp_path):
    """train_art's Trainer from a config with d_model 256 and 4 heads: head width 64, the fused FFN and LayerNorm-backward routes
    stay on (they depend on d_model only), the fused attention block (8 heads) is off."""
    from eyegaze_multimodal_amd.data import synth_windows
    from eyegaze_multimodal_amd.train_art import Trainer
    from tests.test_gpu_train import make_config
    cfg = make_config(tmp_path, model={"num_heads": 4, "num_layers": 2})
    tr = Trainer(cfg, torch.device(DEV))
    x1, x2, y = synth_windows(16, 8, 1024, 3, seed=3)
    losses = []
    for _ in range(3):
        out = tr.train_step(x1.cuda(), x2.cuda(), y.cuda())
        losses.append({k: float(v) for k, v in out.items()})
    assert all(np.isfinite(list(l.values())).all() for l in losses), losses
    eng = next(iter(tr.model._engines.values()))
    assert eng.head_dim == 64 and eng.cfg.num_heads == 4
    assert eng.fuse_ffn and eng.ln_proj and not eng.attn_block and eng.attn_long
