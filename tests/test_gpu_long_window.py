"""Whole model at long windows (S > 160: the long-sequence attention core at every attention call site), built through
train_art.build_model with data.window_size set, so max_len follows the reference's window_size // 4:
  A5 full model (C = 32: cross-attention, spectrogram, robust IBS) at window 2048 -> S = 203;
  A1 temporal only and A2 + spectrogram at window 4096 -> S = 257 / 289.
Logits against the CPU oracle on the same weights, an f32 training step's gradients against oracle autograd, a train-mode step
with the kernels' own dropout masks replayed in the oracle, a graph-captured step, and the attention-probability hook."""
import copy
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import HipAdamW  # noqa: E402
from eyegaze_multimodal_amd import train_art as TA  # noqa: E402
from eyegaze_multimodal_amd.data import randn_windows  # noqa: E402
from oracle import dual_eeg_oracle as O  # noqa: E402
from tests.helpers import GOLDEN, WEIGHT_SEED  # noqa: E402

DEV = "cuda"
B = 4
CASES = [("A5_full_model", 2048, 203), ("A1_baseline_temporal_only", 4096, 257), ("A2_plus_spectrogram", 4096, 289)]
# max |dlogit| gates, <= 1.5x the largest error measured on the MI355X with these seeds over two runs (A5 / A1 / A2: f32 1.01e-6 /
# 7.2e-7 / 1.21e-6, bf16 1.40e-2 / 1.09e-2 / 1.22e-2, fp16 1.14e-3 / 8.1e-4 / 8.7e-4); all inside tests/test_gpu_logits512.py's
# a5_full gates (f32 5e-5 here, bf16 2.9e-2, fp16 4.3e-3).  A5 takes the oracle's synchrony features (oracle_conn_hook), so its
# gate measures the attention path.
GATE = {"A5_full_model": {"f32": 1.5e-6, "bf16": 2.1e-2, "fp16": 1.7e-3},
        "A1_baseline_temporal_only": {"f32": 1.8e-6, "bf16": 1.6e-2, "fp16": 1.2e-3},
        "A2_plus_spectrogram": {"f32": 1.8e-6, "bf16": 1.8e-2, "fp16": 1.3e-3}}
# f32 gradients, relative Frobenius per parameter: tests/test_gpu_model.py's 1e-3 at window 2048; at 4096 the front-end's weight
# gradients sum twice as many rows (temporal_conv.convs.0.weight measured 1.53e-3, the worst)
GRAD_GATE = {"A5_full_model": 1e-3, "A2_plus_spectrogram": 2.2e-3}


def build(name, window, dtype):
    fx = json.loads((GOLDEN / "reference_configs.json").read_text())
    cfg = copy.deepcopy(next(e["config"] for e in fx["entries"] if e["name"] == name))
    cfg["data"]["window_size"] = window
    model = TA.build_model(cfg, compute_dtype=dtype)
    ocfg = O.ModelCfg(**{k: getattr(model.cfg, k) for k in O.ModelCfg.__dataclass_fields__})
    assert ocfg.max_len == window // 4
    sd = O.synthetic_state_dict(ocfg, WEIGHT_SEED)
    model.load_state_dict(sd, strict=True)
    return model.to(DEV), ocfg, sd


def inputs(ocfg, window, seed=11):
    x1, x2, labels = randn_windows(B, ocfg.in_channels, window, seed=seed, num_classes=ocfg.num_classes)
    return x1, x2, labels


def oracle_conn_hook(model, ocfg, x1, x2):
    """the synchrony features from the oracle (forward-hook contract of the matrix generator), so that the logit gate measures
    the attention path and not the sign() decisions of PLI / wPLI (tests/test_gpu_logits512.py)"""
    if not (ocfg.use_ibs and ocfg.use_robust_ibs):
        return None
    ref = O.ibs_connectivity(x1, x2, ocfg)
    return model.ibs_matrix_generator.register_forward_hook(lambda mod, inp, out: ref.to(out.device, out.dtype))


@pytest.mark.parametrize("dtype", ["f32", "bf16", "fp16"])
@pytest.mark.parametrize("name,window,S", CASES)
def test_eval_logits_match_the_oracle(name, window, S, dtype):
    model, ocfg, sd = build(name, window, dtype)
    model.eval()
    x1, x2, labels = inputs(ocfg, window)
    oracle_conn_hook(model, ocfg, x1, x2)
    with torch.no_grad():
        got = model(x1.to(DEV), x2.to(DEV), labels.to(DEV))["logits"].float().cpu().numpy()
        ref = O.forward(x1, x2, sd, ocfg, labels)["logits"].numpy()
    eng = next(iter(model._engines.values()))
    assert eng.S == S and eng.attn_long
    err = float(np.abs(got - ref).max())
    print(f"{name} window {window} {dtype}: max|dlogit| = {err:.3e}")
    assert err <= GATE[name][dtype], err
    if dtype == "f32":
        assert (got.argmax(-1) == ref.argmax(-1)).all()


@pytest.mark.parametrize("name,window,S", [CASES[0], CASES[2]])
def test_f32_training_step_gradients_match_oracle_autograd(name, window, S):
    model, ocfg, sd = build(name, window, "f32")
    model.eval()
    x1, x2, labels = inputs(ocfg, window, seed=12)
    oracle_conn_hook(model, ocfg, x1, x2)
    out = model(x1.to(DEV), x2.to(DEV), labels.to(DEV))
    loss = out["loss_ce"] + (out["loss_ibs_cls"] if "loss_ibs_cls" in out else 0.0)
    loss.backward()
    torch.cuda.synchronize()
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ro = O.forward(x1, x2, params, ocfg, labels)
    (ro["loss_ce"] + (ro["loss_ibs_cls"] if "loss_ibs_cls" in ro else 0.0)).backward()
    fp = model._flat
    gflat = fp.grad.cpu().double()
    gnorm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params.values() if p.grad is not None)))
    assert abs(float(gflat.norm()) / gnorm - 1) < 1e-3
    worst, worst_n = 0.0, None
    for n, p in zip(fp.names, fp.params):
        ref = params[n].grad
        if ref is None:
            continue
        g = gflat[fp.offsets[n]: fp.offsets[n] + p.numel()].view(p.shape)
        if float(ref.norm()) < 1e-5 * gnorm:      # k_proj.bias: mathematically zero (soft-max shift invariance)
            assert float(g.norm()) < 1e-4 * gnorm, n
            continue
        rel = float((g - ref.double()).norm() / ref.double().norm())
        if rel > worst:
            worst, worst_n = rel, n
    print(f"{name} window {window}: worst relative gradient error {worst:.3e} ({worst_n})")
    assert worst < GRAD_GATE[name], (worst_n, worst)


def test_train_mode_step_with_dropout_matches_oracle_with_identical_masks():
    """A1 at window 4096 (S = 257), f32, dropout 0.1 at every site: the oracle replays the kernels' masks (the attention element
    indices stay below 2^32 here, so tests/helpers.py's replica applies)."""
    from tests.helpers import hip_dropout_override
    name, window, _ = CASES[1]
    model, ocfg, sd = build(name, window, "f32")
    model.train()
    x1, x2, labels = inputs(ocfg, window, seed=13)
    seed = 0x1234_5678_9ABC
    eng = model.engine(B, window, torch.device(DEV))
    assert eng.attn_long and eng.NB * ocfg.num_heads * eng.S * (eng.S + 1) < 1 << 32
    eng.set_state(seed=seed, lr=0.0, step=1)
    eng.forward(x1.to(DEV), x2.to(DEV), labels.to(DEV), train=True)
    eng.backward(gloss=torch.ones(1, device=DEV))
    torch.cuda.synchronize()
    got_logits = eng.a["logits"].cpu().numpy()
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    O.DROPOUT_OVERRIDE = hip_dropout_override(seed, B, ocfg.num_layers, O.CTX)
    try:
        out = O.forward(x1, x2, params, ocfg, labels, train=True)
        out["loss_ce"].backward()
    finally:
        O.DROPOUT_OVERRIDE = None
    with torch.no_grad():
        ev = O.forward(x1, x2, sd, ocfg, labels)["logits"].numpy()
    ref_logits = out["logits"].detach().numpy()
    assert np.abs(ref_logits - ev).max() > 1e-3                     # the masks were active
    assert np.abs(got_logits - ref_logits).max() <= 2e-4, np.abs(got_logits - ref_logits).max()
    fp = model._flat
    gflat = fp.grad.cpu().double()
    gnorm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params.values() if p.grad is not None)))
    assert abs(float(gflat.norm()) / gnorm - 1) < 5e-3
    for n, p in zip(fp.names, fp.params):
        ref = params[n].grad
        if ref is None or float(ref.norm()) < 1e-5 * gnorm:
            continue
        g = gflat[fp.offsets[n]: fp.offsets[n] + p.numel()].view(p.shape)
        assert float((g - ref.double()).norm() / ref.double().norm()) < 2e-3, n


def test_captured_step_replays_bit_identically():
    """A5 at window 2048 (S = 203), bf16: a graph-captured training step (graph.py) gives the bits of the eager step."""
    from eyegaze_multimodal_amd.graph import GraphedStep
    name, window, _ = CASES[0]
    x1, x2, labels = inputs(O.ModelCfg(in_channels=32), window, seed=14)
    x1, x2, labels = x1.to(DEV), x2.to(DEV), labels.to(DEV)
    runs = []
    for graphed in (False, True):
        model, ocfg, sd = build(name, window, "bf16")
        model.train()
        eng = model.engine(B, window, torch.device(DEV))
        opt = HipAdamW(model)
        opt.begin_step(eng, seed=5)              # warm-up step: every buffer exists before a capture
        eng.forward(x1, x2, labels, train=True)
        eng.backward(gloss=torch.ones(1, device=DEV), gloss_ibs=torch.ones(1, device=DEV))
        opt.step(eng)
        opt.begin_step(eng, seed=6)
        if graphed:
            GraphedStep(eng, opt, train=True).run(x1, x2, labels)
        else:
            eng.forward(x1, x2, labels, train=True)
            eng.backward(gloss=torch.ones(1, device=DEV), gloss_ibs=torch.ones(1, device=DEV))
            opt.step(eng)
        torch.cuda.synchronize()
        assert eng.attn_long
        runs.append((model._flat.flat.clone(), model._flat.grad.clone(), eng.a["logits"].clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_attention_probability_hook_delivers_long_windows():
    name, window, S = CASES[0]
    model, ocfg, sd = build(name, window, "bf16")
    model.eval()
    seen = []
    model.encoder.layers[0].mha.dropout.register_forward_hook(lambda mod, inp, out: seen.append(inp[0].detach().clone()))
    model.cross_attn.cross_attn.dropout.register_forward_hook(lambda mod, inp, out: seen.append(inp[0].detach().clone()))
    x1, x2, labels = inputs(ocfg, window, seed=15)
    with torch.no_grad():
        model(x1.to(DEV), x2.to(DEV), labels.to(DEV))
    torch.cuda.synchronize()
    assert len(seen) == 4                                   # both streams / directions of each hooked module
    for p in seen:
        assert tuple(p.shape) == (B, ocfg.num_heads, S, S)
        assert torch.isfinite(p).all()
        assert (p.sum(-1) - 1).abs().max().item() < 1e-3
