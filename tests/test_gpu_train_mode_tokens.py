"""TRAIN mode on the token-family configurations: synchrony tokens (matrix and scalar form), spectrogram tokens and the IBS
classifier head, with the oracle fed exactly the masks the kernels draw (tests/helpers.py::hip_dropout_override), as
tests/test_gpu_model.py::test_train_mode_matches_oracle_with_identical_masks does for the configurations without them.  The four
dropout sites these parts own, and their backward, are thereby checked exactly:
  SITE_IBSTOK  eg_gelu_fwd / eg_gelu_bwd          SITE_IBSGEN  GEMM drop1 forward, gate + gate_scale backward
  SITE_SPEC    the same in spec_cnn_forward/_backward   SITE_IBSCLS  p = 0.3 forward, eg_classifier_ce_bwd(use_gate, 1/0.7) backward
The loss is loss_ce + 0.5 * loss_ibs_cls, so a lost gloss_ibs scale shows.  Where the model has matrix-form synchrony tokens both
sides get the ORACLE's connectivity (a forward hook on ibs_matrix_generator / conn_edit=), so the sign()-based features cannot
loosen the gradient gate.

Negative controls (CPU only, on the one GPU result of a5_full f32): the oracle is handed a deliberately wrong mask at one site and
the f32 per-parameter gate must then fail by at least 10x on a parameter directly behind that site.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import DualEEGTransformer  # noqa: E402
from oracle import dual_eeg_oracle as O  # noqa: E402
from tests.helpers import hip_dropout_override, load_golden, t  # noqa: E402

DEV = "cuda"
KIND, SEED, W_IBS = "gen_eeg", 0x1234_5678_9ABC, 0.5
CASES = [("a5_full", "f32"), ("a3_ibs_scalar", "f32"), ("cfg5_a2_spec", "f32"), ("b1_no_inorm", "f32"), ("tiny_full", "f32"),
         ("a5_full", "bf16"), ("a3_ibs_scalar", "bf16")]
# gates: f32 (logits / losses, per-parameter relative Frobenius, global norm ratio); bf16 (logits / losses, norm ratio)
LTOL = {"f32": 2e-4, "bf16": 5e-2}
GTOL = 2e-3
NTOL = {"f32": 5e-3, "bf16": 8e-2}
# a pre-dropout value counts as positive when it exceeds what the compute dtype can move it by
POS = {"f32": 1e-3, "bf16": 5e-2}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    z, kw, cfg, sd = load_golden(name)
    x1, x2, lab = t(z[f"{KIND}/eeg1"]), t(z[f"{KIND}/eeg2"]), t(z["labels"])
    conn = O.ibs_connectivity(x1, x2, cfg) if (cfg.use_ibs and cfg.use_robust_ibs) else None
    return z, kw, cfg, sd, x1, x2, lab, conn


@functools.lru_cache(maxsize=None)
def _engine_run(name, dtype):
    """one train-mode forward + backward of the HIP engine; everything the checks read, on the CPU"""
    z, kw, cfg, sd, x1, x2, lab, conn = _inputs(name)
    model = DualEEGTransformer(**kw, compute_dtype=dtype)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    model.train()
    if conn is not None:
        model.ibs_matrix_generator.register_forward_hook(lambda mod, inp, out: conn.to(out.device, out.dtype))
    B = x1.shape[0]
    eng = model.engine(B, x1.shape[2], torch.device(DEV))
    eng.set_state(seed=SEED, lr=0.0, step=1)
    eng.forward(x1.to(DEV), x2.to(DEV), lab.to(DEV), train=True)
    got = {"logits": eng.a["logits"].float().cpu().numpy(), "loss": float(eng.a["loss"])}
    for key in ("hib", "sp_hp0", "ib_h", "ig_h"):
        if key in eng.a:
            got[key] = eng.a[key].float().cpu()
    one = torch.ones(1, device=DEV)
    if cfg.use_ibs:
        got["ibs_loss"] = float(eng.a["ibs_loss"])
        eng.backward(gloss=one, gloss_ibs=W_IBS * one)
    else:
        eng.backward(gloss=one)
    torch.cuda.synchronize()
    fp = model._flat
    gflat = fp.grad.cpu().double()
    got["grads"] = {n: gflat[fp.offsets[n]: fp.offsets[n] + p.numel()].view(p.shape).clone() for n, p in zip(fp.names, fp.params)}
    got["gnorm"] = float(gflat.norm())
    return got


@functools.lru_cache(maxsize=None)
def _oracle_run(name, defect=None):
    z, kw, cfg, sd, x1, x2, lab, conn = _inputs(name)
    # only the model's parameters take a gradient: spectrogram_generator.window is a buffer (D:66), not in the flat gradient
    params = {k: v.clone().requires_grad_(k != "spectrogram_generator.window") for k, v in sd.items()}
    log = {}
    O.DROPOUT_OVERRIDE = hip_dropout_override(SEED, x1.shape[0], cfg.num_layers, O.CTX, log=log, defect=defect)
    try:
        out = O.forward(x1, x2, params, cfg, lab, train=True, conn_edit=(None if conn is None else (lambda c: conn)))
        (out["loss_ce"] + (W_IBS * out["loss_ibs_cls"] if cfg.use_ibs else 0.0)).backward()
    finally:
        O.DROPOUT_OVERRIDE = None
    ref = {"logits": out["logits"].detach().numpy(), "loss": float(out["loss_ce"].detach()), "log": log,
           "grads": {k: (None if p.grad is None else p.grad.double()) for k, p in params.items()}}
    if cfg.use_ibs:
        ref["ibs_loss"] = float(out["loss_ibs_cls"].detach())
    ref["gnorm"] = float(torch.sqrt(sum((g ** 2).sum() for g in ref["grads"].values() if g is not None)))
    return ref


def _rel(got, ref, n):
    g, r = got["grads"][n], ref["grads"][n]
    return float((g - r).norm() / r.norm())


def _mask_sites(cfg, got, ref):
    """(activation of the engine, oracle keep mask, oracle pre-dropout value) per token-family dropout site of the configuration"""
    log, out = ref["log"], []
    if cfg.use_ibs:
        out.append(("hib", got["hib"], *log[("ibscls", 0)]))
        if cfg.use_robust_ibs:
            keep, pre = log[("ibstok", 0)]
            out.append(("ib_h", got["ib_h"], keep.reshape(-1, 64), pre.reshape(-1, 64)))
        else:
            out.append(("ig_h", got["ig_h"], *log[("ibsgen", 0)]))
    if cfg.use_spectrogram:
        keep = torch.cat([log[("spec", 0)][0], log[("spec", 1)][0]])
        pre = torch.cat([log[("spec", 0)][1], log[("spec", 1)][1]])
        out.append(("sp_hp0", got["sp_hp0"], keep, pre))
    return out


@pytest.mark.parametrize("name,dtype", CASES)
def test_train_mode_matches_oracle_on_token_configurations(name, dtype):
    """Measured on the MI355X against the oracle (gates: LTOL / GTOL / NTOL above, the start gates of the existing train-mode test;
    none needed widening).  Every mask site: 0 mismatches on all live elements.
      configuration      max|dlogit|  |dloss_ce|  |dloss_ibs|  |norm ratio - 1|  worst parameter (relative Frobenius)
      a5_full f32         1.07e-6      < 1e-7      < 1e-7       1.8e-6           1.59e-4  temporal_conv.convs.0.weight
      a3_ibs_scalar f32   1.79e-6      1.2e-7      3.0e-7       1.4e-7           3.87e-6  cross_attn.cross_attn.q_proj.weight
      cfg5_a2_spec f32    1.43e-6      2.4e-7      -            8.6e-6           7.05e-4  temporal_conv.convs.0.weight
      b1_no_inorm f32     1.40e-6      4.8e-7      2.4e-7       1.6e-5           4.32e-4  encoder.layers.3.ffn.linear1.weight
      tiny_full f32       9.5e-7       2.4e-7      1.2e-7       1.7e-7           2.42e-6  spectrogram_generator.spec_conv.3.bias
      a5_full bf16        7.31e-3      7.2e-4      2.70e-3      1.21e-2          (not gated: 2.8e-1, encoder.layers.0.mha.q_proj.bias)
      a3_ibs_scalar bf16  1.06e-2      1.87e-3     1.35e-3      2.58e-2          (not gated: 1.8e-1, cls_token)
    (The oracle's gradient of spectrogram_generator.window, a buffer, is left out: with it the norm ratio of tiny_full is off by
    7.2e-3.)"""
    z, kw, cfg, sd, x1, x2, lab, conn = _inputs(name)
    got, ref = _engine_run(name, dtype), _oracle_run(name)
    # the masks first, at their own sites: an error there is reported here and not three layers later
    for key, act, keep, pre in _mask_sites(cfg, got, ref):
        assert act.shape == keep.shape, (key, act.shape, keep.shape)
        live = pre > POS[dtype]
        assert int(live.sum()) > act.numel() // 8, key
        bad = int(((act != 0) != keep)[live].sum())
        print(f"{name} {dtype}: {key} mask mismatches {bad} of {int(live.sum())} live elements")
        assert bad == 0, (key, bad)
        assert float(act[~keep].abs().max()) == 0.0, key           # dropped elements are exact zeros whatever their value
    # both sides differentiate the same set: the model's parameters, each reached by the loss
    assert {n for n, r in ref["grads"].items() if r is not None} == set(got["grads"])
    dl = float(np.abs(got["logits"] - ref["logits"]).max())
    dce = abs(got["loss"] - ref["loss"])
    dibs = abs(got["ibs_loss"] - ref["ibs_loss"]) if cfg.use_ibs else 0.0
    dn = abs(got["gnorm"] / ref["gnorm"] - 1)
    worst, worst_n = 0.0, None
    zero = []
    for n, g in got["grads"].items():
        r = ref["grads"][n]
        if r is None:
            continue
        if float(r.norm()) < 1e-5 * ref["gnorm"]:      # k_proj.bias: mathematically zero (soft-max shift invariance)
            zero.append((n, float(g.norm())))
            continue
        rel = _rel(got, ref, n)
        if rel > worst:
            worst, worst_n = rel, n
    print(f"{name} {dtype}: max|dlogit| {dl:.3e}  |dloss_ce| {dce:.3e}  |dloss_ibs| {dibs:.3e}  |norm ratio - 1| {dn:.3e}  "
          f"worst parameter {worst:.3e} ({worst_n})")
    assert dl <= LTOL[dtype], dl
    assert dce <= LTOL[dtype] and dibs <= LTOL[dtype], (dce, dibs)
    # masks really were active: train-mode logits differ from the eval fixture
    assert float(np.abs(ref["logits"] - z[f"{KIND}/out/logits"]).max()) > 1e-3
    assert dn < NTOL[dtype], dn
    if dtype == "f32":
        for n, gn in zero:
            assert gn < 1e-4 * ref["gnorm"], n
        assert worst < GTOL, (worst_n, worst)


@pytest.mark.parametrize("defect,param", [("spec_stream0", "spectrogram_generator.proj.3.weight"),
                                          ("ibstok_shift", "ibs_tokenizer.bottleneck.3.weight"),
                                          ("ibscls_noscale", "ibs_classifier.3.weight")])
def test_gate_sees_a_wrong_mask(defect, param):
    """Negative control, no further GPU work: the oracle gets stream 0's spec mask for both streams (its behaviour before it set
    CTX["stream"] around the spectrogram calls) / the ibstok element index shifted by one / the ibscls mask without 1/(1-p); the
    engine's f32 gradients of a5_full must then miss the per-parameter gate by at least 10x on the parameter behind the site, and
    pass it against the true masks.  Measured (gate 2e-3), defective / true oracle: spec_stream0 2.25e-1 / 6.1e-5, ibstok_shift
    3.40e-1 / 6.9e-5, ibscls_noscale 5.48e-1 / 5.9e-7."""
    got = _engine_run("a5_full", "f32")
    good, bad = _rel(got, _oracle_run("a5_full"), param), _rel(got, _oracle_run("a5_full", defect), param)
    print(f"{defect}: {param} relative error {bad:.3e} against the defective oracle, {good:.3e} against the true one")
    assert good < GTOL, good
    assert bad > 10 * GTOL, bad
