"""DualEEGTransformer.predict -- the forward-only engine -- at the model level.  The inference route runs the arithmetic of an
eval-mode forward (the lean launches are the keeping launches without their stores; everything else is the same launch into a
shared scratch set), so every returned key is compared BIT FOR BIT with forward's, on every route: lean (cfg3 in bf16 / fp16), fp32
and EYEGAZE_LN_FUSE=0 (scratch route), S = 115 (three-launch attention), 64-wide heads, the long core at window 2048.  In f32 predict
is also held to the reference's own logits.  Then what predict must NOT do: touch the step state, the forward counter, the dropout
seeds or a gradient buffer; and the loops built on it (predict_windows, Trainer.evaluate with training.inference_eval)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd.engine import InferenceEngine  # noqa: E402
from tests.helpers import t  # noqa: E402
from tests.test_gpu_model import build  # noqa: E402

DEV = "cuda"
REPO = Path(__file__).resolve().parent.parent


def fixture_inputs(z, kind="randn"):
    return t(z[f"{kind}/eeg1"]).to(DEV), t(z[f"{kind}/eeg2"]).to(DEV), t(z["labels"]).to(DEV)


def assert_same_outputs(got, ref):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for k in ref:
        assert not got[k].requires_grad, k
        assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k].detach()), (k, float((got[k] - ref[k].detach()).abs().max()))


def compare_fixture(name, dtype):
    """predict against an eval-mode forward on the fixture's own batch; returns (model, predict's dict, the fixture)"""
    z, kw, cfg, sd, model = build(name, dtype)
    model.eval()
    x1, x2, labels = fixture_inputs(z)
    with torch.no_grad():
        ref = model(x1, x2, labels)
    got = model.predict(x1, x2, labels)
    torch.cuda.synchronize()
    assert_same_outputs(got, ref)
    assert_same_outputs(model.predict(x1, x2), {k: v for k, v in ref.items() if not k.startswith("loss")})       # without labels
    return model, got, z


@pytest.mark.parametrize("name,dtype,lean", [("cfg3_xattn", "bf16", True), ("cfg3_xattn", "fp16", True), ("cfg3_xattn", "f32", False),
                                             ("a5_full", "bf16", None), ("hd64_xattn", "bf16", None)])
def test_predict_equals_the_eval_forward(name, dtype, lean):
    model, _, _ = compare_fixture(name, dtype)
    eng = next(iter(model._infer_engines.values()))
    routes = {(half, how) for _, half, how in eng.routes_taken}
    if lean is True:
        assert routes == {("attn", "lean"), ("ffn", "lean")} and eng.S == 65
    elif lean is False:
        assert routes == {("attn", "scratch"), ("ffn", "scratch")}
    else:                           # S = 115 / 64-wide heads: the attention half has no lean launch; the feed-forward half by its own rule
        assert not eng.attn_block and (name != "hd64_xattn" or eng.head_dim == 64)
        assert routes == {("attn", "scratch"), ("ffn", "lean" if eng.fuse_ffn and eng.ln_fuse else "scratch")}


def test_predict_equals_the_eval_forward_on_the_long_core():
    from tests.test_gpu_long_window import build as build_long, inputs
    model, ocfg, sd = build_long("A5_full_model", 2048, "bf16")
    model.eval()
    x1, x2, labels = (v.to(DEV) for v in inputs(ocfg, 2048))
    with torch.no_grad():
        ref = model(x1, x2, labels)
    got = model.predict(x1, x2, labels)
    eng = next(iter(model._infer_engines.values()))
    assert eng.S == 203 and eng.attn_long
    assert_same_outputs(got, ref)


def test_predict_equals_the_eval_forward_without_the_fused_norms():
    """EYEGAZE_LN_FUSE=0 is read when an engine is made, so the comparison runs in a child process that starts with it set"""
    code = ("from tests.test_gpu_infer_model import compare_fixture\n"
            "model, _, _ = compare_fixture('cfg3_xattn', 'bf16')\n"
            "eng = next(iter(model._infer_engines.values()))\n"
            "assert not eng.ln_fuse and {how for _, _, how in eng.routes_taken} == {'scratch'}, eng.routes_taken\n"
            "print('ln_fuse=0 ok')\n")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(REPO), timeout=300,
                         env={**os.environ, "EYEGAZE_LN_FUSE": "0"})
    assert res.returncode == 0 and "ln_fuse=0 ok" in res.stdout, res.stderr[-3000:]


def test_f32_predict_meets_the_reference_logits():
    """ties the new route to the reference and not only to the project's other route: tests/test_gpu_model.py's f32 gate"""
    _, got, z = compare_fixture("cfg3_xattn", "f32")
    ref = z["randn/out/logits"]
    logits = got["logits"].cpu().numpy()
    err = float(np.abs(logits - ref).max())
    print(f"f32 predict against the reference: max|dlogit| = {err:.3e}")
    assert err <= 4e-6, err
    assert (logits.argmax(-1) == z["randn/out/argmax"]).all()


def train_mode_grads(with_predict):
    torch.manual_seed(1234)                                        # the models' dropout seed base
    z, kw, cfg, sd, model = build("cfg3_xattn", "bf16")
    model.train()
    x1, x2, labels = fixture_inputs(z)
    o1, o2, _ = fixture_inputs(z, "gen_eeg")
    out = model(x1, x2, labels)
    if with_predict:
        eng = next(iter(model._engines.values()))
        count, state = model._fwd_count, eng.state_dev.clone()
        model.predict(o1, o2, labels)
        model.predict(o1[:3], o2[:3])                              # ... and another batch shape
        assert model._fwd_count == count and torch.equal(eng.state_dev, state)
        assert len(model._engines) == 1 and len(model._infer_engines) == 2
    out["loss_ce"].backward()
    torch.cuda.synchronize()
    return [p.grad.clone() for p in model.parameters()], out["logits"].detach().clone()


def test_predict_between_a_forward_and_its_backward_changes_nothing():
    ga, la = train_mode_grads(True)
    gb, lb = train_mode_grads(False)
    assert torch.equal(la, lb)
    assert all(torch.equal(a, b) for a, b in zip(ga, gb)) and any(float(a.abs().max()) > 0 for a in ga)


def test_predict_between_two_training_steps_changes_nothing(tmp_path):
    from eyegaze_multimodal_amd.data import synth_windows
    from eyegaze_multimodal_amd.train_art import Trainer
    from tests.test_gpu_train import make_config
    x1, x2, y = (v.to(DEV) for v in synth_windows(8, 8, 1024, 3, seed=5))
    params = []
    for with_predict in (True, False):
        tr = Trainer(make_config(tmp_path, model={"num_layers": 2}), torch.device(DEV))
        tr.train_step(x1, x2, y)
        if with_predict:
            tr.model.predict(x1[:5], x2[:5], y[:5])
        tr.train_step(x1, x2, y)
        torch.cuda.synchronize()
        params.append(tr.model._flat.flat.clone())
    assert torch.equal(params[0], params[1])


def test_probability_hook_under_predict_and_lean_layers_beside_it():
    z, kw, cfg, sd, model = build("cfg3_xattn", "bf16")
    model.eval()
    x1, x2, labels = fixture_inputs(z)
    seen = {"forward": [], "predict": []}
    key = ["forward"]
    hook = model.encoder.layers[0].mha.dropout.register_forward_hook(lambda mod, inp, out: seen[key[0]].append(inp[0].clone()))
    with torch.no_grad():
        ref = model(x1, x2, labels)
    key[0] = "predict"
    got = model.predict(x1, x2, labels)
    hook.remove()
    assert_same_outputs(got, ref)
    B, H, S = x1.shape[0], cfg.num_heads, 65
    assert len(seen["predict"]) == len(seen["forward"]) == 2 and seen["predict"][0].shape == (B, H, S, S)
    assert all(torch.equal(a, b) for a, b in zip(seen["predict"], seen["forward"]))
    eng = next(iter(model._infer_engines.values()))
    attn = {l: how for l, half, how in eng.routes_taken if half == "attn"}
    assert attn[0] == "scratch" and all(attn[l] == "lean" for l in range(1, cfg.num_layers))


def test_an_inference_engine_refuses_the_training_calls_and_holds_no_gradients():
    z, kw, cfg, sd, model = build("cfg3_xattn", "bf16")
    x1, x2, labels = fixture_inputs(z)
    model.predict(x1, x2, labels)
    fp = model._flat
    assert fp.grad is None and fp.acc is None and not model._engines           # held only through predict: no gradient buffer
    eng = next(iter(model._infer_engines.values()))
    assert isinstance(eng, InferenceEngine) and not eng.g
    assert not any(k.startswith(("qkv", "hff", "r1_", "gbits", "h1")) for k in eng.a)
    m = torch.zeros(1, device=DEV)
    for name, args in (("backward", ()), ("accumulate", (True,)), ("optimizer_step", (m, m))):
        with pytest.raises(L.EgError, match=f"{name}.. on an inference engine"):
            getattr(eng, name)(*args)


def test_predict_windows_equals_three_predict_calls():
    from eyegaze_multimodal_amd.predict import predict_windows
    from eyegaze_multimodal_amd.train_art import macro_metrics
    z, kw, cfg, sd, model = build("cfg3_xattn", "bf16")
    a1, a2, la = fixture_inputs(z)
    b1, b2, _ = fixture_inputs(z, "gen_eeg")
    x1, x2 = torch.cat([a1, b1, a2[:3]]), torch.cat([a2, b2, a1[:3]])          # N = 11
    y = torch.cat([la, la.flip(0), la[:3]])
    assert x1.shape[0] == 11
    res = predict_windows(model, x1.cpu().pin_memory(), x2.cpu().pin_memory(), y.cpu(), batch_size=4)
    outs = [model.predict(x1[i:i + 4], x2[i:i + 4], y[i:i + 4]) for i in (0, 4, 8)]
    logits = torch.cat([o["logits"] for o in outs])
    assert torch.equal(res["logits"], logits)
    pred = logits.argmax(-1)
    assert torch.equal(res["predictions"], pred)
    cm = np.zeros((cfg.num_classes, cfg.num_classes), np.int64)
    np.add.at(cm, (y.cpu().numpy(), pred.cpu().numpy()), 1)
    assert np.array_equal(res["confusion"], cm)
    mean = float(np.mean([float(o["loss_ce"]) for o in outs]))
    assert abs(res["loss"] - mean) <= 1e-6 * abs(mean)
    assert res["metrics"] == macro_metrics(y.cpu().numpy(), pred.cpu().numpy())
    on_device = predict_windows(model, x1, x2, None, batch_size=4)             # device-resident windows, no labels
    assert torch.equal(on_device["logits"], logits) and set(on_device) == {"logits", "predictions"}


def test_trainer_evaluate_on_the_inference_route(tmp_path):
    from eyegaze_multimodal_amd.data import synth_windows
    from eyegaze_multimodal_amd.train_art import Trainer
    from tests.test_gpu_train import make_config
    x1, x2, y = (v.to(DEV) for v in synth_windows(21, 8, 1024, 3, seed=9))
    batches = [(x1[i:i + 8], x2[i:i + 8], y[i:i + 8]) for i in (0, 8, 16)]      # 8 + 8 + 5: the ragged tail included
    evs = []
    for flag in (None, True):
        over = {} if flag is None else {"inference_eval": flag}
        tr = Trainer(make_config(tmp_path, model={"num_layers": 2}, training=over), torch.device(DEV))
        tr.train_step(x1[:8], x2[:8], y[:8])                                   # weights that are no longer the initial ones
        evs.append(tr.evaluate(iter(batches)))
        assert bool(tr.model._infer_engines) == bool(flag)
    plain, infer = evs
    assert set(plain) == set(infer) == {"eval/accuracy", "eval/precision", "eval/recall", "eval/f1", "eval/loss"}
    for k in plain:
        if k == "eval/loss":                                                   # summed on the device in another order
            assert abs(plain[k] - infer[k]) <= 1e-6 * abs(plain[k]), (plain[k], infer[k])
        else:
            assert plain[k] == infer[k], k
