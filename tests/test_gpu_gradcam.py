"""GPU tests of the device Grad-CAM route: eg_gradcam_accumulate against float64 from the same input bits,
predict.gradcam_statistics against tests/gradcam_ref.py over the oracle and over the hook route, the analysis backward's bits,
what a walk leaves untouched, predict.embedding_features."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import HipAdamW  # noqa: E402
from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd import predict as P  # noqa: E402
from tests import gradcam_ref as R  # noqa: E402
from tests.helpers import load_golden  # noqa: E402
from tests.test_gpu_model import DEV, build  # noqa: E402

TD = dict(bf16=torch.bfloat16, fp16=torch.float16, f32=torch.float32)
EG = dict(bf16=L.EG_BF16, fp16=L.EG_F16, f32=L.EG_F32)
SENT = 1234.5
# (B, C, Hp, Wp, ncls).  The issue's six shapes; launch 1 splits a sample's channels over 4 quarters (C = 3, 5 beside it) and launch 2
# lists a class's samples in chunks of 1024 (B = 1023, 1025 beside it, tiny images)
SHAPES = [(1, 1, 4, 4, 1), (5, 3, 4, 8, 3), (4, 8, 32, 8, 3), (33, 8, 32, 8, 16), (2, 32, 32, 8, 3), (3, 2, 8, 68, 3),
          (2, 5, 4, 4, 3), (2, 4, 4, 4, 3), (1023, 1, 4, 4, 3), (1024, 1, 4, 4, 3), (1025, 1, 4, 4, 2)]


@functools.lru_cache(maxsize=None)
def _case(B, C, Hp, Wp, ncls, dtype):
    """inputs (CPU, in the compute dtype) and the float64 expectation with its bound, made once per case"""
    g = torch.Generator().manual_seed(B * 1000 + C * 100 + Hp + Wp)
    n = 2 * B * C
    p1 = torch.zeros(n, Hp + 2, Wp + 4, 32)
    p1[:, 1:Hp + 1, 1:Wp + 1] = torch.randn(n, Hp, Wp, 32, generator=g)
    d2 = torch.zeros(n, Hp + 2, Wp + 4, 64)
    gate = (torch.rand(n, Hp, Wp, 64, generator=g) < 0.5).float()                # about half the entries zero, like a ReLU gate
    d2[:, 1:Hp + 1, 1:Wp + 1] = torch.randn(n, Hp, Wp, 64, generator=g) * 1e-4 * gate
    w2, b2 = torch.randn(64, 32, 3, 3, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1
    p1, d2 = p1.to(TD[dtype]), d2.to(TD[dtype])
    labels = torch.arange(B, dtype=torch.int64) % ncls
    if B >= 3:
        labels[1], labels[B - 1] = -1, ncls                                       # counted nowhere
    exp = R.kernel_expectation(p1, d2, w2, b2, labels.numpy(), B, C, Hp, Wp, ncls)
    return p1, d2, w2, b2, labels, exp


def _call(p1, d2, w2, b2, labels, cams, class_sum, class_count, scratch, B, C, Hp, Wp, ncls, dtype, scale=None):
    L.call("eg_gradcam_accumulate", L.ptr(p1), L.ptr(d2), L.ptr(w2), L.ptr(b2), L.ptr(scale), L.ptr(labels), L.ptr(cams),
           L.ptr(class_sum), L.ptr(class_count), L.ptr(scratch), scratch.numel(), B, C, Hp, Wp, ncls, EG[dtype],
           torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "f32"])
@pytest.mark.parametrize("B,C,Hp,Wp,ncls", SHAPES)
def test_kernel_against_float64_from_the_same_bits(B, C, Hp, Wp, ncls, dtype):
    p1, d2, w2, b2, labels, exp = _case(B, C, Hp, Wp, ncls, dtype)
    p1, d2, w2, b2, labels = (t.to(DEV) for t in (p1, d2, w2, b2, labels))
    need = L.gradcam_scratch_elems(B, C, Hp, Wp)
    assert need == 2 * B * Hp * Wp
    # sentinel-guarded outputs: one guard row in front of and behind each; cams holds the rows of two calls
    cams = torch.full((2 * B + 2, 64, 64), SENT, device=DEV)
    csum = torch.full((ncls + 2, 64, 64), SENT, device=DEV)
    csum[1:ncls + 1] = 0
    ccnt = torch.full((ncls + 2,), 77, device=DEV, dtype=torch.int32)
    ccnt[1:ncls + 1] = 0
    scratch = torch.full((need + 64,), float("nan"), device=DEV)
    _call(p1, d2, w2, b2, labels, cams[1:], csum[1:], ccnt[1:], scratch, B, C, Hp, Wp, ncls, dtype)
    first = cams[1:B + 1].clone()
    got = first.double().cpu().numpy()
    err = np.abs(got - exp["cams"])
    print(f"cams: max |err| {err.max():.3e}  max bound {exp['cams_bound'].max():.3e}  max err/bound "
          f"{(err / np.maximum(exp['cams_bound'], 1e-300)).max():.3f}  max value {exp['cams'].max():.3e}")
    assert np.isfinite(got).all() and exp["cams"].max() > 0 and (err <= exp["cams_bound"]).all()
    s1 = csum[1:ncls + 1].double().cpu().numpy()
    assert (np.abs(s1 - exp["class_sum"]) <= exp["class_bound"]).all()
    assert ccnt[1:ncls + 1].cpu().tolist() == exp["class_count"].tolist() and int(exp["class_count"].sum()) == B - (2 if B >= 3 else 0)
    assert (scratch[need:] != scratch[need:]).all()                              # nothing written past the query's size
    # the second call: scratch holds 3e38, its own cams rows, adds into class_sum and the counts
    scratch.fill_(3e38)
    _call(p1, d2, w2, b2, labels, cams[B + 1:], csum[1:], ccnt[1:], scratch, B, C, Hp, Wp, ncls, dtype)
    assert torch.equal(cams[1:B + 1], first) and torch.equal(cams[B + 1:2 * B + 1], first)     # same bits whatever the scratch held
    s2 = csum[1:ncls + 1].double().cpu().numpy()
    assert (np.abs(s2 - 2 * exp["class_sum"]) <= 2 * exp["class_bound"] + 2 * R.U * 2 * exp["class_sum"]).all()
    assert ccnt[1:ncls + 1].cpu().tolist() == (2 * exp["class_count"]).tolist()
    assert (cams[0] == SENT).all() and (cams[-1] == SENT).all() and (csum[0] == SENT).all() and (csum[-1] == SENT).all()
    assert ccnt[0].item() == 77 and ccnt[-1].item() == 77
    # the loss scale: d2 * 1024 with grad_scale = 1024 gives the unscaled call's maps within the same bound
    scale = torch.full((1,), 1024.0, device=DEV)
    cams3 = torch.empty(B, 64, 64, device=DEV)
    _call(p1, (d2.float() * 1024).to(TD[dtype]), w2, b2, labels, cams3, csum[1:], ccnt[1:], scratch, B, C, Hp, Wp, ncls, dtype, scale)
    err3 = np.abs(cams3.double().cpu().numpy() - exp["cams"])
    print(f"scaled: max |err| {err3.max():.3e}")
    assert (err3 <= exp["cams_bound"]).all()


# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(name, n, target, max_samples=100):
    z, kw, cfg, sd = load_golden(name)
    x1, x2, y = R.windows(z)
    return R.gradcam_ref(R.oracle_runner(sd, cfg), x1[:n], x2[:n], y[:n], 4, max_samples=max_samples, target=target)


def _windows(name, n):
    x1, x2, y = R.windows(load_golden(name)[0])
    return x1[:n].to(DEV), x2[:n].to(DEV), y[:n].to(DEV)


def _check_f32(st, ref):
    scale = max(m.max() for m in ref["class_mean"].values())
    assert scale > 1e-5
    assert st["count"] == ref["count"] and st["class_count"] == ref["class_count"]
    assert (st["predictions"].cpu().numpy() == ref["predictions"]).all()
    e = np.abs(st["cams"].cpu().numpy() - ref["cams"]).max()
    print(f"cams: max |err| {e:.3e} = {e / ref['cams'].max():.2e} of the maps' maximum {ref['cams'].max():.3e}")
    assert e <= 4e-3 * ref["cams"].max()
    for n, m in ref["class_mean"].items():
        e = np.abs(st["class_mean"][n] - m).max()
        print(f"{n}: max |err| {e:.3e} = {e / scale:.2e} of {scale:.3e}")
        assert st["class_mean"][n].shape == (64, 64) and st["class_mean"][n].dtype == np.float32 and e <= 4e-3 * scale


@pytest.mark.parametrize("target", ["predicted", "label"])
def test_model_f32_two_engine_shapes_and_the_ragged_tail(target):
    z, kw, cfg, sd, model = build("cfg5_a2_spec", "f32")
    x1, x2, y = _windows("cfg5_a2_spec", 10)
    st = P.gradcam_statistics(model, x1, x2, y, batch_size=4, target=target)
    ref = _oracle("cfg5_a2_spec", 10, target)
    assert st["cams"].shape == (10, 64, 64) and st["cams"].is_cuda and st["logits"].shape == (10, 3)
    assert list(st["class_mean"]) == R.NAMES and len(model._engines) == 2
    _check_f32(st, ref)
    if target == "label":       # every logit column is driven: the three classes' maps differ from the predicted-class ones
        other = _oracle("cfg5_a2_spec", 10, "predicted")
        assert np.abs(ref["cams"] - other["cams"]).max() > 0.1 * ref["cams"].max()
    else:
        st5 = P.gradcam_statistics(model, x1, x2, y, batch_size=4, max_samples=5)
        assert st5["count"] == 8 and sum(st5["class_count"].values()) == 8 and st5["cams"].shape[0] == 8
        assert torch.equal(st5["cams"], st["cams"][:8])
        # a class that never occurs gets zeros; names beyond the labels too
        st4 = P.gradcam_statistics(model, x1[:4], x2[:4], torch.zeros(4, dtype=torch.int64), batch_size=4,
                                   class_names=["a", "b", "c", "d"])
        assert st4["class_count"] == {"a": 4, "b": 0, "c": 0, "d": 0} and not st4["class_mean"]["d"].any() and st4["class_mean"]["a"].any()


def test_model_f32_with_synchrony_tokens():
    """a5_full: the synchrony tokens shift the spectrogram rows, and their backward is skipped"""
    z, kw, cfg, sd, model = build("a5_full", "f32")
    x1, x2, y = _windows("a5_full", 4)
    st = P.gradcam_statistics(model, x1, x2, y, batch_size=4)
    _check_f32(st, _oracle("a5_full", 4, "predicted"))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_model_16_bit_against_the_oracle(dtype):
    """the project's gate for 16-bit gradients through six layers (tests/test_gpu_hooks.py): direction and scale per class map"""
    z, kw, cfg, sd, model = build("cfg5_a2_spec", dtype)
    x1, x2, y = _windows("cfg5_a2_spec", 10)
    st = P.gradcam_statistics(model, x1, x2, y, batch_size=4)
    ref = _oracle("cfg5_a2_spec", 10, "predicted")
    assert st["class_count"] == ref["class_count"]
    for n, m in ref["class_mean"].items():
        g = st["class_mean"][n]
        cos = float(np.corrcoef(g.ravel(), m.ravel())[0, 1])
        ratio = float(np.linalg.norm(g) / np.linalg.norm(m))
        print(f"{dtype} {n}: correlation {cos:.4f} norm ratio {ratio:.4f}")
        assert np.isfinite(g).all() and cos > 0.8 and 0.7 < ratio < 1.4
    if dtype == "fp16":         # the scaler is never updated
        eng = next(iter(model._engines.values()))
        s0 = eng.read_state()
        P.gradcam_statistics(model, x1, x2, y, batch_size=4)
        s1 = eng.read_state()
        assert eng.scaler_on and s0.loss_scale == s1.loss_scale == 65536.0 and s1.good_steps == s0.good_steps and s1.found_inf == 0


HOOK_ROUTE_GATE = 2 * 1.66e-3       # twice the 1.653e-3 measured on an MI355X, of the maps' maximum


def test_model_bf16_against_the_hook_route():
    """The reference's algorithm through the hook route of the same HIP model on the same windows: both read the same sp_d2 bits;
    they differ in the rounding of the pre-ReLU activation (bf16 in the hook route, never stored here) and of the weights."""
    z, kw, cfg, sd, model = build("cfg5_a2_spec", "bf16")
    x1, x2, y = _windows("cfg5_a2_spec", 10)
    ref = R.gradcam_ref(R.hook_runner(model), x1, x2, y, 4)
    st = P.gradcam_statistics(model, x1, x2, y, batch_size=4)
    assert all(p.requires_grad for p in model.parameters())
    assert (st["predictions"].cpu().numpy() == ref["predictions"]).all() and st["class_count"] == ref["class_count"]
    top = ref["cams"].max()
    e = np.abs(st["cams"].cpu().numpy() - ref["cams"]).max() / top
    em = max(np.abs(st["class_mean"][n] - m).max() for n, m in ref["class_mean"].items()) / top
    print(f"device route vs hook route (bf16): cams {e:.3e}, class means {em:.3e} of the maps' maximum {top:.3e}")
    assert e <= HOOK_ROUTE_GATE and em <= HOOK_ROUTE_GATE


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_analysis_backward_leaves_the_full_backward_s_bits(dtype):
    z, kw, cfg, sd, model = build("cfg5_a2_spec", dtype)
    x1, x2, y = _windows("cfg5_a2_spec", 4)
    eng = model.engine(4, 1024, x1.device)
    one_hot = torch.nn.functional.one_hot(y, 3).float()
    eng.forward(x1, x2, None, train=False)
    eng.backward(glogits=one_hot)
    full = eng.g["sp_d2"].clone()
    eng.g["sp_d2"].zero_()
    eng.forward(x1, x2, None, train=False)
    eng.backward(glogits=one_hot, until="spec_conv2")
    assert full.float().abs().max() > 0 and torch.equal(eng.g["sp_d2"], full)


def test_a_walk_leaves_the_training_state_alone():
    z, kw, cfg, sd, model = build("cfg5_a2_spec", "bf16")
    x1, x2, y = _windows("cfg5_a2_spec", 10)
    eng = model.engine(4, 1024, x1.device)
    opt = HipAdamW(model, lr=1e-4, weight_decay=0.01)
    opt.begin_step(eng, seed=1)
    eng.forward(x1[:4], x2[:4], y[:4], train=True)
    eng.backward(gloss=torch.ones(1, device=DEV))
    opt.step(eng)
    model.eval()
    held = model(x1[:4], x2[:4], y[:4])                       # an autograd forward made BEFORE the walk
    before = dict(flat=model._flat.flat.clone(), state=eng.state_dev.clone(), m=opt.m.clone(), v=opt.v.clone(),
                  logits=model.predict(x1, x2)["logits"].clone())
    a = P.gradcam_statistics(model, x1, x2, y, batch_size=4)
    b = P.gradcam_statistics(model, x1, x2, y, batch_size=4)
    assert torch.equal(a["cams"], b["cams"]) and torch.equal(a["logits"], b["logits"])
    assert all(np.array_equal(a["class_mean"][n], b["class_mean"][n]) for n in R.NAMES) and a["class_count"] == b["class_count"]
    assert torch.equal(model._flat.flat, before["flat"]) and torch.equal(eng.state_dev, before["state"])
    assert torch.equal(opt.m, before["m"]) and torch.equal(opt.v, before["v"])
    assert torch.equal(model.predict(x1, x2)["logits"], before["logits"])
    assert all(p.grad is None for p in model.parameters())
    with pytest.raises(RuntimeError, match="newer forward"):
        held["loss"].backward()


@pytest.mark.parametrize("name", ["cfg5_a2_spec", "a5_full"])
def test_embedding_features_are_predict_s_bits(name):
    z, kw, cfg, sd, model = build(name, "bf16")
    x1, x2, y = _windows(name, 10)
    out = P.embedding_features(model, x1.cpu(), x2.cpu(), y.cpu(), batch_size=4)
    keys = {"z_fuse", "cls1", "cls2", "y_true", "y_pred"} | ({"ibs_token"} if cfg.use_ibs else set())
    assert set(out) == keys and out["z_fuse"].shape == (10, 3 * cfg.d_model)
    for i in range(0, 10, 4):
        ref = model.predict(x1[i:i + 4], x2[i:i + 4])
        for k in keys - {"z_fuse", "y_true", "y_pred"}:
            assert np.array_equal(out[k][i:i + 4], ref[k].cpu().numpy()), k
        assert (out["y_pred"][i:i + 4] == ref["logits"].argmax(1).cpu().numpy()).all()
    c1, c2 = out["cls1"], out["cls2"]
    assert np.array_equal(out["z_fuse"], np.concatenate([c1, c2, np.abs(c1 - c2)], axis=1))
    assert out["y_true"].tolist() == R.LABELS and out["y_pred"].dtype == np.int64
