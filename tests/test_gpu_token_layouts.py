"""The packed weights of the token families and of the image engine, filled through engine.LAYOUTS: every buffer against a
stand-alone launch of its own entry point on the same fp32 parameter, the inference engine against the eval forward on the scalar
synchrony token, and a plan re-recorded on a live engine.  Every operation involved is a copy or a cast, so every comparison is
bit equality.  Models and shapes are tests/test_token_layouts_host.py's: tiny_full's dims, B = 4, T = 1024."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import DualEEGTransformer  # noqa: E402
from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd.image_encoder import GazeCNNEncoder  # noqa: E402
from tests.test_token_layouts_host import B, FAMILIES, T, TOKEN_KEYS  # noqa: E402

DEV = torch.device("cuda", 0)
OUTPUTS = ("logits", "cls1", "cls2", "ibs_logits", "ibs_pool_f")


def model_of(family, dtype, **kw):
    torch.manual_seed(11)
    return DualEEGTransformer(**{**FAMILIES[family], **kw}, compute_dtype=dtype).to(DEV)


def windows(C):
    g = torch.Generator().manual_seed(5)
    return (torch.randn(B, C, T, generator=g).to(DEV), torch.randn(B, C, T, generator=g).to(DEV),
            torch.tensor([0, 1, 2, 0][:B]).to(DEV))


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def standalone(eng, key, pre):
    """w[key] as its own entry point writes it: one launch on the fp32 parameter into a fresh (zeroed) buffer"""
    d, fp, dt, st = eng.cfg.d_model, eng.fp, eng.dtype, eng._cur_stream()
    E = getattr(eng, "C", 0) ** 2
    src, how, args = {
        "spc2": ("spec_conv.3.weight", "eg_pack_conv2d_weight", (64, 32, 0)),
        "spc2T": ("spec_conv.3.weight", "eg_pack_conv2d_weight", (64, 32, 1)),
        "spp0": ("proj.0.weight", "eg_cast", (2 * d * 1024,)),
        "spp0T": ("proj.0.weight", "eg_transpose_cast", (2 * d, 1024, 2 * d)),
        "spp3": ("proj.3.weight", "eg_cast", (d * 2 * d,)),
        "spp3T": ("proj.3.weight", "eg_transpose_cast", (d, 2 * d, d)),
        "ib0": ("bottleneck.0.weight", "eg_cast", (64 * E,)),
        "ib0T": ("bottleneck.0.weight", "eg_transpose_cast", (64, E, 64)),
        "ib3": ("bottleneck.3.weight", "eg_cast", (d * 64,)),
        "ib3T": ("bottleneck.3.weight", "eg_transpose_cast", (d, 64, d)),
        "ig0": ("0.weight", "eg_pack_conv_weight", (2 * d, 28, 1, 28, 64)),
        "ig3": ("3.weight", "eg_cast", (d * 2 * d,)),
        "ig3T": ("3.weight", "eg_transpose_cast", (d, 2 * d, d)),
    }[key]
    out = torch.zeros_like(eng.w[key])
    L.call(how, fp.p_ptr(pre + src), L.ptr(out), *args, dt, st)
    return out


def check_packed(eng, prefix_of):
    keys = [k for k in TOKEN_KEYS if k in eng.w]
    for k in keys:
        bits(eng.w[k]).fill_(0x7b7b if eng.es == 2 else 0x7b7b7b7b)
    eng.stream = eng._cur_stream()
    eng.pack_params()
    for k in keys:
        want = standalone(eng, k, prefix_of(k))
        torch.cuda.synchronize()
        assert torch.equal(bits(eng.w[k]), bits(want)), k
    return keys


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_packed_token_buffers_equal_their_own_entry_points(family, dtype):
    """among them ig0 through mode 9 of the table (16-bit) against the eg_pack_conv_weight launch it replaces"""
    model = model_of(family, dtype)
    eng = model.engine(B, T, DEV)
    pre = {"sp": "spectrogram_generator.", "ib": "ibs_tokenizer.", "ig": "ibs_generator.proj."}
    keys = check_packed(eng, lambda k: pre[k[:2]])
    assert keys == ([k for k in TOKEN_KEYS if k[:2] in ("sp", "ib")] if family == "spec_robust" else ["ig0", "ig3", "ig3T"])
    assert eng.fused_tail == (dtype == "bf16")


def test_packed_image_engine_buffers_equal_their_own_entry_points():
    torch.manual_seed(12)
    model = GazeCNNEncoder(num_classes=3, d_model=64, compute_dtype="bf16").to(DEV)
    eng = model.engine(B, 64, 16, DEV)
    assert check_packed(eng, lambda k: "cnn.") == ["spc2", "spc2T", "spp0", "spp0T", "spp3", "spp3T"]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_inference_forward_equals_the_eval_forward_on_the_scalar_synchrony_token(dtype):
    model = model_of("scalar", dtype).eval()
    x1, x2, y = windows(model.cfg.in_channels)
    eng, inf = model.engine(B, T, DEV), model.inference_engine(B, T, DEV)
    eng.forward(x1, x2, y, train=False)
    inf.forward(x1, x2, y)
    torch.cuda.synchronize()
    assert "ig3T" in eng.w and "ig3T" not in inf.w
    for k in OUTPUTS:
        assert torch.equal(inf.a[k], eng.a[k]) and bool(torch.isfinite(eng.a[k]).all()), k


# tiny dims: f32, because the synchrony classifier's backward-data product needs d_model / 2 >= the K-tile (32 in f32, 64 in bf16);
# ln_proj is off there and its fragment layout was never allocated, so the flag flipped is pack_unused (see the host test).  The
# ln_proj flip itself runs at the d_model = 256 where the route exists, in bf16.
RERECORD = [("spec_robust", "f32", {}, "pack_unused"), ("scalar", "f32", {}, "pack_unused"),
            ("spec_robust", "bf16", dict(d_model=256, num_heads=8, d_ff=1024), "ln_proj"),
            ("scalar", "bf16", dict(d_model=256, num_heads=8, d_ff=1024), "ln_proj")]


@pytest.mark.parametrize("family,dtype,kw,flag", RERECORD, ids=[f"{f}-{d}-{a}" for f, d, _, a in RERECORD])
def test_rerecording_on_a_live_engine_keeps_the_forward_and_feeds_the_backward(family, dtype, kw, flag):
    model = model_of(family, dtype, **kw).eval()
    x1, x2, y = windows(model.cfg.in_channels)
    eng = model.engine(B, T, DEV)
    eng.forward(x1, x2, y, train=False)
    first = {k: eng.a[k].clone() for k in OUTPUTS}
    plan = eng._plan_dev
    assert getattr(eng, flag) == (flag == "ln_proj")
    setattr(eng, flag, not getattr(eng, flag))
    eng.forward(x1, x2, y, train=False)
    assert eng._plan_dev is not plan
    for k in OUTPUTS:
        assert torch.equal(eng.a[k], first[k]), k
    one = torch.ones(1, device=DEV)
    eng.backward(gloss=one, gloss_ibs=one)
    torch.cuda.synchronize()
    grad = model._flat.grad
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
