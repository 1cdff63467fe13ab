"""The column-sliced head launches (eg_heads_fwd and eg_heads_bwd_chain: one launch per product, a workgroup per 16 samples x 64
output columns, the class projection / CE / mean in whichever workgroup finishes last) against the separate launches they replace
(Engine.fused_tail = False: eg_gemm_nt, eg_classifier_ce_fwd / _bwd, eg_gemm_tn + eg_reduce_partials, eg_pool_fuse_bwd), which
this file never treats as the code under test.

Slicing the columns changes WHICH workgroup computes an element, not how: every comparison is torch.equal, there is no tolerance.
  * the heads' forward and backward on the engine's own entry-point calls (Engine._heads_fwd / _heads_bwd), every output living in
    a buffer with sentinel words on both sides: zf, hcl, logits, the per-sample losses and their mean; dhcl, dlogits, dzf, dcomb,
    dz; and the WHOLE flat gradient buffer (the six parameter gradients, and nothing else touched).  B = 4 (one partial group of
    16), 20 (a full and a ragged group), 32, 256; 3 and 16 classes; bf16 and fp16; train (p = 0.1) and eval; with and without
    labels; with gradients arriving from outside on the logits and the two CLS rows;
  * each fused launch runs twice on the same buffers: the counters are left at zero and the second result equals the first;
  * one whole engine step at B = 4 and 32: loss, logits and the whole flat gradient buffer."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import DualEEGTransformer  # noqa: E402
from oracle import dual_eeg_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
T = 1024
PAD = 64                                   # sentinel elements on each side of an output (a multiple of 16 bytes in every dtype)
FWD = ("zf", "hcl", "logits", "sloss", "loss")
BWD = ("dhcl", "dlogits", "dzf", "dcomb", "dzA")


def kwargs(nc):
    return dict(in_channels=8, num_classes=nc, max_len=256, use_spectrogram=False, use_ibs=False, use_cross_attention=True)


def build(dtype, B, nc):
    cfg = O.ModelCfg(**kwargs(nc))
    model = DualEEGTransformer(**kwargs(nc), compute_dtype=dtype)
    model.load_state_dict(O.synthetic_state_dict(cfg, seed=7))
    model = model.to(DEV)
    g = torch.Generator().manual_seed(100 * nc + B)
    x1, x2 = torch.randn(B, 8, T, generator=g).to(DEV), torch.randn(B, 8, T, generator=g).to(DEV)
    labels = torch.randint(0, nc, (B,), generator=g).to(DEV)
    ext = dict(glogits=(0.01 * torch.randn(B, nc, generator=g)).to(DEV), gcls1=(0.01 * torch.randn(B, 256, generator=g)).to(DEV),
               gcls2=(0.01 * torch.randn(B, 256, generator=g)).to(DEV))
    return model, model.engine(B, T, DEV), x1, x2, labels, ext


def fence(store, names):
    """moves store[name] into the middle of a larger buffer full of sentinels; returns {name: whole buffer}"""
    whole = {}
    for n in names:
        t = store[n]
        big = torch.full((t.numel() + 2 * PAD,), 1234.5, device=t.device, dtype=t.dtype)
        store[n] = big[PAD:PAD + t.numel()].view(t.shape)
        whole[n] = big
    return whole


def fences_intact(whole):
    for n, big in whole.items():
        edge = torch.cat([big[:PAD], big[-PAD:]])
        assert torch.equal(edge, torch.full_like(edge, 1234.5)), f"a store landed beside {n}"


def heads(model, eng, fused, x1, x2, labels, train, grads, whole):
    """one forward (this route's heads at its end), then the heads' backward alone; with `fused` the head launches run twice"""
    eng.fused_tail = fused
    fp = model._flat
    for n in FWD:
        eng.a[n].fill_(7.0)
    for n in BWD:
        eng.g[n].fill_(7.0)
    fp.grad.fill_(7.0)
    eng.set_state(seed=5, lr=1e-3, step=1)
    eng.forward(x1, x2, labels, train=train)
    assert eng._fused_heads(backward=True) == fused
    p = eng.train_flags[0]
    assert (p == pytest.approx(0.1)) if train else (p == 0.0)
    out = {n: eng.a[n].clone() for n in FWD}
    if fused:                                 # the launch again, on the buffers and counters the first one left
        eng._heads_fwd(eng.z_final, labels, train, p)
        for n in FWD:
            assert torch.equal(out[n], eng.a[n]), f"second launch: {n}"
        assert int(eng.a["heads_ctr"].abs().sum()) == 0
    incoming = dict.fromkeys(("gloss", "gloss_ibs", "glogits", "gcls1", "gcls2", "gibs_logits", "gibs_token"))
    incoming.update(grads)
    for rep in range(2 if fused else 1):
        eng._heads_bwd(eng._bwd_decisions(None), eng._scale_incoming(False, **incoming))
        again = {n: eng.g[n].clone() for n in BWD}
        again["grad"] = fp.grad.clone()
        if rep:
            for n in again:
                assert torch.equal(out[n], again[n]), f"second launch: {n}"
        out.update(again)
    torch.cuda.synchronize()
    fences_intact(whole)
    return out


def compare(f, s, skip=()):
    for n in f:
        if n not in skip:
            assert torch.equal(f[n], s[n]), (n, float((f[n].float() - s[n].float()).abs().max()))
    assert torch.isfinite(f["logits"]).all() and torch.isfinite(f["grad"]).all()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("nc", [3, 16])
@pytest.mark.parametrize("B", [4, 20, 32, 256])
def test_sliced_heads_equal_the_separate_launches(B, nc, dtype):
    model, eng, x1, x2, labels, ext = build(dtype, B, nc)
    eng._alloc_bwd()
    whole = {**fence(eng.a, FWD), **fence(eng.g, BWD)}
    one = torch.ones(1, device=DEV)
    # train mode (p = 0.1), labels, the loss gradient
    f = heads(model, eng, True, x1, x2, labels, True, dict(gloss=one), whole)
    s = heads(model, eng, False, x1, x2, labels, True, dict(gloss=one), whole)
    compare(f, s)
    assert 0.02 < float((f["hcl"] == 0).float().mean()) < 1.0 and float(f["dcomb"].float().abs().max()) > 0
    # train mode, labels, and gradients from outside on the logits and both CLS rows
    kw = dict(gloss=torch.full((1,), 0.5, device=DEV), **ext)
    compare(heads(model, eng, True, x1, x2, labels, True, kw, whole), heads(model, eng, False, x1, x2, labels, True, kw, whole))
    # evaluation mode without labels: logits only (the losses stay untouched), the gradient arrives on the logits
    kw = dict(glogits=ext["glogits"])
    f = heads(model, eng, True, x1, x2, None, False, kw, whole)
    s = heads(model, eng, False, x1, x2, None, False, kw, whole)
    compare(f, s)
    assert torch.equal(f["loss"], torch.full_like(f["loss"], 7.0)) and torch.equal(f["sloss"], torch.full_like(f["sloss"], 7.0))
    # evaluation mode with labels
    compare(heads(model, eng, True, x1, x2, labels, False, dict(gloss=one), whole),
            heads(model, eng, False, x1, x2, labels, False, dict(gloss=one), whole))


@pytest.mark.parametrize("B", [4, 32])
def test_engine_step_on_the_sliced_heads(B):
    """one whole forward + backward on each route: loss, logits and every word of the flat gradient buffer"""
    model, eng, x1, x2, labels, _ = build("bf16", B, 3)
    got = []
    for fused in (True, False):
        eng.fused_tail = fused
        model._flat.grad.fill_(7.0)
        eng.set_state(seed=9, lr=1e-3, step=1)
        eng.forward(x1, x2, labels, train=True)
        eng.backward(gloss=torch.ones(1, device=DEV))
        torch.cuda.synchronize()
        got.append((eng.a["loss"].clone(), eng.a["logits"].clone(), model._flat.grad.clone()))
    for a, b in zip(*got):
        assert torch.equal(a, b)
    assert torch.isfinite(got[0][2]).all() and float(got[0][2].abs().max()) > 0
