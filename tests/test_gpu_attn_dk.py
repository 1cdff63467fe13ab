"""The attention core with the head width as an argument (csrc/attention_long.hip: eg_attention_dk_fwd / _bwd / _probs).
  * head_dim 64 against fp64 torch (its own reference: tests/test_gpu_ops._attn_ref is 32 wide), forward, lse and backward, at a
    single key, a partial last tile, exact tile edges (64, 128 + 1, 512) and many tiles (2048), kv_shift 0 and NB / 2.
    Gates: those of tests/test_gpu_attn_long.py for the same dtype (16-bit: ctx 2e-2, gradient max error 3e-2 * max(1, scale),
    Frobenius 2e-2; lse 1e-4; f32: ctx 1e-5 / 2e-6, gradients 1e-4 / 1e-5).  Randn inputs give unit-variance scaled scores at either
    width, so they carry over.
  * head_dim 32 through these entry points is eg_attention_long_* bit for bit, dropout on.
  * dropout at width 64: forward and backward against fp64 autograd through the mask replayed on the CPU (the element index does
    not depend on the head width), keep rate, and a backward that gives the same bits twice.
  * the probabilities kernel."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from tests.dropout64 import attn_element_index  # noqa: E402
from tests.test_gpu_ops import DEV, DT, dev_state  # noqa: E402

ALL_DT = [L.EG_BF16, L.EG_F16, L.EG_F32]
BITS = {L.EG_BF16: torch.int16, L.EG_F16: torch.int16, L.EG_F32: torch.int32}


def inputs(NB, S, H, hd, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    D = H * hd
    qkv = torch.randn(NB * S, 3 * D, generator=g).to(DT[dtype])
    dO = torch.randn(NB * S, D, generator=g).to(DT[dtype])
    return qkv, dO


def attn_ref(qkv, NB, S, H, hd, kv_shift):
    """fp64: context rows [NB*S, H*hd] and lse [NB, H, S]"""
    x = qkv.double().reshape(NB, S, 3, H, hd)
    idx = (torch.arange(NB) + kv_shift) % NB
    q = x[:, :, 0].permute(0, 2, 1, 3)
    k = x[idx][:, :, 1].permute(0, 2, 1, 3)
    v = x[idx][:, :, 2].permute(0, 2, 1, 3)
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    o = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(NB * S, H * hd)
    return o, torch.logsumexp(s, -1)


def dk_fwd(qkvd, NB, S, H, hd, kv_shift, dtype, p=0.0, site=0, st=None, fn="eg_attention_dk_fwd"):
    ctx = torch.zeros(NB * S, H * hd, device=DEV, dtype=DT[dtype])
    lse = torch.zeros(NB, H, S, device=DEV)
    heads = (H, hd) if "_dk_" in fn else (H,)
    call(fn, ptr(qkvd), ptr(ctx), ptr(lse), NB, S, *heads, kv_shift, dtype, p, site, ptr(st), 0)
    return ctx, lse


def dk_bwd(qkvd, ctx, dOd, lse, NB, S, H, hd, kv_shift, dtype, p=0.0, site=0, st=None, fn="eg_attention_dk_bwd"):
    dqkv = torch.zeros_like(qkvd)
    scratch = torch.zeros(NB * H * S, device=DEV)
    heads = (H, hd) if "_dk_" in fn else (H,)
    call(fn, ptr(qkvd), ptr(ctx), ptr(dOd), ptr(lse), ptr(dqkv), NB, S, *heads, kv_shift, dtype, p, site, ptr(st),
         ptr(scratch), scratch.numel(), 0)
    return dqkv


@pytest.mark.parametrize("dtype", ALL_DT)
@pytest.mark.parametrize("half_shift", [False, True])
@pytest.mark.parametrize("S", [1, 16, 63, 64, 65, 115, 129, 161, 257, 512, 2048])
def test_width_64_against_fp64(S, half_shift, dtype):
    hd = 64
    NB, H = (4, 2) if S <= 512 else (2, 1)
    kv_shift = NB // 2 if half_shift else 0
    qkv, dO = inputs(NB, S, H, hd, dtype, seed=S + 7 * dtype)
    qkvd, dOd = qkv.to(DEV), dO.to(DEV)
    ctx, lse = dk_fwd(qkvd, NB, S, H, hd, kv_shift, dtype)
    dqkv = dk_bwd(qkvd, ctx, dOd, lse, NB, S, H, hd, kv_shift, dtype)
    torch.cuda.synchronize()
    qr = qkv.double().requires_grad_(True)
    o_ref, lse_ref = attn_ref(qr, NB, S, H, hd, kv_shift)
    o_ref.backward(dO.double())
    got, ref = dqkv.cpu().double(), qr.grad
    c_err = (ctx.cpu().double() - o_ref.detach()).abs().max().item()
    g_err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    print(f"hd64 S={S} shift={kv_shift} dtype={dtype}: ctx {c_err:.3e} lse {(lse.cpu().double() - lse_ref.detach()).abs().max().item():.3e} "
          f"grad max {g_err:.3e} (scale {scale:.3e}) fro {((got - ref).norm() / ref.norm()).item():.3e}")
    torch.testing.assert_close(lse.cpu().double(), lse_ref.detach(), rtol=1e-4, atol=1e-4)
    if dtype == L.EG_F32:
        torch.testing.assert_close(ctx.cpu().double(), o_ref.detach(), rtol=1e-5, atol=2e-6)
        torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-5)
    else:
        torch.testing.assert_close(ctx.cpu().double(), o_ref.detach(), rtol=2e-2, atol=2e-2)
        assert g_err < 3e-2 * max(1.0, scale), (g_err, scale)
        assert ((got - ref).norm() / ref.norm()).item() < 2e-2


@pytest.mark.parametrize("dtype", ALL_DT)
@pytest.mark.parametrize("S", [65, 203])
def test_width_32_is_the_long_core_bit_for_bit(S, dtype):
    NB, H, hd, kv_shift, p, site = 4, 2, 32, 1, 0.25, 19
    st = dev_state(seed=0xD1CE + S)
    qkv, dO = inputs(NB, S, H, hd, dtype, seed=300 + S)
    qkvd, dOd = qkv.to(DEV), dO.to(DEV)
    c_a, l_a = dk_fwd(qkvd, NB, S, H, hd, kv_shift, dtype, p, site, st)
    g_a = dk_bwd(qkvd, c_a, dOd, l_a, NB, S, H, hd, kv_shift, dtype, p, site, st)
    c_b, l_b = dk_fwd(qkvd, NB, S, H, hd, kv_shift, dtype, p, site, st, fn="eg_attention_long_fwd")
    g_b = dk_bwd(qkvd, c_b, dOd, l_b, NB, S, H, hd, kv_shift, dtype, p, site, st, fn="eg_attention_long_bwd")
    torch.cuda.synchronize()
    assert float(c_a.float().abs().sum()) > 0 and float(g_a.float().abs().sum()) > 0
    assert torch.equal(c_a.view(BITS[dtype]), c_b.view(BITS[dtype]))
    assert torch.equal(l_a.view(torch.int32), l_b.view(torch.int32))
    assert torch.equal(g_a.view(BITS[dtype]), g_b.view(BITS[dtype]))


def masked_ref(qkv, dO, w, NB, S, H, hd, kv_shift, keep, p):
    """query window w through fp64 autograd with the keep mask [H, S, S]; returns ctx rows of w, and the gradient of ALL rows
    that this window's loss produces (dQ in window w, dK / dV in window (w + kv_shift) % NB)"""
    x = qkv.double().view(NB, S, 3, H, hd).clone().requires_grad_(True)
    wk = (w + kv_shift) % NB
    q, k, v = x[w, :, 0].permute(1, 0, 2), x[wk, :, 1].permute(1, 0, 2), x[wk, :, 2].permute(1, 0, 2)
    P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), -1)
    o = ((P * keep / (1 - p)) @ v).permute(1, 0, 2).reshape(S, H * hd)
    o.backward(dO[w * S:(w + 1) * S].double())
    return o.detach(), x.grad.reshape(NB * S, 3 * H * hd)


@pytest.mark.parametrize("dtype", ALL_DT)
def test_width_64_dropout_replayed_on_the_cpu(dtype):
    from eyegaze_multimodal_amd.engine import scramble_seed
    from tests.helpers import hip_keep_mask
    NB, H, hd, S, p, site, kv_shift, seed = 4, 2, 64, 139, 0.25, 29, 2, 0xFACADE
    st = dev_state(seed=scramble_seed(seed))      # the words Engine.set_state publishes, which the CPU helper replays
    qkv, dO = inputs(NB, S, H, hd, dtype, seed=41 + dtype)
    qkvd, dOd = qkv.to(DEV), dO.to(DEV)
    ctx, lse = dk_fwd(qkvd, NB, S, H, hd, kv_shift, dtype, p, site, st)
    dqkv = dk_bwd(qkvd, ctx, dOd, lse, NB, S, H, hd, kv_shift, dtype, p, site, st)
    again = dk_bwd(qkvd, ctx, dOd, lse, NB, S, H, hd, kv_shift, dtype, p, site, st)
    torch.cuda.synchronize()
    assert torch.equal(dqkv.view(BITS[dtype]), again.view(BITS[dtype]))
    o_ref, g_ref, rate = [], torch.zeros(NB * S, 3 * H * hd, dtype=torch.float64), []
    for w in range(NB):
        keep = torch.from_numpy(hip_keep_mask(seed, site, attn_element_index(w, H, S).astype(np.uint32), p))
        rate.append(keep.float().mean().item())
        o, g = masked_ref(qkv, dO, w, NB, S, H, hd, kv_shift, keep, p)
        o_ref.append(o)
        g_ref += g
    assert all(0.6 < r < 0.9 for r in rate), rate
    o_ref = torch.cat(o_ref)
    got_o, got_g = ctx.cpu().double(), dqkv.cpu().double()
    print(f"hd64 dropout dtype={dtype}: ctx {(got_o - o_ref).abs().max().item():.3e} grad max {(got_g - g_ref).abs().max().item():.3e} "
          f"fro {((got_g - g_ref).norm() / g_ref.norm()).item():.3e} keep {np.mean(rate):.3f}")
    if dtype == L.EG_F32:
        torch.testing.assert_close(got_o, o_ref, rtol=1e-5, atol=2e-6)
        torch.testing.assert_close(got_g, g_ref, rtol=1e-4, atol=1e-5)
    else:
        torch.testing.assert_close(got_o, o_ref, rtol=2e-2, atol=2e-2)
        err, scale = (got_g - g_ref).abs().max().item(), g_ref.abs().max().item()
        assert err < 3e-2 * max(1.0, scale), (err, scale)
        assert ((got_g - g_ref).norm() / g_ref.norm()).item() < 2e-2


@pytest.mark.parametrize("dtype", [L.EG_BF16, L.EG_F32])
@pytest.mark.parametrize("S", [65, 203])
def test_width_64_probabilities_kernel(S, dtype):
    NB, H, hd, kv_shift = 2, 2, 64, 1
    qkv, _ = inputs(NB, S, H, hd, dtype, seed=S)
    qkvd = qkv.to(DEV)
    _, lse = dk_fwd(qkvd, NB, S, H, hd, kv_shift, dtype)
    probs = torch.full((NB, H, S, S), float("nan"), device=DEV)
    call("eg_attention_dk_probs", ptr(qkvd), ptr(lse), ptr(probs), NB, S, H, hd, kv_shift, dtype, 0)
    torch.cuda.synchronize()
    x = qkv.double().view(NB, S, 3, H, hd)
    idx = (torch.arange(NB) + kv_shift) % NB
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[idx][:, :, 1].permute(0, 2, 1, 3)
    ref = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), -1)
    got = probs.cpu().double()
    torch.testing.assert_close(got, ref, rtol=1e-3, atol=1e-6)
    assert (got.sum(-1) - 1).abs().max().item() < 1e-3
