"""Long-sequence attention core (csrc/attention_long.hip: eg_attention_long_fwd / _bwd / _probs) against fp64 torch, against
the short kernels (eg_attention_fwd / _bwd) where both run, and at element indices past 2^32.  Gates are those of
tests/test_gpu_ops.py for the same dtype (test_attention_fwd_bwd, test_attention_f32_exact); lse at 1e-4."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from tests.dropout64 import attn_element_index, hip_keep_mask64  # noqa: E402
from tests.test_gpu_ops import DEV, DT, _attn_ref, dev_state  # noqa: E402

LONG_S = [161, 203, 257, 333, 512, 1024, 2048]
ALL_DT = [L.EG_BF16, L.EG_F16, L.EG_F32]


def _inputs(NB, S, H, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    D = H * 32
    qkv = torch.randn(NB * S, 3 * D, generator=g).to(DT[dtype])
    dO = torch.randn(NB * S, D, generator=g).to(DT[dtype])
    return qkv, dO


def long_fwd(qkvd, NB, S, H, kv_shift, dtype, p=0.0, site=0, st=None):
    D = H * 32
    ctx = torch.zeros(NB * S, D, device=DEV, dtype=DT[dtype])
    lse = torch.zeros(NB, H, S, device=DEV)
    call("eg_attention_long_fwd", ptr(qkvd), ptr(ctx), ptr(lse), NB, S, H, kv_shift, dtype, p, site, ptr(st), 0)
    return ctx, lse


def long_bwd(qkvd, ctx, dOd, lse, NB, S, H, kv_shift, dtype, p=0.0, site=0, st=None):
    dqkv = torch.zeros_like(qkvd)
    scratch = torch.zeros(NB * H * S, device=DEV)
    call("eg_attention_long_bwd", ptr(qkvd), ptr(ctx), ptr(dOd), ptr(lse), ptr(dqkv), NB, S, H, kv_shift, dtype, p, site, ptr(st),
         ptr(scratch), scratch.numel(), 0)
    return dqkv


def short_fwd_bwd(qkvd, dOd, NB, S, H, kv_shift, dtype, p=0.0, site=0, st=None):
    D = H * 32
    ctx = torch.zeros(NB * S, D, device=DEV, dtype=DT[dtype])
    lse = torch.zeros(NB, H, S, device=DEV)
    call("eg_attention_fwd", ptr(qkvd), ptr(ctx), ptr(lse), NB, S, H, kv_shift, dtype, p, site, ptr(st), 0)
    dqkv = torch.zeros_like(qkvd)
    call("eg_attention_bwd", ptr(qkvd), ptr(ctx), ptr(dOd), ptr(lse), ptr(dqkv), NB, S, H, kv_shift, dtype, p, site, ptr(st), 0)
    return ctx, lse, dqkv


@pytest.mark.parametrize("dtype", ALL_DT)
@pytest.mark.parametrize("half_shift", [False, True])
@pytest.mark.parametrize("S", LONG_S)
def test_long_attention_against_fp64(S, half_shift, dtype):
    NB, H = (4, 2) if S <= 512 else (2, 2)
    kv_shift = NB // 2 if half_shift else 0
    qkv, dO = _inputs(NB, S, H, dtype, seed=S + 7 * dtype)
    qkvd, dOd = qkv.to(DEV), dO.to(DEV)
    ctx, lse = long_fwd(qkvd, NB, S, H, kv_shift, dtype)
    dqkv = long_bwd(qkvd, ctx, dOd, lse, NB, S, H, kv_shift, dtype)
    torch.cuda.synchronize()
    qr = qkv.double().requires_grad_(True)
    o_ref, lse_ref = _attn_ref(qr, NB, S, H, kv_shift)
    o_ref.backward(dO.double())
    torch.testing.assert_close(lse.cpu().double(), lse_ref.detach(), rtol=1e-4, atol=1e-4)
    got, ref = dqkv.cpu().double(), qr.grad
    if dtype == L.EG_F32:
        torch.testing.assert_close(ctx.cpu().double(), o_ref.detach(), rtol=1e-5, atol=2e-6)
        torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-5)
    else:
        torch.testing.assert_close(ctx.cpu().double(), o_ref.detach(), rtol=2e-2, atol=2e-2)
        err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
        assert err < 3e-2 * max(1.0, scale), (err, scale)
        assert ((got - ref).norm() / ref.norm()).item() < 2e-2


@pytest.mark.parametrize("dtype", ALL_DT)
@pytest.mark.parametrize("S", [16, 65, 139, 160])
def test_long_agrees_with_short_kernels_and_draws_the_same_masks(S, dtype):
    """Where both cores run: identical dropout masks (read off the forward with one-hot V rows: ctx[q, j] = P_dropped[q, 32 r + j]),
    and outputs / gradients that agree to 16-bit rounding (fp32: the fp32 gate)."""
    NB, H, kv_shift, p, site = 4, 2, 2, 0.25, 23
    st = dev_state(seed=0x5EED + S)
    qkv, dO = _inputs(NB, S, H, dtype, seed=100 + S)
    qkvd, dOd = qkv.to(DEV), dO.to(DEV)
    c_l, l_l = long_fwd(qkvd, NB, S, H, kv_shift, dtype, p, site, st)
    g_l = long_bwd(qkvd, c_l, dOd, l_l, NB, S, H, kv_shift, dtype, p, site, st)
    c_s, l_s, g_s = short_fwd_bwd(qkvd, dOd, NB, S, H, kv_shift, dtype, p, site, st)
    torch.cuda.synchronize()
    if dtype == L.EG_F32:
        torch.testing.assert_close(c_l, c_s, rtol=1e-5, atol=2e-6)
        torch.testing.assert_close(l_l, l_s, rtol=1e-6, atol=2e-6)
        torch.testing.assert_close(g_l, g_s, rtol=1e-4, atol=1e-5)
    else:
        torch.testing.assert_close(c_l.float(), c_s.float(), rtol=2e-2, atol=1e-2)
        torch.testing.assert_close(l_l, l_s, rtol=1e-4, atol=1e-4)
        a, b = g_l.double().cpu(), g_s.double().cpu()
        assert ((a - b).norm() / b.norm()).item() < 1e-2
    # masks: one-hot V rows expose 32 keys per forward
    D = H * 32
    for r in range((S + 31) // 32):
        x = qkv.clone().view(NB, S, 3, H, 32)
        x[:, :, 2] = 0
        for j in range(32):
            if 32 * r + j < S:
                x[:, 32 * r + j, 2, :, j] = 1
        xd = x.view(NB * S, 3 * D).to(DEV)
        pl, _ = long_fwd(xd, NB, S, H, kv_shift, dtype, p, site, st)
        ps, _, _ = short_fwd_bwd(xd, dOd, NB, S, H, kv_shift, dtype, p, site, st)
        torch.cuda.synchronize()
        ncol = min(32, S - 32 * r)
        ml = (pl.view(NB, S, H, 32)[..., :ncol] != 0).cpu()
        ms = (ps.view(NB, S, H, 32)[..., :ncol] != 0).cpu()
        assert torch.equal(ml, ms), (r, int((ml != ms).sum()))
        assert 0.6 < ml.float().mean().item() < 0.9


def _masked_ref(qkv, dO, w, S, H, keep, p):
    D = H * 32
    rows = slice(w * S, (w + 1) * S)
    x = qkv[rows].double().view(S, 3, H, 32).requires_grad_(True)
    q, k, v = (x[:, i].permute(1, 0, 2) for i in range(3))
    P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(32), -1)
    o = ((P * keep / (1 - p)) @ v).permute(1, 0, 2).reshape(S, D)
    o.backward(dO[rows].double())
    return o.detach(), x.grad.reshape(S, 3 * D)


def test_dropout_past_2_to_the_32_matches_the_64_bit_mask():
    """H = 8, S = 2048 and NB = 264 windows: window 128 holds element indices in [2^32, 2^33) (where a 32-bit index wraps) and
    window 263 indices past 2^33 (the pair index's high word is non-zero).  (NB = 128 ends at exactly 2^32 - 1.)  Forward and
    backward of those windows against fp64 autograd through the 64-bit-index mask reproduced on the CPU (tests/dropout64.py)."""
    NB, H, S, p, site, seed = 264, 8, 2048, 0.25, 31, 0xABCDEF
    D = H * 32
    from eyegaze_multimodal_amd.engine import scramble_seed
    st = dev_state(seed=scramble_seed(seed))      # the words Engine.set_state publishes, which the CPU helper replays
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(NB * S, 3 * D, generator=g).to(torch.bfloat16)
    dO = torch.randn(NB * S, D, generator=g).to(torch.bfloat16)
    qkvd, dOd = qkv.to(DEV), dO.to(DEV)
    ctx, lse = long_fwd(qkvd, NB, S, H, 0, L.EG_BF16, p, site, st)
    dqkv = long_bwd(qkvd, ctx, dOd, lse, NB, S, H, 0, L.EG_BF16, p, site, st)
    torch.cuda.synchronize()
    from tests.helpers import hip_keep_mask
    for w, lo in ((128, 1 << 32), (NB - 1, 1 << 33)):
        idx = attn_element_index(w, H, S)
        assert int(idx.min()) >= lo
        keep = torch.from_numpy(hip_keep_mask64(seed, site, idx, p))
        # the wrapped 32-bit index draws a different mask: the checks below can tell them apart
        assert (hip_keep_mask(seed, site, idx.astype(np.uint32), p) != keep.numpy()).mean() > 0.2
        o, gref = _masked_ref(qkv, dO, w, S, H, keep, p)
        rows = slice(w * S, (w + 1) * S)
        torch.testing.assert_close(ctx[rows].cpu().double(), o, rtol=2e-2, atol=2e-2)
        got = dqkv[rows].cpu().double()
        assert ((got - gref).norm() / gref.norm()).item() < 2e-2, w


def test_backward_is_deterministic():
    NB, H, S, p = 4, 4, 1024, 0.1
    st = dev_state(seed=77)
    for dtype in ALL_DT:
        qkv, dO = _inputs(NB, S, H, dtype, seed=3)
        qkvd, dOd = qkv.to(DEV), dO.to(DEV)
        ctx, lse = long_fwd(qkvd, NB, S, H, 1, dtype, p, 5, st)
        a = long_bwd(qkvd, ctx, dOd, lse, NB, S, H, 1, dtype, p, 5, st)
        b = long_bwd(qkvd, ctx, dOd, lse, NB, S, H, 1, dtype, p, 5, st)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int16 if dtype != L.EG_F32 else torch.int32),
                           b.view(torch.int16 if dtype != L.EG_F32 else torch.int32)), dtype


@pytest.mark.parametrize("dtype", [L.EG_BF16, L.EG_F32])
@pytest.mark.parametrize("S", [203, 1024])
def test_probabilities_kernel(S, dtype):
    NB, H, kv_shift = 2, 2, 1
    qkv, _ = _inputs(NB, S, H, dtype, seed=S)
    qkvd = qkv.to(DEV)
    _, lse = long_fwd(qkvd, NB, S, H, kv_shift, dtype)
    probs = torch.full((NB, H, S, S), float("nan"), device=DEV)
    call("eg_attention_long_probs", ptr(qkvd), ptr(lse), ptr(probs), NB, S, H, kv_shift, dtype, 0)
    torch.cuda.synchronize()
    x = qkv.double().view(NB, S, 3, H, 32)
    idx = (torch.arange(NB) + kv_shift) % NB
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[idx][:, :, 1].permute(0, 2, 1, 3)
    ref = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(32), -1)
    got = probs.cpu().double()
    torch.testing.assert_close(got, ref, rtol=1e-3, atol=1e-6)
    assert (got.sum(-1) - 1).abs().max().item() < 1e-3


def test_long_entry_points_refuse_bad_arguments():
    A = torch.zeros(64, 96, device=DEV, dtype=torch.bfloat16)
    lse = torch.zeros(64, device=DEV)
    small = torch.zeros(8, device=DEV)
    with pytest.raises(L.EgError, match="2048"):
        call("eg_attention_long_fwd", ptr(A), ptr(A), ptr(lse), 1, 2049, 1, 0, L.EG_BF16, 0.0, 0, 0, 0)
    with pytest.raises(L.EgError, match="scratch"):
        call("eg_attention_long_bwd", ptr(A), ptr(A), ptr(A), ptr(lse), ptr(A), 1, 16, 1, 0, L.EG_BF16, 0.0, 0, 0,
             ptr(small), small.numel(), 0)
    with pytest.raises(L.EgError, match="dtype"):
        call("eg_attention_long_fwd", ptr(A), ptr(A), ptr(lse), 1, 16, 1, 0, 7, 0.0, 0, 0, 0)
    with pytest.raises(L.EgError, match="dtype"):
        call("eg_attention_long_probs", ptr(A), ptr(lse), ptr(lse), 1, 16, 1, 0, 7, 0)
    with pytest.raises(L.EgError):
        call("eg_attention_long_fwd", ptr(A), ptr(A), ptr(lse), 2, 16, 1, 2, L.EG_BF16, 0.0, 0, 0, 0)   # kv_shift == NB
    with pytest.raises(L.EgError):
        call("eg_attention_long_fwd", ptr(A), ptr(A), ptr(lse), 1, 16, 1, 0, L.EG_BF16, 0.1, 0, 0, 0)   # dropout without state
    torch.cuda.synchronize()
    assert float(A.float().abs().sum()) == 0.0 and float(lse.abs().sum()) == 0.0        # nothing was launched
