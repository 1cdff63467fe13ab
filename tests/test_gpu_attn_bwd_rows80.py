"""Single-sweep attention backward on 80-row LDS images (csrc/attention.hip: attn_bwd1_kernel with IR = 80 for windows of up to 80
tokens, four workgroups per CU) through eg_attention_fwd / eg_attention_bwd: against fp64 autograd at the gates of
tests/test_gpu_ops.py::test_attention_fwd_bwd (unchanged: max error < 3e-2 max(1, max|ref|), relative Frobenius error < 2e-2, lse at
1e-4), with attention dropout against autograd through the mask recovered from the forward, and with guard rows around dqkv.
S = 65 is the benchmark form (five tiles, single-key tail tile), every other S <= 80 the general form on 80-row images, S = 81 the
first window back on 96-row images.  NB * H = 3 leaves the last workgroup's second head slot as the clamped, store-less one."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from tests.dropout64 import attn_element_index, hip_keep_mask64  # noqa: E402
from tests.test_gpu_ops import DEV, DT, _attn_ref, dev_state  # noqa: E402

S_LIST = list(range(1, 16)) + [16, 17, 64, 65, 66, 79, 80, 81]
SHAPES = [(3, 1), (6, 4)]
DT16 = [L.EG_BF16, L.EG_F16]
GUARD = 4                      # guard rows of 3 D elements in front of and behind dqkv
SENTINEL = 0x5A5B              # a 16-bit pattern (bf16 and fp16: an ordinary finite number) that the kernel must leave alone


def _shifts(NB):
    return (0, max(1, NB // 2))


def _inputs(NB, S, H, dt16, seed):
    g = torch.Generator().manual_seed(seed)
    D = H * 32
    qkv = torch.randn(NB * S, 3 * D, generator=g).to(DT[dt16])
    dO = torch.randn(NB * S, D, generator=g).to(DT[dt16])
    return qkv, dO


def _fwd(qkvd, NB, S, H, kv_shift, dt16, p=0.0, site=0, st=None):
    D = H * 32
    ctx = torch.zeros(NB * S, D, device=DEV, dtype=DT[dt16])
    lse = torch.zeros(NB, H, S, device=DEV)
    call("eg_attention_fwd", ptr(qkvd), ptr(ctx), ptr(lse), NB, S, H, kv_shift, dt16, p, site, ptr(st) if st is not None else 0, 0)
    return ctx, lse


def _bwd_guarded(qkvd, ctx, dOd, lse, NB, S, H, kv_shift, dt16, p=0.0, site=0, st=None):
    """eg_attention_bwd into the middle of a larger buffer; returns (dqkv view, front guard, back guard) as int16 bit patterns' owners"""
    D = H * 32
    buf = torch.full(((NB * S + 2 * GUARD) * 3 * D,), SENTINEL, device=DEV, dtype=torch.int16)
    dqkv = buf[GUARD * 3 * D:(GUARD + NB * S) * 3 * D].view(DT[dt16]).view(NB * S, 3 * D)
    call("eg_attention_bwd", ptr(qkvd), ptr(ctx), ptr(dOd), ptr(lse), ptr(dqkv), NB, S, H, kv_shift, dt16, p, site,
         ptr(st) if st is not None else 0, 0)
    torch.cuda.synchronize()
    front, back = buf[:GUARD * 3 * D], buf[(GUARD + NB * S) * 3 * D:]
    assert bool((front == SENTINEL).all()) and bool((back == SENTINEL).all()), "a store left dqkv's rows"
    return dqkv


def _gates(got, ref):
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err < 3e-2 * max(1.0, scale), (err, scale)
    assert ((got - ref).norm() / ref.norm()).item() < 2e-2


@pytest.mark.parametrize("dt16", DT16)
@pytest.mark.parametrize("NB,H", SHAPES)
@pytest.mark.parametrize("S", S_LIST)
def test_backward_against_fp64(S, NB, H, dt16):
    for kv_shift in _shifts(NB):
        qkv, dO = _inputs(NB, S, H, dt16, seed=1000 * S + 10 * NB + kv_shift)
        qkvd, dOd = qkv.to(DEV), dO.to(DEV)
        ctx, lse = _fwd(qkvd, NB, S, H, kv_shift, dt16)
        dqkv = _bwd_guarded(qkvd, ctx, dOd, lse, NB, S, H, kv_shift, dt16)
        qr = qkv.double().requires_grad_(True)
        o_ref, lse_ref = _attn_ref(qr, NB, S, H, kv_shift)
        torch.testing.assert_close(ctx.cpu().double(), o_ref.detach(), rtol=2e-2, atol=2e-2)
        torch.testing.assert_close(lse.cpu().double(), lse_ref.detach(), rtol=1e-4, atol=1e-4)
        o_ref.backward(dO.double())
        _gates(dqkv.cpu().double(), qr.grad)


@pytest.mark.parametrize("dt16", DT16)
@pytest.mark.parametrize("NB,H", SHAPES)
@pytest.mark.parametrize("S", [16, 17, 64, 65, 66, 79, 80, 81])
def test_two_runs_are_equal_and_stores_stay_inside_their_rows(S, NB, H, dt16):
    """Two runs of one call give the same bits (with NB * H odd: the clamped head slot of the last workgroup, which recomputes window
    NB - 1's head without storing, alters nothing), with and without dropout, and the guard rows around dqkv keep their pattern."""
    st = dev_state(seed=4242)
    kv_shift = _shifts(NB)[1]
    qkv, dO = _inputs(NB, S, H, dt16, seed=7 * S + NB)
    qkvd, dOd = qkv.to(DEV), dO.to(DEV)
    for p, site in ((0.0, 0), (0.25, 9)):
        ctx, lse = _fwd(qkvd, NB, S, H, kv_shift, dt16, p, site, st)
        a = _bwd_guarded(qkvd, ctx, dOd, lse, NB, S, H, kv_shift, dt16, p, site, st)
        b = _bwd_guarded(qkvd, ctx, dOd, lse, NB, S, H, kv_shift, dt16, p, site, st)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (S, p)
        assert bool(torch.isfinite(a.float()).all())


def _recovered_mask(NB, S, H, kv_shift, p, site, st):
    """keep[b, h, q, k] read off the forward itself: with V = one-hot rows of 32 keys at a time, ctx[q, j] is the dropped
    probability of key 32 c + j (the mask depends on seed, site and element index alone, not on V)."""
    D = H * 32
    g = torch.Generator().manual_seed(S)
    base = torch.randn(NB * S, 3 * D, generator=g)
    keep = torch.zeros(NB, H, S, S, dtype=torch.bool)
    for c in range((S + 31) // 32):
        onehot = torch.zeros(S, 32)
        n = min(32, S - 32 * c)
        onehot[32 * c:32 * c + n, :n] = torch.eye(n)
        qkv = base.clone()
        qkv[:, 2 * D:] = onehot.repeat(NB, H)
        ctx, _ = _fwd(qkv.to(torch.bfloat16).to(DEV), NB, S, H, kv_shift, L.EG_BF16, p, site, st)
        torch.cuda.synchronize()
        pd = ctx.cpu().float().view(NB, S, H, 32).permute(0, 2, 1, 3)
        keep[..., 32 * c:32 * c + n] = pd[..., :n] != 0
    return keep


@pytest.mark.parametrize("dt16", DT16)
@pytest.mark.parametrize("S", [65, 80])
def test_dropout_backward_matches_autograd_through_the_forward_mask(S, dt16):
    NB, H, kv_shift, p, site, seed = 3, 2, 1, 0.25, 11, 99
    D = H * 32
    from eyegaze_multimodal_amd.engine import scramble_seed
    st = dev_state(seed=scramble_seed(seed))      # the words Engine.set_state publishes, which the CPU helper replays
    keep = _recovered_mask(NB, S, H, kv_shift, p, site, st)
    assert abs(keep.float().mean().item() - (1 - p)) < 0.02
    # the mask the forward drew is the CPU replica's: element index ((b H + h) S + q) Sp2 + key
    for w in range(NB):
        want = hip_keep_mask64(seed, site, attn_element_index(w, H, S), p)
        assert np.array_equal(keep[w].numpy(), want), w
    qkv, dO = _inputs(NB, S, H, dt16, seed=S + 5)
    qkvd, dOd = qkv.to(DEV), dO.to(DEV)
    ctx, lse = _fwd(qkvd, NB, S, H, kv_shift, dt16, p, site, st)
    dqkv = _bwd_guarded(qkvd, ctx, dOd, lse, NB, S, H, kv_shift, dt16, p, site, st)
    qr = qkv.double().requires_grad_(True)
    x = qr.reshape(NB, S, 3, H, 32)
    idx = (torch.arange(NB) + kv_shift) % NB
    q = x[:, :, 0].permute(0, 2, 1, 3)
    k, v = x[idx][:, :, 1].permute(0, 2, 1, 3), x[idx][:, :, 2].permute(0, 2, 1, 3)
    P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(32), -1)
    o = ((P * keep / (1 - p)) @ v).permute(0, 2, 1, 3).reshape(NB * S, D)
    torch.testing.assert_close(ctx.cpu().double(), o.detach(), rtol=2e-2, atol=2e-2)
    o.backward(dO.double())
    _gates(dqkv.cpu().double(), qr.grad)
