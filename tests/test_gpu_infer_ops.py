"""The forward-only ("lean") forms of the two fused encoder launches and the device-side evaluation tail, through the C ABI:
  * eg_ffn_chain with H and C null and eg_attn_block_fwd with qkv, ctx, lse and r1 null store the normed rows alone.  They run the
    arithmetic of the keeping forms (same LDS images, MFMA chains, rounding points and dropout code), so ln_out is compared BIT FOR
    BIT with the keeping launch's, with and without dropout; canary rows behind ln_out must stay untouched;
  * eg_eval_accumulate against torch.argmax and a numpy confusion matrix, rows with exact ties included, two calls accumulating."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from tests.test_gpu_ops import DEV, DT  # noqa: E402

D = 256
CANARY = 8          # rows behind ln_out that no launch may touch


def gain_bias(seed):
    g = torch.Generator().manual_seed(seed)
    return (1.0 + 0.2 * torch.randn(D, generator=g)).to(DEV), (0.1 * torch.randn(D, generator=g)).to(DEV)


def normed(M, dtype):
    return torch.full((M + CANARY, D), 7.0, device=DEV, dtype=DT[dtype])


def check(M, lean, keep):
    assert torch.isfinite(keep[:M].float()).all() and not torch.equal(keep[:M], torch.full_like(keep[:M], 7.0))
    assert torch.equal(lean[:M], keep[:M]), (int((lean[:M] != keep[:M]).sum()), float((lean[:M].float() - keep[:M].float()).abs().max()))
    assert bool((lean[M:] == 7.0).all()) and bool((keep[M:] == 7.0).all())


def ffn_launch(o, w1f, w2f, gamma, beta, M, F, dtype, p, lean):
    t = DT[dtype]
    y = normed(M, dtype)
    f = L.FfnDesc()
    f.A, f.W1, f.W2, f.state = ptr(o["A"]), ptr(w1f), ptr(w2f), ptr(o["st"])
    f.lda, f.ldg, f.ldr, f.M, f.F, f.dtype = D, F, D, M, F, dtype
    f.bias1, f.bias2, f.act1, f.residual = ptr(o["b1"]), ptr(o["b2"]), L.ACT_RELU, ptr(o["A"])
    f.drop_h_p, f.drop_h_site, f.drop_c1_p, f.drop_c1_site, f.drop_c2_p, f.drop_c2_site = p, 21, p, 22, p, 23
    f.ln_gamma, f.ln_beta, f.ln_out = ptr(gamma), ptr(beta), ptr(y)
    keepalive = None
    if not lean:
        keepalive = (torch.zeros(M, F, device=DEV, dtype=t), torch.zeros(M, D, device=DEV, dtype=t), torch.zeros(M, 2, device=DEV))
        f.H, f.C, f.ln_stats = (ptr(x) for x in keepalive)
        f.ldh, f.ldc = F, D
    call("eg_ffn_chain", C.byref(f), 0)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("dtype", [L.EG_BF16, L.EG_F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("F", [128, 256])           # one chunk; two chunks: both LDS chunk buffers and the weight rings wrap
@pytest.mark.parametrize("M", [1, 80, 81, 161])     # a lone row, a full tile, a one-row second tile, a partial third tile
def test_lean_ffn_chain_gives_the_keeping_forms_normed_rows(M, F, dtype, p):
    import tests.test_gpu_ffn as TF
    o = TF.operands(M, F, dtype, seed=17)
    w1f, w2f = TF.frag_pack(o["W1"], 3, dtype), TF.frag_pack(o["W2"], 5, dtype)
    gamma, beta = gain_bias(M + F)
    keep = ffn_launch(o, w1f, w2f, gamma, beta, M, F, dtype, p, lean=False)
    lean = ffn_launch(o, w1f, w2f, gamma, beta, M, F, dtype, p, lean=True)
    check(M, lean, keep)


def attn_launch(o, wqkv, wo, gamma, beta, NB, S, dtype, p, lean):
    t = DT[dtype]
    M = NB * S
    y = normed(M, dtype)
    d = L.AttnBlockDesc()
    d.x, d.wqkv_frag, d.wo_frag, d.bqkv, d.bo, d.state = ptr(o["x"]), ptr(wqkv), ptr(wo), ptr(o["bqkv"]), ptr(o["bo"]), ptr(o["st"])
    d.NB, d.S, d.d_model, d.num_heads, d.dtype = NB, S, D, 8, dtype
    d.attn_drop_p, d.attn_drop_site, d.out_drop_p, d.out_drop_site = p, 21, p, 22
    d.ln_gamma, d.ln_beta, d.ln_out = ptr(gamma), ptr(beta), ptr(y)
    keepalive = None
    if not lean:
        keepalive = (torch.zeros(M, 3 * D, device=DEV, dtype=t), torch.zeros(M, D, device=DEV, dtype=t),
                     torch.zeros(NB, 8, S, device=DEV), torch.zeros(M, D, device=DEV, dtype=t), torch.zeros(M, 2, device=DEV))
        d.qkv, d.ctx, d.lse, d.r1, d.ln_stats = (ptr(x) for x in keepalive)
    call("eg_attn_block_fwd", C.byref(d), 0)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("dtype", [L.EG_BF16, L.EG_F16], ids=["bf16", "fp16"])
# one tile, a tile edge, a single-key tail tile in the general form, the exact S = 65 instantiation, the last partial tile, the full tile
@pytest.mark.parametrize("S", [1, 16, 17, 65, 79, 80])
@pytest.mark.parametrize("NB", [1, 3])
def test_lean_attention_block_gives_the_keeping_forms_normed_rows(NB, S, dtype, p):
    from tests.test_gpu_attnblock import frag_weights, operands
    o = operands(NB, S, dtype, seed=11)
    wqkv, wo = frag_weights(o, dtype)
    gamma, beta = gain_bias(NB + S)
    keep = attn_launch(o, wqkv, wo, gamma, beta, NB, S, dtype, p, lean=False)
    lean = attn_launch(o, wqkv, wo, gamma, beta, NB, S, dtype, p, lean=True)
    check(NB * S, lean, keep)


@pytest.mark.parametrize("ncls", [2, 3, 16])
@pytest.mark.parametrize("B", [1, 5, 257])
def test_eval_accumulate_against_argmax_and_a_host_confusion_matrix(B, ncls):
    g = torch.Generator().manual_seed(100 * B + ncls)
    cm_ref, loss_ref = np.zeros((ncls, ncls), np.int64), 0.0
    cm = torch.zeros(ncls, ncls, device=DEV, dtype=torch.int32)
    loss_sum = torch.zeros(1, device=DEV)
    for call_no in range(2):
        logits = torch.randn(B, ncls, generator=g)
        logits[::3] = logits[::3].round()                      # coarse values: exact ties within a row
        logits[::4, -1] = logits[::4].max(-1).values           # ... and a tie between the maximum and the LAST class, on purpose
        labels = torch.randint(0, ncls, (B,), generator=g)
        loss = torch.rand(1, generator=g)
        pred = torch.full((B + 4,), -7, device=DEV, dtype=torch.int32)
        dl, dy, dloss = logits.to(DEV), labels.to(DEV), loss.to(DEV)
        call("eg_eval_accumulate", ptr(dl), ptr(dy), ptr(dloss), ptr(pred), ptr(cm), ptr(loss_sum), B, ncls, 0)
        torch.cuda.synchronize()
        ref = torch.argmax(dl, -1).cpu()
        assert torch.equal(pred[:B].cpu().long(), ref) and bool((pred[B:] == -7).all())
        np.add.at(cm_ref, (labels.numpy(), ref.numpy()), 1)
        loss_ref += float(loss)
        assert np.array_equal(cm.cpu().numpy(), cm_ref), call_no
        assert abs(float(loss_sum) - loss_ref) <= 1e-6 * max(1.0, loss_ref)
    assert int(cm.sum()) == 2 * B
    if B > 8 and ncls > 2:
        tied = (logits == logits.max(-1, keepdim=True).values).sum(-1) > 1
        assert bool(tied.any())                                # the data did hold ties


def test_eval_accumulate_without_labels_writes_predictions_only():
    logits = torch.tensor([[0.0, 2.0, 2.0], [1.0, -1.0, 0.5]], device=DEV)
    pred = torch.zeros(2, device=DEV, dtype=torch.int32)
    call("eg_eval_accumulate", ptr(logits), 0, 0, ptr(pred), 0, 0, 2, 3, 0)
    torch.cuda.synchronize()
    assert pred.tolist() == [1, 0]
