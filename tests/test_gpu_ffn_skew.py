"""The skewed chunk loop of ffn_chain_kernel (csrc/ffn.hip: epilogue 1 of chunk c beside product 2 of chunk c - 1) at the smallest
shapes where a skewed loop can go wrong, bit for bit (torch.equal only) against code the loop does not touch:
  * F = 128, 256, 384: one chunk (no merged phase at all), two, and three -- the odd count, where the parity of the chunk image wraps;
  * M = 7, 81, 97: less than one tile, one row into a second workgroup, a ragged second tile;
  * forward form with dropout p = 0.1 writing the gate bits, backward form reading those bits, backward form with the row gate:
    H and C against two eg_gemm_nt launches;
  * the backward form with the norm-1 tail (eg_ffn_bwd_ln_proj) against eg_ffn_chain followed by eg_ln_bwd_proj;
  * the forward form with the fused LayerNorm at F = 384: H and C against the two launches, the normalised rows and statistics held
    to the gate of tests/test_gpu_lnfuse.py against eg_layernorm_fwd; the lean form's rows equal the keeping form's."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
import tests.test_gpu_ffn as TF  # noqa: E402
import tests.test_gpu_ffn_lnproj as TP  # noqa: E402
from tests.test_gpu_lnfuse import check_ln  # noqa: E402

DEV = "cuda"
D = 256
P = 0.1
FS = [128, 256, 384]
MS = [7, 81, 97]
DTYPES = pytest.mark.parametrize("dtype", [L.EG_BF16, L.EG_F16], ids=["bf16", "fp16"])


@functools.lru_cache(maxsize=None)
def forward_case(M, F, dtype):
    """Operands, the two-launch forward reference (computed once, shared, never written again) and the one-launch forward with its bits"""
    o = TF.operands(M, F, dtype, seed=17)
    H2, C2 = TF.two_launches(o, M, F, dtype, "fwd", P)
    bits = TF.gate_bits(M, F)
    H1, C1 = TF.one_launch(o, M, F, dtype, "fwd", P, bits_out=bits)
    return o, H2, C2, H1, C1, bits


@DTYPES
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("F", FS)
def test_forward_form_with_dropout_and_gate_bits(F, M, dtype):
    o, H2, C2, H1, C1, bits = forward_case(M, F, dtype)
    assert torch.equal(H1, H2), float((H1.float() - H2.float()).abs().max())
    assert torch.equal(C1, C2), float((C1.float() - C2.float()).abs().max())
    assert 0.2 < float((H2 > 0).float().mean()) < 0.6                # dropout and ReLU both cut
    assert int((bits != 0).sum()) > 0


@DTYPES
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("F", FS)
def test_backward_forms_with_gate_bits_and_with_the_row_gate(F, M, dtype):
    o, H2f, _, _, _, bits = forward_case(M, F, dtype)
    ob = dict(o, A=o["R"], G=H2f, R=o["A"])                          # the gate: the hidden rows the two-launch forward stored
    H2, C2 = TF.two_launches(ob, M, F, dtype, "bwd", 0.0)
    Hb, Cb = TF.one_launch(ob, M, F, dtype, "bwd", 0.0, bits_in=bits)
    assert torch.equal(Hb, H2), float((Hb.float() - H2.float()).abs().max())
    assert torch.equal(Cb, C2), float((Cb.float() - C2.float()).abs().max())
    Hr, Cr = TF.one_launch(ob, M, F, dtype, "bwd", 0.0)
    assert torch.equal(Hr, H2), float((Hr.float() - H2.float()).abs().max())
    assert torch.equal(Cr, C2), float((Cr.float() - C2.float()).abs().max())
    assert float(H2.float().abs().max()) > 0


@DTYPES
def test_tail_form_equals_ffn_chain_then_ln_bwd_proj(dtype):
    M, F, p1, gate_scale = 81, 384, 0.1, 1 / 0.9
    i = TP.inputs(M, F, dtype, seed=5)
    ref = TP.outputs(M, F, dtype)
    f, n = TP.descs(i, ref, M, F, dtype, p1, gate_scale, True, ptr(ref["C"]))
    call("eg_ffn_chain", C.byref(f), 0)
    call("eg_ln_bwd_proj", C.byref(n), 0)
    got = TP.outputs(M, F, dtype)
    f, n = TP.descs(i, got, M, F, dtype, p1, gate_scale, True, ptr(got["C"]))
    call("eg_ffn_bwd_ln_proj", C.byref(f), C.byref(n), 0)
    torch.cuda.synchronize()
    # eg_ffn_chain's backward form is itself the skewed loop: its H and C are held to the two launches above; here also to the row gate
    for k in ("H", "C", "dx", "dxd", "dC", "part"):
        assert torch.equal(got[k], ref[k]), (k, float((got[k].float() - ref[k].float()).abs().max()))
    assert float(ref["dC"][:M].float().abs().max()) > 0 and float(ref["H"][:M].float().abs().max()) > 0


def lnf_launch(o, M, F, dtype, gamma, beta, lean):
    t = TF.TDT[dtype]
    H = torch.full((M, F), 7.0, device=DEV, dtype=t)
    Cc, y = (torch.full((M, D), 7.0, device=DEV, dtype=t) for _ in range(2))
    st = torch.full((M, 2), 7.0, device=DEV)
    f = L.FfnDesc()
    w1f, w2f = TF.frag_pack(o["W1"], 3, dtype), TF.frag_pack(o["W2"], 5, dtype)
    f.A, f.W1, f.W2, f.state = ptr(o["A"]), ptr(w1f), ptr(w2f), ptr(o["st"])
    if not lean:
        f.H, f.C, f.ln_stats = ptr(H), ptr(Cc), ptr(st)
    f.lda, f.ldh, f.ldc, f.ldg, f.ldr, f.M, f.F, f.dtype = D, F, D, F, D, M, F, dtype
    f.bias1, f.bias2, f.act1, f.residual = ptr(o["b1"]), ptr(o["b2"]), L.ACT_RELU, ptr(o["A"])
    f.drop_h_p, f.drop_h_site, f.drop_c1_p, f.drop_c1_site, f.drop_c2_p, f.drop_c2_site = P, 21, P, 22, P, 23
    f.ln_gamma, f.ln_beta, f.ln_out = ptr(gamma), ptr(beta), ptr(y)
    call("eg_ffn_chain", C.byref(f), 0)
    torch.cuda.synchronize()
    return H, Cc, y, st


@DTYPES
@pytest.mark.parametrize("M", [81, 97])
def test_layernorm_form_and_lean_form_at_three_chunks(M, dtype):
    F = 384
    o, H2, C2, _, _, _ = forward_case(M, F, dtype)
    g = torch.Generator().manual_seed(M + F)
    gamma = (1.0 + 0.2 * torch.randn(D, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(D, generator=g)).to(DEV)
    H, Cc, y, st = lnf_launch(o, M, F, dtype, gamma, beta, lean=False)
    assert torch.equal(H, H2), float((H.float() - H2.float()).abs().max())
    assert torch.equal(Cc, C2), float((Cc.float() - C2.float()).abs().max())
    check_ln(y, st, C2, gamma, beta, dtype)
    Hl, Cl, yl, stl = lnf_launch(o, M, F, dtype, gamma, beta, lean=True)
    assert torch.equal(yl, y), float((yl.float() - y.float()).abs().max())
    assert bool((Hl == 7.0).all()) and bool((Cl == 7.0).all()) and bool((stl == 7.0).all())     # the lean form stores nothing else
