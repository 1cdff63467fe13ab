"""CPU-only: the host side of eg_ffn_bwd_ln_proj (the feed-forward backward launch with norm-1's backward and out_proj's
backward-data product as its tail).  Every check is made before the launch, so each bad descriptor pair is refused here with its
message; the fake non-null pointers are never dereferenced.  And the engine's route `ffn_ln_proj` follows its two parent routes."""
import ctypes as C

import pytest
import torch

from eyegaze_multimodal_amd import DualEEGTransformer
from eyegaze_multimodal_amd import _lib as L
from eyegaze_multimodal_amd.engine import Engine

P = 0x1000      # 16-B aligned, never dereferenced
M, F, D = 1000, 256, 256
WHO = "eg_ffn_bwd_ln_proj: "


def pair(f_kw=None, n_kw=None):
    """a valid descriptor pair (f in the backward form, n reading the rows of the launch itself), then the overrides"""
    f = L.FfnDesc()
    f.A, f.W1, f.W2, f.H, f.C, f.residual, f.gate_bits_in = P, P, P, P, P, P, P
    f.lda, f.ldh, f.ldc, f.ldg, f.ldr = D, F, D, F, D
    f.M, f.F, f.dtype, f.gate_scale = M, F, L.EG_BF16, 1.0
    n = L.LnBwdProjDesc()
    n.dy, n.x, n.stats, n.gamma, n.W_frag, n.dx, n.dx_drop, n.dC, n.partial = P, P, P, P, P, P, P, P, P
    n.M, n.d_model, n.dtype, n.partial_capacity_blocks = M, D, L.EG_BF16, L.lib().eg_ln_bwd_proj_blocks(M)
    for dsc, kw in ((f, f_kw), (n, n_kw)):
        for k, v in (kw or {}).items():
            setattr(dsc, k, v)
    return f, n


BAD = [
    # -- eg_ffn_chain's checks on f
    (dict(A=None), None, WHO + "null operand"),
    (dict(dtype=L.EG_F32), dict(dtype=L.EG_F32), WHO + "16-bit compute dtypes only"),
    (dict(F=100), None, "F must be a multiple of 128"),
    (dict(act1=9), None, WHO + "act1 9"),
    (dict(lda=100), None, WHO + "row strides must be 16-B multiples"),
    (dict(ldc=100), None, WHO + "row strides must be 16-B multiples"),
    (dict(gate=P, ldg=3), None, WHO + "gate stride"),
    (dict(gate_bits_out=P), None, WHO + "a launch either writes gate bits or applies a gate"),
    (dict(gate_bits_in=P + 4), None, WHO + "gate bit words must be 8-B aligned"),
    (dict(ldr=100), None, WHO + "residual stride"),
    (dict(M=1 << 24, F=1024, ldh=1024), dict(M=1 << 24), WHO + "M\\*F exceeds the 32-bit dropout index"),
    (dict(drop_h_p=1.0), None, WHO + "dropout p"),
    (dict(drop_c1_p=0.1), None, WHO + "dropout needs a step state"),
    (dict(A=P + 8), None, WHO + "operands must be 16-B aligned"),
    # -- eg_ln_bwd_proj's checks on n
    (None, dict(x=None), WHO + "null operand"),
    (None, dict(dtype=L.EG_F32), WHO + "16-bit compute dtypes only"),
    (None, dict(d_model=64), WHO + "M=1000, d_model=64 \\(256 only\\)"),
    (None, dict(partial_capacity_blocks=4), WHO + "the partial buffer holds 4 rows, the launch writes 13"),
    (None, dict(drop1_p=1.5), WHO + "dropout p"),
    (None, dict(drop1_p=0.1), WHO + "dropout needs a step state"),
    (None, dict(dx=P + 8), WHO + "operands must be 16-B aligned"),
    # -- the pair
    (dict(gate_bits_in=None), None, WHO + "f must be the backward form: gate_bits_in is not set"),
    (dict(bias1=P), None, WHO + "f must be the backward form: no bias1"),
    (dict(act1=L.ACT_RELU), None, WHO + "f must be the backward form: no bias1, act1"),
    (dict(gate=P), None, WHO + "f must be the backward form: no bias1, act1, gate"),
    (dict(H=None), None, WHO + "f->H \\(the hidden gradient rows\\) must be given"),
    (None, dict(dy=P + 0x100), WHO + "n->dy must be NULL or f->C"),
    (dict(C=None), None, WHO + "n->dy must be NULL or f->C"),
    (None, dict(M=M - 1), WHO + "n->M=999 differs from f->M=1000"),
    (dict(dtype=L.EG_F16), None, WHO + "n->dtype=1 differs from f->dtype=2"),
]


@pytest.mark.parametrize("f_kw,n_kw,msg", BAD, ids=[f"{i:02d}" for i in range(len(BAD))])
def test_each_bad_descriptor_is_refused_with_its_message(f_kw, n_kw, msg):
    f, n = pair(f_kw, n_kw)
    with pytest.raises(L.EgError, match=msg):
        L.call("eg_ffn_bwd_ln_proj", C.byref(f), C.byref(n), 0)


def test_null_descriptors_are_refused():
    f, n = pair()
    with pytest.raises(L.EgError, match=WHO + "null descriptor"):
        L.call("eg_ffn_bwd_ln_proj", None, C.byref(n), 0)
    with pytest.raises(L.EgError, match=WHO + "null descriptor"):
        L.call("eg_ffn_bwd_ln_proj", C.byref(f), None, 0)


def test_the_existing_entry_points_keep_their_own_names_in_their_messages():
    f, n = pair(dict(F=100), dict(partial_capacity_blocks=4))
    with pytest.raises(L.EgError, match="eg_ffn_chain: M=1000, F=100"):
        L.call("eg_ffn_chain", C.byref(f), 0)
    with pytest.raises(L.EgError, match="eg_ln_bwd_proj: the partial buffer holds 4 rows"):
        L.call("eg_ln_bwd_proj", C.byref(n), 0)
    f, n = pair(dict(C=None))
    with pytest.raises(L.EgError, match="eg_ffn_chain: H and C are both given"):      # C alone may be NULL on the fused entry only
        L.call("eg_ffn_chain", C.byref(f), 0)


def engine(monkeypatch, dtype, **kw):
    model = DualEEGTransformer(in_channels=8, max_len=256, use_spectrogram=False, use_ibs=False, **kw)
    cpu = torch.device("cpu")
    model._flat.ensure(cpu)
    monkeypatch.setattr("eyegaze_multimodal_amd.engine.call", lambda name, *args: None)     # launches are not issued
    return Engine(model, 4, 1024, cpu, dtype)


def test_the_route_follows_its_two_parent_routes(monkeypatch):
    eng = engine(monkeypatch, L.EG_BF16)
    assert eng.fuse_ffn and eng.ln_proj and eng.ffn_ln_proj is True
    assert engine(monkeypatch, L.EG_F32).ffn_ln_proj is False
    assert engine(monkeypatch, L.EG_BF16, d_model=64, num_heads=2, d_ff=128, num_layers=2).ffn_ln_proj is False
