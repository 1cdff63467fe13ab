"""eg_ffn_bwd_ln_proj (csrc/ffn.hip): the feed-forward backward launch going on with norm-1's backward and out_proj's backward-data
product on the rows it has just completed, against eg_ffn_chain (backward form) followed by eg_ln_bwd_proj on that launch's C.
Same tiles, arithmetic and summation order, so EVERYTHING is bit-identical: H, C (when requested), dx, dx_drop, dC and each
workgroup's row of the gain / bias partials.  Outputs are pre-filled with 7.0 and carry guard rows behind row M that must keep it.
One engine-level case: a training step with the route on equals the step with the route off, bit for bit."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd._lib import FfnDesc, LnBwdProjDesc, call, ptr  # noqa: E402
from tests.test_gpu_ffn import TDT, frag_pack, gate_bits, one_launch, operands  # noqa: E402
from tests.test_gpu_ops import dev_state  # noqa: E402

DEV = "cuda"
D = 256
GUARD = 3      # rows behind row M (and one partial row behind the last block's)


def inputs(M, F, dtype, seed):
    """The backward form's operands (the gate bit image comes from a forward launch of the same geometry) and norm-1's"""
    t = TDT[dtype]
    o = operands(M, F, dtype, seed)
    bits = gate_bits(M, F)
    one_launch(o, M, F, dtype, "fwd", 0.1, bits_out=bits)
    g = torch.Generator().manual_seed(1000 + seed + M + F)
    x = torch.randn(M, D, generator=g).to(t).to(DEV)                        # r1: the LayerNorm input rows
    gamma = (1.0 + 0.2 * torch.randn(D, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(D, generator=g)).to(DEV)
    Wo = (torch.randn(D, D, generator=g) / math.sqrt(D)).to(DEV)           # out_proj.weight [out, in]
    stats = torch.zeros(M, 2, device=DEV)
    call("eg_layernorm_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(torch.zeros_like(x)), ptr(stats), M, D, dtype, 0)
    return dict(dY=o["R"], res=o["A"], bits=bits, x=x, gamma=gamma, stats=stats, st=dev_state(seed=31 + seed),
                w1f=frag_pack(o["W1"].t().contiguous(), 4, dtype), w2f=frag_pack(o["W2"].t().contiguous(), 6, dtype),
                wof=frag_pack(Wo, 6, dtype))


def outputs(M, F, dtype):
    t, nb = TDT[dtype], L.lib().eg_ln_bwd_proj_blocks(M)
    mk = lambda cols: torch.full((M + GUARD, cols), 7.0, device=DEV, dtype=t)
    return dict(H=mk(F), C=mk(D), dx=mk(D), dxd=mk(D), dC=mk(D), part=torch.full((nb + 1, 2 * D), 7.0, device=DEV))


def descs(i, out, M, F, dtype, p1, gate_scale, store_c, dy):
    f = FfnDesc()
    f.A, f.W1, f.W2, f.H, f.C = ptr(i["dY"]), ptr(i["w1f"]), ptr(i["w2f"]), ptr(out["H"]), ptr(out["C"]) if store_c else None
    f.residual, f.gate_bits_in, f.state, f.gate_scale = ptr(i["res"]), ptr(i["bits"]), ptr(i["st"]), gate_scale
    f.lda, f.ldh, f.ldc, f.ldg, f.ldr = D, F, D, F, D
    f.M, f.F, f.dtype = M, F, dtype
    n = LnBwdProjDesc()
    n.dy, n.x, n.stats, n.gamma, n.W_frag = dy, ptr(i["x"]), ptr(i["stats"]), ptr(i["gamma"]), ptr(i["wof"])
    n.dx, n.dx_drop, n.dC, n.partial, n.state = ptr(out["dx"]), ptr(out["dxd"]), ptr(out["dC"]), ptr(out["part"]), ptr(i["st"])
    n.M, n.d_model, n.dtype, n.partial_capacity_blocks = M, D, dtype, out["part"].shape[0] - 1
    n.drop1_p, n.drop1_site = p1, 5
    return f, n


# M: a partial tile, an exact tile, one row over, ragged many-tile, 52 tiles;  F: one chunk, two chunks, the workload's;
# (drop1_p, gate_scale): off / on;  C stored or not.  Every value appears in each dtype; the small shapes take more combinations.
CASES = [
    (7, 128, 0.0, 1.0, True), (7, 256, 0.1, 1 / 0.9, False), (80, 256, 0.1, 1 / 0.9, True), (80, 128, 0.0, 1.0, False),
    (81, 1024, 0.0, 1.0, False), (81, 128, 0.1, 1 / 0.9, True), (1000, 256, 0.1, 1 / 0.9, False), (1000, 128, 0.0, 1.0, True),
    (4160, 1024, 0.1, 1 / 0.9, True), (4160, 256, 0.0, 1.0, False),
]


@pytest.mark.parametrize("dtype", [L.EG_BF16, L.EG_F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "M%d_F%d_p%g_s%.3g_%s" % (c[:4] + ("C" if c[4] else "noC",)))
def test_one_launch_equals_ffn_chain_then_ln_bwd_proj(case, dtype):
    M, F, p1, gate_scale, store_c = case
    i = inputs(M, F, dtype, seed=3)
    ref = outputs(M, F, dtype)
    f, n = descs(i, ref, M, F, dtype, p1, gate_scale, True, ptr(ref["C"]))
    call("eg_ffn_chain", C.byref(f), 0)
    call("eg_ln_bwd_proj", C.byref(n), 0)
    got = outputs(M, F, dtype)
    f, n = descs(i, got, M, F, dtype, p1, gate_scale, store_c, ptr(got["C"]) if store_c else None)
    call("eg_ffn_bwd_ln_proj", C.byref(f), C.byref(n), 0)
    torch.cuda.synchronize()
    for k in ("H", "C", "dx", "dxd", "dC"):
        if k == "C" and not store_c:
            assert bool((got[k] == 7.0).all())                                   # not requested: not written
            continue
        assert torch.equal(got[k][:M], ref[k][:M]), (k, float((got[k][:M].float() - ref[k][:M].float()).abs().max()))
        assert bool((got[k][M:] == 7.0).all()) and bool((ref[k][M:] == 7.0).all()), k       # nothing stored past M
    assert torch.equal(got["part"], ref["part"])                                 # per block, not merely their sum
    assert bool((got["part"][-1] == 7.0).all()) and bool(torch.isfinite(got["part"][:-1]).all())
    assert float(ref["dC"][:M].float().abs().max()) > 0 and float(ref["H"][:M].float().abs().max()) > 0
    if p1 > 0:
        assert 0.05 < float((got["dxd"][:M] == 0).float().mean()) < 0.3


def test_a_training_step_is_the_same_on_either_route():
    """cfg3 flags, B = 2, T = 1024, bf16: loss, logits and the whole flat gradient buffer, route on against route off"""
    from eyegaze_multimodal_amd import DualEEGTransformer, HipAdamW
    from oracle import dual_eeg_oracle as O
    kw = dict(in_channels=8, num_classes=3, max_len=256, use_spectrogram=False, use_ibs=False, use_cross_attention=True)
    dev, B, T = torch.device("cuda:0"), 2, 1024
    results = []
    for route in (True, False):
        model = DualEEGTransformer(**kw, compute_dtype="bf16")
        model.load_state_dict(O.synthetic_state_dict(O.ModelCfg(**kw), seed=7))
        model = model.to(dev)
        g = torch.Generator().manual_seed(13)
        x1, x2 = torch.randn(B, 8, T, generator=g).to(dev), torch.randn(B, 8, T, generator=g).to(dev)
        labels = torch.randint(0, 3, (B,), generator=g).to(dev)
        eng = model.engine(B, T, dev)
        assert eng.fuse_ffn and eng.ln_proj
        eng.ffn_ln_proj = route
        opt = HipAdamW(model)
        opt.begin_step(eng, seed=21)
        eng.forward(x1, x2, labels, train=True)
        eng.backward(gloss=torch.ones(1, device=dev))
        torch.cuda.synchronize()
        results.append(dict(loss=eng.a["loss"].clone(), logits=eng.a["logits"].clone(), grad=model._flat.grad.clone()))
    on, off = results
    for k in on:
        assert bool(torch.isfinite(on[k]).all()), k
        assert torch.equal(on[k], off[k]), (k, float((on[k].float() - off[k].float()).abs().max()))
    assert float(on["grad"].abs().max()) > 0
