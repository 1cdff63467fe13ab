"""Conv-1 backward-data on its batched route (Engine.conv1_bwd_data: ONE eg_gemm_nt_batch call over the rows that are not
padding and the tap blocks that are not zeros) against one full launch per stride phase (conv1_bwd_batch = False).

The real rows of dh0 must be the same BYTES: a skipped tap block multiplies by zeros, which adds +0 to an accumulator at the
START of its k-ordered chain (0 + 0 = +0, and a chain that starts from +0 is the chain without that block), and a skipped row
is a row of padding that no reader touches.  The pads of dh0pad must not be written at all on the new route.
Cases at d = 256: (k, s) = (25, 4) taps 7/6/6/6, (7, 2) taps 4/3, (5, 1) one phase, (4, 4) one tap each; an odd number of
windows; a T1 at which the phases' first rows and row counts differ.  Then a whole train step at B = 2, T = 256 on both routes."""
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import DualEEGTransformer  # noqa: E402
from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from eyegaze_multimodal_amd.engine import Engine, conv_bwd_data_phases  # noqa: E402
from oracle import dual_eeg_oracle as O  # noqa: E402
from tests.test_gpu_ops import dev_state  # noqa: E402

DEV = torch.device("cuda:0")
D = 256
SENT = 7.0
TDT = {"bf16": (torch.bfloat16, L.EG_BF16), "fp16": (torch.float16, L.EG_F16)}


@pytest.fixture(autouse=True)
def restore_wide_config():
    yield
    call("eg_gemm_wide_config", -1, 1024)


class ConvOnly(Engine):
    """the part of an Engine that conv1_bwd_data reads, over buffers of the test's own (any number of windows)"""

    def __init__(self, k, s, NB, T1, dtype, seed):
        tdt, eg = TDT[dtype]
        self.cfg = types.SimpleNamespace(d_model=D)
        self.dtype, self.tdtype, self.es, self.device = eg, tdt, 2, DEV
        self.k, self.s, self.pad, self.NB, self.T1 = k, s, k // 2, NB, T1
        self.J = (k + s - 1) // s
        self.T2 = (T1 + 2 * self.pad - k) // s + 1
        self.U = (T1 + 2 * self.pad + s - 1) // s
        self.R0 = self.U * s
        self.RY = self.T2 + 2 * (self.J - 1)
        self.stream, self.probes, self.probe_all, self.conv1_bwd_batch = 0, {}, None, True
        self.state_dev = dev_state(seed=99)
        g = torch.Generator().manual_seed(seed)
        self.wf = (torch.randn(D, D, k, generator=g) * 0.05).to(DEV)
        dy = torch.zeros(NB, self.RY, D)
        dy[:, self.J - 1:self.J - 1 + self.T2] = torch.randn(NB, self.T2, D, generator=g) * 0.5
        self.w = {"conv1T": torch.zeros(s, D, self.J * D, device=DEV, dtype=tdt)}
        call("eg_pack_convT_weight", ptr(self.wf), ptr(self.w["conv1T"]), D, D, k, s, eg, 0)
        self.a = {"h0pad": torch.randn(NB, self.R0, D, generator=g).to(tdt).to(DEV)}
        self.g = {"dy1pad": dy.to(tdt).to(DEV), "dh0pad": None}

    def run(self, batch):
        self.g["dh0pad"] = torch.full((self.NB, self.R0, D), SENT, device=DEV, dtype=self.tdtype)
        self.conv1_bwd_data(1.25, batch=batch)
        torch.cuda.synchronize()
        return self.g["dh0pad"]


CASES = [
    # k, s, NB, T1
    (25, 4, 2, 64),
    (25, 4, 3, 63),     # phase 3 has one row fewer
    (7, 2, 3, 64),
    (7, 2, 2, 61),
    (5, 1, 3, 64),
    (4, 4, 2, 64),      # first rows 1 / 1 / 0 / 0
    (4, 4, 3, 60),      # ... with 15 rows each
]
# (every case keeps the FULL launches' reads inside dy1pad: they take U + J - 1 rows per window, which at (4, 4) with T1 = 61
# is one more than the buffer's RY = T2 + 2 (J - 1))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("min_rows", [1, 1024], ids=["wide_batch", "single_launches"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "k%d_s%d_NB%d_T%d" % c)
def test_batched_backward_data_equals_the_full_launches(case, min_rows, dtype):
    k, s, NB, T1 = case
    assert T1 <= 64
    eng = ConvOnly(k, s, NB, T1, dtype, seed=3)
    pad = eng.pad
    assert eng.U + eng.J - 1 <= eng.RY
    call("eg_gemm_wide_config", -1, 1024)
    old = eng.run(batch=False).clone()
    call("eg_gemm_wide_config", -1, min_rows)           # 1: every phase fits the wide kernel -> ONE batched launch
    new = eng.run(batch=True).clone()
    real = slice(pad, pad + T1)
    assert torch.equal(new[:, real].view(torch.int16), old[:, real].view(torch.int16)), \
        float((new[:, real].float() - old[:, real].float()).abs().max())
    # the pads are never written on the new route
    assert bool((new[:, :pad] == SENT).all()) and bool((new[:, pad + T1:] == SENT).all())
    assert bool((new[:, real] != SENT).any(dim=-1).all())
    # both against float64 on the 16-bit operands: conv_transpose1d of dY, gated by h0 > 0 and scaled.  One 16-bit rounding of the
    # result (2^-8 relative in bf16) plus fp32 accumulation over at most 7 * 256 products
    dy = eng.g["dy1pad"][:, eng.J - 1:eng.J - 1 + eng.T2].double().cpu().transpose(1, 2)
    w = eng.wf.to(eng.tdtype).double().cpu()
    ref = F.conv_transpose1d(dy, w, stride=s, padding=pad, output_padding=T1 - ((eng.T2 - 1) * s - 2 * pad + k)).transpose(1, 2)
    gate = eng.a["h0pad"][:, real].double().cpu()
    ref = torch.where(gate > 0, ref * 1.25, torch.zeros_like(ref))
    err = float((new[:, real].double().cpu() - ref).abs().max())
    assert err <= 1e-3 + 2.0 ** -8 * float(ref.abs().max()), err


def test_phase_table_for_the_flagship_front_end():
    """k = 25, s = 4, T1 = 256: taps 7/6/6/6, 64 real rows per phase from u = 3"""
    assert conv_bwd_data_phases(25, 4, 12, 256) == [(0, 3, 64, 0), (1, 3, 64, 1), (2, 3, 64, 1), (3, 3, 64, 1)]
    assert conv_bwd_data_phases(7, 2, 3, 64) == [(0, 2, 32, 0), (1, 1, 32, 1)]
    assert conv_bwd_data_phases(4, 4, 2, 61) == [(0, 1, 15, 0), (1, 1, 15, 0), (2, 0, 16, 0), (3, 0, 15, 0)]


# ------------------------------------------------------------------------------------------------------
# a whole train step, cfg3 flags, B = 2, T = 256
# ------------------------------------------------------------------------------------------------------
KW = dict(in_channels=8, num_classes=3, max_len=256, use_spectrogram=False, use_ibs=False, use_cross_attention=True)
B, T = 2, 256
CONV = ("temporal_conv.convs.0.weight", "temporal_conv.convs.0.bias", "temporal_conv.convs.1.weight", "temporal_conv.convs.1.bias")


def step(model, eng, batch, x1, x2, labels, train):
    eng.conv1_bwd_batch = batch
    model._flat.grad.fill_(SENT)
    eng.a["logits"].fill_(SENT)
    eng.set_state(seed=5, lr=1e-3, step=1)
    eng.forward(x1, x2, labels, train=train)
    eng.backward(gloss=torch.ones(1, device=DEV))
    torch.cuda.synchronize()
    return eng.a["loss"].clone(), eng.a["logits"].clone(), model._flat.grad.clone()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("min_rows", [1, 1024], ids=["wide_batch", "single_launches"])
def test_train_step_is_the_same_on_both_routes(min_rows, dtype):
    cfg = O.ModelCfg(**KW)
    sd = O.synthetic_state_dict(cfg, seed=7)
    model = DualEEGTransformer(**KW, compute_dtype=dtype)
    model.load_state_dict(sd)
    model = model.to(DEV)
    g = torch.Generator().manual_seed(17)
    x1, x2 = torch.randn(B, 8, T, generator=g), torch.randn(B, 8, T, generator=g)
    labels = torch.randint(0, 3, (B,), generator=g)
    eng = model.engine(B, T, DEV)
    assert eng.conv1_bwd_batch and eng.T1 == 64
    dx1, dx2, dl = x1.to(DEV), x2.to(DEV), labels.to(DEV)
    call("eg_gemm_wide_config", -1, 1024)
    old = step(model, eng, False, dx1, dx2, dl, True)
    call("eg_gemm_wide_config", -1, min_rows)
    new = step(model, eng, True, dx1, dx2, dl, True)
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])
    assert torch.equal(new[2].view(torch.int32), old[2].view(torch.int32)), float((new[2] - old[2]).abs().max())
    assert torch.isfinite(new[2]).all() and float(new[2].abs().max()) > 0
    if dtype != "bf16":
        return
    # conv gradients against oracle autograd on bf16-rounded weights and inputs, dropout off, by the project's bf16 gradient gate
    # (tests/test_gpu_model.py::test_bf16_gradients_track_the_oracle: cosine >= 0.8 and norm within 25 % for every tensor that
    # carries >= 2 % of the global norm)
    _, _, grad = step(model, eng, True, dx1, dx2, dl, False)
    rb = lambda v: v.to(torch.bfloat16).float()      # noqa: E731
    params = {k_: rb(v).clone().requires_grad_(True) for k_, v in sd.items()}
    O.forward(rb(x1), rb(x2), params, cfg, labels)["loss_ce"].backward()
    rn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params.values() if p.grad is not None)))
    fp = model._flat
    shapes = dict(zip(fp.names, fp.params))
    for n in CONV:
        r = params[n].grad.double()
        gg = grad[fp.offsets[n]:fp.offsets[n] + shapes[n].numel()].view(shapes[n].shape).double().cpu()
        if float(r.norm()) < 2e-2 * rn:
            continue
        cos, ratio = float((gg * r).sum() / (gg.norm() * r.norm())), float(gg.norm() / r.norm())
        assert cos >= 0.8 and abs(ratio - 1) <= 0.25, (n, cos, ratio)
