"""Synchrony (IBS) tokens at window lengths that are not powers of two: the mixed-radix FFT of eg_ibs_analytic, the partial last
time chunk of eg_ibs_pairs and eg_ibs_scalar, against the CPU oracle (torch.fft), then whole models built through
train_art.build_model at the reference dataset's own window (1000 samples at 250 Hz) and at 2000 samples (S = 200: the long
attention core).  Every case here was refused before (T had to be a power of two)."""
import copy
import ctypes as CT
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import train_art as TA  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from eyegaze_multimodal_amd.data import randn_windows  # noqa: E402
from eyegaze_multimodal_amd.tokens import nbin_for  # noqa: E402
from oracle import dual_eeg_oracle as O  # noqa: E402
from tests.helpers import GOLDEN, WEIGHT_SEED  # noqa: E402

DEV = "cuda"
# 96 = 4 4 2 3, 100 = 4 5 5, 250 = 2 5 5 5 (below one 256-step chunk), 1000 = 4 2 5 5 5, 1125 = 3 3 5 5 5 (odd),
# 1021 (prime: the direct DFT stage), 2000 = 4 4 5 5 5, 2002 = 2 7 11 13 (radix 7 and two other primes), 2046 = 2 3 11 31 and
# 2047 = 23 89 (the largest analytic LDS: 32 T + 96 B = 65 600 B, past 64 KiB)
LENGTHS = [96, 100, 250, 1000, 1125, 1021, 2000, 2002, 2046, 2047]


def bands(bl):
    return (CT.c_float * len(bl))(*[b[0] for b in bl]), (CT.c_float * len(bl))(*[b[1] for b in bl])


def signals(B, Cc, T, fs, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(B, Cc, T, generator=g)
    t_ = torch.arange(T) / fs
    x1 = base + torch.sin(2 * math.pi * 10 * t_) + 0.5 * torch.sin(2 * math.pi * 22 * t_ + 1.0)
    x2 = 0.6 * base.roll(5, dims=2) + 0.4 * torch.randn(B, Cc, T, generator=g) + torch.sin(2 * math.pi * 10 * t_ + 0.7)
    return x1, x2


def analytic(x1, x2, T, fs, bl):
    nb = len(bl)
    lo, hi = bands(bl)
    nsig, nbin = 2 * x1.shape[0] * x1.shape[1], nbin_for(T, fs, max(b[1] for b in bl))
    xcat = torch.cat([x1, x2], 0).contiguous().to(DEV)
    xb, ph = torch.full((nb, nsig, T), float("nan"), device=DEV), torch.full((nb, nsig, T), float("nan"), device=DEV)
    stats, spec = torch.zeros(nb, nsig, 4, device=DEV), torch.zeros(nsig, nbin, 2, device=DEV)
    call("eg_ibs_analytic", ptr(xcat), ptr(xb), ptr(ph), ptr(stats), ptr(spec), nsig, T, fs, nbin, CT.addressof(lo),
         CT.addressof(hi), nb, 0)
    return xb, ph, stats, spec, nbin


def pairs(xb, ph, stats, spec, B, Cc, T, fs, nbin):
    lo, hi = bands(O.ROBUST_BANDS)
    conn = torch.full((B, 6, 7, Cc, Cc), float("nan"), device=DEV)
    call("eg_ibs_pairs", ptr(xb), ptr(ph), ptr(stats), ptr(spec), ptr(conn), B, Cc, T, fs, nbin, CT.addressof(lo),
         CT.addressof(hi), 6, 0)
    return conn


def check_conn(got, ref, T, sign_features):
    """gates of tests/test_gpu_ops.py::test_ibs_connectivity_shapes: sign()-based features (PLI, wPLI) may flip a sample of T
    where a phase difference is ~0 (one flip moves PLI by 2/T), every other feature within 1e-4"""
    assert np.isfinite(got).all()
    for f in range(got.shape[2]):
        d = np.abs(got[:, :, f] - ref[:, :, f])
        if f in sign_features:
            assert (d > 1e-4).mean() < 5e-3 and d.max() < 6.5 / T, (f, d.max())
        else:
            assert d.max() < 1e-4, (f, d.max())


@pytest.mark.parametrize("fs", [256.0, 250.0])
@pytest.mark.parametrize("T", LENGTHS)
def test_analytic_signal_and_connectivity(T, fs):
    B, Cc = (2, 5) if T % 2 else (1, 12)                 # C not a multiple of the 8 x 8 tile either way
    x1, x2 = signals(B, Cc, T, fs, 300 + T)
    xb, ph, stats, spec, nbin = analytic(x1, x2, T, fs, O.ROBUST_BANDS)
    conn = pairs(xb, ph, stats, spec, B, Cc, T, fs, nbin)
    torch.cuda.synchronize()
    # band-limited signal and instantaneous phase of every band against the oracle (rFFT mask + irfft, then FFT Hilbert)
    xcat = torch.cat([x1, x2], 0)
    for b, (lo, hi) in enumerate(O.ROBUST_BANDS):
        ref_xb = O.bandpass(xcat, fs, lo, hi)
        got_xb = xb[b].cpu().reshape(2 * B, Cc, T)
        np.testing.assert_allclose(got_xb.numpy(), ref_xb.numpy(), atol=2e-5, err_msg=f"band {b}")
        hvec = torch.zeros(T)
        hvec[0] = 1
        hvec[1:(T + 1) // 2] = 2
        if T % 2 == 0:
            hvec[T // 2] = 1
        mag = torch.fft.ifft(torch.fft.fft(ref_xb.double(), dim=-1) * hvec, dim=-1).abs()
        dphi = (ph[b].cpu().reshape(2 * B, Cc, T).double() - O.hilbert_phase(ref_xb.double())).numpy()
        dphi = np.abs((dphi + np.pi) % (2 * np.pi) - np.pi)
        keep = (mag > 1e-3 * mag.max()).numpy()
        # a phase error times |analytic| is the error of the analytic signal across its direction: the xb budget, twice over
        tang = (dphi * mag.numpy())[keep]
        assert tang.max() < 4e-5, (b, float(tang.max()), float(dphi[keep].max()))
    # spectrum bins the pairs kernel reads for coherence: the raw rFFT
    ref_spec = torch.fft.rfft(xcat.double(), dim=-1)[..., :nbin]
    got_spec = spec.cpu().double().reshape(2 * B, Cc, nbin, 2)
    err = (torch.view_as_complex(got_spec.contiguous()) - ref_spec).abs().max() / ref_spec.abs().max()
    assert float(err) < 1e-5, float(err)
    ref = O.ibs_connectivity(x1, x2, O.ModelCfg(in_channels=Cc, sampling_rate=fs)).numpy()
    check_conn(conn.cpu().numpy(), ref, T, (1, 2))


@pytest.mark.parametrize("T,fs", [(1000, 250.0), (1125, 250.0), (1000, 256.0)])
def test_scalar_features(T, fs):
    B, Cc = 3, 7
    x1, x2 = signals(B, Cc, T, fs, 500 + T)
    xb, ph, stats, spec, nbin = analytic(x1, x2, T, fs, O.SCALAR_BANDS)
    lo, hi = bands(O.SCALAR_BANDS)
    feats = torch.full((B, 64), float("nan"), device=DEV)
    call("eg_ibs_scalar", ptr(xb), ptr(ph), ptr(spec), ptr(feats), B, Cc, T, fs, nbin, CT.addressof(lo), CT.addressof(hi), 4, 0,
         4, 64, 0)
    torch.cuda.synchronize()
    ref = O.ibs_scalar_features(x1, x2, O.ModelCfg(in_channels=Cc, sampling_rate=fs)).numpy()
    got = feats.cpu().numpy()[:, :28]
    d = np.abs(got - ref)
    flip = np.isin(np.arange(28) % 7, [1, 2])          # the gates of tests/test_gpu_ops.py's scalar check
    assert d[:, ~flip].max() < 1e-4, d[:, ~flip].max()
    assert d[:, flip].max() < 2e-3


@pytest.mark.parametrize("T", [1000, 1021, 100])
def test_two_runs_are_bit_identical(T):
    B, Cc, fs = 2, 12, 250.0
    x1, x2 = signals(B, Cc, T, fs, 700 + T)
    outs = []
    for _ in range(2):
        xb, ph, stats, spec, nbin = analytic(x1, x2, T, fs, O.ROBUST_BANDS)
        conn = pairs(xb, ph, stats, spec, B, Cc, T, fs, nbin)
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in (xb, ph, stats, spec, conn)])
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------------------
# whole models at the reference dataset's window (A5: S = 138, short attention) and at 2000 samples (S = 200, long attention)
B = 4
# max |dlogit| gates: tests/test_gpu_logits512.py's a5_full gates (f32 2.7e-5, bf16 2.9e-2) -- the path behind the synchrony
# features is the one those gates were measured on
GATE = {"f32": 2.7e-5, "bf16": 2.9e-2}


def build(name, window, fs, dtype):
    fx = json.loads((GOLDEN / "reference_configs.json").read_text())
    cfg = copy.deepcopy(next(e["config"] for e in fx["entries"] if e["name"] == name))
    cfg["data"]["window_size"] = window
    cfg["data"]["sampling_rate"] = fs
    model = TA.build_model(cfg, compute_dtype=dtype)
    ocfg = O.ModelCfg(**{k: getattr(model.cfg, k) for k in O.ModelCfg.__dataclass_fields__})
    assert ocfg.sampling_rate == fs
    sd = O.synthetic_state_dict(ocfg, WEIGHT_SEED)
    model.load_state_dict(sd, strict=True)
    return model.to(DEV), ocfg, sd


MODELS = [(1000, 250, 138, False), (2000, 256, 200, True)]


@pytest.mark.parametrize("window,fs,S,long_attn", MODELS)
def test_a5_connectivity_seen_by_the_hook_matches_the_oracle(window, fs, S, long_attn):
    model, ocfg, sd = build("A5_full_model", window, fs, "f32")
    model.eval()
    x1, x2, labels = randn_windows(B, ocfg.in_channels, window, seed=21, num_classes=ocfg.num_classes)
    seen = []
    model.ibs_matrix_generator.register_forward_hook(lambda m, i, o: seen.append(o.detach().float().cpu().numpy()))
    with torch.no_grad():
        model(x1.to(DEV), x2.to(DEV), labels.to(DEV))
    eng = next(iter(model._engines.values()))
    assert eng.S == S and eng.attn_long == long_attn
    ref = O.ibs_connectivity(x1, x2, ocfg).numpy()
    assert len(seen) == 1 and seen[0].shape == ref.shape
    sign = [i for i, f in enumerate(ocfg.feature_indices) if f in (1, 2)]
    check_conn(seen[0], ref, window, sign)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("window,fs,S,long_attn", MODELS)
def test_a5_logits_match_the_oracle(window, fs, S, long_attn, dtype):
    model, ocfg, sd = build("A5_full_model", window, fs, dtype)
    model.eval()
    x1, x2, labels = randn_windows(B, ocfg.in_channels, window, seed=11, num_classes=ocfg.num_classes)
    ref_conn = O.ibs_connectivity(x1, x2, ocfg)          # the oracle's features: the gate measures the rest of the path
    model.ibs_matrix_generator.register_forward_hook(lambda mod, inp, out: ref_conn.to(out.device, out.dtype))
    with torch.no_grad():
        got = model(x1.to(DEV), x2.to(DEV), labels.to(DEV))["logits"].float().cpu().numpy()
        ref = O.forward(x1, x2, sd, ocfg, labels)["logits"].numpy()
    err = float(np.abs(got - ref).max())
    print(f"A5 window {window} fs {fs} {dtype}: max|dlogit| = {err:.3e}")
    assert err <= GATE[dtype], err
    if dtype == "f32":
        assert (got.argmax(-1) == ref.argmax(-1)).all()


@pytest.mark.parametrize("window,fs,S,long_attn", MODELS)
def test_a5_f32_training_step_gradients_match_oracle_autograd(window, fs, S, long_attn):
    """against float64 oracle autograd on the same (oracle) synchrony features; only the model's parameters take a gradient --
    spectrogram_generator.window is a buffer (D:66), and an f32 oracle's own gradient of it is 1.3e-3 off the f64 one here"""
    model, ocfg, sd = build("A5_full_model", window, fs, "f32")
    model.eval()
    x1, x2, labels = randn_windows(B, ocfg.in_channels, window, seed=12, num_classes=ocfg.num_classes)
    ref_conn = O.ibs_connectivity(x1, x2, ocfg)
    model.ibs_matrix_generator.register_forward_hook(lambda mod, inp, out: ref_conn.to(out.device, out.dtype))
    out = model(x1.to(DEV), x2.to(DEV), labels.to(DEV))
    loss = out["loss_ce"] + (out["loss_ibs_cls"] if "loss_ibs_cls" in out else 0.0)
    loss.backward()
    torch.cuda.synchronize()
    fp = model._flat
    names = set(fp.names)
    assert "spectrogram_generator.window" in sd and "spectrogram_generator.window" not in names
    params = {k: v.double().clone().requires_grad_(k in names) for k, v in sd.items()}
    ro = O.forward(x1.double(), x2.double(), params, ocfg, labels, conn_edit=lambda c: ref_conn.double())
    (ro["loss_ce"] + (ro["loss_ibs_cls"] if "loss_ibs_cls" in ro else 0.0)).backward()
    gflat = fp.grad.cpu().double()
    gnorm = float(torch.sqrt(sum((p.grad ** 2).sum() for p in params.values() if p.grad is not None)))
    print(f"A5 window {window}: |grad| / |f64 oracle grad| - 1 = {float(gflat.norm()) / gnorm - 1:.3e}")
    assert abs(float(gflat.norm()) / gnorm - 1) < 1e-3
    worst, worst_n, conv0 = 0.0, None, 0.0
    for n, p in zip(fp.names, fp.params):
        ref = params[n].grad
        if ref is None:
            continue
        g = gflat[fp.offsets[n]: fp.offsets[n] + p.numel()].view(p.shape)
        if float(ref.norm()) < 1e-5 * gnorm:      # k_proj.bias: mathematically zero (soft-max shift invariance)
            assert float(g.norm()) < 1e-4 * gnorm, n
            continue
        rel = float((g - ref).norm() / ref.norm())
        if n.startswith("temporal_conv.convs.0."):
            conv0 = max(conv0, rel)
        elif rel > worst:
            worst, worst_n = rel, n
    print(f"A5 window {window}: worst relative gradient error {worst:.3e} ({worst_n}), conv-0 {conv0:.3e}")
    assert worst < 1e-3, (worst_n, worst)        # tests/test_gpu_long_window.py's A5 gate
    # conv-0's weight / bias gradient at window 1000: measured 5.9e-3 / 1.9e-3 against f64, spread evenly over the 25 taps, the
    # same at 256 Hz and with the oracle's synchrony features in place, so not from the IBS kernels (A1, without IBS, 5.8e-4 at
    # window 1000 against 3.4e-4 at 1024).  DESIGN.md section 8c: the front end's open finding.  2e-4 at window 2000.
    assert conv0 < (1e-2 if window == 1000 else 1e-3), conv0


def test_scalar_ibs_model_logits_at_the_reference_window():
    model, ocfg, sd = build("A3_plus_ibs_scalar", 1000, 250, "f32")
    model.eval()
    x1, x2, labels = randn_windows(B, ocfg.in_channels, 1000, seed=31, num_classes=ocfg.num_classes)
    with torch.no_grad():
        got = model(x1.to(DEV), x2.to(DEV), labels.to(DEV))["logits"].float().cpu().numpy()
        ref = O.forward(x1, x2, sd, ocfg, labels)["logits"].numpy()
    err = float(np.abs(got - ref).max())
    print(f"A3 + scalar IBS window 1000 fs 250 f32: max|dlogit| = {err:.3e}")
    assert err <= GATE["f32"], err
    assert (got.argmax(-1) == ref.argmax(-1)).all()
