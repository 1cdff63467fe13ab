"""GPU: gradient accumulation -- one optimiser step from several micro-batches.
  1. eg_grad_accumulate against torch.add (bit equality), its fused norm partials through eg_clip_coef;
  2. k repeats of one micro-batch step the parameters to the very bits of the k = 1 step (acc = k*g and 1/k are exact);
  3. an accumulated f32 step against the CPU oracle's gradient of the concatenated batch and its clip + AdamW;
  4. the trainer: k = 1 launches nothing new and allocates nothing; k = 3 over 7 micro-batches steps after 3, 6 and in flush();
  5. fp16: an overflow in one micro-step skips the whole update with ONE back-off;
  6. two ranks x k = 2 on one card equal one process x k = 4."""
import ctypes as C
import json
import math
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import HipAdamW  # noqa: E402
from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd import engine as E  # noqa: E402
from eyegaze_multimodal_amd._lib import StepState, call, ptr  # noqa: E402
from eyegaze_multimodal_amd.data import randn_windows  # noqa: E402
from oracle import dual_eeg_oracle as O  # noqa: E402
from tests.helpers import t  # noqa: E402
from tests.test_gpu_model import DEV, build  # noqa: E402

REPO = Path(__file__).resolve().parent.parent


def dev_state(grad_scale=1.0, scaler_on=0, loss_scale=1.0):
    st = StepState()
    st.lr, st.bias_corr1, st.bias_corr2, st.grad_scale, st.clip_coef = 1e-3, 0.1, 0.001, grad_scale, 1.0
    st.loss_scale, st.scaler_on = loss_scale, scaler_on
    host = torch.zeros(L.STATE_WORDS, dtype=torch.int32)
    C.memmove(host.data_ptr(), C.addressof(st), C.sizeof(st))
    return host.to(DEV)


def read_state(ten):
    st = StepState()
    h = ten.cpu()
    C.memmove(C.addressof(st), h.data_ptr(), C.sizeof(st))
    return st


# ------------------------------------------------------------------------------------------------------
# 1. kernel against torch
# ------------------------------------------------------------------------------------------------------
SIZES = [4, 252, 1024, 4100, 1_000_004]       # one lane; short of one block; exactly one block; blocks + a tail; grid-stride trips


def _pair(n, seed=0):
    g = torch.Generator().manual_seed(seed + n)
    a = (torch.randn(n, generator=g) * torch.exp(4 * torch.randn(n, generator=g))).to(DEV)      # wide range of exponents
    b = (torch.randn(n, generator=g) * torch.exp(4 * torch.randn(n, generator=g))).to(DEV)
    return a, b


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nblk", [0, 64, 1024])
def test_accumulate_equals_torch_add_bit_for_bit(n, nblk):
    a, g = _pair(n)
    acc = a.clone()
    part = torch.full((max(nblk, 1),), float("nan"), device=DEV)
    call("eg_grad_accumulate", ptr(acc), ptr(g), n, 0, ptr(part) if nblk else 0, nblk, 0)
    torch.cuda.synchronize()
    want = torch.add(a, g)
    assert torch.equal(acc, want)
    if nblk:
        assert torch.isfinite(part).all()                       # every one of the nblk entries is written
        st = dev_state()
        call("eg_clip_coef", ptr(part), nblk, 1.0, ptr(st), 0)
        torch.cuda.synchronize()
        ref = float(want.double().norm())
        got = read_state(st).grad_norm
        print(f"n={n} nblk={nblk} grad_norm {got!r} float64 {ref!r} rel {abs(got - ref) / ref:.3e}")
        assert abs(got - ref) < 1e-4 * ref


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nblk", [0, 64, 1024])
def test_first_overwrites_a_poisoned_accumulator(n, nblk):
    _, g = _pair(n, seed=1)
    acc = torch.full((n,), float("nan"), device=DEV)
    part = torch.full((max(nblk, 1),), float("nan"), device=DEV)
    call("eg_grad_accumulate", ptr(acc), ptr(g), n, 1, ptr(part) if nblk else 0, nblk, 0)
    torch.cuda.synchronize()
    assert torch.equal(acc, g)
    if nblk:
        ref = float((g.double() ** 2).sum())
        assert torch.isfinite(part).all() and abs(float(part.double().sum()) - ref) < 1e-5 * ref


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("first", [0, 1])
def test_sub_range_leaves_its_neighbours_alone(n, first):
    """a bucket range: 12 floats into larger buffers, sentinels on both sides of the accumulator"""
    off, tail, sent = 12, 20, -7.25
    a, g = _pair(n, seed=2)
    big_acc = torch.full((off + n + tail,), sent, device=DEV)
    big_g = torch.full((off + n + tail,), 3.5, device=DEV)
    big_acc[off:off + n] = a
    big_g[off:off + n] = g
    part = torch.full((64,), float("nan"), device=DEV)
    call("eg_grad_accumulate", ptr(big_acc) + 4 * off, ptr(big_g) + 4 * off, n, first, ptr(part), 64, 0)
    torch.cuda.synchronize()
    assert torch.equal(big_acc[off:off + n], g if first else a + g)
    assert bool((big_acc[:off] == sent).all()) and bool((big_acc[off + n:] == sent).all())
    assert bool((big_g == torch.cat([torch.full((off,), 3.5, device=DEV), g, torch.full((tail,), 3.5, device=DEV)])).all())


@pytest.mark.parametrize("n", [4, 4100])
def test_one_infinity_reaches_found_inf(n):
    a, g = _pair(n, seed=3)
    g[n // 2] = float("inf")
    part = torch.zeros(64, device=DEV)
    call("eg_grad_accumulate", ptr(a), ptr(g), n, 0, ptr(part), 64, 0)
    st = dev_state(scaler_on=1, loss_scale=1024.0)
    call("eg_clip_coef", ptr(part), 64, 1.0, ptr(st), 0)
    torch.cuda.synchronize()
    assert math.isinf(float(a[n // 2])) and read_state(st).found_inf == 1


# ------------------------------------------------------------------------------------------------------
# 2. exactness: the same micro-batch k times
# ------------------------------------------------------------------------------------------------------
def _fixture_batch(z):
    return t(z["randn/eeg1"]).to(DEV), t(z["randn/eeg2"]).to(DEV), t(z["labels"]).to(DEV)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("k", [2, 4])
def test_repeated_micro_batch_steps_to_the_same_bits(dtype, k):
    """acc = k*g exactly (k a power of two; for k = 4 the one inexact partial sum 3g still rounds 3g + g to 4g) and
    grad_scale = 1/k is a power of two, so with the clip out of the way (coefficient exactly 1) AdamW sees the k = 1 gradients"""
    one = torch.ones(1, device=DEV)
    res = []
    for accumulate in (False, True):
        z, kw, cfg, sd, model = build("tiny_a1", dtype)
        model.eval()                                            # no dropout: every micro-step yields the same gradient
        x1, x2, labels = _fixture_batch(z)
        assert x1.shape[0] == 4
        eng = model.engine(4, x1.shape[2], torch.device(DEV))
        opt = HipAdamW(model, lr=1e-3, weight_decay=0.01, max_grad_norm=1e30)
        if not accumulate:
            opt.begin_step(eng, seed=1)
            eng.forward(x1, x2, labels, train=False)
            eng.backward(gloss=one)
            opt.step(eng)
            assert model._flat.acc is None
        else:
            for j in range(k):
                opt.begin_step(eng, seed=1 + j, grad_scale=1.0 / (j + 1), advance=(j == 0))
                eng.forward(x1, x2, labels, train=False)
                eng.backward(gloss=one)
                eng.accumulate(first=(j == 0), norm=(j == k - 1))
            torch.cuda.synchronize()
            assert torch.equal(model._flat.acc, k * model._flat.grad)
            opt.step(eng, accumulated=True, norm_ready=True)
        torch.cuda.synchronize()
        st = eng.read_state()
        assert opt.t == 1 and st.clip_coef == 1.0
        res.append((model._flat.flat.clone(), opt.m.clone(), opt.v.clone(), st.grad_norm, float(sd[next(iter(sd))].abs().sum())))
    (p1, m1, v1, n1, _), (pk, mk, vk, nk, _) = res
    assert torch.equal(m1, mk) and torch.equal(v1, vk)
    assert torch.equal(p1, pk)
    assert abs(n1 - nk) <= 1e-5 * n1                            # two summation orders of the same squares
    assert not torch.equal(p1, torch.zeros_like(p1))


# ------------------------------------------------------------------------------------------------------
# 3. accumulated step against the oracle (f32)
# ------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_8(name):
    """oracle gradients of the 8-sample batch (loss_ce, mean over 8), computed once per configuration and never modified"""
    if name not in _ORACLE:
        z, kw, cfg, sd, _ = build(name, "f32")
        x1, x2, y = randn_windows(8, cfg.in_channels, 1024, seed=11, num_classes=cfg.num_classes)
        P = {k_: v.clone().requires_grad_(True) for k_, v in sd.items()}
        out = O.forward(x1, x2, P, cfg, y)
        out["loss_ce"].backward()
        grads = {k_: (p.grad.detach().clone() if p.grad is not None else None) for k_, p in P.items()}
        _ORACLE[name] = (x1, x2, y, grads)
    return _ORACLE[name]


@pytest.mark.parametrize("name", ["tiny_a1", "cfg3_xattn"])
def test_accumulated_step_matches_the_oracle_on_the_whole_batch(name):
    x1, x2, y, ref = _oracle_8(name)
    z, kw, cfg, sd, model = build(name, "f32")
    model.eval()
    dev = torch.device(DEV)
    eng = model.engine(4, 1024, dev)
    lr = 1e-3
    opt = HipAdamW(model, lr=lr, weight_decay=0.01)
    one = torch.ones(1, device=DEV)
    fp = model._flat
    start = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    for j in range(2):
        sl = slice(4 * j, 4 * j + 4)
        opt.begin_step(eng, seed=3 + j, grad_scale=1.0 / (j + 1), advance=(j == 0))
        eng.forward(x1[sl].to(DEV), x2[sl].to(DEV), y[sl].to(DEV), train=False)
        eng.backward(gloss=one)
        eng.accumulate(first=(j == 0), norm=(j == 1))
    torch.cuda.synchronize()
    acc = fp.acc.cpu().clone()
    opt.step(eng, accumulated=True, norm_ready=True)
    torch.cuda.synchronize()
    st = eng.read_state()
    assert opt.t == 1 and st.grad_scale == 0.5
    got = {n: (0.5 * acc[fp.offsets[n]:fp.offsets[n] + p.numel()]).view(p.shape) for n, p in zip(fp.names, fp.params)}
    gscale = math.sqrt(sum(float((g.double() ** 2).sum()) for g in ref.values() if g is not None))
    worst = 0.0
    for n, g in got.items():
        r = ref[n] if ref[n] is not None else torch.zeros_like(g)
        rn, gn = float(r.double().norm()), float(g.double().norm())
        worst = max(worst, abs(gn - rn) / (2 * 1e-3 * rn + 1e-6 * gscale))
        assert abs(gn - rn) <= 2 * 1e-3 * rn + 1e-6 * gscale, (n, gn, rn)
        # direction too (a norm alone would accept a permuted tensor): that test's full-tensor gate, 1e-3 relative, with its
        # 1e-5 * global floor for the mathematically-zero k_proj.bias gradients
        diff = float((g.double() - r.double()).norm())
        assert diff <= 1e-3 * rn + 1e-5 * gscale, (n, diff, rn)
    print(f"{name}: worst norm-gate use {worst:.3f}; grad_norm hip {st.grad_norm!r} oracle {gscale!r}")
    assert abs(st.grad_norm - gscale) <= 1e-3 * gscale
    # parameters: the oracle's clip + AdamW applied on the CPU to the downloaded HIP accumulator
    P = {n: v.clone() for n, v in start.items()}
    O.clip_and_adamw(P, {n: got[n].clone() for n in P}, {}, step=1, lr=lr, wd=0.01)
    for n, p in model.named_parameters():
        torch.testing.assert_close(p.detach().cpu(), P[n], rtol=1e-5, atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")


# ------------------------------------------------------------------------------------------------------
# 4. trainer
# ------------------------------------------------------------------------------------------------------
@pytest.fixture
def recorded_calls(monkeypatch):
    names = []
    real = L.call

    def rec(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(L, "call", rec)
    monkeypatch.setattr(E, "call", rec)
    return names


def _trainer(tmp_path, route, **training):
    from eyegaze_multimodal_amd.train_art import Trainer
    from tests.test_gpu_train import make_config
    over = dict(training)
    if route == "aux":
        over["use_sym_loss"] = True
    cfg = make_config(tmp_path, model={"num_layers": 2}, training=over)
    tr = Trainer(cfg, torch.device(DEV))
    assert any(tr.aux.values()) == (route == "aux")
    return tr


@pytest.mark.parametrize("route", ["operator", "aux"])
@pytest.mark.parametrize("key", ["absent", "one"])
def test_trainer_without_accumulation_is_todays_step(tmp_path, recorded_calls, route, key):
    tr = _trainer(tmp_path, route, **({} if key == "absent" else {"gradient_accumulation_steps": 1}))
    x1, x2, y = randn_windows(8, 8, 1024, seed=4)
    seed0 = tr.config["system"]["seed"] * 7919
    for i in range(2):
        tr.train_step(x1.to(DEV), x2.to(DEV), y.to(DEV))
        torch.cuda.synchronize()
        stt = tr._last_eng.read_state()
        want = E.scramble_seed(seed0 + (i + 1))                 # the seed of step_no = i + 1, as before
        assert (stt.seed_lo, stt.seed_hi) == (want & 0xFFFFFFFF, (want >> 32) & 0xFFFFFFFF)
    assert tr.flush() is False
    assert "eg_grad_accumulate" not in recorded_calls
    assert recorded_calls.count("eg_grad_sqnorm") == 2 and recorded_calls.count("eg_adamw") == 2
    assert tr.model._flat.acc is None and tr.opt.t == 2 and tr.step_no == 2


@pytest.mark.parametrize("route", ["operator", "aux"])
def test_trainer_k3_over_seven_micro_batches(tmp_path, recorded_calls, route):
    tr = _trainer(tmp_path, route, gradient_accumulation_steps=3)
    x1, x2, y = randn_windows(8, 8, 1024, seed=4)
    x1, x2, y = x1.to(DEV), x2.to(DEV), y.to(DEV)
    fp = None
    steps, scales, seeds, losses, changed = [], [], [], [], []
    prev = None
    for i in range(7):
        out = tr.train_step(x1, x2, y)                          # the same batch every time: only the dropout masks differ
        torch.cuda.synchronize()
        fp = tr.model._flat
        cur = fp.flat.clone()
        changed.append(prev is not None and not torch.equal(cur, prev))
        prev = cur
        stt = tr._last_eng.read_state()
        steps.append((tr.step_no, tr.opt.t, recorded_calls.count("eg_adamw")))
        scales.append(stt.grad_scale)
        seeds.append((stt.seed_lo, stt.seed_hi))
        losses.append({k_: float(v) for k_, v in out.items()})
    assert [s[0] for s in steps] == [0, 0, 1, 1, 1, 2, 2]       # optimiser steps after calls 3 and 6
    assert [s[2] for s in steps] == [0, 0, 1, 1, 1, 2, 2]
    assert [s[1] for s in steps] == [1, 1, 1, 2, 2, 2, 3]       # t belongs to the group: the bias corrections follow it
    assert changed == [False, False, True, False, False, True, False]
    np.testing.assert_allclose(scales, [1, 1 / 2, 1 / 3, 1, 1 / 2, 1 / 3, 1], rtol=1e-7)
    assert tr.pending == 1
    assert tr.flush() is True                                   # the third step: one micro-batch, divisor 1
    torch.cuda.synchronize()
    assert tr.pending == 0 and tr.step_no == 3 and tr.opt.t == 3 and recorded_calls.count("eg_adamw") == 3
    assert tr._last_eng.read_state().grad_scale == 1.0
    assert not torch.equal(fp.flat, prev)
    assert tr.flush() is False
    assert all(np.isfinite(list(l.values())).all() for l in losses), losses
    assert len(set(seeds)) == 7                                 # every micro-step publishes its own dropout seed ...
    assert losses[0]["loss_ce"] != losses[1]["loss_ce"]         # ... and draws other masks: same batch, same parameters
    assert recorded_calls.count("eg_grad_accumulate") == 7
    assert recorded_calls.count("eg_grad_sqnorm") == 1          # full groups take the fused partials; only the flush re-reads


# ------------------------------------------------------------------------------------------------------
# 5. fp16 overflow
# ------------------------------------------------------------------------------------------------------
def test_fp16_overflow_in_one_micro_step_skips_the_group_with_one_back_off():
    z, kw, cfg, sd, model = build("tiny_a1", "fp16")
    model.eval()
    x1, x2, labels = _fixture_batch(z)
    eng = model.engine(x1.shape[0], x1.shape[2], torch.device(DEV))
    eng.reset_scaler(init_scale=2.0 ** 40, growth=2.0, backoff=0.5, growth_interval=1000)     # certain overflow in fp16
    opt = HipAdamW(model, lr=1e-3)
    one = torch.ones(1, device=DEV)
    seed = [0]

    def group(boost=None):
        """k = 2; boost: factor on the loss gradient of the SECOND micro-step only"""
        for j in range(2):
            seed[0] += 1
            opt.begin_step(eng, seed=seed[0], grad_scale=1.0 / (j + 1), advance=(j == 0))
            eng.forward(x1, x2, labels, train=False)
            eng.backward(gloss=(one * boost if (boost and j == 1) else one))
            eng.accumulate(first=(j == 0), norm=(j == 1))
        opt.step(eng, accumulated=True, norm_ready=True)
        torch.cuda.synchronize()
        return eng.read_state()
    before = model._flat.flat.clone()
    s = group()
    assert s.found_inf == 1 and s.skipped == 1 and s.opt_steps == 0
    assert s.loss_scale == 2.0 ** 39                            # backed off once for the group, not once per micro-step
    assert torch.equal(model._flat.flat, before)
    skipped = 1
    for _ in range(40):                                         # the scale keeps halving until both micro-steps fit
        s = group()
        if s.found_inf == 0:
            break
        skipped += 1
        assert torch.equal(model._flat.flat, before)
    assert s.found_inf == 0 and s.skipped == skipped and s.opt_steps == 1 and s.loss_scale == 2.0 ** (40 - skipped)
    after = model._flat.flat.clone()
    assert not torch.equal(after, before)
    # now only ONE micro-step of the group overflows (backward is linear in the loss gradient and twice this scale overflowed):
    # its inf / NaN reach the accumulator, the accumulated norm is not finite, the whole update is skipped
    s = group(boost=2.0 ** 20)
    assert not torch.isfinite(model._flat.acc).all()
    assert s.found_inf == 1 and s.skipped == skipped + 1 and s.opt_steps == 1 and s.loss_scale == 2.0 ** (39 - skipped)
    assert torch.equal(model._flat.flat, after)
    s = group()                                                 # the next group steps
    assert s.found_inf == 0 and s.opt_steps == 2 and s.skipped == skipped + 1 and not torch.equal(model._flat.flat, after)


# ------------------------------------------------------------------------------------------------------
# 6. two ranks on one GPU
# ------------------------------------------------------------------------------------------------------
def test_two_ranks_k2_equal_one_process_k4(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(REPO / "tests" / "ddp_accum_gpu_worker.py"), str(tmp_path)]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(REPO), timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    r0 = json.loads((tmp_path / "rank0.json").read_text())
    r1 = json.loads((tmp_path / "rank1.json").read_text())
    print(r0)
    assert r0["same_params_as_rank0"] and r1["same_params_as_rank0"]
    assert r0["moved"] > 1e-4                                    # the optimiser really stepped
    assert r0["opt_t"] == 1 and r1["opt_t"] == 1
    for r in (r0, r1):
        assert r["collectives_before_last_micro_step"] == 0     # non-final micro-steps issue no collective
        assert r["collectives"] == 8                            # one per bucket, as one plain step: not k times that
    assert r0["grad_rel_err"] < 2e-5, r0                         # the gates of tests/test_gpu_ddp.py
    assert r0["param_rel_err_after_1_update"] < 2e-3, r0
