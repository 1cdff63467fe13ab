"""The parameter-sized tail of the step.  Every comparison here is BIT equality (pure copies, or sums kept in their order):
  * eg_pack_table_ex modes 9 / 10 (convolution weight layouts, staged through LDS) against the stand-alone pack kernels;
  * a train step on the default pack table (layouts that no route reads are not packed) against the full table;
  * the gain / bias gradients of encoder.norm and cross_attn.norm reduced inside the grouped reduce launch against the
    immediate eg_reduce_partials;
  * eg_grad_sqnorm_clip against eg_grad_sqnorm + eg_clip_coef;
  * eg_reduce_table against eg_reduce_partials, entry by entry."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import DualEEGTransformer, HipAdamW  # noqa: E402
from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd._lib import PackEntryEx, ReduceEntry, StepState, call, ptr  # noqa: E402
from eyegaze_multimodal_amd.engine import _reduce_blocks  # noqa: E402
from oracle import dual_eeg_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
KW = dict(in_channels=8, num_classes=3, max_len=256, use_spectrogram=False, use_ibs=False, use_cross_attention=True)
T = 1024
SENTINEL = 0x7b7b
PAD = 64          # sentinel elements kept on both sides of a destination


def to_dev(ctypes_array):
    return torch.frombuffer(bytearray(bytes(ctypes_array)), dtype=torch.uint8).to(DEV)


# ------------------------------------------------------------------------------------------------------
# 1. pack modes 9 / 10
# ------------------------------------------------------------------------------------------------------
# (N, Cin, k, stride, Cp, Kp): conv-0 at the engine's K0; conv-1; an odd Cin below Cp with a padded row tail; J = 2 with a short
# last phase (k = 7, stride 4: phase 3 has one tap)
CONV_SHAPES = [(256, 8, 25, 4, 8, 256), (256, 256, 25, 4, 256, 6400), (32, 3, 5, 2, 8, 64), (16, 8, 7, 4, 8, 64)]


def pack_one(mode, src, N, Cin, p, need_dst, dtype):
    buf = torch.full((need_dst + 2 * PAD,), SENTINEL, dtype=torch.int16, device=DEV)
    e = PackEntryEx()
    e.src, e.dst, e.rows, e.cols, e.ldd, e.mode, e.blk0, e.nblk = ptr(src), ptr(buf) + 2 * PAD, N, Cin, 0, mode, 0, (need_dst + 1023) // 1024
    e.p0, e.p1, e.p2 = p
    e.src_elems, e.dst_elems = src.numel(), need_dst
    tab = (PackEntryEx * 1)(e)
    total = C.c_int(0)
    call("eg_pack_table_ex_check", C.cast(tab, C.c_void_p), 1, dtype, C.byref(total))
    assert total.value == e.nblk
    dtab = to_dev(tab)
    call("eg_pack_table_ex", ptr(dtab), 1, total.value, dtype, 0)
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("dtype", [L.EG_BF16, L.EG_F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pack_table_conv_modes_equal_the_standalone_kernels(shape, dtype):
    N, Cin, k, s, Cp, Kp = shape
    J = (k + s - 1) // s
    g = torch.Generator().manual_seed(N + Cin + k)
    w = torch.randn(N, Cin, k, generator=g).to(DEV)
    for mode, p, need, ref_call in ((9, (k, Cp, Kp), N * Kp, ("eg_pack_conv_weight", N, Cin, k, Cp, Kp)),
                                    (10, (k, s, J), s * Cin * J * N, ("eg_pack_convT_weight", N, Cin, k, s))):
        ref = torch.full((need,), SENTINEL, dtype=torch.int16, device=DEV)
        call(ref_call[0], ptr(w), ptr(ref), *ref_call[1:], dtype, 0)
        got = pack_one(mode, w, N, Cin, p, need, dtype)
        assert torch.equal(got[PAD:PAD + need], ref), (mode, int((got[PAD:PAD + need] != ref).sum()))
        assert int((ref == SENTINEL).sum()) == 0                    # the reference wrote its whole extent (zero padding included)
        assert bool((got[:PAD] == SENTINEL).all()) and bool((got[PAD + need:] == SENTINEL).all()), mode   # nothing outside it


# ------------------------------------------------------------------------------------------------------
# engines
# ------------------------------------------------------------------------------------------------------
def build(B, dtype="bf16", seed=11):
    cfg = O.ModelCfg(**KW)
    model = DualEEGTransformer(**KW, compute_dtype=dtype)
    model.load_state_dict(O.synthetic_state_dict(cfg, seed=7))
    model = model.to(DEV)
    g = torch.Generator().manual_seed(seed + B)
    x1, x2 = torch.randn(B, 8, T, generator=g).to(DEV), torch.randn(B, 8, T, generator=g).to(DEV)
    labels = torch.randint(0, 3, (B,), generator=g).to(DEV)
    return model, model.engine(B, T, DEV), x1, x2, labels


# ------------------------------------------------------------------------------------------------------
# 2. dropped layouts
# ------------------------------------------------------------------------------------------------------
def test_train_step_never_reads_the_dropped_layouts():
    results = []
    for full in (False, True):
        model, eng, x1, x2, labels = build(4)
        assert eng.fuse_ffn and eng.attn_block and eng.ln_proj and eng.pack_unused is False
        eng.pack_unused = full
        if not full:
            for l in range(eng.cfg.num_layers):
                for n in ("w1", "w2", "w1T", "w2T", "qkv", "o", "oT"):
                    eng.w[f"{n}{l}"].fill_(float("nan"))
        opt = HipAdamW(model)
        opt.begin_step(eng, seed=21)
        eng.forward(x1, x2, labels, train=True)
        eng.backward(gloss=torch.ones(1, device=DEV))
        grad = model._flat.grad.clone()
        opt.step(eng)
        torch.cuda.synchronize()
        if not full:        # still NaN: the short table does not write them either
            assert all(bool(torch.isnan(eng.w[f"{n}{l}"].float()).all()) for l in range(eng.cfg.num_layers) for n in ("w1", "oT", "qkv"))
        else:
            assert all(bool(torch.isfinite(eng.w[f"{n}{l}"].float()).all()) for l in range(eng.cfg.num_layers) for n in ("w1", "oT", "qkv"))
        results.append(dict(loss=eng.a["loss"].clone(), logits=eng.a["logits"].clone(), grad=grad, flat=model._flat.flat.clone()))
    short, full = results
    for n in short:
        assert bool(torch.isfinite(short[n]).all()), n
        assert torch.equal(short[n], full[n]), (n, float((short[n] - full[n]).abs().max()))
    assert float(short["grad"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------
# 3. deferred norm partials
# ------------------------------------------------------------------------------------------------------
NORMS = ("encoder.norm.weight", "encoder.norm.bias", "cross_attn.norm.weight", "cross_attn.norm.bias")


@pytest.mark.parametrize("B", [4, 32])
def test_deferred_norm_partials_equal_the_immediate_reduce(B, monkeypatch):
    model, eng, x1, x2, labels = build(B)
    eng.GROUP_MIN_ROWS = 0            # the grouped plan at these small row counts
    fp = model._flat
    one = torch.ones(1, device=DEV)
    numel = dict(zip(fp.names, (p.numel() for p in fp.params)))
    sl = lambda n: slice(fp.offsets[n], fp.offsets[n] + numel[n])

    def run(on_segment):
        names = []
        real = L.call

        def rec(name, *args):
            names.append(name)
            return real(name, *args)
        fp.grad.fill_(7.0)
        eng.set_state(seed=5, lr=0.0, step=1)
        eng.forward(x1, x2, labels, train=True)
        with monkeypatch.context() as m:
            m.setattr("eyegaze_multimodal_amd.engine.call", rec)
            eng.backward(gloss=one, on_segment=on_segment)
        torch.cuda.synchronize()
        return fp.grad.clone(), names

    deferred, calls_d = run(None)
    assert eng._wgrad_group_plan() is not None and eng._wg_plan["whole_norms"] is not None
    assert set(eng._ln_slot) >= {"encoder.norm", "cross_attn.norm"}
    seen = {}
    hook = lambda name: seen.setdefault(name, fp.grad.clone())
    # (a) a listener, the grouped launch in one piece: only the two norms take another route, so EVERY gradient is the same
    monkeypatch.setenv("EYEGAZE_WGRAD_PIECES", "0")
    immediate, calls_i = run(hook)
    assert calls_d.count("eg_reduce_partials") == calls_i.count("eg_reduce_partials") - 2
    assert calls_d.count("eg_reduce_table") == calls_i.count("eg_reduce_table") == 1
    assert torch.equal(deferred, immediate), float((deferred - immediate).abs().max())
    for n in NORMS:
        assert bool((deferred[sl(n)] != 7.0).all()) and bool(torch.isfinite(deferred[sl(n)]).all()), n
        assert float(deferred[sl(n)].abs().max()) > 0
    # the encoder.norm gradients are complete when the segment is announced
    for n in NORMS[:2]:
        assert torch.equal(seen["encoder.norm"][sl(n)], deferred[sl(n)]), n
    # (b) a listener with the launch cut in two pieces (the data-parallel arrangement): the norms are reduced at once as well
    monkeypatch.delenv("EYEGAZE_WGRAD_PIECES")
    seen.clear()
    pieced, calls_p = run(hook)
    assert calls_p.count("eg_reduce_table") == 2
    for n in NORMS:
        assert torch.equal(pieced[sl(n)], deferred[sl(n)]), n
    for n in NORMS[:2]:
        assert torch.equal(seen["encoder.norm"][sl(n)], deferred[sl(n)]), n
    for n in NORMS[2:]:
        assert torch.equal(seen["cross"][sl(n)], deferred[sl(n)]), n


# ------------------------------------------------------------------------------------------------------
# 4. eg_grad_sqnorm_clip
# ------------------------------------------------------------------------------------------------------
def dev_state(grad_scale=1.0, scaler_on=0, loss_scale=1.0):
    st = StepState()
    st.lr, st.bias_corr1, st.bias_corr2, st.grad_scale, st.clip_coef = 1e-3, 0.1, 0.001, grad_scale, 1.0
    st.loss_scale, st.scaler_on = loss_scale, scaler_on
    host = torch.zeros(L.STATE_WORDS, dtype=torch.int32)
    C.memmove(host.data_ptr(), C.addressof(st), C.sizeof(st))
    return host.to(DEV)


SQ_SIZES = [5, 4096, 7_150_001]
_grads = {}


def grad_vector(n):
    if n not in _grads:
        _grads[n] = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.05).to(DEV)
    return _grads[n]


def both_routes(g, nblk, max_norm, **state):
    n = g.numel()
    p_ref, p_got = torch.full((nblk,), 7.0, device=DEV), torch.full((nblk,), 7.0, device=DEV)
    s_ref, s_got = dev_state(**state), dev_state(**state)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    call("eg_grad_sqnorm", ptr(g), n, ptr(p_ref), nblk, 0)
    call("eg_clip_coef", ptr(p_ref), nblk, max_norm, ptr(s_ref), 0)
    for _ in range(2):                 # back to back: the launch must leave its counter at zero
        s_got.copy_(dev_state(**state))
        p_got.fill_(7.0)
        call("eg_grad_sqnorm_clip", ptr(g), n, ptr(p_got), nblk, max_norm, ptr(s_got), ptr(ctr), 0)
        torch.cuda.synchronize()
        assert int(ctr) == 0
        assert torch.equal(p_got.view(torch.int32), p_ref.view(torch.int32))
        assert torch.equal(s_got, s_ref), (s_got.tolist(), s_ref.tolist())      # every word of the state, bit for bit
    st = StepState()
    C.memmove(C.addressof(st), s_got.cpu().data_ptr(), C.sizeof(st))
    return st


@pytest.mark.parametrize("max_norm", [0.0, 1.0])
@pytest.mark.parametrize("nblk", [1, 64, 1024])
@pytest.mark.parametrize("n", SQ_SIZES)
def test_sqnorm_clip_equals_the_two_launches(n, nblk, max_norm):
    g = grad_vector(n)
    st = both_routes(g, nblk, max_norm)
    want = float(g.double().pow(2).sum().sqrt())
    # one block (nblk = 1) adds n / 1024 <= 6983 squares per lane in fp32, one after the other: at most 6983 * 2^-24 = 4.2e-4 of
    # the sum, half of that on the norm; the tree above the lanes adds a few ulp
    assert abs(st.grad_norm - want) <= 2.5e-4 * want and st.found_inf == 0
    assert st.clip_coef == 1.0 if max_norm == 0.0 else 0.0 < st.clip_coef <= 1.0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("n", SQ_SIZES)
def test_sqnorm_clip_flags_an_overflow_like_the_two_launches(n, bad):
    g = grad_vector(n).clone()
    g[n // 2] = bad
    st = both_routes(g, 64, 1.0, scaler_on=1, loss_scale=1024.0)
    assert st.found_inf == 1
    st = both_routes(grad_vector(n), 64, 1.0, scaler_on=1, loss_scale=1024.0)
    assert st.found_inf == 0 and st.grad_norm > 0


def test_optimizer_step_on_the_one_launch_route_keeps_the_parameters():
    finals = []
    for fused in (False, True):
        model, eng, x1, x2, labels = build(4)
        eng.fused_norm_clip = fused
        opt = HipAdamW(model)
        for i in range(2):
            opt.begin_step(eng, seed=100 + i)
            eng.forward(x1, x2, labels, train=True)
            eng.backward(gloss=torch.ones(1, device=DEV))
            opt.step(eng)
        torch.cuda.synchronize()
        finals.append((model._flat.flat.clone(), eng.state_dev.clone()))
    assert torch.equal(finals[0][0], finals[1][0]) and torch.equal(finals[0][1], finals[1][1])


# ------------------------------------------------------------------------------------------------------
# 5. eg_reduce_table against eg_reduce_partials
# ------------------------------------------------------------------------------------------------------
def test_reduce_table_equals_reduce_partials_entry_by_entry():
    g = torch.Generator().manual_seed(9)
    specs = [(256 * 256 + 256, 3), (512, 1024), (8, 2)]        # (n floats, splits): a weight | bias slab, LayerNorm partials, a stub
    parts = [torch.randn(s, n + 12, generator=g).to(DEV) for n, s in specs]                 # stride > n
    outs = [torch.full((n + 4,), 7.0, device=DEV) for n, _ in specs]
    refs = [torch.full((n + 4,), 7.0, device=DEV) for n, _ in specs]
    tab = (ReduceEntry * len(specs))()
    blk = 0
    for e, (n, s), p, o in zip(tab, specs, parts, outs):
        e.partial, e.out, e.n, e.stride, e.splits, e.blk0 = ptr(p), ptr(o), n, n + 12, s, blk
        blk += _reduce_blocks(n, s)
    dtab = to_dev(tab)
    call("eg_reduce_table", ptr(dtab), len(specs), blk, 0)
    for (n, s), p, r in zip(specs, parts, refs):
        call("eg_reduce_partials", ptr(p), ptr(r), n, s, n + 12, 0, 0)
    torch.cuda.synchronize()
    for (n, s), p, o, r in zip(specs, parts, outs, refs):
        assert torch.equal(o.view(torch.int32), r.view(torch.int32)), (n, s, float((o - r).abs().max()))
        assert float(o[n:].min()) == 7.0 and float(o[:n].abs().max()) > 0
        if s == 3:      # per element slab 0 + slab 1 + slab 2, in this order
            assert torch.equal(o[:n], (p[0, :n] + p[1, :n]) + p[2, :n])
