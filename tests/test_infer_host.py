"""CPU-only: the host side of the forward-only route.  The lean forms of eg_attn_block_fwd / eg_ffn_chain are requested by null
pointers; every partial combination is refused before any launch with the rule in the message, and a bad dtype is still reported
first.  eg_eval_accumulate's argument checks, and the confusion-matrix form of the macro metrics.  Nothing is launched: every call
here is refused by a host check, so the addresses only have to be non-null and aligned."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from eyegaze_multimodal_amd import _lib as L
from eyegaze_multimodal_amd import train_art as TA

BUF = torch.zeros(4096, dtype=torch.float32)      # host memory: its address stands in for every operand
P = BUF.data_ptr()
STORED = ("qkv", "ctx", "lse", "r1")


def attn_desc(stored=(), ln_out=True, dtype=L.EG_BF16):
    d = L.AttnBlockDesc()
    d.x = d.wqkv_frag = d.wo_frag = d.bqkv = d.bo = P
    d.NB, d.S, d.d_model, d.num_heads, d.dtype = 2, 65, 256, 8, dtype
    for n in stored:
        setattr(d, n, P)
    if ln_out:
        d.ln_gamma = d.ln_beta = d.ln_out = P
    return d


@pytest.mark.parametrize("stored", [s for r in (1, 2, 3) for s in itertools.combinations(STORED, r)], ids="+".join)
def test_attention_block_refuses_some_but_not_all_stored_results(stored):
    with pytest.raises(L.EgError, match=rf"all given \(the keeping form\) or all null \(the lean form, which needs ln_out\); got {len(stored)} of"):
        L.call("eg_attn_block_fwd", C.byref(attn_desc(stored)), 0)


def test_attention_block_lean_form_needs_ln_out():
    with pytest.raises(L.EgError, match="lean form, which needs ln_out.*got 0 of the four, ln_out null"):
        L.call("eg_attn_block_fwd", C.byref(attn_desc((), ln_out=False)), 0)


@pytest.mark.parametrize("stored", [(), ("qkv",), STORED])
def test_attention_block_reports_a_bad_dtype_before_the_null_rule(stored):
    with pytest.raises(L.EgError, match="needs a 16-bit dtype.*got dtype 7"):
        L.call("eg_attn_block_fwd", C.byref(attn_desc(stored, dtype=7)), 0)


def ffn_desc(H=False, Cc=False, dtype=L.EG_BF16, **kw):
    f = L.FfnDesc()
    f.A = f.W1 = f.W2 = f.bias1 = f.bias2 = f.residual = P
    f.lda, f.ldh, f.ldc, f.ldg, f.ldr, f.M, f.F, f.act1, f.dtype = 256, 128, 256, 128, 256, 81, 128, L.ACT_RELU, dtype
    f.ln_gamma = f.ln_beta = f.ln_out = P
    f.H, f.C = (P if H else None), (P if Cc else None)
    for k, v in kw.items():
        setattr(f, k, v)
    return f


@pytest.mark.parametrize("H,Cc,only", [(True, False, "H"), (False, True, "C")])
def test_ffn_chain_refuses_one_of_h_and_c(H, Cc, only):
    with pytest.raises(L.EgError, match=rf"H and C are both given \(the keeping form\) or both null \(the lean form\); got {only} only"):
        L.call("eg_ffn_chain", C.byref(ffn_desc(H, Cc)), 0)


@pytest.mark.parametrize("kw", [dict(bias1=None), dict(act1=L.ACT_NONE), dict(gate=P), dict(gate_bits_in=P)],
                         ids=["no_bias1", "no_relu", "gate", "gate_bits_in"])
def test_lean_ffn_chain_serves_the_forward_form_only(kw):
    with pytest.raises(L.EgError, match="lean form .H and C null. serves the forward form only: bias1, ReLU, no gate, no gate_bits_in"):
        L.call("eg_ffn_chain", C.byref(ffn_desc(**kw)), 0)


def test_lean_ffn_chain_needs_ln_out_and_writes_no_gate_bits():
    with pytest.raises(L.EgError, match="lean form .H and C null. needs ln_out"):
        L.call("eg_ffn_chain", C.byref(ffn_desc(ln_out=None)), 0)
    with pytest.raises(L.EgError, match="lean form .H and C null. writes no gate_bits_out"):
        L.call("eg_ffn_chain", C.byref(ffn_desc(gate_bits_out=P)), 0)


@pytest.mark.parametrize("H,Cc", [(False, False), (True, False), (True, True)])
def test_ffn_chain_reports_a_bad_dtype_before_the_null_rule(H, Cc):
    with pytest.raises(L.EgError, match="16-bit compute dtypes only .got 7."):
        L.call("eg_ffn_chain", C.byref(ffn_desc(H, Cc, dtype=7)), 0)


def test_eval_accumulate_argument_checks():
    for ncls in (0, 17, -1):
        with pytest.raises(L.EgError, match=rf"ncls={ncls} outside \[1, 16\]"):
            L.call("eg_eval_accumulate", P, P, P, P, P, P, 4, ncls, 0)
    for B in (0, -3):
        with pytest.raises(L.EgError, match=f"B={B}"):
            L.call("eg_eval_accumulate", P, P, P, P, P, P, B, 3, 0)
    with pytest.raises(L.EgError, match="null logits or pred"):
        L.call("eg_eval_accumulate", 0, P, P, P, P, P, 4, 3, 0)
    with pytest.raises(L.EgError, match="null logits or pred"):
        L.call("eg_eval_accumulate", P, P, P, 0, P, P, 4, 3, 0)
    with pytest.raises(L.EgError, match="confusion matrix needs labels"):
        L.call("eg_eval_accumulate", P, 0, P, P, P, P, 4, 3, 0)


def confusion(yt, yp, ncls):
    cm = np.zeros((ncls, ncls), np.int64)
    np.add.at(cm, (yt, yp), 1)
    return cm


@pytest.mark.parametrize("seed", range(8))
def test_macro_metrics_from_the_confusion_matrix_equal_the_label_form(seed):
    """including classes that are never predicted, never present, or neither (left out of the macro averages by both forms)"""
    rng = np.random.default_rng(seed)
    n, ncls = int(rng.integers(1, 300)), int(rng.integers(2, 17))
    yt = rng.integers(0, ncls if seed % 3 else max(1, ncls - 2), n)
    yp = rng.integers(0, ncls if seed % 2 else max(1, ncls // 2), n)
    if seed == 5:
        yt[:] = 1
    assert TA.macro_metrics_from_confusion(confusion(yt, yp, ncls)) == TA.macro_metrics(yt, yp)


def test_macro_metrics_from_the_confusion_matrix_reference_known_answer():
    """5_Metrics/classification_metrics.py:436-472, as tests/test_train_host.py: Accuracy 0.8600, F1 (macro) 0.8612"""
    m = TA.macro_metrics_from_confusion(np.array([[30, 2, 1], [5, 30, 1], [3, 2, 26]]))
    assert abs(m["eval/accuracy"] - 0.86) < 1e-12
    assert abs(m["eval/f1"] - 0.8612) < 5e-5


# ---- the inference engine, recorded on the CPU (profiles/tools/launch_trace.py's recorder: launches are listed, not issued) ----
BACKWARD_LAYOUTS = ("qkvT", "oT", "oTf", "w1T", "w2T", "w1Tf", "w2Tf", "conv1T", "sfT", "c0T", "i0T",
                    "spc2T", "spp0T", "spp3T", "ib0T", "ib3T", "ig3T")


def test_the_layout_table_marks_exactly_these_layouts_as_the_backward_s():
    from eyegaze_multimodal_amd import engine as E
    rows = [lay for groups in E.LAYOUTS.values() for group in groups for lay in group]
    assert sorted(lay.key for lay in rows if lay.bwd) == sorted(BACKWARD_LAYOUTS)
    assert len({lay.key for lay in rows}) == len(rows)


def golden_kwargs(name):
    from tests.helpers import load_golden
    return load_golden(name)[1]


def recorded_inference_forward(kw, dtype, B, T):
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "profiles" / "tools"))
    from launch_trace import Recorder
    from eyegaze_multimodal_amd import DualEEGTransformer, engine as E, tokens
    rec = Recorder(L.call)
    saved = [(m, m.call) for m in (E, tokens)]
    for m, _ in saved:
        m.call = rec
    try:
        model = DualEEGTransformer(**kw)
        cpu = torch.device("cpu")
        model._flat.ensure(cpu, need_grad=False)
        eng = E.InferenceEngine(model, B, T, cpu, dtype)
        x, y = torch.zeros(B, model.cfg.in_channels, T), torch.zeros(B, dtype=torch.long)
        eng.forward(x, x, y)
        eng.forward(x, x, y, pack=False)
    finally:
        for m, c in saved:
            m.call = c
    return model, eng, rec.rows, (x, y)


def held_ranges(model, eng, extra):
    held = list(eng.a.values()) + list(eng.sc.values()) + [model._flat.flat, eng.state_dev, eng._plan_dev, *extra]
    held += [b for b in model.buffers()] + [getattr(eng, "_keep", None)]
    out = [(t_.data_ptr(), t_.data_ptr() + t_.numel() * t_.element_size()) for t_ in held if torch.is_tensor(t_) and t_.numel()]
    out += [(v.data_ptr(), v.data_ptr() + v.numel() * v.element_size()) for v in eng.w.values()]
    # the band-edge arrays of the synchrony kernels (ctypes)
    out += [(C.addressof(c), C.addressof(c) + C.sizeof(c)) for c in getattr(eng, "band_edges", ())]
    return out


def pointers_of(arg):
    """the addresses a recorded launch argument carries: a plain int, or the pointer fields of a descriptor passed by reference"""
    if isinstance(arg, int) and not isinstance(arg, bool):
        return [arg] if arg >= (1 << 32) else []
    obj = getattr(arg, "_obj", None)
    if isinstance(obj, C.Structure):
        return [v for n, tp in obj._fields_ if tp is C.c_void_p and (v := getattr(obj, n))]
    return []


INFER_CASES = {
    "cfg3": (lambda: golden_kwargs("cfg3_xattn"), L.EG_BF16, 4, 1024),
    "a5_full": (lambda: golden_kwargs("a5_full"), L.EG_BF16, 4, 1024),
    "long_S257": (lambda: dict(in_channels=8, max_len=512, use_spectrogram=False, use_ibs=False), L.EG_BF16, 2, 4096),
    "f32": (lambda: golden_kwargs("cfg3_xattn"), L.EG_F32, 4, 1024),
}


@pytest.mark.parametrize("case", sorted(INFER_CASES))
def test_inference_engine_launches_stay_inside_what_it_holds(case):
    kw, dtype, B, T = INFER_CASES[case]
    model, eng, rows, inputs = recorded_inference_forward(kw(), dtype, B, T)
    names = [r[0] for r in rows]
    assert "eg_set_step_state" not in names and not [n for n in names if "bwd" in n or n in ("eg_adamw", "eg_gemm_tn", "eg_grad_sqnorm")]
    assert names.count("eg_pack_table_ex" if eng.fused_tail else "eg_pack_table") == 1          # pack=False did not pack again
    assert not [k for k in eng.w if isinstance(k, str) and k.rstrip("0123456789x") in BACKWARD_LAYOUTS]
    assert model._flat.grad is None and not eng.g
    if case == "long_S257":
        assert eng.S == 257 and eng.attn_long
    if case == "cfg3":
        assert {how for _, _, how in eng.routes_taken} == {"lean"} and "hff" not in eng.sc


SMALL_LN_UNFUSED = (lambda: dict(in_channels=8, max_len=256, use_spectrogram=False, use_ibs=False), L.EG_BF16, 4, 1024)


@pytest.mark.parametrize("case", sorted(INFER_CASES) + ["small_ln_unfused"])
def test_inference_forward_issues_the_entry_points_of_an_eval_forward(case, monkeypatch):
    """Engine.forward(train=False) and InferenceEngine.forward call the same entry points in the same order once the pack launches
    (eg_pack*: the inference engine packs fewer layouts, through the same table launch) are set aside"""
    from eyegaze_multimodal_amd import DualEEGTransformer, engine as E, tokens
    if case == "small_ln_unfused":
        monkeypatch.setenv("EYEGAZE_LN_FUSE", "0")
    kw, dtype, B, T = SMALL_LN_UNFUSED if case == "small_ln_unfused" else INFER_CASES[case]
    names = []
    for m in (E, tokens):
        monkeypatch.setattr(m, "call", lambda name, *args: names.append(name) if name != "eg_pack_table_ex_check" else L.call(name, *args))
    issued = {}
    for cls in (E.Engine, E.InferenceEngine):
        model = DualEEGTransformer(**kw())
        cpu = torch.device("cpu")
        model._flat.ensure(cpu, need_grad=cls is E.Engine)
        eng = cls(model, B, T, cpu, dtype)
        assert eng.ln_fuse == (case != "small_ln_unfused")
        x, y = torch.zeros(B, model.cfg.in_channels, T), torch.zeros(B, dtype=torch.long)
        del names[:]
        eng.forward(x, x, y, train=False) if cls is E.Engine else eng.forward(x, x, y)
        issued[cls] = [n for n in names if not n.startswith("eg_pack")]
    assert len(issued[E.Engine]) > 20 and issued[E.InferenceEngine] == issued[E.Engine]


def test_inference_engine_pointers_lie_inside_tensors_it_holds():
    """every address of every launch -- taken from the live argument objects, so descriptor fields count too"""
    from eyegaze_multimodal_amd import DualEEGTransformer, engine as E, tokens
    seen = []
    saved = [(m, m.call) for m in (E, tokens)]
    for m, _ in saved:
        m.call = lambda name, *args: seen.append((name, args)) if name != "eg_pack_table_ex_check" else L.call(name, *args)
    try:
        for case in sorted(INFER_CASES):
            kw, dtype, B, T = INFER_CASES[case]
            model = DualEEGTransformer(**kw())
            cpu = torch.device("cpu")
            model._flat.ensure(cpu, need_grad=False)
            eng = E.InferenceEngine(model, B, T, cpu, dtype)
            x, y = torch.zeros(B, model.cfg.in_channels, T), torch.zeros(B, dtype=torch.long)
            del seen[:]
            eng.forward(x, x, y)
            ranges = held_ranges(model, eng, (x, y))
            assert len(seen) > 20
            for name, args in seen:
                for a in args:
                    for p in pointers_of(a):
                        assert any(lo <= p < hi for lo, hi in ranges), (case, name, hex(p))
    finally:
        for m, c in saved:
            m.call = c


def test_inference_workspace_does_not_grow_with_the_layers():
    from eyegaze_multimodal_amd import DualEEGTransformer, engine as E
    sizes, train = [], []
    for layers in (2, 6):
        model = DualEEGTransformer(**{**golden_kwargs("cfg3_xattn"), "num_layers": layers})
        sizes.append(E.inference_workspace_bytes(model.cfg, 256, 1024, L.EG_BF16))
        cpu = torch.device("cpu")
        model._flat.ensure(cpu)
        eng = E.Engine(model, 4, 1024, cpu, L.EG_BF16, state_dev=torch.zeros(L.STATE_WORDS, dtype=torch.int32))
        train.append(sum(v.numel() * v.element_size() for v in eng.a.values()))
        inf = E.InferenceEngine(model, 4, 1024, cpu, L.EG_BF16)
        own = sum(v.numel() * v.element_size() for k, v in inf.a.items() if k not in ("x0", "heads_ctr"))
        assert E.inference_workspace_bytes(model.cfg, 4, 1024, L.EG_BF16)[1] == own       # the formula is the allocation
    assert sizes[0] == sizes[1] and sizes[0][0] > sizes[0][1] > 0
    assert train[1] > 2 * train[0] > 0
