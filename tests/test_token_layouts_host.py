"""CPU-only: the packed weights of the token families (spectrogram CNN, matrix-form and scalar synchrony tokens) and of the image
engine are stages of engine.LAYOUTS.  Launches are recorded, not issued (profiles/tools/launch_trace.py's Recorder; the host audit
of the pack table really runs).  The dims are the golden config tiny_full's, with spectrogram + matrix-form synchrony tokens and
with the scalar synchrony token alone, B = 4, T = 1024, bf16 and f32."""
import sys
from pathlib import Path

import pytest
import torch

from eyegaze_multimodal_amd import DualEEGTransformer, engine as E, image_encoder, tokens
from eyegaze_multimodal_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "profiles" / "tools"))
from launch_trace import Recorder  # noqa: E402

TINY = dict(d_model=64, num_layers=2, num_heads=2, d_ff=128, in_channels=8, max_len=256)
FAMILIES = {"spec_robust": dict(TINY, use_spectrogram=True, use_ibs=True, use_robust_ibs=True),
            "scalar": dict(TINY, use_spectrogram=False, use_ibs=True, use_robust_ibs=False)}
B, T = 4, 1024
CPU = torch.device("cpu")
DTYPES = {"bf16": L.EG_BF16, "f32": L.EG_F32}
BWD_KEYS = ("spc2T", "spp0T", "spp3T", "ib0T", "ib3T", "ig3T")
TOKEN_KEYS = ("spc2", "spc2T", "spp0", "spp0T", "spp3", "spp3T", "ib0", "ib0T", "ib3", "ib3T", "ig0", "ig3", "ig3T")
SOURCE = {"spp0": "spectrogram_generator.proj.0.weight", "spp3": "spectrogram_generator.proj.3.weight",
          "ib0": "ibs_tokenizer.bottleneck.0.weight", "ib3": "ibs_tokenizer.bottleneck.3.weight",
          "ig0": "ibs_generator.proj.0.weight", "ig3": "ibs_generator.proj.3.weight"}
CAST, TRANSPOSE, CONV = 0, 1, 9


def expected_entries(family, dtype, inference):
    """(key, mode) of the token entries in table order: CNN first, then the synchrony tokens.  spc2 / spc2T have no table mode
    (own launches); ig0 is a mode-9 entry under the 16-bit engines' eg_pack_table_ex and its own launch in f32."""
    if family == "spec_robust":
        want = [("spp0", CAST), ("spp0T", TRANSPOSE), ("spp3", CAST), ("spp3T", TRANSPOSE),
                ("ib0", CAST), ("ib0T", TRANSPOSE), ("ib3", CAST), ("ib3T", TRANSPOSE)]
    else:
        want = ([("ig0", CONV)] if dtype != "f32" else []) + [("ig3", CAST), ("ig3T", TRANSPOSE)]
    return [(k, m) for k, m in want if not (inference and k in BWD_KEYS)]


@pytest.fixture
def rec(monkeypatch):
    r = Recorder(L.call)
    for m in (E, tokens, image_encoder):
        monkeypatch.setattr(m, "call", r)
    return r


def make(rec, kw, cls, dtype):
    model = DualEEGTransformer(**kw)
    model._flat.ensure(CPU, need_grad=cls is E.Engine)
    eng = cls(model, B, T, CPU, DTYPES[dtype])
    rec.engines = [("", eng)]
    return eng


def forward(eng):
    x, y = torch.zeros(B, eng.C, T), torch.zeros(B, dtype=torch.long)
    eng.forward(x, x, y, train=False) if isinstance(eng, E.Engine) else eng.forward(x, x, y)


def table(eng):
    kind = L.PackEntryEx if eng.fused_tail else L.PackEntry
    return list((kind * eng._plan_n).from_buffer_copy(bytes(eng._plan_dev.numpy())))


def inside(eng, e, key):
    t = eng.w.get(key)
    return t is not None and t.data_ptr() <= e.dst < t.data_ptr() + t.numel() * t.element_size()


def token_entries(eng, ents):
    """[(index, key, entry)] of the entries that write a token-family buffer"""
    return [(i, k, e) for i, e in enumerate(ents) for k in TOKEN_KEYS if inside(eng, e, k)]


def launches(rec, name, key=None):
    """recorded launches of `name` (whose destination, argument 2, is w[key])"""
    return [r for r in rec.rows if r[0] == name and (key is None or r[2] == [f"w.{key}", 0])]


def rerecords(rec, eng, attr):
    """flips the routing attribute on the live engine and packs again: a new plan, audited again where the table has an audit"""
    audits, plan = len(launches(rec, "eg_pack_table_ex_check")), eng._plan_dev
    setattr(eng, attr, not getattr(eng, attr))
    eng.pack_params()
    assert eng._plan_dev is not plan
    assert len(launches(rec, "eg_pack_table_ex_check")) == audits + (1 if eng.fused_tail else 0)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("cls", [E.Engine, E.InferenceEngine], ids=["train", "infer"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_a_live_engine_rerecords_its_plan(rec, family, cls, dtype):
    """The inference engine holds no backward layout, so ln_proj may take any value on it.  The training engine at d_model = 64 has
    ln_proj off and never allocated the fragment layout that the route reads (Engine._held), so turning it ON is no state of that
    engine: there pack_unused is flipped, which keys the plan just the same.  The literal ln_proj flip on a training engine is the
    next test's, at the d_model = 256 where the route exists."""
    eng = make(rec, FAMILIES[family], cls, dtype)
    forward(eng)
    rerecords(rec, eng, "ln_proj" if cls is E.InferenceEngine else "pack_unused")
    forward(eng)


@pytest.mark.parametrize("cls", [E.Engine, E.InferenceEngine], ids=["train", "infer"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_flipping_ln_proj_on_a_live_engine_with_token_families_rerecords(rec, family, cls):
    kw = dict(FAMILIES[family], d_model=256, num_heads=8, d_ff=1024)
    eng = make(rec, kw, cls, "bf16")
    assert eng.ln_proj == (cls is E.Engine) and eng.fused_tail
    forward(eng)
    rerecords(rec, eng, "ln_proj")
    if cls is E.Engine:         # the separate backward-data product's out_proj^T is packed now
        assert any(inside(eng, e, "oT0") for e in table(eng))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("cls", [E.Engine, E.InferenceEngine], ids=["train", "infer"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_value_of_w_a_and_g_is_a_tensor(rec, family, cls, dtype):
    eng = make(rec, FAMILIES[family], cls, dtype)
    forward(eng)
    if cls is E.Engine:
        eng._alloc_bwd()
        assert eng.g
    for kind in ("w", "a", "g"):
        assert all(torch.is_tensor(v) for v in getattr(eng, kind).values()), kind
    lo, hi = eng.band_edges                 # the synchrony kernels' band edges: host arrays, kept alive beside the tensors
    assert len(lo) == len(hi) == eng.ib["nb"]


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("cls", [E.Engine, E.InferenceEngine], ids=["train", "infer"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_each_held_token_layout_is_hit_by_exactly_one_entry(rec, family, cls, dtype):
    eng = make(rec, FAMILIES[family], cls, dtype)
    eng.pack_params()
    ents = table(eng)
    want = expected_entries(family, dtype, cls is E.InferenceEngine)
    got = token_entries(eng, ents)
    assert [(k, e.mode) for _, k, e in got] == want
    # after the heads' (and the synchrony classifier's) entries: the tail of the table
    assert [i for i, _, _ in got] == list(range(len(ents) - len(want), len(ents)))
    held = [k for k in TOKEN_KEYS if k in eng.w]
    in_table = [k for k, _ in want]
    assert sorted(held) == sorted(in_table + [k for k in held if k.startswith("spc2") or (k == "ig0" and dtype == "f32")])
    for _, k, e in got:
        assert e.dst == eng.w[k].data_ptr() and e.src == eng.fp.p_ptr(SOURCE[k.rstrip("T")]) and e.nblk > 0


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_inference_engine_holds_and_records_no_backward_token_layout(rec, family, dtype):
    train = make(rec, FAMILIES[family], E.Engine, dtype)
    train.pack_params()
    infer = make(rec, FAMILIES[family], E.InferenceEngine, dtype)
    infer.pack_params()
    assert not [k for k in infer.w if k in BWD_KEYS]
    assert sorted(k for k in train.w if k in BWD_KEYS) == (["ib0T", "ib3T", "spc2T", "spp0T", "spp3T"] if family == "spec_robust" else ["ig3T"])
    t_ents, i_ents = token_entries(train, table(train)), token_entries(infer, table(infer))

    def fields(e):      # every field but src / dst -- and blk0, the entry's place among the blocks of a table that is shorter here
        ex = (e.p0, e.p1, e.p2, e.src_elems, e.dst_elems) if hasattr(e, "p0") else ()
        return (e.rows, e.cols, e.ldd, e.mode, e.nblk, *ex)
    assert [(k, fields(e)) for _, k, e in i_ents] == [(k, fields(e)) for _, k, e in t_ents if k not in BWD_KEYS]
    assert len(i_ents) == len(expected_entries(family, dtype, True))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("cls", [E.Engine, E.InferenceEngine], ids=["train", "infer"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_packs_outside_the_table_are_issued_on_every_call(rec, family, cls, dtype):
    eng = make(rec, FAMILIES[family], cls, dtype)
    for call_no in (0, 1):                  # the recording call, then a replay
        del rec.rows[:]
        eng.pack_params()
        assert len(launches(rec, "eg_pack_table_ex_check")) == (1 if call_no == 0 and dtype != "f32" else 0)
        conv2d = launches(rec, "eg_pack_conv2d_weight")
        if family == "spec_robust":
            assert [r[2][0] for r in conv2d] == (["w.spc2"] if cls is E.InferenceEngine else ["w.spc2", "w.spc2T"])
            assert len(launches(rec, "eg_rows_bcast_f32")) == 1                 # ib_add
        else:
            assert not conv2d
            assert len(launches(rec, "eg_pack_conv_weight", "ig0")) == (1 if dtype == "f32" else 0)
        # ... and before the one table launch, which ends the call
        assert [r[0] for r in rec.rows].index("eg_pack_table_ex" if dtype != "f32" else "eg_pack_table") == len(rec.rows) - 1


def test_image_engine_packs_through_the_same_walk(rec):
    model = image_encoder.GazeCNNEncoder(num_classes=3, d_model=64, compute_dtype="bf16")
    model._flat.ensure(CPU)
    eng = image_encoder.ImageEngine(model, B, 64, 16, CPU, L.EG_BF16)
    rec.engines = [("", eng)]
    assert sorted(eng.w) == sorted(["spc2", "spc2T", "spp0", "spp0T", "spp3", "spp3T"])
    for call_no in (0, 1):
        del rec.rows[:]
        eng.pack_params()
        assert [r[0] for r in rec.rows] == ["eg_pack_conv2d_weight", "eg_pack_conv2d_weight", "eg_pack_table"]
        assert [r[2][0] for r in rec.rows[:2]] == ["w.spc2", "w.spc2T"]
    ents = table(eng)
    assert [(k, e.mode) for _, k, e in token_entries(eng, ents)] == [("spp0", CAST), ("spp0T", TRANSPOSE), ("spp3", CAST), ("spp3T", TRANSPOSE)]
    assert len(ents) == 4 and all(e.dst == eng.w[k].data_ptr() for (_, k, e) in token_entries(eng, ents))
    assert all(torch.is_tensor(v) for kind in ("w", "a", "g") for v in getattr(eng, kind).values())
