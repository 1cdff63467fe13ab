"""CPU-only: the pack table of the default 16-bit engine leaves out the layouts that its routes never read, `pack_unused`
restores the full table, and a routing flag flipped on a live engine re-records the plan.  Every launch is recorded instead of
issued; the host-side audit of the table really runs."""
import pytest
import torch

from eyegaze_multimodal_amd import DualEEGTransformer
from eyegaze_multimodal_amd import _lib as L
from eyegaze_multimodal_amd.engine import Engine

DROPPED = ("w1", "w2", "w1T", "w2T", "qkv", "o", "oT")


@pytest.fixture
def engine(monkeypatch):
    model = DualEEGTransformer(in_channels=8, max_len=256, use_spectrogram=False, use_ibs=False)
    cpu = torch.device("cpu")
    model._flat.ensure(cpu)
    seen = {}

    def fake_call(name, *args):
        seen.setdefault(name, []).append(args)
        if name == "eg_pack_table_ex_check":
            L.call(name, *args)
    monkeypatch.setattr("eyegaze_multimodal_amd.engine.call", fake_call)
    eng = Engine(model, 4, 1024, cpu, L.EG_BF16)
    eng.seen = seen
    return eng


def table(eng):
    eng.pack_params()
    return list((L.PackEntryEx * eng._plan_n).from_buffer_copy(bytes(eng._plan_dev.numpy())))


def fields(e):
    return (e.src, e.dst, e.rows, e.cols, e.ldd, e.mode, e.nblk, e.p0, e.p1, e.p2, e.src_elems, e.dst_elems)


def inside(eng, e, name):
    t = eng.w[name]
    return t.data_ptr() <= e.dst < t.data_ptr() + t.numel() * t.element_size()


def hits(eng, ents, names):
    return sorted(n for n in names for e in ents if inside(eng, e, n))


def test_default_engine_drops_the_layouts_nobody_reads(engine):
    eng = engine
    assert eng.fuse_ffn and eng.attn_block and eng.ln_proj and eng.pack_unused is False
    layers = range(eng.cfg.num_layers)
    dropped = [f"{n}{l}" for n in DROPPED for l in layers]
    ents = table(eng)
    assert [e.mode for e in ents[:3]] == [9, 9, 10]
    assert hits(eng, ents, dropped) == []
    # the cross-attention block keeps its row-major layouts, the layers keep what their fused kernels read
    assert set(hits(eng, ents, ["qkvx", "ox", "oTx"])) == {"qkvx", "ox", "oTx"}
    kept = [f"{n}{l}" for n in ("qkvT", "bqkv", "oTf", "wqkvb", "wob", "w1f", "w2f", "w2Tf", "w1Tf") for l in layers]
    assert set(hits(eng, ents, kept)) == set(kept)
    blocks = [e.blk0 for e in ents]
    assert blocks == sorted(blocks) and blocks[0] == 0 and ents[-1].blk0 + ents[-1].nblk == eng._plan_blocks


def test_pack_unused_restores_the_full_table(engine):
    eng = engine
    layers = range(eng.cfg.num_layers)
    short = table(eng)
    eng.pack_unused = True
    full = table(eng)
    dropped = [f"{n}{l}" for n in DROPPED for l in layers]
    assert set(hits(eng, full, dropped)) == set(dropped)
    # per layer: 3 + 1 row-major attention casts, out_proj^T, 2 casts + 2 transposes of the feed-forward pair
    assert len(full) == len(short) + 9 * eng.cfg.num_layers
    # the full table is the short one plus the dropped entries, in the recording order of _pack_body
    extra = [e for e in full if any(inside(eng, e, n) for n in dropped)]
    rest = [e for e in full if not any(inside(eng, e, n) for n in dropped)]
    assert [fields(e) for e in rest] == [fields(e) for e in short]
    assert all(e.mode in (0, 1) for e in extra)
    # every route off records exactly the same row-major entries as pack_unused does: that is the table before this change
    want = []
    for l in layers:
        want += [(f"qkv{l}", 0)] * 3 + [(f"o{l}", 0), (f"oT{l}", 1), (f"w1{l}", 0), (f"w1T{l}", 1), (f"w2{l}", 0), (f"w2T{l}", 1)]
    assert [(next(n for n in dropped if inside(eng, e, n)), e.mode) for e in extra] == want


def test_flipping_a_route_rerecords_the_plan(engine):
    eng = engine
    layers = range(eng.cfg.num_layers)
    assert hits(eng, table(eng), [f"oT{l}" for l in layers]) == []
    n0 = len(eng.seen["eg_pack_table_ex_check"])
    table(eng)
    assert len(eng.seen["eg_pack_table_ex_check"]) == n0          # unchanged flags: the recorded plan is replayed
    eng.ln_proj = False
    ents = table(eng)
    assert len(eng.seen["eg_pack_table_ex_check"]) == n0 + 1
    assert hits(eng, ents, [f"oT{l}" for l in layers]) == [f"oT{l}" for l in layers]
    assert hits(eng, ents, [f"w1{l}" for l in layers] + [f"qkv{l}" for l in layers]) == []
    eng.fuse_ffn = False
    ents = table(eng)
    assert set(hits(eng, ents, [f"{n}{l}" for n in ("w1", "w1T", "w2", "w2T") for l in layers])) == \
        {f"{n}{l}" for n in ("w1", "w1T", "w2", "w2T") for l in layers}
    eng.attn_block = False
    ents = table(eng)
    assert set(hits(eng, ents, [f"{n}{l}" for n in ("qkv", "o") for l in layers])) == {f"{n}{l}" for n in ("qkv", "o") for l in layers}


def test_sqnorm_clip_rejects_bad_arguments():
    F = 0x10000
    with pytest.raises(L.EgError, match="bad arguments"):
        L.call("eg_grad_sqnorm_clip", F, 16, F, 4, 1.0, F, 0, 0)
    with pytest.raises(L.EgError, match="bad arguments"):
        L.call("eg_grad_sqnorm_clip", F, 16, F, 5000, 1.0, F, F, 0)
    with pytest.raises(L.EgError, match="alignment"):
        L.call("eg_grad_sqnorm_clip", F + 4, 16, F, 4, 1.0, F, F, 0)


def test_norm_partials_ride_in_the_grouped_reduce_without_a_listener(monkeypatch):
    """B = 32 has enough rows for the grouped weight-gradient plan; the launches are recorded, not issued"""
    model = DualEEGTransformer(in_channels=8, max_len=256, use_spectrogram=False, use_ibs=False)
    cpu = torch.device("cpu")
    model._flat.ensure(cpu)
    seen = []

    def fake_call(name, *args):
        seen.append((name, args))
        if name == "eg_pack_table_ex_check":
            L.call(name, *args)
    monkeypatch.setattr("eyegaze_multimodal_amd.engine.call", fake_call)
    eng = Engine(model, 32, 1024, cpu, L.EG_BF16)
    x = torch.zeros(32, 8, 1024)
    eng.forward(x, x, torch.zeros(32, dtype=torch.long), train=True)

    def backward(**kw):
        del seen[:]
        eng.backward(gloss=torch.ones(1), **kw)
        return [n for n, _ in seen], [a for n, a in seen if n == "eg_reduce_table"]

    names, tables = backward()
    pl = eng._wg_plan
    d, nl = eng.cfg.d_model, eng.cfg.num_layers
    assert len(tables) == 1 and tables[0][1:3] == (pl["whole_norms"]["nr"], pl["whole_norms"]["rblocks"])
    assert pl["whole_norms"]["nr"] == pl["nr"] + 2 and eng._ln_slot["encoder.norm"] == 2 * nl
    rt = (L.ReduceEntry * pl["whole_norms"]["nr"]).from_buffer_copy(bytes(pl["whole_norms"]["rt"].numpy()))
    # the LayerNorm entries lead the table, the two norms outside the layers last among them; block ranges are contiguous
    lns = rt[:2 * nl + 2]
    assert all(r.n == 2 * d and r.splits > 8 for r in lns) and all(r.splits <= 8 for r in rt[2 * nl + 2:])
    grad = model._flat
    assert [r.out for r in lns[-2:]] == [grad.g_ptr("encoder.norm.weight"), grad.g_ptr("cross_attn.norm.weight")]
    assert [r.splits for r in lns[-2:]] == [eng.LN_BLOCKS] * 2
    blk = 0
    for r in rt:
        assert r.blk0 == blk
        blk += (r.n // 4 + 255) // 256 if r.splits <= 8 else (r.n // 4 + 7) // 8
    assert blk == pl["whole_norms"]["rblocks"]
    deferred = names.count("eg_reduce_partials")
    # a listener: the two norms are reduced at once again, and the grouped launches carry the layers' entries only
    names, tables = backward(on_segment=lambda name: None)
    assert names.count("eg_reduce_partials") == deferred + 2
    assert sum(t[1] for t in tables) == pl["nr"]
