"""CPU-only: the fused tail's entry points reject null operands, shapes they do not cover and pack-table entries that would read or
write past their buffers -- on the host, before any launch (the addresses below are never dereferenced)."""
import ctypes as C

import pytest

from eyegaze_multimodal_amd import _lib as L

F = 0x10000      # a fake, 16-B aligned device address


def test_fused_heads_reject_null_operands_and_uncovered_shapes():
    with pytest.raises(L.EgError, match="null pointer"):
        L.call("eg_heads_fwd", 0, F, F, F, F, F, F, F, F, 0, F, 0, 0, 0, 4, 256, 3, 0.0, 0, 0, L.EG_BF16, 0)
    with pytest.raises(L.EgError, match="built for 256"):
        L.call("eg_heads_fwd", F, F, F, F, F, F, F, F, F, 0, F, 0, 0, 0, 4, 128, 3, 0.0, 0, 0, L.EG_BF16, 0)
    with pytest.raises(L.EgError, match=r"ncls=17 must be in \[1,16\]"):
        L.call("eg_heads_fwd", F, F, F, F, F, F, F, F, F, 0, F, 0, 0, 0, 4, 256, 17, 0.0, 0, 0, L.EG_BF16, 0)
    with pytest.raises(L.EgError, match="labels need sample_loss, loss and the launch counter"):
        L.call("eg_heads_fwd", F, F, F, F, F, F, F, F, F, F, F, F, F, 0, 4, 256, 3, 0.0, 0, 0, L.EG_BF16, 0)
    with pytest.raises(L.EgError, match="dropout needs the step state"):
        L.call("eg_heads_fwd", F, F, F, F, F, F, F, F, F, 0, F, 0, 0, 0, 4, 256, 3, 0.1, 3, 0, L.EG_BF16, 0)
    with pytest.raises(L.EgError, match="bf16 / fp16 only"):
        L.call("eg_heads_fwd", F, F, F, F, F, F, F, F, F, 0, F, 0, 0, 0, 4, 256, 3, 0.0, 0, 0, L.EG_F32, 0)
    with pytest.raises(L.EgError, match="null pointer"):
        L.call("eg_classifier_ce_bwd_fused", F, F, F, 0, 0, 0, F, F, 0, F, 4, 256, 3, 1, 1.0, L.EG_BF16, 0)
    with pytest.raises(L.EgError, match=r"B=5000 \(<= 256\)"):
        L.call("eg_classifier_ce_bwd_fused", F, F, F, 0, 0, 0, F, F, F, F, 5000, 256, 3, 1, 1.0, L.EG_BF16, 0)
    with pytest.raises(L.EgError, match="null pointer"):
        L.call("eg_heads_bwd_chain", F, F, F, F, F, F, 0, F, 4, 256, L.EG_BF16, 0)
    with pytest.raises(L.EgError, match="at most 256 rows"):
        L.call("eg_heads_bwd_chain", F, F, F, F, F, F, F, F, 257, 256, L.EG_BF16, 0)
    with pytest.raises(L.EgError, match="built for 256"):
        L.call("eg_heads_bwd_chain", F, F, F, F, F, F, F, F, 4, 512, L.EG_BF16, 0)
    with pytest.raises(L.EgError, match="null pointer"):
        L.call("eg_heads_bwd_pool", F, F, F, 0, 0, 0, 0, F, 0, F, F, 4, 65, 256, 1, 0, 1, L.EG_BF16, 0)
    with pytest.raises(L.EgError, match=r"B=300 \(<= 256\)"):
        L.call("eg_heads_bwd_pool", F, F, F, 0, 0, 0, 0, F, F, F, F, 300, 65, 256, 1, 0, 1, L.EG_BF16, 0)
    with pytest.raises(L.EgError, match="bf16 / fp16 only"):
        L.call("eg_heads_bwd_pool", F, F, F, 0, 0, 0, 0, F, F, F, F, 4, 65, 256, 1, 0, 1, L.EG_F32, 0)


def test_token_grad_tail_rejects_bad_arguments():
    m = L.rowmap(256, 66 * 256, 64)
    with pytest.raises(L.EgError, match="null pointer"):
        L.call("eg_token_grad_tail", F, 0, F, m, F, F, 8, 65, 256, 64, 1, 1.0, L.EG_BF16, 0)
    with pytest.raises(L.EgError, match="bad shape"):
        L.call("eg_token_grad_tail", F, F, F, m, F, F, 8, 65, 256, 65, 1, 1.0, L.EG_BF16, 0)
    with pytest.raises(L.EgError, match="multiple of 64"):
        L.call("eg_token_grad_tail", F, F, F, m, F, F, 8, 65, 96, 64, 1, 1.0, L.EG_BF16, 0)
    with pytest.raises(L.EgError, match="bf16 / fp16 only"):
        L.call("eg_token_grad_tail", F, F, F, m, F, F, 8, 65, 256, 64, 1, 1.0, L.EG_F32, 0)


def entry(mode, rows, cols, nblk, blk0=0, ldd=0, p=(0, 0, 0), src_elems=0, dst_elems=0, src=F, dst=F):
    e = L.PackEntryEx()
    e.src, e.dst, e.rows, e.cols, e.ldd, e.mode, e.blk0, e.nblk = src, dst, rows, cols, ldd, mode, blk0, nblk
    e.p0, e.p1, e.p2 = p
    e.src_elems, e.dst_elems = src_elems, dst_elems
    return e


def check(*ents, dtype=L.EG_BF16):
    tab = (L.PackEntryEx * len(ents))(*ents)
    total = C.c_int(0)
    L.call("eg_pack_table_ex_check", C.cast(tab, C.c_void_p), len(ents), dtype, C.byref(total))
    return total.value


def test_pack_table_ex_audit():
    N, Cin, k, Cp, Kp, s, J = 256, 8, 7, 8, 64, 2, 4
    conv = entry(9, N, Cin, 16, p=(k, Cp, Kp), src_elems=N * Cin * k, dst_elems=N * Kp)
    convT = entry(10, N, Cin, 16, blk0=16, p=(k, s, J), src_elems=N * Cin * k, dst_elems=s * Cin * J * N)
    cast = entry(0, 1, 4096, 4, blk0=32)
    assert check(conv, convT, cast) == 36
    with pytest.raises(L.EgError, match="must state src_elems and dst_elems"):
        check(entry(9, N, Cin, 16, p=(k, Cp, Kp)))
    with pytest.raises(L.EgError, match=r"reads 14336 elements of a 14335-element source"):
        check(entry(9, N, Cin, 16, p=(k, Cp, Kp), src_elems=N * Cin * k - 1, dst_elems=N * Kp))
    with pytest.raises(L.EgError, match=r"writes 16384 elements of a 16383-element destination"):
        check(entry(9, N, Cin, 16, p=(k, Cp, Kp), src_elems=N * Cin * k, dst_elems=N * Kp - 1))
    with pytest.raises(L.EgError, match="Cp=8 Kp=48 too small"):
        check(entry(9, N, Cin, 12, p=(k, Cp, 48), src_elems=N * Cin * k, dst_elems=N * 48))
    with pytest.raises(L.EgError, match="do not match k=7"):
        check(entry(10, N, Cin, 16, p=(k, s, 3), src_elems=N * Cin * k, dst_elems=s * Cin * J * N))
    with pytest.raises(L.EgError, match="nblk=15, mode 9 at this shape takes 16"):
        check(entry(9, N, Cin, 15, p=(k, Cp, Kp), src_elems=N * Cin * k, dst_elems=N * Kp))
    with pytest.raises(L.EgError, match="blk0=3, expected 16"):
        check(conv, entry(0, 1, 4096, 4, blk0=3))
    with pytest.raises(L.EgError, match="unknown mode 11"):
        check(entry(11, 4, 4, 1))
    with pytest.raises(L.EgError, match="transpose ldd=100 < rows=256"):
        check(entry(1, 256, 256, 64, ldd=100))
    with pytest.raises(L.EgError, match=r"writes 65536 elements of a 65000-element destination"):
        check(entry(1, 256, 256, 64, ldd=256, dst_elems=65000))
    with pytest.raises(L.EgError, match="needs a 16-bit dtype"):
        check(entry(3, 1024, 256, 128), dtype=L.EG_F32)
    with pytest.raises(L.EgError, match=r"mode 7 needs src \[256, 256\]"):
        check(entry(7, 256, 128, 16))
    with pytest.raises(L.EgError, match="alignment"):
        check(entry(0, 1, 4096, 4, src=F + 4))
    with pytest.raises(L.EgError, match="bad arguments"):
        L.call("eg_pack_table_ex", 0, 1, 1, L.EG_BF16, 0)


def test_engine_builds_and_audits_the_extended_table(monkeypatch):
    """the engine states the extents of every entry it can attribute to one of its buffers, the convolution entries included"""
    import torch
    from eyegaze_multimodal_amd import DualEEGTransformer
    from eyegaze_multimodal_amd.engine import Engine
    model = DualEEGTransformer(in_channels=8, max_len=256, use_spectrogram=False, use_ibs=False)
    cpu = torch.device("cpu")
    model._flat.ensure(cpu)
    seen = {}

    def fake_call(name, *args):          # every launch is recorded instead of issued; the host-side audit really runs
        seen.setdefault(name, []).append(args)
        if name == "eg_pack_table_ex_check":
            L.call(name, *args)
    monkeypatch.setattr("eyegaze_multimodal_amd.engine.call", fake_call)
    eng = Engine(model, 4, 1024, cpu, L.EG_BF16)
    assert eng.fused_tail
    eng.pack_params()
    assert "eg_pack_table_ex" in seen and "eg_pack_conv_weight" not in seen and "eg_pack_convT_weight" not in seen
    raw = bytes(eng._plan_dev.numpy())
    ents = (L.PackEntryEx * eng._plan_n).from_buffer_copy(raw)
    assert [e.mode for e in ents[:3]] == [9, 9, 10]
    assert all(e.src_elems > 0 and e.dst_elems > 0 for e in ents)
    eng.fused_tail = False
    seen.clear()
    eng.pack_params()
    assert "eg_pack_table" in seen and len(seen["eg_pack_conv_weight"]) == 2 and len(seen["eg_pack_convT_weight"]) == 1
