"""The head kernels (csrc/heads.hip) and the 128-tile weight gradient against their fp64 statements (tests/anchor_ref.py).

eg_heads_fwd / eg_heads_bwd_pool / eg_classifier_ce_bwd_fused / eg_token_grad_tail and the 256-tile eg_gemm_tn are held bit for
bit to the launches below; this file holds those launches themselves, in every dtype: eg_pool_fuse_fwd and _bwd (ties a == c
planted, every optional incoming gradient present and NULL, dz compared whole), eg_classifier_ce_fwd / _bwd (labels and the
incoming logit gradient present and NULL, the ReLU gate with its scale, dW and db), eg_batch_rowsum, eg_rows_gather_gate,
eg_rows_bcast_f32, eg_rows_copy (exact) and eg_gemm_tn's 128 tile with part_rows, has_bias and x_tile_stride.  Every element
must lie within 1.5 u |ref| + slack; the slack of the products is derived, that of the rest measured on the CPU."""
import ctypes as C
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd._lib import GemmTNDesc, call, ptr, rowmap  # noqa: E402
from tests import anchor_ref as R  # noqa: E402

DEV = "cuda"
SENT = R.SENT


def full(shape, dtype=torch.float32):
    return torch.full(shape, SENT, device=DEV, dtype=dtype)


def cpu(t):
    return t.double().cpu()


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("B,S,D,off", R.POOL_CASES)
def test_pool_fuse_fwd_bwd_match_fp64(B, S, D, off, dtype):
    t = R.pool_case(B, S, D, off, dtype)
    eg, tdt = R.EG[dtype], R.TDT[dtype]
    d = {k: v.to(DEV) for k, v in t.items()}
    for n_ibs in R.POOL_IBS:
        n_ibs = min(n_ibs, S - 1)                     # the tokens 1 .. n_ibs must exist
        what = "B%d S%d D%d off%d n_ibs%d %s" % (B, S, D, off, n_ibs, dtype)
        cls1, cls2, ipf = full((B + 1, D)), full((B + 1, D)), full((B + 1, D))
        comb, zf, ip = full((B + 1, 3 * D), tdt), full((B + 1, 3 * D), tdt), full((B + 1, D), tdt)
        call("eg_pool_fuse_fwd", ptr(d["z"]), ptr(cls1), ptr(cls2), ptr(comb), ptr(zf), ptr(ipf), ptr(ip), B, S, D, off, n_ibs, 1, eg, 0)
        torch.cuda.synchronize()
        for buf in (cls1, cls2, comb, zf) + ((ipf, ip) if n_ibs else ()):
            assert bool((buf[B] == SENT).all()), what + ": wrote past the last sample"
        if not n_ibs:
            assert bool((ipf == SENT).all()) and bool((ip == SENT).all())
        assert bool((zf[:B, :D] == SENT).all()), what + ": zf[:, :D] belongs to the fusion product"
        got = dict(cls1=cpu(cls1[:B]), cls2=cpu(cls2[:B]), comb=cpu(comb[:B]), pool=cpu(zf[:B, D:]))
        if n_ibs:
            got.update(ibs=cpu(ip[:B]), ibs_f32=cpu(ipf[:B]))
        R.assert_all_within(got, R.pool_fwd_outputs(t, B, off, n_ibs, dtype), what + " fwd")
        # backward: every optional incoming gradient on its own, all of them, none of them
        names = ("gcls1", "gcls2", "dibs_pool", "gibs_pool")
        for present in [set(), set(names)] + [{n} for n in names]:
            dz = full((2 * B + 1, S, D), tdt)
            opt = [ptr(d[n]) if n in present else 0 for n in names]
            call("eg_pool_fuse_bwd", ptr(d["z"]), ptr(d["dcomb"]), ptr(d["dzf"]), opt[0], opt[1], opt[2], opt[3], ptr(dz), B, S, D, off,
                 n_ibs, 1, eg, 0)
            torch.cuda.synchronize()
            assert bool((dz[2 * B] == SENT).all())
            ref = R.pool_bwd_outputs(t, B, off, n_ibs, present, dtype)
            R.assert_all_within(dict(dz=cpu(dz[:2 * B])), ref, what + " bwd " + ",".join(sorted(present)))
            nowhere = ref["dz"][0] == 0                 # rows no gradient reaches are written as exact zeros
            assert bool((cpu(dz[:2 * B])[nowhere] == 0).all())


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("B,K,ncls", R.CE_CASES)
def test_classifier_ce_fwd_bwd_match_fp64(B, K, ncls, dtype):
    t = R.ce_case(B, K, ncls, dtype)
    eg, tdt = R.EG[dtype], R.TDT[dtype]
    d = {k: v.to(DEV) for k, v in t.items()}
    logits_ref = None
    for with_labels in (True, False):
        what = "B%d K%d ncls%d %s labels=%d" % (B, K, ncls, dtype, with_labels)
        logits, sl, loss = full((B + 1, ncls)), full((B + 1,)), full((2,))
        call("eg_classifier_ce_fwd", ptr(d["h"]), ptr(d["W"]), ptr(d["bias"]), ptr(d["labels"]) if with_labels else 0, ptr(logits),
             ptr(sl), ptr(loss), B, K, ncls, eg, 0)
        torch.cuda.synchronize()
        assert bool((logits[B] == SENT).all()) and float(sl[B]) == SENT and float(loss[1]) == SENT
        got = dict(logits=cpu(logits[:B]))
        if with_labels:
            got.update(sample_loss=cpu(sl[:B]), loss=cpu(loss[:1]))
        else:
            assert bool((sl == SENT).all()) and bool((loss == SENT).all())
        R.assert_all_within(got, R.ce_fwd_outputs(t, with_labels), what + " fwd")
        if logits_ref is None:
            logits_ref = logits[:B].contiguous()
        else:
            assert torch.equal(logits[:B], logits_ref)            # the logits do not depend on the labels
    stored = logits_ref.cpu()                                     # the backward reads the STORED logits, on both sides
    for with_labels, with_glogits, use_gate in itertools.product((True, False), (True, False), (1, 0)):
        what = "B%d K%d ncls%d %s labels=%d glogits=%d gate=%d" % (B, K, ncls, dtype, with_labels, with_glogits, use_gate)
        dlog, dh, dW, db = full((B + 1, ncls)), full((B + 1, K), tdt), full((ncls + 1, K)), full((ncls + 1,))
        call("eg_classifier_ce_bwd", ptr(d["h"]), ptr(d["W"]), ptr(logits_ref), ptr(d["labels"]) if with_labels else 0,
             ptr(d["gloss"]) if with_labels else 0, ptr(d["glogits"]) if with_glogits else 0, ptr(dlog), ptr(dh), ptr(dW), ptr(db), B, K,
             ncls, use_gate, R.CE_GATE_SCALE, eg, 0)
        torch.cuda.synchronize()
        for buf, n in ((dlog, B), (dh, B), (dW, ncls)):
            assert bool((buf[n] == SENT).all()), what + ": wrote past the end"
        assert float(db[ncls]) == SENT
        got = dict(dlogits=cpu(dlog[:B]), dh=cpu(dh[:B]), dW=cpu(dW[:ncls]), db=cpu(db[:ncls]))
        R.assert_all_within(got, R.ce_bwd_outputs(t, stored, with_labels, with_glogits, use_gate, dtype), what)
        if use_gate:
            assert bool((got["dh"][t["h"].double() <= 0] == 0).all()), what + ": the closed gate must give exact zeros"


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("NB", [1, 13, 16, 40])
def test_batch_rowsum_matches_fp64(NB, dtype):
    S, D, rows = 7, 96, 5
    g = torch.Generator().manual_seed(NB)
    dseq = torch.randn(NB, S, D, generator=g).to(R.TDT[dtype])
    dd = dseq.to(DEV)
    out = full((rows + 1, D))
    call("eg_batch_rowsum", ptr(dd), ptr(out), NB, S, D, rows, R.EG[dtype], 0)
    torch.cuda.synchronize()
    assert bool((out[rows] == SENT).all())
    ref = R.batch_rowsum_ref(dseq, rows)
    sl = R.f32_slack(lambda dt, order: R.batch_rowsum_ref(dseq, rows, dt=dt, order=order), ref)
    R.assert_within(cpu(out[:rows]), ref["out"], R.U["f32"], sl["out"], "NB%d %s (slack %.3g)" % (NB, dtype, sl["out"]))


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("pair_shift,gated", [(0, 0), (0, 1), (3, 0), (3, 1)])
def test_rows_gather_gate_matches_fp64(pair_shift, gated, dtype):
    nb, S, D, Rr, off = 3, 9, 72, 4, 2
    tdt = R.TDT[dtype]
    g = torch.Generator().manual_seed(11 + pair_shift)
    src = torch.randn(2 * nb, S, D, generator=g).to(tdt)
    gate = torch.randn(nb, Rr, D, generator=g)
    gate[:, :, ::5], gate[:, :, 1::5] = 0.0, -0.0
    gate = gate.to(tdt)
    dmap = (2 * D, 11 * D, 4)                          # every other row of groups of 11: gaps keep their sentinel
    dst = torch.full((nb * 11 * D + 16,), SENT).to(tdt)
    sd, gd, dd = src.to(DEV), gate.to(DEV), dst.to(DEV)
    scale = R.f32(1.0 / 0.9)
    call("eg_rows_gather_gate", ptr(sd), ptr(gd) if gated else 0, ptr(dd), rowmap(*dmap), nb, S, D, Rr, off, pair_shift, scale,
         R.EG[dtype], 0)
    torch.cuda.synchronize()
    ref, written = R.rows_gather_gate_ref(src, gate if gated else None, dst, dmap, nb, Rr, off, pair_shift, scale)
    got = cpu(dd)
    assert bool((got[~written] == SENT).all()), "a gap or the tail was overwritten"
    # one fp32 sum and one fp32 product in front of the store: 2 * 2^-24 relative, far inside the 0.5 u the factor 1.5 leaves
    # for the 16-bit types; for f32 they are the result's own roundings
    R.assert_within(got, ref, R.U[dtype], 2.0 ** -23 * ref.abs() * written, "pair_shift%d gated%d %s" % (pair_shift, gated, dtype))
    if gated:
        closed = torch.zeros_like(written)
        o = R.row_off(dmap, torch.arange(nb * Rr))[:, None] + torch.arange(D)[None, :]
        closed[o] = (gate.double() <= 0).reshape(nb * Rr, D)
        assert bool((got[closed] == 0).all())


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_rows_bcast_and_copy_match_fp64(dtype):
    NB, S, D, Rr, off, src_nb = 5, 8, 40, 3, 2, 2
    tdt = R.TDT[dtype]
    g = torch.Generator().manual_seed(4)
    src, pos = torch.randn(src_nb, Rr, D, generator=g), torch.randn(S, D, generator=g)
    seq = torch.randn(NB, S, D, generator=g).to(tdt)
    srcd, posd = src.to(DEV), pos.to(DEV)
    for with_pos in (True, False):
        sd = seq.to(DEV)
        call("eg_rows_bcast_f32", ptr(srcd), ptr(posd) if with_pos else 0, ptr(sd), NB, S, D, Rr, off, src_nb, R.EG[dtype], 0)
        torch.cuda.synchronize()
        ref = R.rows_bcast_ref(src, pos if with_pos else None, seq, off, src_nb)
        got = cpu(sd)
        touched = torch.zeros(NB, S, D, dtype=torch.bool)
        touched[:, off:off + Rr] = True
        assert torch.equal(got[~touched], seq.double()[~touched])
        R.assert_within(got, ref, R.U[dtype], 0.0, "bcast pos=%d %s" % (with_pos, dtype))    # one fp32 sum, then the store
    sd = seq.to(DEV)
    call("eg_rows_copy", ptr(sd), S, D, Rr, off, 1, 3, 2, R.EG[dtype], 0)
    torch.cuda.synchronize()
    assert torch.equal(sd.cpu(), R.rows_copy_ref(seq, Rr, off, 1, 3, 2))                     # a copy: exact


TN_CASES = [(M, N, K, splits, pr, hb, 0) for (M, N, K) in ((70, 64, 128), (1000, 256, 256)) for splits in (1, 3)
            for pr in (0, 1) for hb in (0, 1)] + [(70, 64, 256, 3, 1, 1, 192)]


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("M,N,K,splits,half_parts,has_bias,xts", TN_CASES)
def test_gemm_tn_128_tile_matches_fp64(M, N, K, splits, half_parts, has_bias, xts, dtype):
    tdt = R.TDT[dtype]
    part_rows = N // 2 if half_parts else 0
    g = torch.Generator().manual_seed(M + N + K)
    ldy = N + 8
    dY = torch.randn(M, ldy, generator=g).to(tdt)
    if xts:                                            # 128-column tiles of an X row xts elements apart
        ldx = (K // 128) * xts + 8
        X = torch.randn(M, ldx, generator=g).to(tdt)
    else:
        ldx = K + 8
        X = torch.randn(M, ldx, generator=g).to(tdt)
    dY[3, :], X[5, :] = 0.0, 0.0
    slab = (N // (part_rows or N)) * ((part_rows or N) * K + ((part_rows or N) if has_bias else 0))
    part = full((splits * slab + 8,))
    dYd, Xd = dY.to(DEV), X.to(DEV)
    d = GemmTNDesc()
    d.dY, d.X, d.partial = ptr(dYd), ptr(Xd), ptr(part)
    d.y, d.x = rowmap(ldy), rowmap(ldx)
    d.M, d.N, d.K, d.splits, d.dtype = M, N, K, splits, R.EG[dtype]
    d.x_tile_stride, d.part_rows, d.has_bias, d.tile = xts, part_rows, has_bias, 128
    call("eg_gemm_tn", C.byref(d), 0)
    out = full((slab + 4,))
    call("eg_reduce_partials", ptr(part), ptr(out), slab, splits, slab, 0, 0)
    torch.cuda.synchronize()
    assert bool((part[splits * slab:] == SENT).all()) and bool((out[slab:] == SENT).all())
    ref, slack = R.gemm_tn_ref(dY, X, M=M, N=N, K=K, y=(ldy, 0, 0), x=(ldx, 0, 0), x_tile_stride=xts, part_rows=part_rows,
                               has_bias=has_bias)
    R.assert_within(cpu(out[:slab]), ref, R.U["f32"], slack, "M%d N%d K%d splits%d part_rows%d bias%d xts%d %s"
                    % (M, N, K, splits, part_rows, has_bias, xts, dtype))
