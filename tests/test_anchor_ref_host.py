"""tests/anchor_ref.py on the CPU: (1) its fp64 references agree with torch's own operators and autograd to 1e-12, so what the
GPU anchor tests compare against is the operation and not a private reading of it; (2) its comparator, at the bounds the GPU
tests use and on THEIR case tables, accepts the correctly rounded reference and rejects each of the listed defects in every
dtype -- the bounds are neither too tight for a correct kernel's one rounding nor loose enough to pass a wrong one.

A defect is tried on the cases whose switches can show it (anchor_ref.gemm_defects_for and the parametrisations below name
them from the case's switches, never from the outcome): a mask defect needs a dropout, `p by c` an out_pre whose rows are
spaced differently from C's, the CE mean B > 1, and so on."""

import pytest
import torch
import torch.nn.functional as F

from tests import anchor_ref as R
from tests.anchor_ref import F64, U

REL = 1e-12


def close(got, ref, what=""):
    scale = max(float(ref.abs().max()), 1e-300)
    err = float((got - ref).abs().max())
    assert err <= REL * scale, (what, err, scale)


def stored(ref_outputs):
    """the correctly rounded outputs: every output rounded once to the format its bound names (u = 0: an exact copy)"""
    fmt = {U["bf16"]: torch.bfloat16, U["fp16"]: torch.float16, U["f32"]: torch.float32}
    return {k: (r if u == 0 else r.to(fmt[u]).to(F64)) for k, (r, u, s) in ref_outputs.items()}


def stored_as(defective, ref_outputs):
    """a defective reference, rounded as a kernel would store it"""
    fmt = {U["bf16"]: torch.bfloat16, U["fp16"]: torch.float16, U["f32"]: torch.float32}
    return {k: (defective[k] if u == 0 else defective[k].to(fmt[u]).to(F64)) for k, (r, u, s) in ref_outputs.items()}


# ------------------------------------------------------------------------------------------------------
# 1. the references against torch, in float64
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M", [(4, 1), (100, 130), (256, 7)])
def test_layernorm_refs_match_torch(D, M):
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(M, D, generator=g, dtype=F64) * 2 + 0.5).requires_grad_(True)
    gamma, beta = torch.randn(D, generator=g, dtype=F64).requires_grad_(True), torch.randn(D, generator=g, dtype=F64).requires_grad_(True)
    dy = torch.randn(M, D, generator=g, dtype=F64)
    ref = F.layer_norm(x, (D,), gamma, beta, 1e-5)
    ref.backward(dy)
    y, mean, rstd = R.layernorm_ref(x.detach(), gamma.detach(), beta.detach())
    close(y, ref.detach(), "y")
    close(mean, x.detach().mean(1), "mean")
    close(rstd, 1 / torch.sqrt(x.detach().var(1, unbiased=False) + 1e-5), "rstd")
    dx, dd, dg, db = R.layernorm_bwd_ref(dy, x.detach(), mean, rstd, gamma.detach())
    close(dx, x.grad, "dx")
    assert torch.equal(dd, dx)                       # no dropout: dx_drop is dx
    close(dg, gamma.grad, "dgamma")
    close(db, beta.grad, "dbeta")
    # dx_drop = drop1(drop2(dx)): the masks multiply, in either order
    dx, dd, _, _ = R.layernorm_bwd_ref(dy, x.detach(), mean, rstd, gamma.detach(), (0.1, 5), (0.2, 6), seed=3)
    keep = R.norm_keep(M, D, (0.1, 5), (0.2, 6), 3)
    close(dd, torch.where(keep, dx * R.drop_scale(0.1) * R.drop_scale(0.2), torch.zeros_like(dx)), "dx_drop")
    for order in R.ORDERS:                           # the three summation orders are the same sums
        close(R.layernorm_ref(x.detach(), gamma.detach(), beta.detach(), order=order)[0], ref.detach(), order)


@pytest.mark.parametrize("B,K,ncls", [(1, 64, 1), (5, 200, 3), (33, 256, 16)])
def test_classifier_ce_refs_match_torch(B, K, ncls):
    g = torch.Generator().manual_seed(B + K)
    h = torch.randn(B, K, generator=g, dtype=F64).requires_grad_(True)
    W = (torch.randn(ncls, K, generator=g, dtype=F64) * 0.2).requires_grad_(True)
    b = torch.randn(ncls, generator=g, dtype=F64).requires_grad_(True)
    labels = torch.randint(0, ncls, (B,), generator=g)
    glogits = torch.randn(B, ncls, generator=g, dtype=F64)
    logits = F.linear(h, W, b)
    loss = F.cross_entropy(logits, labels)
    logits.retain_grad()
    (2.0 * loss + (glogits * logits).sum()).backward()
    out = R.classifier_ce_ref(h.detach(), W.detach(), b.detach(), labels)
    close(out["logits"], logits.detach(), "logits")
    close(out["loss"], loss.detach().reshape(1), "loss")
    close(out["sample_loss"], F.cross_entropy(logits.detach(), labels, reduction="none"), "sample_loss")
    bw = R.classifier_ce_bwd_ref(h.detach(), W.detach(), logits.detach(), labels, torch.tensor([2.0]), glogits)
    close(bw["dlogits"], logits.grad, "dlogits")
    close(bw["dh"], h.grad, "dh")
    close(bw["dW"], W.grad, "dW")
    close(bw["db"], b.grad, "db")
    # without labels only the incoming logit gradient flows; the gate closes dh where h <= 0
    bw = R.classifier_ce_bwd_ref(h.detach(), W.detach(), logits.detach(), None, None, glogits, use_gate=1, gate_scale=1.25)
    close(bw["dlogits"], glogits, "dlogits, no labels")
    close(bw["dh"], torch.where(h.detach() > 0, (glogits @ W.detach()) * 1.25, torch.zeros_like(h.detach())), "gated dh")


def test_gelu_epilogue_matches_torch():
    g = torch.Generator().manual_seed(2)
    M, N, K = 33, 8, 64
    A, W, bias = torch.randn(M * K, generator=g, dtype=F64), torch.randn(N * K, generator=g, dtype=F64), torch.randn(N, generator=g, dtype=F64)
    res = torch.randn(M * N, generator=g, dtype=F64)
    out = R.gemm_nt_ref(A, W, M=M, N=N, K=K, a=(K, 0, 0), c=(N, 0, 0), bias=bias, residual=res, act=R.ACT_GELU,
                        C=torch.zeros(M * N, dtype=F64))
    ref = F.gelu(F.linear(A.view(M, K), W.view(N, K), bias)) + res.view(M, N)
    close(out["C"].view(M, N), ref, "gelu")


class PoolFuse(torch.nn.Module):
    """the reference model's cls slice, mean pools and symmetric-fusion operands (dual_eeg_transformer.py:1193-1223)"""

    def forward(self, z, B, off, n_ibs):
        z1, z2 = z[:B], z[B:]
        a, c = z1[:, 0], z2[:, 0]
        comb = torch.cat([a + c, a * c, torch.abs(a - c)], dim=1)
        pool = torch.cat([z1[:, off:].mean(dim=1), z2[:, off:].mean(dim=1)], dim=1)
        ibs = z1[:, 1:1 + n_ibs].mean(dim=1) if n_ibs else None
        return a, c, comb, pool, ibs


@pytest.mark.parametrize("B,S,D,off", R.POOL_CASES)
@pytest.mark.parametrize("n_ibs", R.POOL_IBS)
def test_pool_fuse_refs_match_a_torch_module(B, S, D, off, n_ibs):
    if n_ibs and 1 + n_ibs > S:
        n_ibs = S - 1
    t = {k: v.to(F64) for k, v in R.pool_case(B, S, D, off, "f32").items()}
    z = t["z"].clone().requires_grad_(True)
    a, c, comb, pool, ibs = PoolFuse()(z, B, off, n_ibs)
    ref = R.pool_fuse_fwd_ref(t["z"], B, off, n_ibs, 1)
    close(ref["cls1"], a.detach()), close(ref["cls2"], c.detach()), close(ref["comb"], comb.detach()), close(ref["pool"], pool.detach())
    loss = (t["dcomb"] * comb).sum() + (t["dzf"][:, D:] * pool).sum() + (t["gcls1"] * a).sum() + (t["gcls2"] * c).sum()
    if n_ibs:
        close(ref["ibs"], ibs.detach())
        loss = loss + ((t["dibs_pool"] + t["gibs_pool"]) * ibs).sum()
    loss.backward()
    assert int((t["z"][:B, 0] == t["z"][B:, 0]).sum()) >= 3          # the planted ties are there: torch's |.|' gives 0 on them
    opt = {k: t[k] for k in ("gcls1", "gcls2", "dibs_pool", "gibs_pool")}
    close(R.pool_fuse_bwd_ref(t["z"], t["dcomb"], t["dzf"], B, off, n_ibs, 1, **opt)["dz"], z.grad, "dz")


def test_row_mapped_gemm_is_conv1d():
    """strided Conv1d (k = 25, stride 4, padding 12) as a product over overlapping rows of a channel-last, zero-padded signal:
    the row map and row_off of gemm_nt_ref against F.conv1d"""
    NB, Cc, T, dm, k, s = 3, 8, 256, 16, 25, 4
    pad, K0 = k // 2, 256
    g = torch.Generator().manual_seed(5)
    x = torch.randn(NB, Cc, T, generator=g, dtype=F64)
    w = torch.randn(dm, Cc, k, generator=g, dtype=F64)
    b = torch.randn(dm, generator=g, dtype=F64)
    T1 = (T + 2 * pad - k) // s + 1
    Tp = max(T + 2 * pad, s * (T1 - 1) + K0 // Cc + 1)
    xt = torch.zeros(NB, Tp, Cc, dtype=F64)
    xt[:, pad:pad + T] = x.transpose(1, 2)
    wp = torch.zeros(dm, K0, dtype=F64)
    wp[:, :k * Cc] = w.permute(0, 2, 1).reshape(dm, k * Cc)          # tap-major, channel-minor
    M = NB * T1
    out = R.gemm_nt_ref(xt, wp, M=M, N=dm, K=K0, a=(s * Cc, Tp * Cc, T1), c=(dm, 0, 0), bias=b, act=R.ACT_RELU,
                        C=torch.zeros(M * dm, dtype=F64))
    ref = torch.relu(F.conv1d(x, w, b, stride=s, padding=pad)).transpose(1, 2).reshape(M, dm)
    close(out["C"].view(M, dm), ref, "conv1d")
    assert [int(v) for v in R.row_off((4, 100, 3), torch.arange(7))] == [0, 4, 8, 100, 104, 108, 200]
    assert [int(v) for v in R.row_off((5, 0, 0), torch.arange(3))] == [0, 5, 10]


def test_gemm_tn_ref_layout():
    g = torch.Generator().manual_seed(8)
    M, N, K = 9, 8, 256
    dY, X = torch.randn(M, N, generator=g, dtype=F64), torch.randn(M, K, generator=g, dtype=F64)
    slab, slack = R.gemm_tn_ref(dY, X, M=M, N=N, K=K, y=(N, 0, 0), x=(K, 0, 0), part_rows=4, has_bias=1)
    dW, db = dY.T @ X, dY.sum(0)
    want = torch.cat([dW[:4].reshape(-1), db[:4], dW[4:].reshape(-1), db[4:]])
    close(slab, want, "slab")
    assert slab.numel() == (N // 4) * (4 * K + 4) and bool((slack > 0).all())
    Xs = torch.zeros(M, 2, 192, dtype=F64)               # 128-column tiles 192 elements apart
    Xs[:, :, :128] = X.view(M, 2, 128)
    slab2, _ = R.gemm_tn_ref(dY, Xs, M=M, N=N, K=K, y=(N, 0, 0), x=(384, 0, 0), x_tile_stride=192)
    close(slab2, dW.reshape(-1), "x_tile_stride")


# ------------------------------------------------------------------------------------------------------
# 2. the comparator: accepts the rounded reference, rejects every defect, on the GPU tests' own tables
# ------------------------------------------------------------------------------------------------------
def test_comparator_leaves_no_element_out():
    ref = torch.ones(1000, dtype=F64)
    got = ref.clone()
    assert R.within(got, ref, U["bf16"], 0.0)[0]
    got[617] = 1.0 + 2.0 ** -7                       # ONE element two bf16 roundings off
    ok, msg = R.within(got, ref, U["bf16"], 0.0)
    assert not ok and "index 617" in msg and "slack" in msg
    got[617] = float("nan")
    assert not R.within(got, ref, U["bf16"], 0.0)[0]
    assert R.within(torch.tensor([2.0 ** -25]), torch.tensor([0.0]), U["fp16"], 0.0)[0]      # half an fp16 subnormal step
    assert not R.within(torch.tensor([2.0 ** -25]), torch.tensor([0.0]), U["bf16"], 0.0)[0]


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("name", list(R.GEMM_CASES))
def test_gemm_bounds_on_the_gpu_case_table(name, dtype):
    A, W, kw = R.gemm_case(name, dtype)
    res = R.gemm_nt_ref(A, W, **kw)
    ref = R.gemm_outputs(res, dtype)
    assert not R.rejects(stored(ref), ref), "the correctly rounded reference must hold"
    assert bool((res["C"][~res["written_C"]] == R.SENT).all())
    for defect in R.gemm_defects_for(name):
        bad = R.gemm_nt_ref(A, W, defect=defect, **kw)
        assert R.rejects(stored_as(bad, ref), ref), "%s passed the comparator" % defect


def test_every_gemm_defect_is_tried_somewhere():
    tried = {d for name in R.GEMM_CASES for d in R.gemm_defects_for(name)}
    assert tried == set(R.GEMM_DEFECTS)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("D,M,kind", R.NORM_CASES)
def test_norm_bounds_on_the_gpu_case_table(D, M, kind, dtype):
    x, gamma, beta, dy = R.norm_case(D, M, kind, dtype)
    ref = R.norm_fwd_outputs(x, gamma, beta, dtype)
    assert not R.rejects(stored(ref), ref)
    bad = R.norm_fwd_outputs(x, gamma, beta, dtype, defect="rstd_no_eps")
    assert R.rejects(stored_as(bad, ref), ref), "rstd without eps passed (the fp32 statistics show it in every dtype)"
    mean, rstd = ref["mean"][0].float(), ref["rstd"][0].float()              # as stored
    for d1, d2 in R.NORM_DROPS:                       # the block count is the launch's business, not the operation's
        refb = R.norm_bwd_outputs(dy, x, mean, rstd, gamma, d1, d2, dtype)
        assert not R.rejects(stored(refb), refb)
        defects = ["mask_shift", "no_drop_scale"] + (["drop2_at_drop1"] if d1[0] > 0 and d2[0] > 0 else [])
        for defect in defects:
            if D * M < 16 and defect != "no_drop_scale":
                continue                              # four elements: two masks may agree by chance
            badb = R.norm_bwd_outputs(dy, x, mean, rstd, gamma, d1, d2, dtype, defect=defect)
            assert R.rejects(stored_as(badb, refb), refb), "%s passed the comparator" % defect


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("B,S,D,off", R.POOL_CASES)
def test_pool_bounds_on_the_gpu_case_table(B, S, D, off, dtype):
    t = R.pool_case(B, S, D, off, dtype)
    for n_ibs in R.POOL_IBS:
        n_ibs = min(n_ibs, S - 1)
        ref = R.pool_fwd_outputs(t, B, off, n_ibs, dtype)
        assert not R.rejects(stored(ref), ref)
        for present in (set(), {"gcls1", "gcls2", "dibs_pool", "gibs_pool"}):
            refb = R.pool_bwd_outputs(t, B, off, n_ibs, present, dtype)
            assert not R.rejects(stored(refb), refb)
            bad = R.pool_bwd_outputs(t, B, off, n_ibs, present, dtype, defect="sign0_plus")
            assert R.rejects(stored_as(bad, refb), refb), "sign(0) = +1 passed the comparator"


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("B,K,ncls", R.CE_CASES)
def test_ce_bounds_on_the_gpu_case_table(B, K, ncls, dtype):
    t = R.ce_case(B, K, ncls, dtype)
    ref = R.ce_fwd_outputs(t, True)
    assert not R.rejects(stored(ref), ref)
    logits = ref["logits"][0].float()
    if B > 1 and ncls > 1:                            # one class: every loss is 0, and so is its mean
        assert R.rejects(stored_as(R.ce_fwd_outputs(t, True, defect="ce_no_mean"), ref), ref), "CE without its mean passed"
    for with_labels in (True, False):
        for with_glogits in (True, False):
            refb = R.ce_bwd_outputs(t, logits, with_labels, with_glogits, 1, dtype)
            assert not R.rejects(stored(refb), refb)
            if with_labels and B > 1 and ncls > 1:
                bad = R.ce_bwd_outputs(t, logits, with_labels, with_glogits, 1, dtype, defect="ce_no_mean")
                assert R.rejects(stored_as(bad, refb), refb), "dlogits without 1 / B passed"
            if (with_labels and ncls > 1) or with_glogits:
                bad = R.ce_bwd_outputs(t, logits, with_labels, with_glogits, 1, dtype, defect="no_gate_scale")
                assert R.rejects(stored_as(bad, refb), refb), "dh without gate_scale passed"
