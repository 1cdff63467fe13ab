"""fp64 statements of the ANCHOR kernels -- the kernels that the bit-equality tests of the fused routes copy -- and the one
comparator that holds a kernel's output to them.  CPU only: nothing here needs a GPU or the library.

Every reference takes its inputs ALREADY ROUNDED to the compute dtype (a bf16 tensor holds bf16 values; LayerNorm statistics,
biases, parameters and logits are fp32 values) and evaluates the operation in float64, in the order the header states it
(include/eyegaze_hip.h).  Every choice an operation makes -- the ReLU gate `> 0`, a dropout draw, sign(a - c) -- is decided on
stored values, identically on both sides, so the comparator needs no exclusion: no element is ever left out.

The comparator's bound per element is   1.5 * u * |ref| + slack   (+ 2^-25 absolute for fp16: half a subnormal step)
  u      one rounding of the stored result, the unit roundoff 2^-p of a format with p significand bits (the hidden one counted):
         2^-8 bf16 (p = 8), 2^-11 fp16 (p = 11), 2^-24 f32 (p = 24).  The plan for these tests named 2^-9 for bf16; that is half
         of bf16's unit roundoff and refuses the correctly rounded reference itself (4.0466 stores as 4.03125, 0.97 * 2^-8 off:
         tests/test_anchor_ref_host.py shows the rounded reference accepted at 2^-8 and every listed defect still rejected).
         The factor 1.5 covers the fp32 value that the kernel rounds being itself a rounded fp32 value (2^-24 << u / 2 for the
         16-bit types; for f32 the last operation IS the rounding)
  slack  the error of the fp32 arithmetic in front of that rounding.
         products: DERIVED.  A running fp32 sum of K terms t_k carries at most K * 2^-24 * sum |t_k| (first order); the order of
         the additions inside an MFMA is not documented, hence a factor 2:   2 K 2^-24 * s * (|A| |W|^T + |bias|),  s the product
         of the scale factors applied afterwards (gate_scale, 1 / (1 - p1), 1 / (1 - p2)).  16-bit products are exact in fp32
         (8 + 8 and 11 + 11 significand bits), fp32 products round once each, which the same bound covers with room (K + 1
         roundings against 2 K).  GELU: |d gelu / dv| <= 1.13 carries the accumulator's error through, and erff's own error
         (a few units of 2^-24 of 1 + erf <= 2, times |v| / 2) adds 16 * 2^-24 * |v|: both factors are stated in gemm_nt_ref.
         the rest: MEASURED on the CPU, never from the code under test: the same reference formula is evaluated in float32 (in
         three summation orders: torch's, reversed, sequential) and its largest error against float64, times 8, is the slack of
         that output of that case (f32_slack).  The assertion message carries it.
"""
import math

import numpy as np
import torch

from tests.helpers import hip_keep_mask

U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "f32": 2.0 ** -24}
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
EG = {"f32": 0, "bf16": 1, "fp16": 2}          # EG_F32, EG_BF16, EG_F16
DTYPES = ("bf16", "fp16", "f32")
SENT = 7.0                                      # what every output buffer holds where nothing may be written
F64 = torch.float64
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2


# ------------------------------------------------------------------------------------------------------
# the comparator
# ------------------------------------------------------------------------------------------------------
def within(got, ref, u, slack):
    """(ok, message): |got - ref| <= 1.5 u |ref| + slack for EVERY element (slack: a number or a tensor shaped as ref)."""
    got, ref = torch.as_tensor(got).to(F64), torch.as_tensor(ref).to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    slack_t = torch.as_tensor(slack).to(F64).expand_as(ref)
    bound = 1.5 * u * ref.abs() + slack_t
    if u == U["fp16"]:
        bound = bound + 2.0 ** -25
    err = (got - ref).abs()
    bad = ~(err <= bound)                       # a NaN on either side is bad
    if not bool(bad.any()):
        return True, ""
    i = int(torch.argmax(torch.where(bad, torch.nan_to_num(err - bound, nan=float("inf"), posinf=float("inf")),
                                     torch.full_like(err, -1.0)).flatten()))
    g, r, s = float(got.flatten()[i]), float(ref.flatten()[i]), float(slack_t.flatten()[i])
    return False, ("%d of %d elements outside 1.5 * %.3g * |ref| + slack; worst at flat index %d: got %.9g, ref %.9g, error %.3g, "
                   "slack %.3g (largest slack %.3g)" % (int(bad.sum()), bad.numel(), u, i, g, r, abs(g - r), s, float(slack_t.max())))


def assert_within(got, ref, u, slack, what=""):
    ok, msg = within(got, ref, u, slack)
    assert ok, "%s: %s" % (what, msg)


def assert_all_within(got, ref, what=""):
    """got: name -> tensor; ref: name -> (tensor, u, slack).  Every output of the reference must be present and hold."""
    for k, (r, u, s) in ref.items():
        assert_within(got[k], r, u, s, "%s %s" % (what, k))


def rejects(got, ref):
    """True when at least one output of `got` fails the comparator."""
    return any(not within(got[k], r, u, s)[0] for k, (r, u, s) in ref.items())


def rounded(t, dtype):
    """the values a store in `dtype` leaves behind, as float64"""
    return t.to(TDT[dtype]).to(F64)


# ------------------------------------------------------------------------------------------------------
# shared pieces: row maps, dropout, ordered sums
# ------------------------------------------------------------------------------------------------------
def row_off(m, r):
    """csrc/common.h row_off: m = (row_stride, group_stride, rows_per_group), r an int64 tensor of logical rows"""
    row_stride, group_stride, rows_per_group = m
    if rows_per_group <= 0:
        return r * row_stride
    g = torch.div(r, rows_per_group, rounding_mode="floor")
    return g * group_stride + (r - g * rows_per_group) * row_stride


def drop_scale(p):
    """make_drop's 1 / (1 - p), formed in fp32 on the host: a parameter of the operation, taken as stored"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def f32(v):
    return float(np.float32(v))


def keep_mask(seed, site, idx, p):
    """the kernel's keep decisions for element indices idx (int64 tensor) when the state was built with
    dev_state(seed=scramble_seed(seed)); p == 0 keeps everything"""
    if p <= 0:
        return torch.ones(idx.shape, dtype=torch.bool)
    flat = (idx.reshape(-1).numpy().astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    return torch.from_numpy(hip_keep_mask(seed, site, flat, p)).reshape(idx.shape)


def _sum(t, dim, order="torch"):
    """sum over `dim` (kept out of the result) in one of three orders; in float64 they agree to 1e-16, in float32 they sample
    the error a summation order may leave"""
    if order == "flip":
        return t.flip(dim).sum(dim)
    if order == "seq":
        return t.cumsum(dim).select(dim, t.shape[dim] - 1)
    return t.sum(dim)


ORDERS = ("torch", "flip", "seq")


def f32_slack(fn, ref64):
    """8 x the largest error, per output, of fn evaluated in float32 against the float64 outputs ref64 (name -> tensor)"""
    worst = {k: 0.0 for k in ref64}
    for order in ORDERS:
        out = fn(torch.float32, order)
        for k in ref64:
            e = (out[k].to(F64) - ref64[k]).abs()
            e = torch.nan_to_num(e, nan=0.0, posinf=0.0)       # a non-finite reference is compared as such, it needs no slack
            worst[k] = max(worst[k], float(e.max()) if e.numel() else 0.0)
    return {k: 8.0 * v for k, v in worst.items()}


# ------------------------------------------------------------------------------------------------------
# eg_gemm_nt
# ------------------------------------------------------------------------------------------------------
GEMM_DEFECTS = ("mask_shift", "drop2_at_drop1", "no_drop_scale", "no_gate_scale", "gate_ge", "pre_after_residual", "p_by_c",
                "physical_row_index")


def gemm_nt_ref(A, W, *, M, N, K, a, c, r=None, p=None, ldw=None, bias=None, residual=None, gate=None, C=None, out_pre=None,
                base=0, act=ACT_NONE, gate_scale=1.0, drop1=(0.0, 0), drop2=(0.0, 0), seed=0, a_seg_len=0, a_seg_stride=0,
                defect=None):
    """The header's epilogue, literally:  v = acc + bias; v = act(v); v = gate > 0 ? v * gate_scale : 0; v = drop1(v);
    v = drop2(v); out_pre = v; v += residual; C = v.
    A, W, residual, gate, C, out_pre are FLAT buffers (any dtype; C / out_pre as they stand before the launch).  Row m of A
    starts at row_off(a, m) and is K / a_seg_len runs of a_seg_len elements, a_seg_stride apart; W is [N, ldw]; row m of C and
    of gate starts at base + row_off(c, m), of residual at base + row_off(r, m), of out_pre at base + row_off(p, m) (`base`:
    the element offset of the pointer the descriptor carries into each of those buffers).  Dropout element index: m * N + n,
    m the LOGICAL row.  Returns flat float64 buffers C / out_pre, the slack of each element (0 where nothing is written),
    the masks of written elements, and `zero`: the written elements of C's rows that the gate or a dropout sets to exact 0
    in out_pre (in C too when there is no residual)."""
    assert defect is None or defect in GEMM_DEFECTS, defect
    r, p, ldw = r or c, p or c, ldw or K
    rows = torch.arange(M, dtype=torch.int64)
    cols = torch.arange(N, dtype=torch.int64)
    k = torch.arange(K, dtype=torch.int64)
    kcol = torch.div(k, a_seg_len, rounding_mode="floor") * a_seg_stride + k % a_seg_len if a_seg_len else k
    Ar = A.reshape(-1).to(F64)[row_off(a, rows)[:, None] + kcol[None, :]]
    Wr = W.reshape(-1).to(F64)[(cols * ldw)[:, None] + k[None, :]]
    v = Ar @ Wr.T
    mag = Ar.abs() @ Wr.abs().T
    if bias is not None:
        v = v + bias.to(F64)
        mag = mag + bias.to(F64).abs()
    err = 2.0 * K * 2.0 ** -24 * mag                     # of the fp32 accumulator plus bias
    if act == ACT_RELU:
        v = v.clamp_min(0.0)                             # Lipschitz 1, exact
    elif act == ACT_GELU:
        err = 1.13 * err + 16.0 * 2.0 ** -24 * v.abs()   # |gelu'| <= 1.13; erff and the two products (module docstring)
        v = 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))
    coff = base + row_off(c, rows)[:, None] + cols[None, :]
    s = 1.0
    zero = torch.zeros(M, N, dtype=torch.bool)
    if gate is not None:
        gv = gate.reshape(-1).to(F64)[coff]
        gs = 1.0 if defect == "no_gate_scale" else gate_scale
        open_ = gv >= 0 if defect == "gate_ge" else gv > 0
        v = torch.where(open_, v * gs, torch.zeros_like(v))
        zero |= ~(gv > 0)
        s *= gate_scale
    idx = rows[:, None] * N + cols[None, :]
    if defect == "physical_row_index":
        idx = coff - base
    if defect == "mask_shift":
        idx = idx + 2
    for j, (pp, site) in enumerate((drop1, drop2)):
        if pp > 0:
            if j == 1 and defect == "drop2_at_drop1":
                site = drop1[1]
            keep = keep_mask(seed, site, idx, pp)
            sc = 1.0 if defect == "no_drop_scale" else drop_scale(pp)
            v = torch.where(keep, v * sc, torch.zeros_like(v))
            true_site = (drop1, drop2)[j][1]
            zero |= ~keep_mask(seed, true_site, rows[:, None] * N + cols[None, :], pp)
            s *= drop_scale(pp)
    slack = s * err
    res = {}
    rv = residual.reshape(-1).to(F64)[base + row_off(r, rows)[:, None] + cols[None, :]] if residual is not None else None
    if out_pre is not None:
        P = out_pre.reshape(-1).to(F64).clone()
        poff = coff if defect == "p_by_c" else base + row_off(p, rows)[:, None] + cols[None, :]
        true_poff = base + row_off(p, rows)[:, None] + cols[None, :]
        P[poff] = v + rv if (defect == "pre_after_residual" and rv is not None) else v
        ps, pw = torch.zeros_like(P), torch.zeros(P.shape, dtype=torch.bool)
        ps[true_poff] = slack
        pw[true_poff] = True
        pz = torch.zeros(P.shape, dtype=torch.bool)
        pz[true_poff] = zero
        res.update(out_pre=P, slack_pre=ps, written_pre=pw, zero_pre=pz)
    if rv is not None:
        v = v + rv
    Cb = C.reshape(-1).to(F64).clone()
    Cb[coff] = v
    cs, cw, cz = torch.zeros_like(Cb), torch.zeros(Cb.shape, dtype=torch.bool), torch.zeros(Cb.shape, dtype=torch.bool)
    cs[coff] = slack
    cw[coff] = True
    if rv is None:
        cz[coff] = zero
    res.update(C=Cb, slack_C=cs, written_C=cw, zero_C=cz)
    return res


def gemm_outputs(res, dtype):
    """name -> (ref, u, slack) of a gemm_nt_ref result, for assert_all_within / rejects"""
    o = {"C": (res["C"], U[dtype], res["slack_C"])}
    if "out_pre" in res:
        o["out_pre"] = (res["out_pre"], U[dtype], res["slack_pre"])
    return o


def gemm_tn_ref(dY, X, *, M, N, K, y, x, x_tile_stride=0, part_rows=0, has_bias=0):
    """dW[n, k] = sum_m dY[m, n] X[m, k] and, with has_bias, db[n] = sum_m dY[m, n], in the slab layout of the header: N / part_rows
    parts of [part_rows x K weights | part_rows bias sums].  Element (m, k) of X lies at row_off(x, m) + (k / 128) * x_tile_stride
    + k % 128 (x_tile_stride 0 = 128 = contiguous).  Returns (slab, slack): the reduced slab as a flat float64 vector and the
    derived product slack with the sum running over M."""
    rows = torch.arange(M, dtype=torch.int64)
    k = torch.arange(K, dtype=torch.int64)
    ts = x_tile_stride or 128
    Yr = dY.reshape(-1).to(F64)[row_off(y, rows)[:, None] + torch.arange(N)[None, :]]
    Xr = X.reshape(-1).to(F64)[row_off(x, rows)[:, None] + (torch.div(k, 128, rounding_mode="floor") * ts + k % 128)[None, :]]
    dW, mag = Yr.T @ Xr, Yr.abs().T @ Xr.abs()
    db, magb = Yr.sum(0), Yr.abs().sum(0)
    pr = part_rows or N
    parts, slacks = [], []
    for q in range(N // pr):
        parts.append(dW[q * pr:(q + 1) * pr].reshape(-1))
        slacks.append(mag[q * pr:(q + 1) * pr].reshape(-1))
        if has_bias:
            parts.append(db[q * pr:(q + 1) * pr])
            slacks.append(magb[q * pr:(q + 1) * pr])
    return torch.cat(parts), 2.0 * M * 2.0 ** -24 * torch.cat(slacks)


# ------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------
NORM_DEFECTS = ("rstd_no_eps", "mask_shift", "drop2_at_drop1", "no_drop_scale")


def layernorm_ref(x, gamma, beta, eps=1e-5, dt=F64, order="torch", defect=None):
    """y = (x - mean) * rstd * gamma + beta over the last dim, biased variance, rstd = 1 / sqrt(var + eps): (y, mean, rstd)"""
    x, gamma, beta = x.to(dt), gamma.to(dt), beta.to(dt)
    D = x.shape[-1]
    mean = _sum(x, 1, order) / D
    d = x - mean[:, None]
    var = _sum(d * d, 1, order) / D
    rstd = 1.0 / torch.sqrt(var if defect == "rstd_no_eps" else var + eps)
    return d * rstd[:, None] * gamma + beta, mean, rstd


def layernorm_bwd_ref(dy, x, mean, rstd, gamma, drop1=(0.0, 0), drop2=(0.0, 0), seed=0, dt=F64, order="torch", defect=None):
    """LayerNorm backward from the STORED statistics (fp32 values): (dx, dx_drop, dgamma, dbeta) with
    dx_drop = drop1(drop2(dx)), dropout element index row * D + col.  With p == 0 at both sites dx_drop = dx."""
    dy, x, mean, rstd, gamma = dy.to(dt), x.to(dt), mean.to(dt), rstd.to(dt), gamma.to(dt)
    M, D = x.shape
    xh = (x - mean[:, None]) * rstd[:, None]
    dgamma, dbeta = _sum(dy * xh, 0, order), _sum(dy, 0, order)
    dxh = dy * gamma
    c1, c2 = _sum(dxh, 1, order) / D, _sum(dxh * xh, 1, order) / D
    dx = rstd[:, None] * (dxh - c1[:, None] - xh * c2[:, None])
    idx = torch.arange(M, dtype=torch.int64)[:, None] * D + torch.arange(D, dtype=torch.int64)[None, :]
    if defect == "mask_shift":
        idx = idx + 2
    dd = dx
    for j, (pp, site) in enumerate((drop1, drop2)):
        if pp > 0:
            if j == 1 and defect == "drop2_at_drop1":
                site = drop1[1]
            sc = 1.0 if defect == "no_drop_scale" else drop_scale(pp)
            dd = torch.where(keep_mask(seed, site, idx, pp), dd * sc, torch.zeros_like(dd))
    return dx, dd, dgamma, dbeta


def norm_keep(M, D, drop1, drop2, seed):
    """the elements of dx_drop that both sites keep"""
    idx = torch.arange(M, dtype=torch.int64)[:, None] * D + torch.arange(D, dtype=torch.int64)[None, :]
    return keep_mask(seed, drop1[1], idx, drop1[0]) & keep_mask(seed, drop2[1], idx, drop2[0])


# ------------------------------------------------------------------------------------------------------
# heads (csrc/heads.hip)
# ------------------------------------------------------------------------------------------------------
def pool_fuse_fwd_ref(z, B, off, n_ibs, ibs_first, dt=F64, order="torch"):
    """z [2 B, S, D], stream 1 = samples [0, B), stream 2 = [B, 2 B): cls1 / cls2 = z[:, 0] of each stream (copies), comb =
    [a + c | a * c | |a - c|], pool = [mean over s >= off of stream 1 | of stream 2] (what zf[:, D:3D] receives; zf[:, :D] is not
    written), ibs = mean over s in [ibs_first, ibs_first + n_ibs) of stream 1 (absent when n_ibs == 0)"""
    z = z.to(dt)
    z1, z2 = z[:B], z[B:]
    a, c = z1[:, 0], z2[:, 0]
    S = z.shape[1]
    out = dict(cls1=a, cls2=c, comb=torch.cat([a + c, a * c, (a - c).abs()], 1),
               pool=torch.cat([_sum(z1[:, off:], 1, order), _sum(z2[:, off:], 1, order)], 1) / (S - off))
    if n_ibs > 0:
        out["ibs"] = _sum(z1[:, ibs_first:ibs_first + n_ibs], 1, order) / n_ibs
    return out


def pool_fuse_bwd_ref(z, dcomb, dzf, B, off, n_ibs, ibs_first, gcls1=None, gcls2=None, dibs_pool=None, gibs_pool=None, dt=F64,
                      order="torch", defect=None):
    """the whole dz [2 B, S, D], zeros where nothing flows.  sign(a - c) is +1, -1 and, for a == c, 0."""
    z, dcomb, dzf = z.to(dt), dcomb.to(dt), dzf.to(dt)
    _, S, D = z.shape
    a, c = z[:B, 0], z[B:, 0]
    g0, g1, g2 = dcomb[:, :D], dcomb[:, D:2 * D], dcomb[:, 2 * D:]
    one = torch.ones((), dtype=dt)
    if defect == "sign0_plus":
        sg = torch.where(a >= c, one, -one)
    else:
        sg = torch.where(a > c, one, torch.where(a < c, -one, 0 * one))
    da = g0 + g1 * c + g2 * sg
    dc = g0 + g1 * a - g2 * sg
    if gcls1 is not None:
        da = da + gcls1.to(dt)
    if gcls2 is not None:
        dc = dc + gcls2.to(dt)
    dz = torch.zeros(2 * B, S, D, dtype=dt)
    dz[:B, 0], dz[B:, 0] = da, dc
    dz[:B, off:] += (dzf[:, D:2 * D] / (S - off))[:, None, :]
    dz[B:, off:] += (dzf[:, 2 * D:] / (S - off))[:, None, :]
    if n_ibs > 0:
        di = torch.zeros(B, D, dtype=dt)
        if dibs_pool is not None:
            di = di + dibs_pool.to(dt)
        if gibs_pool is not None:
            di = di + gibs_pool.to(dt)
        dz[:B, ibs_first:ibs_first + n_ibs] += (di / n_ibs)[:, None, :]
    return dict(dz=dz)


def classifier_ce_ref(h, W, bias, labels=None, dt=F64, order="torch", defect=None):
    """logits = h W^T + b; with labels the per-sample cross-entropy and its mean over B"""
    h, W, bias = h.to(dt), W.to(dt), bias.to(dt)
    logits = _sum(h[:, None, :] * W[None, :, :], 2, order) + bias
    out = dict(logits=logits)
    if labels is not None:
        mx = logits.max(1).values
        lse = mx + torch.log(_sum(torch.exp(logits - mx[:, None]), 1, order))
        sl = lse - logits.gather(1, labels[:, None])[:, 0]
        out.update(sample_loss=sl, loss=(_sum(sl, 0, order) if defect == "ce_no_mean" else _sum(sl, 0, order) / sl.shape[0]).reshape(1))
    return out


def classifier_ce_bwd_ref(h, W, logits, labels=None, gloss=None, glogits=None, use_gate=0, gate_scale=1.0, dt=F64, order="torch",
                          defect=None):
    """from the STORED logits: dlogits = gloss * (softmax - onehot) / B + glogits (the first term only with labels and gloss),
    dh = (dlogits W) gated by h > 0 and scaled by gate_scale when use_gate, dW = dlogits^T h, db = column sums of dlogits"""
    h, W, logits = h.to(dt), W.to(dt), logits.to(dt)
    B, ncls = logits.shape
    dl = torch.zeros(B, ncls, dtype=dt)
    if labels is not None and gloss is not None:
        e = torch.exp(logits - logits.max(1, keepdim=True).values)
        sm = e / _sum(e, 1, order)[:, None]
        onehot = torch.zeros(B, ncls, dtype=dt).scatter_(1, labels[:, None], 1.0)
        gl = float(gloss) if defect == "ce_no_mean" else float(gloss) / B
        dl = gl * (sm - onehot)
    if glogits is not None:
        dl = dl + glogits.to(dt)
    dh = _sum(dl[:, :, None] * W[None, :, :], 1, order)
    if use_gate:
        dh = torch.where(h > 0, dh * (1.0 if defect == "no_gate_scale" else gate_scale), torch.zeros_like(dh))
    return dict(dlogits=dl, dh=dh, dW=_sum(dl[:, :, None] * h[:, None, :], 0, order), db=_sum(dl, 0, order))


def batch_rowsum_ref(dseq, rows, dt=F64, order="torch"):
    """out[s, :] = sum over b of dseq[b, s, :] for s < rows"""
    return dict(out=_sum(dseq.to(dt)[:, :rows], 0, order))


def rows_gather_gate_ref(src, gate, dst, dmap, nb, R, off, pair_shift, gate_scale, dt=F64):
    """dst row b * R + r (at row_off(dmap, .) of the FLAT buffer dst, D elements) = (src[b, off + r] (+ src[b + pair_shift, off + r]))
    * (gate[b, r] > 0 ? gate_scale : 0), ungated when gate is None.  Returns (flat buffer, written mask)."""
    src = src.to(dt)
    D = src.shape[2]
    v = src[:nb, off:off + R]
    if pair_shift:
        v = v + src[pair_shift:pair_shift + nb, off:off + R]
    if gate is not None:
        v = torch.where(gate.to(dt).reshape(nb, R, D) > 0, v * gate_scale, torch.zeros_like(v))
    out = dst.reshape(-1).to(dt).clone()
    o = row_off(dmap, torch.arange(nb * R, dtype=torch.int64))[:, None] + torch.arange(D, dtype=torch.int64)[None, :]
    out[o] = v.reshape(nb * R, D)
    w = torch.zeros(out.shape, dtype=torch.bool)
    w[o] = True
    return out, w


def rows_bcast_ref(src, pos, seq, off, src_nb, dt=F64):
    """seq[b, off + r, :] = src[b % src_nb, r, :] + pos[off + r, :] (pos may be None); seq [NB, S, D] as it stands before"""
    out = seq.to(dt).clone()
    NB, R = seq.shape[0], src.shape[1]
    v = src.to(dt)[torch.arange(NB) % src_nb]
    if pos is not None:
        v = v + pos.to(dt)[off:off + R][None]
    out[:, off:off + R] = v
    return out


def rows_copy_ref(seq, R, off, b_src0, b_dst0, nb):
    """seq[b_dst0 + b, off + r, :] = seq[b_src0 + b, off + r, :]: a copy, exact in every dtype"""
    out = seq.clone()
    out[b_dst0:b_dst0 + nb, off:off + R] = seq[b_src0:b_src0 + nb, off:off + R]
    return out


# ------------------------------------------------------------------------------------------------------
# case tables (shared by the GPU tests and by the comparator's sensitivity test on the CPU)
# ------------------------------------------------------------------------------------------------------
ROUTE_TILED, ROUTE_WIDE, ROUTE_ROWSTREAM = 0, 1, 2
FULL = dict(bias=1, act=ACT_RELU, gate=1, gate_scale=1.25, drop1=(0.1, 5), drop2=(0.2, 6), out_pre=1, residual=1)
# name -> shape, the route a 16-bit call must take, the wide tile to force (0 = by rule), epilogue switches, layout switches
GEMM_CASES = {
    "tiled_full": dict(M=130, N=136, K=192, route=ROUTE_TILED, ldw_pad=8, strides=(2, 1, 3), **FULL),
    "tiled_gelu": dict(M=33, N=8, K=64, route=ROUTE_TILED, bias=1, act=ACT_GELU, residual=1),
    "tiled_grouped": dict(M=160, N=40, K=192, route=ROUTE_TILED, sliding=1, gate=1, gate_scale=1.25),
    "tiled_segmented": dict(M=300, N=64, K=192, route=ROUTE_TILED, a_seg_len=64, a_seg_stride=96, bias=1),
    "narrow_full": dict(M=1030, N=64, K=128, route=ROUTE_TILED, strides=(2, 1, 3), **FULL),
    "rowstream_relu_drop": dict(M=1037, N=512, K=256, route=ROUTE_ROWSTREAM, act=ACT_RELU, drop1=(0.2, 5), out_pre=1, residual=1,
                                strides=(2, 1, 3)),
    "rowstream_gate": dict(M=8, N=256, K=256, route=ROUTE_ROWSTREAM, gate=1, gate_scale=1.25),
    "rowstream_bias": dict(M=520, N=768, K=256, route=ROUTE_ROWSTREAM, bias=1),
    "wide128_drops": dict(M=1040, N=256, K=192, route=ROUTE_WIDE, tile=128, drop1=(0.1, 5), drop2=(0.2, 6), out_pre=1, residual=1,
                          strides=(2, 1, 3)),
    "wide160_drops": dict(M=1040, N=256, K=192, route=ROUTE_WIDE, tile=160, drop1=(0.1, 5), drop2=(0.2, 6), out_pre=1, residual=1,
                          strides=(2, 1, 3)),
    "wide_sliding_gate": dict(M=1040, N=256, K=448, route=ROUTE_WIDE, sliding=1, gate=1, gate_scale=1.25),
}
GUARD = 8          # sentinel rows (of the buffer's own row length) in front of and behind every output


def gemm_case(name, dtype, seed=0):
    """operands of GEMM_CASES[name] on the CPU, rounded to dtype, and the keyword arguments of gemm_nt_ref.  C, gate, residual
    and out_pre sit `base` elements into buffers that carry GUARD sentinel rows at both ends; c, r, p use three different row
    strides where the case asks for it (the gaps keep their sentinel)."""
    cs = GEMM_CASES[name]
    M, N, K = cs["M"], cs["N"], cs["K"]
    t = TDT[dtype]
    g = torch.Generator().manual_seed(1000 + seed + 7 * M + N + K)
    ldw = K + cs.get("ldw_pad", 0)
    if cs.get("sliding"):
        grp = 3 + K // 64                                 # rows of 64 elements; row j of a group of 4 reads K elements from its j-th row on
        A = (torch.randn(M // 4 * grp * 64, generator=g) * 0.5).to(t)
        a = (64, grp * 64, 4)
        c = (2 * N, 9 * N, 4)                             # every other row of groups of 9
        crows, clen = M // 4 * 9, N
    elif cs.get("a_seg_len"):
        lda = 2 * cs["a_seg_stride"] + cs["a_seg_len"] + 8
        A = (torch.randn(M * lda, generator=g) * 0.5).to(t)
        a, c, crows, clen = (lda, 0, 0), (N, 0, 0), M, N
    else:
        lda = K + 8
        A = (torch.randn(M * lda, generator=g) * 0.5).to(t)
        a, c, crows, clen = (lda, 0, 0), (N, 0, 0), M, N
    W = (torch.randn(N * ldw, generator=g) / math.sqrt(K)).to(t)
    A[torch.randint(0, A.numel(), (37,), generator=g)] = 0          # a few exact zeros
    W[torch.randint(0, W.numel(), (37,), generator=g)] = 0
    maps = {"c": c, "r": c, "p": c}
    lens = {"c": clen, "r": clen, "p": clen}
    if cs.get("strides"):
        for key, mul in zip("crp", cs["strides"]):
            lens[key] = mul * N + 8 * (mul - 1)           # row strides 2 N + 8 (C and the gate), N (residual), 3 N + 16 (out_pre): multiples of 8, all different
            maps[key] = (lens[key], 0, 0)

    def gate_values(n):
        v = torch.randn(n, generator=g)
        v[torch.randint(0, n, (n // 16,), generator=g)] = 0.0       # +0.0
        v[torch.randint(0, n, (n // 16,), generator=g)] = -0.0      # -0.0
        return v.to(t)
    # one base for every buffer: GUARD rows of the longest row, in front of and behind the rows of each
    base = GUARD * max(lens.values())
    kw = dict(M=M, N=N, K=K, a=a, c=maps["c"], r=maps["r"], p=maps["p"], ldw=ldw, base=base, act=cs.get("act", 0),
              gate_scale=cs.get("gate_scale", 1.0), drop1=cs.get("drop1", (0.0, 0)), drop2=cs.get("drop2", (0.0, 0)),
              seed=4321 + seed, a_seg_len=cs.get("a_seg_len", 0), a_seg_stride=cs.get("a_seg_stride", 0))

    def sized(key, fill=None):
        n = 2 * base + crows * lens[key]
        return torch.full((n,), SENT).to(t) if fill is None else fill(n)
    kw["C"] = sized("c")
    kw["bias"] = torch.randn(N, generator=g) if cs.get("bias") else None
    kw["residual"] = sized("r", lambda n: torch.randn(n, generator=g).to(t)) if cs.get("residual") else None
    kw["gate"] = sized("c", gate_values) if cs.get("gate") else None
    kw["out_pre"] = sized("p") if cs.get("out_pre") else None
    return A, W, kw


def gemm_defects_for(name):
    """the defects a case can show, from its switches alone"""
    cs = GEMM_CASES[name]
    drop, two = cs.get("drop1", (0, 0))[0] > 0, cs.get("drop2", (0, 0))[0] > 0
    out = []
    if drop:
        out += ["mask_shift", "no_drop_scale"]
    if drop and two:
        out.append("drop2_at_drop1")
    if cs.get("gate"):
        out += ["no_gate_scale", "gate_ge"]
    if cs.get("out_pre") and cs.get("residual"):
        out.append("pre_after_residual")
    if cs.get("out_pre") and cs.get("strides"):
        out.append("p_by_c")
    if drop and cs.get("strides"):
        out.append("physical_row_index")      # the C rows are further apart than N: their offsets are not m * N
    return out


# LayerNorm: (D, M, input kind); every case runs forward, then backward at every (nblk, drops) of NORM_NBLK x NORM_DROPS
NORM_CASES = [(D, M, "randn") for D in (4, 64, 100, 256, 1024) for M in (1, 130)] + [(256, 130, "offset"), (100, 130, "offset")]
NORM_NBLK = (1, 32, 200)                                                    # 200: more blocks than rows
NORM_DROPS = [((0.1, 5), (0.0, 0)), ((0.0, 0), (0.2, 6)), ((0.1, 5), (0.2, 6))]   # (drop1, drop2) as (p, site)
NORM_SEED = 99


def norm_case(D, M, kind, dtype):
    g = torch.Generator().manual_seed(31 * D + M)
    t = TDT[dtype]
    if kind == "offset":                              # row mean 100, spread 0.01: the cancellation case
        x = (100.0 + 0.01 * torch.randn(M, D, generator=g)).to(t)
    else:
        x = (torch.randn(M, D, generator=g) * 2 + 0.5).to(t)
    gamma, beta = torch.randn(D, generator=g) * 0.5 + 1, torch.randn(D, generator=g) * 0.5
    dy = torch.randn(M, D, generator=g).to(t)
    return x, gamma, beta, dy


def norm_fwd_outputs(x, gamma, beta, dtype, defect=None):
    """name -> (ref, u, slack) of the forward; the statistics are fp32 whatever the dtype"""
    y, mean, rstd = layernorm_ref(x, gamma, beta, defect=defect)
    ref = dict(y=y, mean=mean, rstd=rstd)
    if defect is not None:
        return ref
    sl = f32_slack(lambda dt, order: dict(zip(("y", "mean", "rstd"), layernorm_ref(x, gamma, beta, dt=dt, order=order))), ref)
    return {"y": (y, U[dtype], sl["y"]), "mean": (mean, U["f32"], sl["mean"]), "rstd": (rstd, U["f32"], sl["rstd"])}


def norm_bwd_outputs(dy, x, mean, rstd, gamma, drop1, drop2, dtype, defect=None):
    names = ("dx", "dx_drop", "dgamma", "dbeta")
    ref = dict(zip(names, layernorm_bwd_ref(dy, x, mean, rstd, gamma, drop1, drop2, NORM_SEED, defect=defect)))
    if defect is not None:
        return ref
    sl = f32_slack(lambda dt, order: dict(zip(names, layernorm_bwd_ref(dy, x, mean, rstd, gamma, drop1, drop2, NORM_SEED, dt=dt,
                                                                       order=order))), ref)
    return {k: (ref[k], U[dtype] if k in ("dx", "dx_drop") else U["f32"], sl[k]) for k in names}


# heads
POOL_CASES = [(1, 3, 64, 1), (5, 20, 256, 5), (17, 65, 96, 9)]          # (B, S, D, off)
POOL_IBS = (0, 3)
CE_CASES = [(B, K, ncls) for B in (1, 5, 33) for K in (64, 200, 256) for ncls in (1, 3, 16)]
CE_GATE_SCALE = f32(1.0 / 0.9)


def pool_case(B, S, D, off, dtype):
    g = torch.Generator().manual_seed(B * 1000 + S * 10 + off)
    t = TDT[dtype]
    z = torch.randn(2 * B, S, D, generator=g).to(t)
    ties = torch.randint(0, D, (max(3, D // 8),), generator=g)
    z[B:, 0, ties] = z[:B, 0, ties]                    # a == c: sign(a - c) = 0
    r16 = lambda *s: torch.randn(*s, generator=g).to(t)
    r32 = lambda *s: torch.randn(*s, generator=g)
    return dict(z=z, dcomb=r16(B, 3 * D), dzf=r16(B, 3 * D), gcls1=r32(B, D), gcls2=r32(B, D), dibs_pool=r16(B, D), gibs_pool=r32(B, D))


def pool_fwd_outputs(t, B, off, n_ibs, dtype):
    ref = pool_fuse_fwd_ref(t["z"], B, off, n_ibs, 1)
    sl = f32_slack(lambda dt, order: pool_fuse_fwd_ref(t["z"], B, off, n_ibs, 1, dt=dt, order=order), ref)
    us = dict(cls1=0.0, cls2=0.0, comb=U[dtype], pool=U[dtype], ibs=U[dtype])
    out = {k: (ref[k], us[k], 0.0 if k in ("cls1", "cls2") else sl[k]) for k in ref}
    if n_ibs:
        out["ibs_f32"] = (ref["ibs"], U["f32"], sl["ibs"])
    return out


def pool_bwd_outputs(t, B, off, n_ibs, present, dtype, defect=None):
    """present: the optional incoming gradients that are given (a set of names)"""
    opt = {k: (t[k] if k in present else None) for k in ("gcls1", "gcls2", "dibs_pool", "gibs_pool")}
    ref = pool_fuse_bwd_ref(t["z"], t["dcomb"], t["dzf"], B, off, n_ibs, 1, defect=defect, **opt)
    if defect is not None:
        return ref
    sl = f32_slack(lambda dt, order: pool_fuse_bwd_ref(t["z"], t["dcomb"], t["dzf"], B, off, n_ibs, 1, dt=dt, order=order, **opt), ref)
    return {"dz": (ref["dz"], U[dtype], sl["dz"])}


def ce_case(B, K, ncls, dtype):
    g = torch.Generator().manual_seed(B * 100 + K + ncls)
    h = torch.randn(B, K, generator=g).to(TDT[dtype])
    h[:, ::7] = 0.0                                    # gate: exact zeros close the gate
    return dict(h=h, W=torch.randn(ncls, K, generator=g) * 0.2, bias=torch.randn(ncls, generator=g) * 0.1,
                labels=torch.randint(0, ncls, (B,), generator=g), glogits=torch.randn(B, ncls, generator=g) * 0.1,
                gloss=torch.tensor([2.0]))


def ce_fwd_outputs(t, with_labels, defect=None):
    lab = t["labels"] if with_labels else None
    ref = classifier_ce_ref(t["h"], t["W"], t["bias"], lab, defect=defect)
    if defect is not None:
        return ref
    sl = f32_slack(lambda dt, order: classifier_ce_ref(t["h"], t["W"], t["bias"], lab, dt=dt, order=order), ref)
    return {k: (ref[k], U["f32"], sl[k]) for k in ref}


def ce_bwd_outputs(t, logits, with_labels, with_glogits, use_gate, dtype, defect=None):
    kw = dict(labels=t["labels"] if with_labels else None, gloss=t["gloss"] if with_labels else None,
              glogits=t["glogits"] if with_glogits else None, use_gate=use_gate, gate_scale=CE_GATE_SCALE)
    ref = classifier_ce_bwd_ref(t["h"], t["W"], logits, defect=defect, **kw)
    if defect is not None:
        return ref
    sl = f32_slack(lambda dt, order: classifier_ce_bwd_ref(t["h"], t["W"], logits, dt=dt, order=order, **kw), ref)
    return {k: (ref[k], U[dtype] if k == "dh" else U["f32"], sl[k]) for k in ref}
