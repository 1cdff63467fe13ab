"""fp64 statement of the attention cores (csrc/attention.hip, csrc/attention_long.hip), the elementwise bounds that hold a kernel
to it, the inputs on which a wrong kernel shows, and two fp32 CPU emulations of the kernels' arithmetic.  CPU only.

The operation, over the fused buffer qkv [NB*S, 3*H*hd] (row = window * S + token; columns [Q | K | V], each H heads of hd):
    s = Q K^T / sqrt(hd) of query window b against key / value window (b + kv_shift) % NB,   lse = logsumexp_k s,
    P = exp(s - lse),   M = keep / (1 - p) (all ones without dropout),   o = (P o M) V,
    delta = rowsum(dO o o),   dP = dO V^T,   dS = P o (M o dP - delta),
    dQ = dS K / sqrt(hd),   dK = dS^T Q / sqrt(hd),   dV = (P o M)^T dO,   dK / dV stored in window (b + kv_shift) % NB.
Inputs are taken ALREADY ROUNDED to the compute dtype; 1 / (1 - p) is the fp32 value the host forms (anchor_ref.drop_scale).

The bound of every output element is derived to first order from where the kernels round (u: unit roundoff of the stored type,
u_P = u in 16 bit -- P o M, and dS, are rounded to the 16-bit type in front of their MFMAs: attention.hip:127 / :237 / :242-243,
attention_long.hip:159 / :303-304 / :388 -- and 0 in f32; e = 2^-24):
    scores   ds_  = 2 hd e scale (|Q| |K|^T) + 2 e |s|                 the fp32 dot product (any order) and its scaling
    rho[q]        = 2 max_k ds_ + 2^-20 (2 + max_k |s - lse|)          relative error of a recomputed / normalised probability
    lse           : 2 e |lse| + 2 max_k ds_ + 2^-19
    ctx           : 1.5 u |o| + (u_P + rho + 2 S e) (P~ |V|),  P~ = P o M
    delta         : Dd[q] = sum_d |dO| tol_ctx + 2 hd e sum_d |dO o|   (delta is taken from the STORED ctx)
    dP            : DdP = 2 hd e (|dO| |V|^T)
    dS            : DdS = (rho + u_P) |dS| + P o (M o DdP + Dd) + rho P o (|M o dP| + |delta|)
    dQ            : 1.5 u |dQ| + scale (DdS |K|) + 2 S e scale (|dS| |K|);     dK: the same with DdS^T |Q|
    dV            : 1.5 u |dV| + sum_q (u_P + rho[q] + 2 S e) P~[q, k] |dO[q]|
    fp16 only     : a 16-bit rounding is also off by up to eta = 2^-25 absolutely (half the smallest subnormal): 1.5 u |x| becomes
                    max(1.5 u |x|, eta) for the stored outputs, eta (M |V|) is added to ctx, eta (M^T |dO|) to dV, eta scale sum |K|
                    to dQ and eta scale sum |Q| to dK (the rounded P o M and dS operands).
No blanket factor, no element left out.  tests/test_attn_ref_host.py shows both emulations accepted on the GPU test's own case
table and each listed defect rejected by a named case.
"""
import math

import numpy as np
import torch

from tests.anchor_ref import DTYPES, F64, TDT, U, drop_scale
from tests.dropout64 import hip_keep_mask64

E24 = 2.0 ** -24
ETA = 2.0 ** -25
NAMES = ("ctx", "lse", "dq", "dk", "dv")


def f32v(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------------
def to_heads(rows, NB, S, H, hd):
    """[NB*S, H*hd] -> [NB, H, S, hd]"""
    return rows.reshape(NB, S, H, hd).permute(0, 2, 1, 3)


def to_rows(x):
    """[NB, H, S, hd] -> [NB*S, H*hd]"""
    NB, H, S, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(NB * S, H * hd)


def split_qkv(qkv, NB, S, H, hd):
    """(Q, K, V) of the fused buffer, each [NB, H, S, hd], every one in ITS OWN window"""
    x = qkv.reshape(NB, S, 3, H, hd)
    return tuple(x[:, :, i].permute(0, 2, 1, 3) for i in range(3))


def kv_index(NB, kv_shift):
    return (torch.arange(NB) + kv_shift) % NB


def attn_keep(NB, H, S, seed, site, p, pitch=None, shift=0):
    """the kernels' keep decisions [NB, H, S, S] for a state built with dev_state(seed=scramble_seed(seed)): element index
    ((w H + h) S + q) Sp2 + key, Sp2 = (S + 1) & ~1.  `pitch` / `shift` build the wrong masks of the host test's defects."""
    if p <= 0:
        return torch.ones(NB, H, S, S, dtype=torch.bool)
    pitch = ((S + 1) & ~1) if pitch is None else pitch
    row = np.arange(NB * H * S, dtype=np.uint64).reshape(NB, H, S, 1)
    idx = row * np.uint64(pitch) + np.arange(S, dtype=np.uint64).reshape(1, 1, 1, S) + np.uint64(shift)
    return torch.from_numpy(hip_keep_mask64(seed, site, idx, p))


# ------------------------------------------------------------------------------------------------------
# the fp64 statement and its bounds
# ------------------------------------------------------------------------------------------------------
def attention_ref(qkv, dO, NB, S, H, hd, kv_shift, keep=None, p=0.0):
    """Closed form in float64.  Returns a dict: ctx, dq, dk, dv [NB, H, S, hd] (dk / dv in the window they are stored in), lse
    [NB, H, S], the row-layout o [NB*S, H*hd] and dqkv [NB*S, 3*H*hd], and the intermediates the bounds are made of."""
    assert hd in (32, 64)
    scale = 1.0 / math.sqrt(hd)
    q, k, v = (t.to(F64) for t in split_qkv(qkv, NB, S, H, hd))
    idx = kv_index(NB, kv_shift)
    k, v = k[idx], v[idx]
    g = to_heads(dO.to(F64), NB, S, H, hd)
    s = (q @ k.mT) * scale
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    M = torch.ones_like(P) if keep is None or p <= 0 else keep.to(F64) * drop_scale(p)
    Pt = P * M
    o = Pt @ v
    delta = (g * o).sum(-1)
    dP = g @ v.mT
    dS = P * (M * dP - delta[..., None])
    dq = (dS @ k) * scale
    dk_pair, dv_pair = (dS.mT @ q) * scale, Pt.mT @ g
    dk, dv = torch.zeros_like(dk_pair), torch.zeros_like(dv_pair)
    dk[idx], dv[idx] = dk_pair, dv_pair
    dqkv = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(NB * S, 3 * H * hd)
    return dict(ctx=o, lse=lse, dq=dq, dk=dk, dv=dv, o=to_rows(o), dqkv=dqkv, q=q, k=k, v=v, g=g, s=s, P=P, M=M, dP=dP, dS=dS,
                delta=delta, idx=idx, S=S, hd=hd, scale=scale)


def bounds(r, dtype):
    """name -> elementwise tolerance (shaped as the reference) of ctx, lse, dq, dk, dv: the module docstring, term by term.
    Also 'rho' [NB, H, S], which the probabilities' bound uses."""
    u = U[dtype]
    uP = 0.0 if dtype == "f32" else u
    eta = ETA if dtype == "fp16" else 0.0
    S, hd, scale = r["S"], r["hd"], r["scale"]
    q, k, v, g, s, P, M, lse = (r[n] for n in ("q", "k", "v", "g", "s", "P", "M", "lse"))
    aq, ak, av, ag = q.abs(), k.abs(), v.abs(), g.abs()

    def st(x):                                   # one rounding of a stored output
        return torch.clamp(1.5 * u * x.abs(), min=eta)
    ds_ = 2 * hd * E24 * scale * (aq @ ak.mT) + 2 * E24 * s.abs()
    mds = ds_.amax(-1)
    rho = 2 * mds + 2.0 ** -20 * (2 + (s - lse[..., None]).abs().amax(-1))
    tol_lse = 2 * E24 * lse.abs() + 2 * mds + 2.0 ** -19
    Pt = P * M
    rel = (uP + rho + 2 * S * E24)[..., None]                       # per query
    tol_ctx = st(r["ctx"]) + rel * (Pt @ av) + eta * (M @ av)
    Dd = (ag * tol_ctx).sum(-1) + 2 * hd * E24 * (g * r["ctx"]).abs().sum(-1)
    DdP = 2 * hd * E24 * (ag @ av.mT)
    dS, dP, delta = r["dS"], r["dP"], r["delta"]
    DdS = ((rho + uP)[..., None] * dS.abs() + P * (M * DdP + Dd[..., None])
           + rho[..., None] * P * ((M * dP).abs() + delta.abs()[..., None]))
    acc = 2 * S * E24 * scale
    tol_dq = scale * (DdS @ ak) + acc * (dS.abs() @ ak) + eta * scale * ak.sum(-2, keepdim=True)
    tol_dk = scale * (DdS.mT @ aq) + acc * (dS.abs().mT @ aq) + eta * scale * aq.sum(-2, keepdim=True)
    tol_dv = (rel * Pt).mT @ ag + eta * (M.mT @ ag)
    land_k, land_v = torch.zeros_like(tol_dk), torch.zeros_like(tol_dv)
    land_k[r["idx"]], land_v[r["idx"]] = tol_dk, tol_dv
    return dict(ctx=tol_ctx, lse=tol_lse, dq=st(r["dq"]) + tol_dq, dk=st(r["dk"]) + land_k, dv=st(r["dv"]) + land_v, rho=rho)


def probs_ref(r, dtype):
    """(ref, tol) of the probabilities kernels: the fp64 soft-max P within rho P + 2^-24 P.  The kernels evaluate exp(s - lse) from
    the lse array they are given; its error (the lse bound, about rho) is part of rho's 2 max_k ds_ + 2^-20 (...) here, and the GPU
    test feeds the forward's lse, itself held to its bound."""
    return r["P"], (bounds(r, dtype)["rho"][..., None] + E24) * r["P"]


# ------------------------------------------------------------------------------------------------------
# the one comparator
# ------------------------------------------------------------------------------------------------------
AXES = {"ctx": "query", "dq": "query", "dk": "key", "dv": "key", "lse": "query", "probs": "query"}


def compare(got, ref, tol, what, name):
    """(ratio, message): the worst err / tol over EVERY element (inf where a non-zero error meets a zero bound, or a NaN), and,
    when it exceeds 1, a message naming route / case, the output, the worst element's indices and its figures"""
    got, ref, tol = got.to(F64), ref.to(F64), tol.to(F64).expand_as(ref)
    assert got.shape == ref.shape, (what, name, got.shape, ref.shape)
    err = (got - ref).abs()
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)          # an exact element holds at a zero bound
    ratio = torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf"))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst <= 1.0:
        return worst, ""
    i = np.unravel_index(int(torch.argmax(ratio)), ratio.shape)
    labels = ("window", "head", AXES.get(name, "row"), "key" if name == "probs" else "column")
    where = ", ".join("%s %d" % (lab, j) for lab, j in zip(labels, i))
    return worst, ("%s %s: %d of %d elements outside their bound; worst at (%s): got %.9g, ref %.9g, error %.3g, bound %.3g, "
                   "err/tol %.3g" % (what, name, int((ratio > 1).sum()), ratio.numel(), where, float(got[i]), float(ref[i]),
                                     float(err[i]), float(tol[i]), worst))


def compare_all(got, r, tol, what, names=NAMES):
    """name -> err/tol of every output, and the messages of those that fail"""
    ratios, msgs = {}, []
    for n in names:
        ratios[n], m = compare(got[n], r[n], tol[n], what, n)
        if m:
            msgs.append(m)
    return ratios, msgs


def outputs_from_rows(ctx_rows, lse, dqkv_rows, NB, S, H, hd):
    """the kernels' buffers (any dtype, on the CPU) in the layout of the reference"""
    x = dqkv_rows.to(F64).reshape(NB, S, 3, H, hd)
    dq, dk, dv = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    return dict(ctx=to_heads(ctx_rows.to(F64), NB, S, H, hd), lse=lse.to(F64).reshape(NB, H, S), dq=dq, dk=dk, dv=dv)


# ------------------------------------------------------------------------------------------------------
# input classes (seeded, rounded to the dtype before use) and the case table of the GPU test
# ------------------------------------------------------------------------------------------------------
CLASSES = ("randn", "neg", "peak", "rise", "high", "gradscale")
HIGH_C = {32: 10.0, 64: 8.375}          # hd / 8 coordinates of q and of k at c: scores near 70.7 / 70.1 (both exact in bf16)


def make_inputs(cls, NB, S, H, hd, dtype, seed):
    """(qkv [NB*S, 3*H*hd], dO [NB*S, H*hd]) as tensors of the dtype"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda sc=1.0: torch.randn(NB, H, S, hd, generator=g) * sc
    nc = hd // 8
    if cls in ("randn", "gradscale"):
        q, k = rn(), rn()
    elif cls == "neg":                   # scores -11.3 (hd 32) / -16 (hd 64) + small noise: an admitted padded score 0 dominates
        q, k = rn(0.25), rn(0.25)
        q[..., :nc], k[..., :nc] = 4.0, -4.0
    elif cls == "peak":
        q, k = rn(3.0), rn(3.0)
    elif cls == "rise":                  # a ramp along the key index, and the last key well above it: the row maximum IS the last key
        q, k = rn(0.25), rn(0.25)
        q[..., 0] = 4.0
        k[..., 0] = 8.0 * torch.arange(1, S + 1) / S
        k[..., S - 1, 0] += 1.0
    elif cls == "high":
        q, k = rn(0.75), rn(0.75)
        q[..., :nc], k[..., :nc] = HIGH_C[hd], HIGH_C[hd]
    else:
        raise KeyError(cls)
    v, dO = rn(), rn(1024.0 if cls == "gradscale" else 1.0)
    qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(NB * S, 3 * H * hd)
    return qkv.to(TDT[dtype]), to_rows(dO).to(TDT[dtype])


def check_class(cls, r):
    """the property that names the class, asserted on the fp64 reference of the ROUNDED inputs"""
    s = r["s"]
    if cls == "neg":
        assert float(s.max()) <= -8.0, float(s.max())
    elif cls == "peak":
        assert float(s.abs().max()) > 25.0 and float(r["P"].amax(-1).median()) > 0.5
    elif cls == "rise":
        assert bool((s.argmax(-1) == r["S"] - 1).all())
    elif cls == "high":
        assert 60.0 <= float(s.min()) and float(s.max()) <= 80.0, (float(s.min()), float(s.max()))
    elif cls == "gradscale":
        assert float(r["dS"].abs().max()) < 2.0 ** 15, float(r["dS"].abs().max())


SHAPES = ((1, 1), (2, 2), (2, 0))        # (H, kv_shift) at NB = 3: NB * H odd at H = 1, kv_shift 1 and 2 are each other's inverse
SHORT_RANDN = (1, 2, 17, 65, 80, 81, 96, 97, 113, 128, 129, 145, 160)
SHORT_OTHER = (65, 97, 160)
LONG_RANDN = (1, 63, 64, 65, 129, 203, 333)
LONG_OTHER = (65, 129, 203)
DK_RANDN = (1, 65, 128, 129, 203)
DK_OTHER = (65, 129)
DROP_S = {"short": (17, 113, 160), "long": (129, 203), "dk": (65,)}
DROP_P = 0.25
HD = {"short": 32, "long": 32, "dk": 64}


def _table():
    cases = {}

    def add(route, cls, S, p=0.0, NB=3, shape=None):
        i = len(cases)
        H, sh = shape or SHAPES[i % 3]
        name = "%s-%s-S%d%s" % (route, cls, S, "-drop" if p else "")
        cases[name] = dict(route=route, cls=cls, S=S, NB=NB, H=H, kv_shift=sh, hd=HD[route], p=p, site=3 + i % 5, seed=4000 + i)
    for route, rand, other in (("short", SHORT_RANDN, SHORT_OTHER), ("long", LONG_RANDN, LONG_OTHER), ("dk", DK_RANDN, DK_OTHER)):
        for S in rand:
            add(route, "randn", S)
        for cls in CLASSES[1:]:
            for S in other:
                add(route, cls, S)
        for S in DROP_S[route]:
            add(route, "randn", S, p=DROP_P)
        add(route, "peak", 65, p=DROP_P)                   # rows whose dominant key is dropped: outputs near 1e-6, the fp16 floor eta
    add("long", "rise", 1024, NB=1, shape=(1, 0))          # sixteen tiles of rising maxima
    return cases


CASES = _table()
PROBS_CASES = {"%s-%s-S%d" % (route, cls, S): dict(route=route, cls=cls, S=S, NB=3, H=1, kv_shift=1, hd=HD[route], seed=7000 + j)
               for j, (route, S) in enumerate((("short", 97), ("long", 129), ("dk", 65))) for cls in ("neg", "high")}


def case_dtypes(name):
    """gradscale exists in fp16 only: that is where a scaled loss is used"""
    return ("fp16",) if "gradscale" in name else DTYPES


def case_ids():
    return [(n, d) for n in CASES for d in case_dtypes(n)]


def build_case(cs, dtype):
    """(qkv, dO, keep or None, reference, bounds) of a case; the class property is asserted on the way"""
    NB, S, H, hd = cs["NB"], cs["S"], cs["H"], cs["hd"]
    qkv, dO = make_inputs(cs["cls"], NB, S, H, hd, dtype, cs["seed"])
    keep = attn_keep(NB, H, S, cs["seed"], cs["site"], cs["p"]) if cs.get("p") else None
    r = attention_ref(qkv, dO, NB, S, H, hd, cs["kv_shift"], keep, cs.get("p", 0.0))
    check_class(cs["cls"], r)
    return qkv, dO, keep, r, bounds(r, dtype)


# ------------------------------------------------------------------------------------------------------
# fp32 emulations of the kernels' arithmetic, with the 16-bit roundings at the kernels' sites (for the host test only)
# ------------------------------------------------------------------------------------------------------
DEFECTS = ("pad_key", "no_rescale_sum", "no_rescale_out", "lse_no_max", "dkdv_window", "mask_pitch", "mask_shift", "no_dp_scale",
           "delta_undropped", "scale32_at_64")
LT = 64                                   # keys per tile of the long core


def emulate(route, qkv, dO, NB, S, H, hd, kv_shift, dtype, keep=None, p=0.0, defect=None):
    """float32 arithmetic of the short core (route 'short': normalise, mask, round P o M) or the long core ('long', 'dk': 64-key
    tiles, running max, unnormalised rounded p, o *= alpha, final 1 / l); the backward rounds P o M and dS in both.  Returns the
    stored outputs as float64 in the reference's layout.  `defect`: one of DEFECTS (the two mask defects are a wrong `keep`)."""
    assert defect is None or defect in DEFECTS, defect
    f = torch.float32
    rnd = (lambda x: x) if dtype == "f32" else (lambda x: x.to(TDT[dtype]).to(f))
    scale = f32v(1.0 / math.sqrt(32 if defect == "scale32_at_64" else hd))
    q, k, v = (t.to(f) for t in split_qkv(qkv, NB, S, H, hd))
    idx = kv_index(NB, kv_shift)
    k, v = k[idx], v[idx]
    g = to_heads(dO.to(f), NB, S, H, hd)
    dsc = f32v(drop_scale(p)) if p > 0 else 1.0
    M = torch.ones(NB, H, S, S, dtype=f) if keep is None or p <= 0 else keep.to(f) * dsc
    s = (q @ k.mT) * scale
    pad = defect == "pad_key" and S % (16 if route == "short" else LT) != 0       # one padded key of the last tile at score 0
    if route == "short":
        sx = torch.cat([s, torch.zeros(NB, H, S, 1)], -1) if pad else s
        mx = sx.amax(-1)
        ex = torch.exp(sx - mx[..., None])
        tot = ex.sum(-1)
        lse = (torch.log(tot) if defect == "lse_no_max" else mx + torch.log(tot))
        Pm = rnd(ex[..., :S] * (1.0 / tot)[..., None] * M)
        ctx = rnd(Pm @ v)
    else:
        m = torch.full((NB, H, S), -float("inf"))
        l = torch.zeros(NB, H, S)
        o = torch.zeros(NB, H, S, hd)
        for k0 in range(0, S, LT):
            st = s[..., k0:k0 + LT]
            last = k0 + LT >= S
            sx = torch.cat([st, torch.zeros(NB, H, S, 1)], -1) if (pad and last) else st
            mnew = torch.maximum(m, sx.amax(-1))
            alpha = torch.exp(m - mnew)
            px = torch.exp(sx - mnew[..., None])
            l = (l if defect == "no_rescale_sum" else l * alpha) + px.sum(-1)
            if defect != "no_rescale_out":
                o = o * alpha[..., None]
            o = o + rnd(px[..., :st.shape[-1]] * M[..., k0:k0 + LT]) @ v[..., k0:k0 + LT, :]
            m = mnew
        lse = (torch.log(l) if defect == "lse_no_max" else m + torch.log(l))
        ctx = rnd(o * (1.0 / l)[..., None])
    # backward, from the stored ctx and lse
    delta = (g * (rnd((torch.softmax(s, -1)) @ v) if defect == "delta_undropped" else ctx)).sum(-1)
    pr = torch.exp(s - lse[..., None])
    Mb = keep.to(f) if (defect == "no_dp_scale" and keep is not None) else M
    pd = rnd(pr * M)
    dS = rnd(pr * ((g @ v.mT) * Mb - delta[..., None]))
    dq = rnd((dS @ k) * scale)
    dk_pair, dv_pair = rnd((dS.mT @ q) * scale), rnd(pd.mT @ g)
    land = kv_index(NB, NB - kv_shift if defect == "dkdv_window" else kv_shift)
    dk, dv = torch.zeros_like(dk_pair), torch.zeros_like(dv_pair)
    dk[land], dv[land] = dk_pair, dv_pair
    return {n: t.to(F64) for n, t in dict(ctx=ctx, lse=lse, dq=dq, dk=dk, dv=dv).items()}

