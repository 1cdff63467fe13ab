"""tests/attn_ref.py on the CPU: (1) the closed-form fp64 attention forward and backward is torch autograd's to 1e-12, with and
without a keep mask, at both head widths and every window pairing of NB = 3; (2) on the GPU test's own case table
(attn_ref.CASES) and in every dtype, the bounds accept the fp32 emulation of the route's arithmetic -- 16-bit roundings of P o M
and dS where the kernels round them, running-max tiling for the long cores -- with no element left out; (3) each listed defect
is rejected by the cases named for it below, in every dtype those cases run in.  The cases of a defect are named from their
switches (a mask defect needs a dropout, the row-pitch defect an odd S, the window defect a kv_shift that is not its own
inverse, the rescale defects more than one key tile), never from the outcome.

`pytest -s tests/test_attn_ref_host.py::test_emulations_are_accepted_on_the_gpu_case_table` prints the worst err / tol of each
emulation per route, dtype and output (the figures DESIGN.md section 4b quotes)."""
import math

import pytest
import torch

from tests import attn_ref as A
from tests.anchor_ref import DTYPES, F64, drop_scale

REL = 1e-12


def close(got, ref, what=""):
    scale = max(float(ref.abs().max()), 1e-300)
    err = float((got - ref).abs().max())
    assert err <= REL * scale, (what, err, scale)


# ------------------------------------------------------------------------------------------------------
# 1. the closed form against autograd
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("kv_shift", [0, 1, 2])
@pytest.mark.parametrize("hd", [32, 64])
def test_closed_form_is_autograd(hd, kv_shift, p):
    NB, S, H = 3, 13, 2
    g = torch.Generator().manual_seed(100 * hd + 10 * kv_shift + int(p > 0))
    qkv = torch.randn(NB * S, 3 * H * hd, generator=g, dtype=F64)
    dO = torch.randn(NB * S, H * hd, generator=g, dtype=F64)
    keep = A.attn_keep(NB, H, S, 77, 5, p) if p else None
    r = A.attention_ref(qkv, dO, NB, S, H, hd, kv_shift, keep, p)
    x = qkv.clone().requires_grad_(True)
    xv = x.reshape(NB, S, 3, H, hd)
    idx = (torch.arange(NB) + kv_shift) % NB
    q = xv[:, :, 0].permute(0, 2, 1, 3)
    k, v = xv[idx][:, :, 1].permute(0, 2, 1, 3), xv[idx][:, :, 2].permute(0, 2, 1, 3)
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    P = torch.softmax(s, -1)
    if p:
        assert 0 < int((~keep).sum()) < keep.numel()
        P = P * keep * drop_scale(p)
    o = (P @ v).permute(0, 2, 1, 3).reshape(NB * S, H * hd)
    o.backward(dO)
    close(r["o"], o.detach(), "o")
    close(r["lse"], torch.logsumexp(s.detach(), -1), "lse")
    close(r["dqkv"], x.grad, "dqkv")
    # the head layout is the row layout, and dK / dV lie in window (b + kv_shift) % NB
    got = A.outputs_from_rows(r["o"], r["lse"], r["dqkv"], NB, S, H, hd)
    for n in A.NAMES:
        assert torch.equal(got[n], r[n]), n
    only = A.attention_ref(qkv, dO * (torch.arange(NB * S) < S)[:, None], NB, S, H, hd, kv_shift, keep, p)      # window 0's loss alone
    for n in ("dk", "dv"):
        elsewhere = [w for w in range(NB) if w != kv_shift]
        assert float(only[n][kv_shift].abs().max()) > 0 and float(only[n][elsewhere].abs().max()) == 0, n


def test_case_table_is_the_one_the_issue_names():
    c = A.CASES
    for route, rand, other in (("short", A.SHORT_RANDN, A.SHORT_OTHER), ("long", A.LONG_RANDN, A.LONG_OTHER), ("dk", A.DK_RANDN, A.DK_OTHER)):
        assert all("%s-randn-S%d" % (route, S) in c for S in rand)
        assert all("%s-%s-S%d" % (route, cls, S) in c for cls in A.CLASSES[1:] for S in other)
        assert all("%s-randn-S%d-drop" % (route, S) in c for S in A.DROP_S[route])
        assert {(v["H"], v["kv_shift"]) for v in c.values() if v["route"] == route and v["NB"] == 3} == set(A.SHAPES)
    assert c["long-rise-S1024"]["NB"] == 1 and all(v["NB"] == 3 for n, v in c.items() if n != "long-rise-S1024")
    assert all(v["p"] == (0.25 if n.endswith("-drop") else 0.0) for n, v in c.items())


# ------------------------------------------------------------------------------------------------------
# 2. the emulations are accepted, every element, on the GPU test's case table
# ------------------------------------------------------------------------------------------------------
WORST = {}


def run(name, dtype, defect=None):
    cs = A.CASES[name]
    qkv, dO, keep, r, tol = A.build_case(cs, dtype)
    if defect == "mask_pitch":
        keep = A.attn_keep(cs["NB"], cs["H"], cs["S"], cs["seed"], cs["site"], cs["p"], pitch=cs["S"])
    elif defect == "mask_shift":
        keep = A.attn_keep(cs["NB"], cs["H"], cs["S"], cs["seed"], cs["site"], cs["p"], shift=1)
    got = A.emulate(cs["route"], qkv, dO, cs["NB"], cs["S"], cs["H"], cs["hd"], cs["kv_shift"], dtype, keep, cs["p"], defect=defect)
    return A.compare_all(got, r, tol, "%s %s" % (name, dtype))


def test_emulations_are_accepted_on_the_gpu_case_table():
    failures = []
    for name, dtype in A.case_ids():
        ratios, msgs = run(name, dtype)
        failures += msgs
        for n, v in ratios.items():
            key = (A.CASES[name]["route"], dtype, n)
            if v >= WORST.get(key, (0.0, ""))[0]:
                WORST[key] = (v, name)
    for route in ("short", "long", "dk"):
        for dtype in DTYPES:
            print("emulation %-5s %-4s " % (route, dtype) + "  ".join("%s %.3f (%s)" % ((n,) + WORST[(route, dtype, n)]) for n in A.NAMES))
    assert not failures, "\n".join(failures)
    assert max(v for v, _ in WORST.values()) > 0.3          # the bounds are within a factor of a few of what the arithmetic does


# ------------------------------------------------------------------------------------------------------
# 3. every defect is rejected by the cases named for it
# ------------------------------------------------------------------------------------------------------
DROPS = [n for n in A.CASES if n.endswith("-drop")]
DEFECT_CASES = {
    # a padded key of the last tile admitted at score 0: where every real score is <= -8 it takes the whole row
    "pad_key": ["short-neg-S65", "short-neg-S97", "long-neg-S65", "long-neg-S203", "dk-neg-S65", "dk-neg-S129"],
    # l, or o, not multiplied by exp(m - mnew): later tiles hold the maximum
    "no_rescale_sum": ["long-rise-S129", "long-rise-S1024", "long-peak-S203", "dk-rise-S129"],
    "no_rescale_out": ["long-rise-S129", "long-rise-S1024", "long-peak-S203", "dk-rise-S129"],
    "lse_no_max": ["short-high-S65", "long-high-S129", "dk-high-S65", "short-neg-S160"],
    # per route, the first case of each kv_shift that is not its own inverse (S >= 63: more than a handful of keys)
    "dkdv_window": [next(n for n, c in A.CASES.items() if c["route"] == route and c["kv_shift"] == sh and c["S"] >= 63)
                    for route in ("short", "long", "dk") for sh in (1, 2)],
    "mask_pitch": [n for n in DROPS if A.CASES[n]["S"] & 1],
    "mask_shift": DROPS,
    "no_dp_scale": DROPS,
    "delta_undropped": DROPS,
    "scale32_at_64": ["dk-randn-S65", "dk-peak-S129", "dk-randn-S65-drop"],
}


def test_every_defect_has_cases_that_can_show_it():
    assert set(DEFECT_CASES) == set(A.DEFECTS)
    assert {A.CASES[n]["kv_shift"] for n in DEFECT_CASES["dkdv_window"]} == {1, 2}        # neither is its own inverse at NB = 3
    assert {A.CASES[n]["route"] for n in DEFECT_CASES["dkdv_window"]} == {"short", "long", "dk"}
    assert all(A.CASES[n]["S"] > A.LT and A.CASES[n]["route"] != "short" for d in ("no_rescale_sum", "no_rescale_out") for n in DEFECT_CASES[d])
    assert {A.CASES[n]["route"] for n in DROPS} == {"short", "long", "dk"} and len(DEFECT_CASES["mask_pitch"]) >= 4


@pytest.mark.parametrize("defect", A.DEFECTS)
def test_defect_is_rejected(defect):
    for name in DEFECT_CASES[defect]:
        for dtype in A.case_dtypes(name):
            ratios, msgs = run(name, dtype, defect)
            assert msgs, "%s passes %s in %s: %r" % (defect, name, dtype, ratios)
            if defect == "pad_key":        # not by lse alone: the context rows themselves leave their bound
                assert ratios["ctx"] > 2 and ratios["dv"] > 2, (name, dtype, ratios)
            if defect == "dkdv_window":
                assert ratios["dk"] > 2 and ratios["dv"] > 2 and ratios["dq"] <= 1 and ratios["ctx"] <= 1, (name, dtype, ratios)


def test_comparator_names_the_worst_element_and_refuses_nan():
    cs = A.CASES["short-randn-S17"]
    qkv, dO, keep, r, tol = A.build_case(cs, "bf16")
    got = A.emulate("short", qkv, dO, cs["NB"], cs["S"], cs["H"], cs["hd"], cs["kv_shift"], "bf16")
    got["dk"][2, 0, 5, 7] += 1.0
    ratio, msg = A.compare(got["dk"], r["dk"], tol["dk"], "short short-randn-S17 bf16", "dk")
    assert ratio > 1 and "window 2, head 0, key 5, column 7" in msg and "err/tol" in msg and "short-randn-S17" in msg
    got["ctx"][1, 0, 3, 2] = float("nan")
    ratio, msg = A.compare(got["ctx"], r["ctx"], tol["ctx"], "x", "ctx")
    assert ratio == float("inf") and "window 1, head 0, query 3, column 2" in msg
    # an exact zero holds at a zero bound, anything else does not
    z = torch.zeros(1, 1, 2, 2, dtype=F64)
    assert A.compare(z, z, z, "x", "ctx")[0] == 0.0 and A.compare(z + 1e-30, z, z, "x", "ctx")[0] == float("inf")


def test_dropped_elements_carry_a_zero_bound():
    """with V one-hot, ctx[q, j] IS P~[q, key j]: where the key is dropped the reference is 0 and so is the bound (bf16, f32; fp16:
    half a subnormal step, which no non-zero fp16 value fits in)"""
    NB, S, H, hd, p = 3, 17, 1, 32, 0.25
    qkv, dO = A.make_inputs("randn", NB, S, H, hd, "bf16", 5)
    x = qkv.clone().reshape(NB, S, 3, H, hd)
    x[:, :, 2] = 0
    for j in range(S):
        x[:, j, 2, :, j] = 1
    keep = A.attn_keep(NB, H, S, 9, 4, p)
    r = A.attention_ref(x.reshape(NB * S, -1), dO, NB, S, H, hd, 1, keep, p)
    for dtype in DTYPES:
        tol = A.bounds(r, dtype)["ctx"][..., :S]
        assert float(tol[~keep].max()) == (A.ETA if dtype == "fp16" else 0.0) and float(r["ctx"][..., :S][~keep].abs().max()) == 0.0
        assert float(tol[keep].min()) > 0


def test_fp16_floor_is_needed_and_suffices(monkeypatch):
    """peaked rows whose dominant key is dropped leave outputs near 1e-6: the correct emulation holds with the floor eta = 2^-25 of
    every 16-bit rounding (the table test above) and leaves the bound by orders of magnitude without it; bf16 has no such floor"""
    for name in ("short-peak-S65-drop", "long-peak-S65-drop", "dk-peak-S65-drop"):
        assert max(run(name, "fp16")[0].values()) <= 1.0
    monkeypatch.setattr(A, "ETA", 0.0)
    for name in ("short-peak-S65-drop", "long-peak-S65-drop", "dk-peak-S65-drop"):
        assert run(name, "fp16")[0]["ctx"] > 10, name
        assert max(run(name, "bf16")[0].values()) <= 1.0
