"""Every attention core against its fp64 statement (tests/attn_ref.py), element by element with no element left out: the short
core (eg_attention_fwd / _bwd: S <= 160, the 96 / 128 / 160 capacity templates and the 80-row images), the long core at width 32
(eg_attention_long_*) and at width 64 (eg_attention_dk_*), and their probabilities kernels, in bf16, fp16 and f32.

The forward feeds the backward, as the engine does.  Every case is NB = 3 windows (NB * H odd at H = 1; kv_shift 1 and 2 are each
other's inverse, so the dK / dV kernels' inverted window pairing cannot hide) but the S = 1024 case of sixteen key tiles.  Inputs
come in classes (attn_ref.make_inputs): randn, and inputs built so that a tile-edge or a rescaling mistake takes whole rows with
it -- all scores <= -8, a near one-hot soft-max, the row maximum in the last key, scores near +70, and in fp16 gradients scaled
by 1024.  Dropout masks are replayed on the CPU (tests/dropout64.py, engine.scramble_seed), never read back from a kernel.
ctx, lse, dqkv, the delta scratch and the probabilities live inside larger buffers of a sentinel pattern that must be intact
after every call.  The bound of each element is derived in attn_ref's docstring; tests/test_attn_ref_host.py shows it accept
fp32 emulations of the kernels' arithmetic and reject a list of defects.  A failure names route, case, output, the worst element's
window, head, query or key and column, and its err / tol; every test prints its err / tol per output (pytest -s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from eyegaze_multimodal_amd.engine import scramble_seed  # noqa: E402
from tests import attn_ref as A  # noqa: E402
from tests.anchor_ref import DTYPES, EG, F64, TDT  # noqa: E402
from tests.test_gpu_ops import dev_state  # noqa: E402

DEV = "cuda"
FWD = {"short": "eg_attention_fwd", "long": "eg_attention_long_fwd", "dk": "eg_attention_dk_fwd"}
BWD = {"short": "eg_attention_bwd", "long": "eg_attention_long_bwd", "dk": "eg_attention_dk_bwd"}
PROBS = {"short": "eg_attention_probs", "long": "eg_attention_long_probs", "dk": "eg_attention_dk_probs"}
SENT = {2: 0x5A5B, 4: 0x5A5B5C5D}          # bit patterns of ordinary finite numbers in bf16, fp16 and f32
BITS = {2: torch.int16, 4: torch.int32}


class Guarded:
    """an [nrows, ncols] output inside a larger buffer of the sentinel pattern: at least four rows' worth (a multiple of 64
    elements, so the view stays 16-byte aligned) in front of it and behind it"""

    def __init__(self, nrows, ncols, tdt):
        self.size = torch.empty(0, dtype=tdt).element_size()
        self.n = nrows * ncols
        self.g = (max(4 * ncols, 64) + 63) // 64 * 64
        self.buf = torch.full((self.n + 2 * self.g,), SENT[self.size], device=DEV, dtype=BITS[self.size])
        self.t = self.buf[self.g:self.g + self.n].view(tdt).view(nrows, ncols)

    def intact(self):
        return bool((self.buf[:self.g] == SENT[self.size]).all()) and bool((self.buf[self.g + self.n:] == SENT[self.size]).all())


def heads(cs):
    return (cs["H"], cs["hd"]) if cs["route"] == "dk" else (cs["H"],)


def forward(cs, dtype, qkvd, st):
    NB, S, H, hd = cs["NB"], cs["S"], cs["H"], cs["hd"]
    ctx, lse = Guarded(NB * S, H * hd, TDT[dtype]), Guarded(NB * H, S, torch.float32)
    call(FWD[cs["route"]], ptr(qkvd), ptr(ctx.t), ptr(lse.t), NB, S, *heads(cs), cs["kv_shift"], EG[dtype], cs.get("p", 0.0),
         cs.get("site", 0), ptr(st), 0)
    torch.cuda.synchronize()
    assert ctx.intact() and lse.intact(), "%s: a forward store left ctx / lse" % FWD[cs["route"]]
    return ctx, lse


def backward(cs, dtype, qkvd, dOd, ctx, lse, st):
    NB, S, H, hd = cs["NB"], cs["S"], cs["H"], cs["hd"]
    dqkv = Guarded(NB * S, 3 * H * hd, TDT[dtype])
    args = [ptr(qkvd), ptr(ctx.t), ptr(dOd), ptr(lse.t), ptr(dqkv.t), NB, S, *heads(cs), cs["kv_shift"], EG[dtype], cs["p"], cs["site"],
            ptr(st)]
    scratch = None
    if cs["route"] != "short":
        scratch = Guarded(NB * H, S, torch.float32)               # delta
        args += [ptr(scratch.t), scratch.n]
    call(BWD[cs["route"]], *args, 0)
    torch.cuda.synchronize()
    assert dqkv.intact() and ctx.intact() and lse.intact() and (scratch is None or scratch.intact()), \
        "%s: a backward store left dqkv / the scratch" % BWD[cs["route"]]
    return dqkv


@pytest.mark.parametrize("name,dtype", A.case_ids(), ids=["%s-%s" % nd for nd in A.case_ids()])
def test_attention_matches_fp64(name, dtype):
    cs = A.CASES[name]
    NB, S, H, hd = cs["NB"], cs["S"], cs["H"], cs["hd"]
    qkv, dO, keep, r, tol = A.build_case(cs, dtype)
    st = dev_state(seed=scramble_seed(cs["seed"])) if cs["p"] else None      # the words Engine.set_state publishes
    qkvd, dOd = qkv.to(DEV), dO.to(DEV)
    ctx, lse = forward(cs, dtype, qkvd, st)
    dqkv = backward(cs, dtype, qkvd, dOd, ctx, lse, st)
    got = A.outputs_from_rows(ctx.t.cpu(), lse.t.cpu(), dqkv.t.cpu(), NB, S, H, hd)
    ratios, msgs = A.compare_all(got, r, tol, "%s %s %s" % (cs["route"], name, dtype))
    print("ANCHOR %s %s %s " % (cs["route"], dtype, name) + " ".join("%s=%.3f" % (n, ratios[n]) for n in A.NAMES))
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [n for n in A.CASES if n.endswith("-drop")])
def test_dropped_elements_contribute_exactly_nothing(name, dtype):
    """V one-hot over hd keys at a time: ctx[q, j] IS the dropped probability of key c * hd + j, so a dropped element has
    reference 0 and bound 0 (fp16: half a subnormal step) and a kept one its own bound; every key chunk of the window"""
    cs = A.CASES[name]
    NB, S, H, hd, p = cs["NB"], cs["S"], cs["H"], cs["hd"], cs["p"]
    qkv, dO = A.make_inputs(cs["cls"], NB, S, H, hd, dtype, cs["seed"])
    keep = A.attn_keep(NB, H, S, cs["seed"], cs["site"], p)
    st = dev_state(seed=scramble_seed(cs["seed"]))
    worst = 0.0
    for c in range((S + hd - 1) // hd):
        n = min(hd, S - c * hd)
        x = qkv.clone().reshape(NB, S, 3, H, hd)
        x[:, :, 2] = 0
        for j in range(n):
            x[:, c * hd + j, 2, :, j] = 1
        x = x.reshape(NB * S, 3 * H * hd)
        r = A.attention_ref(x, dO, NB, S, H, hd, cs["kv_shift"], keep, p)
        tol = A.bounds(r, dtype)
        ctx, lse = forward(cs, dtype, x.to(DEV), st)
        got = A.to_heads(ctx.t.cpu().to(F64), NB, S, H, hd)
        dropped = ~keep[..., c * hd:c * hd + n]
        assert int(dropped.sum()) > 0 and float(got[..., :n][dropped].abs().max()) == 0.0, "%s %s chunk %d: a dropped key reached ctx" % (name, dtype, c)
        for out, g in (("ctx", got), ("lse", lse.t.cpu().reshape(NB, H, S))):
            ratio, msg = A.compare(g, r[out], tol[out], "%s %s %s one-hot V chunk %d" % (cs["route"], name, dtype, c), out)
            assert not msg, msg
            worst = max(worst, ratio)
    print("ANCHOR-ONEHOT %s %s %s worst=%.3f" % (cs["route"], dtype, name, worst))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(A.PROBS_CASES))
def test_probabilities_match_fp64(name, dtype):
    """the fp64 soft-max within rho P + 2^-24 P per element, from the forward's lse (itself held to its bound); rows sum to 1
    within S times the row's largest bound"""
    cs = A.PROBS_CASES[name]
    NB, S, H, hd = cs["NB"], cs["S"], cs["H"], cs["hd"]
    qkv, dO = A.make_inputs(cs["cls"], NB, S, H, hd, dtype, cs["seed"])
    r = A.attention_ref(qkv, dO, NB, S, H, hd, cs["kv_shift"])
    A.check_class(cs["cls"], r)
    qkvd = qkv.to(DEV)
    ctx, lse = forward(cs, dtype, qkvd, None)
    what = "%s %s %s" % (cs["route"], name, dtype)
    lse_got = lse.t.cpu().reshape(NB, H, S)
    ratio_l, msg = A.compare(lse_got, r["lse"], A.bounds(r, dtype)["lse"], what, "lse")
    assert not msg, msg
    probs = Guarded(NB * H * S, S, torch.float32)
    call(PROBS[cs["route"]], ptr(qkvd), ptr(lse.t), ptr(probs.t), NB, S, *heads(cs), cs["kv_shift"], EG[dtype], 0)
    torch.cuda.synchronize()
    assert probs.intact() and lse.intact(), "%s: a store left probs" % PROBS[cs["route"]]
    got = probs.t.cpu().to(F64).reshape(NB, H, S, S)
    ref, tol = A.probs_ref(r, dtype)
    ratio, msg = A.compare(got, ref, tol, what, "probs")
    rows = (got.sum(-1) - 1).abs() / (S * tol.amax(-1))
    print("ANCHOR-PROBS %s %s %s probs=%.3f lse=%.3f rowsum=%.3f" % (cs["route"], dtype, name, ratio, ratio_l, float(rows.max())))
    assert not msg, msg
    assert float(rows.max()) <= 1.0, "%s: a row sums to 1 +- %.3g, %.3g of its bound" % (what, float((got.sum(-1) - 1).abs().max()), float(rows.max()))
