"""Attention statistics on the device (csrc/attnstats.hip: eg_attention_stats; predict.attention_statistics).
Kernel level: qkv = randn * 1.5 in the compute dtype, lse from eg_attention_dk_fwd at p = 0, expected values from the existing
probabilities kernel (eg_attention_dk_probs, pinned to the reference by tests/golden/hooks.npz) reduced with torch in float64.
Both sides read the same input bits and the 16-bit products are exact in fp32, so only the order of accumulation and exp differ:
the gate is atol 2e-5 on these [0, 1]-valued means in all three dtypes, the project's f32 gate for attention probabilities
(tests/test_gpu_hooks.py).  Shapes: a single key, one ragged tile, one past a tile, the short core's limit and one past it, five
ragged tiles; NB = 2 runs one sample per tile (the direct add into map_sum), NB = 6 splits the samples over workgroups (partials
and the reduce launch); S = 900 folds two samples into one split beside a split of one; S = 1000 walks three samples on the direct
path; S = 2048 is the window-length limit.
Model level: cfg3_xattn (S = 65) against tests/attn_stats_ref.py over the reference's recorded probabilities (the gates of
test_cross_attention_probability_hook), and against the hook route of the same model at 2e-5."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from eyegaze_multimodal_amd.predict import attention_statistics  # noqa: E402
from tests.attn_stats_ref import attn_stats_ref  # noqa: E402
from tests.helpers import GOLDEN, t  # noqa: E402
from tests.test_gpu_attn_dk import dk_fwd  # noqa: E402
from tests.test_gpu_model import DEV, build  # noqa: E402
from tests.test_gpu_ops import DT  # noqa: E402

HZ = np.load(GOLDEN / "hooks.npz", allow_pickle=False)
ATOL = 2e-5
GUARD, SENTINEL = 256, -7.0


def _case(NB, S, H, hd, kv_shift, dtype, seed):
    """qkv, lse on the device and the float64 expectations: per-sample maps' batch sum [S, S] and diagonals [NB/2, S]"""
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(NB * S, 3 * H * hd, generator=g) * 1.5).to(DT[dtype]).to(DEV)
    _, lse = dk_fwd(qkv, NB, S, H, hd, kv_shift, dtype)
    probs = torch.empty(NB, H, S, S, device=DEV)
    call("eg_attention_dk_probs", ptr(qkv), ptr(lse), ptr(probs), NB, S, H, hd, kv_shift, dtype, 0)
    per = (probs[:NB // 2].double().sum(1) + probs[NB // 2:].double().sum(1)) / (2 * H)          # [NB/2, S, S]
    return qkv, lse, per.sum(0), torch.diagonal(per, dim1=1, dim2=2).contiguous()


def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def _run(cases, NB, S, H, hd, kv_shift, dtype, fill):
    """both cases' calls into ONE map_sum and consecutive diag rows, inside sentinel-guarded buffers; scratch pre-filled with `fill`"""
    nb2 = NB // 2
    mbuf, m = _guarded(S * S)
    dbuf, d = _guarded(2 * nb2 * S)
    m.zero_()
    d.fill_(SENTINEL)
    scratch = torch.full((L.attn_stats_scratch_elems(NB, S, H),), fill, device=DEV)
    snaps = []
    for i, (qkv, lse, _, _) in enumerate(cases):
        call("eg_attention_stats", ptr(qkv), ptr(lse), ptr(m), ptr(d[i * nb2 * S:]), ptr(scratch), scratch.numel(), NB, S, H, hd,
             kv_shift, dtype, 0)
        snaps.append((m.clone().view(S, S), d.clone().view(2, nb2, S)))
    torch.cuda.synchronize()
    assert _guards_intact(mbuf) and _guards_intact(dbuf), "a write outside map_sum[S, S] / diag[NB/2, S]"
    return snaps


def _check(NB, S, H, hd, half_shift, dtype):
    kv_shift = NB // 2 if half_shift else 0
    nb2 = NB // 2
    cases = [_case(NB, S, H, hd, kv_shift, dtype, seed=1000 * s + S + 7 * dtype + NB) for s in (1, 2)]
    (m1, d1), (m2, d2) = _run(cases, NB, S, H, hd, kv_shift, dtype, float("nan"))
    err = {"map": float((m1.double() / nb2 - cases[0][2] / nb2).abs().max()),
           "diag": float((d1[0].double() - cases[0][3]).abs().max()),
           "map2": float((m2.double() / nb2 - (cases[0][2] + cases[1][2]) / nb2).abs().max()),
           "diag2": float((d2[1].double() - cases[1][3]).abs().max())}
    print(f"NB={NB} S={S} H={H} hd={hd} kv_shift={kv_shift} dtype={dtype}: " + " ".join(f"{k}={v:.3g}" for k, v in err.items()))
    assert max(err.values()) <= ATOL, err
    assert bool((d1[1] == SENTINEL).all()), "the first call wrote diag rows beyond its own"
    assert torch.equal(d2[0], d1[0]), "the second call touched the first call's diag rows"
    again = _run(cases, NB, S, H, hd, kv_shift, dtype, 3.0e38)               # other scratch contents, same bits
    assert torch.equal(again[1][0], m2) and torch.equal(again[1][1], d2) and torch.equal(again[0][0], m1)


@pytest.mark.parametrize("dtype", [L.EG_BF16, L.EG_F16, L.EG_F32])
@pytest.mark.parametrize("half_shift", [False, True])
@pytest.mark.parametrize("NB", [2, 6])
@pytest.mark.parametrize("hd,H", [(32, 4), (64, 2)])
@pytest.mark.parametrize("S", [1, 63, 65, 160, 161, 300])
def test_kernel_against_the_probabilities_kernel(S, hd, H, NB, half_shift, dtype):
    _check(NB, S, H, hd, half_shift, dtype)


@pytest.mark.parametrize("NB,S,H,hd,dtype", [(2, 2048, 2, 32, L.EG_BF16),        # the longest window
                                             (6, 900, 2, 32, L.EG_BF16),         # splits of two samples and of one
                                             (6, 900, 1, 64, L.EG_F32),
                                             (6, 1000, 1, 32, L.EG_F16)])        # three samples, added into map_sum directly
def test_kernel_long_windows_and_folded_splits(NB, S, H, hd, dtype):
    _check(NB, S, H, hd, True, dtype)


# ------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------
def _close(got, want, atol):
    assert got["count"] == want["count"]
    np.testing.assert_allclose(got["mean_map"], want["mean_map"], rtol=0, atol=atol)
    np.testing.assert_allclose(got["diagonals"], want["diagonals"], rtol=0, atol=atol)
    assert list(got["diagonal_stats"]) == list(want["diagonal_stats"])
    for name, w in want["diagonal_stats"].items():
        g = got["diagonal_stats"][name]
        assert g["count"] == w["count"]
        np.testing.assert_allclose(g["mean_diagonal_vector"], w["mean_diagonal_vector"], rtol=0, atol=atol)
        np.testing.assert_allclose(g["mean_diagonal_value"], w["mean_diagonal_value"], rtol=0, atol=atol)


def _windows(z):
    return t(z["gen_eeg/eeg1"]).to(DEV), t(z["gen_eeg/eeg2"]).to(DEV), t(z["labels"])


@pytest.mark.parametrize("dtype,atol", [("f32", 2e-5), ("bf16", 2e-2)])
def test_statistics_match_the_reference_probabilities(dtype, atol):
    z, kw, cfg, sd, model = build("cfg3_xattn", dtype)
    x1, x2, _ = _windows(z)
    labels = torch.tensor([2, 0])
    got = attention_statistics(model, x1[:2], x2[:2], labels, batch_size=1)
    assert got["mean_map"].shape == (65, 65) and got["mean_map"].dtype == np.float32 and got["diagonals"].shape == (2, 65)
    _close(got, attn_stats_ref(HZ["xattn_probs"][0], HZ["xattn_probs"][1], labels, 1), atol)
    assert list(got["diagonal_stats"]) == ["Cooperation", "Single"]
    one = attention_statistics(model, x1[:2], x2[:2], labels, batch_size=1, max_samples=1)      # tested before each batch
    _close(one, attn_stats_ref(HZ["xattn_probs"][0], HZ["xattn_probs"][1], labels, 1, 1), atol)
    assert one["count"] == 1 and one["logits"].shape == (1, 3)
    # an encoder layer: the two streams' self-attention in place of the two directions
    l0 = attention_statistics(model, x1[:1], x2[:1], labels[:1], where=0, class_names=["a", "b"])
    _close(l0, attn_stats_ref(HZ["self0_probs"][0], HZ["self0_probs"][1], labels[:1], 256, class_names=["a", "b"]), atol)
    assert list(l0["diagonal_stats"]) == ["2"]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_statistics_match_the_hook_route_over_a_ragged_walk(dtype):
    z, kw, cfg, sd, model = build("cfg3_xattn", dtype)
    x1, x2, labels = _windows(z)
    seen, logits = [], []
    h = model.cross_attn.cross_attn.dropout.register_forward_hook(lambda m, i, o: seen.append(i[0].double().cpu().numpy()))
    for sl in (slice(0, 3), slice(3, 4)):                       # the batches attention_statistics walks: 3, then the tail of 1
        logits.append(model.predict(x1[sl], x2[sl])["logits"])
    h.remove()
    assert len(seen) == 4
    want = attn_stats_ref(np.concatenate(seen[0::2]), np.concatenate(seen[1::2]), labels, 3, None)
    got = attention_statistics(model, x1, x2, labels, batch_size=3, max_samples=None)
    assert got["count"] == 4 and len(model._infer_engines) == 2
    _close(got, want, ATOL)
    assert torch.equal(got["logits"], torch.cat(logits)), "logits differ from model.predict's"
    assert torch.equal(got["predictions"], torch.cat(logits).argmax(-1))
    assert got["diagonal_stats"]["Single"]["count"] == 2            # labels 0 1 2 0
    # max_samples counts whole batches: 3 windows reach 2
    assert attention_statistics(model, x1, x2, labels, batch_size=3, max_samples=2)["count"] == 3


def test_predict_is_undisturbed_and_takes_the_lean_routes_again():
    z, kw, cfg, sd, model = build("cfg3_xattn", "bf16")
    x1, x2, labels = _windows(z)
    before = model.predict(x1, x2)["logits"]
    flat = model._flat.flat.clone()
    got = attention_statistics(model, x1, x2, labels, where=0)
    eng = model.inference_engine(4, x1.shape[2], x1.device)
    attn = {l: how for l, half, how in eng.routes_taken if half == "attn"}
    assert eng.attn_stats is None and attn[0] == "scratch" and all(attn[l] == "lean" for l in range(1, cfg.num_layers))
    assert torch.equal(got["logits"], before)
    after = model.predict(x1, x2)["logits"]
    assert torch.equal(after, before) and torch.equal(model._flat.flat, flat)
    assert {how for _, _, how in eng.routes_taken} == {"lean"}
    assert not model._engines and model._fwd_count == 0             # no training engine, no forward counted


def test_without_cross_attention_the_result_is_empty():
    z, kw, cfg, sd, model = build("cfg2_concat", "bf16")
    x1, x2, labels = _windows(z)
    assert attention_statistics(model, x1, x2, labels) == {}
    assert attention_statistics(model, x1, x2, labels, where=1)["mean_map"].shape == (65, 65)
    with pytest.raises(ValueError):
        attention_statistics(model, x1, x2, labels, where=cfg.num_layers)
