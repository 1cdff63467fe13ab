"""Connectivity analyses on the device: eg_ibs_inorm_band, eg_ibs_class_accumulate,
InferenceEngine.forward_band_masks / conn_stats, predict.frequency_sensitivity / connectivity_statistics.

Kernel level.  eg_ibs_inorm_band against eg_ibs_inorm itself, bit for bit: on the same matrices (zero_band = -1) and on a copy with
one band zeroed.  eg_ibs_class_accumulate against tests/conn_stats_ref.py under the bound that holds for ANY order of adding n fp32
terms, |err| <= gamma_{n-1} sum|v_i| with gamma_k = k u / (1 - k u), u = 2^-24 (n: the class's sample count over all calls, sum|v_i|
from the inputs): derived, no measured slack.  The kernel walks the samples in splits of SPLIT = 16 (doubled while the grid would
exceed 1024 workgroups: 32 at B = 130, C = 32); the B below sit on both sides of one split, of a whole number of splits, and of
the doubling.
Model level.  a5_full (B = 4, C = 8, T = 1024) against the hook route of the same model -- HIP against HIP, torch.equal -- and
against tests/golden/hooks.npz at the tolerances tests/test_gpu_hooks.py holds that route to."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import DualEEGTransformer, _lib as L  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from eyegaze_multimodal_amd.predict import (BAND_NAMES, band_metrics_from_confusion, connectivity_statistics,  # noqa: E402
                                            frequency_sensitivity, predict_windows)
from tests.conn_stats_ref import U, class_sums, conn_stats_ref, masked_inorm_ref, summation_bound  # noqa: E402
from tests.helpers import GOLDEN, t  # noqa: E402
from tests.test_gpu_hooks import _conn_close  # noqa: E402
from tests.test_gpu_model import DEV, build  # noqa: E402
from tests.test_gpu_ops import DT  # noqa: E402

HZ = np.load(GOLDEN / "hooks.npz", allow_pickle=False)
SPLIT = 16                          # samples per split of eg_ibs_class_accumulate (CA_CHUNK in csrc/signal.hip)
GUARD, SENTINEL = 256, -7.0
FIDX = {7: [0, 1, 2, 3, 4, 5, 6], 4: [0, 1, 2, 5], 3: [3, 4, 6]}


def _guarded(n, dtype=torch.float32):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------
# eg_ibs_inorm_band
# ------------------------------------------------------------------------------------------------
def _inorm(conn, fd, g, b, shape, use_norm, dtype, zero_band=None, xhat=True):
    """(out, xhat) of eg_ibs_inorm (zero_band None) or eg_ibs_inorm_band, inside guarded buffers; xhat=False passes NULL"""
    B, nb, nf, E = shape
    obuf, out = _guarded(B * nb * nf * E, DT[dtype])
    xbuf, xh = _guarded(B * nb * nf * E)
    args = (ptr(conn), ptr(fd), ptr(g) if use_norm else 0, ptr(b) if use_norm else 0, ptr(out), ptr(xh) if xhat else 0, B, nb, nf, E,
            use_norm)
    if zero_band is None:
        call("eg_ibs_inorm", *args, dtype, 0)
    else:
        call("eg_ibs_inorm_band", *args, zero_band, dtype, 0)
    torch.cuda.synchronize()
    assert _guards_intact(obuf) and _guards_intact(xbuf), "a write outside out / xhat"
    return out.clone(), xh.clone()


@pytest.mark.parametrize("dtype", [L.EG_F32, L.EG_BF16, L.EG_F16])
@pytest.mark.parametrize("use_norm", [0, 1])
@pytest.mark.parametrize("B,nb,nf,Cn", [(1, 6, 7, 3), (3, 6, 4, 8), (2, 4, 3, 17), (2, 6, 7, 32)])
def test_inorm_band_gives_the_bits_of_inorm(B, nb, nf, Cn, use_norm, dtype):
    E = Cn * Cn
    shape = (B, nb, nf, E)
    g_ = torch.Generator().manual_seed(100 * Cn + nf)
    conn = ((torch.rand(B, nb, 7, E, generator=g_) * 2 - 1) * np.pi).to(DEV)
    fd = torch.tensor(FIDX[nf], dtype=torch.int32, device=DEV)
    g, b = (torch.randn(E, generator=g_) * 0.5 + 1).to(DEV), torch.randn(E, generator=g_).to(DEV)
    want_out, want_xh = _inorm(conn, fd, g, b, shape, use_norm, dtype)
    untouched = torch.full_like(want_xh, SENTINEL)
    if dtype == L.EG_F32 and not use_norm:      # the rows are the selected matrices themselves (tests/conn_stats_ref.py)
        ref = masked_inorm_ref(conn.cpu().numpy(), FIDX[nf], None, None, -1)
        assert np.array_equal(want_out.cpu().numpy().reshape(ref.shape), ref)
    got_out, got_xh = _inorm(conn, fd, g, b, shape, use_norm, dtype, zero_band=-1)
    assert torch.equal(got_out, want_out) and torch.equal(got_xh, want_xh if use_norm else untouched)
    lean_out, lean_xh = _inorm(conn, fd, g, b, shape, use_norm, dtype, zero_band=-1, xhat=False)
    assert torch.equal(lean_out, want_out) and torch.equal(lean_xh, untouched), "xhat = NULL changed out or wrote next to it"
    for band in range(nb):
        zeroed = conn.clone()
        zeroed[:, band] = 0
        want_out, want_xh = _inorm(zeroed, fd, g, b, shape, use_norm, dtype)
        got_out, got_xh = _inorm(conn, fd, g, b, shape, use_norm, dtype, zero_band=band)
        assert torch.equal(got_out, want_out) and torch.equal(got_xh, want_xh if use_norm else untouched), band
        lean_out, lean_xh = _inorm(conn, fd, g, b, shape, use_norm, dtype, zero_band=band, xhat=False)
        assert torch.equal(lean_out, want_out) and torch.equal(lean_xh, untouched), band


# ------------------------------------------------------------------------------------------------
# eg_ibs_class_accumulate
# ------------------------------------------------------------------------------------------------
def _accumulate(calls, nb, nf, E, ncls, fill):
    """every (conn, labels) of `calls` into ONE class_sum / class_count inside guarded buffers; scratch pre-filled with `fill`"""
    ncol = nb * nf * E
    sbuf, s = _guarded(ncls * ncol)
    cbuf, c = _guarded(ncls, torch.int32)
    s.zero_(), c.zero_()
    fd = torch.tensor(FIDX[nf], dtype=torch.int32, device=DEV)
    for conn, labels in calls:
        B = conn.shape[0]
        need = L.ibs_class_scratch_elems(B, nb, nf, E, ncls)
        assert need >= 0 and (need == 0) == (B <= SPLIT)
        scr_buf, scr = _guarded(need)
        scr.fill_(fill)
        call("eg_ibs_class_accumulate", ptr(conn), ptr(fd), ptr(labels), ptr(s), ptr(c), ptr(scr), need, B, nb, nf, E, ncls, 0)
        torch.cuda.synchronize()
        assert _guards_intact(scr_buf), "a write outside the scratch"
    assert _guards_intact(sbuf) and _guards_intact(cbuf), "a write outside class_sum / class_count"
    return s.clone().view(ncls, nb, nf, E), c.clone()


def _labels(kind, B, ncls, g_):
    if kind == "mixed":             # every class, and -1 and ncls, which count nowhere
        y = torch.randint(-1, ncls + 1, (B,), generator=g_)
        y[: min(B, 2)] = torch.tensor([-1, ncls])[: min(B, 2)]
    elif kind == "one_class":
        y = torch.full((B,), ncls - 1)
    else:                           # "a_class_with_none": class 0 never occurs (ncls = 1: no sample counts at all)
        y = torch.randint(1, max(ncls, 2), (B,), generator=g_)
    return y.to(torch.int64)


@pytest.mark.parametrize("nf", [7, 4])
@pytest.mark.parametrize("B,Cn,ncls", [(1, 3, 1), (5, 8, 3), (64, 8, 3), (257, 8, 16), (33, 32, 3), (130, 32, 3)])
def test_class_accumulate_within_the_summation_bound(B, Cn, ncls, nf):
    nb, E = 6, Cn * Cn
    g_ = torch.Generator().manual_seed(1000 * B + 10 * Cn + nf)
    conns = [((torch.rand(B, nb, 7, E, generator=g_) * 2 - 1) * np.pi) for _ in range(2)]
    dev_conns = [c.to(DEV) for c in conns]
    sel = [c.numpy()[:, :, FIDX[nf]] for c in conns]
    for kind in ("mixed", "one_class", "a_class_with_none"):
        ys = [_labels(kind, B, ncls, g_) for _ in range(2)]
        calls = [(c, y.to(DEV)) for c, y in zip(dev_conns, ys)]
        got_sum, got_cnt = _accumulate(calls, nb, nf, E, ncls, float("nan"))
        for ncalls in (1, 2):       # the first call alone (computed afresh), then two calls into the same outputs
            if ncalls == 1:
                s, c = _accumulate(calls[:1], nb, nf, E, ncls, float("nan"))
            else:
                s, c = got_sum, got_cnt
            want, counts, mags = class_sums(np.concatenate(sel[:ncalls]), torch.cat(ys[:ncalls]).numpy(), ncls)
            assert c.cpu().numpy().tolist() == counts.tolist(), (kind, ncalls)
            err = np.abs(s.double().cpu().numpy() - want)
            bound = summation_bound(counts.reshape(-1, 1, 1, 1), mags)
            print(f"B={B} C={Cn} ncls={ncls} nf={nf} {kind} calls={ncalls}: counts={counts.tolist()} max err={err.max():.3g} "
                  f"max err/bound={np.max(err / np.maximum(bound, 1e-300)):.3g}")
            assert (err <= bound).all(), (kind, ncalls, float(err.max()))
        if kind == "a_class_with_none":
            assert got_cnt[0] == 0 and not got_sum[0].any()
        again_sum, again_cnt = _accumulate(calls, nb, nf, E, ncls, 3.0e38)           # other scratch contents, same bits
        assert torch.equal(again_sum, got_sum) and torch.equal(again_cnt, got_cnt), kind


# ------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------
def _windows(z):
    return t(z["gen_eeg/eeg1"]).to(DEV), t(z["gen_eeg/eeg2"]).to(DEV), t(z["labels"])


def _mask_hook(band):
    def mask(m, i, o):              # the reference's FrequencyMaskHook (eeg_metrics.py:332-336)
        o[:, band, :, :, :] = 0
        return o
    return mask


def _hook_route(model, x1, x2, labels, batch_size):
    """[1 + 6, N, ncls] logits and the seven confusion matrices of seven predict_windows walks, six with a mask hook registered"""
    logits, cms = [], []
    for band in (None, 0, 1, 2, 3, 4, 5):
        h = model.ibs_matrix_generator.register_forward_hook(_mask_hook(band)) if band is not None else None
        try:
            out = predict_windows(model, x1, x2, labels, batch_size=batch_size)
        finally:
            if h is not None:
                h.remove()
        logits.append(out["logits"].clone())
        cms.append(out["confusion"])
    return torch.stack(logits), np.stack(cms)


def _variant(name, dtype, **over):
    """the fixture's model, or with `over` a randomly initialised one of the same shape"""
    if not over:
        return build(name, dtype)
    z, kw, cfg, sd, _ = build(name, dtype)
    torch.manual_seed(7)
    model = DualEEGTransformer(**{**kw, **over}, compute_dtype=dtype).to(DEV)
    return z, kw, model.cfg, None, model


@pytest.mark.parametrize("dtype,over,batch_size", [("f32", {}, 256), ("bf16", {}, 256), ("f32", dict(ibs_feature_type="phase"), 256),
                                                   ("bf16", dict(ibs_instance_norm=False), 256), ("f32", {}, 3), ("bf16", {}, 3)],
                         ids=["f32", "bf16", "phase", "no_inorm", "ragged_f32", "ragged_bf16"])
def test_frequency_sensitivity_gives_the_bits_of_the_hook_walks(dtype, over, batch_size):
    z, kw, cfg, sd, model = _variant("a5_full", dtype, **over)
    x1, x2, labels = _windows(z)
    want, want_cm = _hook_route(model, x1, x2, labels, batch_size)
    got = frequency_sensitivity(model, x1, x2, labels, batch_size=batch_size)
    assert got["logits"].shape == (7, 4, cfg.num_classes) and got["confusion"].shape == (7, cfg.num_classes, cfg.num_classes)
    if batch_size >= 4:
        assert torch.equal(got["logits"][0], model.predict(x1, x2)["logits"]), "the unmasked variant differs from model.predict"
    for v in range(7):
        assert torch.equal(got["logits"][v], want[v]), f"variant {v}: max diff {float((got['logits'][v] - want[v]).abs().max()):.3g}"
    assert len({got["logits"][v].cpu().numpy().tobytes() for v in range(7)}) == 7, "masking a band changed nothing"
    assert np.array_equal(got["confusion"], want_cm) and got["confusion"].sum() == 7 * 4
    assert list(got["sensitivity"]) == BAND_NAMES and got["baseline"] == band_metrics_from_confusion(want_cm[0])
    for b, name in enumerate(BAND_NAMES):
        assert got["sensitivity"][name] == band_metrics_from_confusion(want_cm[1 + b])
    if dtype == "f32" and not over:
        base, masked = got["logits"][0].cpu().numpy(), got["logits"][1:].cpu().numpy()
        print(f"batch_size={batch_size}: |logits - reference| base {np.abs(base - HZ['ibs_base_logits']).max():.3g} "
              f"masked {np.abs(masked - HZ['ibs_masked_logits']).max():.3g}")
        np.testing.assert_allclose(base, HZ["ibs_base_logits"], rtol=0, atol=2e-4)
        np.testing.assert_allclose(masked, HZ["ibs_masked_logits"], rtol=0, atol=2e-4)


def test_frequency_sensitivity_of_a_scalar_synchrony_model_is_the_baseline():
    z, kw, cfg, sd, model = build("a3_ibs_scalar", "bf16")
    x1, x2, labels = _windows(z)
    got = frequency_sensitivity(model, x1, x2, labels)
    want = predict_windows(model, x1, x2, labels)
    for v in range(7):
        assert torch.equal(got["logits"][v], want["logits"]) and np.array_equal(got["confusion"][v], want["confusion"])
    assert all(m == got["baseline"] for m in got["sensitivity"].values()) and list(got["sensitivity"]) == BAND_NAMES
    assert got["baseline"] == {"accuracy": want["metrics"]["eval/accuracy"], "f1": want["metrics"]["eval/f1"]}
    assert connectivity_statistics(model, x1, x2, labels) == {}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_class_means_match_the_capture_hook_and_the_reference(dtype):
    z, kw, cfg, sd, model = build("a5_full", dtype)
    x1, x2, _ = _windows(z)
    labels = torch.tensor([0, 1, 1, 2])
    seen, logits = [], []
    h = model.ibs_matrix_generator.register_forward_hook(lambda m, i, o: seen.append(o.detach().cpu().numpy()))
    for sl in (slice(0, 3), slice(3, 4)):                       # the batches connectivity_statistics walks
        logits.append(model.predict(x1[sl], x2[sl])["logits"])
    h.remove()
    captured = np.concatenate(seen)
    assert captured.shape == (4, 6, 7, 8, 8)
    got = connectivity_statistics(model, x1, x2, labels, batch_size=3)
    assert got["count"] == 4 and got["class_count"] == {"Single": 1, "Competition": 2, "Cooperation": 1}
    assert torch.equal(got["logits"], torch.cat(logits)) and torch.equal(got["predictions"], torch.cat(logits).argmax(-1))
    want = conn_stats_ref(captured, labels.numpy())
    sums, counts, mags = class_sums(captured, labels.numpy(), 3)
    n = counts.reshape(-1, 1, 1, 1, 1)
    bsum = summation_bound(n, mags)
    tol = bsum / n + U * (np.abs(sums) + bsum) / n              # the summation bound, and one rounding of the division
    for c, name in enumerate(["Single", "Competition", "Cooperation"]):
        m = got["class_mean"][name]
        assert m.shape == (6, 7, 8, 8) and m.dtype == np.float32
        err = np.abs(m.astype(np.float64) - want["class_mean"][name])
        print(f"{dtype} {name}: |mean - float64 mean of the captured matrices| {err.max():.3g} (allowed {tol[c].max():.3g})")
        assert (err <= tol[c]).all()
    np.testing.assert_array_equal(got["difference"], got["class_mean"]["Cooperation"] - got["class_mean"]["Competition"])
    # against the reference's matrices: a mean of samples that each meet test_gpu_hooks._conn_close's bounds meets them
    ref = conn_stats_ref(HZ["ibs_conn"], labels.numpy())
    _conn_close(np.stack(list(got["class_mean"].values())), np.stack(list(ref["class_mean"].values())))
    # max_samples counts whole batches: 3 windows reach 2; a class that never occurred has a zero mean
    part = connectivity_statistics(model, x1, x2, labels, batch_size=3, max_samples=2)
    assert part["count"] == 3 and part["class_count"]["Cooperation"] == 0 and not part["class_mean"]["Cooperation"].any()
    np.testing.assert_array_equal(part["class_mean"]["Single"], got["class_mean"]["Single"])
    named = connectivity_statistics(model, x1, x2, labels, batch_size=3, class_names=["a", "b"])     # label 2 counts nowhere
    assert list(named["class_mean"]) == ["a", "b"] and "difference" not in named and named["class_count"] == {"a": 1, "b": 2}
    # the matrices the tokeniser consumes are the ones that are averaged: a hook that halves them halves the means
    h = model.ibs_matrix_generator.register_forward_hook(lambda m, i, o: o * 0.5)
    try:
        half = connectivity_statistics(model, x1, x2, labels, batch_size=3)
    finally:
        h.remove()
    for name, m in got["class_mean"].items():
        np.testing.assert_array_equal(half["class_mean"][name], m * np.float32(0.5))
    assert not torch.equal(half["logits"], got["logits"])


def test_command_line_flags_on_the_shard_route_and_the_resident_route(tmp_path):
    """predict.main with --connectivity-stats --frequency-sensitivity over CSV recordings, an untrained A5-style model of one
    layer: both routes write the same arrays, and they are the two public calls' results"""
    import json
    from types import SimpleNamespace

    import yaml

    from eyegaze_multimodal_amd import predict as P
    from eyegaze_multimodal_amd import train_art as TA
    from tests.test_gpu_train import make_config
    rng = np.random.default_rng(0)
    eeg = tmp_path / "EEGseg"
    eeg.mkdir()
    names = ["Single", "Competition", "Cooperation"]
    items, tt = [], np.arange(1024 + 512) / 256.0
    for i in range(12):
        c = i % 3
        for who in (1, 2):
            x = 1e-5 * rng.standard_normal((8, len(tt))) + 2e-5 * np.sin(2 * np.pi * [6.0, 14.0, 31.0][c] * tt + rng.uniform(0, 6.28))
            np.savetxt(eeg / f"pair{i}_p{who}.csv", x.astype(np.float32), delimiter=",", fmt="%.7e")
        items.append({"player1": f"pair{i}_p1", "player2": f"pair{i}_p2", "class": names[c]})
    (tmp_path / "meta.json").write_text(json.dumps(items))
    files = {}
    for resident in (False, True):
        out = tmp_path / f"resident_{resident}"
        (out / "run").mkdir(parents=True)
        cfg = make_config(out, ablation={"use_ibs": True}, model={"num_layers": 1},
                          data={"synthetic": False, "metadata_path": str(tmp_path / "meta.json"), "eeg_base_path": str(eeg),
                                "max_samples": None, "resident": resident},
                          training={"per_device_eval_batch_size": 4})
        (out / "cfg.yaml").write_text(yaml.safe_dump(cfg))
        torch.manual_seed(3)
        torch.save({"model_state_dict": TA.build_model(cfg, None).state_dict()}, out / "model.pt")
        P.main(SimpleNamespace(config=str(out / "cfg.yaml"), checkpoint=str(out / "model.pt"), out=str(out / "pred.npz"), split="test",
                               dtype=None, resident=resident, attention_stats=None, attention_max_samples=200,
                               connectivity_stats=True, frequency_sensitivity=True))
        files[resident] = np.load(out / "pred.npz")
    pa, pb = files[False], files[True]
    want = {f"conn_class_{n}_mean" for n in names} | {"conn_difference", "conn_class_count", "band_confusion"} \
        | {f"band_{b}_{m}" for b in BAND_NAMES for m in ("accuracy", "f1")}
    assert want <= set(pa.files) and set(pa.files) == set(pb.files)
    for k in pa.files:
        assert pa[k].tobytes() == pb[k].tobytes(), k
    n = len(pa["labels"])
    assert n >= 2 and pa["conn_class_count"].sum() == n and pa["conn_class_Single_mean"].shape == (6, 7, 8, 8)
    assert pa["band_confusion"].shape == (7, 3, 3) and (pa["band_confusion"].sum((1, 2)) == n).all()
    assert np.array_equal(pa["band_confusion"][0], pa["confusion"])              # the unmasked variant is the plain walk
    np.testing.assert_array_equal(pa["conn_difference"], pa["conn_class_Cooperation_mean"] - pa["conn_class_Competition_mean"])
    assert float(pa["band_alpha_accuracy"]) == band_metrics_from_confusion(pa["band_confusion"][4])["accuracy"]


def test_predict_and_a_training_step_are_undisturbed():
    z, kw, cfg, sd, model = build("a5_full", "bf16")
    x1, x2, labels = _windows(z)

    def step():
        model.train()
        model._fwd_count = 0                                    # the dropout seed of the first forward, every time
        model.zero_grad()
        out = model(x1, x2, labels.to(DEV))
        out["loss"].backward()
        model.eval()
        return [out["logits"].detach().clone()] + [p.grad.clone() for p in model.parameters() if p.grad is not None]

    before = model.predict(x1, x2)["logits"]
    eng = model.inference_engine(4, x1.shape[2], x1.device)
    routes, held = list(eng.routes_taken), set(eng.a)
    step0 = step()
    flat = model._flat.flat.clone()
    fs = frequency_sensitivity(model, x1, x2, labels)
    cs = connectivity_statistics(model, x1, x2, labels)
    assert eng.conn_stats is None and eng.attn_stats is None and eng.a["x0"] is eng.a["xa"] and set(eng.a) == held
    assert torch.equal(fs["logits"][0], before) and torch.equal(cs["logits"], before)
    after = model.predict(x1, x2)["logits"]
    assert torch.equal(after, before) and torch.equal(model._flat.flat, flat)
    assert eng.routes_taken == routes
    for a_, b_ in zip(step(), step0):
        assert torch.equal(a_, b_)
    # a request that does not fit the batch is refused before the launch, and the attribute does not outlive the call
    from eyegaze_multimodal_amd.engine import ConnStats
    eng.conn_stats = ConnStats(labels[:3].to(DEV), torch.zeros(3, 6, 7, 8, 8, device=DEV), torch.zeros(3, device=DEV, dtype=torch.int32),
                               torch.zeros(0, device=DEV))
    try:
        with pytest.raises(L.EgError, match="conn_stats.labels"):
            eng.forward(x1, x2, None)
    finally:
        eng.conn_stats = None
    assert torch.equal(model.predict(x1, x2)["logits"], before)
