"""CPU-only: the connectivity analyses' semantics, C ABI and launch lists.
  * tests/conn_stats_ref.py (the float64 restatement the GPU tests compare with) against the reference's own
    compute_mean_ibs_by_class / compute_ibs_difference (5_Metrics/eeg_metrics.py:271-311), loaded by file path and fed
    tests/golden/hooks.npz::ibs_conn; skipped where the reference tree is absent;
  * predict.band_metrics_from_confusion on hand-made matrices and against sklearn;
  * the header declares the three new functions, _lib binds them, the ABI version is still 5;
  * every refusal of eg_ibs_inorm_band / eg_ibs_class_accumulate happens on the host, before any launch;
  * the launches of InferenceEngine.forward_band_masks and of a forward with conn_stats, recorded, not issued;
  * the argument checks of predict.connectivity_statistics / predict.frequency_sensitivity."""
import importlib.util
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.conn_stats_ref import class_sums, conn_stats_ref, masked_inorm_ref, summation_bound
from tests.helpers import GOLDEN

REPO = Path(__file__).resolve().parent.parent
BUF = torch.zeros(4096, dtype=torch.float32)      # host memory: its address stands in for every operand of a refused call
P = BUF.data_ptr()


def _reference_metrics():
    from oracle.make_golden import REF
    path = REF / "5_Metrics" / "eeg_metrics.py"
    if not path.exists():
        pytest.skip("the reference tree is not present")
    pytest.importorskip("sklearn.metrics")
    pytest.importorskip("tqdm")
    spec = importlib.util.spec_from_file_location("reference_eeg_metrics", str(path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("labels", [[0, 1, 1, 2], [0, 0, 2, 2]], ids=["all_classes", "one_absent"])
def test_restatement_matches_the_reference_functions(labels):
    ref = _reference_metrics()
    conn = np.load(GOLDEN / "hooks.npz", allow_pickle=False)["ibs_conn"]                 # [4, 6, 7, 8, 8] f32
    names = ["Single", "Competition", "Cooperation"]
    want = ref.compute_mean_ibs_by_class(conn, np.array(labels), names)
    got = conn_stats_ref(conn, labels)
    assert list(got["class_mean"]) == list(want) == names
    for n in names:
        assert got["class_mean"][n].shape == (6, 7, 8, 8) and got["class_count"][n] == labels.count(names.index(n))
        # the reference averages in fp32: a mean of at most 2 values of magnitude <= pi differs from the float64 one by < 1e-6
        np.testing.assert_allclose(got["class_mean"][n], want[n], rtol=0, atol=1e-6)
    if 1 not in labels:
        assert not got["class_mean"]["Competition"].any() and not want["Competition"].any()
    np.testing.assert_allclose(got["difference"], ref.compute_ibs_difference(want["Cooperation"], want["Competition"]), rtol=0, atol=2e-6)


def test_restatement_of_the_sums_and_the_masked_norm():
    rng = np.random.default_rng(0)
    m = rng.uniform(-np.pi, np.pi, (5, 2, 3, 4)).astype(np.float32)
    sums, counts, mags = class_sums(m, [0, 2, -1, 3, 2], 3)
    assert counts.tolist() == [1, 0, 2]
    np.testing.assert_array_equal(sums[0], m[0].astype(np.float64))
    np.testing.assert_array_equal(sums[1], 0)
    np.testing.assert_array_equal(sums[2], m[1].astype(np.float64) + m[4])
    np.testing.assert_array_equal(mags[2], np.abs(m[1].astype(np.float64)) + np.abs(m[4]))
    assert summation_bound(1, mags[0]).max() == 0 and summation_bound(2, mags[2]).max() < 2 * np.pi * 2.0 ** -23
    conn = rng.uniform(-1, 1, (2, 3, 7, 5))
    x = torch.from_numpy(conn[:, :, [0, 1, 2, 5]].copy())
    x[:, 1] = 0
    norm = torch.nn.InstanceNorm1d(5, affine=True).double()
    with torch.no_grad():
        norm.weight.copy_(torch.linspace(0.5, 1.5, 5)), norm.bias.copy_(torch.linspace(-1, 1, 5))
        want = norm(x.reshape(2, 12, 5).transpose(1, 2)).transpose(1, 2).numpy()       # the tokeniser's call (D:897-901)
    got = masked_inorm_ref(conn, [0, 1, 2, 5], norm.weight.detach().numpy(), norm.bias.detach().numpy(), 1)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(masked_inorm_ref(conn, [3, 4, 6], None, None, -1), conn[:, :, [3, 4, 6]].reshape(2, 9, 5))


# ------------------------------------------------------------------------------------------------
def test_band_metrics_on_hand_made_confusion_matrices():
    from eyegaze_multimodal_amd.predict import band_metrics_from_confusion as metric
    # class 2 is never predicted: precision 0 by zero_division, F1 0; it still counts in the macro mean
    m = metric([[3, 1, 0], [0, 4, 0], [1, 1, 0]])
    f0, f1 = 2 * (3 / 4) * (3 / 4) / (3 / 4 + 3 / 4), 2 * (4 / 6) * 1.0 / (4 / 6 + 1.0)
    assert m["accuracy"] == 7 / 10 and abs(m["f1"] - (f0 + f1 + 0.0) / 3) < 1e-15
    # class 1 is in neither the labels nor the predictions: left out of the mean
    m = metric([[2, 0, 1], [0, 0, 0], [0, 0, 3]])
    g0, g2 = 2 * 1.0 * (2 / 3) / (1.0 + 2 / 3), 2 * (3 / 4) * 1.0 / (3 / 4 + 1.0)
    assert m["accuracy"] == 5 / 6 and abs(m["f1"] - (g0 + g2) / 2) < 1e-15
    assert metric(np.diag([5, 2, 9])) == {"accuracy": 1.0, "f1": 1.0}
    assert set(metric(np.eye(3, dtype=np.int32))) == {"accuracy", "f1"}


@pytest.mark.parametrize("seed", range(6))
def test_band_metrics_equal_sklearn(seed):
    sk = pytest.importorskip("sklearn.metrics")
    from eyegaze_multimodal_amd.predict import band_metrics_from_confusion as metric
    rng = np.random.default_rng(seed)
    n, ncls = int(rng.integers(1, 200)), 3
    yt, yp = rng.integers(0, ncls if seed % 2 else 2, n), rng.integers(0, ncls if seed % 3 else 2, n)
    cm = np.zeros((ncls, ncls), np.int64)
    np.add.at(cm, (yt, yp), 1)
    got = metric(cm)
    assert abs(got["accuracy"] - sk.accuracy_score(yt, yp)) < 1e-12
    assert abs(got["f1"] - sk.precision_recall_fscore_support(yt, yp, average="macro", zero_division=0)[2]) < 1e-12


# ------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_three_functions():
    from eyegaze_multimodal_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "eyegaze_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+eg_ibs_inorm_band\s*\(const float\* conn, const int\* fidx, const float\* gamma, const float\* beta, void\* out, "
                     r"float\* xhat, int B,\s*int nbands, int nfeat, int E, int use_norm, int zero_band, int dtype, void\* stream\)", text)
    assert re.search(r"\bint64_t\s+eg_ibs_class_accumulate_scratch_elems\s*\(int B, int nbands, int nfeat, int E, int ncls\)", text)
    assert re.search(r"\bint\s+eg_ibs_class_accumulate\s*\(const float\* conn, const int\* fidx, const int64_t\* labels, float\* class_sum, "
                     r"int32_t\* class_count,\s*float\* scratch, int64_t scratch_elems, int B, int nbands, int nfeat, int E, int ncls, "
                     r"void\* stream\)", text)
    assert re.search(r"\bint\s+eg_ibs_inorm\s*\(const float\* conn, const int\* fidx, const float\* gamma, const float\* beta, void\* out,\s*"
                     r"float\* xhat, int B,\s*int nbands, int nfeat, int E, int use_norm, int dtype, void\* stream\)", text)      # unchanged
    assert "#define EG_ABI_VERSION 5" in text and L.lib().eg_abi_version() == 5 and L.ABI_VERSION == 5
    assert len(L.SIGNATURES["eg_ibs_inorm_band"]) == 14 and len(L.SIGNATURES["eg_ibs_inorm"]) == 13
    assert len(L.SIGNATURES["eg_ibs_class_accumulate"]) == 13 and len(L.SIGNATURES["eg_ibs_class_accumulate_scratch_elems"]) == 5
    assert all(L.exported_symbols()[n] for n in ("eg_ibs_inorm_band", "eg_ibs_class_accumulate", "eg_ibs_class_accumulate_scratch_elems"))


def _band(conn=P, fidx=P, gamma=P, beta=P, out=P, xhat=P, B=2, nbands=6, nfeat=7, E=64, use_norm=1, zero_band=-1, dtype=None):
    from eyegaze_multimodal_amd import _lib as L
    L.call("eg_ibs_inorm_band", conn, fidx, gamma, beta, out, xhat, B, nbands, nfeat, E, use_norm, zero_band,
           L.EG_BF16 if dtype is None else dtype, 0)


def test_inorm_band_refusals_need_no_gpu():
    from eyegaze_multimodal_amd import _lib as L
    who = "eg_ibs_inorm_band"
    with pytest.raises(L.EgError, match=f"{who}: bad dtype 7"):                    # reported first: everything else is wrong too
        _band(dtype=7, conn=0, zero_band=9)
    for zb, nb in ((6, 6), (-2, 6), (4, 4), (100, 6)):
        with pytest.raises(L.EgError, match=rf"{who}: zero_band={zb} outside \[-1, {nb}\)"):
            _band(zero_band=zb, nbands=nb)
    for name in ("conn", "fidx", "out"):
        with pytest.raises(L.EgError, match=f"{who}: null pointer"):
            _band(**{name: 0})
    for name in ("gamma", "beta"):
        with pytest.raises(L.EgError, match=f"{who}: instance norm needs gamma and beta"):
            _band(**{name: 0})
    for bad in (dict(B=0), dict(B=65536), dict(nbands=0), dict(nbands=9), dict(nfeat=0), dict(nfeat=8), dict(E=0)):
        with pytest.raises(L.EgError, match=f"{who}: bad shape"):
            _band(**bad)


def _acc(conn=P, fidx=P, labels=P, class_sum=P, class_count=P, scratch=P, scratch_elems=None, B=64, nbands=6, nfeat=7, E=64, ncls=3):
    from eyegaze_multimodal_amd import _lib as L
    if scratch_elems is None:
        scratch_elems = max(L.ibs_class_scratch_elems(B, nbands, nfeat, E, ncls), 0)
    L.call("eg_ibs_class_accumulate", conn, fidx, labels, class_sum, class_count, scratch, scratch_elems, B, nbands, nfeat, E, ncls, 0)


def test_class_accumulate_refusals_need_no_gpu():
    from eyegaze_multimodal_amd import _lib as L
    who = "eg_ibs_class_accumulate"
    for ncls in (0, 17, -1):
        with pytest.raises(L.EgError, match=rf"{who}: ncls={ncls} outside \[1, 16\]"):
            _acc(ncls=ncls, scratch_elems=0)
    for bad in (dict(B=0), dict(nbands=0), dict(nbands=9), dict(nfeat=0), dict(nfeat=8), dict(E=0)):
        with pytest.raises(L.EgError, match=f"{who}: bad shape"):
            _acc(scratch_elems=0, **bad)
    for name in ("conn", "fidx", "labels", "class_sum", "class_count", "scratch"):
        with pytest.raises(L.EgError, match=f"{who}: null pointer"):
            _acc(**{name: 0})
    need = L.ibs_class_scratch_elems(64, 6, 7, 64, 3)
    assert need == 4 * 3 * 6 * 7 * 64                                  # 64 samples in splits of 16: four partials per class sum
    with pytest.raises(L.EgError, match=f"{who}: scratch holds {need - 1} floats, {need} are needed"):
        _acc(scratch_elems=need - 1)
    with pytest.raises(L.EgError, match=f"{who}: null pointer"):       # one split needs no scratch, the outputs still must exist
        _acc(B=5, scratch=0, scratch_elems=0, class_sum=0)


@pytest.mark.parametrize("B,nbands,nfeat,E,ncls", [(1, 6, 7, 9, 1), (5, 6, 7, 64, 3), (64, 6, 4, 64, 3), (257, 6, 7, 64, 16),
                                                   (33, 6, 7, 1024, 3), (256, 6, 7, 1024, 3), (256, 6, 7, 4, 3)])
def test_class_accumulate_scratch_is_a_function_of_the_shapes(B, nbands, nfeat, E, ncls):
    from eyegaze_multimodal_amd import _lib as L
    need = L.ibs_class_scratch_elems(B, nbands, nfeat, E, ncls)
    ncol = nbands * nfeat * E
    assert need >= 0 and need % (ncls * ncol) == 0
    splits = need // (ncls * ncol)
    assert splits == 0 if B <= 16 else 2 <= splits <= -(-B // 16)
    assert need * 4 <= max(B * nbands * 7 * E * 4, 1 << 20) * ncls     # never more than a few copies of one batch's matrices
    if (B, E) == (256, 1024):
        assert splits == 4                                             # C = 32: chunks of 64 samples, 672 workgroups
    for bad in ((0, 6, 7, 64, 3), (4, 0, 7, 64, 3), (4, 9, 7, 64, 3), (4, 6, 8, 64, 3), (4, 6, 7, 0, 3), (4, 6, 7, 64, 0),
                (4, 6, 7, 64, 17)):
        assert L.ibs_class_scratch_elems(*bad) == -1


# ---- launches recorded on the CPU (profiles/tools/launch_trace.py's Recorder: listed, not issued) ----
def _recorded(kw, dtype, B, T, run):
    sys.path.insert(0, str(REPO / "profiles" / "tools"))
    from launch_trace import Recorder
    from eyegaze_multimodal_amd import DualEEGTransformer, _lib as L, engine as E, tokens
    rec = Recorder(L.call)
    saved = [(m, m.call) for m in (E, tokens)]
    for m, _ in saved:
        m.call = rec
    try:
        model = DualEEGTransformer(**kw)
        cpu = torch.device("cpu")
        model._flat.ensure(cpu, need_grad=False)
        eng = E.InferenceEngine(model, B, T, cpu, dtype)
        x = torch.zeros(B, model.cfg.in_channels, T)
        eng.forward(x, x, None)                        # packs; the lists below are of pack=False calls
        out = []
        for fn in run:
            rec.rows = []
            fn(eng, x)
            out.append([r[0] for r in rec.rows])
    finally:
        for m, c in saved:
            m.call = c
    return eng, out


def _a5_full():
    from tests.helpers import load_golden
    return load_golden("a5_full")[1]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_forward_band_masks_shares_what_the_mask_does_not_touch(dtype):
    from eyegaze_multimodal_amd import _lib as L
    seen = []
    bands = [None, 0, 1, 2, 3, 4, 5]
    eng, (plain, masked) = _recorded(_a5_full(), dict(bf16=L.EG_BF16, f32=L.EG_F32)[dtype], 4, 1024, [
        lambda eng, x: eng.forward(x, x, None, pack=False),
        lambda eng, x: eng.forward_band_masks(x, x, bands, seen.append, pack=False)])
    assert seen == list(range(7)) and eng.a["x0"] is eng.a["xa"] and "xf" in eng.sc
    i = plain.index("eg_ibs_inorm")
    tok = plain[i:i + 5]
    assert [n for n in tok if n.startswith("eg_g")] == ["eg_gemm_nt", "eg_gelu_fwd", "eg_gemm_nt"] and tok[4] == "eg_rows_copy"
    k = masked.index("eg_ibs_inorm_band")
    shared, encoder = plain[:i] + plain[i + 5:k + 5], plain[k + 5:]
    # the front end, eg_ibs_analytic / eg_ibs_pairs and the spectrogram family once, then seven times the tokeniser and the encoder
    assert masked[:k] == shared
    for name in ("eg_window_pack", "eg_ibs_analytic", "eg_ibs_pairs", "eg_stft_logmag", "eg_spec_conv1_fwd"):
        assert masked.count(name) == plain.count(name) >= 1 and name in shared and name not in encoder
    assert masked[k:] == (["eg_ibs_inorm_band"] + tok[1:] + encoder) * 7
    assert masked.count("eg_ibs_inorm_band") == 7 and "eg_ibs_inorm" not in masked and "eg_ibs_class_accumulate" not in masked
    layer = "eg_attn_block_fwd" if eng.attn_block else eng._attn_core + "_fwd"
    assert encoder.count(layer) >= eng.cfg.num_layers and masked.count(layer) == 7 * encoder.count(layer)
    assert masked.count("eg_layernorm_fwd") == 7 * plain.count("eg_layernorm_fwd") > 0         # the final norm at least


def test_conn_stats_adds_one_launch_and_unset_adds_none():
    from eyegaze_multimodal_amd import _lib as L, engine as E
    B = 4

    def with_stats(eng, x):
        ncls, nb, nf, Cn = 3, eng.ib["nb"], eng.cfg.num_ibs_features, eng.C
        eng.conn_stats = E.ConnStats(torch.zeros(B, dtype=torch.int64), torch.zeros(ncls, nb, nf, Cn, Cn),
                                     torch.zeros(ncls, dtype=torch.int32),
                                     torch.zeros(max(L.ibs_class_scratch_elems(B, nb, nf, Cn * Cn, ncls), 0)))
        try:
            eng.forward(x, x, None, pack=False)
            eng.forward_band_masks(x, x, [None, 3], lambda i: None, pack=False)
        finally:
            eng.conn_stats = None

    def bad_request(eng, x):
        eng.conn_stats = E.ConnStats(torch.zeros(B, dtype=torch.int32), torch.zeros(3, 6, 7, 8, 8), torch.zeros(3, dtype=torch.int32),
                                     torch.zeros(0))
        try:
            with pytest.raises(L.EgError, match="conn_stats.labels must be a contiguous torch.int64"):
                eng.forward(x, x, None, pack=False)
        finally:
            eng.conn_stats = None

    plain_fwd = lambda eng, x: eng.forward(x, x, None, pack=False)
    eng, (before, stats, _, after) = _recorded(_a5_full(), L.EG_BF16, B, 1024, [plain_fwd, with_stats, bad_request, plain_fwd])
    assert eng.conn_stats is None and after == before and "eg_ibs_class_accumulate" not in before
    i = before.index("eg_ibs_pairs")
    assert stats[:len(before) + 1] == before[:i + 1] + ["eg_ibs_class_accumulate"] + before[i + 1:]
    assert stats.count("eg_ibs_class_accumulate") == 2 and stats.count("eg_ibs_pairs") == 2      # once per forward_band_masks call


def test_the_parent_s_launch_list_is_unchanged():
    """a forward of the inference engine and an eval forward of the training engine still issue the same entry points, and the
    synchrony tokeniser's five launches are where they were: straight after eg_ibs_pairs"""
    from eyegaze_multimodal_amd import _lib as L
    eng, (plain,) = _recorded(_a5_full(), L.EG_BF16, 4, 1024, [lambda eng, x: eng.forward(x, x, None, pack=False)])
    i = plain.index("eg_ibs_pairs")
    assert plain[i + 1:i + 6] == ["eg_ibs_inorm", "eg_gemm_nt", "eg_gelu_fwd", "eg_gemm_nt", "eg_rows_copy"]
    assert plain[i + 6] == "eg_stft_logmag" and plain.count("eg_rows_copy") == 1


@pytest.mark.parametrize("kw", [dict(in_channels=8, max_len=256, use_spectrogram=False, use_robust_ibs=False),
                                dict(in_channels=8, max_len=256, use_spectrogram=False, use_ibs=False)], ids=["scalar_ibs", "no_ibs"])
def test_a_model_without_matrices_runs_one_pass(kw):
    from eyegaze_multimodal_amd import _lib as L
    seen = []
    eng, (plain, masked) = _recorded(kw, L.EG_BF16, 4, 1024, [
        lambda eng, x: eng.forward(x, x, None, pack=False),
        lambda eng, x: eng.forward_band_masks(x, x, [None, 0, 1, 2, 3, 4, 5], seen.append, pack=False)])
    assert masked == plain and seen == list(range(7)) and "xf" not in eng.sc


def test_forward_band_masks_refuses_a_band_out_of_range():
    from eyegaze_multimodal_amd import _lib as L
    for bad in (6, -1, "alpha", 1.0):
        with pytest.raises(L.EgError, match="a band is None or an int in"):
            _recorded(_a5_full(), L.EG_BF16, 4, 1024, [lambda eng, x: eng.forward_band_masks(x, x, [None, bad], lambda i: None)])


def test_argument_checks_of_the_two_public_calls():
    from eyegaze_multimodal_amd import DualEEGTransformer
    from eyegaze_multimodal_amd.predict import connectivity_statistics, frequency_sensitivity
    model = DualEEGTransformer(**_a5_full())
    x, y = torch.zeros(4, 8, 1024), torch.zeros(4, dtype=torch.long)
    for fn in (connectivity_statistics, frequency_sensitivity):
        with pytest.raises(ValueError, match="N >= 1"):
            fn(model, x[:0], x[:0], y[:0])
        with pytest.raises(ValueError, match="batch_size >= 1"):
            fn(model, x, x, y, batch_size=0)
        with pytest.raises(ValueError, match="labelled windows"):
            fn(model, x, x, y[:3])
        with pytest.raises(ValueError):
            fn(model, x, x, None)
    with pytest.raises(ValueError, match="max_samples"):
        connectivity_statistics(model, x, x, y, max_samples=0)
    with pytest.raises(ValueError, match="6 band names"):
        frequency_sensitivity(model, x, x, y, band_names=["a", "b"])
    with pytest.raises(ValueError, match="1 to 16 class names"):
        connectivity_statistics(model, x, x, y, class_names=[str(i) for i in range(17)])
