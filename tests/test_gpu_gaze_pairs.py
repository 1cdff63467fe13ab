"""GPU tests of the gaze pair analysis.  eg_gaze_pair_stats against the numpy restatement (tests/gazepair_ref.py,
itself pinned to the reference by tests/test_gaze_pairs_host.py): mask counts as integers, the IoU as fp32 bits, the fp64 sums
inside n 2^-53 sum |terms| of math.fsum, centres and distances inside the bound that propagates; against the reference's own
outputs (tests/golden/gaze_pairs.npz) under the CPU test's gates.  Every call runs with sentinels behind `out` and the workspace
and compares its inputs byte for byte afterwards.  eg_row_cosine against F.normalize's values and an fp64 numpy value; the model
level against MultimodalTrainer.evaluate and numpy group-bys."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd import gaze as G  # noqa: E402
from eyegaze_multimodal_amd import gaze_analysis as A  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from tests import gazepair_ref as R  # noqa: E402
from tests.test_gaze_pairs_host import GOLD, KINDS, PAIRS, SIZES, TABLES, check_against_fixture, f32_bits  # noqa: E402

DEV = "cuda"
SENTINEL = -7777.25     # in every double behind (and, before the call, inside) out and the workspace
GUARD = 64              # sentinel doubles behind every buffer
NF = L.GAZE_PAIR_FIELDS


def stream():
    return torch.cuda.current_stream().cuda_stream


def raw_call(store: np.ndarray, pairs, table: np.ndarray, threshold: float = 0.1):
    """one eg_gaze_pair_stats call assembled here: sentinels behind out and the workspace, the store, the table and pair_img
    compared byte for byte afterwards -> (out [n_pairs, 14] f64, workspace [n_images, 8] f64), host arrays; a row that was not
    written still holds SENTINEL"""
    n, F, W, _ = store.shape
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    d_store, d_tab, d_pairs = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (store, table.astype(np.float32), pairs))
    need = L.gaze_pair_stats_workspace_bytes(n)
    assert need == 64 * n
    ws = torch.full((need // 8 + GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    out = torch.full((len(pairs) * NF + GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    call("eg_gaze_pair_stats", ptr(d_store), n, F, W, ptr(d_pairs), len(pairs), ptr(d_tab), float(threshold), ptr(ws), need, ptr(out),
         stream())
    torch.cuda.synchronize()
    assert (ws[need // 8:] == SENTINEL).all() and (out[len(pairs) * NF:] == SENTINEL).all()
    assert d_store.cpu().numpy().tobytes() == store.tobytes() and d_pairs.cpu().numpy().tobytes() == pairs.tobytes()
    assert d_tab.cpu().numpy().tobytes() == table.astype(np.float32).tobytes()
    return out[:len(pairs) * NF].view(-1, NF).cpu().numpy(), ws[:need // 8].view(n, 8).cpu().numpy()


def as_rows(out: np.ndarray):
    return [dict(zip(R.FIELDS, (float(v) for v in row))) for row in out]


def judge_against_restatement(out: np.ndarray, ws: np.ndarray, store: np.ndarray, pairs, table: np.ndarray, threshold: float = 0.1):
    want, st = R.pair_table(store, pairs, table, threshold)
    for i, s in st.items():
        assert abs(s["S"]) >= 1.0 or s["A"] == 0.0, (i, s["S"])                  # the branch cannot hinge on the last bits of S
        b = R.sum_bounds(s)
        for k, name in enumerate(("S", "Sy", "Sx", "A")):
            assert abs(ws[i, k] - s[name]) <= b[name], (i, name, ws[i, k], s[name], b[name])
        assert ws[i, 4] == float(s["min"]) and ws[i, 5] == float(s["max"]) and ws[i, 6] == 0.0 and ws[i, 7] == 0.0
    for p, ((a, b), got, ref) in enumerate(zip(np.asarray(pairs).tolist(), as_rows(out), want)):
        for k in ("inter", "union", "na", "nb"):
            assert got[k] == ref[k], (p, k, got[k], ref[k])
        assert f32_bits(got["overlap"]) == f32_bits(ref["overlap"]) and float(np.float32(got["overlap"])) == got["overlap"], p
        for img, side in ((a, "a"), (b, "b")):
            by, bx = R.centre_bounds(st[img], R.U64)
            assert abs(got[f"cy_{side}"] - ref[f"cy_{side}"]) <= by and abs(got[f"cx_{side}"] - ref[f"cx_{side}"]) <= bx, (p, side)
            assert got[f"S_{side}"] == ws[img, 0] and got[f"A_{side}"] == ws[img, 3]
        assert abs(got["distance"] - ref["distance"]) <= R.distance_bound(st[a], st[b], R.U64, ref["distance"]), p


# ---------------------------------------------------------------------------------------------------------------
# eg_gaze_pair_stats
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES)
def test_pair_stats_against_the_restatement_and_the_reference(size, kind):
    """(8, 8): the smallest served, 4 chunks; (16, 24): every image on a 16-byte boundary; (17, 23): 1173 bytes per image, only
    image 0 on a boundary, 7 tail pixels; (64, 64): 256 chunks, one per thread"""
    prefix = f"{size[0]}x{size[1]}"
    store = GOLD[f"{prefix}/store"]
    out, ws = raw_call(store, PAIRS, TABLES[kind])
    judge_against_restatement(out, ws, store, PAIRS, TABLES[kind])
    check_against_fixture(prefix, store, PAIRS, kind)[0](as_rows(out))
    same = R.PAIRS.index((1, 1))
    assert out[same, 0] == 0.0 and out[same, 1] == 1.0                          # (a, a): exactly


@pytest.mark.parametrize("kind", KINDS)
def test_the_large_pair_of_the_fixture(kind):
    store = R.seeded_images(int(GOLD["big/seed"]), *R.BIG, 2)
    out, ws = raw_call(store, [(0, 1)], TABLES[kind])
    judge_against_restatement(out, ws, store, [(0, 1)], TABLES[kind])
    check_against_fixture("big", store, [(0, 1)], kind)[0](as_rows(out))


def test_the_largest_served_size():
    """(512, 512): 16384 chunks, 64 steps per thread; against the restatement only"""
    store = R.seeded_images(512, 512, 512, 2)
    out, ws = raw_call(store, [(0, 1)], TABLES["raw"])
    judge_against_restatement(out, ws, store, [(0, 1)], TABLES["raw"])


def test_more_than_one_step_per_thread_with_a_tail_and_a_threshold():
    """(75, 75): 5625 pixels = 351 chunks (threads 0-94 take two) and 9 tail pixels, every image but the first off the 16-byte
    grid; at another threshold"""
    store = R.with_extras(R.seeded_images(75, 75, 75, 4))
    pairs = [(0, 1), (1, 2), (3, 0), (2, 2), (4, 5), (5, 1)]
    for kind, thr in (("raw", 0.35), ("norm", 0.1)):
        out, ws = raw_call(store, pairs, TABLES[kind], thr)
        judge_against_restatement(out, ws, store, pairs, TABLES[kind], thr)


def test_pairs_outside_the_store_are_skipped_and_nothing_else_is_touched():
    store = GOLD["17x23/store"]
    pairs = [(0, 1), (-1, 2), (3, len(store)), (4, 5), (len(store), -1)]
    out, ws = raw_call(store, pairs, TABLES["raw"])
    assert (out[[1, 2, 4]] == SENTINEL).all()                                  # skipped by design: their rows are not written
    alone, _ = raw_call(store, [(0, 1), (4, 5)], TABLES["raw"])
    assert out[[0, 3]].tobytes() == alone.tobytes()
    assert not (ws == SENTINEL).any()                                          # every image of the store is computed


def test_bytes_do_not_depend_on_the_run_the_batch_or_the_place_in_the_store():
    store = GOLD["17x23/store"]
    rng = np.random.default_rng(5)
    pairs = rng.integers(0, len(store), (37, 2)).astype(np.int32)
    pairs[11] = (0, 1)
    for kind in KINDS:
        first, ws1 = raw_call(store, pairs, TABLES[kind])
        again, ws2 = raw_call(store, pairs, TABLES[kind])
        assert first.tobytes() == again.tobytes() and ws1.tobytes() == ws2.tobytes()
        alone, _ = raw_call(store, [(0, 1)], TABLES[kind])
        assert alone[0].tobytes() == first[11].tobytes()
        # the same two images one place further on: other base addresses, 1173 bytes apart (image 0's wide loads become narrow ones)
        moved, ws3 = raw_call(np.roll(store, 1, axis=0), [(1, 2)], TABLES[kind])
        assert moved[0].tobytes() == first[11].tobytes() and ws3[1:].tobytes() == ws1[:-1].tobytes()


def test_spatial_statistics_and_sensitivity():
    store_np = GOLD["16x24/store"]
    store = G.GazeImageStore(torch.from_numpy(store_np).to(DEV))
    for kind in KINDS:
        got = A.spatial_statistics(store, PAIRS, normalised=kind == "norm")
        raw, _ = raw_call(store_np, PAIRS, TABLES[kind])
        assert set(got) == {"distance", "overlap", "cy_a", "cx_a", "cy_b", "cx_b", "inter", "union", "na", "nb", "total", "abs_total"}
        assert all(v.device.type == "cuda" for v in got.values())
        for i, k in enumerate(R.FIELDS[:6]):
            assert got[k].dtype == torch.float64 and got[k].cpu().numpy().tobytes() == np.ascontiguousarray(raw[:, i]).tobytes(), k
        for i, k in enumerate(("inter", "union", "na", "nb")):
            assert got[k].dtype == torch.int64 and np.array_equal(got[k].cpu().numpy(), raw[:, 6 + i].astype(np.int64)), k
        assert np.array_equal(got["total"].cpu().numpy(), raw[:, 10:12]) and np.array_equal(got["abs_total"].cpu().numpy(), raw[:, 12:14])
    # a device tensor of pairs is taken as it is; the rows gathered through win_pair are the pairs' rows
    pair_dev = torch.from_numpy(np.ascontiguousarray(PAIRS)).to(DEV)
    rng = np.random.default_rng(7)
    win_pair = rng.integers(0, len(PAIRS), 50)
    labels, pred = rng.integers(0, 3, 50), rng.integers(0, 3, 50)
    st = A.spatial_statistics(store, pair_dev, normalised=False)
    rows = A.spatial_sensitivity(store, pair_dev, torch.from_numpy(win_pair).to(DEV), torch.from_numpy(pred).to(DEV), labels, normalised=False)
    assert list(rows) == ["distance", "overlap", "correct", "label", "label_name"]
    assert np.array_equal(rows["distance"], st["distance"].cpu().numpy()[win_pair])
    assert np.array_equal(rows["overlap"], st["overlap"].cpu().numpy()[win_pair])
    assert np.array_equal(rows["correct"], (pred == labels).astype(np.int64)) and np.array_equal(rows["label"], labels)
    assert rows["label_name"].tolist() == [A.DEFAULT_CLASS_NAMES[l] for l in labels]
    with pytest.raises(ValueError, match="win_pair names pair"):
        A.spatial_sensitivity(store, pair_dev, [0, len(PAIRS)], [0, 0], [0, 0])


# ---------------------------------------------------------------------------------------------------------------
# eg_row_cosine
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.COSINE_D)
def test_row_cosine(D):
    a, b = R.cosine_inputs(int(GOLD["seed"]), D)
    da, db = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    out = torch.full((R.COSINE_N + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    call("eg_row_cosine", ptr(da), ptr(db), R.COSINE_N, D, ptr(out), stream())
    torch.cuda.synchronize()
    assert (out[R.COSINE_N:] == SENTINEL).all() and torch.equal(da.cpu(), torch.from_numpy(a)) and torch.equal(db.cpu(), torch.from_numpy(b))
    got = out[:R.COSINE_N].cpu().numpy()
    assert got[3] == 0.0                                                       # a zero row: the 1e-12 clamp, 0 / 1e-12 |b|
    # F.normalize's route: every element of either unit vector within 2 u, their D products within 3 u each, summed in fp32 in
    # any order (D u more); |sum of products of unit vectors| <= 1 by Cauchy-Schwarz: (D + 6) u in all
    assert np.all(np.abs(got - GOLD[f"cosine/{D}"]) <= (D + 6) * 2.0 ** -24)
    assert np.all(np.abs(got.astype(np.float64) - R.row_cosine(a, b)) <= 4 * 2.0 ** -24)
    assert abs(got[4] + 1.0) <= 4 * 2.0 ** -24                                   # b = -a
    assert np.array_equal(A.row_cosine(da, db).cpu().numpy(), got)
    table = A.feature_correlation(da, db, [0, 1, 2, 0, 1])
    assert list(table) == ["similarity", "label", "label_name"] and np.array_equal(table["similarity"], got)
    assert table["label_name"].tolist() == ["Single", "Competition", "Cooperation", "Single", "Competition"]


# ---------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------
def test_predictions_pair_performance_and_feature_correlation(monkeypatch):
    from eyegaze_multimodal_amd import train_art
    from eyegaze_multimodal_amd.train_multimodal_fuzzy_fusion import build_from_config, synth_multimodal
    B, C, T, F_, W_ = 8, 8, 1024, 64, 16
    config = {"data": {"window_size": T, "num_classes": 3},
              "eeg_encoder": {"in_channels": C, "d_model": 64, "num_layers": 2, "num_heads": 2, "d_ff": 128, "use_spectrogram": True,
                              "use_ibs": False, "use_cross_attention": True},
              "gaze_encoder": {"d_model": 64}, "fusion": {"mode": "full"},
              "training": {"encoder_learning_rate": 1e-4, "fusion_learning_rate": 1e-3, "weight_decay": 0.01, "epochs": 1,
                           "compute_dtype": "bf16"}}
    tr = build_from_config(config, DEV)
    data = [t.to(DEV) for t in synth_multimodal(2 * B, C, T, F_, W_, 3, seed=21)]
    batches = [tuple(t[k * B:(k + 1) * B] for t in data) for k in range(2)]
    seen = []
    real = train_art.macro_metrics
    monkeypatch.setattr(train_art, "macro_metrics", lambda yt, yp: seen.append((yt.copy(), yp.copy())) or real(yt, yp))
    metrics = tr.evaluate(batches)
    got = A.predict_multimodal(tr, batches)
    (yt, yp), = seen
    assert np.array_equal(got["y_true"], yt) and np.array_equal(got["y_pred"], yp)      # the argmax evaluate computes
    assert got["y_prob"].shape == (2 * B, 3) and np.allclose(got["y_prob"].sum(1), 1.0, atol=1e-6)
    assert np.array_equal(got["y_prob"].argmax(1), yp) and abs(float(got["alpha"].mean()) - metrics["alpha_mean"]) < 1e-6
    # pair accuracy against a numpy group-by
    ids = np.random.default_rng(3).integers(100, 105, 2 * B)
    table = A.pair_performance(torch.from_numpy(ids).to(DEV), torch.from_numpy(yt).to(DEV), torch.from_numpy(yp).to(DEV))
    want = sorted(((float(np.mean(yt[ids == i] == yp[ids == i])), int(i), int(np.sum(yt[ids == i] == yp[ids == i])), int(np.sum(ids == i)))
                   for i in np.unique(ids)))
    assert [tuple(r) for r in zip(table["accuracy"].tolist(), table["pair_id"].tolist(), table["correct_count"].tolist(),
                                  table["total_count"].tolist())] == want
    # the image engine's pooled features of its last forward, player against player
    img = tr._engines(B, T, F_, W_)[1]
    feat = img.a["feat"].float().view(B, 2, -1).cpu().numpy()
    corr = A.image_feature_correlation(img, batches[1][4])
    assert np.all(np.abs(corr["similarity"] - R.row_cosine(feat[:, 0], feat[:, 1])) <= 4 * 2.0 ** -24)
    assert np.array_equal(corr["label"], batches[1][4].cpu().numpy())
