"""CPU tests of the gaze pair analysis: the numpy restatement (tests/gazepair_ref.py) against the reference's own
outputs (tests/golden/gaze_pairs.npz, written by tests/make_golden_gaze_pairs.py from 6_Utils/error_analysis.py) -- mask counts as
integers, the IoU as fp32 bits, centres and distances inside the worst-case bound of an fp32 summation in any order -- the host
statistics of gaze_analysis.py against the reference's DataFrames and scipy's p-values, and every refusal of the two entry points
that is reached without a GPU."""
import numpy as np
import pytest

from eyegaze_multimodal_amd import _lib as L
from eyegaze_multimodal_amd import gaze_analysis as A
from tests import gazepair_ref as R
from tests.test_capi_symbols import REPO

GOLD = np.load(REPO / "tests" / "golden" / "gaze_pairs.npz")
SIZES = [tuple(int(v) for v in s) for s in GOLD["sizes"]]
PAIRS = GOLD["pairs"]
KINDS = ("norm", "raw")
TABLES = R.tables()
# The worst relative difference between betainc's p-values and scipy's over the fixture's 18 tests, measured here, is 1.64e-13
# (test_p_values_against_scipy prints it); the gate is 16 times that.  A gate looser than 1e-9 would mean that the continued
# fraction is wrong, not that the gate is tight.
P_MEASURED = 1.64e-13
P_GATE = 16 * P_MEASURED


def f32_bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def check_against_fixture(prefix: str, store: np.ndarray, pairs, kind: str):
    """the CPU gates of the issue, for restatement rows and (tests/test_gpu_gaze_pairs.py) device rows alike: returns a function
    that judges a list of row dicts"""
    _, st = R.pair_table(store, pairs, TABLES[kind])
    cen, dist = GOLD[f"{prefix}/{kind}/centres"], GOLD[f"{prefix}/{kind}/distance"]
    counts, over = GOLD[f"{prefix}/{kind}/counts"], GOLD[f"{prefix}/{kind}/overlap"]

    def judge(rows):
        assert len(rows) == len(pairs)
        for p, ((a, b), row) in enumerate(zip(np.asarray(pairs).tolist(), rows)):
            assert [int(row[k]) for k in ("inter", "union", "na", "nb")] == counts[p].tolist(), (prefix, kind, p)
            assert f32_bits(row["overlap"]) == f32_bits(over[p]) and float(np.float32(row["overlap"])) == row["overlap"], (prefix, kind, p)
            for img, side in ((a, "a"), (b, "b")):
                by, bx = R.centre_bounds(st[img], R.U32)
                assert abs(row[f"cy_{side}"] - cen[img, 0]) <= by and abs(row[f"cx_{side}"] - cen[img, 1]) <= bx, (prefix, kind, p, side)
            assert abs(row["distance"] - dist[p]) <= R.distance_bound(st[a], st[b], R.U32), (prefix, kind, p)
    return judge, st


# ---------------------------------------------------------------------------------------------------------------
# the restatement is the reference's
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES)
def test_restatement_against_the_reference(size, kind):
    prefix = f"{size[0]}x{size[1]}"
    store = GOLD[f"{prefix}/store"]
    rows, _ = R.pair_table(store, PAIRS, TABLES[kind])
    judge, st = check_against_fixture(prefix, store, PAIRS, kind)
    judge(rows)
    for i, s in st.items():                                                    # the branch the reference took
        assert (s["S"] >= 1e-8) == bool(GOLD[f"{prefix}/{kind}/centres"][i, 2]) and R.well_conditioned(s)


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_on_the_large_pair(kind):
    store = R.seeded_images(int(GOLD["big/seed"]), *R.BIG, 2)
    rows, _ = R.pair_table(store, [(0, 1)], TABLES[kind])
    check_against_fixture("big", store, [(0, 1)], kind)[0](rows)


def test_fixture_covers_what_it_claims():
    assert SIZES == R.SIZES == [(8, 8), (16, 24), (17, 23), (64, 64)] and PAIRS.tolist() == [list(p) for p in R.PAIRS]
    assert (16 * 24 * 3) % 16 == 0 and (17 * 23 * 3) % 16 != 0                  # wide loads everywhere; unaligned bases and a tail
    for F, W in SIZES:
        p = f"{F}x{W}"
        store = GOLD[f"{p}/store"]
        assert np.array_equal(store, R.with_extras(R.seeded_images(int(GOLD[f"{p}/seed"]), F, W)))
        assert not store[R.ZERO].any() and (store[R.CONST] == np.asarray(R.CONST_RGB, np.uint8)).all()
        zz = R.PAIRS.index((R.ZERO, R.ZERO))
        assert GOLD[f"{p}/raw/counts"][zz].tolist() == [0, 0, 0, 0] and GOLD[f"{p}/raw/overlap"][zz] == 0.0
        assert GOLD[f"{p}/raw/centres"][R.ZERO].tolist() == [112.0, 112.0, 0.0]  # S == 0: the literal, whatever F and W are
        same = R.PAIRS.index((1, 1))
        for kind in KINDS:
            assert GOLD[f"{p}/{kind}/distance"][same] == 0.0 and GOLD[f"{p}/{kind}/overlap"][same] == 1.0
            taken = GOLD[f"{p}/{kind}/centres"][:, 2]
            assert 0 < taken.sum() < len(taken) or kind == "raw"                # both branches under the normalised table
        assert GOLD[f"{p}/raw/centres"][:, 2].sum() == 7                       # raw: every image but the all-zero one
    counts = np.bincount(PAIRS.ravel())
    assert counts[0] >= 4                                                      # an image shared by several pairs


def test_threshold_and_epsilon_act_as_float32():
    """the mask at the threshold: a pixel with q == float32(0.1) is outside (0.1f > 0.1f is false), one ulp above is inside"""
    g = np.asarray([[0.0, 1.0, np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(1))]], np.float32)
    st = R.image_stats(g)
    # d = (1 - 0) + 1e-8f rounds to 1: q == g
    assert R.mask(g, st, 0.1).tolist() == [[False, True, False, True]]


# ---------------------------------------------------------------------------------------------------------------
# host statistics
# ---------------------------------------------------------------------------------------------------------------
def frame(prefix):
    return {str(c): GOLD[f"{prefix}/{c}"] for c in GOLD[f"{prefix}/columns"]}


def close(a, b, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= rel * np.abs(b)))


def test_pair_performance_statistics_and_hard_pairs():
    import torch
    ids, yt, yp = (torch.from_numpy(GOLD[f"perf/{k}"]) for k in ("pair_ids", "y_true", "y_pred"))
    got, want = A.pair_performance(ids, yt, yp), frame("perf/pair_stats")
    assert list(got) == list(want)
    order = np.lexsort((want["pair_id"], want["accuracy"]))                    # the reference leaves ties in no defined order
    for k in ("pair_id", "correct_count", "total_count"):
        assert np.array_equal(got[k], want[k][order]) and got[k].dtype == np.int64, k
    assert np.array_equal(got["accuracy"], want["accuracy"][order])            # the sort key: the same fp64 quotients
    assert np.array_equal(np.sort(got["accuracy"]), got["accuracy"]) and 5 not in got["pair_id"]
    assert sorted(A.hard_pairs(got)) == sorted(GOLD["perf/hard_pairs"].tolist())
    assert sorted(A.hard_pairs(got, 50)) == sorted(GOLD["perf/hard_pairs_50"].tolist())
    summary = A.pair_statistics(got)
    assert list(summary) == [str(k) for k in GOLD["perf/summary_keys"]]
    assert close(list(summary.values()), GOLD["perf/summary"])
    assert summary["n_pairs"] == 12 and isinstance(summary["n_pairs"], int) and isinstance(summary["hard_pairs_count"], int)
    # ties are broken by pair_id
    tie = A.pair_performance(torch.tensor([9, 9, 2, 2, 7]), torch.tensor([0, 1, 0, 1, 2]), torch.tensor([0, 0, 0, 0, 2]))
    assert tie["pair_id"].tolist() == [2, 9, 7] and tie["accuracy"].tolist() == [0.5, 0.5, 1.0]


def test_error_distribution_and_confusion_analysis():
    yt, yp = GOLD["perf/y_true"], GOLD["perf/y_pred"]
    for got, want in ((A.error_distribution(yt, yp), frame("perf/errors")), (A.confusion_analysis(yt, yp), frame("perf/confusion"))):
        assert list(got) == list(want)
        for k in want:
            if want[k].dtype.kind == "f":
                assert close(got[k], want[k]), k
            else:
                assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("case", range(int(GOLD["stats/n_cases"])))
def test_class_statistics_and_tests_by_class(case):
    values, labels = GOLD[f"stats/{case}/values"], GOLD[f"stats/{case}/labels"]
    got, want = A.class_statistics(values, labels), frame(f"stats/{case}/class")
    assert list(got) == list(want)
    assert np.array_equal(got["class"], want["class"]) and np.array_equal(got["n_samples"], want["n_samples"])
    for k in ("mean", "std", "min", "max", "median", "q25", "q75"):
        assert close(got[k], want[k]), k
    got, want = A.statistical_tests_by_class(values, labels), frame(f"stats/{case}/tests")
    assert list(got) == list(want)
    for k in ("comparison", "effect_size", "significant"):
        assert np.array_equal(got[k], want[k]), k
    assert close(got["statistic"], want["statistic"])


def test_p_values_against_scipy():
    worst, n = 0.0, 0
    for case in range(int(GOLD["stats/n_cases"])):
        got = A.statistical_tests_by_class(GOLD[f"stats/{case}/values"], GOLD[f"stats/{case}/labels"])["p_value"]
        want = GOLD[f"stats/{case}/tests/p_value"]
        assert got.shape == want.shape and (want > 0).all()
        worst, n = max(worst, float(np.max(np.abs(got - want) / want))), n + len(want)
    print(f"p-values: worst relative difference to scipy over {n} tests {worst:.3e}, gate {P_GATE:.3e}")
    assert P_GATE < 1e-9 and n == 18
    assert worst <= P_GATE, worst


def test_betainc_identities():
    assert A.betainc(1.0, 1.0, 0.3) == pytest.approx(0.3, rel=1e-15)            # the uniform distribution
    assert A.betainc(2.0, 3.0, 0.4) + A.betainc(3.0, 2.0, 0.6) == pytest.approx(1.0, rel=1e-15)
    assert A.betainc(0.5, 0.5, 0.5) == pytest.approx(0.5, rel=1e-14)            # the arcsine law's median
    assert A.betainc(2.0, 1.0, 0.25) == pytest.approx(0.0625, rel=1e-14)        # x^a for b = 1
    assert A.betainc(3.0, 2.0, 0.0) == 0.0 and A.betainc(3.0, 2.0, 1.0) == 1.0 and np.isnan(A.betainc(0.0, 1.0, 0.5))


def test_fewer_than_two_classes_give_no_rows():
    got = A.statistical_tests_by_class(np.arange(5.0), np.zeros(5, np.int64))
    assert list(got) == ["comparison", "statistic", "p_value", "significant", "effect_size"] and all(len(v) == 0 for v in got.values())


def test_write_csv(tmp_path):
    got = A.statistical_tests_by_class(GOLD["stats/0/values"], GOLD["stats/0/labels"])
    A.write_csv(tmp_path / "t.csv", got)
    lines = (tmp_path / "t.csv").read_text().splitlines()
    assert lines[0] == "comparison,statistic,p_value,significant,effect_size" and len(lines) == 5
    assert lines[1].startswith("ANOVA (all classes),5.58840") and lines[1].endswith(",True,eta^2 = 0.114")
    assert lines[2].endswith(",False,Cohen's d = -0.579")


def test_module_imports_neither_scipy_nor_pandas():
    import subprocess
    import sys
    code = ("import sys; import eyegaze_multimodal_amd.gaze_analysis; "
            "assert 'scipy' not in sys.modules and 'pandas' not in sys.modules, sorted(m for m in sys.modules if m in ('scipy', 'pandas'))")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=REPO)


# ---------------------------------------------------------------------------------------------------------------
# refusals that need no GPU
# ---------------------------------------------------------------------------------------------------------------
FAKE = 0x1000          # never dereferenced: every call below is refused before any launch


def pair_stats_args(**kw):
    a = dict(store=FAKE, n_images=4, F=16, W=24, pair_img=FAKE, n_pairs=3, norm=FAKE, threshold=0.1, workspace=FAKE,
             workspace_bytes=4 * 64, out=FAKE, stream=0)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw, match", [
    (dict(store=0), "null pointer"), (dict(pair_img=0), "null pointer"), (dict(norm=0), "null pointer"),
    (dict(workspace=0), "null pointer"), (dict(out=0), "null pointer"),
    (dict(n_images=0), "bad shape"), (dict(n_images=-3), "bad shape"), (dict(n_pairs=0), "bad shape"),
    (dict(F=7), r"F=7 outside \[8, 512\]"), (dict(F=513), "F=513 outside"), (dict(W=7), r"W=7 outside \[8, 512\]"),
    (dict(W=513), "W=513 outside"),
    (dict(threshold=float("nan")), "not finite"), (dict(threshold=float("inf")), "not finite"),
    (dict(workspace_bytes=4 * 64 - 1), "need 256 workspace bytes, the workspace has 255"),
    (dict(workspace=FAKE + 4), "8-byte boundaries"), (dict(out=FAKE + 1), "8-byte boundaries"),
])
def test_pair_stats_refusals(kw, match):
    with pytest.raises(L.EgError, match=match):
        L.call("eg_gaze_pair_stats", *pair_stats_args(**kw))


def test_pair_stats_workspace_bytes():
    assert L.gaze_pair_stats_workspace_bytes(1) == 64 and L.gaze_pair_stats_workspace_bytes(4096) == 4096 * 64
    assert L.gaze_pair_stats_workspace_bytes(0) == -1 and L.gaze_pair_stats_workspace_bytes(-1) == -1
    assert L.GAZE_PAIR_FIELDS == len(R.FIELDS) == len(A.PAIR_FIELDS) == 14


@pytest.mark.parametrize("args, match", [
    ((0, FAKE, 5, 64, FAKE, 0), "null pointer"), ((FAKE, 0, 5, 64, FAKE, 0), "null pointer"), ((FAKE, FAKE, 5, 64, 0, 0), "null pointer"),
    ((FAKE, FAKE, 0, 64, FAKE, 0), "N=0"), ((FAKE, FAKE, 5, 0, FAKE, 0), r"D=0 outside \[1, 4096\]"),
    ((FAKE, FAKE, 5, 4097, FAKE, 0), "D=4097 outside"),
])
def test_row_cosine_refusals(args, match):
    with pytest.raises(L.EgError, match=match):
        L.call("eg_row_cosine", *args)


def test_python_side_refusals():
    import torch
    from eyegaze_multimodal_amd import gaze as G
    store = G.GazeImageStore(torch.zeros(3, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="names images"):
        A.spatial_statistics(store, np.asarray([[0, 3]]))
    with pytest.raises(ValueError, match="n_pairs > 0"):
        A.spatial_statistics(store, np.zeros((0, 2), np.int64))
    with pytest.raises(ValueError, match="finite"):
        A.spatial_statistics(store, np.asarray([[0, 1]]), threshold=float("nan"))
    with pytest.raises(ValueError, match="three \\[n\\] tensors"):
        A.pair_performance(torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="two \\[N, D\\] tensors"):
        A.row_cosine(torch.zeros(3, 4), torch.zeros(3, 5))
