"""CPU tests of the t-SNE stages: the numpy restatement (tests/tsne_ref.py) against sklearn's recorded results
(tests/golden/tsne.npz, written by tests/make_golden_tsne.py) and, where scikit-learn is installed, against sklearn itself; the
host-side refusals of the eg_tsne_* entry points; the stop rules of the descent on a stub objective; the CSV columns."""
import csv
import re
from pathlib import Path

import numpy as np
import pytest

from tests import tsne_ref as R

REPO = Path(__file__).resolve().parent.parent
CASES = [(97, 24, 10.0), (257, 40, 30.0), (65, 768, 20.0)]


@pytest.fixture(scope="module")
def gold():
    return np.load(REPO / "tests" / "golden" / "tsne.npz")


def square(condensed, N):
    out = np.zeros((N, N), np.float64)
    out[np.triu_indices(N, 1)] = condensed
    return out + out.T


def test_fixture_is_what_the_maker_says(gold):
    assert (REPO / "tests" / "golden" / "tsne.npz").stat().st_size < 1 << 20
    for c, (N, D, _) in enumerate(CASES):
        assert gold[f"s{c}_X"].shape == (N, D) and gold[f"s{c}_X"].dtype == np.float32
        assert gold[f"s{c}_dist"].shape == (N * (N - 1) // 2,) and gold[f"s{c}_P"].dtype == np.float64
    assert gold["q_X"].shape == (300, 64) and gold["q_init"].shape == (8, 300, 2) and gold["q_kl"].shape == (8,)


@pytest.mark.parametrize("c", range(3))
def test_restatement_of_the_affinities_against_the_fixture(gold, c):
    N, _, perp = CASES[c]
    dist = square(gold[f"s{c}_dist"], N)
    # sklearn's distances (|x|^2 + |y|^2 - 2 x.y, rounded to float32) against the direct fp64 ones: the recorded distance
    direct, off = R.sqdist(gold[f"s{c}_X"]), ~np.eye(N, dtype=bool)
    assert (np.abs(direct - dist)[off] / direct[off]).max() <= 1.0001 * float(gold[f"s{c}_dist_restatement_distance"])
    cond, beta, steps = R.binary_search_perplexity(dist, perp)
    assert steps.max() <= 23 and (beta > 0).all()
    H = np.array([R.row_entropy(dist[i], i, beta[i])[0] for i in range(N)])
    assert np.abs(H - np.log(perp)).max() <= 1e-5
    P_sk = square(gold[f"s{c}_P"], N)
    P64, P32 = R.joint_from_cond(cond), R.joint_probabilities(dist, perp, np.float32)
    d64, d32 = np.abs(P64 - P_sk).max() / P_sk.max(), np.abs(P32 - P_sk).max() / P_sk.max()
    print(f"case {c}: P {d64:.2e} (fp64) / {d32:.2e} (float32 storage) from sklearn's, recorded "
          f"{float(gold[f's{c}_P_restatement_distance']):.2e}")
    assert d64 <= 1e-12 and d32 <= 1.0001 * float(gold[f"s{c}_P_restatement_distance"])
    assert abs(P64.sum() - 1.0) < 1e-12 + N * N * R.TINY                     # (the 2^-52 floor under every entry adds up)
    assert (P64 == P64.T).all() and (np.diag(P64) == 0).all()


@pytest.mark.parametrize("c", range(3))
def test_restatement_of_the_gradient_against_the_fixture(gold, c):
    N = CASES[c][0]
    P = square(gold[f"s{c}_P"].astype(np.float32), N)                         # the float32 P the entry point is fed
    for k in range(2):
        for ex in (12, 1):
            tag = f"s{c}_pos{k}_e{ex}"
            kl, grad = R.kl_divergence(gold[f"s{c}_pos{k}"], P, float(ex))
            assert abs(kl - gold[tag + "_kl"]) / abs(gold[tag + "_kl"]) <= 1.0001 * float(gold[tag + "_kl_restatement_distance"]) + 1e-15
            d = np.abs(grad.astype(np.float32) - gold[tag + "_grad"]).max() / np.abs(gold[tag + "_grad"]).max()
            assert d <= 1.0001 * float(gold[tag + "_grad_restatement_distance"]) + 1e-15


def test_restatement_of_the_descent_reaches_sklearns_divergence(gold):
    """the fp64 driver from the first fixture init: its KL -- what t-SNE optimises -- lies inside sklearn's seed spread taken
    again as the margin; the coordinates are no yardstick (they differ by the scale of the map after 50 iterations)"""
    X, P = gold["q_X"], square(gold["q_P"], 300)
    Y, kl, it = R.tsne(P, gold["q_init"][0], max_iter=500)
    kls, tr = gold["q_kl"], gold["q_trust"]
    trust = R.trustworthiness(X, Y)
    print(f"restatement: KL {kl:.4f} (sklearn {kls.min():.4f} .. {kls.max():.4f}), trustworthiness {trust:.4f} "
          f"(sklearn {tr.min():.4f} .. {tr.max():.4f}), last iteration {it}")
    assert it == 499 and abs(R.kl_divergence(Y, P)[0] - kl) < 0.05          # the error is read before the last update
    assert R.kl_divergence(Y, P)[0] <= kls.max() + (kls.max() - kls.min())
    assert trust >= tr.min() - (tr.max() - tr.min())


def test_update_restatement():
    rng = np.random.default_rng(0)
    Y, u, g, gr = (rng.standard_normal((50, 2)).astype(np.float32) for _ in range(4))
    g = np.abs(g) + np.float32(0.01)
    u[:5], gr[5:10] = 0, 0
    Y2, u2, g2, q = R.update_f32(Y, u, g, gr, 0.5, 200.0)
    inc = u.astype(np.float64) * gr < 0
    assert np.allclose(g2, np.maximum(np.where(inc, g + 0.2, g * 0.8), 0.01), rtol=1e-6)
    assert np.allclose(u2, 0.5 * u - 200.0 * gr * g2, rtol=1e-5, atol=1e-5) and np.allclose(Y2, Y + u2, atol=1e-5)
    assert all(a.dtype == np.float32 for a in (Y2, u2, g2)) and abs(q - ((gr * g2).astype(np.float64) ** 2).sum()) <= 1e-6 * q


# ---------------------------------------------------------------------------------------------------------------
# the stop rules of the driver on a stub objective
# ---------------------------------------------------------------------------------------------------------------
def run_stub(errors, norms, it, max_iter, patience, min_grad_norm=1e-7):
    from eyegaze_multimodal_amd.embedding import descend
    calls = []

    def step(i, check):
        calls.append((i, check))
        return (errors(i), norms(i)) if check else None
    return descend(step, it, max_iter, patience, min_grad_norm), calls


def test_descent_reads_every_50th_iteration_and_the_last():
    (err, it), calls = run_stub(lambda i: 1000.0 - i, lambda i: 1.0, 0, 120, 300)
    assert it == 119 and err == 1000.0 - 119 and len(calls) == 120
    assert [i for i, check in calls if check] == [49, 99, 119]


def test_descent_stops_without_progress():
    # the error improves until iteration 99 and never again: with patience 100 the check at 249 (249 - 99 > 100) ends the run
    (err, it), calls = run_stub(lambda i: 5.0 - 0.01 * i if i <= 99 else 7.0, lambda i: 1.0, 0, 1000, 100)
    assert it == 249 and err == 7.0 and len(calls) == 250
    # the first check is the best one (49); 199 - 49 = 150 is not MORE than 150, 249 - 49 is
    (err, it), _ = run_stub(lambda i: 5.0 + i, lambda i: 1.0, 0, 1000, 150)
    assert it == 249
    # a phase that starts at 250 counts from its own first check
    (err, it), _ = run_stub(lambda i: float(i), lambda i: 1.0, 250, 1000, 300)
    assert it == 649                                                         # best at 299; 649 - 299 = 350 > 300


def test_descent_stops_at_a_small_gradient_norm_and_matches_the_restatement():
    (err, it), _ = run_stub(lambda i: 1000.0 - i, lambda i: 1e-7 if i >= 140 else 1.0, 0, 1000, 300)
    assert it == 149 and err == 1000.0 - 149
    for errors, norms, start, last, patience in [(lambda i: (i * 7919) % 13, lambda i: 1.0, 0, 400, 60),
                                                 (lambda i: 3.0, lambda i: 1.0, 250, 700, 100)]:
        step = lambda i, check: (errors(i), norms(i))
        assert run_stub(errors, norms, start, last, patience)[0] == R.descend(step, start, last, patience, 1e-7)
    (err, it), calls = run_stub(lambda i: 1.0, lambda i: 1.0, 5, 5, 10)      # an empty range runs nothing
    assert it == 5 and not calls


def test_tsne_refuses_other_than_two_components():
    from eyegaze_multimodal_amd import embedding as E
    with pytest.raises(ValueError, match="two components"):
        E.tsne(np.zeros((10, 4), np.float32), n_components=3)


def test_embedding_maps_refuses_more_windows_than_the_exact_method_serves():
    """nothing is subsampled silently: the refusal names max_samples, before the model is touched"""
    import torch
    from eyegaze_multimodal_amd import predict as PR
    x = torch.empty(16385, 0, 0)
    with pytest.raises(ValueError, match="set max_samples"):
        PR.embedding_maps(None, x, x, torch.zeros(16385))
    with pytest.raises(ValueError, match="max_samples >= 2"):
        PR.embedding_maps(None, x, x, torch.zeros(16385), max_samples=1)


# ---------------------------------------------------------------------------------------------------------------
# the C ABI: declarations, binding, host-side refusals (no launch, so no GPU)
# ---------------------------------------------------------------------------------------------------------------
ENTRIES = {"eg_tsne_workspace_bytes": 1, "eg_tsne_sqdist": 5, "eg_tsne_affinities": 7, "eg_tsne_joint": 6, "eg_tsne_gradient": 9,
           "eg_tsne_update": 10}


def test_header_binding_and_build_list_agree():
    from eyegaze_multimodal_amd import _lib as L
    from eyegaze_multimodal_amd import build
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "eyegaze_hip.h").read_text(), flags=re.S)
    assert "tsne.hip" in build.SOURCES and L.ABI_VERSION == 5 and "#define EG_ABI_VERSION 5" in text
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b(?:int|int64_t)\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m and len(m.group(1).split(",")) == len(L.SIGNATURES[name]) == nargs, name
    assert f"#define EG_TSNE_MAX_N {L.TSNE_MAX_N}" in text and f"#define EG_TSNE_MAX_D {L.TSNE_MAX_D}" in text


def test_workspace_size():
    from eyegaze_multimodal_amd import _lib as L
    assert L.tsne_workspace_bytes(1) == -1 and L.tsne_workspace_bytes(16385) == -1
    for N in (2, 15, 16, 17, 300, 16384):
        assert L.tsne_workspace_bytes(N) == 8 * max(N + 1, 2 * -(-N // 16))


def test_host_side_refusals():
    """every refusal happens before any launch; the pointers below are never dereferenced"""
    from eyegaze_multimodal_amd import _lib as L
    p, N = 0x1000, 100
    ws = L.tsne_workspace_bytes(N)
    bad = [("null pointer", "eg_tsne_sqdist", (0, N, 8, p, 0)), ("null pointer", "eg_tsne_sqdist", (p, N, 8, 0, 0)),
           (r"N=1 outside \[2, 16384\]", "eg_tsne_sqdist", (p, 1, 8, p, 0)),
           (r"N=16385 outside", "eg_tsne_sqdist", (p, 16385, 8, p, 0)),
           (r"D=0 outside \[1, 4096\]", "eg_tsne_sqdist", (p, N, 0, p, 0)), ("D=4097 outside", "eg_tsne_sqdist", (p, N, 4097, p, 0)),
           ("null pointer", "eg_tsne_affinities", (p, N, 30.0, p, 0, p, 0)), ("null pointer", "eg_tsne_affinities", (p, N, 30.0, p, p, 0, 0)),
           ("N=1 outside", "eg_tsne_affinities", (p, 1, 0.5, p + 64, p, p, 0)),
           (r"perplexity=0 outside \(0, N=100\)", "eg_tsne_affinities", (p, N, 0.0, p + 64, p, p, 0)),
           ("perplexity=-3 outside", "eg_tsne_affinities", (p, N, -3.0, p + 64, p, p, 0)),
           ("perplexity=100 outside", "eg_tsne_affinities", (p, N, 100.0, p + 64, p, p, 0)),
           ("may not be written over dist", "eg_tsne_affinities", (p, N, 30.0, p, p, p, 0)),
           ("null pointer", "eg_tsne_joint", (p, N, 0, ws, p + 64, 0)), ("N=1 outside", "eg_tsne_joint", (p, 1, p, ws, p + 64, 0)),
           (f"needs {ws} workspace bytes, the workspace holds {ws - 1}", "eg_tsne_joint", (p, N, p, ws - 1, p + 64, 0)),
           ("may not be written over cond", "eg_tsne_joint", (p, N, p, ws, p, 0)),
           ("null pointer", "eg_tsne_gradient", (p, 0, 1.0, N, p, ws, p, 0, 0)), ("null pointer", "eg_tsne_gradient", (p, p, 1.0, N, p, ws, 0, 0, 0)),
           ("N=16385 outside", "eg_tsne_gradient", (p, p, 1.0, 16385, p, 1 << 30, p, 0, 0)),
           (f"needs {ws} workspace bytes", "eg_tsne_gradient", (p, p, 1.0, N, p, 0, p, 0, 0)),
           ("exaggeration=0 must be > 0", "eg_tsne_gradient", (p, p, 0.0, N, p, ws, p, 0, 0)),
           ("8-byte boundary", "eg_tsne_gradient", (p + 4, p, 1.0, N, p, ws, p, 0, 0)),
           ("null pointer", "eg_tsne_update", (p, p, 0, p, N, 0.5, 200.0, 0.01, 0, 0)), ("N=1 outside", "eg_tsne_update", (p, p, p, p, 1, 0.5, 200.0, 0.01, 0, 0)),
           ("learning_rate=0", "eg_tsne_update", (p, p, p, p, N, 0.5, 0.0, 0.01, 0, 0))]
    for match, name, args in bad:
        with pytest.raises(L.EgError, match=match):
            L.call(name, *args)


# ---------------------------------------------------------------------------------------------------------------
# the CSV of run_embedding_analysis
# ---------------------------------------------------------------------------------------------------------------
def test_csv_columns(tmp_path):
    from eyegaze_multimodal_amd import embedding as E
    coords = np.array([[1.5, -2.25], [0.1, 3.0], [7.0, 8.0]], np.float32)
    E.write_tsne_csv(tmp_path / "tsne_z_fuse.csv", coords, [0, 2, 1], [1, 2, 5], ["Single", "Competition", "Cooperation"])
    rows = list(csv.reader(open(tmp_path / "tsne_z_fuse.csv", newline="")))
    assert rows[0] == ["Sample_ID", "True_Label", "Pred_Label", "TSNE_1", "TSNE_2"] and len(rows) == 4
    assert rows[1][:3] == ["0", "Single", "Competition"] and rows[3][:3] == ["2", "Competition", "5"]
    got = np.array([[float(r[3]), float(r[4])] for r in rows[1:]], np.float32)
    assert got.tobytes() == coords.tobytes()                                  # the float32 coordinates survive the text


# ---------------------------------------------------------------------------------------------------------------
# against live scikit-learn, where it is installed
# ---------------------------------------------------------------------------------------------------------------
def test_restatement_against_live_sklearn(gold):
    pytest.importorskip("sklearn")
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne as T
    from sklearn.manifold import trustworthiness
    N, _, perp = CASES[0]
    X, dist = gold["s0_X"], square(gold["s0_dist"], N)
    P = T._joint_probabilities(dist.astype(np.float32), perp, 0)
    mine = R.joint_probabilities(dist, perp)
    assert np.abs(mine - squareform(P)).max() / P.max() <= 1e-12
    Y = gold["s0_pos1"].astype(np.float64)
    for ex in (12.0, 1.0):
        kl, grad = T._kl_divergence(Y.ravel(), P * ex, 1, N, 2)
        kl_r, grad_r = R.kl_divergence(Y, squareform(P), ex)
        assert abs(kl - kl_r) <= 1e-12 * abs(kl) and np.abs(grad_r.ravel() - grad).max() <= 1e-12 * np.abs(grad).max()
    # ten iterations of sklearn's own descent and of the restatement from the same start: still the same map (4e-5), as later not
    y0 = gold["s0_pos0"].astype(np.float64)
    lr = max(N / 12.0 / 4.0, 50.0)
    sk, _, _ = T._gradient_descent(T._kl_divergence, y0.ravel().copy(), it=0, max_iter=10, n_iter_check=50, momentum=0.5,
                                   learning_rate=lr, args=[P * 12.0, 1, N, 2], kwargs={})
    mine, _, it = R.tsne(squareform(P), y0, max_iter=10)
    assert it == 9 and np.abs(mine.ravel() - sk).max() <= 1e-4 * np.abs(sk).max()
    assert abs(trustworthiness(X, gold["s0_pos1"], n_neighbors=10) - R.trustworthiness(X, gold["s0_pos1"])) <= 1e-12
