"""GPU tests of the exact t-SNE stages: every eg_tsne_* entry point alone with sentinels behind every output and
workspace and its inputs checked byte for byte, against sklearn's recorded results (tests/golden/tsne.npz) and the numpy
restatement (tests/tsne_ref.py); the driver against manual calls; the maps it reaches against sklearn's by what t-SNE optimises.

Yardsticks.  Distances: |d - d64| <= 2^-22 d64 (one float32 rounding, 4x margin).  Affinities: steps < 100; with the device's beta
the entropy recomputed in fp64 within 1e-5 + 1e-9 of ln perplexity; cond within 2^-22 relative of exp(-d beta) / S in fp64 -- plus
2^-149, the spacing of float32 below 2^-126, where no float32 holds a relative bound.  Joint P, gradient and KL: at most twice the
distance of the restatement from sklearn's fp64 result, recorded by tests/make_golden_tsne.py with the restatement's outputs in
the formats the entry points are declared with (float32 cond, P and gradient; fp64 in between) -- kept in fp64 throughout, the
restatement's search is sklearn's to 3e-16, a figure no float32 output can be held to.  Update: 4 * 2^-24 * (|momentum update| +
|lr gains grad|) per element, gains exact.  Quality: the KL of the returned map, recomputed in fp64 from sklearn's P, at most
KL_max + (KL_max - KL_min) of sklearn's eight runs; trustworthiness at least T_min - (T_max - T_min).  The coordinates themselves
are compared nowhere: two correct descents differ by the scale of the map after 50 iterations."""
import csv
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd import embedding as E  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from tests import tsne_ref as R  # noqa: E402

DEV = "cuda"
GUARD = 64
CASES = [(97, 24, 10.0), (257, 40, 30.0), (65, 768, 20.0)]
GOLD = np.load(Path(__file__).resolve().parent / "golden" / "tsne.npz")
SENTINELS = {torch.float32: 12345.0, torch.float64: 12345.0, torch.int32: -77, torch.uint8: 0xA5}


def stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """an output or workspace of n elements with GUARD sentinel elements behind it"""

    def __init__(self, n, dtype=torch.float32):
        self.n, self.sent = n, SENTINELS[dtype]
        self.buf = torch.full((n + GUARD,), self.sent, dtype=dtype, device=DEV)

    @property
    def t(self):
        return self.buf[:self.n]

    def ok(self):
        return bool((self.buf[self.n:] == self.sent).all())


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def unchanged(t, host):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(host).tobytes()


def square(condensed, N, dtype=np.float64):
    out = np.zeros((N, N), dtype)
    out[np.triu_indices(N, 1)] = condensed
    return out + out.T


# ---------------------------------------------------------------------------------------------------------------
# eg_tsne_sqdist
# ---------------------------------------------------------------------------------------------------------------
def sqdist_inputs():
    rng = np.random.default_rng(5)
    extra = [(33, 1), (2, 4096), (130, 33), (64, 32), (31, 7)]        # one dimension, the widest rows, sizes off and on the 32-tile
    return [GOLD[f"s{c}_X"] for c in range(3)] + [rng.standard_normal(s).astype(np.float32) for s in extra]


@pytest.mark.parametrize("k", range(8))
def test_distances_are_the_fp64_sums_rounded_once(k):
    X = sqdist_inputs()[k]
    if k == 4:
        X[1] = X[0] + np.float32(1e-3) * X[1]                          # near neighbours: |x|^2 + |y|^2 - 2xy would cancel here
    N, D = X.shape
    x, out = dev(X), Guarded(N * N)
    call("eg_tsne_sqdist", ptr(x), N, D, ptr(out.t), stream())
    got, ref = out.t.view(N, N).cpu().numpy().astype(np.float64), R.sqdist(X)
    assert out.ok() and unchanged(x, X)
    err = np.abs(got - ref) / np.maximum(ref, 1e-300)
    print(f"N={N} D={D}: max relative error {err.max():.2e} (bound {2.0 ** -22:.2e})")
    assert (np.abs(got - ref) <= 2.0 ** -22 * ref).all()
    assert (got == got.T).all() and (np.diag(got) == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# eg_tsne_affinities and eg_tsne_joint, fed the fixture's distances
# ---------------------------------------------------------------------------------------------------------------
def run_affinities(dist32, N, perp):
    d = dev(dist32)
    cond, beta, steps = Guarded(N * N), Guarded(N, torch.float64), Guarded(N, torch.int32)
    call("eg_tsne_affinities", ptr(d), N, perp, ptr(cond.t), ptr(beta.t), ptr(steps.t), stream())
    assert cond.ok() and beta.ok() and steps.ok() and unchanged(d, dist32)
    return cond, beta.t.cpu().numpy(), steps.t.cpu().numpy()


def run_joint(cond_t, N):
    before = cond_t.cpu().numpy()
    ws, P = Guarded(L.tsne_workspace_bytes(N), torch.uint8), Guarded(N * N)
    call("eg_tsne_joint", ptr(cond_t), N, ptr(ws.t), ws.n, ptr(P.t), stream())
    assert ws.ok() and P.ok() and unchanged(cond_t, before)
    return P.t.view(N, N).cpu().numpy()


@pytest.mark.parametrize("c", range(3))
def test_affinities_and_joint_probabilities(c):
    N, _, perp = CASES[c]
    dist32 = square(GOLD[f"s{c}_dist"], N, np.float32)
    cond, beta, steps = run_affinities(dist32, N, perp)
    assert steps.max() < 100 and steps.min() >= 0
    dist, got = dist32.astype(np.float64), cond.t.view(N, N).cpu().numpy()
    worst_h = worst_c = 0.0
    for i in range(N):
        H, ref, _ = R.row_entropy(dist[i], i, beta[i])
        worst_h = max(worst_h, abs(H - np.log(perp)))
        tol = 2.0 ** -22 * ref + 2.0 ** -149
        worst_c = max(worst_c, float((np.abs(got[i] - ref) / tol).max()))
        assert got[i, i] == 0.0
    print(f"case {c}: steps <= {steps.max()}, |H - ln perplexity| <= {worst_h:.2e}, cond at {worst_c:.2f} of its tolerance")
    assert worst_h <= 1e-5 + 1e-9 and worst_c <= 1.0
    _, beta_r, steps_r = R.binary_search_perplexity(dist32, perp)
    print(f"         beta differs from the restatement's by at most {np.abs(beta / beta_r - 1).max():.2e}, "
          f"steps equal: {bool((steps == steps_r).all())}")
    # joint P against sklearn's
    P = run_joint(cond.t, N).astype(np.float64)
    P_sk = square(GOLD[f"s{c}_P"], N)
    d, bound = np.abs(P - P_sk).max() / P_sk.max(), 2.0 * float(GOLD[f"s{c}_P_restatement_distance"])
    print(f"         max|dP| / max P = {d:.2e} (bound {bound:.2e})")
    assert d <= bound
    off = ~np.eye(N, dtype=bool)
    assert (P == P.T).all() and (np.diag(P) == 0).all() and P[off].min() >= 2.0 ** -52 and abs(P.sum() - 1.0) < 1e-6


def test_joint_floor_and_two_runs():
    """far rows: the conditional probabilities underflow and P sits on its 2^-52 floor; two runs give the same bytes"""
    N = 40
    X = np.zeros((N, 3), np.float32)
    X[:, 0] = np.arange(N) * 40.0
    P1, beta, steps = E.joint_probabilities(X, 2.0)
    P2, _, _ = E.joint_probabilities(X, 2.0)
    assert torch.equal(P1, P2) and int(steps.max()) < 100
    P = P1.cpu().numpy()
    assert P[0, N - 1] == np.float32(2.0 ** -52) and (P == P.T).all() and (np.diag(P) == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# eg_tsne_gradient
# ---------------------------------------------------------------------------------------------------------------
def run_gradient(Y, P, ex, with_stats=True):
    N = Y.shape[0]
    y, p = dev(Y), dev(P)
    ws, grad, stats = Guarded(L.tsne_workspace_bytes(N), torch.uint8), Guarded(2 * N), Guarded(2, torch.float64)
    call("eg_tsne_gradient", ptr(y), ptr(p), ex, N, ptr(ws.t), ws.n, ptr(grad.t), ptr(stats.t) if with_stats else 0, stream())
    assert ws.ok() and grad.ok() and stats.ok() and unchanged(y, Y) and unchanged(p, P)
    assert float(stats.t[1]) == SENTINELS[torch.float64]                         # stats[1] is eg_tsne_update's
    return grad.t.view(N, 2).cpu().numpy(), float(stats.t[0])


@pytest.mark.parametrize("c", range(3))
def test_gradient_and_divergence_at_the_fixture_positions(c):
    N = CASES[c][0]
    P32 = square(GOLD[f"s{c}_P"].astype(np.float32), N, np.float32)
    for k in range(2):
        Y = GOLD[f"s{c}_pos{k}"]
        for ex in (12, 1):
            tag = f"s{c}_pos{k}_e{ex}"
            grad, kl = run_gradient(Y, P32, float(ex))
            ref_g, ref_kl = GOLD[tag + "_grad"], float(GOLD[tag + "_kl"])
            dg, dk = np.abs(grad - ref_g).max() / np.abs(ref_g).max(), abs(kl - ref_kl) / abs(ref_kl)
            bg, bk = 2.0 * float(GOLD[tag + "_grad_restatement_distance"]), 2.0 * float(GOLD[tag + "_kl_restatement_distance"])
            print(f"{tag}: gradient {dg:.2e} of max|grad| (bound {bg:.2e}), KL {dk:.2e} relative (bound {bk:.2e})")
            assert dg <= bg and dk <= bk
            lean, none = run_gradient(Y, P32, float(ex), with_stats=False)
            assert lean.tobytes() == grad.tobytes() and none == SENTINELS[torch.float64]      # the same bytes without the KL


def test_gradient_at_the_largest_n():
    """N = 16384: 1024 workgroups, Y fills 128 KB of LDS.  The expectation is fp64 on the device in row blocks; the bound is one
    float32 rounding of the largest entry with a 2x margin (2^-23 max|grad|), the KL's 1e-10 relative (fp64 sums in another order)"""
    N, ex = 16384, 12.0
    g = torch.Generator(device=DEV).manual_seed(3)
    Y = torch.randn(N, 2, device=DEV, generator=g) * 3.0
    P = torch.rand(N, N, device=DEV, generator=g)
    P = (P + P.T) / (2.0 * float(N) * N)
    P.fill_diagonal_(0.0)
    Yb, Pb = Y.clone(), P[:64].clone()
    ws, grad, stats = Guarded(L.tsne_workspace_bytes(N), torch.uint8), Guarded(2 * N), Guarded(2, torch.float64)
    call("eg_tsne_gradient", ptr(Y), ptr(P), ex, N, ptr(ws.t), ws.n, ptr(grad.t), ptr(stats.t), stream())
    assert ws.ok() and grad.ok() and stats.ok() and torch.equal(Y, Yb) and torch.equal(P[:64], Pb)
    Yd = Y.double()
    blocks = [(i, min(i + 1024, N)) for i in range(0, N, 1024)]

    def w_block(a, b):
        w = 1.0 / (1.0 + (Yd[a:b, None, :] - Yd[None, :, :]).square().sum(-1))
        w[torch.arange(b - a), torch.arange(a, b)] = 0.0
        return w
    Z = sum(w_block(a, b).sum() for a, b in blocks)
    ref, kl = torch.empty(N, 2, dtype=torch.float64, device=DEV), 0.0
    for a, b in blocks:
        w = w_block(a, b)
        q, p = (w / Z).clamp_min(2.0 ** -52), ex * P[a:b].double()
        m = (p - q) * w
        ref[a:b] = 4.0 * (m.sum(1, keepdim=True) * Yd[a:b] - m @ Yd)
        t = p * torch.log(p.clamp_min(2.0 ** -52) / q)
        t[torch.arange(b - a), torch.arange(a, b)] = 0.0
        kl += float(t.sum())
    d = float((grad.t.view(N, 2).double() - ref).abs().max() / ref.abs().max())
    print(f"N={N}: gradient {d:.2e} of max|grad| (bound {2.0 ** -23:.2e}), KL {float(stats.t[0]):.6f} against {kl:.6f}")
    assert d <= 2.0 ** -23 and abs(float(stats.t[0]) - kl) <= 1e-10 * abs(kl)


# ---------------------------------------------------------------------------------------------------------------
# eg_tsne_update
# ---------------------------------------------------------------------------------------------------------------
def test_update_is_the_float32_body():
    N, momentum, lr = 1000, 0.8, 123.5
    rng = np.random.default_rng(11)
    Y, u, gr = (rng.standard_normal((N, 2)).astype(np.float32) for _ in range(3))
    gains = rng.uniform(0.005, 3.0, (N, 2)).astype(np.float32)
    gains[:20] = np.float32(0.01)                                               # on the clamp: * 0.8 falls below it
    u[20:60], gr[40:80] = 0.0, 0.0                                              # zeros on either side and on both
    u[80:90] *= np.float32(1e-30)                                               # a product that underflows to +-0: not < 0
    gr[80:90] *= np.float32(1e-30)
    y, ud, gd, grd = Guarded(2 * N), Guarded(2 * N), Guarded(2 * N), dev(gr)
    for t, a in ((y, Y), (ud, u), (gd, gains)):
        t.t.copy_(dev(a).view(-1))
    stats = Guarded(2, torch.float64)
    call("eg_tsne_update", ptr(y.t), ptr(ud.t), ptr(gd.t), ptr(grd), N, momentum, lr, 0.01, ptr(stats.t), stream())
    assert y.ok() and ud.ok() and gd.ok() and stats.ok() and unchanged(grd, gr)
    Yr, ur, gr_, q = R.update_f32(Y, u, gains, gr, momentum, lr)
    got_y, got_u, got_g = (t.t.view(N, 2).cpu().numpy() for t in (y, ud, gd))
    assert got_g.tobytes() == gr_.tobytes()                                      # gains exact
    tol = 4 * 2.0 ** -24 * (np.abs(np.float32(momentum) * u) + np.abs(np.float32(lr) * gr_ * gr)).astype(np.float64)
    du, dy = np.abs(got_u.astype(np.float64) - ur), np.abs(got_y.astype(np.float64) - Yr)
    print(f"update: {int((du > 0).sum())} elements differ from the restatement, Y: {int((dy > 0).sum())}")
    assert (du <= tol).all() and (dy <= tol + 2.0 ** -23 * np.abs(Yr)).all()    # Y: one more rounded sum
    assert float(stats.t[0]) == SENTINELS[torch.float64] and abs(float(stats.t[1]) - q) <= 1e-12 * q
    # without stats: the same bytes
    y2, u2, g2 = dev(Y), dev(u), dev(gains)
    call("eg_tsne_update", ptr(y2), ptr(u2), ptr(g2), ptr(grd), N, momentum, lr, 0.01, 0, stream())
    assert unchanged(y2, got_y) and unchanged(u2, got_u) and unchanged(g2, got_g)


# ---------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------
def manual_descent(P, Y0, phases, lr):
    """phases: [(iterations, exaggeration, momentum)]; plain gradient / update calls without stats"""
    N = Y0.shape[0]
    Y, grad = dev(Y0), torch.empty(N, 2, device=DEV)
    ws = torch.empty(L.tsne_workspace_bytes(N), dtype=torch.uint8, device=DEV)
    for n, ex, momentum in phases:
        u, g = torch.zeros_like(Y), torch.ones_like(Y)
        for _ in range(n):
            call("eg_tsne_gradient", ptr(Y), ptr(P), ex, N, ptr(ws), ws.numel(), ptr(grad), 0, stream())
            call("eg_tsne_update", ptr(Y), ptr(u), ptr(g), ptr(grad), N, momentum, lr, 0.01, 0, stream())
    return Y


def test_driver_is_the_manual_steps_and_repeats_its_bytes(monkeypatch):
    X, Y0 = GOLD["q_X"], GOLD["q_init"][0]
    P, _, _ = E.joint_probabilities(X, 30.0)
    lr = max(300 / 12.0 / 4.0, 50.0)
    Y, kl, it = E.tsne(X, max_iter=60, init=Y0, P=P)
    assert it == 59 and np.isfinite(kl) and unchanged(dev(Y0), Y0)
    assert torch.equal(Y, manual_descent(P, Y0, [(60, 12.0, 0.5)], lr))         # 60 < 250: all of it in the first phase
    monkeypatch.setattr(E, "EXPLORATION_ITER", 40)
    Ya, kla, ita = E.tsne(X, max_iter=60, init=Y0, P=P)
    Yb, klb, itb = E.tsne(X, max_iter=60, init=Y0)                               # P computed again: the same bytes
    assert ita == itb == 59 and kla == klb and torch.equal(Ya, Yb)
    assert torch.equal(Ya, manual_descent(P, Y0, [(40, 12.0, 0.5), (20, 1.0, 0.8)], lr))
    assert not torch.equal(Ya, Y)
    # the divergence the driver returns is the one of the map BEFORE the last update, on the unexaggerated P
    Yc = manual_descent(P, Y0, [(40, 12.0, 0.5), (19, 1.0, 0.8)], lr)
    assert abs(R.kl_divergence(Yc.cpu().numpy(), P.cpu().numpy())[0] - kla) <= 1e-9 * abs(kla)


def test_tsne_arguments():
    X = GOLD["s0_X"]
    with pytest.raises(ValueError, match="two components"):
        E.tsne(X, n_components=3)
    with pytest.raises(ValueError, match="init must be"):
        E.tsne(X, init="spectral")
    with pytest.raises(ValueError, match=r"\[97, 2\]"):
        E.tsne(X, init=np.zeros((96, 2), np.float32))
    with pytest.raises(ValueError, match="outside"):
        E.tsne(X[:1])
    Y, kl, it = E.tsne(X[:20], perplexity=30, max_iter=20, init="random")         # perplexity capped to N - 1
    assert Y.shape == (20, 2) and np.isfinite(kl) and it == 19
    draw = 1e-4 * np.random.RandomState(42).standard_normal((20, 2)).astype(np.float32)          # sklearn's draw for "random"
    Ya, _, _ = E.tsne(X[:20], perplexity=5, max_iter=5, init="random")
    Yb, _, _ = E.tsne(X[:20], perplexity=5, max_iter=5, init=draw)
    Yc, _, _ = E.tsne(X[:20], perplexity=5, max_iter=5, init="random", random_state=7)
    assert torch.equal(Ya, Yb) and not torch.equal(Ya, Yc)


@pytest.fixture(scope="module")
def quality_P():
    return E.joint_probabilities(GOLD["q_X"], 30.0)[0]


@pytest.mark.parametrize("seed", range(8))
def test_quality_against_sklearns_runs(seed, quality_P):
    X, P_sk = GOLD["q_X"], square(GOLD["q_P"], 300)
    kls, tr = GOLD["q_kl"], GOLD["q_trust"]
    Y, kl_dev, it = E.tsne(X, max_iter=500, init=GOLD["q_init"][seed], P=quality_P)
    Y = Y.cpu().numpy()
    kl, trust = R.kl_divergence(Y, P_sk)[0], R.trustworthiness(X, Y)
    print(f"seed {seed}: KL {kl:.4f} (sklearn {float(kls[seed]):.4f}; {kls.min():.4f} .. {kls.max():.4f}), trustworthiness "
          f"{trust:.4f} (sklearn {tr.min():.4f} .. {tr.max():.4f}), device KL at the last iteration {kl_dev:.4f}")
    assert it == 499 and np.isfinite(Y).all()
    assert kl <= kls.max() + (kls.max() - kls.min())
    assert trust >= tr.min() - (tr.max() - tr.min())


def test_pca_init():
    X, ref = GOLD["q_X"], GOLD["q_pca_init"]
    got = E.pca_init(X).cpu().numpy()
    d = np.abs(got - ref).max() / 1e-4
    print(f"pca_init: {d:.2e} of the scale from the exact fp64 init (sklearn's randomized solver: {float(GOLD['q_pca_sklearn_distance']):.2e})")
    assert got.dtype == np.float32 and d <= 1e-5 and abs(got[:, 0].std() - 1e-4) < 1e-9
    Y, kl, it = E.tsne(X, max_iter=300)                                          # the default init end to end, both phases
    assert it == 299 and np.isfinite(kl) and R.trustworthiness(X, Y.cpu().numpy()) > 0.85


# ---------------------------------------------------------------------------------------------------------------
# predict.embedding_maps
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a5_full", "cfg5_a2_spec"])
def test_embedding_maps(name, tmp_path):
    from eyegaze_multimodal_amd import predict as PR
    from tests.test_gpu_model import build
    z, kw, cfg, sd, model = build(name, "bf16")
    g = torch.Generator().manual_seed(9)
    N = 70
    x1, x2 = torch.randn(N, 8, 1024, generator=g), torch.randn(N, 8, 1024, generator=g)
    y = torch.arange(N) % 3
    out = PR.embedding_maps(model, x1, x2, y, batch_size=32, out_dir=tmp_path, max_iter=300)
    keys = ["z_fuse"] + (["ibs_token"] if cfg.use_ibs else [])
    assert set(out) == set(keys) | {"y_true", "y_pred"}
    assert not (tmp_path / "tsne_ibs_token.csv").exists() or cfg.use_ibs
    for k in keys:
        assert out[k]["coords"].shape == (N, 2) and np.isfinite(out[k]["coords"]).all()
        assert np.isfinite(out[k]["kl_divergence"]) and out[k]["kl_divergence"] > 0 and out[k]["n_iter"] <= 299
        rows = list(csv.reader(open(tmp_path / f"tsne_{k}.csv", newline="")))
        assert rows[0] == E.CSV_COLUMNS and len(rows) == N + 1
        assert [r[1] for r in rows[1:4]] == ["Single", "Competition", "Cooperation"]
        assert np.array([[float(r[3]), float(r[4])] for r in rows[1:]], np.float32).tobytes() == out[k]["coords"].tobytes()
    with pytest.raises(ValueError, match="max_samples"):
        PR.embedding_maps(model, x1[:1], x2[:1], y[:1])
    few = PR.embedding_maps(model, x1, x2, y, batch_size=32, max_samples=40, max_iter=20)
    assert few["z_fuse"]["coords"].shape == (40, 2) and len(few["y_true"]) == 40

