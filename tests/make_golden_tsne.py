"""Writes tests/golden/tsne.npz: inputs, sklearn's own stage results and how far the numpy restatement (tests/tsne_ref.py) lies
from them -- the yardsticks of tests/test_tsne_host.py and tests/test_gpu_tsne.py.  Needs scikit-learn (written
with 1.7.2); the tests do not.

    python -m tests.make_golden_tsne

Stage cases (N, D, perplexity): per case the float32 input, sklearn's squared distances as float32 (condensed, symmetrised from
the upper triangle), sklearn's _joint_probabilities of them (condensed, fp64), and _kl_divergence (value and gradient, fp64) at
two float32 positions -- a 1e-4-scale draw, and sklearn's own _gradient_descent after 100 iterations of the first phase -- each at
exaggeration 12 and 1, evaluated with sklearn's fp64 P.  Next to each, the restatement's distance from sklearn's fp64 result IN
THE FORMATS OF THE STAGED ENTRY POINTS (float32 conditional probabilities, float32 P, float32 gradient, fp64 in between): of its
P (max|dP| / max P), and of its gradient (relative to max|grad|) and KL (relative) when fed the float32 P.  Kept in fp64
throughout, the restatement's search takes sklearn's steps exactly and its P lies 3e-16 from sklearn's (P_fp64_distance):
no float32 output can be held to that, so the yardstick is what the formats themselves cost.
Quality case: eight 1e-4-scale inits, sklearn's P (float32), and per init the KL -- recomputed by _kl_divergence in fp64 from
sklearn's fp64 P -- and the trustworthiness at 10 neighbours of TSNE(method="exact", max_iter=500, init=that array)."""
from pathlib import Path

import numpy as np

from tests import tsne_ref as R

OUT = Path(__file__).resolve().parent / "golden" / "tsne.npz"
STAGE_CASES = [(97, 24, 10.0), (257, 40, 30.0), (65, 768, 20.0)]
QUALITY_CASE = (300, 64, 30.0)
QUALITY_ITER = 500
EXAGGERATIONS = (12.0, 1.0)


def clusters(rng, N, D):
    """three Gaussian clusters: centres of scale 3, unit noise"""
    centres = 3.0 * rng.standard_normal((3, D))
    return (centres[rng.integers(0, 3, N)] + rng.standard_normal((N, D))).astype(np.float32)


def main():
    from scipy.spatial.distance import squareform
    from sklearn.decomposition import PCA
    from sklearn.manifold import TSNE, trustworthiness
    from sklearn.manifold import _t_sne as T
    from sklearn.metrics import pairwise_distances
    rng = np.random.default_rng(20261021)
    out = {}
    for c, (N, D, perp) in enumerate(STAGE_CASES):
        X = clusters(rng, N, D)
        dist = squareform(squareform(pairwise_distances(X, metric="euclidean", squared=True).astype(np.float32), checks=False))
        P = T._joint_probabilities(dist, perp, 0)                                         # condensed, fp64
        mine = R.joint_probabilities(dist, perp, np.float32).astype(np.float64)
        out[f"s{c}_P_fp64_distance"] = np.abs(R.joint_probabilities(dist, perp) - squareform(P)).max() / P.max()
        out[f"s{c}_X"], out[f"s{c}_dist"], out[f"s{c}_P"] = X, squareform(dist).astype(np.float32), P
        out[f"s{c}_P_restatement_distance"] = np.abs(mine - squareform(P)).max() / P.max()
        out[f"s{c}_dist_restatement_distance"] = (np.abs(R.sqdist(X) - dist) / np.maximum(R.sqdist(X), 1e-30))[~np.eye(N, dtype=bool)].max()
        P32 = squareform(P.astype(np.float32)).astype(np.float64)
        lr = max(N / 12.0 / 4.0, 50.0)
        y0 = (1e-4 * np.random.RandomState(c).standard_normal((N, 2))).astype(np.float32)
        y100, _, _ = T._gradient_descent(T._kl_divergence, y0.astype(np.float64).ravel(), it=0, max_iter=100, n_iter_check=50,
                                         momentum=0.5, learning_rate=lr, args=[P * 12.0, 1, N, 2], kwargs={})
        for k, pos in enumerate((y0, y100.reshape(N, 2).astype(np.float32))):
            out[f"s{c}_pos{k}"] = pos
            for ex in EXAGGERATIONS:
                kl, grad = T._kl_divergence(pos.astype(np.float64).ravel(), P * ex, 1, N, 2)
                kl_r, grad_r = R.kl_divergence(pos, P32, ex)
                tag = f"s{c}_pos{k}_e{int(ex)}"
                out[tag + "_kl"], out[tag + "_grad"] = kl, grad.reshape(N, 2)
                out[tag + "_kl_restatement_distance"] = abs(kl_r - kl) / abs(kl)
                out[tag + "_grad_restatement_distance"] = np.abs(grad_r.astype(np.float32) - grad.reshape(N, 2)).max() / np.abs(grad).max()
                print(tag, f"kl {kl:.6f} (restatement {out[tag + '_kl_restatement_distance']:.2e}) "
                           f"grad {out[tag + '_grad_restatement_distance']:.2e} of max|grad| {np.abs(grad).max():.3e}")
        print(f"case {c}: P {out[f's{c}_P_restatement_distance']:.2e} (all fp64: {out[f's{c}_P_fp64_distance']:.2e}), distances {out[f's{c}_dist_restatement_distance']:.2e}")

    N, D, perp = QUALITY_CASE
    X = clusters(rng, N, D)
    P = T._joint_probabilities(pairwise_distances(X, metric="euclidean", squared=True), perp, 0)
    out["q_X"], out["q_P"] = X, P.astype(np.float32)
    inits, kls, trusts = [], [], []
    for seed in range(8):
        y0 = (1e-4 * np.random.RandomState(seed).standard_normal((N, 2))).astype(np.float32)
        emb = TSNE(n_components=2, perplexity=perp, max_iter=QUALITY_ITER, method="exact", init=y0.copy()).fit_transform(X)
        kl, _ = T._kl_divergence(emb.astype(np.float64).ravel(), P, 1, N, 2)
        inits.append(y0), kls.append(kl), trusts.append(trustworthiness(X, emb, n_neighbors=10))
        print(f"quality seed {seed}: KL {kl:.4f} trustworthiness {trusts[-1]:.4f} "
              f"(restatement's trustworthiness of the same map {R.trustworthiness(X, emb):.4f})")
    out["q_init"], out["q_kl"], out["q_trust"] = np.stack(inits), np.array(kls), np.array(trusts)
    # the exact PCA init, and how far sklearn's randomized one lies from it
    out["q_pca_init"] = R.pca_init(X)
    sk = PCA(n_components=2, svd_solver="randomized", random_state=42).fit_transform(X).astype(np.float32)
    sk = sk / np.std(sk[:, 0]) * 1e-4
    out["q_pca_sklearn_distance"] = np.abs(sk - out["q_pca_init"]).max() / 1e-4
    print(f"pca init: sklearn's randomized solver lies {out['q_pca_sklearn_distance']:.2e} of the scale from the exact one")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
