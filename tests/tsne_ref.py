"""Numpy restatement of sklearn's exact t-SNE (sklearn/manifold/_t_sne.py and _utils.pyx, 1.7.2), stage by stage, in fp64 unless
said otherwise: the yardstick of tests/test_tsne_host.py and tests/test_gpu_tsne.py.  No sklearn import: tests/make_golden_tsne.py
records how far each stage lies from sklearn itself (tests/golden/tsne.npz)."""
import numpy as np

TINY = float(np.finfo(np.float64).eps)          # 2^-52, sklearn's MACHINE_EPSILON
EXPLORATION_ITER = 250                          # TSNE._EXPLORATION_MAX_ITER
N_ITER_CHECK = 50                               # TSNE._N_ITER_CHECK
PERPLEXITY_TOLERANCE = 1e-5


def sqdist(X):
    """[N, N] fp64 squared distances of the rows from the differences themselves"""
    X = np.asarray(X, np.float64)
    out = np.empty((len(X), len(X)))
    for i in range(len(X)):
        out[i] = ((X[i] - X) ** 2).sum(axis=1)
    return out


def row_entropy(d, i, beta):
    """(H, p / S, S) of row i's conditional distribution at precision beta; d: the row's squared distances"""
    p = np.exp(-np.asarray(d, np.float64) * beta)
    p[i] = 0.0
    S = p.sum()
    if S == 0.0:
        S = 1e-8
    return np.log(S) + beta * (d * p).sum() / S, p / S, S


def binary_search_perplexity(dist, perplexity):
    """-> (cond [N, N] fp64, beta [N], steps [N]); steps counts how often beta moved (100: the search ran out)"""
    dist = np.asarray(dist, np.float32).astype(np.float64)
    N, target = len(dist), np.log(perplexity)
    cond, betas, steps = np.zeros((N, N)), np.empty(N), np.full(N, 100, np.int32)
    for i in range(N):
        beta, lo, hi = 1.0, -np.inf, np.inf
        for l in range(100):
            H, cond[i], _ = row_entropy(dist[i], i, beta)
            diff = H - target
            if abs(diff) <= PERPLEXITY_TOLERANCE:
                steps[i] = l
                break
            if l == 99:
                break
            if diff > 0.0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        betas[i] = beta
    return cond, betas, steps


def joint_from_cond(cond):
    cond = np.asarray(cond, np.float64)
    P = cond + cond.T
    P = np.maximum(P / max(P.sum(), TINY), TINY)
    np.fill_diagonal(P, 0.0)
    return P


def joint_probabilities(dist, perplexity, storage=np.float64):
    """square [N, N] P of sklearn's _joint_probabilities (which returns its condensed form).  storage float32: the staged
    pipeline's formats -- the conditional probabilities and P each rounded once to float32, fp64 arithmetic in between"""
    cond = binary_search_perplexity(dist, perplexity)[0]
    return joint_from_cond(cond.astype(storage)).astype(storage)


def kl_divergence(Y, P, exaggeration=1.0):
    """sklearn's _kl_divergence at one degree of freedom on the square P: (KL of e P, grad [N, 2] fp64)"""
    Y, P = np.asarray(Y, np.float64), np.asarray(P, np.float64) * exaggeration
    N = len(Y)
    off = ~np.eye(N, dtype=bool)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    w = 1.0 / (1.0 + d)
    Q = np.maximum(w / w[off].sum(), TINY)
    kl = float((P[off] * np.log(np.maximum(P[off], TINY) / Q[off])).sum())
    m = (P - Q) * w
    np.fill_diagonal(m, 0.0)
    grad = 4.0 * (m.sum(1)[:, None] * Y - m @ Y)
    return kl, grad


def update_f32(Y, update, gains, grad, momentum, learning_rate, min_gain=0.01):
    """the body of sklearn's _gradient_descent, every operation rounded to float32 -> (Y, update, gains, sum (grad gains)^2)"""
    f = np.float32
    Y, update, gains, grad = (np.array(a, f) for a in (Y, update, gains, grad))
    inc = update * grad < f(0.0)
    gains = np.where(inc, gains + f(0.2), gains * f(0.8)).astype(f)
    gains = np.maximum(gains, f(min_gain))
    g = (grad * gains).astype(f)
    update = (f(momentum) * update).astype(f) - (f(learning_rate) * g).astype(f)
    return (Y + update).astype(f), update.astype(f), gains, float((g.astype(np.float64) ** 2).sum())


def descend(step, it, max_iter, n_iter_without_progress, min_grad_norm, n_iter_check=N_ITER_CHECK):
    """The loop and the two stop rules of sklearn's _gradient_descent.  step(i, check) runs iteration i and returns
    (error, gradient norm) when check is set (every n_iter_check-th iteration and the last), anything otherwise.
    -> (error of the last checked iteration, index of the last iteration run)"""
    error = best_error = np.finfo(float).max
    best_iter = i = it
    for i in range(it, max_iter):
        converge = (i + 1) % n_iter_check == 0
        res = step(i, converge or i == max_iter - 1)
        if converge or i == max_iter - 1:
            error = res[0]
        if converge:
            if error < best_error:
                best_error, best_iter = error, i
            elif i - best_iter > n_iter_without_progress:
                break
            if res[1] <= min_grad_norm:
                break
    return error, i


def tsne(P, Y0, max_iter=1000, early_exaggeration=12.0, n_iter_without_progress=300, min_grad_norm=1e-7, exploration=EXPLORATION_ITER,
         dtype=np.float64):
    """TSNE._tsne for method="exact" from the square P and the init Y0 -> (Y, kl_divergence, n_iter).  dtype float64 follows
    sklearn fed a float64 init; float32 uses update_f32 (the device's descent).  learning_rate is "auto"."""
    N = len(Y0)
    lr = max(N / early_exaggeration / 4.0, 50.0)
    st = {"Y": np.array(Y0, dtype)}

    def phase(it, last, momentum, ex, patience):
        st["u"], st["g"] = np.zeros_like(st["Y"]), np.ones_like(st["Y"])

        def step(i, check):
            kl, grad = kl_divergence(st["Y"], P, ex)
            if dtype == np.float32:
                st["Y"], st["u"], st["g"], q = update_f32(st["Y"], st["u"], st["g"], grad.astype(np.float32), momentum, lr)
            else:
                inc = st["u"] * grad < 0.0
                st["g"] = np.maximum(np.where(inc, st["g"] + 0.2, st["g"] * 0.8), 0.01)
                grad = grad * st["g"]
                st["u"] = momentum * st["u"] - lr * grad
                st["Y"] = st["Y"] + st["u"]
                q = float((grad ** 2).sum())
            return kl, np.sqrt(q)
        return descend(step, it, last, patience, min_grad_norm)

    kl, it = phase(0, min(exploration, max_iter), 0.5, early_exaggeration, exploration)
    if it + 1 < max_iter:
        kl, it = phase(it + 1, max_iter, 0.8, 1.0, n_iter_without_progress)
    return st["Y"], kl, it


def trustworthiness(X, Y, n_neighbors=10):
    """sklearn.manifold.trustworthiness with the euclidean metric"""
    dX, dY = np.sqrt(sqdist(X)), sqdist(Y)
    np.fill_diagonal(dX, np.inf)
    np.fill_diagonal(dY, np.inf)
    n = len(dX)
    rank = np.empty((n, n), np.int64)
    rank[np.arange(n)[:, None], np.argsort(dX, axis=1)] = np.arange(1, n + 1)
    near = np.argsort(dY, axis=1, kind="stable")[:, :n_neighbors]
    r = rank[np.arange(n)[:, None], near] - n_neighbors
    return 1.0 - r[r > 0].sum() * (2.0 / (n * n_neighbors * (2.0 * n - 3.0 * n_neighbors - 1.0)))


def pca_init(X, n_components=2):
    """exact PCA init of TSNE(init="pca"): the top principal axes by eigh, sklearn's svd_flip signs, std(col 0) = 1e-4, float32"""
    X = np.asarray(X, np.float64)
    Xc = X - X.mean(axis=0)
    w, V = np.linalg.eigh(Xc.T @ Xc)
    V = V[:, ::-1][:, :n_components]
    V = V * np.sign(V[np.abs(V).argmax(axis=0), np.arange(n_components)])
    emb = (Xc @ V).astype(np.float32)
    return emb / np.std(emb[:, 0]) * np.float32(1e-4)
