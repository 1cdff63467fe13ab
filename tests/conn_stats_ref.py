"""What predict.connectivity_statistics and eg_ibs_inorm_band must compute, restated in numpy / float64.  The class sums, counts,
means and difference are 5_Metrics/eeg_metrics.py:271-311 over given matrices; tests/test_conn_stats_host.py pins them to the
reference's own functions.  The masked instance norm is InstanceNorm1d over the token axis (dual_eeg_transformer.py:897-901) of
the matrices with one band zeroed (eeg_metrics.py:332-336)."""
import numpy as np

CLASS_NAMES = ["Single", "Competition", "Cooperation"]
U = 2.0 ** -24                     # unit roundoff of fp32


def class_sums(matrices, labels, ncls):
    """(sums [ncls, ...] f64, counts [ncls] i64, abs [ncls, ...] f64 = the sums of |v|); a label outside [0, ncls) counts nowhere"""
    m, y = np.asarray(matrices, dtype=np.float64), np.asarray(labels, dtype=np.int64)
    sums, mags = np.zeros((ncls,) + m.shape[1:]), np.zeros((ncls,) + m.shape[1:])
    counts = np.zeros(ncls, np.int64)
    for c in range(ncls):
        sel = y == c
        counts[c] = sel.sum()
        sums[c], mags[c] = m[sel].sum(0), np.abs(m[sel]).sum(0)
    return sums, counts, mags


def summation_bound(n, mags):
    """|fl(sum) - sum| <= gamma_{n-1} sum|v_i| for ANY order of adding n fp32 terms (Higham, Accuracy and Stability, eq. 4.4):
    gamma_k = k u / (1 - k u)"""
    k = np.maximum(np.asarray(n, dtype=np.float64) - 1, 0)
    return (k * U / (1 - k * U)) * mags


def conn_stats_ref(matrices, labels, class_names=None):
    """class_mean / class_count / difference / count under predict.connectivity_statistics' keys, float64"""
    names = CLASS_NAMES if class_names is None else list(class_names)
    sums, counts, _ = class_sums(matrices, labels, len(names))
    mean = sums / np.maximum(counts, 1).reshape((-1,) + (1,) * (sums.ndim - 1))
    out = {"class_mean": {n: mean[c] for c, n in enumerate(names)}, "class_count": {n: int(counts[c]) for c, n in enumerate(names)},
           "count": len(np.asarray(labels))}
    if "Cooperation" in names and "Competition" in names:
        out["difference"] = mean[names.index("Cooperation")] - mean[names.index("Competition")]
    return out


def masked_inorm_ref(conn, fidx, gamma, beta, zero_band):
    """conn [B, nbands, 7, E] -> token rows [B, nbands * nfeat, E] f64: band zero_band zeroed (-1: none), then instance norm over
    the token axis (biased variance, eps 1e-5) and the affine; gamma None: the selected rows as they are"""
    x = np.asarray(conn, dtype=np.float64)[:, :, list(fidx)].copy()
    if zero_band >= 0:
        x[:, zero_band] = 0
    x = x.reshape(x.shape[0], -1, x.shape[-1])
    if gamma is None:
        return x
    xh = (x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + 1e-5)
    return xh * np.asarray(gamma, dtype=np.float64) + np.asarray(beta, dtype=np.float64)
