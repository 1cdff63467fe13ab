"""Test infrastructure: the attention statistics of the reference's analysis (5_Metrics/eeg_metrics.py:465-594) restated in
numpy / float64 over given probabilities.  tests/test_attn_stats_host.py pins this restatement to the reference's own function."""
import numpy as np

CLASS_NAMES = ["Single", "Competition", "Cooperation"]


def attn_stats_ref(p1, p2, labels, batch_size, max_samples=200, class_names=None):
    """p1, p2: [n, H, S, S] probabilities of the two directions (or streams); labels [n].  Batches of batch_size are taken while
    the count is below max_samples (None: all).  Returns mean_map [S, S], diagonals [count, S], count and
    diagonal_stats {name: {mean_diagonal_vector, mean_diagonal_value, count}}, all float64."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    N = p1.shape[0]
    n = N if max_samples is None else min(N, -(-max_samples // batch_size) * batch_size)
    per_sample = 0.5 * (p1[:n].mean(axis=1) + p2[:n].mean(axis=1))          # [n, S, S]
    diagonals = np.stack([np.diagonal(m) for m in per_sample])
    y = np.asarray(labels)[:n].astype(np.int64)
    names = CLASS_NAMES if class_names is None else list(class_names)
    stats = {}
    for c in dict.fromkeys(y.tolist()):
        v = diagonals[y == c].mean(axis=0)
        stats[names[c] if 0 <= c < len(names) else str(c)] = {"mean_diagonal_vector": v, "mean_diagonal_value": v.mean(),
                                                             "count": int((y == c).sum())}
    return {"mean_map": per_sample.sum(axis=0) / n, "diagonals": diagonals, "count": n, "diagonal_stats": stats}
