"""K21 restated with numpy and scipy, column by column: what engine.rank_sums must return, to the integer."""
import numpy as np
from scipy.stats import rankdata


def rank_sums(Y, codes, n_groups, cols=None):
    """(count int64, rank_sums float64 n_groups x n_sel, ties int64 n_sel) of the dense array Y (anything with .toarray() is made
    dense first).  Ranks are scipy.stats.rankdata(method="average") over the used rows; ties come from np.unique's counts."""
    Y = np.asarray(Y.toarray() if hasattr(Y, "toarray") else Y)
    codes = np.asarray(codes)
    cols = np.arange(Y.shape[1]) if cols is None else np.asarray(cols)
    used = codes >= 0
    g = codes[used]
    count = np.bincount(g, minlength=n_groups).astype(np.int64)
    R = np.zeros((n_groups, cols.size), dtype=np.float64)
    ties = np.zeros(cols.size, dtype=np.int64)
    for k, c in enumerate(cols):
        y = Y[used, c].astype(np.float64) + 0.0            # -0.0 + 0.0 = +0.0: np.unique then sees one zero
        if y.size == 0:
            continue
        r = rankdata(y, method="average")
        R[:, k] = np.bincount(g, weights=r, minlength=n_groups)
        t = np.unique(y, return_counts=True)[1].astype(np.int64)
        ties[k] = int((t ** 3 - t).sum())
    return count, R, ties


def z_scores(count, R, ties, tie_correct):
    """the rank-sum z of every group against the rest, written out per element (engine.rank_sum_z's rule)"""
    N = float(count.sum())
    z = np.zeros_like(R)
    for g in range(R.shape[0]):
        n = float(count[g])
        for j in range(R.shape[1]):
            c = ties[j] / (N * (N - 1)) if tie_correct else 0.0
            var = n * (N - n) / 12 * ((N + 1) - c)
            num = R[g, j] - n * (N + 1) / 2
            z[g, j] = num / np.sqrt(var) if var > 0 else 0.0
    return z
