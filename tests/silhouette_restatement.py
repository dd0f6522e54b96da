"""The silhouette of labelled points restated the plain way: from a full float64 distance matrix (tests/neighbors_restatement.py's
``distance_rows``: direct differences of exactly the uploaded values), a, b and s by the definition, in loops over the clusters and
the points.  Independent of the device code; tests/test_silhouette_args.py pins it to ``sklearn.metrics.silhouette_samples`` with
``metric="precomputed"`` (not with ``metric="euclidean"``: that side expands |x|^2 + |y|^2 - 2 x.y and is the less accurate one).

a_i: the mean distance from i to the OTHER members of its cluster (i is left out by index, so a copy of it counts at distance 0);
b_i: the smallest, over the other clusters, of the mean distance from i to the cluster's members; s_i = (b_i - a_i) / max(a_i, b_i),
0 when i's cluster has one member and 0 when max(a_i, b_i) = 0.  Valid for 2 <= k <= n - 1 clusters."""
import numpy as np

import neighbors_restatement as NR


def codes_of(labels):
    """(codes, k): the labels numbered in sorted order, as numpy's unique does"""
    uniq, codes = np.unique(np.asarray(labels), return_inverse=True)
    return codes.reshape(-1), len(uniq)


def samples(Dref, labels):
    """s (float64, one per point) from the n x n distance matrix Dref"""
    Dref = np.asarray(Dref, dtype=np.float64)
    n = Dref.shape[0]
    codes, k = codes_of(labels)
    if Dref.shape != (n, n) or codes.shape != (n,):
        raise ValueError("an n x n matrix and n labels")
    if not 2 <= k <= n - 1:
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % k)
    members = [np.flatnonzero(codes == c) for c in range(k)]
    sums = np.empty((n, k))
    for c in range(k):                                           # the sum of every point's distances to cluster c
        sums[:, c] = Dref[:, members[c]].sum(axis=1)
    s = np.zeros(n)
    for i in range(n):
        own = codes[i]
        size = members[own].size
        if size == 1:
            continue
        a = Dref[i, members[own][members[own] != i]].sum() / (size - 1)
        b = min(sums[i, c] / members[c].size for c in range(k) if c != own)
        top = max(a, b)
        s[i] = (b - a) / top if top > 0 else 0.0
    return s


def of_points(X, labels, metric="euclidean"):
    """(s, the distance matrix used) of the rows of X as they are stored"""
    Dref = NR.distance_rows(X, metric)
    return samples(Dref, labels), Dref


def bound(D, n, dtype):
    """absolute, on every s_i and on their mean.  Every distance of the device carries a relative error <= (D + 6) u (K16's contract,
    u = 2^-24 / 2^-53), a float64 mean of at most n non-negative terms adds <= n 2^-53; with eps their sum, s = 1 - a / b or
    b / a - 1 moves by at most 2 eps, and with K16's factor 2 of slack the bound is 4 eps."""
    u = 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53
    return 4 * ((D + 6) * u + n * 2.0 ** -53)
