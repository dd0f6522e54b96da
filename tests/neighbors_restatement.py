"""The cell neighbour graph restated in numpy / scipy, the plain way: float64 direct differences in row chunks, a full sort of every
row, the smoothing rule as a Python loop and the fuzzy union with scipy.  Independent of the device code.

scanpy and umap-learn are not installed here: this file is the rule the device is held to (pilot_amd/csrc/knn_kernels.hpp states the
same one), not anyone's memory of umap-learn.  ``n_neighbors`` counts the cell itself, as scanpy's does; the cell is left out of its
own neighbours by index, and the sums below run over the ``n_neighbors - 1`` others."""
import numpy as np
import scipy.sparse as sp

SMOOTH_STEPS, SMOOTH_TOL, SMOOTH_FLOOR = 64, 1e-5, 1e-3


def unit_rows(X):
    """every row of X divided by its norm: the sum of squares in float64, columns in ascending order (one rounding per product and
    per sum), the quotient in float64, rounded to X's dtype -- the values whose distances the cosine metric takes"""
    X = np.asarray(X)
    Z = X.astype(np.float64)
    ssq = np.zeros(Z.shape[0])
    for d in range(Z.shape[1]):
        ssq = ssq + Z[:, d] * Z[:, d]
    return (Z / np.sqrt(ssq)[:, None]).astype(X.dtype)


def stored(X, metric):
    """the float64 copy of the values the distances are taken between"""
    if metric not in ("euclidean", "cosine"):
        raise ValueError(metric)
    return (unit_rows(X) if metric == "cosine" else np.asarray(X)).astype(np.float64)


def distance_rows(X, metric, rows=None, chunk=256):
    """the rows ``rows`` (default: all) of the full n x n distance matrix, float64: sqrt(sum_d (x_d - y_d)^2), or for cosine half that
    sum between the unit rows; the diagonal comes out 0 and is NOT masked here"""
    Z = stored(X, metric)
    begin, end = (0, Z.shape[0]) if rows is None else rows
    out = np.empty((end - begin, Z.shape[0]))
    for r0 in range(begin, end, chunk):
        r1 = min(r0 + chunk, end)
        sq = np.zeros((r1 - r0, Z.shape[0]))
        for d in range(Z.shape[1]):
            diff = Z[r0:r1, d][:, None] - Z[None, :, d]
            sq += diff * diff
        out[r0 - begin:r1 - begin] = 0.5 * sq if metric == "cosine" else np.sqrt(sq)
    return out


def select(full, k, begin=0):
    """(indices int32 (m, k), distances (m, k)) of the rows ``begin ..`` of a distance matrix: the k smallest entries of every row
    but its own column, in (distance, index) order"""
    m, n = full.shape
    idx = np.empty((m, k), dtype=np.int32)
    dist = np.empty((m, k))
    js = np.arange(n)
    for r in range(m):
        others = js[js != begin + r]
        order = others[np.lexsort((others, full[r, others]))][:k]
        idx[r], dist[r] = order, full[r, order]
    return idx, dist


def knn(X, k, metric="euclidean", rows=None):
    """(indices, distances, full (m, n)): the k nearest other rows of the query rows in (distance, index) order"""
    full = distance_rows(X, metric, rows)
    return select(full, k, 0 if rows is None else rows[0]) + (full,)


def smooth(distances, n_neighbors):
    """(weights, sigma, rho) of the n x (n_neighbors - 1) distances"""
    D = np.asarray(distances, dtype=np.float64)
    n, k = D.shape
    assert k == n_neighbors - 1
    target = np.log2(n_neighbors)
    global_mean = D.mean()
    W, sigma, rho = np.empty((n, k)), np.empty(n), np.empty(n)
    for i in range(n):
        d = D[i]
        pos = d[d > 0.0]
        r = pos.min() if pos.size else 0.0
        g = d - r
        lo, hi, mid = 0.0, np.inf, 1.0
        for _ in range(SMOOTH_STEPS):
            psum = float(np.exp(-(np.maximum(g, 0.0) / mid)).sum())          # a term is exactly 1 where d_j <= rho
            if abs(psum - target) < SMOOTH_TOL:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if hi == np.inf else (lo + hi) / 2.0
        floor = SMOOTH_FLOOR * (d.mean() if r > 0.0 else global_mean)
        mid = max(mid, floor)
        W[i] = np.exp(-(np.maximum(g, 0.0) / mid)) if mid > 0.0 else 1.0
        sigma[i], rho[i] = mid, r
    return W, sigma, rho


def union(indices, weights):
    """A + A^T - A o A^T of the n x n matrix A with weights[i, c] at (i, indices[i, c]), as a dense float64 array"""
    n, k = indices.shape
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), k), np.asarray(indices).ravel()] = np.asarray(weights).ravel()
    return A + A.T - A * A.T


def connectivities(indices, distances, n_neighbors):
    """the symmetric CSR matrix engine.knn_connectivities returns"""
    C = sp.csr_matrix(union(indices, smooth(distances, n_neighbors)[0]))
    C.eliminate_zeros()
    return C
