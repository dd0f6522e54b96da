"""K16 on the device: engine.knn / engine.knn_smooth / engine.knn_connectivities (knn_kernels.hpp) and tl.neighbors against
tests/neighbors_restatement.py, which forms the full distance matrix in float64 by direct differences and sorts every row.

The accuracy contract.  u = 2^-24 (float32) or 2^-53 (float64).  A term (x_d - y_d)^2 carries a relative error
<= 3u, a sum of D non-negative terms in a fixed order adds <= (D - 1)u, the square root (or the halving) <= u; with a factor 2 of
slack TOL = (D + 6) u, relative, on every returned distance.  The reference is the float64 direct-difference distance between
exactly the uploaded values (for cosine: the rows normalised in float64 and rounded to the element type, as the kernel forms them).
For every row i, with Dref the full reference row and kth its k-th smallest entry over j != i:
 (a) the k indices are distinct, in range and none equals i;
 (b) |dist[i, c] - Dref[i, idx[i, c]]| <= TOL Dref[i, idx[i, c]] (an exact 0 for duplicates);
 (c) dist[i, :] does not decrease, and where two returned distances are equal their indices ascend;
 (d) no returned j has Dref[i, j] > kth (1 + 2 TOL), and every j != i with Dref[i, j] < kth (1 - 2 TOL) is returned.
Nothing is skipped or exempted.  Where the distances are exact in the element type (integer lattices) the indices must equal the
reference's (distance, index) order.  Conditions on the inputs are asserted on the restatement before the device is looked at.

Shapes: the smallest at which each path of the kernel is taken -- n = k + 1; D = 1; several corpus tiles and query blocks (a block
holds 256 queries, a float32 tile of 50 dims 128 corpus rows); n prime; D past the 64 dims a query keeps in registers (wide) and past
the 512 / 256 dims one staged tile holds (very_wide: the dims pass through LDS in groups)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.spatial.distance import cdist

import neighbors_restatement as NR
from pilot_amd import engine, tl

pytestmark = pytest.mark.gpu

U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
DTYPES = [np.float32, np.float64]
WEIGHT_TOL = 2e-5            # the bisection stops within 1e-5 of its target and every weight is one monotone term of that sum


def _tol(D, dtype):
    return (D + 6) * U[np.dtype(dtype)]


@functools.lru_cache(maxsize=None)
def _cloud(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "off_centre":
        X = 4096.0 + rng.normal(size=(1100, 50))
    elif name == "duplicates":
        X = np.tile(rng.normal(size=(100, 8)), (3, 1))[rng.permutation(300)]
    elif name == "lattice2":
        X = np.stack(np.meshgrid(np.arange(17.0), np.arange(17.0), indexing="ij"), axis=-1).reshape(-1, 2)
    elif name == "lattice4":
        X = np.stack(np.meshgrid(*[np.arange(5.0)] * 4, indexing="ij"), axis=-1).reshape(-1, 4)
    elif name == "scaled":
        X = _cloud("pilot") * 10.0 ** rng.uniform(-3.0, 3.0, (1100, 1))
    else:
        shape = {"tiny": (16, 3), "one_dim": (65, 1), "pilot": (1100, 50), "odd": (3001, 50), "wide": (257, 130), "very_wide": (70, 600)}[name]
        X = rng.normal(size=shape)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _uploaded(name, dtype):
    X = np.ascontiguousarray(_cloud(name).astype(dtype))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _full(name, dtype, metric="euclidean"):
    """the reference distance matrix of the uploaded values, computed once and left unchanged"""
    full = NR.distance_rows(_uploaded(name, dtype), metric)
    full.setflags(write=False)
    return full


def _arg(name, dtype, route):
    X = _uploaded(name, dtype)
    return engine.DeviceMatrix.upload(X) if route == "device" else X


def _check(idx, dist, full, D, dtype, what, begin=0, exact=False):
    """(a) - (d) of the contract for the query rows begin .. begin + m of the reference rows ``full`` (m x n)"""
    m, n = full.shape
    k = idx.shape[1]
    t = _tol(D, dtype)
    rows = np.arange(m)
    assert idx.shape == dist.shape == (m, k) and idx.dtype == np.int32 and dist.dtype == np.float64
    # (a)
    assert idx.min() >= 0 and idx.max() < n and (idx != (begin + rows)[:, None]).all()
    assert (np.diff(np.sort(idx, axis=1), axis=1) > 0).all()
    # (b)
    at = np.take_along_axis(full, idx.astype(np.int64), axis=1)
    err = np.abs(dist - at)
    worst = float((err[at > 0] / at[at > 0]).max()) if (at > 0).any() else 0.0
    print("%s: max relative distance error %.2e (TOL %.2e), %d exact zeros" % (what, worst, t, int((at == 0).sum())))
    assert (err <= t * at).all(), what
    # (c)
    step = np.diff(dist, axis=1)
    assert (step >= 0).all() and (np.diff(idx, axis=1)[step == 0] > 0).all(), what
    # (d)
    others = np.array(full)
    others[rows, begin + rows] = np.inf
    kth = np.partition(others, k - 1, axis=1)[:, k - 1][:, None]
    assert (at <= kth * (1 + 2 * t)).all(), what
    got = np.zeros((m, n), dtype=bool)
    got[rows[:, None], idx] = True
    assert not ((others < kth * (1 - 2 * t)) & ~got).any(), what
    if exact:
        assert np.array_equal(idx, NR.select(full, k, begin)[0]), what


# ---- euclidean ------------------------------------------------------------------------------------------------------------------
RNG_CASES = [("tiny", 15), ("one_dim", 1), ("one_dim", 14), ("pilot", 14), ("pilot", 64), ("odd", 14), ("wide", 14), ("very_wide", 5)]


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,k", RNG_CASES)
def test_rng_cases(name, k, dtype, route):
    full = _full(name, dtype)
    n, D = _cloud(name).shape
    assert n >= k + 1 and (name != "tiny" or n == k + 1)
    idx, dist = engine.knn(_arg(name, dtype, route), k)
    _check(idx, dist, full, D, dtype, "%s k=%d %s %s" % (name, k, np.dtype(dtype).name, route))
    if name == "tiny":                                             # n = k + 1: every other row is a neighbour
        assert np.array_equal(np.sort(idx, axis=1), np.array([[j for j in range(n) if j != i] for i in range(n)]))


def test_off_centre():
    """every coordinate 4096 + N(0, 1), float32: |x|^2 is 1e7 times a neighbour's squared distance, so |x|^2 + |y|^2 - 2 x.y rounded
    in float32 is wrong by O(1) there while the direct differences are exact to TOL"""
    X, full = _uploaded("off_centre", np.float32), _full("off_centre", np.float32)
    k, D = 14, X.shape[1]
    ref_idx, ref_dist = NR.select(full, k)
    norms = (X.astype(np.float64) ** 2).sum(axis=1)
    ratio = norms.max() / np.median(ref_dist[:, -1] ** 2)
    sq = (X * X).sum(axis=1, dtype=np.float32)
    expansion = sq[:, None] + sq[None, :] - np.float32(2.0) * (X @ X.T)           # float32 throughout
    at = np.take_along_axis(expansion.astype(np.float64), ref_idx.astype(np.int64), axis=1)
    miss = np.abs(at - ref_dist ** 2).max() / np.median(ref_dist[:, -1] ** 2)
    print("off_centre: max|x|^2 / median kth^2 = %.2e; the float32 expansion misses d^2 by up to %.2e of the median kth^2" % (ratio, miss))
    assert ratio >= 1e5 and miss > 100 * 2 * _tol(D, np.float32)
    idx, dist = engine.knn(X, k)
    _check(idx, dist, full, D, np.float32, "off_centre")


@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicates(dtype):
    X, full = _uploaded("duplicates", dtype), _full("duplicates", dtype)
    n, D = X.shape
    same = full == 0.0
    assert (same.sum(axis=1) == 3).all()                           # every row is present three times, itself included
    idx, dist = engine.knn(X, 5)
    _check(idx, dist, full, D, dtype, "duplicates %s" % np.dtype(dtype).name)
    copies = np.array([[j for j in np.flatnonzero(same[i]) if j != i] for i in range(n)])
    assert (dist[:, :2] == 0.0).all() and (dist[:, 2] > 0.0).all() and np.array_equal(idx[:, :2], copies)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["lattice2", "lattice4"])
def test_lattice(name, dtype):
    """integer coordinates: every squared distance is exact, ties come in bulk, and the order is the reference's"""
    X, full = _uploaded(name, dtype), _full(name, dtype)
    assert X.shape == {"lattice2": (289, 2), "lattice4": (625, 4)}[name] and np.array_equal(X, np.rint(X)) and np.abs(X).max() <= 16
    ref_idx, ref_dist = NR.select(full, 8)
    assert (np.diff(ref_dist, axis=1) == 0).mean() > 0.5           # more ties than not
    idx, dist = engine.knn(X, 8)
    _check(idx, dist, full, X.shape[1], dtype, "%s %s" % (name, np.dtype(dtype).name), exact=True)
    assert np.array_equal(dist, ref_dist)                          # sqrt of an exact integer, correctly rounded on either side


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_query_range_and_repeat(dtype, metric):
    X = _uploaded("pilot", dtype)
    a = engine.knn(X, 14, metric=metric)
    b = engine.knn(X, 14, metric=metric)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))      # identical bits
    sub = engine.knn(X, 14, metric=metric, rows=(517, 901))
    assert sub[0].shape == (384, 14) and np.array_equal(sub[0], a[0][517:901])
    assert np.array_equal(sub[1].view(np.uint64), a[1][517:901].view(np.uint64))
    _check(sub[0], sub[1], _full("pilot", dtype, metric)[517:901], 50, dtype, "rows %s %s" % (metric, np.dtype(dtype).name), begin=517)
    dev = engine.knn(engine.DeviceMatrix.upload(X), 14, metric=metric, rows=(1099, 1100))                  # the last row alone
    assert np.array_equal(dev[0], a[0][1099:]) and np.array_equal(dev[1], a[1][1099:])


# ---- cosine ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["pilot", "wide", "scaled"])
def test_cosine(name, dtype, route):
    X, full = _uploaded(name, dtype), _full(name, dtype, "cosine")
    D, u, t = X.shape[1], U[np.dtype(dtype)], _tol(X.shape[1], dtype)
    what = "cosine %s %s %s" % (name, np.dtype(dtype).name, route)
    if name == "scaled":
        norms = np.linalg.norm(X.astype(np.float64), axis=1)
        assert norms.max() / norms.min() >= 1e4
    idx, dist = engine.knn(_arg(name, dtype, route), 14, metric="cosine")
    _check(idx, dist, full, D, dtype, what)
    # against the true value: rounding the unit rows to the element type moves |x^ - y^| by at most 2u
    true = np.take_along_axis(cdist(X.astype(np.float64), X.astype(np.float64), "cosine"), idx.astype(np.int64), axis=1)
    bound = t * true + 2 * u * np.sqrt(2 * true) * 2 + 4 * u * u
    print("%s: max |got - true| / bound = %.3f" % (what, float((np.abs(dist - true) / bound).max())))
    assert (np.abs(dist - true) <= bound).all(), what


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["host", "device"])
def test_refused(route):
    up = engine.DeviceMatrix.upload if route == "device" else (lambda A: A)
    for bad in (np.nan, np.inf, -np.inf):
        X = np.array(_uploaded("pilot", np.float32))
        X[7, 31] = bad
        X[900, 2] = bad
        for metric in ("euclidean", "cosine"):
            with pytest.raises(ValueError, match="row 7 "):
                engine.knn(up(X), 14, metric=metric)
    X = np.array(_uploaded("pilot", np.float64))
    X[11] = 0.0
    X[640] = 0.0
    with pytest.raises(ValueError, match="row 11 "):
        engine.knn(up(X), 14, metric="cosine")
    with pytest.raises(ValueError, match="row 11 "):
        engine.knn(up(X), 14, metric="cosine", rows=(0, 5))        # the corpus is checked, not the query range
    idx, dist = engine.knn(up(X), 14)                              # a zero row is an ordinary point of the euclidean metric
    assert idx[11, 0] == 640 and dist[11, 0] == 0.0 and idx[640, 0] == 11


# ---- connectivities -------------------------------------------------------------------------------------------------------------
def _smooth_inputs(case):
    if case == "pilot":
        return NR.select(_full("pilot", np.float32), 14)
    idx, dist = NR.select(_full("duplicates", np.float64), 5)
    if case == "all_zero_rows":
        dist = dist.copy()
        dist[::7] = 0.0                                            # cells whose neighbours all coincide with them: rho = 0
    return idx, dist


@pytest.mark.parametrize("case", ["pilot", "duplicates", "all_zero_rows"])
def test_smooth(case):
    idx, dist = _smooth_inputs(case)
    n_neighbors = dist.shape[1] + 1
    W, sigma, rho = NR.smooth(dist, n_neighbors)
    if case == "duplicates":
        assert (dist[:, :2] == 0).all() and (rho == dist[:, 2]).all()          # rho skips the zero distances
    if case == "all_zero_rows":
        assert (rho[::7] == 0).all() and (sigma[::7] == 1e-3 * dist.mean()).all() and dist.mean() > 0       # the global-mean floor
    w, s, r = engine.knn_smooth(dist, n_neighbors)
    assert w.shape == W.shape and s.shape == sigma.shape == r.shape and w.dtype == s.dtype == r.dtype == np.float64
    print("smooth %s: max |weight - restatement| = %.2e (bound %.0e); max relative sigma difference %.2e"
          % (case, float(np.abs(w - W).max()), WEIGHT_TOL, float((np.abs(s - sigma) / sigma).max())))
    assert np.abs(w - W).max() <= WEIGHT_TOL and np.array_equal(r, rho)
    assert ((w >= 0) & (w <= 1)).all() and (w[dist <= rho[:, None]] == 1.0).all()
    C = engine.knn_connectivities(idx, dist, n_neighbors)
    assert sp.isspmatrix_csr(C) and C.shape == (dist.shape[0],) * 2 and C.dtype == np.float64
    A = C.toarray()
    assert np.array_equal(A, A.T) and (np.diag(A) == 0).all()
    assert np.array_equal(A, NR.union(idx, w))                     # the union of the device's weights, to the bit
    assert np.abs(A - NR.union(idx, W)).max() <= 2 * WEIGHT_TOL    # a + b - ab of two weights, each within the bound


# ---- tl -------------------------------------------------------------------------------------------------------------------------
class _Adata:
    def __init__(self, X):
        self.obsm, self.uns = {"X_pca": X}, {}


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_tl_neighbors(metric):
    X = _uploaded("pilot", np.float32)
    ad = _Adata(X)
    assert tl.neighbors(ad, n_neighbors=15, n_pcs=30, metric=metric) is None
    G, C = ad.obsp["distances"], ad.obsp["connectivities"]
    assert set(ad.obsp) == {"distances", "connectivities"} and set(ad.uns) == {"neighbors"}
    assert ad.uns["neighbors"] == {"connectivities_key": "connectivities", "distances_key": "distances",
                                   "params": {"n_neighbors": 15, "method": "umap", "metric": metric, "use_rep": "X_pca", "n_pcs": 30}}
    for M in (G, C):
        assert sp.isspmatrix_csr(M) and M.shape == (1100, 1100) and M.dtype == np.float64
    assert (np.diff(G.indptr) == 14).all()
    # the strided window of the first 30 columns gives what a packed copy of them gives
    packed = np.ascontiguousarray(X[:, :30])
    idx, dist = engine.knn(packed, 14, metric=metric)
    assert np.array_equal(G.indices.reshape(1100, 14), idx) and np.array_equal(G.data.reshape(1100, 14), dist)
    _check(idx, dist, NR.distance_rows(packed, metric), 30, np.float32, "tl %s" % metric)
    assert np.array_equal(C.toarray(), engine.knn_connectivities(idx, dist, 15).toarray()) and np.array_equal(C.toarray(), C.toarray().T)
    assert np.abs(C.toarray() - NR.connectivities(idx, dist, 15).toarray()).max() <= 2 * WEIGHT_TOL
    assert np.array_equal(X, _uploaded("pilot", np.float32))
    tl.neighbors(ad, n_neighbors=4, key_added="small", metric=metric)
    assert set(ad.obsp) == {"distances", "connectivities", "small_distances", "small_connectivities"} and set(ad.uns) == {"neighbors", "small"}
    assert (np.diff(ad.obsp["small_distances"].indptr) == 3).all() and ad.uns["small"]["params"]["n_pcs"] is None
