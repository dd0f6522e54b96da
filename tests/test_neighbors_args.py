"""The cell neighbour graph (K16), the parts that need no device.  The C ABI refuses every argument it can judge before any HIP call (a
box without a device returns PILOT_OT_EHIP from the first HIP call, so PILOT_OT_EINVAL / PILOT_OT_ENOTSUP show the check came first),
and engine.knn / engine.knn_smooth / engine.knn_connectivities / tl.neighbors raise before the library is touched (the library handle
is replaced by an object that fails the test on any use).  tl.neighbors' outputs are checked with the engine calls replaced by
tests/neighbors_restatement.py, and the restatement against scipy's cdist."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.spatial.distance import cdist

import neighbors_restatement as NR
from pilot_amd import _lib, engine, tl


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def _rows_rc(n=10, D=3, ld=None, dtype=1, metric=0, k=2, rows=None, null=None):
    L = _lib.load()
    X = np.ones((max(min(n, 100), 1), max(D, 1)))
    idx = np.zeros(100 * 65, dtype=np.int32)
    dist = np.zeros(100 * 65)
    p = dict(X=ctypes.c_void_p(X.ctypes.data), indices=_lib.iptr(idx), distances=_lib.dptr(dist))
    if null:
        p[null] = None
    begin, end = (0, n) if rows is None else rows
    rc = L.pilot_ot_knn_rows(p["X"], 0, dtype, n, D, D if ld is None else ld, metric, k, begin, end, p["indices"], p["distances"])
    return rc, L.pilot_ot_last_error()


@pytest.mark.parametrize("bad,code,fragment", [
    (dict(null="X"), _lib.EINVAL, b"NULL"), (dict(null="indices"), _lib.EINVAL, b"NULL"), (dict(null="distances"), _lib.EINVAL, b"NULL"),
    (dict(k=0), _lib.EINVAL, b"k=0"), (dict(k=-3), _lib.EINVAL, b"k=-3"),
    (dict(n=100, k=65), _lib.ENOTSUP, b"at most 64"),
    (dict(n=2, k=2), _lib.EINVAL, b"k + 1"), (dict(n=0, k=1), _lib.EINVAL, b"k + 1"),
    (dict(n=2 ** 31, k=2), _lib.ENOTSUP, b"32-bit"),
    (dict(D=0), _lib.EINVAL, b"D=0"), (dict(D=-1), _lib.EINVAL, b"D=-1"),
    (dict(ld=2), _lib.EINVAL, b"ld"),
    (dict(rows=(-1, 4)), _lib.EINVAL, b"row range"), (dict(rows=(4, 4)), _lib.EINVAL, b"row range"),
    (dict(rows=(5, 3)), _lib.EINVAL, b"row range"), (dict(rows=(0, 11)), _lib.EINVAL, b"row range"),
    (dict(metric=2), _lib.EINVAL, b"metric"), (dict(metric=-1), _lib.EINVAL, b"metric"),
    (dict(dtype=2), _lib.EINVAL, b"dtype"),
])
def test_knn_rows_refuses_before_any_hip_call(bad, code, fragment):
    rc, msg = _rows_rc(**bad)
    assert rc == code and fragment in msg, (bad, rc, msg)


def _smooth_rc(n=4, k=3, null=None, value=None):
    L = _lib.load()
    d = np.ones(4 * 65)
    if value is not None:
        d[5] = value
    out = np.zeros(4 * 65)
    p = dict(distances=_lib.dptr(d), weights=_lib.dptr(out), sigma=_lib.dptr(out), rho=_lib.dptr(out))
    if null:
        p[null] = None
    rc = L.pilot_ot_knn_smooth(p["distances"], n, k, p["weights"], p["sigma"], p["rho"])
    return rc, L.pilot_ot_last_error()


@pytest.mark.parametrize("bad,code,fragment", [
    (dict(null="distances"), _lib.EINVAL, b"NULL"), (dict(null="weights"), _lib.EINVAL, b"NULL"), (dict(null="sigma"), _lib.EINVAL, b"NULL"),
    (dict(null="rho"), _lib.EINVAL, b"NULL"),
    (dict(k=0), _lib.EINVAL, b"k=0"), (dict(k=65), _lib.ENOTSUP, b"at most 64"), (dict(n=0), _lib.EINVAL, b"n=0"),
    (dict(n=2 ** 31), _lib.ENOTSUP, b"32-bit"),
    (dict(value=-1.0), _lib.EINVAL, b"distances[1, 2]"), (dict(value=float("nan")), _lib.EINVAL, b"distances[1, 2]"),
    (dict(value=float("inf")), _lib.EINVAL, b"distances[1, 2]"),
])
def test_knn_smooth_refuses_before_any_hip_call(bad, code, fragment):
    rc, msg = _smooth_rc(**bad)
    assert rc == code and fragment in msg, (bad, rc, msg)


def test_good_arguments_get_as_far_as_the_device():
    want = _lib.OK if _lib.device_count() > 0 else _lib.EHIP
    for kw in (dict(), dict(metric=1), dict(dtype=0, ld=6), dict(k=9), dict(rows=(3, 7)), dict(n=65, k=64)):
        rc, msg = _rows_rc(**kw)
        assert rc == want, (kw, msg)
    rc, msg = _smooth_rc()
    assert rc == want, msg
    assert "pilot_ot_knn_rows" in _lib.SYMBOLS and "pilot_ot_knn_smooth" in _lib.SYMBOLS
    assert _lib.KNN_ROWS_MAX_K == 64 == engine.KNN_MAX_K and _lib.ROW_METRICS == {"euclidean": 0, "cosine": 1}


# ---- engine ---------------------------------------------------------------------------------------------------------------------
X = (np.arange(60, dtype=np.float64).reshape(20, 3) * 7) % 11


@pytest.mark.parametrize("kw", [
    dict(k=0), dict(k=-1), dict(k=65), dict(k=2.0), dict(k=True), dict(k=None), dict(k=20),         # 20 rows: k <= 19
    dict(metric="sqeuclidean"), dict(metric=0), dict(metric=None),
    dict(rows=(-1, 4)), dict(rows=(4, 4)), dict(rows=(5, 3)), dict(rows=(0, 21)), dict(rows=(0.5, 3)), dict(rows=(0, True)),
])
def test_engine_knn_argument_errors(no_library, kw):
    args = dict(k=3)
    args.update(kw)
    for arg in (X, X.astype(np.float32), engine.DeviceMatrix(0x1000, 20, shape=(20, 3))):
        with pytest.raises(ValueError):
            engine.knn(arg, **args)


def test_engine_knn_shapes(no_library):
    for arg in (X.ravel(), np.ones((4, 0)), np.ones((2, 3, 4)), None, engine.DeviceMatrix(0x1000, 20, shape=(20, 3), dtype=np.int32)):
        with pytest.raises(ValueError):
            engine.knn(arg, 2)
    # every check passed: the call is the first use of the library (a strided window and an integer matrix included)
    for arg, kw in ((X, dict()), (X[:, :2], dict()), (X.astype(np.int64), dict(metric="cosine")), (X, dict(rows=(3, 9))),
                    (engine.DeviceMatrix(0x1000, 20, shape=(20, 3), dtype=np.float32), dict(k=19))):
        with pytest.raises(AssertionError, match="touched"):
            engine.knn(arg, **{**dict(k=3), **kw})


def test_engine_graph_argument_errors(no_library):
    idx = np.array([[1, 2], [0, 2], [0, 1]], dtype=np.int32)
    dist = np.array([[1.0, 2.0], [1.0, 1.5], [1.5, 2.0]])
    for bad in (dict(distances=dist[:, :1]), dict(n_neighbors=2), dict(n_neighbors=3.0), dict(n_neighbors=True), dict(distances=dist.ravel()),
                dict(distances=-dist), dict(distances=np.where(dist > 1.9, np.nan, dist)), dict(distances=np.ones((3, 65)), n_neighbors=66),
                dict(distances=np.ones((0, 2)))):
        args = {**dict(distances=dist, n_neighbors=3), **bad}
        with pytest.raises(ValueError):
            engine.knn_smooth(**args)
        with pytest.raises(ValueError):
            engine.knn_connectivities(idx, **args)
    for bad_idx in (idx[:2], idx.astype(np.float64), idx + 1, idx - 1):
        with pytest.raises(ValueError):
            engine.knn_connectivities(bad_idx, dist, 3)
    with pytest.raises(AssertionError, match="touched"):
        engine.knn_smooth(dist, 3)
    with pytest.raises(AssertionError, match="touched"):
        engine.knn_connectivities(idx, dist, 3)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_agrees_with_scipy():
    rng = np.random.default_rng(0)
    Y = rng.normal(size=(90, 7))
    for metric in ("euclidean", "cosine"):
        idx, dist, full = NR.knn(Y, 6, metric)
        ref = cdist(Y, Y, metric)
        off = ~np.eye(90, dtype=bool)
        assert np.abs(full - ref)[off].max() <= 1e-13
        np.fill_diagonal(ref, np.inf)
        assert np.array_equal(idx, np.argsort(ref, axis=1, kind="stable")[:, :6])          # no ties in this cloud
        assert (np.diff(dist, axis=1) >= 0).all() and (idx != np.arange(90)[:, None]).all()
    sub = NR.knn(Y, 6, "cosine", rows=(17, 40))
    assert np.array_equal(sub[0], idx[17:40]) and np.array_equal(sub[1], dist[17:40])
    U = NR.unit_rows(Y.astype(np.float32))
    assert U.dtype == np.float32 and np.abs(np.linalg.norm(U.astype(np.float64), axis=1) - 1.0).max() <= 4 * 2.0 ** -24
    # ties go by index: a point between two mirror images
    T = np.array([[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [5.0, 5.0]])
    assert NR.knn(T, 3)[0][0].tolist() == [1, 2, 3] and NR.knn(T, 2)[0][4].tolist() == [1, 3]


def test_restatement_smoothing_rule():
    rng = np.random.default_rng(1)
    d = np.sort(rng.gamma(2.0, 1.0, (40, 14)), axis=1)
    d[3] = 0.0                                                     # rho = 0: the floor is the global mean's
    d[5, :4] = 0.0                                                 # duplicates: rho is the smallest NON-zero distance
    W, sigma, rho = NR.smooth(d, 15)
    assert rho[3] == 0.0 and sigma[3] == 1e-3 * d.mean() and (W[3] == 1.0).all()
    assert rho[5] == d[5, 4] and (W[5, :5] == 1.0).all() and (W[5, 5:] < 1.0).all()
    assert np.array_equal(rho[[0, 1]], d[[0, 1], 0]) and (W[:, 0] == 1.0).all() and ((W >= 0) & (W <= 1)).all()
    # row 5: five weights of 1 are already above log2(15), so sigma falls to its floor of 1e-3 x the row's mean
    assert sigma[5] == 1e-3 * d[5].mean()
    rows = np.delete(np.arange(40), [3, 5])
    sums = np.exp(-np.maximum(d - rho[:, None], 0.0) / sigma[:, None]).sum(axis=1)
    assert np.abs(sums[rows] - np.log2(15)).max() < 1e-5              # the bisection's stopping rule
    assert (np.diff(W, axis=1) <= 0).all()


# ---- connectivities and tl.neighbors with the engine calls replaced by the restatement ----------------------------------------------
@pytest.fixture
def restated(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())
    calls = []

    def knn(Xa, k, metric="euclidean", rows=None):
        calls.append((Xa, k, metric))
        return NR.knn(np.asarray(Xa), k, metric, rows)[:2]

    monkeypatch.setattr(engine, "knn", knn)
    monkeypatch.setattr(engine, "knn_smooth", lambda distances, n_neighbors: NR.smooth(distances, n_neighbors))
    return calls


def test_connectivities_of_a_hand_made_graph(restated):
    idx = np.array([[1, 2], [0, 2], [1, 3], [4, 2], [3, 2]], dtype=np.int32)
    dist = np.array([[1.0, 2.0], [1.0, 1.5], [1.5, 3.0], [0.5, 3.0], [0.5, 4.0]])
    C = engine.knn_connectivities(idx, dist, 3)
    assert sp.isspmatrix_csr(C) and C.shape == (5, 5) and C.dtype == np.float64
    A = C.toarray()
    assert np.array_equal(A, A.T) and (np.diag(A) == 0).all()
    assert np.array_equal(A, NR.union(idx, NR.smooth(dist, 3)[0]))
    assert A[0, 1] == 1.0 and A[3, 4] == 1.0                        # the nearest neighbour has weight 1 on either side
    assert A[2, 0] == A[0, 2] > 0 and 0 not in idx[2]               # one-sided edges are kept
    assert A[0, 3] == 0.0 and A[0, 4] == 0.0
    w02, w20 = NR.smooth(dist, 3)[0][0, 1], 0.0
    assert A[0, 2] == w02 + w20 - w02 * w20


class _Adata:
    def __init__(self, n=40, D=6, dtype=np.float32, obsp=True):
        rng = np.random.default_rng(3)
        self.obsm = {"X_pca": rng.normal(size=(n, D)).astype(dtype), "X_other": rng.normal(size=(n, 3))}
        self.uns = {}
        if obsp:
            self.obsp = {}


def test_tl_neighbors_argument_errors(no_library):
    ad = _Adata()
    for kw in (dict(n_neighbors=1), dict(n_neighbors=0), dict(n_neighbors=66), dict(n_neighbors=15.0), dict(n_neighbors=True),
               dict(n_neighbors=41), dict(use_rep="X_umap"), dict(metric="manhattan"), dict(n_pcs=0), dict(n_pcs=7), dict(n_pcs=2.0),
               dict(use_rep="X_other", n_pcs=4)):
        with pytest.raises(ValueError):
            tl.neighbors(ad, **kw)
    assert not ad.obsp and not ad.uns
    for kw in (dict(), dict(n_neighbors=40), dict(n_pcs=6), dict(metric="cosine", use_rep="X_other")):
        with pytest.raises(AssertionError, match="touched"):
            tl.neighbors(ad, **kw)
    with pytest.raises(NotImplementedError, match="tl.neighbors.*Louvain"):
        tl.extract_annot_expression(ad, reclustering=True)


@pytest.mark.parametrize("key_added", [None, "nb"])
def test_tl_neighbors_layout(restated, key_added):
    ad = _Adata(obsp=key_added is None)
    if key_added is not None:
        del ad.obsm["X_other"]
    assert tl.neighbors(ad, n_neighbors=5, n_pcs=4, metric="cosine", key_added=key_added) is None
    names = ("neighbors", "distances", "connectivities") if key_added is None else ("nb", "nb_distances", "nb_connectivities")
    assert set(ad.uns) == {names[0]} and set(ad.obsp) == set(names[1:])
    assert ad.uns[names[0]] == {"connectivities_key": names[2], "distances_key": names[1],
                                "params": {"n_neighbors": 5, "method": "umap", "metric": "cosine", "use_rep": "X_pca", "n_pcs": 4}}
    (Xa, k, metric), = restated
    assert k == 4 and metric == "cosine" and Xa.shape == (40, 4) and Xa.dtype == np.float32
    assert np.shares_memory(Xa, ad.obsm["X_pca"]) and Xa.strides == (24, 4)          # the column window, not a copy
    G, C = ad.obsp[names[1]], ad.obsp[names[2]]
    idx, dist, _ = NR.knn(ad.obsm["X_pca"][:, :4], 4, "cosine")
    for M in (G, C):
        assert sp.isspmatrix_csr(M) and M.shape == (40, 40) and M.dtype == np.float64
    assert (np.diff(G.indptr) == 4).all() and np.array_equal(G.indices.reshape(40, 4), idx) and np.array_equal(G.data.reshape(40, 4), dist)
    assert np.array_equal(C.toarray(), NR.connectivities(idx, dist, 5).toarray()) and np.array_equal(C.toarray(), C.toarray().T)
    # zero distances (duplicated cells) are dropped from the stored entries, as scanpy's eliminate_zeros() does
    ad2 = _Adata()
    ad2.obsm["X_pca"][1] = ad2.obsm["X_pca"][0]
    tl.neighbors(ad2, n_neighbors=5)
    assert np.diff(ad2.obsp["distances"].indptr).tolist() == [3, 3] + [4] * 38
    assert ad2.uns["neighbors"]["params"] == {"n_neighbors": 5, "method": "umap", "metric": "euclidean", "use_rep": "X_pca", "n_pcs": None}
