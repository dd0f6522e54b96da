"""Louvain communities (K17), the parts that need no device.  The C ABI refuses every argument it can judge before any HIP call (a box
without a device returns PILOT_OT_EHIP from the first HIP call, so PILOT_OT_EINVAL / PILOT_OT_ENOTSUP show the check came first);
engine.louvain / tl.louvain / tl.reclustering_data raise before the library is touched (the library handle is replaced by an object
that fails the test on any use).  The restatement (tests/louvain_restatement.py) is checked against networkx's modularity and for
the properties the rule promises."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import louvain_graphs as LG
import louvain_restatement as LR
from pilot_amd import _lib, engine, tl


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def _rc(n=4, indptr=(0, 2, 3, 5, 6), indices=(1, 2, 0, 0, 3, 2), weights=(1, 2, 1, 2, 1, 1), resolution=1.0, tol=1e-3, max_levels=32,
        null=None):
    L = _lib.load()
    ip, ix, w = np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int32), np.array(weights, dtype=np.float64)
    labels, q, info = np.full(16, -7, dtype=np.int32), ctypes.c_double(-7.0), np.full(3, -7, dtype=np.int32)
    p = dict(indptr=_lib.lptr(ip), indices=_lib.iptr(ix), weights=_lib.dptr(w), labels=_lib.iptr(labels), modularity=ctypes.byref(q),
             info=_lib.iptr(info))
    if null:
        p[null] = None
    rc = L.pilot_ot_louvain(n, p["indptr"], p["indices"], p["weights"], resolution, tol, max_levels, p["labels"], p["modularity"], p["info"])
    return rc, L.pilot_ot_last_error(), labels, q.value, info


@pytest.mark.parametrize("bad,code,fragment", [
    (dict(null="indptr"), _lib.EINVAL, b"NULL"), (dict(null="indices"), _lib.EINVAL, b"NULL"), (dict(null="weights"), _lib.EINVAL, b"NULL"),
    (dict(null="labels"), _lib.EINVAL, b"NULL"), (dict(null="modularity"), _lib.EINVAL, b"NULL"), (dict(null="info"), _lib.EINVAL, b"NULL"),
    (dict(n=-1), _lib.EINVAL, b"n=-1"),
    (dict(indptr=(1, 2, 3, 5, 6)), _lib.EINVAL, b"indptr[0]"), (dict(indptr=(0, 2, 1, 5, 6)), _lib.EINVAL, b"indptr[2]"),
    (dict(indices=(1, 2, 0, 0, -1, 2)), _lib.EINVAL, b"indices[4]"), (dict(indices=(1, 4, 0, 0, 3, 2)), _lib.EINVAL, b"indices[1]"),
    (dict(weights=(1, 2, -1, 2, 1, 1)), _lib.EINVAL, b"weights[2]"), (dict(weights=(1, 2, 1, float("nan"), 1, 1)), _lib.EINVAL, b"weights[3]"),
    (dict(weights=(1, 2, 1, 2, 1, float("inf"))), _lib.EINVAL, b"weights[5]"),
    (dict(resolution=-0.5), _lib.EINVAL, b"resolution"), (dict(resolution=float("nan")), _lib.EINVAL, b"resolution"),
    (dict(resolution=float("inf")), _lib.EINVAL, b"resolution"),
    (dict(tol=-1e-9), _lib.EINVAL, b"tol"), (dict(tol=float("nan")), _lib.EINVAL, b"tol"),
    (dict(max_levels=0), _lib.EINVAL, b"max_levels"), (dict(max_levels=-2), _lib.EINVAL, b"max_levels"),
    (dict(n=2 ** 31), _lib.ENOTSUP, b"32-bit"),
    (dict(weights=(1e200, 2, 1, 2, 1, 1)), _lib.EINVAL, b"overflows"),
])
def test_louvain_refuses_before_any_hip_call(bad, code, fragment):
    rc, msg, labels, q, info = _rc(**bad)
    assert rc == code and fragment in msg, (bad, rc, msg)
    assert (labels == -7).all()


def test_louvain_refuses_too_many_entries():
    """more than INT_MAX entries in A + A^T: the cap is lowered through the test switch, 2^31 entries are not made"""
    try:
        _lib.test_switch("PILOT_OT_LOUVAIN_MAX_NNZ", "5")       # the graph of _rc has 6 entries in S
        rc, msg, _, _, _ = _rc()
        assert rc == _lib.ENOTSUP and b"32-bit edge indices" in msg, (rc, msg)
    finally:
        _lib.test_switch("PILOT_OT_LOUVAIN_MAX_NNZ", None)


def test_louvain_without_weight_needs_no_device():
    rc, msg, labels, q, info = _rc(n=0, indptr=(0,), indices=(), weights=())
    assert rc == _lib.OK and q == 0.0 and info.tolist() == [0, 0, 0] and (labels == -7).all(), msg
    for kw in (dict(n=5, indptr=(0,) * 6, indices=(), weights=()), dict(n=5, indptr=(0, 1, 1, 2, 2, 2), indices=(1, 4), weights=(0, 0))):
        rc, msg, labels, q, info = _rc(**kw)
        assert rc == _lib.OK and q == 0.0 and info.tolist() == [0, 0, 5] and labels[:5].tolist() == [0, 1, 2, 3, 4], (kw, msg)
        assert LR.louvain(sp.csr_matrix((5, 5)))[2] == (0, 0, 5)


def test_good_arguments_get_as_far_as_the_device():
    want = _lib.OK if _lib.device_count() > 0 else _lib.EHIP
    for kw in (dict(), dict(resolution=0.0), dict(tol=0.0), dict(max_levels=1), dict(n=1, indptr=(0, 1), indices=(0,), weights=(2,)),
               dict(indices=(2, 1, 0, 0, 3, 3))):
        rc, msg, _, _, _ = _rc(**kw)
        assert rc == want, (kw, msg)
    assert "pilot_ot_louvain" in _lib.SYMBOLS


# ---- engine and tl ----------------------------------------------------------------------------------------------------------------
G4 = sp.csr_matrix(np.array([[0, 1, 2, 0], [1, 0, 0, 0], [2, 0, 0, 1], [0, 0, 1, 0]], dtype=np.float64))


@pytest.mark.parametrize("kw", [
    dict(graph=np.ones((3, 4))), dict(graph=sp.csr_matrix(np.ones((3, 4)))), dict(graph=np.ones(4)), dict(graph=np.ones((2, 2, 2))),
    dict(graph=None), dict(graph=np.array([["a", "b"], ["c", "d"]])), dict(graph=-G4), dict(graph=G4 * np.nan), dict(graph=G4 * np.inf),
    dict(graph=G4.toarray() * -1.0),
    dict(resolution=-1), dict(resolution=np.nan), dict(resolution=np.inf), dict(resolution="1"), dict(resolution=None), dict(resolution=True),
    dict(tol=-1e-3), dict(tol=np.nan), dict(tol=None), dict(max_levels=0), dict(max_levels=2.0), dict(max_levels=True), dict(max_levels=None),
])
def test_engine_louvain_argument_errors(no_library, kw):
    with pytest.raises(ValueError):
        engine.louvain(**{**dict(graph=G4), **kw})


def test_engine_louvain_reaches_the_library_last(no_library):
    for graph in (G4, G4.tocoo(), G4.tocsc(), G4.toarray(), G4.toarray().astype(np.int64), G4.astype(np.float32), sp.csr_matrix((0, 0))):
        with pytest.raises(AssertionError, match="touched"):
            engine.louvain(graph, resolution=0.5, tol=0, max_levels=3, return_info=True)


class _Adata:
    def __init__(self, graph=True):
        self.obs = pd.DataFrame({"a": ["x"] * 4})
        self.uns, self.obsp = {}, {}
        if graph:
            self.uns["neighbors"] = {"connectivities_key": "connectivities", "distances_key": "distances", "params": {}}
            self.obsp = {"connectivities": G4, "distances": G4}


def test_tl_louvain_argument_errors(no_library):
    with pytest.raises(ValueError, match="tl.neighbors"):
        tl.louvain(_Adata(graph=False))
    with pytest.raises(ValueError, match="tl.neighbors"):
        tl.louvain(_Adata(), neighbors_key="other")
    half = _Adata()
    del half.obsp["distances"]
    with pytest.raises(ValueError, match="tl.neighbors"):
        tl.louvain(half, mode="distances")
    ad = _Adata()
    for kw in (dict(mode="both"), dict(mode=None), dict(resolution=-1.0), dict(resolution=np.nan)):
        with pytest.raises(ValueError):
            tl.louvain(ad, **kw)
    assert list(ad.obs.columns) == ["a"] and set(ad.uns) == {"neighbors"}
    for kw in (dict(), dict(mode="distances", resolution=0.3, key_added="c")):
        with pytest.raises(AssertionError, match="touched"):
            tl.louvain(ad, **kw)


def test_tl_louvain_layout(monkeypatch):
    """obs / uns as specified, with the engine call replaced by the restatement"""
    def restated(graph, resolution=1.0, tol=1e-3, max_levels=32, return_info=False):
        labels, q, (levels, sweeps, k) = LR.louvain(graph, resolution, tol, max_levels)
        return labels, {"modularity": q, "levels": levels, "sweeps": sweeps, "communities": k}

    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())
    monkeypatch.setattr(engine, "louvain", restated)
    ad = _Adata()
    ad.obs = pd.DataFrame({"a": ["x"] * 40})
    ring = LG.ring_of_cliques()
    ad.obsp = {"nb_connectivities": ring, "nb_distances": ring}
    ad.uns = {"nb": {"connectivities_key": "nb_connectivities", "distances_key": "nb_distances"}}
    assert tl.louvain(ad, neighbors_key="nb") is None
    col = ad.obs["louvain"]
    assert isinstance(col.dtype, pd.CategoricalDtype) and list(col.cat.categories) == [str(c) for c in range(8)]
    assert col.astype(str).tolist() == [str(i // 5) for i in range(40)]
    assert ad.uns["louvain"] == {"params": {"resolution": 1.0, "mode": "connectivities"}, "modularity": LR.modularity(ring, np.arange(40) // 5)}


def test_tl_reclustering_data_argument_errors(no_library):
    X = np.random.default_rng(0).normal(size=(30, 4))
    for kw in (dict(method_="gauss"), dict(method_=None), dict(mode="both"), dict(resu=-0.1), dict(resu=np.nan)):
        with pytest.raises(ValueError):
            tl.reclustering_data(X, **kw)
    with pytest.raises(ValueError):
        tl.reclustering_data(X.ravel())
    with pytest.raises(ValueError):                                # 15 neighbours need 15 cells
        tl.reclustering_data(X[:10])
    with pytest.raises(AssertionError, match="touched"):
        tl.reclustering_data(X)
    with pytest.raises(AssertionError, match="touched"):
        tl.reclustering_data(np.ones((60, 55)))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_modularity_agrees_with_networkx():
    nx = pytest.importorskip("networkx")
    ring = LG.ring_of_cliques()
    W = LG.random_symmetric(60, 5, seed=2)
    rng = np.random.default_rng(4)
    for A, labels in ((ring, np.arange(40) // 5), (ring, np.arange(40) // 10), (W, rng.integers(0, 5, 60)), (W, LR.louvain(W)[0])):
        G = nx.from_scipy_sparse_array(A)
        parts = [set(np.flatnonzero(labels == c).tolist()) for c in np.unique(labels)]
        for gamma in (1.0, 0.5):
            assert abs(LR.modularity(A, labels, gamma) - nx.community.modularity(G, parts, weight="weight", resolution=gamma)) <= 1e-14


def test_restatement_keeps_its_promises():
    for A, gamma, tol in ((LG.ring_of_cliques(), 1.0, 0.0), (LG.random_symmetric(), 1.0, 1e-3), (LG.directed_knn_ranks(), 0.5, 0.0),
                          (LG.hub(), 0.25, 0.0), (LG.odd_ends()[0], 1.0, 0.0)):
        trace = []
        labels, q, (levels, sweeps, k) = LR.louvain(A, gamma, tol, trace=trace)
        assert len(trace) == levels and 1 <= levels <= 32 and sweeps <= 128 * levels
        for kept in trace:                                          # Qs never decreases over the kept sweeps of a level
            assert (np.diff(kept) > 0).all(), kept
        assert LG.numbered_by_size(labels) and labels.dtype == np.int32 and k == labels.max() + 1
        assert abs(q - LR.modularity(A, labels, gamma)) <= 1e-13
        assert q >= LR.modularity(A, np.arange(A.shape[0]), gamma)
    ring = LR.louvain(LG.ring_of_cliques(), 1.0, 0.0)[0]
    assert ring.tolist() == (np.arange(40) // 5).tolist()
    assert LG.same_partition(ring, LR.sequential_louvain(LG.ring_of_cliques())[0])
    # a level cannot run more than its share; one level only
    assert LR.louvain(LG.random_symmetric(), max_levels=1)[2][0] == 1
    # the inputs of the exact cases are exact
    for A in (LG.ring_of_cliques(), LG.random_symmetric(), LG.directed_knn_ranks(), LG.hub(), LG.odd_ends()[0]):
        assert LG.exact_enough(A)
    assert (LG.directed_knn_ranks() != LG.directed_knn_ranks().T).nnz > 0
    odd, n = LG.odd_ends()
    assert odd.nnz > LR.as_csr(odd).nnz                             # repeats and a stored zero
    assert LR.ordered_sum(np.arange(1000.0)) == 499500.0


def test_tile_crossing_graph_is_what_the_device_tests_need():
    """the structure tests/test_gpu_louvain.py relies on to reach the tiled sort, the scan's carry and every degree bin's limits
    (no restatement run here)"""
    A = LG.tile_crossing()
    assert A.shape == (9000, 9000) and (A != A.T).nnz == 0 and LG.exact_enough(A) and A.data.min() >= 1.0
    S = LR.as_csr(A) + LR.as_csr(A).T
    deg = np.diff(S.tocsr().indptr)
    assert deg[:11].tolist() == list(LG.LADDER) == [63, 64, 65, 256, 257, 512, 513, 4096, 4097, 8192, 8193]
    assert deg[11:32].tolist() == [0] * 21 and (deg == 0).sum() == 21 and deg[32:].max() == 19
    assert A.shape[0] > 8192 and S.nnz == 106198 > 8192 and A.data.sum() == 347014.0
    assert S.diagonal().sum() == 0.0
    B = LG.tile_crossing()                                          # deterministic
    assert (A != B).nnz == 0 and np.array_equal(A.indices, B.indices)
    for n in (2049, 4096):                                          # the two sizes of the unsymmetric graph past one sort tile
        K = LG.directed_knn_ranks(n=n)
        assert K.shape == (n, n) and (K != K.T).nnz > 0 and LG.exact_enough(K)
