"""Leiden communities (K20), the parts that need no device: the restatement (tests/leiden_restatement.py) keeps what the rule
promises -- connected communities above all --, the C ABI and the Python layers refuse what they can judge before any HIP call
(the library handle is replaced by an object that fails the test on any use), tl.rand_index is scikit-learn's rand_score, and
tl.leiden_clustering's resolution loop is the reference's, with an end."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
from sklearn.metrics import rand_score

import leiden_restatement as LD
import louvain_graphs as LG
import louvain_restatement as LR
import silhouette_cohorts as C
from pilot_amd import _lib, engine, tl

GAMMAS = (1.0, 0.5, 0.25, 2.0)


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _graph(name):
    if name == "odd_ends":
        return LG.odd_ends()[0]
    if name == "uniform_union_graph":
        return LG.uniform_union_graph(400)
    return getattr(LG, name)()


@pytest.mark.parametrize("name", ["ring_of_cliques", "random_symmetric", "directed_knn_ranks", "hub", "odd_ends", "uniform_union_graph"])
def test_restatement_returns_connected_communities(name):
    """every community connected in S, Q the independent modularity, the counts consistent, at four resolutions; the settle step
    really cancels moves on the graphs that have contested singletons"""
    A = _graph(name)
    tol = 1e-3 if name == "uniform_union_graph" else 0.0
    cancelled = 0
    for gamma in GAMMAS:
        trace = []
        labels, q, (levels, move_sweeps, refine_sweeps, k) = LD.leiden(A, gamma, tol, trace=trace)
        assert LD.disconnected(A, labels) == 0, (name, gamma)
        assert abs(q - LR.modularity(A, labels, gamma)) <= 1e-13, (name, gamma, q)
        assert labels.dtype == np.int32 and LG.numbered_by_size(labels) and k == labels.max() + 1
        assert 1 <= levels <= 32 and levels <= move_sweeps <= 128 * levels and len(trace) == refine_sweeps <= 128 * levels
        for t in trace:
            assert t["moved"] <= t["decided"] and t["cancelled"] >= 0 and t["moved"] == len(t["moved_nodes"])
            assert np.isin(t["moved_nodes"], t["decided_nodes"]).all()       # only a node that decided moves
        cancelled += sum(t["cancelled"] for t in trace)
        if name == "ring_of_cliques" and gamma == 1.0:
            assert labels.tolist() == (np.arange(40) // 5).tolist()
    print("%s: moves cancelled by the settle step over the four resolutions: %d" % (name, cancelled))
    if name in ("random_symmetric", "hub", "directed_knn_ranks", "odd_ends"):
        assert cancelled > 0


def test_restatement_finds_the_planted_blobs():
    X, planted = LG.blobs(n=600)
    idx, dist, _ = LG.NR.knn(X, 14)
    A = LG.NR.connectivities(idx, dist, 15)
    labels, q, info = LD.leiden(A)
    assert LG.same_partition(labels, planted) and info[3] == 6 and LD.disconnected(A, labels) == 0
    assert abs(q - LR.modularity(A, labels, 1.0)) <= 1e-13


def test_restatement_edges():
    """no weight, no node, one level only; disconnected() counts what it says"""
    assert LD.leiden(sp.csr_matrix((5, 5)))[2] == (0, 0, 0, 5) and LD.leiden(sp.csr_matrix((0, 0)))[0].shape == (0,)
    labels, q, info = LD.leiden(sp.csr_matrix(np.array([[3.0]])), 0.5)
    assert labels.tolist() == [0] and info == (1, 1, 0, 1) and abs(q - 0.5) <= 1e-15
    labels, q, info = LD.leiden(LG.random_symmetric(), max_levels=1)
    assert info[0] == 1 and abs(q - LR.modularity(LG.random_symmetric(), labels, 1.0)) <= 1e-13
    ring = LG.ring_of_cliques()
    assert LD.disconnected(ring, np.arange(40) // 5) == 0
    assert LD.disconnected(ring, np.arange(40) // 5 % 4) == 4         # cliques c and c + 4 share no edge
    assert LD.disconnected(ring, np.arange(40)) == 0


def test_louvain_restatement_returns_disconnected_communities():
    """the contrast K20 exists for, on the smallest of the rows DESIGN.md K20 lists (the larger ones are checked beside the device
    in tests/test_gpu_leiden.py): at tol = 0 K17's rule leaves 2 communities of hub() at resolution 2 in pieces, K20's none"""
    A = LG.hub()
    assert LD.disconnected(A, LR.louvain(A, 2.0, 0.0)[0]) == 2
    assert LD.disconnected(A, LD.leiden(A, 2.0, 0.0)[0]) == 0


# ---- the Rand index ---------------------------------------------------------------------------------------------------------------
def test_rand_index_is_sklearns():
    rng = np.random.default_rng(3)
    for n, ka, kb in ((2, 1, 2), (15, 3, 3), (60, 3, 5), (200, 7, 2), (33, 1, 1)):
        a, b = rng.integers(0, ka, n), rng.integers(0, kb, n)
        assert abs(tl.rand_index(a, b) - rand_score(a, b)) <= 1e-15
        assert abs(tl.rand_index(a.astype(str), b) - rand_score(a, b)) <= 1e-15
    assert tl.rand_index([0, 0, 1, 1], ["x", "x", "y", "y"]) == 1.0 and tl.rand_index([0], [5]) == 1.0
    assert tl.rand_index([0, 0, 1, 1], [0, 1, 0, 1]) == rand_score([0, 0, 1, 1], [0, 1, 0, 1])
    with pytest.raises(ValueError):
        tl.rand_index([0, 1], [0, 1, 2])


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def _rc(n=4, indptr=(0, 2, 3, 5, 6), indices=(1, 2, 0, 0, 3, 2), weights=(1, 2, 1, 2, 1, 1), resolution=1.0, tol=1e-3, max_levels=32,
        null=None):
    L = _lib.load()
    ip, ix, w = np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int32), np.array(weights, dtype=np.float64)
    labels, q, info = np.full(16, -7, dtype=np.int32), ctypes.c_double(-7.0), np.full(4, -7, dtype=np.int32)
    p = dict(indptr=_lib.lptr(ip), indices=_lib.iptr(ix), weights=_lib.dptr(w), labels=_lib.iptr(labels), modularity=ctypes.byref(q),
             info=_lib.iptr(info))
    if null:
        p[null] = None
    rc = L.pilot_ot_leiden(n, p["indptr"], p["indices"], p["weights"], resolution, tol, max_levels, p["labels"], p["modularity"], p["info"])
    return rc, L.pilot_ot_last_error(), labels, q.value, info


@pytest.mark.parametrize("bad,code,fragment", [
    (dict(null="indptr"), _lib.EINVAL, b"NULL"), (dict(null="labels"), _lib.EINVAL, b"NULL"), (dict(null="info"), _lib.EINVAL, b"NULL"),
    (dict(n=-1), _lib.EINVAL, b"n=-1"), (dict(indptr=(0, 2, 1, 5, 6)), _lib.EINVAL, b"indptr[2]"),
    (dict(indices=(1, 4, 0, 0, 3, 2)), _lib.EINVAL, b"indices[1]"), (dict(weights=(1, 2, -1, 2, 1, 1)), _lib.EINVAL, b"weights[2]"),
    (dict(resolution=-0.5), _lib.EINVAL, b"resolution"), (dict(tol=float("nan")), _lib.EINVAL, b"tol"),
    (dict(max_levels=0), _lib.EINVAL, b"max_levels"), (dict(n=2 ** 31), _lib.ENOTSUP, b"32-bit"),
    (dict(weights=(1e200, 2, 1, 2, 1, 1)), _lib.EINVAL, b"overflows"),
])
def test_leiden_refuses_before_any_hip_call(bad, code, fragment):
    rc, msg, labels, q, info = _rc(**bad)
    assert rc == code and fragment in msg, (bad, rc, msg)
    assert (labels == -7).all()


def test_leiden_abi_without_weight_needs_no_device():
    rc, msg, labels, q, info = _rc(n=0, indptr=(0,), indices=(), weights=())
    assert rc == _lib.OK and q == 0.0 and info.tolist() == [0, 0, 0, 0] and (labels == -7).all(), msg
    rc, msg, labels, q, info = _rc(n=5, indptr=(0, 1, 1, 2, 2, 2), indices=(1, 4), weights=(0, 0))
    assert rc == _lib.OK and q == 0.0 and info.tolist() == [0, 0, 0, 5] and labels[:5].tolist() == [0, 1, 2, 3, 4], msg
    try:
        _lib.test_switch("PILOT_OT_LOUVAIN_MAX_NNZ", "5")
        rc, msg, _, _, _ = _rc()
        assert rc == _lib.ENOTSUP and b"32-bit edge indices" in msg
    finally:
        _lib.test_switch("PILOT_OT_LOUVAIN_MAX_NNZ", None)
    rc, msg, _, _, _ = _rc()
    assert rc == (_lib.OK if _lib.device_count() > 0 else _lib.EHIP), msg
    assert "pilot_ot_leiden" in _lib.SYMBOLS


# ---- engine and tl ----------------------------------------------------------------------------------------------------------------
G4 = sp.csr_matrix(np.array([[0, 1, 2, 0], [1, 0, 0, 0], [2, 0, 0, 1], [0, 0, 1, 0]], dtype=np.float64))


@pytest.mark.parametrize("kw", [
    dict(graph=np.ones((3, 4))), dict(graph=np.ones(4)), dict(graph=None), dict(graph=-G4), dict(graph=G4 * np.nan),
    dict(resolution=-1), dict(resolution=np.nan), dict(resolution="1"), dict(resolution=True),
    dict(tol=-1e-3), dict(tol=None), dict(max_levels=0), dict(max_levels=2.0),
])
def test_engine_leiden_argument_errors(no_library, kw):
    with pytest.raises(ValueError):
        engine.leiden(**{**dict(graph=G4), **kw})


def test_engine_leiden_reaches_the_library_last(no_library):
    for graph in (G4, G4.tocoo(), G4.toarray(), sp.csr_matrix((0, 0))):
        with pytest.raises(AssertionError, match="touched"):
            engine.leiden(graph, resolution=0.5, tol=0, max_levels=3, return_info=True)


class _Adata:
    def __init__(self, graph):
        self.obs = pd.DataFrame({"a": ["x"] * graph.shape[0]})
        self.uns = {"neighbors": {"connectivities_key": "connectivities", "distances_key": "distances", "params": {}}}
        self.obsp = {"connectivities": graph, "distances": graph}


def test_tl_leiden(no_library, monkeypatch):
    ad = _Adata(G4)
    with pytest.raises(ValueError, match="tl.neighbors"):
        tl.leiden(ad, neighbors_key="other")
    for kw in (dict(mode="both"), dict(resolution=-1.0)):
        with pytest.raises(ValueError):
            tl.leiden(ad, **kw)
    with pytest.raises(AssertionError, match="touched"):
        tl.leiden(ad)
    assert list(ad.obs.columns) == ["a"] and set(ad.uns) == {"neighbors"}

    def restated(graph, resolution=1.0, tol=1e-3, max_levels=32, return_info=False):
        labels, q, (levels, ms, rs, k) = LD.leiden(graph, resolution, tol, max_levels)
        return labels, {"modularity": q, "levels": levels, "move_sweeps": ms, "refine_sweeps": rs, "communities": k}

    monkeypatch.setattr(engine, "leiden", restated)
    ring = LG.ring_of_cliques()
    ad = _Adata(ring)
    assert tl.leiden(ad) is None
    col = ad.obs["leiden"]
    assert isinstance(col.dtype, pd.CategoricalDtype) and list(col.cat.categories) == [str(c) for c in range(8)]
    assert col.astype(str).tolist() == [str(i // 5) for i in range(40)]
    assert ad.uns["leiden"] == {"params": {"resolution": 1.0, "mode": "connectivities"}, "modularity": LR.modularity(ring, np.arange(40) // 5)}


def test_method_is_checked_before_device_work(no_library):
    for bad in ("nope", None, "Leiden", 1):
        with pytest.raises(ValueError, match="method"):
            tl.select_best_sil(C.emd_adata("three_groups"), method=bad)
        with pytest.raises(ValueError, match="method"):
            tl.clustering_emd(C.emd_adata("three_groups"), method=bad)
        with pytest.raises(ValueError, match="method"):
            tl.select_best_resolution(_Adata(G4), method=bad)
    for method in ("louvain", "leiden"):
        with pytest.raises(AssertionError, match="touched"):
            tl.select_best_sil(C.emd_adata("three_groups"), method=method)
        with pytest.raises(AssertionError, match="touched"):
            tl.clustering_emd(C.emd_adata("three_groups"), method=method)


def _annot(group, names=("ctrl", "mild", "severe")):
    """two cells a sample, the columns where the reference expects them: cell_type, sampleID, status"""
    sample = np.repeat(np.arange(len(group)), 2)
    return pd.DataFrame({"cell_type": "T", "sampleID": ["s%02d" % s for s in sample], "status": [names[group[s]] for s in sample]})


def test_clustering_refusals(no_library):
    _, group, E = C.cohort("three_groups")
    df = _annot(group)
    for kw in (dict(EMD=E[:, :50]), dict(EMD=E[0]), dict(EMD=E[:14, :14], df=_annot(group[:14])), dict(EMD=E[:40, :40]),
               dict(category="stage"), dict(sample_col=7), dict(sample_col="sampleID"), dict(res=-0.1), dict(res=np.nan), dict(metric="l1"),
               dict(steper=0), dict(steper=-0.01), dict(steper=np.nan), dict(max_steps=0), dict(max_steps=2.5)):
        with pytest.raises(ValueError):
            tl.leiden_clustering(**{**dict(EMD=E, df=df), **kw})
    with pytest.raises(AssertionError, match="touched"):
        tl.leiden_clustering(E, df)
    for uns in ({}, {"EMD": np.array(E)}, {"EMD": np.array(E[:14, :14]), "annot": _annot(group[:14])}):
        with pytest.raises(ValueError):
            tl.sil_ari(C.Adata(uns=uns))
    with pytest.raises(ValueError):
        tl.sil_ari(C.Adata(uns={"EMD": np.array(E), "annot": df}), metric="l1")


def test_clustering_loop_is_the_references_with_an_end(monkeypatch):
    """the loop against a stand-in for engine.leiden whose cluster count is a function of the resolution: res += steper while there
    are too few clusters, res -= 0.001 while too many, stop at equality; a count that jumps over the target oscillates, and that
    ends in a ValueError naming the last two (resolution, clusters)"""
    _, group, E = C.cohort("three_groups")
    df = _annot(group)
    monkeypatch.setattr(tl, "_emd_graph", lambda E, metric: "graph")
    calls = []

    def stand_in(count):
        def leiden(graph, resolution=1.0, return_info=False):
            assert graph == "graph" and return_info
            calls.append(resolution)
            k = count(resolution)
            return (np.arange(60) % k).astype(np.int32), {"communities": k, "modularity": 0.0}
        return leiden

    monkeypatch.setattr(engine, "leiden", stand_in(lambda r: 1 if r < 0.0295 else (5 if r > 0.0305 else 3)))
    labels, score, true = tl.leiden_clustering(E, df, res=0.01, steper=0.0125)
    assert np.allclose(calls, [0.01, 0.0225, 0.035, 0.034, 0.033, 0.032, 0.031, 0.030]) and labels.dtype == int
    assert labels.tolist() == (np.arange(60) % 3).tolist() and true == ["ctrl mild severe".split()[g] for g in group]
    assert score == rand_score(true, labels)
    del calls[:]
    monkeypatch.setattr(engine, "leiden", stand_in(lambda r: 2 if r < 0.0155 else 4))
    with pytest.raises(ValueError, match="3 clusters in 50 steps") as err:
        tl.leiden_clustering(E, df, max_steps=50)
    assert len(calls) == 50 and {2, 4} == {2 if r < 0.0155 else 4 for r in calls[10:]}              # it went on oscillating
    assert "resolution %g with 4 clusters and %g with 4" % (calls[-2], calls[-1]) in str(err.value)
    monkeypatch.setattr(engine, "leiden", stand_in(lambda r: 7))
    with pytest.raises(ValueError, match="fell"):
        tl.leiden_clustering(E, df, res=0.0025)
