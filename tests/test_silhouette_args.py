"""The silhouette of labelled points (K18) and the resolution sweeps, the parts that need no device.  The C ABI refuses every argument
it can judge before any HIP call (a box without a device returns PILOT_OT_EHIP from the first HIP call, so PILOT_OT_EINVAL /
PILOT_OT_ENOTSUP show the check came first); engine.silhouette_samples, tl.silhouette, tl.select_best_resolution, tl.select_best_sil
and tl.clustering_emd raise before the library is touched (the library handle is replaced by an object that fails the test on any
use).  tests/silhouette_restatement.py is pinned to scikit-learn, and the sweeps are run with the engine calls replaced by the
restatements, which pins what tl composes: the resolution list, the best-resolution rule, the frame and proportion_df."""
import ctypes

import numpy as np
import pandas as pd
import pytest
from sklearn.metrics import silhouette_samples, silhouette_score

import louvain_restatement as LR
import neighbors_restatement as NR
import silhouette_cohorts as C
import silhouette_restatement as SR
from pilot_amd import _lib, engine, tl


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())


# ---- the restatement against scikit-learn --------------------------------------------------------------------------------------
def test_restatement_is_sklearns_precomputed_silhouette():
    rng = np.random.default_rng(300)
    X = rng.normal(size=(300, 5))
    labels = rng.integers(0, 4, 300)
    labels[17] = 4                                                 # a singleton
    X[[40, 41, 42]] = X[40]                                        # a cluster of three copies of one point
    labels[[40, 41, 42]] = 5
    s, Dref = SR.of_points(X, labels)
    want = silhouette_samples(Dref, labels, metric="precomputed")
    worst = float(np.abs(s - want).max())
    print("restatement - sklearn(precomputed): %.2e" % worst)
    assert worst <= 4 * 300 * 2.0 ** -53                           # both sides average the same float64 distances, in another order
    assert s[17] == 0.0 and (s[[40, 41, 42]] == 1.0).all()
    with pytest.raises(ValueError, match="Valid values are 2 to n_samples - 1"):
        SR.samples(Dref, np.zeros(300))
    with pytest.raises(ValueError, match="Valid values are 2 to n_samples - 1"):
        SR.samples(Dref, np.arange(300))


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def _points_rc(n=10, D=3, ld=None, dtype=1, metric=0, k=2, codes=None, null=None):
    L = _lib.load()
    X = np.ones((max(min(n, 100), 1), max(D, 1)))
    codes = np.ascontiguousarray((np.arange(max(min(n, 100), 1)) % max(k, 1)) if codes is None else codes, dtype=np.int32)
    samples, score = np.zeros(100), ctypes.c_double(0.0)
    p = dict(X=ctypes.c_void_p(X.ctypes.data), codes=_lib.iptr(codes), samples=_lib.dptr(samples), score=ctypes.byref(score))
    if null:
        p[null] = None
    rc = L.pilot_ot_silhouette_points(p["X"], 0, dtype, n, D, D if ld is None else ld, metric, p["codes"], k, p["samples"], p["score"])
    return rc, L.pilot_ot_last_error()


@pytest.mark.parametrize("bad,code,fragment", [
    (dict(null="X"), _lib.EINVAL, b"NULL"), (dict(null="codes"), _lib.EINVAL, b"NULL"), (dict(null="samples"), _lib.EINVAL, b"NULL"),
    (dict(null="score"), _lib.EINVAL, b"NULL"),
    (dict(D=0), _lib.EINVAL, b"D=0"), (dict(D=-1), _lib.EINVAL, b"D=-1"), (dict(ld=2), _lib.EINVAL, b"ld"),
    (dict(dtype=2), _lib.EINVAL, b"dtype"), (dict(metric=2), _lib.EINVAL, b"metric"), (dict(metric=-1), _lib.EINVAL, b"metric"),
    (dict(k=1), _lib.EINVAL, b"2 to n - 1"), (dict(k=10), _lib.EINVAL, b"2 to n - 1"), (dict(n=2, k=2), _lib.EINVAL, b"2 to n - 1"),
    (dict(n=2 ** 31, k=2), _lib.ENOTSUP, b"32-bit"),
    (dict(codes=[0, 1, 2, 0, 1, 2, 0, 1, 3, 0], k=3), _lib.EINVAL, b"codes[8]=3"),
    (dict(codes=[0, 1, 2, 0, 1, -1, 0, 1, 2, 0], k=3), _lib.EINVAL, b"codes[5]=-1"),
    (dict(codes=[0, 2, 2, 0, 0, 2, 0, 0, 2, 0], k=3), _lib.EINVAL, b"code 1 has no rows"),
])
def test_silhouette_points_refuses_before_any_hip_call(bad, code, fragment):
    rc, msg = _points_rc(**bad)
    assert rc == code and fragment in msg, (bad, rc, msg)


@pytest.mark.parametrize("D,dtype,tile", [(1, np.float32, 512), (50, np.float32, 128), (50, np.float64, 64), (64, np.float32, 128),
                                          (130, np.float32, 48), (130, np.float64, 16), (600, np.float32, 16), (600, np.float64, 16)])
def test_geometry(D, dtype, tile):
    """a block holds 256 queries; the 32 KiB tile holds as many sub-tiles of 16 rows as fit with the dims padded to 16, at least one"""
    item = np.dtype(dtype).itemsize
    assert tile == 16 * max(1, (32 * 1024 // item) // (16 * ((D + 15) // 16 * 16)))
    assert engine.silhouette_geometry(D, dtype) == (256, tile)
    with pytest.raises(ValueError, match="D=0"):
        engine.silhouette_geometry(0, dtype)
    with pytest.raises(ValueError, match="float32 or float64"):
        engine.silhouette_geometry(D, np.int32)


# ---- engine ---------------------------------------------------------------------------------------------------------------------
def test_engine_refuses_before_the_library(no_library):
    X = np.random.default_rng(0).normal(size=(12, 3))
    with pytest.raises(ValueError, match="Number of labels is 1. Valid values are 2 to n_samples - 1"):
        engine.silhouette_samples(X, np.zeros(12))                 # k = 1
    with pytest.raises(ValueError, match="Number of labels is 12. Valid values are 2 to n_samples - 1"):
        engine.silhouette_samples(X, np.arange(12))                # k = C
    with pytest.raises(ValueError, match="one label per sample"):
        engine.silhouette_samples(X, np.arange(11) % 2)
    with pytest.raises(ValueError, match="one label per sample"):
        engine.silhouette_samples(X, np.zeros((12, 2)))
    with pytest.raises(ValueError, match="metric='manhattan'"):
        engine.silhouette_samples(X, np.arange(12) % 2, metric="manhattan")
    with pytest.raises(ValueError, match="no columns"):
        engine.silhouette_samples(np.empty((12, 0)), np.arange(12) % 2)
    with pytest.raises(ValueError, match="2-D"):
        engine.silhouette_samples(np.zeros(12), np.arange(12) % 2)
    dev = engine.DeviceMatrix(0x1000, 12, shape=(12, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="Valid values are 2 to n_samples - 1"):
        engine.silhouette_samples(dev, ["a"] * 12)


# ---- tl: refusals ---------------------------------------------------------------------------------------------------------------
def test_tl_cell_level_refuses_before_the_library(no_library):
    X = np.random.default_rng(0).normal(size=(20, 4)).astype(np.float32)
    ad = C.Adata(obsm={"X_pca": X}, obs=pd.DataFrame({"louvain": ["0"] * 20}))
    with pytest.raises(ValueError, match="no 'X_umap'"):
        tl.silhouette(ad, use_rep="X_umap")
    with pytest.raises(ValueError, match="no 'leiden'"):
        tl.silhouette(ad, labels_key="leiden")
    with pytest.raises(ValueError, match="metric='l1'"):
        tl.silhouette(ad, metric="l1")
    with pytest.raises(ValueError, match="n_pcs=5"):
        tl.silhouette(ad, n_pcs=5)
    with pytest.raises(ValueError, match="Number of labels is 1"):
        tl.silhouette(ad)
    assert list(ad.obs.columns) == ["louvain"]
    with pytest.raises(ValueError, match="run tl.neighbors first"):
        tl.select_best_resolution(ad)                              # no uns['neighbors'], no obsp
    ad.uns["neighbors"] = {"connectivities_key": "connectivities", "distances_key": "distances"}
    ad.obsp = {}
    with pytest.raises(ValueError, match="run tl.neighbors first"):
        tl.select_best_resolution(ad)                              # the key is named, the matrix is missing
    with pytest.raises(ValueError, match="mode='weights'"):
        tl.select_best_resolution(ad, mode="weights")
    with pytest.raises(ValueError, match="metric='l1'"):
        tl.select_best_resolution(ad, metric="l1")
    ad.obsp = {"connectivities": None}
    with pytest.raises(ValueError, match="resolution=-0.5"):
        tl.select_best_resolution(ad, resolutions=[0.4, -0.5])     # judged before the graph is looked at
    assert "best_res" not in ad.uns


@pytest.mark.parametrize("call", [tl.select_best_sil, tl.clustering_emd])
def test_tl_sample_level_refuses_before_the_library(no_library, call):
    with pytest.raises(ValueError, match="no 'EMD'"):
        call(C.Adata())
    with pytest.raises(ValueError, match="14 samples"):
        call(C.emd_adata("three_groups", n=14))                    # N < 15
    with pytest.raises(ValueError, match="metric='l1'"):
        call(C.emd_adata("three_groups"), metric="l1")
    bad = dict(res=np.inf) if call is tl.clustering_emd else dict(resolutions=[0.2, np.inf])
    with pytest.raises(ValueError, match="resolution=inf"):
        call(C.emd_adata("three_groups"), **bad)
    ad = C.emd_adata("three_groups")
    ad.uns["EMD"] = ad.uns["EMD"][:, :30]
    with pytest.raises(ValueError, match="samples x samples"):
        call(ad)


def test_clustering_emd_refuses_before_the_library(no_library):
    for key in ("proportions", "annot"):
        ad = C.emd_adata("three_groups")
        del ad.uns[key]
        with pytest.raises(ValueError, match="no '%s'" % key):
            tl.clustering_emd(ad)
    with pytest.raises(ValueError, match="resolution=-1"):
        tl.clustering_emd(C.emd_adata("three_groups"), res=-1)
    ad = C.emd_adata("three_groups")
    ad.uns["proportions"].pop("s07")
    with pytest.raises(ValueError, match="59 samples x 4 cell types"):
        tl.clustering_emd(ad)


# ---- tl: the resolution list and the best-resolution rule ---------------------------------------------------------------------
def test_resolution_list_is_the_references_expression():
    got = tl._resolution_list(None, 0.2, 0.1, 2)
    assert got == C.REFERENCE_RESOLUTIONS and len(got) == 19 and got[0] == 0.2 and abs(got[-1] - 2.0) < 1e-12
    assert tl._resolution_list([], 0.2, 0.1, 2) == got             # the reference's default argument
    assert tl._resolution_list([0.5, 1], 0.2, 0.1, 2) == [0.5, 1.0]
    assert tl._resolution_list(None, 0.1, 0.25, 1) == [0.1 + 0.25 * i for i in range(int((1 - 0.1) / 0.25) + 1)]


@pytest.mark.parametrize("scores,want", [
    ([0.3, 0.5, 0.5, 0.4], 0.3), ([0.5, np.nan, 0.9, np.nan], 0.4), ([np.nan] * 4, 0.2), ([-0.2, -0.1, 0.0, -0.3], 0.2),
    ([np.nan, -0.1, 0.1, 0.1], 0.4)])
def test_best_resolution_rule(scores, want):
    res = [0.2, 0.3, 0.4, 0.5]
    assert tl._best_resolution(res, scores, 0.2) == want == C.best_by_rule(res, scores, 0.2)


# ---- tl: what the sweeps compose, with the engine replaced by the restatements -------------------------------------------------
@pytest.fixture
def cpu_engine(monkeypatch, no_library):
    monkeypatch.setattr(engine, "knn", lambda X, k, metric="euclidean", rows=None: NR.knn(X, k, metric)[:2])
    monkeypatch.setattr(engine, "knn_connectivities", NR.connectivities)

    def louvain(graph, resolution=1.0, tol=1e-3, max_levels=32, return_info=False):
        labels, q, (levels, sweeps, k) = LR.louvain(graph, resolution=resolution, tol=tol, max_levels=max_levels)
        return (labels, {"modularity": q, "levels": levels, "sweeps": sweeps, "communities": k}) if return_info else labels

    def silhouette_of_rows(E, labels, metric="cosine", normalize_by_max=False, return_samples=False):
        assert not return_samples
        return silhouette_score(E / E.max() if normalize_by_max else E, labels, metric=metric)

    def silhouette_points(X, labels, metric="euclidean", return_score=False):
        s = SR.of_points(np.asarray(X), labels, metric)[0]
        return (s, s.mean()) if return_score else s

    monkeypatch.setattr(engine, "louvain", louvain)
    monkeypatch.setattr(engine, "silhouette_of_rows", silhouette_of_rows)
    monkeypatch.setattr(engine, "silhouette_samples", silhouette_points)


def test_select_best_sil_and_clustering_emd_on_the_cpu(cpu_engine):
    _, group, E = C.cohort("three_groups")
    ad = C.emd_adata("three_groups")
    frame = tl.select_best_sil(ad)
    want = C.cpu_sweep(E, "cosine", C.REFERENCE_RESOLUTIONS)
    assert list(frame.columns) == ["resolution", "silhouette", "n_clusters", "modularity"]
    assert list(frame["resolution"]) == C.REFERENCE_RESOLUTIONS
    assert list(frame["n_clusters"]) == [w[2] for w in want] and list(frame["silhouette"]) == [w[1] for w in want]
    assert list(frame["modularity"]) == [w[3] for w in want]
    # the cohort: resolutions 0.2 - 0.9 return exactly the three groups, the later ones split them
    assert all(C.same_partition(w[0], group) for w in want[:8]) and [w[2] for w in want[:8]] == [3] * 8
    assert all(4 <= w[2] <= 7 and w[1] < 0.8 for w in want[8:]) and abs(want[0][1] - 0.990) < 1e-3
    assert ad.uns["best_res"] == 0.2 == C.best_by_rule(frame["resolution"], frame["silhouette"], 0.2)
    assert np.array_equal(ad.uns["EMD"], E)

    df = tl.clustering_emd(ad, res=ad.uns["best_res"])
    assert list(df.columns) == ["T", "B", "NK", "Mono", "Predicted_Labels", "sampleID"]
    assert list(df.index) == list(df["sampleID"]) == list(ad.uns["proportions"].keys())
    assert np.array_equal(df[C.CELL_TYPES].to_numpy(), np.stack(list(ad.uns["proportions"].values())))
    assert all(isinstance(v, str) for v in df["Predicted_Labels"]) and set(df["Predicted_Labels"]) == {"0", "1", "2"}
    assert C.same_partition(df["Predicted_Labels"], group)
    assert ad.uns["clustering_emd"]["params"] == {"res": 0.2, "metric": "cosine"}
    assert ad.uns["clustering_emd"]["silhouette"] == C.cpu_sweep(E, "cosine", [0.2], normalize=True)[0][1]
    # the frame a later function takes its sub-groups from
    assert tl._sample_labels(df, "Predicted_Labels") == dict(zip(df["sampleID"], df["Predicted_Labels"]))


def test_a_single_cluster_scores_nan_and_is_never_best(cpu_engine):
    _, _, E = C.cohort("one_blob")
    (labels, sil, k, _), = C.cpu_sweep(E, "cosine", [0.05])
    assert k == 1 and np.isnan(sil) and (labels == 0).all()
    two = C.cpu_sweep(E, "cosine", [0.2])[0]
    assert two[2] == 2 and two[1] > 0
    ad = C.emd_adata("one_blob")
    frame = tl.select_best_sil(ad, resolutions=[0.05, 0.2, 0.01])
    assert list(frame["n_clusters"]) == [1, 2, 1] and np.isnan(frame["silhouette"][0]) and np.isnan(frame["silhouette"][2])
    assert frame["silhouette"][1] == two[1] and ad.uns["best_res"] == 0.2
    frame = tl.select_best_sil(ad, resolutions=[0.05, 0.01])      # nothing valid: the reference's initial value, start
    assert np.isnan(frame["silhouette"]).all() and ad.uns["best_res"] == 0.2
    df = tl.clustering_emd(ad, res=0.05)
    assert set(df["Predicted_Labels"]) == {"0"} and np.isnan(ad.uns["clustering_emd"]["silhouette"])


def test_select_best_resolution_and_silhouette_on_the_cpu(cpu_engine):
    points, group, _ = C.cohort("three_groups")
    X = np.ascontiguousarray(np.hstack([points, np.zeros((60, 1))]), dtype=np.float32)
    ad = C.Adata(obsm={"X_pca": X})
    tl.neighbors(ad, n_pcs=2)
    frame = tl.select_best_resolution(ad, resolutions=[0.3, 1.5], n_pcs=2)
    graph = ad.obsp["connectivities"]
    for row, res in zip(frame.itertuples(), [0.3, 1.5]):
        labels, q, (_, _, k) = LR.louvain(graph, resolution=res)
        assert (row.resolution, row.n_clusters, row.modularity) == (res, k, q)
        assert row.silhouette == SR.of_points(X[:, :2], labels)[0].mean()
    assert frame["n_clusters"][0] == 3 and ad.uns["best_res"] == 0.3 and set(ad.obs.columns) == set()
    ad.obs["louvain"] = pd.Categorical([str(g) for g in group])
    score = tl.silhouette(ad, n_pcs=2)
    assert ad.obs["louvain_silhouette"].dtype == np.float64 and score == ad.obs["louvain_silhouette"].mean()
    assert np.array_equal(ad.obs["louvain_silhouette"], SR.of_points(X[:, :2], group)[0])
    tl.silhouette(ad, n_pcs=2, key_added="sil", metric="cosine")
    assert np.array_equal(ad.obs["sil"], SR.of_points(X[:, :2], group, "cosine")[0])
