"""K18 on the device: engine.silhouette_samples (silhouette_kernels.hpp on K16's sweep) and the tl functions on top of it, against
tests/silhouette_restatement.py, which takes the float64 direct-difference distance matrix of exactly the uploaded values (for
cosine: of the rows normalised in float64 and rounded to the element type, as the kernel forms them) and computes a, b, s by the
definition.

The accuracy contract.  u = 2^-24 (float32) or 2^-53 (float64).  K16's contract gives every distance a relative
error <= (D + 6) u; a float64 mean of at most C non-negative terms adds <= C 2^-53; with eps their sum, s = 1 - a / b or b / a - 1
moves by at most 2 eps (the minimum over the clusters and the max() are continuous), and with K16's factor 2 of slack
|s_i - s_ref,i| <= 4 ((D + 6) u + C 2^-53), absolute, on every point and on the mean.  Nothing is skipped or exempted.  Conditions on
the inputs -- where the cluster boundaries fall in the kernel's tiles above all -- are asserted before the device is looked at.

Shapes: the smallest at which each path of the kernel is taken -- 16 x 3; D = 1 and one row past a wave (65 x 1); a partial last
query block and several corpus tiles (1100 x 50: a block holds 256 queries, a float32 tile of 50 dims 128 corpus rows); D past the 64
dims a query keeps in registers and one row past a block (257 x 130); D past what one staged tile holds (70 x 600: the dims pass
through LDS in groups)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import consumers_restatement as CR
import neighbors_restatement as NR
import silhouette_cohorts as C
import silhouette_restatement as SR
from pilot_amd import engine, tl

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
ROUTES = ["host", "device"]
SHAPES = {"tiny": (16, 3), "one_dim": (65, 1), "pilot": (1100, 50), "wide": (257, 130), "very_wide": (70, 600)}


@functools.lru_cache(maxsize=None)
def _cloud(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "off_centre":
        X = 4096.0 + rng.normal(size=(1100, 50))
    elif name == "scaled":
        X = _cloud("pilot") * 10.0 ** rng.choice([-3.0, 3.0], size=(1100, 1))
    elif name == "blobs":
        X = rng.normal(size=(600, 10)) + 8.0 * rng.normal(size=(6, 10))[rng.integers(0, 6, 600)]
    else:
        X = rng.normal(size=SHAPES[name])
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _uploaded(name, dtype):
    X = np.ascontiguousarray(_cloud(name).astype(dtype))
    X.setflags(write=False)
    return X


def _arg(X, route):
    return engine.DeviceMatrix.upload(X) if route == "device" else X


@functools.lru_cache(maxsize=None)
def _labels(kind, n, tile=0):
    """labellings by name.  The kernel orders the rows by (label, row), so the sizes of the clusters in label order place the
    boundaries in its corpus; the rows themselves carry the labels in shuffled order."""
    rng = np.random.default_rng(n + sum(map(ord, kind)))
    if kind == "halves":
        sizes = [n // 2, n - n // 2]
    elif kind == "thirds":
        sizes = [n // 3, n // 3, n - 2 * (n // 3)]
    elif kind == "pair_and_singletons":                            # k = n - 1
        sizes = [2] + [1] * (n - 2)
    elif kind == "pairs":
        sizes = [2] * (n // 2)
    else:                                                          # "mixed": see test_cases
        sizes = [tile, 1, 2, 2 * tile + 5]
        sizes.append(n - sum(sizes))
    assert sum(sizes) == n and min(sizes) >= 1
    labels = np.repeat(np.arange(len(sizes)), sizes)[rng.permutation(n)]
    labels.setflags(write=False)
    return labels


@functools.lru_cache(maxsize=None)
def _reference(name, dtype, metric, kind, tile=0):
    """(s, its mean) of the restatement for the uploaded values, computed once and left unchanged"""
    X = _uploaded(name, dtype)
    s = SR.samples(_full(name, dtype, metric), _labels(kind, X.shape[0], tile))
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _full(name, dtype, metric):
    full = NR.distance_rows(_uploaded(name, dtype), metric)
    full.setflags(write=False)
    return full


def _check(got, want, D, dtype, what):
    s, score = got
    n = want.size
    tol = SR.bound(D, n, dtype)
    assert s.shape == (n,) and s.dtype == np.float64 and isinstance(score, float)
    worst, mean_err = float(np.abs(s - want).max()), abs(score - float(want.mean()))
    print("%s: max |s - s_ref| = %.2e, mean %.2e (bound %.2e)" % (what, worst, mean_err, tol))
    assert np.isfinite(s).all() and worst <= tol and mean_err <= tol, what


# ---- the kernel cases -------------------------------------------------------------------------------------------------------------
CASES = [("tiny", "halves"), ("tiny", "pair_and_singletons"), ("one_dim", "thirds"), ("pilot", "mixed"), ("pilot", "pairs"),
         ("pilot", "pair_and_singletons"), ("wide", "thirds"), ("very_wide", "thirds")]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,kind", CASES)
def test_cases(name, kind, dtype, route):
    X = _uploaded(name, dtype)
    n, D = X.shape
    block, tile = engine.silhouette_geometry(D, dtype)
    labels = _labels(kind, n, tile)
    sizes = np.bincount(labels)
    ends = np.cumsum(sizes)
    assert block == 256 and tile % 16 == 0
    if name == "tiny":
        assert n == 16 and (list(sizes) == [8, 8] if kind == "halves" else len(sizes) == n - 1 and sizes[0] == 2)
    if name == "one_dim":
        assert D == 1 and n == 64 + 1 and len(sizes) == 3
    if name == "pilot":
        assert n % block != 0 and n > 4 * block and n > 8 * tile          # a partial last query block, several corpus tiles
        if kind == "mixed":
            assert ends[0] % tile == 0                                     # a boundary exactly on a tile edge
            assert ends[1] % tile != 0 and ends[2] // tile == ends[1] // tile   # boundaries inside a tile
            assert sizes[1] == 1 and sizes[2] == 2                         # a singleton and a pair
            assert sizes[3] > 2 * tile and ends[3] // tile - ends[2] // tile >= 2   # a cluster longer than one tile
        if kind == "pairs":
            assert len(sizes) == 550 and (sizes == 2).all()
        if kind == "pair_and_singletons":
            assert len(sizes) == 1099
    if name == "wide":
        assert D > 64 and n == block + 1
    if name == "very_wide":
        assert tile == 16 and 16 * ((D + 15) // 16 * 16) * np.dtype(dtype).itemsize > 32 * 1024     # the dims pass in groups
    want = _reference(name, dtype, "euclidean", kind, tile if kind == "mixed" else 0)
    assert (want[sizes[labels] == 1] == 0.0).all()
    got = engine.silhouette_samples(_arg(X, route), labels, return_score=True)
    _check(got, want, D, dtype, "%s %s %s %s" % (name, kind, np.dtype(dtype).name, route))
    assert (got[0][sizes[labels] == 1] == 0.0).all()                       # singletons: exactly 0


@pytest.mark.parametrize("route", ROUTES)
def test_off_centre(route):
    """every coordinate 4096 + N(0, 1), float32: |x|^2 is 1e5 times a squared distance, so |x|^2 + |y|^2 - 2 x.y rounded in float32
    misses the distances by far more than the bound allows; the direct differences do not"""
    X = _uploaded("off_centre", np.float32)
    n, D = X.shape
    full = _full("off_centre", np.float32, "euclidean")
    labels = _labels("thirds", n)
    sq = (X * X).sum(axis=1, dtype=np.float32)
    expansion = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - np.float32(2.0) * (X @ X.T), 0)).astype(np.float64)
    np.fill_diagonal(expansion, 0.0)
    miss = np.abs(SR.samples(expansion, labels) - SR.samples(full, labels)).max()
    print("off_centre: the float32 expansion misses s by %.2e (bound %.2e)" % (miss, SR.bound(D, n, np.float32)))
    assert miss > 10 * SR.bound(D, n, np.float32)
    got = engine.silhouette_samples(_arg(X, route), labels, return_score=True)
    _check(got, _reference("off_centre", np.float32, "euclidean", "thirds"), D, np.float32, "off_centre %s" % route)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cosine(dtype, route):
    n, D = SHAPES["pilot"]
    tile = engine.silhouette_geometry(D, dtype)[1]
    labels = _labels("mixed", n, tile)
    got = {}
    for name in ("pilot", "scaled"):
        X = _uploaded(name, dtype)
        got[name] = engine.silhouette_samples(_arg(X, route), labels, metric="cosine", return_score=True)
        _check(got[name], _reference(name, dtype, "cosine", "mixed", tile), D, dtype, "cosine %s %s %s" % (name, np.dtype(dtype).name, route))
    norms = np.linalg.norm(_uploaded("scaled", dtype).astype(np.float64), axis=1) \
        / np.linalg.norm(_uploaded("pilot", dtype).astype(np.float64), axis=1)
    assert norms.max() / norms.min() >= 1e5
    tol = SR.bound(D, n, dtype)
    move = float(np.abs(got["scaled"][0] - got["pilot"][0]).max())
    print("cosine %s: rows scaled by 10^+-3 move s by %.2e (bound %.2e)" % (np.dtype(dtype).name, move, tol))
    assert move <= tol and abs(got["scaled"][1] - got["pilot"][1]) <= tol


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_values(dtype, route):
    rng = np.random.default_rng(5)
    X = rng.normal(size=(300, 8)).astype(dtype)
    labels = rng.integers(0, 3, 300)
    X[[7, 150, 299]] = X[7]                                        # a cluster made only of copies of one point: a = 0 < b
    labels[[7, 150, 299]] = 3
    X[60] = X[61]                                                  # a copy in ANOTHER cluster counts at distance 0, it is not left out
    labels[60], labels[61] = 0, 1
    labels[200] = 4                                                # a singleton
    want, full = SR.of_points(X, labels)
    assert (want[[7, 150, 299]] == 1.0).all() and want[200] == 0.0 and full[60, 61] == 0.0
    s = engine.silhouette_samples(_arg(X, route), labels)
    assert (s[[7, 150, 299]] == 1.0).all() and s[200] == 0.0
    assert np.abs(s - want).max() <= SR.bound(8, 300, dtype)
    same = np.ones((40, 5), dtype=dtype) * dtype(1.25)             # identical points in two clusters: a = b = 0
    for metric in ("euclidean", "cosine"):
        s, score = engine.silhouette_samples(_arg(same, route), np.arange(40) % 2, metric=metric, return_score=True)
        assert (s == 0.0).all() and score == 0.0


# ---- labels, views, bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_string_labels_and_row_order(dtype, route):
    """labels of another type in shuffled order; permuting rows and labels together permutes s, within the bound (a cluster's
    members are then added in another order)"""
    X = _uploaded("pilot", dtype)
    n, D = X.shape
    tile = engine.silhouette_geometry(D, dtype)[1]
    ints = _labels("mixed", n, tile)
    names = np.array(["delta", "alpha", "echo", "bravo", "charlie"])[ints]      # sorted, the names number the clusters differently
    want = _reference("pilot", dtype, "euclidean", "mixed", tile)
    s = engine.silhouette_samples(_arg(X, route), names)
    assert np.abs(s - want).max() <= SR.bound(D, n, dtype)
    assert np.array_equal(engine.silhouette_samples(_arg(X, route), list(names)), s)
    perm = np.random.default_rng(9).permutation(n)
    moved = engine.silhouette_samples(_arg(np.ascontiguousarray(X[perm]), route), names[perm])
    print("rows permuted %s: s moves by %.2e" % (np.dtype(dtype).name, float(np.abs(moved - s[perm]).max())))
    assert np.abs(moved - s[perm]).max() <= SR.bound(D, n, dtype) and np.abs(moved - want[perm]).max() <= SR.bound(D, n, dtype)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_window_repeat_and_routes(dtype, metric):
    X = _uploaded("pilot", dtype)
    labels = _labels("mixed", 1100, engine.silhouette_geometry(30, dtype)[1])
    window = X[:, 10:40]                                           # a strided column window of a wider array, taken as it is
    assert not window.flags.c_contiguous and window.strides[1] == X.itemsize
    a = engine.silhouette_samples(window, labels, metric=metric, return_score=True)
    packed = np.ascontiguousarray(window)
    _check(a, SR.of_points(packed, labels, metric)[0], 30, dtype, "window %s %s" % (metric, np.dtype(dtype).name))
    for other in (engine.silhouette_samples(window, labels, metric=metric, return_score=True),               # a repeated call
                  engine.silhouette_samples(packed, labels, metric=metric, return_score=True),
                  engine.silhouette_samples(engine.DeviceMatrix.upload(packed), labels, metric=metric, return_score=True)):
        assert np.array_equal(a[0].view(np.uint64), other[0].view(np.uint64)) and a[1] == other[1]           # identical bits
    assert np.array_equal(X, _uploaded("pilot", dtype))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_refused(route):
    labels = _labels("thirds", 1100)
    for bad in (np.nan, np.inf, -np.inf):
        X = np.array(_uploaded("pilot", np.float32))
        X[7, 31] = bad
        X[900, 2] = bad
        for metric in ("euclidean", "cosine"):
            with pytest.raises(ValueError, match="row 7 "):
                engine.silhouette_samples(_arg(X, route), labels, metric=metric)
    X = np.array(_uploaded("pilot", np.float64))
    X[11] = 0.0
    X[640] = 0.0
    with pytest.raises(ValueError, match="row 11 "):
        engine.silhouette_samples(_arg(X, route), labels, metric="cosine")
    s = engine.silhouette_samples(_arg(X, route), labels)          # a zero row is an ordinary point of the euclidean metric
    assert np.abs(s - SR.of_points(X, labels)[0]).max() <= SR.bound(50, 1100, np.float64)


# ---- the old and the new kernel ---------------------------------------------------------------------------------------------------
def test_agrees_with_silhouette_of_rows():
    """the rows of a 60 x 60 EMD-like matrix as points: K18 against the matrix path (row distances then silhouette, K7), each within
    its own bound of the exact value -- K18's, and the one tests/test_gpu_consumers_sizes.py holds the Euclidean chain to"""
    _, group, E = C.cohort("three_groups")
    N = E.shape[0]
    new = engine.silhouette_samples(E, group, "euclidean", return_score=True)
    old = engine.silhouette_of_rows(E, group, "euclidean", return_samples=True)
    tol = SR.bound(N, N, np.float64) + CR.silhouette_bound(N) + 3 * 2 * CR.euclid_bound(N)
    worst = float(np.abs(new[0] - old[1]).max())
    print("K18 - K7 on 60 x 60: %.2e, means %.2e (bound %.2e)" % (worst, abs(new[1] - old[0]), tol))
    assert worst <= tol and abs(new[1] - old[0]) <= tol


# ---- the sweeps -----------------------------------------------------------------------------------------------------------------
def test_select_best_sil_and_clustering_emd():
    _, group, E = C.cohort("three_groups")
    ad = C.emd_adata("three_groups")
    frame = tl.select_best_sil(ad)
    assert list(frame.columns) == ["resolution", "silhouette", "n_clusters", "modularity"]
    assert list(frame["resolution"]) == C.REFERENCE_RESOLUTIONS and len(frame) == 19
    idx, dist = engine.knn(E, 14, metric="cosine")
    graph = engine.knn_connectivities(idx, dist, 15)
    for row in frame.itertuples():
        labels, info = engine.louvain(graph, resolution=row.resolution, return_info=True)
        assert row.n_clusters == info["communities"] == len(np.unique(labels)) and row.modularity == info["modularity"]
        assert row.silhouette == engine.silhouette_of_rows(E, labels, metric="cosine")          # bit for bit
    assert ad.uns["best_res"] == C.best_by_rule(frame["resolution"], frame["silhouette"], 0.2)
    assert ad.uns["best_res"] == 0.2
    assert np.array_equal(ad.uns["EMD"], E)

    df = tl.clustering_emd(ad, res=ad.uns["best_res"])
    assert C.same_partition(df["Predicted_Labels"], group) and set(df["Predicted_Labels"]) == {"0", "1", "2"}
    assert all(isinstance(v, str) for v in df["Predicted_Labels"])
    assert np.array_equal(df["Predicted_Labels"].astype(int), engine.louvain(graph, resolution=0.2))
    assert list(df.columns) == ["T", "B", "NK", "Mono", "Predicted_Labels", "sampleID"]
    assert list(df["sampleID"]) == list(ad.uns["proportions"].keys()) == list(df.index)
    assert np.array_equal(df[C.CELL_TYPES].to_numpy(), np.stack(list(ad.uns["proportions"].values())))
    assert ad.uns["clustering_emd"]["silhouette"] == engine.silhouette_of_rows(E, engine.louvain(graph, resolution=0.2), metric="cosine",
                                                                                normalize_by_max=True)


def test_one_cluster_scores_nan_and_is_not_chosen():
    _, _, E = C.cohort("one_blob")
    (labels, sil, k, _), = C.cpu_sweep(E, "cosine", [0.05])       # on the restatement: one cluster at this resolution
    assert k == 1 and np.isnan(sil)
    ad = C.emd_adata("one_blob")
    frame = tl.select_best_sil(ad, resolutions=[0.05, 0.2])
    assert frame["n_clusters"][0] == 1 and np.isnan(frame["silhouette"][0])
    assert frame["n_clusters"][1] >= 2 and frame["silhouette"][1] > 0 and ad.uns["best_res"] == 0.2
    frame = tl.select_best_sil(ad, resolutions=[0.05])
    assert np.isnan(frame["silhouette"]).all() and ad.uns["best_res"] == 0.2                    # the reference's initial value, start
    df = tl.clustering_emd(ad, res=0.05)
    assert set(df["Predicted_Labels"]) == {"0"} and np.isnan(ad.uns["clustering_emd"]["silhouette"])


def test_select_best_resolution_and_tl_silhouette():
    X = _uploaded("blobs", np.float32)
    ad = C.Adata(obsm={"X_pca": X})
    tl.neighbors(ad, n_pcs=8)
    frame = tl.select_best_resolution(ad, n_pcs=8)
    assert list(frame.columns) == ["resolution", "silhouette", "n_clusters", "modularity"]
    assert list(frame["resolution"]) == C.REFERENCE_RESOLUTIONS
    graph = ad.obsp["connectivities"]
    assert sp.isspmatrix_csr(graph) and graph.shape == (600, 600)
    packed = np.ascontiguousarray(X[:, :8])
    for row in frame.itertuples():
        labels, info = engine.louvain(graph, resolution=row.resolution, return_info=True)
        assert row.n_clusters == info["communities"] and row.modularity == info["modularity"] and 2 <= row.n_clusters <= 599
        assert row.silhouette == engine.silhouette_samples(packed, labels, return_score=True)[1]             # bit for bit
    assert ad.uns["best_res"] == C.best_by_rule(frame["resolution"], frame["silhouette"], 0.2)
    assert "louvain" not in ad.obs and set(ad.obs.columns) == set()                              # it writes no labels

    tl.louvain(ad, resolution=ad.uns["best_res"])
    score = tl.silhouette(ad, n_pcs=8)
    best = frame["silhouette"][list(frame["resolution"]).index(ad.uns["best_res"])]
    assert ad.obs["louvain_silhouette"].dtype == np.float64 and score == best
    want = SR.of_points(packed, np.asarray(ad.obs["louvain"]))[0]
    assert np.abs(ad.obs["louvain_silhouette"].to_numpy() - want).max() <= SR.bound(8, 600, np.float32)
    assert abs(score - want.mean()) <= SR.bound(8, 600, np.float32)
    cos = tl.silhouette(ad, n_pcs=8, metric="cosine", key_added="cos")
    assert abs(cos - ad.obs["cos"].mean()) <= 600 * 2.0 ** -53 and not np.array_equal(ad.obs["cos"], ad.obs["louvain_silhouette"])
    assert np.array_equal(X, _uploaded("blobs", np.float32))
