"""Louvain communities on the device (K17) against tests/louvain_restatement.py.

Exact cases: integer weights, resolution in {1, 0.5, 0.25}, tol = 0.  Every quantity of the rule is then an integer (or a multiple of
1/4) below 2^53 in float64, so no sum order or rounding can excuse a difference: the labels must equal the restatement's element
for element, under every setting of the degree bins.  Float weights: a planted partition, where the partition must be the
restatement's, and graphs without structure, where the modularity is held to the sequential reference's."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import louvain_graphs as LG
import louvain_restatement as LR
from pilot_amd import _lib, engine, tl

pytestmark = pytest.mark.gpu

GAMMAS = (1.0, 0.5, 0.25)
# the modularity the synchronous RESTATEMENT gives up against the sequential reference on LG.uniform_union_graph(), measured on the
# CPU (resolution: deficit; tol = 1e-3): Q 0.866019 against 0.868165, and 0.940116 against 0.949333.  The device is allowed twice the
# larger one, for near-ties it may break the other way; nothing here was taken from the device code.
SYNC_DEFICITS = {1.0: 0.0021464, 0.1: 0.0092173}
MARGIN = 2 * max(SYNC_DEFICITS.values())


def _check_exact(A, gamma, expect=None):
    assert LG.exact_enough(A)
    labels, info = engine.louvain(A, resolution=gamma, tol=0.0, return_info=True)
    ref, q, (levels, sweeps, k) = expect if expect is not None else LR.louvain(A, gamma, 0.0)
    assert labels.dtype == np.int32 and np.array_equal(labels, ref), (gamma, labels.tolist(), ref.tolist())
    assert (info["levels"], info["sweeps"], info["communities"]) == (levels, sweeps, k)
    assert abs(info["modularity"] - q) <= 1e-14 and abs(q - LR.modularity(A, ref, gamma)) <= 1e-13
    return labels


@pytest.mark.parametrize("gamma", GAMMAS)
def test_ring_of_cliques(gamma):
    labels = _check_exact(LG.ring_of_cliques(), gamma)
    if gamma == 1.0:
        assert labels.tolist() == (np.arange(40) // 5).tolist()


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("name", ["random_symmetric", "directed_knn_ranks", "hub"])
def test_exact_graphs(name, gamma):
    A = getattr(LG, name)()
    if name == "directed_knn_ranks":
        assert (A != A.T).nnz > 0
    if name == "hub":
        assert np.diff(A.indptr).max() >= 150                      # beyond the wave bin at level 0
    _check_exact(A, gamma)


@pytest.mark.parametrize("gamma", GAMMAS)
def test_odd_ends(gamma):
    """isolated nodes, a node whose only entry is a self-loop, repeated and unsorted columns, a stored zero; then no entry at all,
    and one node"""
    A, n = LG.odd_ends()
    labels = _check_exact(A, gamma)
    assert len({labels[2], labels[9], labels[5]}) == 3 and (labels == labels[5]).sum() == 1
    for dense in (A.toarray(), A.tocoo()):
        assert np.array_equal(engine.louvain(dense, resolution=gamma, tol=0.0), labels)
    empty, info = engine.louvain(sp.csr_matrix((5, 5)), resolution=gamma, return_info=True)
    assert empty.tolist() == [0, 1, 2, 3, 4] and info == {"modularity": 0.0, "levels": 0, "sweeps": 0, "communities": 5}
    for one in (sp.csr_matrix((1, 1)), sp.csr_matrix(np.array([[3.0]]))):
        labels1, info = engine.louvain(one, resolution=gamma, return_info=True)
        assert labels1.tolist() == [0] and info["communities"] == 1
    assert info["levels"] == 1 and info["sweeps"] == 1 and abs(info["modularity"] - (1.0 - gamma)) <= 1e-15
    assert engine.louvain(sp.csr_matrix((0, 0))).shape == (0,)


@pytest.mark.parametrize("name", ["random_symmetric", "hub"])
def test_every_degree_bin_gives_the_same_labels(name):
    """(wave limit, workgroup limit): all three move kernels on one small graph; the labels never change"""
    A = getattr(LG, name)()
    expect = {gamma: LR.louvain(A, gamma, 0.0) for gamma in GAMMAS}
    try:
        for bins in ("2,8", "2,100000", "100000,100000"):
            _lib.test_switch("PILOT_OT_LOUVAIN_BINS", bins)
            for gamma in GAMMAS:
                _check_exact(A, gamma, expect[gamma])
    finally:
        _lib.test_switch("PILOT_OT_LOUVAIN_BINS", None)


class _Adata:
    def __init__(self, X, n):
        self.X = X
        self.obs = pd.DataFrame({"cell": np.arange(n)})
        self.obsm, self.varm, self.uns, self.obsp = {}, {}, {}, {}
        self.var_names = ["g%d" % j for j in range(X.shape[1])] if X is not None else []


def test_planted_partition_through_tl():
    """1 500 points of 6 Gaussian blobs in 10-D at separation LG.BLOB_SEPARATION = 3.0, where the synchronous restatement and the
    sequential reference return the same partition (chosen on the CPU)"""
    X, planted = LG.blobs()
    ad = _Adata(None, 1500)
    ad.obsm["X_pca"] = X
    tl.neighbors(ad, n_neighbors=15)
    for mode in ("connectivities", "distances"):
        key = "louvain_" + mode
        assert tl.louvain(ad, mode=mode, key_added=key) is None
        col = ad.obs[key]
        k = len(col.cat.categories)
        assert isinstance(col.dtype, pd.CategoricalDtype) and list(col.cat.categories) == [str(c) for c in range(k)]
        labels = col.cat.codes.to_numpy()
        ref, q_ref, _ = LR.louvain(ad.obsp[mode])
        assert LG.same_partition(labels, ref) and LG.same_partition(labels, planted) and LG.numbered_by_size(labels)
        assert set(ad.uns[key]) == {"params", "modularity"} and ad.uns[key]["params"] == {"resolution": 1.0, "mode": mode}
        q = ad.uns[key]["modularity"]
        assert abs(q - LR.modularity(ad.obsp[mode], labels, 1.0)) <= 1e-12
        again, info = engine.louvain(ad.obsp[mode], return_info=True)
        assert np.array_equal(again, labels) and info["modularity"] == q                   # the same bits
        assert info["communities"] == k == 6


@pytest.fixture(scope="module")
def uniform_graph():
    return LG.uniform_union_graph()


@pytest.mark.parametrize("gamma", [1.0, 0.1])
def test_no_structure(uniform_graph, gamma):
    """the 14-NN union graph of 1 000 uniform 2-D points: a valid partition numbered by size, the reported Q the independent one, the
    same bits twice, and Q within MARGIN of the sequential reference's"""
    A = uniform_graph
    labels, info = engine.louvain(A, resolution=gamma, return_info=True)
    assert labels.shape == (1000,) and labels.dtype == np.int32 and LG.numbered_by_size(labels)
    assert info["communities"] == labels.max() + 1 and 1 <= info["levels"] <= 32 and info["sweeps"] <= 128 * info["levels"]
    q = info["modularity"]
    assert abs(q - LR.modularity(A, labels, gamma)) <= 1e-12
    again, info2 = engine.louvain(A, resolution=gamma, return_info=True)
    assert np.array_equal(again, labels) and info2 == info
    q_seq = LR.sequential_louvain(A, gamma)[1]
    print("gamma %g: Q_device %.6f Q_sequential %.6f margin %.6f" % (gamma, q, q_seq, MARGIN))
    assert q >= q_seq - MARGIN, (q, q_seq)


def test_reclustering_data():
    """both branches: the labels are engine.louvain of the graph tl.neighbors makes from the same representation"""
    rng = np.random.default_rng(12)
    X = rng.normal(size=(400, 30)) + 4.0 * rng.normal(size=(4, 30))[np.arange(400) % 4]
    for mode in ("distances", "connectivities"):
        ad = _Adata(None, 400)
        ad.obsm["X"] = X
        tl.neighbors(ad, use_rep="X")                              # scanpy's defaults: 15, euclidean
        want = engine.louvain(ad.obsp[mode], resolution=0.01)
        got = tl.reclustering_data(X, mode=mode)
        assert got.dtype == np.int32 and np.array_equal(got, want)
    assert LG.same_partition(got, np.arange(400) % 4)
    # an AnnData of sparse counts: tl.pca (normalised and scaled), 25 of its components, cosine neighbours
    rates = rng.gamma(2.0, 1.0, size=(3, 80)) * 3.0
    counts = sp.csr_matrix(rng.poisson(rates[np.arange(300) % 3]).astype(np.float32))
    ad = _Adata(counts, 300)
    got = tl.reclustering_data(ad, resu=0.5, normalization=True, n_neighbor=10, origine_scr_rna=True, dimension_rect=True, n_component=25)
    ref = _Adata(counts, 300)
    tl.pca(ref, n_comps=50, normalize=True, target_sum=1e6, scale=True, max_value=10)
    tl.neighbors(ref, n_neighbors=10, metric="cosine", n_pcs=25)
    assert np.array_equal(got, engine.louvain(ref.obsp["distances"], resolution=0.5))
    assert (counts != ad.X).nnz == 0 and ad.uns["neighbors"]["params"]["n_pcs"] == 25
    with pytest.raises(ValueError):
        tl.reclustering_data(X, method_="gauss")
