"""The CPU references the consumer-kernel GPU tests rely on (tests/consumers_restatement.py) are scikit-learn's and scipy's:
checked here without a GPU, on the inputs the GPU tests build."""
import numpy as np
import pytest
from scipy.spatial.distance import cdist
from sklearn.metrics import silhouette_samples
from sklearn.metrics.pairwise import cosine_distances
from sklearn.neighbors import NearestNeighbors

import consumers_restatement as R


@pytest.mark.parametrize("N,k", [(600, 1), (600, 64), (600, 599), (513, 2)])
def test_stable_argsort_selects_scikit_learns_neighbours(N, k):
    D = R.cloud_distances(N, seed=N)
    R.assert_tie_free(np.sort(D, axis=1), k, N)
    want = R.knn_kernel_reference(D, k, 0.3)
    nb = NearestNeighbors(n_neighbors=k, metric="precomputed").fit(D).kneighbors(D, return_distance=False)
    mask = np.zeros((N, N), dtype=bool)
    mask[np.arange(N)[:, None], nb] = True
    np.testing.assert_array_equal(want > 0, mask)
    assert ((want > 0).sum(1) == k).all() and (np.diag(want) == 1.0).all()


def test_tied_rows_follow_the_stated_rule():
    N = 200
    D = R.tied_distances(N, seed=1)
    below = np.flatnonzero(D[R.TIE_ROW] < 0.5)
    for extra, ties in ((3, [62, 63, 64]), (5, [62, 63, 64, 65, 190]), (7, [62, 63, 64, 65, 190, 191, 192])):
        want = R.knn_kernel_reference(D, R.N_BELOW + extra, 1.0)
        assert sorted(np.flatnonzero(want[R.TIE_ROW])) == sorted(list(below) + ties)
    want = R.knn_kernel_reference(D, 9, 1.0)
    assert list(np.flatnonzero(want[R.FLAT_ROW])) == [0, 1, 2, 3, 4, 5, 6, 7, R.FLAT_ROW]
    want = R.knn_kernel_reference(D, 1, 1.0)
    assert list(np.flatnonzero(want[40])) == [5] and list(np.flatnonzero(want[N - 3])) == [5]      # the lowest-index zero, not itself


@pytest.mark.parametrize("C,layout", [(2, "random"), (5, "blocks"), (257, "random")])
def test_bincount_restatement_is_scikit_learns_silhouette(C, layout):
    N = 600
    D = R.symmetric_distances(N, seed=C)
    labels = R.cluster_labels(N, C, seed=C, layout=layout)
    np.testing.assert_array_equal(R.silhouette_bincount(D, labels), silhouette_samples(D, labels, metric="precomputed"))
    # ids without members change nothing: the same labelling spread over a wider id range
    wide = np.where(labels >= 3, labels + 2, labels)
    np.testing.assert_array_equal(R.silhouette_bincount(D, wide, n_clusters=C + 4), R.silhouette_bincount(D, labels))


@pytest.mark.parametrize("N", [65, 600])
def test_scipy_and_scikit_learn_sit_inside_the_derived_bounds(N):
    """The bounds have room for an honest fp64 evaluation: scipy / scikit-learn against the long-double rows."""
    E = R.distance_like_matrix(N, seed=N, max_at="last")
    rows = R.probe_rows(N)
    want = R.row_distances_longdouble(E, rows, "euclidean")
    assert (np.abs(cdist(E[rows], E) - want) <= R.euclid_bound(N) * want).all()
    assert want[list(rows).index(3), N - 2] == 0
    want = R.row_distances_longdouble(E, rows, "cosine")
    assert np.abs(cosine_distances(E[rows], E) - want).max() <= R.cosine_bound(N)
