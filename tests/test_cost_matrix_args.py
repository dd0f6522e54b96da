"""Argument checks of the host-buffer cost-matrix entry point (pilot_ot_cost_matrix_ex / engine.pdist_square): the size limit
is refused before any device staging, so these run on a box without a GPU."""
import numpy as np
import pytest

from pilot_amd import _lib, engine


@pytest.mark.parametrize("K,D", [(4097, 1), (2, 4097), (4097, 4097)])
def test_more_than_4096_centroids_or_dimensions_is_refused_before_staging(K, D):
    X = np.zeros((K, D))
    out = np.zeros((K, K)) if K * K <= 4 else np.empty((K, K))
    rc = _lib.load().pilot_ot_cost_matrix_ex(_lib.dptr(X), K, D, _lib.METRICS["cosine"], None, _lib.dptr(out))
    assert rc == _lib.ENOTSUP
    assert _lib.load().pilot_ot_last_error().decode() == "K=%d D=%d: at most 4096 centroids / dimensions" % (K, D)
    with pytest.raises(NotImplementedError, match="at most 4096"):
        engine.pdist_square(X, metric="euclidean")


def test_mahalanobis_above_4096_dimensions_is_refused_before_staging():
    X = np.zeros((2, 4097))
    out = np.zeros((2, 2))
    aux = np.zeros(1)
    rc = _lib.load().pilot_ot_cost_matrix_ex(_lib.dptr(X), 2, 4097, _lib.METRICS["mahalanobis"], _lib.dptr(aux), _lib.dptr(out))
    assert rc == _lib.ENOTSUP
