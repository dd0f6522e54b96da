"""Principal components restated in numpy, the plain way: the standardised matrix is formed densely in float64 and its centred copy
goes through ``np.linalg.svd``.  Independent of the device code -- no implicit operator, no Lanczos.

scanpy 1.9's ``pp.scale`` (ddof-1 standard deviation, 0 -> 1, ``np.clip``-free upper clip ``X[X > max_value] = max_value``), then
``tl.pca``: scikit-learn's centring, ``variance = s^2 / (n - 1)``, ``variance_ratio = variance / sum of the column variances`` and
scikit-learn 1.3's u-based ``svd_flip`` (the score of largest magnitude in every component is positive, lowest row on ties).
scanpy is not installed here: this file is the rule the device is held to."""
import numpy as np


def standardise(Y, scale=True, max_value=10.0):
    """the dense float64 Z of ``Y`` (rows x columns)"""
    Z = np.array(Y, dtype=np.float64)
    if not scale:
        return Z
    mean = Z.mean(axis=0)
    var = ((Z - mean) ** 2).sum(axis=0) / (Z.shape[0] - 1)
    std = np.sqrt(var)
    std[std == 0] = 1.0
    Z = (Z - mean) / std
    if max_value is not None:
        Z[Z > max_value] = max_value
    return Z


def pca(Y, n_comps, scale=True, max_value=10.0, cols=None):
    """(scores, pcs, variance, variance_ratio, all_variances): ``all_variances`` every eigenvalue / (n - 1), for the gap condition"""
    Y = np.asarray(Y)
    if cols is not None:
        Y = Y[:, np.asarray(cols)]
    Z = standardise(Y, scale, max_value)
    n = Z.shape[0]
    Zc = Z - Z.mean(axis=0)
    U, s, Vt = np.linalg.svd(Zc, full_matrices=False)
    at = np.argmax(np.abs(U), axis=0)                              # (argmax: the first of equal magnitudes)
    signs = np.sign(U[at, np.arange(U.shape[1])])
    signs[signs == 0] = 1.0
    U, Vt = U * signs, Vt * signs[:, None]
    all_var = s ** 2 / (n - 1)
    total = (Zc ** 2).sum(axis=0).sum() / (n - 1)
    k = n_comps
    return U[:, :k] * s[:k], Vt[:k].T.copy(), all_var[:k], all_var[:k] / total, all_var


def clipped(Y, max_value=10.0, cols=None):
    """entries the upper clip changes"""
    Y = np.asarray(Y)
    if cols is not None:
        Y = Y[:, np.asarray(cols)]
    return int((standardise(Y, True, None) > max_value).sum())
