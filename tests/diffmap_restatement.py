"""pydiffmap's diffusion map as pl.trajectory calls it (pilotpy/plot/ploting.py:109-110), restated in numpy / scipy.

``DiffusionMap.from_sklearn(n_evecs, epsilon, alpha, k).fit_transform(X)`` of pydiffmap 0.2.x with a numeric epsilon, no weight
function and no bandwidth normalisation; X = the rows of E / E.max().  Restated from memory of pydiffmap 0.2.0.1 (no copy of its
source in this project): the 'or' symmetrisation, the 4 epsilon of the kernel and the sqrt(-1 / lambda) scaling are UNPINNED
(``tools/pin_with_pydiffmap.py`` compares this module with the real package where it installs).

1. K: row i holds exp(-d_ij^2 / (4 epsilon)) on its k nearest rows (itself included; exactly k, ties in index order).
2. K <- 0.5 (K + K^T + |K - K^T|)                       (symmetrisation 'or')
3. q = K.sum(1); K_alpha = K diag(q^-alpha)
4. P = diag(1 / K_alpha.sum(1)) K_alpha; L = (P - I) / epsilon
5. eigs(L, k=n_evecs + 1, which='LR'), sorted descending, the first (lambda = 0) dropped, real parts
6. dmap = evecs diag(sqrt(-1 / evals))
"""
import numpy as np
import scipy.sparse as sps
from scipy.spatial.distance import cdist
from scipy.sparse.linalg import eigs


def knn_kernel(X, k, epsilon):
    """Step 1 on the rows of X (dense N x N result)."""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    D = cdist(X, X)
    k = min(int(k), N)
    K = np.zeros((N, N))
    for i in range(N):
        nb = np.argsort(D[i], kind="stable")[:k]
        K[i, nb] = np.exp(-D[i, nb] ** 2 / (4.0 * epsilon))
    return K


def markov_operator(K, alpha):
    """Steps 2-4 up to P (sparse CSR), and the symmetrised kernel."""
    K = sps.csr_matrix(np.asarray(K, dtype=np.float64))
    K = 0.5 * (K + K.T + abs(K - K.T))
    q = np.asarray(K.sum(1)).ravel()
    Ka = K @ sps.diags(q ** -alpha)
    r = np.asarray(Ka.sum(1)).ravel()
    P = sps.diags(1.0 / r) @ Ka
    return sps.csr_matrix(P), K


def diffusion_map_from_kernel(K, epsilon, alpha, n_evecs):
    """Steps 2-6 from a kernel matrix.  Returns (dmap, evecs, evals), evals = the eigenvalues of L (descending, first dropped)."""
    P, _ = markov_operator(K, alpha)
    N = P.shape[0]
    L = (P - sps.eye(N)) / epsilon
    evals, evecs = eigs(L, k=n_evecs + 1, which="LR")
    ix = evals.argsort()[::-1][1:]
    evals = np.real(evals[ix])
    evecs = np.real(evecs[:, ix])
    dmap = evecs @ np.diag(np.sqrt(-1.0 / evals))
    return dmap, evecs, evals


def diffusion_map_of_rows(E, n_evecs=2, epsilon=1.0, alpha=0.5, k=64):
    """pl.trajectory's embedding of the matrix E (steps 1-6 on the rows of E / E.max())."""
    E = np.asarray(E, dtype=np.float64)
    return diffusion_map_from_kernel(knn_kernel(E / E.max(), k, epsilon), epsilon, alpha, n_evecs)


def mu_spectrum(K, alpha):
    """All eigenvalues mu of P (real: P is similar to a symmetric matrix), descending -- for the spectral gaps of a fixture."""
    _, Ks = markov_operator(K, alpha)
    Ks = Ks.toarray()
    qa = Ks.sum(1) ** -alpha
    A = qa[:, None] * Ks * qa[None, :]
    w = 1.0 / np.sqrt(A.sum(1))
    S = A * w[:, None] * w[None, :]
    return np.linalg.eigvalsh(0.5 * (S + S.T))[::-1]


def align_signs(got, want):
    """Flip the columns of `want` to the sign of the matching columns of `got` (eigenvectors are defined up to sign)."""
    s = np.sign((got * want).sum(0))
    s[s == 0] = 1.0
    return want * s
