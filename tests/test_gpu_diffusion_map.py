"""Diffusion map on the device (K8: pilot_ot_diffusion_map_dev / _of_rows, engine.diffusion_map_*, tl.diffusion_map) against the
numpy / scipy restatement of pydiffmap (tests/diffmap_restatement.py) and a dense eigensolver; symmetric clouds (lattices, rings, a
three-fold cohort), whose leading eigenvalues repeat, against the dense eigensolver by eigenvalue lists, residuals and projectors."""
import functools

import numpy as np
import pytest
from scipy.spatial.distance import cdist

import consumers_restatement as C
import diffmap_restatement as R
from conftest import GOLDEN_REAL, golden_adata, load_golden
from pilot_amd import _lib, engine, tl
from pilot_amd.synthetic import CONFIGS, make_problem

pytestmark = pytest.mark.gpu

GAP = 1e-4          # eigenvectors are compared only where mu is this far from its neighbours (asserted, never skipped)


@pytest.fixture(scope="module")
def kidney():
    """The reference test's own cohort at PILOT's defaults: all 634 rows of its exact matrix (the fixture stores every third)."""
    g = load_golden(GOLDEN_REAL)
    ad, cell_col = golden_adata(g)
    tl.wasserstein_distance(ad, clusters_col=cell_col, sample_col="sampleID", status="status", data_type="Pathomics")
    assert np.abs(ad.uns["EMD"][::int(g["row_step"])] - g["emd_unreg"]).max() <= 1e-12
    return ad


@pytest.fixture(scope="module")
def matrices(kidney):
    cache = {}

    def get(name):
        if name not in cache:
            if name == "c1":
                cache[name] = load_golden("c1_20x10x10")["emd_unreg"]
            elif name == "kidney":
                cache[name] = kidney.uns["EMD"]
            else:
                cache[name] = engine.emd_grid(*make_problem(**CONFIGS[name]))
        return cache[name]
    return get


def column_gaps(mu, n_evecs):
    """distance of mu[c + 1] (the c-th returned pair) to its neighbours in the descending spectrum"""
    out = []
    for c in range(n_evecs):
        lo = mu[c + 1] - mu[c + 2] if c + 2 < len(mu) else np.inf
        out.append(min(mu[c] - mu[c + 1], lo))
    return np.array(out)


def check_sign_rule(evecs):
    for c in range(evecs.shape[1]):
        a = int(np.argmax(np.abs(evecs[:, c])))            # (the first of equal magnitudes)
        assert evecs[a, c] > 0.0, "column %d: largest entry %d is negative" % (c, a)


def check_against_restatement(K, dmap, evecs, evals, eps, alpha, n_evecs):
    rd, re, rl = R.diffusion_map_from_kernel(K, eps, alpha, n_evecs)
    assert np.abs(evals - rl).max() <= 1e-10 / eps, (evals, rl)
    P, _ = R.markov_operator(K, alpha)
    mu = 1.0 + eps * evals
    res = np.abs(P @ evecs - evecs * mu[None, :]).max()
    assert res <= 1e-10, "residual |P psi - mu psi| = %.3e" % res
    np.testing.assert_allclose(np.linalg.norm(evecs, axis=0), 1.0, rtol=0, atol=1e-12)
    check_sign_rule(evecs)
    gaps = column_gaps(R.mu_spectrum(K, alpha), n_evecs)
    assert gaps.min() >= GAP, "fixture gap %.2e < %.0e: pick another case rather than loosening the tolerance" % (gaps.min(), GAP)
    re = R.align_signs(evecs, re)
    rd = R.align_signs(dmap, rd)
    assert (np.abs(evecs - re).max(0) / np.abs(re).max(0)).max() <= 1e-6
    assert (np.abs(dmap - rd).max(0) / np.abs(rd).max(0)).max() <= 1e-6


def check_kernel_against_stable_argsort(K, E, knn, eps):
    """The device's kNN kernel matrix K (K7) against an independent one: scipy's row distances of E / E.max(), the k smallest
    of every row by a stable argsort (ties in index order), exp(-d^2 / (4 eps)) there and 0 elsewhere.  The device rounds its
    distances differently from scipy (each within (N/2 + 3) u relative of the exact one, tests/consumers_restatement.py), so an
    entry whose distance lies within that of the row's k-th may fall on either side of the cut: such rows are counted on the
    reference alone and must be at most 1 % of the rows (a condition on the fixture, not a tolerance); everywhere else the zero
    pattern is exact.  A kept value is exp of a distance with relative error e = 2 (N/2 + 3) u: 2 e d^2 / (4 eps) relative,
    plus the 4 u of the two exps."""
    N = E.shape[0]
    X = E / E.max()
    D = cdist(X, X)
    want = C.knn_kernel_reference(D, knn, eps)
    e = 2 * C.euclid_bound(N)
    near = C.near_cut_entries(D, knn, e)
    n_close = int(near.any(1).sum())
    print("    [measured] N=%d knn=%d: %d rows with an entry within the rounding bound of the k-th distance" % (N, knn, n_close))
    assert n_close <= 0.01 * N, "%d of %d rows are tied at the cut within rounding: pick another knn for this fixture" % (n_close, N)
    assert ((K > 0).sum(1) == min(knn, N)).all()
    assert (((K > 0) == (want > 0)) | near).all(), "kept neighbours differ from the stable-argsort rule away from the cut"
    kept = K > 0
    G = np.exp(-D ** 2 / (4.0 * eps))
    tol = C.KNN_VALUE_BOUND + 2 * e * D ** 2 / (4.0 * eps)
    assert (np.abs(K - G)[kept] <= (tol * G)[kept]).all()


# (matrix, knn, epsilon, alpha, n_evecs): every value of each parameter appears; knn >= N is the full Gaussian kernel
CASES = [
    ("c1", 5, 1.0, 0.5, 2), ("c1", 16, 0.3, 0.0, 5), ("c1", 64, 1.0, 1.0, 10), ("c1", 20, 0.3, 0.5, 1),
    ("kidney", 64, 1.0, 0.5, 2), ("kidney", 5, 0.3, 1.0, 1), ("kidney", 16, 1.0, 0.0, 10), ("kidney", 634, 0.3, 0.5, 5),
    ("c2", 64, 1.0, 0.5, 2), ("c2", 5, 1.0, 0.0, 5), ("c2", 16, 0.3, 1.0, 10), ("c2", 100, 1.0, 0.5, 1),
    ("c3", 64, 1.0, 0.5, 2), ("c3", 16, 0.3, 0.5, 5), ("c3", 5, 1.0, 1.0, 1), ("c3", 600, 0.3, 0.0, 2),
]


@pytest.mark.parametrize("name,knn,eps,alpha,n_evecs", CASES)
def test_matches_the_pydiffmap_restatement(matrices, name, knn, eps, alpha, n_evecs):
    E = matrices(name)
    _, K = engine.diffusion_kernel_of_rows(E, k=knn, epsilon=eps, return_distances=False)     # step 1: K7's kernel
    check_kernel_against_stable_argsort(K, E, knn, eps)                                       # ... held to an independent one
    dmap, evecs, evals, info = engine.diffusion_map_of_rows(E, n_evecs=n_evecs, epsilon=eps, alpha=alpha, k=knn, return_info=True)
    assert info["flags"] == 0 and info["converged"] and not info["degenerate"], info
    assert dmap.shape == evecs.shape == (E.shape[0], n_evecs) and evals.shape == (n_evecs,)
    assert (np.diff(evals) <= 0).all() and (evals < 0).all()
    check_against_restatement(K, dmap, evecs, evals, eps, alpha, n_evecs)


@pytest.mark.parametrize("N", [2, 3, 64, 65, 333, 1025])
def test_full_gaussian_kernel_against_a_dense_eigensolver(N):
    """k >= N: the full Gaussian kernel of a random planar cloud; the eigenpairs of S = D^-1/2 A D^-1/2 from numpy's eigh.
    N = 1025 is above the Lanczos basis cap (1024 vectors)."""
    rng = np.random.default_rng(N)
    X = rng.random((N, 2))
    eps, alpha = 0.02, 0.5
    K = np.exp(-((X[:, None, :] - X[None, :, :]) ** 2).sum(-1) / (4 * eps))
    n_evecs = min(N - 1, 4)
    dmap, evecs, evals, info = engine.diffusion_map_from_kernel(K, n_evecs=n_evecs, epsilon=eps, alpha=alpha, return_info=True)
    assert info["flags"] == 0, info
    assert info["steps"] <= min(N, 1024)
    qa = K.sum(1) ** -alpha
    A = qa[:, None] * K * qa[None, :]
    d = A.sum(1)
    S = A / np.sqrt(d)[:, None] / np.sqrt(d)[None, :]
    mu, phi = np.linalg.eigh(0.5 * (S + S.T))
    mu, phi = mu[::-1], phi[:, ::-1]
    assert np.abs(evals - (mu[1:n_evecs + 1] - 1.0) / eps).max() <= 1e-10 / eps
    assert column_gaps(mu, n_evecs).min() >= GAP
    psi = phi[:, 1:n_evecs + 1] / np.sqrt(d)[:, None]
    psi /= np.linalg.norm(psi, axis=0)
    psi = R.align_signs(evecs, psi)
    assert (np.abs(evecs - psi).max(0) / np.abs(psi).max(0)).max() <= 1e-6
    np.testing.assert_allclose(dmap, evecs * np.sqrt(-1.0 / evals), rtol=1e-14, atol=0)
    check_sign_rule(evecs)


# ---- repeated eigenvalues: symmetric clouds ------------------------------------------------------------------------------------------
# A point cloud with a symmetry (a square lattice, a ring, a three-fold cohort) gives the Markov operator repeated eigenvalues among
# the leading ones, and a Krylov space grown from one vector holds one direction per distinct eigenvalue: a single-vector Lanczos
# run that accepts as soon as the wanted Ritz pairs have converged can return the next distinct eigenvalue in place of the copy.
def _lattice(a):
    i, j = np.meshgrid(np.arange(a, dtype=np.float64), np.arange(a, dtype=np.float64), indexing="ij")
    return np.stack([i.ravel(), j.ravel()], axis=1)


def _ring(N):
    t = 2.0 * np.pi * np.arange(N) / N
    return np.stack([np.cos(t), np.sin(t)], axis=1)


def _threefold():
    rng = np.random.default_rng(11)
    X = rng.standard_normal((15, 2)) + np.array([3.0, 0.0])        # 15 points drawn once, placed at radius 3
    out = []
    for turn in (0.0, 2.0 * np.pi / 3.0, 4.0 * np.pi / 3.0):
        c, s_ = np.cos(turn), np.sin(turn)
        out.append(X @ np.array([[c, s_], [-s_, c]]))
    return np.concatenate(out)


CLOUDS = {"lattice5": (lambda: _lattice(5), 2.0), "lattice6": (lambda: _lattice(6), 0.5), "lattice8": (lambda: _lattice(8), 1.0),
          "lattice10": (lambda: _lattice(10), 0.5), "ring12": (lambda: _ring(12), 0.05), "ring64": (lambda: _ring(64), 0.05),
          "ring200": (lambda: _ring(200), 0.05), "threefold": (_threefold, 1.0)}
SYMMETRIC_CASES = ([(c, al, ne) for c in ("lattice5", "lattice6", "lattice8", "lattice10") for al in (0.0, 0.5, 1.0) for ne in (1, 2, 3, 4, 5)]
                   + [(c, 0.5, ne) for c in ("ring12", "ring64", "ring200") for ne in (1, 2, 4)]
                   + [("threefold", 0.5, ne) for ne in (1, 2, 3, 4)])


@functools.lru_cache(maxsize=None)
def _symmetric_reference(cloud, alpha):
    """(K, d, P, mu descending, phi to match) of the full Gaussian kernel of the cloud: numpy's eigh of S, as in
    test_full_gaussian_kernel_against_a_dense_eigensolver"""
    make, eps = CLOUDS[cloud]
    X = make()
    K = np.exp(-((X[:, None, :] - X[None, :, :]) ** 2).sum(-1) / (4 * eps))
    qa = K.sum(1) ** -alpha
    A = qa[:, None] * K * qa[None, :]
    d = A.sum(1)
    S = A / np.sqrt(d)[:, None] / np.sqrt(d)[None, :]
    mu, phi = np.linalg.eigh(0.5 * (S + S.T))
    mu, phi = mu[::-1].copy(), phi[:, ::-1].copy()
    P = A / d[:, None]
    assert mu[0] - mu[1] >= GAP                                    # a connected graph: mu = 1 is simple
    if cloud != "threefold":                                       # an exactly repeated pair among the first five after mu = 1
        assert (np.abs(np.diff(mu[1:6])) <= 1e-13).any(), (cloud, alpha, mu[:6])
    for a in (K, d, P, mu, phi):
        a.setflags(write=False)
    return K, d, P, mu, phi


def _wanted_clusters(mu, n_evecs):
    """index ranges [a, b) of the descending spectrum mu: maximal runs closer than GAP, wholly inside the wanted 1 .. n_evecs and
    GAP away from the rest"""
    out, a = [], 1
    while a <= n_evecs:
        b = a + 1
        while b < mu.size and mu[b - 1] - mu[b] < GAP:
            b += 1
        if b <= n_evecs + 1 and mu[a - 1] - mu[a] >= GAP and mu[a] - mu[b - 1] < GAP:
            out.append((a, b))
        a = b
    return out


@pytest.mark.parametrize("cloud,alpha,n_evecs", SYMMETRIC_CASES)
def test_repeated_eigenvalues_of_symmetric_clouds(cloud, alpha, n_evecs):
    """The eigenvalues as a sorted list with their multiplicity, eigenvectors by their residual (a column is defined only up to a
    rotation inside its eigenspace), and the projector of every cluster of eigenvalues that lies inside the wanted set.  The sign
    rule: the device takes the entry of largest magnitude before it normalises the column, and a symmetric cloud has entries that
    differ in the last bit only, which the division can make equal; so an entry within 8 ulp of the largest must be positive."""
    eps = CLOUDS[cloud][1]
    K, d, P, mu, phi = _symmetric_reference(cloud, alpha)
    N = K.shape[0]
    dmap, evecs, evals, info = engine.diffusion_map_from_kernel(np.array(K), n_evecs=n_evecs, epsilon=eps, alpha=alpha, return_info=True)
    what = "%s alpha=%g n_evecs=%d" % (cloud, alpha, n_evecs)
    want = (mu[1:n_evecs + 1] - 1.0) / eps
    print("%s: %d steps, flags %d, mu %s, reference %s" % (what, info["steps"], info["flags"], 1.0 + eps * evals, mu[1:n_evecs + 1]))
    assert info["converged"] and not info["degenerate"] and info["flags"] == 0, (what, info)
    assert info["steps"] <= N
    assert dmap.shape == evecs.shape == (N, n_evecs) and evals.shape == (n_evecs,)
    e_val = np.abs(evals - want).max()
    res = np.abs(P @ evecs - evecs * (1.0 + eps * evals)[None, :]).max()
    print("%s: evals %.2e (tol %.0e), residual %.2e (1e-10)" % (what, e_val, 1e-10 / eps, res))
    assert e_val <= 1e-10 / eps, (what, evals, want)
    assert res <= 1e-10, what
    np.testing.assert_allclose(np.linalg.norm(evecs, axis=0), 1.0, rtol=0, atol=1e-12)
    for c in range(n_evecs):
        big = np.abs(evecs[:, c]) >= np.abs(evecs[:, c]).max() * (1.0 - 8 * np.finfo(np.float64).eps)
        assert (evecs[big, c] > 0.0).any(), "%s column %d: the largest entries are negative" % (what, c)
    np.testing.assert_allclose(dmap, evecs * np.sqrt(-1.0 / evals), rtol=1e-14, atol=0)
    for a, b in _wanted_clusters(mu, n_evecs):
        q, _ = np.linalg.qr(np.sqrt(d)[:, None] * evecs[:, a - 1:b - 1])
        e_proj = np.abs(q @ q.T - phi[:, a:b] @ phi[:, a:b].T).max()
        print("%s: cluster [%d, %d): projector %.2e (tol 1e-6)" % (what, a, b, e_proj))
        assert e_proj <= 1e-6, what


def test_cluster_rule_of_the_symmetric_cases():
    mu = np.array([1.0, 0.8, 0.8, 0.7, 0.5, 0.5, 0.5, 0.1])
    assert [_wanted_clusters(mu, k) for k in (1, 2, 3, 4, 6)] == [[], [(1, 3)], [(1, 3), (3, 4)], [(1, 3), (3, 4)], [(1, 3), (3, 4), (4, 7)]]


def test_repeated_calls_and_both_routes_give_identical_bits():
    """Fixed-order sums, no float atomics: the same call twice, and the host-array route against the DeviceMatrix route (the
    matrix where the pair grid left it)."""
    P, M = make_problem(**CONFIGS["c2"])
    plan = engine.DevicePlan(P, M)
    plan.run(0.1)
    plan.sync()
    E = plan.fetch()[0]
    a = engine.diffusion_map_of_rows(E, n_evecs=5, return_info=True)
    b = engine.diffusion_map_of_rows(E, n_evecs=5, return_info=True)
    c = engine.diffusion_map_of_rows(plan.device_matrix(), n_evecs=5, return_info=True)
    plan.close()
    for x in (b, c):
        for u, v in zip(a[:3], x[:3]):
            np.testing.assert_array_equal(u, v)
        assert a[3] == x[3]


def test_from_kernel_host_and_device_routes_release_their_buffers():
    """diffusion_map_from_kernel of a host kernel matrix (uploaded into a buffer of the call's own) and of a DeviceMatrix of it give
    the same bits; so does a second call, which takes its device buffers anew after the first released them."""
    rng = np.random.default_rng(6)
    X = rng.standard_normal((6, 3))
    Kmat = engine.knn_gaussian_kernel(cdist(X, X), k=4, epsilon=1.0)
    first = engine.diffusion_map_from_kernel(Kmat, n_evecs=2, return_info=True)
    dev = engine.diffusion_map_from_kernel(engine.DeviceMatrix.upload(Kmat), n_evecs=2, return_info=True)
    again = engine.diffusion_map_from_kernel(Kmat, n_evecs=2, return_info=True)
    assert first[0].shape == first[1].shape == (6, 2) and first[2].shape == (2,)
    for other in (dev, again):
        for u, v in zip(first[:3], other[:3]):
            assert np.array_equal(np.ascontiguousarray(u).view(np.uint64), np.ascontiguousarray(v).view(np.uint64))
        assert first[3] == other[3]


def _two_clusters(n1=40, n2=30, seed=5):
    rng = np.random.default_rng(seed)
    X = np.r_[rng.random((n1, 2)), rng.random((n2, 2)) + 50.0]
    return np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))


def test_disconnected_kernel_is_degenerate():
    """Block-diagonal kernel: eigenvalue 1 twice.  The Lanczos basis opens with the known eigenvector sqrt(d); its breakdown
    restarts orthogonally to it, where the second eigenvalue 1 is found."""
    D = _two_clusters()
    K = np.exp(-D ** 2 / 4.0)
    K[D > 10.0] = 0.0
    dmap, evecs, evals, info = engine.diffusion_map_from_kernel(K, n_evecs=2, epsilon=1.0, return_info=True)
    assert info["degenerate"] and info["flags"] & _lib.DIFFMAP_DEGENERATE
    assert abs(evals[0]) <= 1e-10                              # the repeated mu = 1: lambda = 0
    with pytest.raises(ValueError):
        engine.diffusion_map_from_kernel(K, n_evecs=2, epsilon=1.0)
    ad = type("A", (), {})()
    ad.uns = {"EMD": D}
    with pytest.raises(ValueError, match="knn"):
        tl.diffusion_map(ad, knn=5)
    assert set(ad.uns) == {"EMD"}
    # three components: mu = 1 three times, and the copy a single restart vector does not show needs a second restart
    rng = np.random.default_rng(7)
    X = np.r_[rng.random((30, 2)), rng.random((25, 2)) + 50.0, rng.random((20, 2)) + 100.0]
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    K = np.exp(-D ** 2 / 4.0)
    K[D > 10.0] = 0.0
    dmap, evecs, evals, info = engine.diffusion_map_from_kernel(K, n_evecs=2, epsilon=1.0, return_info=True)
    print("three components: evals %s, %d steps, flags %d" % (evals, info["steps"], info["flags"]))
    assert info["degenerate"] and info["flags"] & _lib.DIFFMAP_DEGENERATE
    assert abs(evals[0]) <= 1e-10 and abs(evals[1]) <= 1e-10
    with pytest.raises(ValueError):
        engine.diffusion_map_from_kernel(K, n_evecs=2, epsilon=1.0)


def test_small_basis_is_not_converged(matrices, switches):
    E = matrices("c2")
    switches.setenv("PILOT_OT_DIFFMAP_BASIS", "4")
    dmap, evecs, evals, info = engine.diffusion_map_of_rows(E, n_evecs=2, return_info=True)
    assert not info["converged"] and info["flags"] & _lib.DIFFMAP_NOT_CONVERGED and info["steps"] == 4
    with pytest.raises(ValueError):
        engine.diffusion_map_of_rows(E, n_evecs=2)
    ad = type("A", (), {})()
    ad.uns = {"EMD": E}
    with pytest.raises(ValueError, match="converge"):
        tl.diffusion_map(ad)
    switches.delenv("PILOT_OT_DIFFMAP_BASIS")
    assert engine.diffusion_map_of_rows(E, n_evecs=2, return_info=True)[3]["converged"]


@pytest.mark.parametrize("cohort", ["c1", "kidney"])
def test_tl_diffusion_map_fills_the_embedding(kidney, cohort, tmp_path, monkeypatch):
    """tl.diffusion_map after tl.wasserstein_distance: uns['embedding'] is what pl.trajectory computes (ploting.py:95-110, its
    defaults n_evecs=2, epsilon=1, alpha=0.5, knn=64), engine's dmap bit for bit; nothing else in uns changes."""
    monkeypatch.chdir(tmp_path)
    if cohort == "c1":
        g = load_golden("c1_20x10x10")
        ad, cell_col = golden_adata(g)
        tl.wasserstein_distance(ad, emb_matrix="X_pca", clusters_col=cell_col, sample_col="sampleID", status="status")
        knn = 64
    else:
        ad, knn = kidney, 64
    before = dict(ad.uns)
    emb = tl.diffusion_map(ad)
    assert set(ad.uns) == set(before) | {"embedding"}
    assert all(ad.uns[k] is before[k] for k in before)
    assert ad.uns["embedding"] is emb
    E = ad.uns["EMD"]
    assert isinstance(emb, np.ndarray) and emb.dtype == np.float64 and emb.shape == (E.shape[0], 2)
    dmap, evecs, evals = engine.diffusion_map_of_rows(E, n_evecs=2, epsilon=1.0, alpha=0.5, k=knn)
    np.testing.assert_array_equal(emb, dmap)
    _, K = engine.diffusion_kernel_of_rows(E, k=knn, epsilon=1.0, return_distances=False)
    check_against_restatement(K, dmap, evecs, evals, 1.0, 0.5, 2)
    del ad.uns["embedding"]
