"""The consumers of the finished matrix (K7, consumer_kernels.hpp: row distances, silhouette, kNN Gaussian kernel) at the sizes
they run at and at their LDS limits, each against an independent CPU reference (scipy / scikit-learn and the restatements of
tests/consumers_restatement.py, whose module docstring derives every bound used here; u = 2^-53).

What is pinned, and where:

* row distances: N = 63 .. 2000 around the 64-wide tile and the 16-wide k chunk, both ends of the max reduction's grid-stride
  walk (N^2 up to 4 M > its 262 144 threads), inputs scaled by 1e-6 and 1e6, identical rows;
* kNN kernel: N = 65 .. 16384 -- both regimes of the bitonic sort (N <= 512: one pair per thread; above: several), every
  padded size 1024 .. 16384, the 128 KiB LDS request, k = 1 .. N + 3; ties that straddle the 64-wide chunks of the tie walk;
  the refusal at N = 16385 before anything is staged;
* silhouette: C = 2 .. 600 (above 256 a thread owns several clusters), cluster ids without members, n_clusters 4096 / 4097,
  and the real staged / unstaged boundary of the row in LDS (N = 12 790 / 12 810, the 150 KiB request);
* the chains of tl.Sil_computing / tl.diffusion_kernel at the c4 size (N = 2000), from a host array and from HBM.

Every test prints what it measured before it asserts (run with -s to see it).  What the kernels achieve on an MI355X, largest
figure over all cases of a kind, beside the derived bound:

* Euclidean: 6.4 u from scipy (0.0 u when not normalised: the same sums in the same order), 25.2 u from long double at
  N = 2000 (bound 1003 u), 3.8 u at N = 63 (bound 34.5 u); at most 0.11 of the bound anywhere;
* cosine: 65 u from scikit-learn (bound 8012 u), 43 u from long double (bound 4006 u), at N = 2000;
* kNN kernel: zero pattern exact everywhere; kept values at most 2.0 u from numpy's exp (one ulp; bound 4 u);
* silhouette: samples 0.0 u from scikit-learn in every case (both sides add in index order), the score up to 17 u (numpy's
  mean adds pairwise, the library in order; bound (2 N + 8) u);
* chains at N = 2000: samples 5.8e-16 (Euclidean, bound 1.1e-12) and 4.4e-14 (cosine, bound 4.7e-11) from the CPU composition,
  kept kernel values 6.3e-15 relative (bound 5.6e-12);
* the N = 16385 refusals return in 0.01 .. 0.05 ms; a host call at N = 16384 takes 0.26 s, at N = 12 790 / 12 810 0.14 / 0.10 s.
"""
import time

import numpy as np
import pytest
from scipy.spatial.distance import cdist
from sklearn.metrics import silhouette_samples
from sklearn.metrics.pairwise import cosine_distances
from sklearn.neighbors import NearestNeighbors

import consumers_restatement as R
from pilot_amd import _lib, engine

pytestmark = pytest.mark.gpu

U = R.U

def _say(fmt, *args):
    print("    [measured] " + fmt % args, flush=True)


# ---- 1. row distances and the max reduction ----------------------------------------------------------------------------------
def check_euclidean(got, X, N, what):
    """the whole matrix against scipy (2 x the bound: both sides round), the probe rows against long double (the bound)"""
    ref = cdist(X, X)
    rel = np.abs(got - ref) / np.where(ref > 0, ref, 1.0)
    rows = R.probe_rows(N)
    want = R.row_distances_longdouble(X, rows, "euclidean")
    rel_ld = np.abs(got[rows] - want) / np.where(want > 0, want, 1)
    _say("%s N=%d euclidean: %.1f u vs scipy (bound %.1f u), %.1f u vs long double (bound %.1f u)", what, N, rel.max() / U,
         2 * R.euclid_bound(N) / U, float(rel_ld.max()) / U, R.euclid_bound(N) / U)
    assert (np.abs(got - ref) <= 2 * R.euclid_bound(N) * ref).all()
    assert (np.abs(got[rows] - want) <= R.euclid_bound(N) * want).all()
    assert (np.diag(got) == 0).all()


def check_cosine(got, X, N, what):
    ref = cosine_distances(X)
    rows = R.probe_rows(N)
    want = R.row_distances_longdouble(X, rows, "cosine")
    _say("%s N=%d cosine: %.1f u vs scikit-learn (bound %d u), %.1f u vs long double (bound %d u)", what, N,
         np.abs(got - ref).max() / U, 2 * R.cosine_bound(N) / U, float(np.abs(got[rows] - want).max()) / U, R.cosine_bound(N) / U)
    assert np.abs(got - ref).max() <= 2 * R.cosine_bound(N)
    assert np.abs(got[rows] - want).max() <= R.cosine_bound(N)
    assert (np.diag(got) == 0).all() and got.min() >= 0 and got.max() <= 2


ROW_CASES = [(N, None) for N in (63, 64, 65, 127, 128, 129)] + [(N, at) for N in (600, 1024, 2000) for at in ("last", "first")]


@pytest.mark.parametrize("N,max_at", ROW_CASES)
def test_row_distances_at_tile_edges_and_cohort_sizes(N, max_at):
    """Euclidean, Euclidean of E / max(E) and cosine.  For N >= 600 the maximum of E sits in the last / the first element, so a
    max reduction that misses either end of its walk normalises by the wrong number.  Rows 3 and N - 2 are identical: their
    Euclidean distance is exactly 0.0 and their cosine distance within its bound of 0."""
    E = R.distance_like_matrix(N, seed=N, max_at=max_at)
    what = "max %s" % max_at if max_at else "plain"
    D = engine.row_distances(E, metric="euclidean")
    check_euclidean(D, E, N, what)
    Dn = engine.row_distances(E, metric="euclidean", normalize_by_max=True)
    check_euclidean(Dn, E / E.max(), N, what + ", / max")
    Dc = engine.row_distances(E, metric="cosine")
    check_cosine(Dc, E, N, what)
    for M in (D, Dn):
        assert M[3, N - 2] == 0.0 and M[N - 2, 3] == 0.0
    assert Dc[3, N - 2] <= R.cosine_bound(N) and Dc[N - 2, 3] <= R.cosine_bound(N)


@pytest.mark.parametrize("N", [63, 64, 65, 127, 128, 129, 600, 1024, 2000])
@pytest.mark.parametrize("scale", [1e-6, 1e6])
def test_row_distances_of_scaled_inputs(N, scale):
    """The same E times 1e-6 and times 1e6: the Euclidean bound is relative and holds as it stands (an absolute tolerance
    would be void for the small matrix and hopeless for the large one); the cosine does not see the scale."""
    E = R.distance_like_matrix(N, seed=N, max_at="last" if N >= 600 else None)
    Es = E * scale
    check_euclidean(engine.row_distances(Es, metric="euclidean"), Es, N, "x %g" % scale)
    Dc = engine.row_distances(Es, metric="cosine")
    check_cosine(Dc, Es, N, "x %g" % scale)
    # unchanged: each side within its bound of its own exact value; rounding E * scale moves x.y, |x|^2, |y|^2 by 2 u each
    assert np.abs(Dc - engine.row_distances(E, metric="cosine")).max() <= 2 * R.cosine_bound(N) + 8 * U


# ---- 2. kNN kernel, tie-free -------------------------------------------------------------------------------------------------
EPS = 0.3          # unit-cube cloud: d^2 <= 3, exp(-d^2 / (4 eps)) >= 0.08 -- no kept value near underflow, whatever k


def ks_of(N, which):
    return [dict(one=1, two=2, k64=64, nm1=N - 1, n=N, np3=N + 3)[w] for w in which]


ALL_K = ("one", "two", "k64", "nm1", "n", "np3")
KNN_CASES = [(65, ("one", "k64", "np3")), (512, ("two", "n")), (513, ALL_K), (1024, ("k64", "nm1")), (1025, ("one", "n")),
             (2000, ALL_K), (4097, ("two", "k64")), (8192, ("k64", "nm1")), (8193, ("one", "k64", "np3"))]


def check_knn(K, D, order, rows, k, eps, what):
    """rows of the device kernel matrix against the stable-argsort reference: zero pattern exact, kept values within 4 u"""
    want = R.knn_kernel_from_order(D[rows], order, k, eps)
    got = K[rows]
    kept = want > 0
    np.testing.assert_array_equal(got > 0, kept, err_msg="%s: kept neighbours differ from the stable-argsort rule" % what)
    gap = (np.abs(got[kept] - want[kept]) / want[kept]).max()
    _say("%s: kept values %.2f u from numpy's exp (bound 4 u)", what, gap / U)
    assert gap <= R.KNN_VALUE_BOUND


def check_sklearn_sets(D, order, rows, k, N):
    """on tie-free rows the stable-argsort sets are scikit-learn's kneighbors sets: the reference is scikit-learn's"""
    kk = min(k, N)
    probe = rows[:: max(1, len(rows) // 64)]
    nn = NearestNeighbors(n_neighbors=kk, metric="precomputed").fit(D)
    nb = nn.kneighbors(D[probe], return_distance=False)
    ours = order[:: max(1, len(rows) // 64), :kk]
    assert (np.sort(nb, axis=1) == np.sort(ours, axis=1)).all()


@pytest.mark.parametrize("N,which", KNN_CASES)
def test_knn_kernel_tie_free(N, which):
    D = R.cloud_distances(N, seed=N)
    order = R.stable_order(D)
    Ds = np.take_along_axis(D, order, axis=1)
    rows = np.arange(N)
    for k in ks_of(N, which):
        R.assert_tie_free(Ds, k, N)
        K = engine.knn_gaussian_kernel(D, k=k, epsilon=EPS)
        assert ((K > 0).sum(1) == min(k, N)).all()
        check_knn(K, D, order, rows, k, EPS, "N=%d k=%d" % (N, k))
        if N <= 2000:
            check_sklearn_sets(D, order, rows, k, N)


def test_knn_kernel_tie_free_at_the_largest_n():
    """N = 16384: the 128 KiB sort (hipFuncSetAttribute beyond the 64 KiB default), NP2 = N.  Every k; the reference on 512 fixed
    rows (the first and the last among them), the count of exactly min(k, N) entries on every row."""
    N = 16384
    D = R.cloud_distances(N, seed=N)
    rows = np.unique(np.r_[0, N - 1, np.arange(7, N, N // 510)[:510]])
    assert len(rows) == 512 and rows[0] == 0 and rows[-1] == N - 1
    order = R.stable_order(D[rows])
    Ds = np.take_along_axis(D[rows], order, axis=1)
    nn = NearestNeighbors(metric="precomputed").fit(D)
    for k in ks_of(N, ALL_K):
        R.assert_tie_free(Ds, k, N)
        t0 = time.perf_counter()
        K = engine.knn_gaussian_kernel(D, k=k, epsilon=EPS)
        _say("N=%d k=%d: host call %.2f s", N, k, time.perf_counter() - t0)
        assert (np.count_nonzero(K, axis=1) == min(k, N)).all()
        check_knn(K, D, order, rows, k, EPS, "N=%d k=%d" % (N, k))
        nb = nn.kneighbors(D[rows[::8]], n_neighbors=min(k, N), return_distance=False)
        assert (np.sort(nb, axis=1) == np.sort(order[::8, :min(k, N)], axis=1)).all()
        del K


# ---- 3. kNN kernel, ties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [200, 2000])
def test_knn_kernel_ties_across_the_chunks_of_the_tie_walk(N):
    """Distances rounded to two decimals, three identical points, and the two hand-made rows of R.tied_distances: the k-th
    value shared by entries on both sides of column 64 and of the last chunk edge (1984 at N = 2000), and a row tied N - 1
    ways.  Positions included: everything against the stable-argsort rule.  With k = 1 a point with an identical twin of lower
    index keeps the twin, not itself."""
    D = R.tied_distances(N, seed=N)
    order = R.stable_order(D)
    rows = np.arange(N)
    e0, e1 = R.chunk_edges(N)
    below = set(np.flatnonzero(D[R.TIE_ROW] < 0.5))
    for k, ties in ((1, None), (R.N_BELOW + 3, [e0 - 2, e0 - 1, e0]), (R.N_BELOW + 5, [e0 - 2, e0 - 1, e0, e0 + 1, e1 - 2]),
                    (R.N_BELOW + 7, [e0 - 2, e0 - 1, e0, e0 + 1, e1 - 2, e1 - 1, e1]), (64, None), (N - 1, None)):
        K = engine.knn_gaussian_kernel(D, k=k, epsilon=1.0)
        assert ((K > 0).sum(1) == k).all()
        check_knn(K, D, order, rows, k, 1.0, "ties N=%d k=%d" % (N, k))
        if ties is not None:
            assert set(np.flatnonzero(K[R.TIE_ROW])) == below | set(ties)
        if k == 1:
            assert list(np.flatnonzero(K[40])) == [5] and list(np.flatnonzero(K[N - 3])) == [5] and K[40, 5] == 1.0
        if 1 < k < N:
            first = [j for j in range(k) if j != R.FLAT_ROW][:k - 1]
            assert sorted(np.flatnonzero(K[R.FLAT_ROW])) == sorted(first + [R.FLAT_ROW])


# ---- 4. kNN refusal ----------------------------------------------------------------------------------------------------------
def test_knn_kernel_refuses_rows_beyond_the_lds_sort_before_staging_anything():
    """N = 16385: the next power of two (256 KiB) does not fit LDS.  Every entry point that reaches the kNN kernel says so,
    naming N, before it allocates or uploads its N x N buffers (never-touched host pages here: nothing is read either)."""
    N = 16385
    E = np.zeros((N, N))
    out = np.empty((N, N))
    L = _lib.load()
    for name, call in (("pilot_ot_knn_kernel", lambda: L.pilot_ot_knn_kernel(_lib.dptr(E), N, 64, 1.0, _lib.dptr(out))),
                       ("pilot_ot_diffusion_kernel_of_rows",
                        lambda: L.pilot_ot_diffusion_kernel_of_rows(E.ctypes.data, 0, N, 64, 1.0, None, _lib.dptr(out))),
                       ("pilot_ot_diffusion_map_of_rows",
                        lambda: L.pilot_ot_diffusion_map_of_rows(E.ctypes.data, 0, N, 64, 1.0, 0.5, 2, _lib.dptr(out), None,
                                                                 _lib.dptr(out), _lib.iptr(np.zeros(2, dtype=np.int32))))):
        t0 = time.perf_counter()
        rc = call()
        _say("%s(N=%d) returned %d after %.3f ms", name, N, rc, 1e3 * (time.perf_counter() - t0))
        assert rc == _lib.ENOTSUP
        assert "N=16385" in L.pilot_ot_last_error().decode()
    for fn in (lambda: engine.knn_gaussian_kernel(E, k=64), lambda: engine.diffusion_kernel_of_rows(E, k=64),
               lambda: engine.diffusion_map_of_rows(E, n_evecs=2, k=64)):
        with pytest.raises(NotImplementedError, match="N=16385"):
            fn()


# ---- 5. silhouette -----------------------------------------------------------------------------------------------------------
def silhouette_abi(D, labels, n_clusters):
    """pilot_ot_silhouette as the C ABI takes it: label ids as given (engine renumbers them), n_clusters as given"""
    import ctypes
    D = np.ascontiguousarray(D, dtype=np.float64)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    score = ctypes.c_double(0.0)
    samples = np.empty(D.shape[0])
    _lib.check(_lib.load().pilot_ot_silhouette(_lib.dptr(D), _lib.iptr(labels), D.shape[0], int(n_clusters), ctypes.byref(score),
                                               _lib.dptr(samples)))
    return score.value, samples


def check_silhouette(score, samples, want, N, what):
    gap = np.abs(samples - want).max()
    _say("%s: samples %.1f u, score %.1f u from scikit-learn (bound %d u)", what, gap / U, abs(score - want.mean()) / U,
         R.silhouette_bound(N) / U)
    assert gap <= R.silhouette_bound(N)
    assert abs(score - want.mean()) <= R.silhouette_bound(N)


@pytest.mark.parametrize("layout", ["random", "blocks"])
@pytest.mark.parametrize("N,C", [(600, 2), (600, 5), (600, 257), (2000, 2), (2000, 5), (2000, 257), (2000, 600)])
def test_silhouette_at_cohort_sizes_and_many_clusters(N, C, layout):
    """C > 256: a thread of the 256 adds up several clusters.  For C > 2 the last cluster is a singleton (s = 0)."""
    D = R.symmetric_distances(N, seed=N + C)
    labels = R.cluster_labels(N, C, seed=C, layout=layout)
    want = silhouette_samples(D, labels, metric="precomputed")
    np.testing.assert_array_equal(R.silhouette_bincount(D, labels), want)
    score, samples = engine.silhouette_precomputed(D, labels, return_samples=True)
    check_silhouette(score, samples, want, N, "N=%d C=%d %s" % (N, C, layout))
    if C > 2:
        assert samples[labels == C - 1].tolist() == [0.0]


@pytest.mark.parametrize("N,C,empty", [(600, 6, (3,)), (2000, 302, (3, 300))])
def test_silhouette_with_cluster_ids_that_have_no_members(N, C, empty):
    """n_clusters larger than the labels in use, which the C ABI allows: ids in the middle of the range (and, at C = 302, in a
    thread's second trip) without a member.  Same bits as the renumbered call; values as the bincount restatement (which is
    scikit-learn's silhouette_samples bit for bit wherever scikit-learn can be asked)."""
    D = R.symmetric_distances(N, seed=N)
    dense = R.cluster_labels(N, C - len(empty), seed=N, layout="random")
    ids = np.array([c for c in range(C) if c not in empty], dtype=np.int32)
    labels = ids[dense]
    assert set(np.unique(labels)) == set(ids) and not set(empty) & set(labels)
    score, samples = silhouette_abi(D, labels, C)
    score_r, samples_r = engine.silhouette_precomputed(D, labels, return_samples=True)
    np.testing.assert_array_equal(samples, samples_r)
    assert score == score_r
    want = R.silhouette_bincount(D, labels, n_clusters=C)
    np.testing.assert_array_equal(want, silhouette_samples(D, dense, metric="precomputed"))
    check_silhouette(score, samples, want, N, "N=%d C=%d without %s" % (N, C, list(empty)))


def test_silhouette_cluster_count_limit():
    """n_clusters = 4096 is accepted (4091 ids without members; same bits as the renumbered call), 4097 refused"""
    N = 600
    D = R.symmetric_distances(N, seed=1)
    labels = R.cluster_labels(N, 5, seed=1)
    score, samples = silhouette_abi(D, labels, 4096)
    score_r, samples_r = engine.silhouette_precomputed(D, labels, return_samples=True)
    np.testing.assert_array_equal(samples, samples_r)
    assert score == score_r
    check_silhouette(score, samples, silhouette_samples(D, labels, metric="precomputed"), N, "n_clusters=4096")
    with pytest.raises(ValueError, match="4097"):
        silhouette_abi(D, labels, 4097)


def staged_in_lds(N, C):
    """the rule of pilot_ot_silhouette_dev: the row (N doubles), the labels (N ints) and C sums within 150 KiB"""
    return 8 * (N + C) + 4 * N <= 150 * 1024


def test_silhouette_on_both_sides_of_the_lds_boundary(switches):
    """N = 12 790 (153 520 bytes: the row is staged, the 150 KiB request) and N = 12 810 (153 760 bytes: read from global memory),
    C = 5, nothing forced, against scikit-learn; at N = 12 790 the forced unstaged form gives the same bits."""
    C = 5
    assert staged_in_lds(12790, C) and not staged_in_lds(12810, C)
    big = R.symmetric_distances(12810, seed=12810)
    for N in (12790, 12810):
        D = np.ascontiguousarray(big[:N, :N])
        labels = R.cluster_labels(N, C, seed=N)
        want = silhouette_samples(D, labels, metric="precomputed")
        t0 = time.perf_counter()
        score, samples = engine.silhouette_precomputed(D, labels, return_samples=True)
        _say("N=%d (%s): host call %.2f s", N, "staged" if staged_in_lds(N, C) else "unstaged", time.perf_counter() - t0)
        check_silhouette(score, samples, want, N, "N=%d C=%d" % (N, C))
        if N == 12790:
            switches.setenv("PILOT_OT_SIL_UNSTAGED", "1")
            score_u, samples_u = engine.silhouette_precomputed(D, labels, return_samples=True)
            switches.delenv("PILOT_OT_SIL_UNSTAGED")
            np.testing.assert_array_equal(samples, samples_u)
            assert score == score_u


# ---- 6. chains at the c4 size ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c4_sized():
    """a synthetic 2000 x 2000 distance matrix (cdist of a 3-D cloud), its normalised rows and their scipy row distances"""
    X = np.random.default_rng(2000).random((2000, 3))
    E = cdist(X, X)
    Xn = E / E.max()
    return E, Xn, cdist(Xn, Xn)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_silhouette_chain_at_the_c4_size(c4_sized, metric):
    """silhouette_of_rows(normalised) = row distances -> silhouette without leaving the device, against the same composed on
    the CPU.  The distances the device silhouette reads differ from the CPU's by their own bound e (relative 2 (N/2 + 3) u
    for Euclidean; absolute 2 (2 N + 6) u for cosine), so a and b move by e a, e b (by e), and s = (b - a) / max(a, b) by at
    most 3 e (3 e / max(a, b)), on top of the silhouette's own (2 N + 8) u."""
    E, Xn, Dn = c4_sized
    N = E.shape[0]
    labels = R.cluster_labels(N, 5, seed=4)
    D_ref = Dn if metric == "euclidean" else cosine_distances(Xn)
    want, a, b = R.silhouette_bincount(D_ref, labels, return_ab=True)
    np.testing.assert_array_equal(want, silhouette_samples(D_ref, labels, metric="precomputed"))
    if metric == "euclidean":
        tol = R.silhouette_bound(N) + 3 * 2 * R.euclid_bound(N)
    else:
        tol = R.silhouette_bound(N) + 3 * 2 * R.cosine_bound(N) / np.maximum(a, b).min()
    host = engine.silhouette_of_rows(E, labels, metric=metric, normalize_by_max=True, return_samples=True)
    dev = engine.silhouette_of_rows(engine.DeviceMatrix.upload(E), labels, metric=metric, normalize_by_max=True, return_samples=True)
    np.testing.assert_array_equal(host[1], dev[1])
    assert host[0] == dev[0]
    _say("chain %s N=%d: samples %.3e from the CPU composition (bound %.3e)", metric, N, np.abs(host[1] - want).max(), tol)
    assert np.abs(host[1] - want).max() <= tol and abs(host[0] - want.mean()) <= tol


def test_diffusion_kernel_chain_at_the_c4_size(c4_sized):
    """diffusion_kernel_of_rows(k = 64, eps = 1) against cdist -> stable-argsort kernel on the CPU; both routes bit for bit.
    The input is tie-free beyond the distances' rounding (asserted), so the zero pattern is exact; a kept value is
    exp(-d^2 / 4 eps) of a distance with relative error e = 2 (N/2 + 3) u: relative 2 e d^2 / (4 eps), plus the 4 u of exp."""
    E, Xn, Dn = c4_sized
    N, k, eps = E.shape[0], 64, 1.0
    order = R.stable_order(Dn)
    R.assert_tie_free(np.take_along_axis(Dn, order, axis=1), k, N)
    want = R.knn_kernel_from_order(Dn, order, k, eps)
    Dh, Kh = engine.diffusion_kernel_of_rows(E, k=k, epsilon=eps)
    Dd, Kd = engine.diffusion_kernel_of_rows(engine.DeviceMatrix.upload(E), k=k, epsilon=eps)
    np.testing.assert_array_equal(Dh, Dd)
    np.testing.assert_array_equal(Kh, Kd)
    assert (np.abs(Dh - Dn) <= 2 * R.euclid_bound(N) * Dn).all()
    np.testing.assert_array_equal(Kh > 0, want > 0)
    tol = R.KNN_VALUE_BOUND + 2 * (2 * R.euclid_bound(N)) * Dn ** 2 / (4 * eps)
    kept = want > 0
    rel = np.abs(Kh - want)[kept] / want[kept]
    _say("chain kernel N=%d: kept values %.3e relative from the CPU composition (largest bound %.3e)", N, rel.max(), tol[kept].max())
    assert (rel <= tol[kept]).all()
