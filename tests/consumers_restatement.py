"""CPU references of the consumers of the finished matrix (K7: row distances, silhouette, kNN Gaussian kernel), the derived
error bounds the GPU tests hold the kernels to, and the input builders that keep those references valid.  numpy only here;
the tests set these beside scipy / scikit-learn.

Bounds (u = 2^-53, the unit roundoff of fp64; none of them is fitted to what a kernel returns):

* Euclidean: every term of sum_k (x_ik - x_jk)^2 is non-negative, so a length-N sum in ANY order has a relative error of at
  most (N - 1) u on top of the 2 u of a term; the square root halves it and adds its own rounding:
  |got - want| <= (N / 2 + 3) u want against a long-double evaluation, twice that against another fp64 evaluation.
* cosine of non-negative rows: x.y, |x|^2 and |y|^2 are such sums too and the quotient is at most 1, so the absolute error is
  at most (2 N + 6) u against long double, twice that against another fp64 evaluation.
* silhouette samples: a and b are means of N non-negative distances, s = (b - a) / max(a, b): (2 N + 8) u absolute.
* kNN kernel: the zero pattern is exact; a kept value is exp of the same fp64 argument on both sides, each exp within an
  ulp: 4 u relative.
"""
import numpy as np

U = 2.0 ** -53
assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the long-double references need an extended type"


def euclid_bound(N):
    """relative, against long double (twice that between two fp64 evaluations)"""
    return (N / 2 + 3) * U


def cosine_bound(N):
    """absolute, against long double (twice that between two fp64 evaluations); non-negative inputs"""
    return (2 * N + 6) * U


def silhouette_bound(N):
    """absolute, per sample and for their mean"""
    return (2 * N + 8) * U


KNN_VALUE_BOUND = 4 * U          # relative, kept entries


# ---- row distances -----------------------------------------------------------------------------------------------------------
TILE = 64                        # row_distance_kernel's output tile


def probe_rows(N):
    """The rows evaluated in long double: the first, the last, both sides of the first and of the last tile edge, one mid-matrix,
    and the two that distance_like_matrix makes identical."""
    last_edge = TILE * ((N - 1) // TILE)
    rows = {0, N - 1, N // 2, TILE - 1, TILE, last_edge - 1, last_edge, 3, N - 2}
    return np.array(sorted(r for r in rows if 0 <= r < N))


def row_distances_longdouble(X, rows, metric):
    """Rows `rows` of the row-distance matrix of X, every operation in long double.  euclidean: sqrt(sum (x - y)^2);
    cosine: 1 - x.y / (|x| |y|) clipped to [0, 2], 0 on the diagonal (sklearn's cosine_distances)."""
    XL = np.asarray(X, dtype=np.longdouble)
    out = np.empty((len(rows), XL.shape[0]), dtype=np.longdouble)
    if metric == "cosine":
        norms = np.sqrt((XL * XL).sum(1))
    for n, i in enumerate(rows):
        if metric == "euclidean":
            d = XL - XL[i][None, :]
            out[n] = np.sqrt((d * d).sum(1))
        else:
            out[n] = np.clip(1 - (XL * XL[i][None, :]).sum(1) / (norms * norms[i]), 0, 2)
            out[n, i] = 0
    return out


def distance_like_matrix(N, seed, max_at=None, duplicate=True):
    """A non-negative N x N matrix whose rows are the points: symmetric uniform noise with a zero diagonal, like a distance
    matrix.  max_at = "first" / "last": the maximum is moved into element [0, 0] / [N - 1, N - 1], the two ends of the buffer the
    max reduction walks.  duplicate: rows 3 and N - 2 are made identical (two identical patients)."""
    rng = np.random.default_rng(seed)
    E = rng.random((N, N))
    E = E + E.T
    np.fill_diagonal(E, 0.0)
    if duplicate and N >= 8:
        E[N - 2] = E[3]
    if max_at is not None:
        at = (0, 0) if max_at == "first" else (N - 1, N - 1)
        E[at] = 2.5
        assert np.argmax(E) == (0 if max_at == "first" else N * N - 1) and (E == E.max()).sum() == 1
    assert (E >= 0).all()
    return E


# ---- kNN Gaussian kernel -----------------------------------------------------------------------------------------------------
def stable_order(D):
    """Every row's columns by ascending distance, ties in index order: the stated rule of the kNN kernel."""
    return np.argsort(D, axis=1, kind="stable")


def knn_kernel_from_order(D, order, k, epsilon):
    """exp(-D^2 / (4 epsilon)) on the first min(k, N) columns of `order` of every row of D, 0 elsewhere; asserts that no kept
    value underflows towards the 0 that marks a dropped entry."""
    n, N = D.shape
    idx = order[:, :min(int(k), N)]
    want = np.zeros((n, N))
    r = np.arange(n)[:, None]
    want[r, idx] = np.exp(-D[r, idx] ** 2 / (4.0 * epsilon))
    assert want[r, idx].min() > 1e-300, "epsilon=%g lets a kept kernel value underflow" % epsilon
    return want


def knn_kernel_reference(D, k, epsilon):
    return knn_kernel_from_order(D, stable_order(D), k, epsilon)


def assert_tie_free(D_sorted, k, N):
    """Condition of the tie-free cases: the k-th and the (k + 1)-th smallest distance of every row differ by more than the
    Euclidean bound (both roundings), so which side of the cut an entry is on is never a matter of rounding."""
    if k >= D_sorted.shape[1]:
        return
    a, b = D_sorted[:, k - 1], D_sorted[:, k]
    assert (b - a > 2 * euclid_bound(N) * (a + b)).all(), "a row is tied at k=%d within the rounding bound: a tie case" % k


def cloud_distances(N, seed, dim=3):
    """Euclidean distances of N uniform points of the unit cube (no two rows' entries equal, checked by the callers with
    assert_tie_free), as float64 N x N."""
    rng = np.random.default_rng(seed)
    X = rng.random((N, dim))
    sq = (X * X).sum(1)
    D2 = sq[:, None] + sq[None, :]
    D2 -= 2.0 * (X @ X.T)
    np.maximum(D2, 0.0, out=D2)
    np.sqrt(D2, out=D2)
    np.fill_diagonal(D2, 0.0)
    return D2


def chunk_edges(N):
    """The tie walk counts in chunks of 64 columns: the first chunk boundary and the last one below N (64, 1984 at N = 2000)."""
    return 64, 64 * ((N - 1) // 64)


TIE_ROW, FLAT_ROW, N_BELOW = 70, 71, 10


def tied_distances(N, seed):
    """Distances rounded to two decimals (ties everywhere) of a cloud that holds three identical points (rows 5, 40 and
    N - 3: several exact zeros in those rows), plus two rows placed by hand:

    * row TIE_ROW: N_BELOW entries below 0.5 (itself, 0, among them), the value 0.5 at the two columns on either side of both
      chunk edges of chunk_edges(N) (62 .. 65 and, at N = 2000, 1982 .. 1985), 5 elsewhere.  With k = N_BELOW + 3 the last
      kept tie is the first column of the second chunk, with k = N_BELOW + 5 the cut falls inside the last-but-one chunk, with
      k = N_BELOW + 7 the last kept tie is the first column of the last chunk: the count carried from chunk to chunk decides;
    * row FLAT_ROW: 1 everywhere but itself: the k-th value is tied N - 1 ways."""
    rng = np.random.default_rng(seed)
    X = rng.random((N, 3))
    X[40] = X[5]
    X[N - 3] = X[5]
    D = np.round(np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)), 2)
    np.fill_diagonal(D, 0.0)
    e0, e1 = chunk_edges(N)
    assert e1 - 2 > 110 and e1 + 1 < N
    D[TIE_ROW] = 5.0
    D[TIE_ROW, TIE_ROW] = 0.0
    D[TIE_ROW, 100:100 + N_BELOW - 1] = 0.01 * np.arange(1, N_BELOW)
    D[TIE_ROW, [e0 - 2, e0 - 1, e0, e0 + 1, e1 - 2, e1 - 1, e1, e1 + 1]] = 0.5
    assert (D[TIE_ROW] < 0.5).sum() == N_BELOW and (D[TIE_ROW] == 0.5).sum() == 8
    D[FLAT_ROW] = 1.0
    D[FLAT_ROW, FLAT_ROW] = 0.0
    assert (D[5, [5, 40, N - 3]] == 0).all() and (D[40, [5, 40, N - 3]] == 0).all()
    return D


def near_cut_entries(D, k, rel):
    """Entries whose distance lies within the rounding bound of their row's k-th smallest one (the k-th itself excepted when
    nothing else is that close): a device that rounds the distances differently may put them on either side of the cut.
    rel: the relative bound of ONE distance.  Returns a boolean N x N mask (all False when k >= N)."""
    n, N = D.shape
    if k >= N:
        return np.zeros(D.shape, dtype=bool)
    kth = np.partition(D, k - 1, axis=1)[:, k - 1][:, None]
    near = np.abs(D - kth) <= rel * (D + kth)
    near[near.sum(1) == 1] = False          # only the k-th entry itself: the cut is clear
    return near


# ---- silhouette --------------------------------------------------------------------------------------------------------------
def silhouette_bincount(D, labels, n_clusters=None, return_ab=False):
    """silhouette_samples(D, labels, metric="precomputed") restated with np.bincount(labels, weights=row) -- the sums
    scikit-learn itself takes, in index order -- for label ids in [0, n_clusters), of which some may have no member (what
    scikit-learn, which renumbers the labels, cannot be asked)."""
    D = np.asarray(D, dtype=np.float64)
    labels = np.asarray(labels)
    C = int(labels.max()) + 1 if n_clusters is None else int(n_clusters)
    sizes = np.bincount(labels, minlength=C)
    used = int((sizes > 0).sum())
    assert 2 <= used <= len(labels) - 1, "silhouette needs 2 .. N - 1 distinct labels"
    N = len(labels)
    s, a, b = np.zeros(N), np.zeros(N), np.zeros(N)
    for i in range(N):
        sums = np.bincount(labels, weights=D[i], minlength=C)
        li = labels[i]
        with np.errstate(divide="ignore", invalid="ignore"):
            means = sums / sizes
        means[li] = np.inf
        means[sizes == 0] = np.inf
        b[i] = means.min()
        if sizes[li] > 1:
            a[i] = sums[li] / (sizes[li] - 1)
            mx = max(a[i], b[i])
            s[i] = (b[i] - a[i]) / mx if mx > 0 else 0.0
    return (s, a, b) if return_ab else s


def symmetric_distances(N, seed):
    """A random symmetric matrix with a zero diagonal, given to the silhouette directly as the precomputed distances."""
    rng = np.random.default_rng(seed)
    D = rng.random((N, N))
    D += D.T.copy()
    np.fill_diagonal(D, 0.0)
    return D


def cluster_labels(N, C, seed, layout="random", singleton=True):
    """int32 labels that use every id of [0, C): random, or sorted in blocks; with `singleton` (C > 2) id C - 1 has one member."""
    rng = np.random.default_rng(seed)
    if singleton and C > 2:
        lab = np.r_[np.arange(C), rng.integers(0, C - 1, N - C)]
    else:
        lab = np.r_[np.arange(C), rng.integers(0, C, N - C)]
    lab = np.sort(lab) if layout == "blocks" else rng.permutation(lab)
    sizes = np.bincount(lab, minlength=C)
    assert (sizes > 0).all() and 2 <= C <= N - 1 and (not (singleton and C > 2) or sizes[C - 1] == 1)
    return np.ascontiguousarray(lab, dtype=np.int32)
