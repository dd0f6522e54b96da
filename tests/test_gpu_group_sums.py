"""K14 on the device: engine.group_sums (group_sums_kernel, csr_group_sums_kernel, group_sums_join_kernel) against np.add.at on
float64 (tests/pseudobulk_restatement.py::group_sums).

Integer-valued data (counts 0..50, every sum far below 2^24): every partial sum is an integer a float64 holds exactly, so the
result must EQUAL the restatement bit for bit, by every route -- a host array, a DeviceMatrix, a device_columns window with a
leading dimension above its width, and a DeviceCSR -- whatever the order of the additions.

General values: a sum of n terms taken in ANY order errs by at most (n - 1) u sum|y| (u = 2^-53), so each entry is held to
max(n_g, 64) * 2^-53 * sum|y| over that entry's rows.  The bound is the textbook one, not a measurement; it covers every slice and
join order the kernels may use.

L = pilot_ot_group_sums_slice_rows() (rows per slice), B = pilot_ot_group_sums_col_block() (columns per wave of the sparse kernel):
the shapes sit on either side of both."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import pseudobulk_restatement as PR
from pilot_amd import _lib, engine

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
DTYPES = [np.float32, np.float64]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _routes(Y, with_csr=True):
    """the same matrix by every route: name -> what engine.group_sums takes"""
    n, G = Y.shape
    wide = np.zeros((n, G + 5), dtype=Y.dtype)
    wide[:, 3:3 + G] = Y
    wide[:, :3], wide[:, 3 + G:] = 7.0, 9.0                         # the columns beside the window must stay out of every sum
    out = {"host": Y, "device": engine.DeviceMatrix.upload(Y), "window": engine.device_columns(engine.DeviceMatrix.upload(wide), 3, 3 + G)}
    if with_csr:
        out["csr"] = engine.DeviceCSR.upload(sp.csr_matrix(Y))
    return out


def _exact(Y, codes, n_groups, cols=None, what=""):
    want = PR.group_sums(Y, codes, n_groups, cols)
    for name, route in _routes(Y).items():
        got = engine.group_sums(route, codes, n_groups, cols=cols)
        assert got[0].dtype == np.int64 and got[1].dtype == np.float64, (what, name)
        assert _same(got, want), "%s, %s: differs from the restatement" % (what, name)
    return want


def _counts(rng, n, G, dtype):
    return rng.integers(0, 51, (n, G)).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_shapes_bit_for_bit(dtype):
    rng = np.random.default_rng(1)
    _exact(_counts(rng, 1, 1, dtype), np.array([0]), 1, what="1 x 1")
    count, sums = _exact(_counts(rng, 3, 5, dtype), np.array([0, 2, 2]), 3, what="3 x 5")
    assert list(count) == [1, 0, 2] and (sums[1] == 0).all() and not np.signbit(sums[1]).any()        # an empty group: 0.0, not NaN
    for G in (255, 256, 257):
        _exact(_counts(rng, 257, G, dtype), rng.integers(0, 2, 257), 2, what="257 x %d" % G)


@pytest.mark.parametrize("dtype", DTYPES)
def test_groups_around_the_slice_length(dtype):
    L = engine.group_sums_slice_rows()
    rng = np.random.default_rng(2)
    for big in (L - 1, L, L + 1, 2 * L + 1):
        n = big + 3
        codes = np.full(n, 1)
        codes[[0, n // 2, n - 1]] = [0, 2, 3]                      # single-row groups before, inside and after the long one
        count, _ = _exact(_counts(rng, n, 70, dtype), codes, 4, what="a group of %d rows" % big)
        assert list(count) == [1, big, 1, 1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_many_groups(dtype):
    rng = np.random.default_rng(3)
    count, _ = _exact(_counts(rng, 300, 33, dtype), rng.integers(0, 1000, 300), 1000, what="1 000 groups over 300 rows")
    assert (count == 0).sum() > 700
    codes = rng.integers(0, 600, 5000)
    codes[rng.random(5000) < 0.1] = -1
    codes[rng.random(5000) < 0.02] = -7                            # any negative code skips
    _exact(_counts(rng, 5000, 300, dtype), codes, 600, what="5 000 x 300, 600 groups")


@pytest.mark.parametrize("dtype", DTYPES)
def test_column_lists(dtype):
    rng = np.random.default_rng(4)
    L = engine.group_sums_slice_rows()
    n = 2 * L + 40
    Y, codes = _counts(rng, n, 300, dtype), rng.integers(-1, 3, n)
    full = _exact(Y, codes, 3, what="every column")
    for cols in (rng.permutation(300), np.array([5, 299, 5, 0, 17, 299]), np.array([123])):
        got = _exact(Y, codes, 3, cols=cols, what="cols of length %d" % cols.size)
        assert np.array_equal(got[1], full[1][:, cols])
    count, sums = engine.group_sums(Y, codes, 3, cols=np.zeros(0, dtype=np.int64))
    assert sums.shape == (3, 0) and np.array_equal(count, full[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_sparse_edges(dtype):
    """indices unsorted within rows, explicitly stored zeros, empty rows, a column no row stores, rows of 63 / 64 / 65 / 200 / 257
    stored entries (one batch of lanes, one more, one pass of the wave's unrolled batches, one more)"""
    rng = np.random.default_rng(5)
    n, G = 40, 400
    indptr, indices, data = [0], [], []
    fill = {3: 63, 4: 64, 5: 65, 6: 200, 7: 257, 8: 0, 9: 0, 39: 0}
    for r in range(n):
        k = fill.get(r, int(rng.integers(1, 30)))
        c = rng.permutation(np.delete(np.arange(G), 11))[:k]       # column 11 is never stored; the order within the row is random
        v = rng.integers(1, 51, k).astype(np.float64)
        v[rng.random(k) < 0.1] = 0.0                               # stored zeros
        indices.extend(c.tolist()), data.extend(v.tolist()), indptr.append(len(indices))
    X = sp.csr_matrix((np.asarray(data, dtype=dtype), np.asarray(indices, dtype=np.int32), np.asarray(indptr, dtype=np.int64)), shape=(n, G))
    assert not X.has_sorted_indices and (X.data == 0).any()
    Y = X.toarray()
    codes = rng.integers(0, 3, n)
    codes[[2, 8]] = -1
    C = engine.DeviceCSR.upload(X)
    want = PR.group_sums(Y, codes, 3)
    got = C.group_sums(codes, 3)
    assert _same(got, want) and (got[1][:, 11] == 0).all()
    assert _same(engine.group_sums(C, codes, 3), want) and _same(engine.group_sums(Y, codes, 3), want)
    cols = np.array([11, 0, 399, 0, 200])
    assert _same(C.group_sums(codes, 3, cols=cols), PR.group_sums(Y, codes, 3, cols))
    empty = engine.DeviceCSR.upload(sp.csr_matrix((5, 7), dtype=dtype))                         # nothing stored at all
    count, sums = empty.group_sums(np.array([0, 1, 1, -1, 0]), 2)
    assert list(count) == [2, 2] and sums.shape == (2, 7) and (sums == 0).all()


def test_sparse_column_blocks():
    """B + 1 columns with entries in columns B - 1, B (= the last) and 0: the second block holds one column"""
    B = engine.group_sums_col_block()
    L = engine.group_sums_slice_rows()
    n = L + 2
    rng = np.random.default_rng(6)
    Y = np.zeros((n, B + 1), dtype=np.float32)
    for j in (0, B - 1, B):
        Y[:, j] = rng.integers(0, 51, n)
    codes = rng.integers(0, 2, n) * 2                              # groups 0 and 2 of 3; together more rows than one slice
    codes[:L + 1] = 0
    C = engine.DeviceCSR.upload(sp.csr_matrix(Y))
    want = PR.group_sums(Y, codes, 3)
    assert _same(C.group_sums(codes, 3), want) and _same(engine.group_sums(Y, codes, 3), want)
    assert want[1][0, B] > 0 and want[1][0, B - 1] > 0
    cols = np.array([B, 0, B - 1, B])
    assert _same(C.group_sums(codes, 3, cols=cols), PR.group_sums(Y, codes, 3, cols))


@functools.lru_cache(maxsize=None)
def _general(dtype):
    """70 001 x 300, standard normal values times per-column scales at one entry in ten; 7 groups of very unequal size"""
    rng = np.random.default_rng(7)
    n, G = 70001, 300
    Y = (rng.standard_normal((n, G)) * np.exp(rng.uniform(-3.0, 6.0, G))).astype(dtype)
    Y[rng.random((n, G)) >= 0.1] = 0
    codes = rng.choice(7, n, p=[0.6, 0.3, 0.05, 0.03, 0.015, 0.004, 0.001])
    codes[rng.random(n) < 0.05] = -1
    codes[:3] = [6, -1, 5]
    return Y, codes, PR.group_sums(Y, codes, 7), PR.abs_sums(Y, codes, 7)


def _within_bound(got, want, scale, what):
    count, sums = want
    assert np.array_equal(got[0], count)
    bound = np.maximum(count, 64)[:, None] * U * scale
    err = np.abs(got[1] - sums)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))
    print("%s: worst error / bound = %.3f" % (what, worst))
    assert (err <= bound).all(), what


@pytest.mark.parametrize("dtype", DTYPES)
def test_general_values_within_the_summation_bound(dtype):
    Y, codes, want, scale = _general(dtype)
    assert want[0].min() >= 20 and want[0].max() > 30000
    routes = _routes(Y)
    first = {}
    for name, route in routes.items():
        first[name] = engine.group_sums(route, codes, 7)
        _within_bound(first[name], want, scale, "70 001 x 300 %s, %s" % (np.dtype(dtype).name, name))
    assert _same(first["host"], first["device"])                   # one route's sums: a host array and the same data in HBM
    for name, route in routes.items():                             # a second run: the same bits
        assert _same(engine.group_sums(route, codes, 7), first[name]), name
    cols = np.array([299, 0, 150, 0])
    sub = engine.group_sums(routes["device"], codes, 7, cols=cols)
    _within_bound(sub, (want[0], want[1][:, cols]), scale[:, cols], "cols")
    assert _same(engine.group_sums(Y, codes, 7, cols=cols), sub)
    _within_bound(routes["csr"].group_sums(codes, 7, cols=cols), (want[0], want[1][:, cols]), scale[:, cols], "csr cols")


def test_sums_after_normalize_need_no_column_form():
    rng = np.random.default_rng(8)
    n, G = 700, 500
    K = rng.poisson(0.2, (n, G)).astype(np.float32)
    codes = rng.integers(-1, 40, n)
    C = engine.DeviceCSR.upload(sp.csr_matrix(K))
    assert _same(C.group_sums(codes, 40), PR.group_sums(K, codes, 40))
    C.normalize_log1p()                                            # the values change; no per-column call has been made
    V = engine.download(C.densify())                               # the float32 values the sums are taken over
    got = C.group_sums(codes, 40)
    _within_bound(got, PR.group_sums(V, codes, 40), PR.abs_sums(V, codes, 40), "after normalize_log1p")
    assert _same(C.group_sums(codes, 40), got) and _same(engine.group_sums(V, codes, 40), got)


@pytest.mark.parametrize("dtype", DTYPES)
def test_skipped_rows_enter_nothing(dtype):
    """NaN, Inf and 1e36 in the skipped rows -- the first row of the matrix, the rows around a slice boundary of the long group,
    the last row -- leave the bits of the sums over the other rows alone"""
    L = engine.group_sums_slice_rows()
    rng = np.random.default_rng(9)
    n, G = 3 * L + 50, 130
    Y = (rng.standard_normal((n, G)) * 100.0).astype(dtype)
    codes = np.where(rng.random(n) < 0.8, 0, rng.integers(1, 5, n))
    skip = np.zeros(n, dtype=bool)
    skip[[0, 1, L - 1, L, L + 1, 2 * L, n - 1]] = True
    skip |= rng.random(n) < 0.1
    codes[skip] = -1
    poison = np.array([np.nan, np.inf, -np.inf, 1e36], dtype=dtype)
    Y[skip] = poison[rng.integers(0, 4, (int(skip.sum()), G))]
    keep = ~skip
    clean = engine.group_sums(np.ascontiguousarray(Y[keep]), codes[keep], 5)
    assert np.isfinite(clean[1]).all() and clean[0][0] > 2 * L
    for name, route in _routes(Y, with_csr=False).items():
        assert _same(engine.group_sums(route, codes, 5), clean), name
    Z = Y.copy()
    Z[np.abs(Z) < 50.0] = 0                                        # sparse values: the poison stays, being large or NaN
    S = sp.csr_matrix((Z != 0).astype(dtype))                      # the pattern first (NaN != 0), then the values into it
    at = S.nonzero()
    S.data = Z[at]
    assert np.isnan(S.data).any() and np.isinf(S.data).any()
    want = engine.group_sums(np.ascontiguousarray(Z[keep]), codes[keep], 5)
    assert _same(engine.DeviceCSR.upload(S).group_sums(codes, 5), want)
    assert _same(engine.DeviceCSR.upload(sp.csr_matrix(Z[keep])).group_sums(codes[keep], 5), want)
    _within_bound(want, PR.group_sums(Z[keep], codes[keep], 5), PR.abs_sums(Z[keep], codes[keep], 5), "skipped rows deleted")


def test_the_checks_that_need_a_matrix():
    """pilot_ot_csr_group_sums through ctypes, with a live handle: a code reaching n_groups and a column out of range are named"""
    L = _lib.load()
    C = engine.DeviceCSR.upload(sp.csr_matrix(np.eye(4, 3)))
    count, sums = np.zeros(8, dtype=np.int64), np.zeros((8, 3))
    cp = count.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))

    def call(codes=(0, 1, 0, 1), ng=2, cols=None, n_cols=3):
        codes = np.asarray(codes, dtype=np.int32)
        cols = None if cols is None else np.asarray(cols, dtype=np.int32)
        return L.pilot_ot_csr_group_sums(C.h, _lib.iptr(codes), ng, None if cols is None else _lib.iptr(cols), n_cols, cp, _lib.dptr(sums))
    assert call() == _lib.OK and list(count[:2]) == [2, 2] and np.array_equal(sums[:2], [[1, 0, 1], [0, 1, 0]])
    assert call(codes=(0, 2, 0, 1)) == _lib.EINVAL and b"codes[1]=2" in L.pilot_ot_last_error()
    assert call(cols=(0, 3), n_cols=2) == _lib.EINVAL and b"cols[1]=3" in L.pilot_ot_last_error()
    assert call(cols=(0, -1), n_cols=2) == _lib.EINVAL and b"cols[1]=-1" in L.pilot_ot_last_error()
    assert call(n_cols=2) == _lib.EINVAL and b"n_sel=2" in L.pilot_ot_last_error()
    assert L.pilot_ot_csr_group_sums(C.h, None, 2, None, 3, cp, _lib.dptr(sums)) == _lib.EINVAL and b"NULL" in L.pilot_ot_last_error()
