"""K13 on the device: engine.DeviceCSR (csr_kernels.hpp) against numpy on the densified matrix in float64 -- two-pass moments
(tests/limma_restatement.py::group_moments) and tests/trajfit_restatement.py::normalize_log1p -- and the sparse routes of tl.

Bounds, from the summation order the kernels implement, u = 2^-53.

Moments.  A workgroup of 256 threads owns a column with s stored entries.  Thread t adds its entries t, t + 256, ... in order (at
most ceil(s / 256) terms), the 256 partials are joined by a butterfly of 6 steps inside each wave and the 4 wave sums are added in
wave order (3 more): every stored value passes through at most d = ceil(s / 256) + 9 additions, so the computed sum S' obeys
|S' - S| <= d u sum|t(y)| and, after the division by the group's row count n_g >= stored entries,

    |mean error| <= (d + 1) u max|t(y)|.

m2 = sum_stored (t(y) - mean')^2 + (n_g - s_g) mean'^2 is mathematically m2_true + n_g (mean' - mean)^2: the mean's error enters
to second order only, n_g ((d + 1) u max|t|)^2, which is below u^2 n_g d^2 (max|t| / std)^2 m2 / n_g -- 1e-19 relative even at
mean / std = 1e4.  Every term is non-negative, so rounding does not amplify: each term carries 3 u (subtraction, square, fma), the
absent rows' term 3 u, and the summation d u:

    m2 relative <= (d + 6) u.

With s <= n, d + 6 <= n / 256 + 16 <= max(n, 64) for every n >= 1, so the rule of tests/test_gpu_group_moments.py holds here
unchanged: mean to tol max|t(y)| absolute, m2 to tol relative, tol = min(1e-11, max(n, 64) u).  expm1 is the device's float64
expm1, within 2 ulp of numpy's, as in that module.  The same reasoning covers every group: a group's accumulators see only its
own entries.

Normalise.  A row's total over its k stored values: lane l adds entries l, l + 64, ... (ceil(k / 64) terms), then 6 butterfly
steps: relative error (ceil(k / 64) + 6) u on a sum of non-negative counts, below the k u the bound below allows.  Then one
division, one product and the device log1p (ROCm's ocml documents 1 ulp for f64 log1p; the 8 below covers it with the
product, the division and the reference's own rounding), and for float32 storage one rounding, 2^-24:

    f64: relative error <= (k + 8) u per element,        f32: (k + 8) u + 2^-24.

Integer counts have exact totals in any order, so the sparse route must give the bits of the dense kernel."""
import functools

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import limma_restatement as LR
import subgroup_helpers as S
import trajfit_restatement as TR
from pilot_amd import _lib, engine, tl

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
DTYPES = [np.float32, np.float64]


def _tol(n):
    return min(1e-11, max(n, 64) * U)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[1:], b[1:])) and np.array_equal(a[0], b[0])


def _check(got, want, scale, what, n):
    (gc, gm, gq), (wc, wm, wq) = got, want
    assert gc.dtype == np.int64 and np.array_equal(gc, wc), what
    assert gm.shape == wm.shape and gq.shape == wq.shape
    assert np.array_equal(np.isnan(gm), np.isnan(wm)) and np.array_equal(np.isnan(gq), np.isnan(wq)), what
    assert np.array_equal(np.isnan(gm), np.broadcast_to((wc == 0)[:, None], gm.shape)), what
    ok = ~np.isnan(wm)
    e_mean = np.abs(gm - wm)[ok].max(initial=0.0) / scale
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(wq > 0, np.abs(gq - wq) / wq, np.abs(gq - wq))
    e_m2 = rel[ok].max(initial=0.0)
    print("%s: mean err / max|y| = %.3e, m2 rel err = %.3e (tol %.1e)" % (what, e_mean, e_m2, _tol(n)))
    assert e_mean <= _tol(n) and e_m2 <= _tol(n), what
    assert (gq[wc == 1] == 0.0).all(), what                        # one row: exactly 0


def _random_csr(rng, n, G, fill, dtype, positive=False):
    """about ``fill`` of the entries stored, values of either sign (or log1p-scale positive ones)"""
    mask = rng.random((n, G)) < fill
    vals = np.log1p(rng.poisson(3.0, (n, G)) + 1.0) if positive else rng.standard_normal((n, G)) * 2.0 + 1.0
    X = sp.csr_matrix(np.where(mask, vals, 0.0).astype(dtype))
    assert X.dtype == dtype
    return X


def _dense(X):
    return np.asarray(X.toarray())


def _codes(rng, n, n_groups):
    if n == 1:
        return np.zeros(1, dtype=np.int64)
    if n == 3:
        return np.array([0, 2, 2])                                 # group 0 one row, group 1 empty
    return rng.integers(-1, n_groups, n)


def _edges(dtype, seed=5):
    """600 x 400 with: an empty row (7) and an empty column (11), a full column (13), an explicitly stored 0, duplicate entries,
    unsorted indices in every row, a row of 330 stored values (more than five passes of a 64-lane wave), the full column's 600
    entries (more than two passes of the 256-thread workgroup), and more rows than one slice of the transpose"""
    rng = np.random.default_rng(seed)
    n, G = 600, 400
    assert n > engine.csr_slice_rows()
    mask = rng.random((n, G)) < 0.08
    mask[5, :330] = True
    mask[:, 13] = True
    mask[7, :] = False
    mask[:, 11] = False
    vals = rng.standard_normal((n, G)) * 2.0 + 1.0
    vals[np.abs(vals) < 0.01] = 0.5
    indptr, indices, data = [0], [], []
    for i in range(n):
        js = np.flatnonzero(mask[i])[::-1]                         # descending: unsorted for scipy
        v = vals[i, js]
        if i == 2:
            v[0] = 0.0                                             # an explicitly stored zero
        if i in (3, 5):                                            # duplicates: the first stored column twice more (an exact sum in any order)
            js, v = np.r_[js, js[0], js[0]], np.r_[2.0, v[1:], 0.25, -1.5]
        indices += list(js)
        data += list(v)
        indptr.append(len(indices))
    X = sp.csr_matrix((np.asarray(data, dtype=dtype), np.asarray(indices, dtype=np.int32), np.asarray(indptr, dtype=np.int32)), shape=(n, G))
    assert not X.has_canonical_format and (X.data == 0).sum() == 1
    D = _dense(X)
    assert (D[7] == 0).all() and (D[:, 11] == 0).all() and (D[np.arange(n) != 7, 13] != 0).all() and np.diff(X.indptr).max() >= 330
    return X, D


# ---- moments -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,G,n_groups,fill", [(1, 1, 1, 1.0), (1, 1, 1, 0.0), (3, 5, 3, 0.5), (257, 255, 2, 0.1), (257, 256, 2, 0.1),
                                               (257, 257, 2, 0.1), (None, 40, 2, 0.1)])
def test_moments_against_two_pass(dtype, n, G, n_groups, fill):
    n = engine.csr_slice_rows() + 1 if n is None else n             # one slice of the transpose plus one row
    rng = np.random.default_rng(n * 1000 + G)
    X, codes = _random_csr(rng, n, G, fill, dtype), _codes(rng, n, n_groups)
    Y = _dense(X)
    assert (X.nnz > 0) == (fill > 0)
    C = engine.DeviceCSR.upload(X)
    assert C.shape == (n, G) and C.dtype == dtype and C.nnz == X.nnz
    got = C.group_moments(codes, n_groups)
    what = "%s %d x %d, %d groups" % (np.dtype(dtype).name, n, G, n_groups)
    _check(got, LR.group_moments(Y, codes, n_groups), max(float(np.abs(Y).max()), 1e-300), what, n)
    assert _same(engine.group_moments(C, codes, n_groups), got)    # the module-level function forwards; a second call: same bits
    if n == 3:
        assert list(got[0]) == [1, 0, 2] and np.isnan(got[1][1]).all() and (got[2][0] == 0.0).all()
        assert np.array_equal(got[1][0], Y[0].astype(np.float64))
    if n == 257:                                                   # all of a column's stored values in one group, per column
        for j in (0, G // 2, G - 1):
            one = np.where(Y[:, j] != 0, 1, rng.integers(-1, 1, n))
            _check(C.group_moments(one, 2), LR.group_moments(Y, one, 2), np.abs(Y).max(), what + ", column %d in group 1" % j, n)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_groups", [1, 2, 8])
def test_moments_of_the_edge_matrix(dtype, n_groups):
    X, Y = _edges(dtype)
    n, G = Y.shape
    rng = np.random.default_rng(n_groups)
    codes = rng.integers(-1, n_groups, n)
    if n_groups == 8:
        codes[codes == 2] = -1                                     # group 2 empty
        codes[np.flatnonzero(codes == 3)[1:]] = -1                 # group 3 one row
    assert (codes < 0).any()
    C = engine.DeviceCSR.upload(X)
    assert C.nnz == X.nnz - 4                                      # the duplicates were summed; the stored zero stays
    want = LR.group_moments(Y, codes, n_groups)
    got = C.group_moments(codes, n_groups)
    _check(got, want, np.abs(Y).max(), "edges %s, %d groups" % (np.dtype(dtype).name, n_groups), n)
    assert (got[1][:, 11][want[0] > 0] == 0.0).all() and (got[2][:, 11][want[0] > 0] == 0.0).all()     # the empty column
    perm = rng.permutation(G)
    assert _same(C.group_moments(codes, n_groups, cols=perm), tuple([got[0]] + [a[:, perm] for a in got[1:]]))
    sub = np.array([13, 399, 0, 11, 200])
    assert _same(C.group_moments(codes, n_groups, cols=sub), tuple([got[0]] + [a[:, sub] for a in got[1:]]))
    empty = C.group_moments(codes, n_groups, cols=np.zeros(0, dtype=np.int64))
    assert np.array_equal(empty[0], got[0]) and empty[1].shape == (n_groups, 0)
    if n_groups == 2:                                              # a group's result does not depend on its number
        back = C.group_moments(np.where(codes < 0, -1, 1 - codes), 2)
        assert _same(back, (got[0][::-1], got[1][::-1], got[2][::-1]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_expm1_transform(dtype):
    rng = np.random.default_rng(3)
    n, G = 2001, 130
    X = _random_csr(rng, n, G, 0.15, dtype, positive=True)
    Y = _dense(X)
    codes = rng.integers(-1, 2, n)
    C = engine.DeviceCSR.upload(X)
    got = C.group_moments(codes, 2, transform="expm1")
    _check(got, LR.group_moments(Y, codes, 2, transform="expm1"), np.expm1(Y.astype(np.float64)).max(), "expm1 %s" % np.dtype(dtype).name, n)
    cols = np.array([129, 7, 12])
    assert _same(C.group_moments(codes, 2, transform="expm1", cols=cols), tuple([got[0]] + [a[:, cols] for a in got[1:]]))
    one = C.group_moments(np.zeros(n, dtype=np.int32), 1, transform="expm1")       # what highly_variable_genes asks for
    _check(one, LR.group_moments(Y, np.zeros(n, dtype=int), 1, transform="expm1"), np.expm1(Y.astype(np.float64)).max(), "expm1, one group", n)


# K12's slice rule, restated as in tests/test_gpu_group_moments.py (not imported from the code under test): for n <= 1031 and at
# most two column tiles, S = max(1, n // 128) slices, slice s starting at n // S * s + n % S * s // S
def _slice_starts(n):
    assert n <= 1031
    S = max(1, n // 128)
    return np.array([n // S * s + n % S * s // S for s in range(S)])


# (id, storage, transform, the value stored in every skipped row, its least ratio to the used rows' largest |t(y)|)
POISONS = [("f64-1e12", np.float64, None, 1e12, 1e10), ("f32-1e6", np.float32, None, 1e6, 1e4),
           ("f32-max", np.float32, None, float(np.finfo(np.float32).max), 1e36),
           ("f64-expm1-700", np.float64, "expm1", 700.0, 1e12), ("f32-expm1-88", np.float32, "expm1", 88.0, 1e12)]
POISON_IDS = [p[0] for p in POISONS]


@pytest.mark.parametrize("n_groups", [2, 5])
@pytest.mark.parametrize("n,G", [(257, 255), (1024, 256), (1031, 257)])
@pytest.mark.parametrize("poison", POISONS, ids=POISON_IDS)
def test_skipped_rows_on_another_scale(poison, n, G, n_groups):
    """the matrix of tests/test_gpu_group_moments.py::test_skipped_rows_on_another_scale as CSR: the used rows at about 10 % fill,
    every skipped row (the first row of each of K12's slices among them) stored in full with a finite value far above the used
    ones.  K13 is two-pass about the true mean and reads a skipped row's value only to discard it, so the bounds above hold
    unchanged; the dense kernel on the same matrix is held to the same reference, so the two routes agree within twice the bound."""
    _, dtype, transform, value, factor = poison
    rng = np.random.default_rng([n, G, n_groups, POISON_IDS.index(poison[0])])
    codes = rng.integers(-1, n_groups, n)
    codes[_slice_starts(n)] = -1
    skipped = codes < 0
    vals = np.log1p(rng.poisson(3.0, (n, G)) + 1.0) if transform == "expm1" else rng.standard_normal((n, G)) * 2.0 + 1.0
    Y = np.where(rng.random((n, G)) < 0.1, vals, 0.0).astype(dtype)
    Y[skipped] = value
    X = sp.csr_matrix(Y)
    assert X.dtype == dtype and X.nnz == (Y != 0).sum() and skipped[_slice_starts(n)].all() and (~skipped).any()
    assert 0.05 < (Y[~skipped] != 0).mean() < 0.15 and (np.diff(X.indptr)[skipped] == G).all()     # the poison is stored
    t = np.expm1(Y.astype(np.float64)) if transform == "expm1" else Y.astype(np.float64)
    scale = np.abs(t[~skipped]).max()
    assert np.isfinite(t).all() and scale > 0 and np.abs(t[skipped]).min() >= factor * scale
    want = LR.group_moments(Y, codes, n_groups, transform=transform)
    what = "%s %d x %d, %d groups" % (poison[0], n, G, n_groups)
    C = engine.DeviceCSR.upload(X)
    got = C.group_moments(codes, n_groups, transform=transform)
    _check(got, want, scale, what + ", CSR", n)
    assert _same(C.group_moments(codes, n_groups, transform=transform), got)
    _check(engine.group_moments(Y, codes, n_groups, transform=transform), want, scale, what + ", dense", n)
    _check(engine.group_moments(C.densify(), codes, n_groups, transform=transform), want, scale, what + ", densified", n)


def test_cancellation_at_mean_over_std_1e4():
    """float32 columns at 50 % fill over 70 001 rows whose stored values have mean / std = 1e4: a raw-moment form is off by
    (mean / std)^2 u = 1e-8 on the m2 of the groups that hold the stored rows"""
    rng = np.random.default_rng(4)
    n, G = 70001, 6
    std = rng.uniform(0.5, 2.0, G)
    stored = rng.random(n) < 0.5                                   # the same rows in every column: the codes can follow them
    V = np.where(stored[:, None], 1e4 * std + std * rng.standard_normal((n, G)), 0.0).astype(np.float32)
    X = sp.csr_matrix(V)
    codes = np.where(stored, rng.integers(0, 2, n), 2)             # groups 0 and 1: stored rows only; group 2: the rest ...
    codes[np.flatnonzero(stored)[:50]] = 2                         # ... and 50 stored rows
    want = LR.group_moments(V, codes, 3)
    ratio = want[1][:2] / np.sqrt(want[2][:2] / (want[0][:2, None] - 1))
    assert ratio.min() > 9e3
    W = V.astype(np.float64)
    raw = np.stack([(W[codes == g] ** 2).sum(axis=0) - (codes == g).sum() * W[codes == g].mean(axis=0) ** 2 for g in (0, 1, 2)])
    assert (np.abs(raw - want[2]) / want[2]).max() > 1e-10        # the raw form fails this very bound on the host
    got = engine.DeviceCSR.upload(X).group_moments(codes, 3)
    _check(got, want, np.abs(V).max(), "mean / std = 1e4 at 50 % fill", n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_largest_shape_and_reproducibility(dtype):
    """K12's largest shape, 137 slices of the transpose: twice, and after destroy and a fresh upload, the same bits"""
    rng = np.random.default_rng(9)
    n, G = 70001, 300
    mask = rng.random((n, G)) < 0.05
    X = sp.csr_matrix(np.where(mask, rng.standard_normal((n, G)) + 2.0, 0.0).astype(dtype))
    codes = rng.integers(-1, 2, n)
    C = engine.DeviceCSR.upload(X)
    got = C.group_moments(codes, 2)
    _check(got, LR.group_moments(_dense(X), codes, 2), np.abs(X.data).max(), "70 001 x 300 %s" % np.dtype(dtype).name, n)
    assert _same(C.group_moments(codes, 2), got)
    C.close()
    with pytest.raises(ValueError):
        C.group_moments(codes, 2)
    C = engine.DeviceCSR.upload(X)
    assert _same(C.group_moments(codes, 2), got)
    assert np.array_equal(C.column_nnz(), mask.sum(axis=0))


# ---- normalise ---------------------------------------------------------------------------------------------------------------------
def _dense_normalize(Y):
    out = np.empty_like(Y)
    tl._lib_check_normalize(np.ascontiguousarray(Y), np.arange(Y.shape[1], dtype=np.int32), out)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_normalize_counts_bit_for_bit(dtype):
    """integer counts: the bits of pilot_ot_normalize_log1p of the dense matrix (that kernel is older than this module)"""
    rng = np.random.default_rng(12)
    n, G = 301, 700
    K = rng.poisson(0.08, (n, G))
    K[4, :] = 0                                                    # a cell without counts
    K[5, :400] = rng.poisson(3.0, 400) + 1                         # more stored values than one pass of the wave
    for X in (sp.csr_matrix(K.astype(dtype)), sp.csr_matrix(K.astype(np.int64)), sp.csr_matrix(K > 0)):
        want_dtype = dtype if X.dtype == dtype else np.float32     # integer and bool data go up as float32
        C = engine.DeviceCSR.upload(X)
        assert C.dtype == want_dtype
        before = C.group_moments(np.zeros(n, dtype=int), 1)        # (the column form exists now)
        C.normalize_log1p()
        got = engine.download(C.densify())
        want = _dense_normalize(_dense(X).astype(want_dtype))
        assert got.dtype == want_dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
        assert (got[4] == 0).all()
        after = C.group_moments(np.zeros(n, dtype=int), 1)         # normalising dropped the column form: these are the new values
        _check(after, LR.group_moments(want, np.zeros(n, dtype=int), 1), np.abs(want).max(), "after normalize", n)
        assert not _same(before, after)


@pytest.mark.parametrize("dtype", DTYPES)
def test_normalize_against_restatement(dtype):
    rng = np.random.default_rng(13)
    n, G = 300, 500
    mask = rng.random((n, G)) < 0.1
    mask[9, :] = False
    mask[10, :450] = True
    Y = np.where(mask, rng.gamma(2.0, 1.5, (n, G)), 0.0).astype(dtype)
    for target in (1e4, 37.5):
        C = engine.DeviceCSR.upload(sp.csr_matrix(Y)).normalize_log1p(target)
        got = engine.download(C.densify()).astype(np.float64)
        want = TR.normalize_log1p(Y, target)
        k = (Y != 0).sum(axis=1, keepdims=True)
        bound = (k + 8) * U + (2.0 ** -24 if dtype == np.float32 else 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(want > 0, np.abs(got - want) / want, np.abs(got - want))
        print("normalize %s target %g: worst rel err / bound = %.3f" % (np.dtype(dtype).name, target, (rel / bound).max()))
        assert (rel <= bound).all()
        assert (got[9] == 0).all() and (got[~mask] == 0).all()


# ---- column stats and densify ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_column_nnz_and_densify(dtype):
    X, Y = _edges(dtype)
    C = engine.DeviceCSR.upload(X)
    nnz = C.column_nnz()
    assert nnz.dtype == np.int64 and np.array_equal(nnz, (Y != 0).sum(axis=0))
    assert nnz[11] == 0 and nnz[13] == 599 and (X.data == 0).any()
    rng = np.random.default_rng(1)
    for cols in (None, rng.permutation(400), np.array([13, 399, 0, 11, 200]), np.zeros(0, dtype=np.int64)):
        D = C.densify(cols)
        want = Y if cols is None else Y[:, cols]
        assert isinstance(D, engine.DeviceMatrix) and D.shape == want.shape and D.dtype == dtype
        got = engine.download(D)
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8))
    for n, G, fill in ((1, 1, 1.0), (1, 1, 0.0), (3, 5, 0.5), (257, 255, 0.1), (257, 256, 0.1), (257, 257, 0.1)):
        Z = _random_csr(rng, n, G, fill, dtype)
        C = engine.DeviceCSR.upload(Z)
        assert np.array_equal(engine.download(C.densify()), _dense(Z)) and np.array_equal(C.column_nnz(), (_dense(Z) != 0).sum(axis=0))


def test_the_checks_that_need_a_matrix():
    """through ctypes, with a live handle: a code reaching n_groups and a column out of range are named"""
    import ctypes
    L = _lib.load()
    C = engine.DeviceCSR.upload(sp.csr_matrix(np.eye(4, 3)))
    count, mean, m2 = np.zeros(8, dtype=np.int64), np.zeros((8, 3)), np.zeros((8, 3))
    cp = count.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))

    def call(codes=(0, 1, 0, 1), ng=2, cols=None, n_cols=3):
        codes = np.asarray(codes, dtype=np.int32)
        cols = None if cols is None else np.asarray(cols, dtype=np.int32)
        return L.pilot_ot_csr_group_moments(C.h, _lib.iptr(codes), ng, None if cols is None else _lib.iptr(cols), n_cols, 0, cp,
                                            _lib.dptr(mean), _lib.dptr(m2))
    assert call() == _lib.OK
    assert call(codes=(0, 2, 0, 1)) == _lib.EINVAL and b"codes[1]=2" in L.pilot_ot_last_error()
    assert call(cols=(0, 3), n_cols=2) == _lib.EINVAL and b"cols[1]=3" in L.pilot_ot_last_error()
    assert call(n_cols=2) == _lib.EINVAL and b"n_cols" in L.pilot_ot_last_error()
    buf = engine._DeviceBuffer(4 * 3 * 8)
    bad = np.array([0, 3], dtype=np.int32)
    assert L.pilot_ot_csr_densify(C.h, _lib.iptr(bad), 2, buf.ptr) == _lib.EINVAL and b"cols[1]=3" in L.pilot_ot_last_error()
    bad = np.array([1, 1], dtype=np.int32)
    assert L.pilot_ot_csr_densify(C.h, _lib.iptr(bad), 2, buf.ptr) == _lib.EINVAL and b"repeats" in L.pilot_ot_last_error()


# ---- tl ----------------------------------------------------------------------------------------------------------------------------
G1, G2 = S.GROUPS[0], S.GROUPS[1]


@functools.lru_cache(maxsize=None)
def _cohort():
    adata, props, _ = S.cohort(seed=19)
    return adata, props, S.Cohort(sp.csr_matrix(adata.X), adata.obs, adata.var_names)


def _rel(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err, scale = np.abs(got - want)[ok], np.abs(want)[ok]
    worst = float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), err), initial=0.0))
    print("%s: max rel err %.3e (tol %g)" % (what, worst, tol))
    assert worst <= tol, what


def _check_table(res, want, what):
    """the tolerances of tests/test_gpu_diff_expressions.py::_check_table, between two frames"""
    assert list(res.columns) == ["logFC", "AveExpr", "t", "P.Value", "adj.P.Val"] and list(res.index) == list(want.index)
    _rel(res["logFC"], want["logFC"], 1e-11, what + " logFC")
    _rel(res["AveExpr"], want["AveExpr"], 1e-11, what + " AveExpr")
    _rel(res.attrs["df_prior"], want.attrs["df_prior"], 1e-9, what + " df_prior")
    _rel(res.attrs["s2_prior"], want.attrs["s2_prior"], 1e-9, what + " s2_prior")
    _rel(res["t"], want["t"], 1e-9, what + " t")
    for col in ("P.Value", "adj.P.Val"):
        big = want[col].values > 1e-300
        _rel(res[col].values[big], want[col].values[big], 1e-8, what + " " + col)
        assert (res[col].values[~big] <= 1e-300).all()


def test_highly_variable_genes_csr_against_dense():
    """normalised values, 120 top genes.  Both routes hold each mean of expm1 to tol max|t| and each m2 to tol relative with
    tol = max(n, 64) u = 4.5e-13 at 4 000 cells; with max|t| / mean below 1e3 (asserted) that is 1e-9 relative on the means and on
    var / mean, so 1e-9 absolute on its logarithm.  The sets agree when no normalised dispersion lies within 1e-6 of the cut-off
    (asserted on the dense route)."""
    adata, _, csr = _cohort()
    rows = S.cell_values(adata)[1]
    dense = tl._cell_type_values(adata, rows, True)
    want = tl.highly_variable_genes(dense, 120)
    t = np.expm1(dense.astype(np.float64))
    live = t.mean(axis=0) > 0
    assert (t.max(axis=0)[live] / t.mean(axis=0)[live]).max() < 1e3
    dn = want["dispersions_norm"].values
    cutoff = np.sort(dn[~np.isnan(dn)])[::-1][119]
    assert np.nanmin(np.abs(dn - cutoff)[dn != cutoff]) > 1e-6
    C = tl._cell_type_matrix(csr, rows, True)
    assert isinstance(C, engine.DeviceCSR)
    got = tl.highly_variable_genes(C, 120)
    _rel(got["means"], want["means"], 1e-9, "HVG means, CSR against dense")
    assert np.array_equal(np.isnan(got["dispersions"]), np.isnan(want["dispersions"]))
    assert np.nanmax(np.abs(got["dispersions"].values - want["dispersions"].values)) <= 1e-9
    assert np.array_equal(got["highly_variable"].values, want["highly_variable"].values) and want["highly_variable"].sum() >= 100


def test_diff_expressions_csr_against_dense():
    """normalisation on and HVG on; the 'reference' design, whose logFC is a weighted sum of non-negative means (no cancellation:
    asserted away from 0 on the dense route)"""
    adata, props, csr = _cohort()
    want = tl.compute_diff_expressions(adata, S.CELL, props, normalization=True, n_top_genes=120)
    assert len(want) >= 100 and np.abs(want["logFC"].values).min() > 1e-4
    got = tl.compute_diff_expressions(csr, S.CELL, props, normalization=True, n_top_genes=120)
    _check_table(got, want, "CSR against dense")
    pick = [want.index[40], want.index[2], want.index[77]]
    _check_table(tl.compute_diff_expressions(csr, S.CELL, props, selected_genes=pick, normalization=True, n_top_genes=120),
                 tl.compute_diff_expressions(adata, S.CELL, props, selected_genes=pick, normalization=True, n_top_genes=120), "three selected genes")


def test_extract_cells_csr_against_dense():
    """normalised float32 values by two routes whose row totals may differ in the last bits: two float32 ulps, as
    tests/test_gpu_diff_expressions.py::test_extract_cells_frame allows against the restatement"""
    adata, _, csr = _cohort()
    want = tl.extract_cells_from_gene_expression_for_clustering(adata, "sampleID", "cell_types", [S.CELL], n_top_genes=120, highly_variable_genes_=True)
    got = tl.extract_cells_from_gene_expression_for_clustering(csr, "sampleID", "cell_types", [S.CELL], n_top_genes=120, highly_variable_genes_=True)
    assert list(got.columns) == list(want.columns) and len(got.columns) > 100 and list(got["sampleID"]) == list(want["sampleID"])
    a, b = got.drop(columns="sampleID").to_numpy(), want.drop(columns="sampleID").to_numpy()
    assert a.dtype == np.float32 == b.dtype and np.abs(a - b).max() <= 2.4e-7 * np.abs(b).max()
    plain = tl.extract_cells_from_gene_expression_for_clustering(csr, "sampleID", "cell_types", [S.CELL], normalization=False)
    assert np.array_equal(plain.drop(columns="sampleID").to_numpy(), S.cell_values(adata)[0])


class _Adata:
    def __init__(self, X, obs, var_names, uns):
        self.X, self.obs, self.var_names, self.uns = X, obs, var_names, uns


def test_nothing_densifies_on_the_host(monkeypatch):
    """a sparse adata.X whose toarray / todense raise goes through every gene-level entry point"""
    rng = np.random.default_rng(21)
    n_samples, n_genes = 30, 60
    sample = np.repeat(np.arange(n_samples), rng.integers(8, 20, n_samples))
    ctype = rng.choice(["T", "B"], sample.size, p=[0.6, 0.4])
    time = rng.permutation(n_samples)
    lam = rng.gamma(0.5, 2.0, n_genes)[None, :] * np.exp(np.outer(time[sample] / n_samples, rng.normal(0, 2, n_genes)))
    X = sp.csr_matrix(rng.poisson(lam).astype(np.float32))
    obs = pd.DataFrame({"cell_types": ctype, "sampleID": ["s%d" % s for s in sample]})
    orders = pd.DataFrame({"sampleID": ["s%d" % s for s in np.argsort(time)], "Time_score": np.arange(1, n_samples + 1)})
    props = pd.DataFrame({"sampIeD": ["s%d" % s for s in range(n_samples)], "Predicted_Labels": [G1, G2] * (n_samples // 2)})
    ad = _Adata(X, obs, ["g%d" % i for i in range(n_genes)], dict(orders=orders))

    def boom(self, *a, **k):
        raise AssertionError("the sparse matrix was made dense on the host")
    for cls in {type(X), sp.csr_matrix, sp.csc_matrix}:
        monkeypatch.setattr(cls, "toarray", boom)
        monkeypatch.setattr(cls, "todense", boom)
    with pytest.raises(AssertionError):
        X[:2].toarray()
    tables = {c: tl.genes_importance(ad, c, p_value=1) for c in ("T", "B")}
    assert len(tables["T"]) > 5 and len(tables["B"]) > 5
    curves, noised, names = tl.get_noised_curves(ad, "T", tables["T"], table_filter_thr=0.0, table_filter_pval_thr=1.0)
    assert curves.shape[0] == noised.shape[0] > 5
    res = tl.compute_diff_expressions(ad, "T", props, group1=G1, group2=G2, normalization=True, n_top_genes=30)
    assert len(res) >= 20
    common = [g for g in tables["T"]["Gene ID"] if g in set(tables["B"]["Gene ID"])][:3]
    assert common
    frame = tl.infer_gene_cluster_differentiation(ad, tables, gene_list=common, n_points=10, end=n_samples, n_bootstraps=4, random_state=0)
    assert len(frame) == 2 * len(common)
