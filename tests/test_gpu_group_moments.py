"""K12 on the device: engine.group_moments (group_moments_kernel + group_moments_join_kernel) against numpy two-pass float64
moments (tests/limma_restatement.py::group_moments).

Bounds, from the summation order the kernels implement (moments_kernels.hpp), u = 2^-53 = 1.1e-16.  A wave owns one row slice of
one column tile and walks it in chunks of R = 8 rows; every value is first taken relative to the slice's shift K (its first
row), d = t(y) - K.  Per chunk and group: the sum of at most 8 terms (7 u), its mean (2 u more), the squared deviations from that
mean (at most 8 terms: 10 u relative on a sum of non-negative terms), and Chan's update of the running (n, mean, m2).  The slices
are joined by the same update in slice order.  With C chunks per slice and S slices a column's result has passed through at most
C + S updates, each adding at most 3 u |mean - K| to the running mean and 4 u relative to the running m2 (a sum of non-negative
terms, so relative errors do not amplify); the shift returns with one rounding, u |mean|.  To first order

    |mean error| <= (9 + 3 (C + S)) u max|t(y) - K| + u max|t(y)|,
    m2 relative  <= (14 + 4 (C + S)) u + 2 (C + S) 3 u rho,   rho = max|running mean - K| / (between-chunk spread),

where the second m2 term is the running mean's error entering delta^2 n_a n_c / (n_a + n_c); the between-chunk terms carry only
about 1 / R of m2, and with K a row of the data rho is O(1) whatever mean / std is -- that is what the shift is for (a raw
sum(y^2) - n mean^2 would lose (mean / std)^2 u = 1e-8 at mean / std = 1e4).  The host makes slices of at least 128 rows, so
C <= ceil(n / (8 S)) + 1, and S <= 8 CUs / tiles: at the largest case here, n = 70 001 with 2 column tiles, S = 546 and C = 17,
which gives 1.9e-13 max|d| for the mean and 2.5e-13 + 3.7e-13 rho for m2 -- below the worst-case bound of a plain sequential
float64 sum, n u = 7.8e-12.  The tests hold mean to tol max|t(y)| absolute and m2 to tol relative with tol = min(1e-11,
max(n, 64) u): never wider than 1e-11 nor than n u wherever n >= 64 (7.8e-12 at n = 70 001, 2.9e-14 at n = 257), and 64 u =
7.1e-15 at the tiny shapes, where C + S <= 2 and the fixed terms above (14 + 8 + 12 rho) u stay below it for rho <= 3.
expm1 is the device's float64 expm1, within 2 ulp of numpy's: 2 u max|t| on the mean and 4 u sqrt(1 + (mean / std)^2) relative
on m2, inside the same bounds.  Empty groups must be NaN exactly where the restatement's are, a single-row
group's m2 exactly 0, and two runs, and the host and DeviceMatrix routes, must agree to the bit."""
import numpy as np
import pytest

import limma_restatement as LR
from pilot_amd import engine

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


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


def _data(rng, n, G, dtype):
    return np.ascontiguousarray(rng.standard_normal((n, G)) * rng.uniform(0.5, 3.0, G) + rng.uniform(-5.0, 5.0, G), dtype=dtype)


def _codes(rng, n, n_groups):
    if n == 1:
        return np.zeros(1, dtype=np.int64)
    if n == 3:
        return np.array([0, 2, 2])                                 # group 0 one row, group 1 empty
    return rng.integers(-1, n_groups, n)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,G,n_groups", [(1, 1, 1), (3, 5, 3), (257, 255, 2), (257, 256, 2), (257, 257, 2), (70001, 300, 2)])
def test_against_two_pass(dtype, n, G, n_groups):
    rng = np.random.default_rng(n * 1000 + G)
    Y, codes = _data(rng, n, G, dtype), _codes(rng, n, n_groups)
    want = LR.group_moments(Y, codes, n_groups)
    got = engine.group_moments(Y, codes, n_groups)
    _check(got, want, np.abs(Y).max(), "%s %d x %d, %d groups" % (np.dtype(dtype).name, n, G, n_groups), n)
    D = engine.DeviceMatrix.upload(Y)
    assert _same(engine.group_moments(D, codes, n_groups), got)        # the route does not change the bits
    assert _same(engine.group_moments(Y, codes, n_groups), got) and _same(engine.group_moments(D, codes, n_groups), got)
    if n == 3:
        assert list(got[0]) == [1, 0, 2] and np.isnan(got[1][1]).all() and (got[2][0] == 0.0).all()
        assert np.array_equal(got[1][0], Y[0].astype(np.float64))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("start,width", [(4, 131), (3, 130), (1, 257)])
def test_leading_dimension_larger_than_the_columns(dtype, start, width):
    """a column window of a wider matrix in HBM: ld = 400 > width; starts on and off a 16-byte boundary"""
    rng = np.random.default_rng(start)
    W, codes = _data(rng, 1500, 400, dtype), rng.integers(-1, 2, 1500)
    D = engine.DeviceMatrix.upload(W)
    V = engine.device_columns(D, start, start + width)
    view = W[:, start:start + width]
    want = LR.group_moments(view, codes, 2)
    got = engine.group_moments(V, codes, 2)
    _check(got, want, np.abs(view).max(), "window %d:%d of 400 %s" % (start, start + width, np.dtype(dtype).name), 1500)
    assert _same(engine.group_moments(np.ascontiguousarray(view), codes, 2), got)
    cols = np.array([width - 1, 0, 7, 7, 2])
    assert _same(engine.group_moments(V, codes, 2, cols=cols), tuple([got[0]] + [a[:, cols] for a in got[1:]]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cols_in_any_order(dtype):
    rng = np.random.default_rng(8)
    Y, codes = _data(rng, 5000, 700, dtype), rng.integers(-1, 3, 5000)
    cols = rng.permutation(700)[:300]
    assert (np.diff(cols) < 0).any()
    want = LR.group_moments(Y, codes, 3, cols=cols)
    got = engine.group_moments(Y, codes, 3, cols=cols)
    _check(got, want, np.abs(Y).max(), "300 of 700 columns, %s" % np.dtype(dtype).name, 5000)
    full = engine.group_moments(Y, codes, 3)
    # Here a gathered column carries the bits of the full pass.  That is no property of the call: the slice count is
    # min(n // 128, ceil(8 CUs / column tiles)), and the two calls agree only because 5 000 rows give 39 slices for 2 tiles and
    # for 3 on any device of more than 14 CUs.  Each is held to the two-pass reference above whatever the slicing.
    assert _same(got, tuple([full[0]] + [a[:, cols] for a in full[1:]]))
    assert _same(engine.group_moments(engine.DeviceMatrix.upload(Y), codes, 3, cols=cols), got)
    empty = engine.group_moments(Y, codes, 3, cols=np.zeros(0, dtype=np.int64))
    assert np.array_equal(empty[0], full[0]) and empty[1].shape == (3, 0)


def test_all_rows_skipped_and_no_rows():
    rng = np.random.default_rng(1)
    Y = _data(rng, 900, 70, np.float32)
    Y[5, 3] = np.nan                                               # a skipped row's values are never used
    for codes, n_groups in ((np.full(900, -1), 2), (np.full(900, -7), 1)):
        count, mean, m2 = engine.group_moments(Y, codes, n_groups)
        assert (count == 0).all() and np.isnan(mean).all() and np.isnan(m2).all() and mean.shape == (n_groups, 70)
    count, mean, m2 = engine.group_moments(Y[:0], np.zeros(0, dtype=np.int64), 2)
    assert (count == 0).all() and np.isnan(mean).all() and np.isnan(m2).all()
    Y[0, 2] = np.inf                                               # ... nor as a slice's shift when they are not finite
    codes = np.where(np.isin(np.arange(900), [0, 5]), -1, 0)
    _check(engine.group_moments(Y, codes, 1), LR.group_moments(Y, codes, 1), np.abs(Y[np.isfinite(Y)]).max(), "NaN / inf in skipped rows", 900)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_groups", [4, 8])
def test_many_groups(dtype, n_groups):
    rng = np.random.default_rng(n_groups)
    Y = _data(rng, 20011, 261, dtype)
    codes = rng.integers(-1, n_groups, 20011)
    codes[codes == 2] = -1                                         # group 2 empty
    codes[np.flatnonzero(codes == 3)[1:]] = -1                     # group 3 one row
    want = LR.group_moments(Y, codes, n_groups)
    assert want[0][2] == 0 and want[0][3] == 1
    got = engine.group_moments(Y, codes, n_groups)
    _check(got, want, np.abs(Y).max(), "%d groups %s" % (n_groups, np.dtype(dtype).name), 20011)
    if n_groups == 8:                                              # 5 groups take the 8-group kernel as well
        _check(engine.group_moments(Y, np.minimum(codes, 4), 5), LR.group_moments(Y, np.minimum(codes, 4), 5), np.abs(Y).max(), "5 groups", 20011)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_expm1_transform(dtype):
    rng = np.random.default_rng(3)
    Y = np.ascontiguousarray(np.log1p(rng.poisson(rng.lognormal(0.5, 1.2, 333), (9001, 333))), dtype=dtype)
    Y[:, 7] = 0.0
    codes = rng.integers(-1, 2, 9001)
    want = LR.group_moments(Y, codes, 2, transform="expm1")
    got = engine.group_moments(Y, codes, 2, transform="expm1")
    _check(got, want, np.expm1(Y.astype(np.float64)).max(), "expm1 %s" % np.dtype(dtype).name, 9001)
    assert (got[1][:, 7] == 0.0).all() and (got[2][:, 7] == 0.0).all()
    assert _same(engine.group_moments(engine.DeviceMatrix.upload(Y), codes, 2, transform="expm1"), got)
    cols = np.array([300, 7, 12])
    assert _same(engine.group_moments(Y, codes, 2, transform="expm1", cols=cols), tuple([got[0]] + [a[:, cols] for a in got[1:]]))


def test_cancellation_at_mean_over_std_1e4():
    """float32 columns with mean / std = 1e4 over 70 001 rows: a raw-moment kernel is off by (mean / std)^2 u = 1e-8 on m2"""
    rng = np.random.default_rng(4)
    n, G = 70001, 260
    std = rng.uniform(0.5, 2.0, G)
    Y = np.ascontiguousarray(1e4 * std + std * rng.standard_normal((n, G)), dtype=np.float32)
    codes = rng.integers(0, 2, n)
    want = LR.group_moments(Y, codes, 2)
    ratio = want[1] / np.sqrt(want[2] / (want[0][:, None] - 1))
    assert ratio.min() > 9e3
    V = Y.astype(np.float64)
    raw = np.stack([(V[codes == g] ** 2).sum(axis=0) - (codes == g).sum() * V[codes == g].mean(axis=0) ** 2 for g in (0, 1)])
    assert (np.abs(raw - want[2]) / want[2]).max() > 1e-10        # the raw form fails this very bound on the host
    got = engine.group_moments(Y, codes, 2)
    _check(got, want, np.abs(Y).max(), "mean / std = 1e4", n)
