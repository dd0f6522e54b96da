"""K12 on the device: engine.group_moments (group_moments_kernel + group_moments_join_kernel) against numpy two-pass float64
moments (tests/limma_restatement.py::group_moments).

Bounds, from the summation order the kernels implement (moments_kernels.hpp), u = 2^-53 = 1.1e-16.  A wave owns one row slice of
one column tile and walks it in chunks of R = 8 rows; every value is first taken relative to the slice's shift K (its first
USED row, code >= 0; a skipped row never sets it), d = t(y) - K.  Per chunk and group: the sum of at most 8 terms (7 u), its mean (2 u more), the squared deviations from that
mean (at most 8 terms: 10 u relative on a sum of non-negative terms), and Chan's update of the running (n, mean, m2).  The slices
are joined by the same update in slice order.  With C chunks per slice and S slices a column's result has passed through at most
C + S updates, each adding at most 3 u |mean - K| to the running mean and 4 u relative to the running m2 (a sum of non-negative
terms, so relative errors do not amplify); the shift returns with one rounding, u |mean|.  To first order

    |mean error| <= (9 + 3 (C + S)) u max|t(y) - K| + u max|t(y)|,
    m2 relative  <= (14 + 4 (C + S)) u + 2 (C + S) 3 u rho,   rho = max|running mean - K| / (between-chunk spread),

where the second m2 term is the running mean's error entering delta^2 n_a n_c / (n_a + n_c); the between-chunk terms carry only
about 1 / R of m2.  K is the slice's first used row and rho is measured between that row and each group's running mean, so rho
is O(1), whatever mean / std is, only when the groups of one call lie within a few standard deviations of each other's scale
(one shift serves every group; groups that lie far apart are outside these bounds and are not tested) -- that is what the shift
is for (a raw sum(y^2) - n mean^2 would lose (mean / std)^2 u = 1e-8 at mean / std = 1e4).  A skipped row may hold anything,
on any scale: the tests below fill the skipped rows, every slice's first row among them, with values 1e4 to 1e36 times the
used ones and hold the results to the same bounds.  The host makes slices of at least 128 rows, so
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


# ---- skipped rows on another scale ---------------------------------------------------------------------------------------------
# The host's slice rule, restated (not imported): min(n // 128, ceil(8 CUs / column tiles)) slices, so for n <= 1031 and at most
# two column tiles (<= 512 selected columns) S = max(1, n // 128) on any device of two or more CUs; slice s starts at
# n // S * s + n % S * s // S.
def _slice_starts(n):
    assert n <= 1031
    S = max(1, n // 128)
    return np.array([n // S * s + n % S * s // S for s in range(S)] + [n])


# (id, storage, transform, the value in every skipped row, its least ratio to the used rows' largest |t(y)|)
POISONS = [("f64-1e12", np.float64, None, 1e12, 1e10), ("f32-1e6", np.float32, None, 1e6, 1e4),
           ("f32-max", np.float32, None, float(np.finfo(np.float32).max), 1e36),
           ("f64-expm1-700", np.float64, "expm1", 700.0, 1e12), ("f32-expm1-88", np.float32, "expm1", 88.0, 1e12)]
POISON_IDS = [p[0] for p in POISONS]


def _t(Y, transform):
    V = np.asarray(Y, dtype=np.float64)
    return np.expm1(V) if transform == "expm1" else V


def _used_values(rng, n, G, dtype, transform):
    if transform == "expm1":                                       # log1p-scale counts, as highly_variable_genes sees them
        return np.ascontiguousarray(np.log1p(rng.poisson(rng.lognormal(0.5, 1.2, G), (n, G))), dtype=dtype)
    return _data(rng, n, G, dtype)


def _poisoned(rng, n, G, dtype, transform, poison, factor, codes):
    """used rows from the module's distributions, every skipped row filled with ``poison``; the premises asserted; returns
    (Y, the largest |t(y)| over the used rows)"""
    Y = _used_values(rng, n, G, dtype, transform)
    skipped = codes < 0
    Y[skipped] = poison
    assert skipped[_slice_starts(n)[:-1]].all() and (~skipped).any()                 # every slice's first row is a skipped one
    t = _t(Y, transform)
    scale = np.abs(t[~skipped]).max()
    assert np.isfinite(t).all() and scale > 0 and np.abs(t[skipped]).min() >= factor * scale
    return Y, scale


@pytest.mark.parametrize("n_groups", [1, 2, 3, 5])                 # the 1-, 2-, 4- and 8-group kernels
@pytest.mark.parametrize("n,G", [(n, G) for n in (257, 1024, 1031) for G in (255, 256, 257)])
@pytest.mark.parametrize("poison", POISONS, ids=POISON_IDS)
def test_skipped_rows_on_another_scale(poison, n, G, n_groups):
    """every skipped row, each slice's first row among them, holds a finite value far above the used rows: by every route Y can
    arrive the result is the two-pass reference's within the module's bounds.  A shift taken from the slice's first row whatever
    its code fails this: replayed on the host, 1e-5 on the mean and on m2 for 1e12 in float64 storage, 5e-12 / 1.5e-11 for 1e6
    in float32 storage at n = 257 (tol 2.9e-14), and nothing left at all of float32's largest value."""
    _, dtype, transform, value, factor = poison
    rng = np.random.default_rng([n, G, n_groups, POISON_IDS.index(poison[0])])
    codes = rng.integers(-1, n_groups, n)
    codes[_slice_starts(n)[:-1]] = -1
    Y, scale = _poisoned(rng, n, G, dtype, transform, value, factor, codes)
    what = "%s %d x %d, %d groups" % (poison[0], n, G, n_groups)
    want = LR.group_moments(Y, codes, n_groups, transform=transform)
    got = engine.group_moments(Y, codes, n_groups, transform=transform)
    _check(got, want, scale, what + ", host array", n)
    D = engine.DeviceMatrix.upload(Y)
    assert _same(engine.group_moments(D, codes, n_groups, transform=transform), got)
    assert _same(engine.group_moments(Y, codes, n_groups, transform=transform), got)
    # a window of a wider matrix: ld = G + 11 > G, the window's start 3 elements (12 or 24 bytes) off a 16-byte boundary
    W = np.ascontiguousarray(rng.standard_normal((n, G + 11)), dtype=dtype)
    W[codes < 0] = value
    W[:, 3:3 + G] = Y
    V = engine.device_columns(engine.DeviceMatrix.upload(W), 3, 3 + G)
    assert V.ld > G and (3 * np.dtype(dtype).itemsize) % 16 != 0
    win = engine.group_moments(V, codes, n_groups, transform=transform)
    _check(win, want, scale, what + ", window", n)
    assert _same(win, got)                                         # the same n and columns: the same slices
    cols = rng.permutation(G)[:G // 2 + 3]
    assert (np.diff(cols) < 0).any()
    sub = engine.group_moments(D, codes, n_groups, transform=transform, cols=cols)
    _check(sub, LR.group_moments(Y, codes, n_groups, transform=transform, cols=cols), scale, what + ", cols", n)
    assert _same(engine.group_moments(Y, codes, n_groups, transform=transform, cols=cols), sub)
    # one column tile here against two above, yet the same max(1, n // 128) slices by the rule restated above: the same bits
    assert _same(sub, tuple([got[0]] + [a[:, cols] for a in got[1:]]))


@pytest.mark.parametrize("poison", POISONS[:3], ids=POISON_IDS[:3])
def test_runs_of_skipped_rows(poison):
    """n = 1031, 8 slices starting at 0, 128, 257, 386, 515, 644, 773, 902.  Rows 250:390 are skipped: slice 2 contributes nothing
    and the run spills into both neighbours.  Slice 4 has only its last row used, slice 6 only its second.  Group 2 is that second
    row alone (m2 == 0.0 exactly, the mean the row itself), group 3 is empty (NaN)."""
    _, dtype, transform, value, factor = poison
    n, G, n_groups = 1031, 257, 4
    starts = _slice_starts(n)
    assert list(starts) == [0, 128, 257, 386, 515, 644, 773, 902, 1031]
    rng = np.random.default_rng(POISON_IDS.index(poison[0]))
    codes = rng.integers(-1, 2, n)
    codes[starts[:-1]] = -1
    codes[250:390], codes[249], codes[390] = -1, 0, 1
    codes[starts[4]:starts[5]] = -1
    codes[starts[5] - 1] = 0
    codes[starts[6]:starts[7]] = -1
    codes[starts[6] + 1] = 2
    assert (codes[250:390] < 0).all() and codes[249] >= 0 and codes[390] >= 0 and 250 < starts[2] and starts[3] < 390
    assert (codes[starts[4]:starts[5]] >= 0).sum() == 1 and (codes[starts[6]:starts[7]] >= 0).sum() == 1
    Y, scale = _poisoned(rng, n, G, dtype, transform, value, factor, codes)
    want = LR.group_moments(Y, codes, n_groups)
    assert want[0][2] == 1 and want[0][3] == 0 and want[0][0] > 100 and want[0][1] > 100
    got = engine.group_moments(Y, codes, n_groups)
    _check(got, want, scale, "runs of skipped rows, %s" % poison[0], n)
    assert (got[2][2] == 0.0).all() and np.array_equal(got[1][2], Y[starts[6] + 1].astype(np.float64))
    assert np.isnan(got[1][3]).all() and np.isnan(got[2][3]).all()
    assert _same(engine.group_moments(engine.DeviceMatrix.upload(Y), codes, n_groups), got)
    # the single row as a group of its own in the 2-group kernel, everything else skipped but one far slice
    lone = np.full(n, -1)
    lone[starts[6] + 1] = 1
    lone[5:100] = 0
    Y2 = Y.copy()
    Y2[lone < 0] = value
    got = engine.group_moments(Y2, lone, 2)
    _check(got, LR.group_moments(Y2, lone, 2), np.abs(Y2[lone >= 0].astype(np.float64)).max(), "a lone row, %s" % poison[0], n)
    assert got[0][1] == 1 and (got[2][1] == 0.0).all() and np.array_equal(got[1][1], Y2[starts[6] + 1].astype(np.float64))


@pytest.mark.parametrize("poison", POISONS[:2], ids=POISON_IDS[:2])
def test_first_used_row_not_finite_in_one_column(poison):
    """the first used row of slice 3 holds +inf in column 100 alone, below poisoned skipped rows: that column's shift is 0 and
    its results are not asserted (a non-finite value in a used row is outside the contract); every other column, the three that
    share its lane included, is held to the bounds"""
    _, dtype, transform, value, factor = poison
    n, G, n_groups, j = 1031, 257, 2, 100
    starts = _slice_starts(n)
    rng = np.random.default_rng(7 + POISON_IDS.index(poison[0]))
    codes = rng.integers(-1, n_groups, n)
    codes[starts[:-1]] = -1
    codes[starts[3]:starts[3] + 3] = -1
    first = starts[3] + 3
    codes[first] = 1
    Y, scale = _poisoned(rng, n, G, dtype, transform, value, factor, codes)
    Y[first, j] = np.inf
    assert (codes[starts[3]:first] < 0).all() and (Y[starts[3]:first] == dtype(value)).all() and np.isinf(Y[first]).sum() == 1
    keep = np.arange(G) != j
    want = LR.group_moments(np.ascontiguousarray(Y[:, keep]), codes, n_groups)
    for route in (Y, engine.DeviceMatrix.upload(Y)):
        count, mean, m2 = engine.group_moments(route, codes, n_groups)
        _check((count, mean[:, keep], m2[:, keep]), want, scale, "+inf in a first used row, %s" % poison[0], n)
