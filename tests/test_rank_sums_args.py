"""Rank sums (K21), the parts that need no device.  engine.rank_sum_z and engine.kruskal_h, fed by the restatement
(tests/rank_sums_restatement.py), against scipy.stats.mannwhitneyu(use_continuity=False, method="asymptotic") and
scipy.stats.kruskal: U exactly, z, H and the p-values at rtol = 1e-12 (the expressions agree bit for bit here; the margin only
frees the order of operations in the tail).  pilot_ot_rank_sums and pilot_ot_csr_rank_sums refuse every bad argument before any
HIP call (a box without a device returns PILOT_OT_EHIP from the first HIP call, so PILOT_OT_EINVAL / ENOTSUP shows the check came
first); engine.rank_sums, DeviceCSR.rank_sums and the tl entry points raise before the library is touched (its handle is replaced
by an object that fails the test on any use)."""
import ctypes

import numpy as np
import pandas as pd
import pytest
from scipy import stats

import rank_sums_restatement as RR
import subgroup_helpers as S
from pilot_amd import _lib, engine, tl

LLP = ctypes.POINTER(ctypes.c_longlong)


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())


# ---- the host tail against scipy --------------------------------------------------------------------------------------------------
def _poisson(rng, shape):
    return rng.poisson(0.8, shape).astype(np.float64)


def _log_normalised(rng, shape):
    counts = rng.poisson(rng.gamma(2.0, 0.7, (1, shape[1])), shape).astype(np.float64)
    return np.log1p(counts * 1e4 / np.maximum(counts.sum(axis=1, keepdims=True), 1.0))


def _normals(rng, shape):
    return rng.standard_normal(shape)


def _rounded(rng, shape):
    return np.round(rng.standard_normal(shape), 1)


KINDS = {"poisson": _poisson, "log-normalised": _log_normalised, "normals": _normals, "rounded normals": _rounded}


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("n,n_groups", [(40, 2), (151, 3), (400, 5)])
def test_host_tail_against_scipy(kind, n, n_groups):
    rng = np.random.default_rng(n + len(kind))
    Y = KINDS[kind](rng, (n, 12))
    codes = rng.integers(0, n_groups, n)
    codes[rng.random(n) < 0.15] = -1
    used = codes >= 0
    count, R, ties = RR.rank_sums(Y, codes, n_groups)
    assert count.min() >= 2
    z, U = engine.rank_sum_z(count, R, ties, tie_correct=True)
    for g in range(n_groups):
        for j in range(Y.shape[1]):
            want = stats.mannwhitneyu(Y[codes == g, j], Y[used & (codes != g), j], use_continuity=False, method="asymptotic")
            assert U[g, j] == want.statistic
            np.testing.assert_allclose(2.0 * stats.norm.sf(abs(z[g, j])), want.pvalue, rtol=1e-12, atol=0)
            assert (z[g, j] > 0) == (want.statistic > count[g] * (count.sum() - count[g]) / 2) or z[g, j] == 0
    np.testing.assert_allclose(z, RR.z_scores(count, R, ties, True), rtol=1e-12, atol=0)
    plain = engine.rank_sum_z(count, R, ties)[0]
    np.testing.assert_allclose(plain, RR.z_scores(count, R, ties, False), rtol=1e-12, atol=0)
    assert (np.abs(plain) <= np.abs(z)).all()                       # the tie term only lowers the variance
    H, p, df = engine.kruskal_h(count, R, ties)
    assert df == n_groups - 1
    for j in range(Y.shape[1]):
        want = stats.kruskal(*(Y[codes == g, j] for g in range(n_groups)))
        np.testing.assert_allclose(H[j], want.statistic, rtol=1e-12, atol=0)
        np.testing.assert_allclose(p[j], want.pvalue, rtol=1e-12, atol=0)


def test_host_tail_edges():
    Y = np.array([[1.0, 2.0, 0.0], [1.0, 0.0, 0.0], [1.0, 5.0, 3.0], [1.0, 5.0, 0.0], [1.0, 1.0, 0.0], [1.0, 7.0, 0.0]])
    codes = np.array([0, 0, 2, 2, 2, 0])                            # group 1 has no rows
    count, R, ties = RR.rank_sums(Y, codes, 3)
    assert list(count) == [3, 0, 3] and list(ties) == [6 ** 3 - 6, 6, 5 ** 3 - 5]
    for correct in (False, True):
        z, U = engine.rank_sum_z(count, R, ties, tie_correct=correct)
        assert (z[:, 0] == 0).all() and (z[1] == 0).all()           # an all-equal column; an empty group
        assert np.isfinite(z).all() and z[0, 1] == -z[2, 1] != 0
        np.testing.assert_array_equal(U[:, 0], [4.5, 0.0, 4.5])
    H, p, df = engine.kruskal_h(count, R, ties)
    assert df == 1 and np.isnan(H[0]) and np.isnan(p[0])
    want = stats.kruskal(Y[codes == 0, 1], Y[codes == 2, 1])
    np.testing.assert_allclose([H[1], p[1]], [want.statistic, want.pvalue], rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        engine.rank_sum_z(count, R[:2], ties)
    with pytest.raises(ValueError):
        engine.kruskal_h(count, R, ties[:2])


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
GOOD = dict(y=True, dtype=0, n=6, total=5, ld=5, codes=[0, 1, 0, 1, -1, 0], ng=2, cols=None, n_cols=5, count=True, rank2=True, ties=True)


def _dense_call(**kw):
    a = dict(GOOD)
    a.update(kw)
    L = _lib.load()
    Y = np.zeros((6, 8), dtype=np.float32)
    codes = None if a["codes"] is None else np.ascontiguousarray(a["codes"], dtype=np.int32)
    cols = None if a["cols"] is None else np.ascontiguousarray(a["cols"], dtype=np.int32)
    groups = max(8, min(a["ng"], 1024))
    count, rank2, ties = np.zeros(groups, dtype=np.int64), np.zeros((groups, 8), dtype=np.int64), np.zeros(8, dtype=np.int64)
    bad_row, bad_col = ctypes.c_longlong(5), ctypes.c_int(5)
    rc = L.pilot_ot_rank_sums(ctypes.c_void_p(Y.ctypes.data) if a["y"] else None, 0, a["dtype"], a["n"], a["total"], a["ld"],
                              None if codes is None else _lib.iptr(codes), a["ng"], None if cols is None else _lib.iptr(cols),
                              a["n_cols"], _lib.lptr(count) if a["count"] else None, _lib.lptr(rank2) if a["rank2"] else None,
                              _lib.lptr(ties) if a["ties"] else None, ctypes.byref(bad_row), ctypes.byref(bad_col))
    assert bad_row.value == -1 and bad_col.value == -1
    return rc, L.pilot_ot_last_error(), (count, rank2, ties)


@pytest.mark.parametrize("bad,fragment", [
    (dict(y=False), b"NULL"), (dict(codes=None), b"NULL"), (dict(count=False), b"NULL"), (dict(rank2=False), b"NULL"),
    (dict(ties=False), b"NULL"),
    (dict(n=-1), b"n=-1"),
    (dict(total=0, n_cols=0, ld=0), b"n_cols_total=0"),
    (dict(ld=4), b"ld=4"),
    (dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"),
    (dict(ng=0), b"n_groups"), (dict(ng=-3), b"n_groups"), (dict(ng=1025), b"n_groups"),
    (dict(n_cols=-1, cols=[0]), b"n_sel=-1"),
    (dict(n_cols=4), b"n_sel=4"),
    (dict(cols=[0, 5], n_cols=2), b"outside [0, 5)"),
    (dict(cols=[-1], n_cols=1), b"outside [0, 5)"),
    (dict(codes=[0, 1, 2, 1, -1, 0]), b"codes[2]=2"),
])
def test_dense_entry_point_refuses_before_any_hip_call(bad, fragment):
    rc, msg, _ = _dense_call(**bad)
    assert rc == _lib.EINVAL and fragment in msg, (bad, msg)


def test_too_many_used_rows_are_refused_before_any_hip_call():
    L = _lib.load()
    n = 2 ** 21
    Y = np.zeros((n, 1), dtype=np.float32)
    codes = np.zeros(n, dtype=np.int32)
    count, rank2, ties = np.zeros(1, dtype=np.int64), np.zeros((1, 1), dtype=np.int64), np.zeros(1, dtype=np.int64)
    rc = L.pilot_ot_rank_sums(ctypes.c_void_p(Y.ctypes.data), 0, 0, n, 1, 1, _lib.iptr(codes), 1, None, 1, _lib.lptr(count),
                              _lib.lptr(rank2), _lib.lptr(ties), None, None)
    assert rc == _lib.ENOTSUP and b"used rows" in L.pilot_ot_last_error()


def test_good_arguments_get_as_far_as_the_device():
    for kw in (dict(), dict(ng=1024), dict(cols=[4, 0, 4], n_cols=3), dict(ld=8)):
        rc, msg, _ = _dense_call(**kw)
        assert rc == (_lib.OK if _lib.device_count() > 0 else _lib.EHIP), (kw, msg)


def test_what_needs_no_device_needs_none():
    """no selected column, or no used row: the counts (and zeros) come back without a device"""
    rc, msg, out = _dense_call(cols=[0], n_cols=0)
    assert rc == _lib.OK and list(out[0][:2]) == [3, 2], msg
    rc, msg, out = _dense_call(codes=[-1] * 6)
    assert rc == _lib.OK and not out[0].any() and not out[1].any() and not out[2].any(), msg


def test_sparse_entry_point_refuses_what_it_can_judge_without_a_matrix():
    L = _lib.load()
    count, rank2, ties = np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64)
    codes = np.zeros(4, dtype=np.int32)

    def call(ng=2, n_cols=1):
        return L.pilot_ot_csr_rank_sums(None, _lib.iptr(codes), ng, None, n_cols, _lib.lptr(count), _lib.lptr(rank2), _lib.lptr(ties),
                                        None, None)
    for ng in (0, -1, 1025):
        assert call(ng=ng) == _lib.EINVAL and b"n_groups" in L.pilot_ot_last_error()
    assert call(n_cols=-1) == _lib.EINVAL and b"n_cols=-1" in L.pilot_ot_last_error()
    assert call() == _lib.EINVAL and b"NULL" in L.pilot_ot_last_error()


def test_constants_and_symbols():
    L = _lib.load()
    w, W, T = engine.rank_sums_limits()
    assert (w, W, T) == (L.pilot_ot_rank_sums_wave_max(), L.pilot_ot_rank_sums_wg_max(), L.pilot_ot_rank_sums_sort_tile())
    assert w == 64 and W & (W - 1) == 0 and T & (T - 1) == 0 and w < W
    assert 16 * max(W, T) + 12 * 1024 + 8 <= 160 * 1024            # float64 records and 1024 groups' accumulators within the LDS
    for name in ("pilot_ot_rank_sums", "pilot_ot_csr_rank_sums", "pilot_ot_rank_sums_wave_max", "pilot_ot_rank_sums_wg_max",
                 "pilot_ot_rank_sums_sort_tile"):
        assert name in _lib.SYMBOLS


# ---- engine ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def shell(no_library):
    """a DeviceCSR of 6 x 5 around a handle that must never be used"""
    C = engine.DeviceCSR(ctypes.c_void_p(0x1000), (6, 5), np.float32, 7)
    yield C
    C.h = None                                                     # (nothing to destroy)


CODES = np.array([0, 1, 0, 1, -1, 0])
BAD_ARGS = [
    dict(codes=CODES[:5]),
    dict(codes=CODES.reshape(2, 3)),
    dict(codes=CODES.astype(np.float64)),
    dict(codes=np.array([0, 1, 2, 1, -1, 0])),
    dict(n_groups=0), dict(n_groups=1025), dict(n_groups=2.5), dict(n_groups=True),
    dict(cols=[0, 5]), dict(cols=[-1]), dict(cols=[[0, 1]]), dict(cols=[0.0]),
]


@pytest.mark.parametrize("kwargs", BAD_ARGS)
def test_rank_sums_argument_errors(shell, kwargs):
    args = dict(codes=CODES, n_groups=2)
    args.update(kwargs)
    with pytest.raises(ValueError):
        engine.rank_sums(np.zeros((6, 5), dtype=np.float32), **args)
    with pytest.raises(ValueError):
        shell.rank_sums(**args)
    with pytest.raises(ValueError):                                # the module-level function forwards a DeviceCSR
        engine.rank_sums(shell, **args)


def test_rank_sums_matrix_arguments_and_row_limit(shell):
    for Y in (np.zeros((6, 5), dtype=np.int32), np.zeros(6, dtype=np.float32), np.zeros((5, 6), dtype=np.float32).T, [[0.0] * 5] * 6):
        with pytest.raises(ValueError):
            engine.rank_sums(Y, CODES, 2)
    D = engine.DeviceMatrix(0x1000, 6, shape=(6, 5), dtype=np.float32)
    with pytest.raises(ValueError):
        engine.rank_sums(engine.device_columns(D, 1, 4), CODES, 2, cols=[3])
    for route in (D, engine.device_columns(D, 1, 4), np.zeros((6, 5))):    # every check passed: the call is the first use of the library
        with pytest.raises(AssertionError, match="touched"):
            engine.rank_sums(route, CODES, 1024)
    with pytest.raises(AssertionError, match="touched"):
        shell.rank_sums(CODES, 600, cols=[4, 0, 4])
    n = 2 ** 21 + 5
    big = engine.DeviceMatrix(0x1000, n, shape=(n, 1), dtype=np.float32)
    codes = np.zeros(n, dtype=np.int32)
    with pytest.raises(NotImplementedError, match="used rows"):
        engine.rank_sums(big, codes, 1)
    codes[:6] = -1                                                 # 2^21 - 1 used rows: allowed
    with pytest.raises(AssertionError, match="touched"):
        engine.rank_sums(big, codes, 1)


# ---- tl ---------------------------------------------------------------------------------------------------------------------------
class _Adata:
    def __init__(self, X, obs, var_names):
        self.X, self.obs, self.var_names, self.uns = X, obs, var_names, {}


def _clustered():
    obs = pd.DataFrame({"cluster": pd.Categorical(["0", "1", "0", "2", "1", "0"], categories=["0", "1", "2", "3"])})
    return _Adata(np.zeros((6, 4), dtype=np.float32), obs, ["a", "b", "c", "d"])


@pytest.mark.parametrize("kwargs,fragment", [
    (dict(method="t-test"), "t-test"),
    (dict(method="logreg"), "logreg"),
    (dict(groupby="nowhere"), "nowhere"),
    (dict(groups=["0", "7"]), "7"),
    (dict(groups="0"), "list"),
    (dict(reference="9"), "9"),
    (dict(groups=["3", "0"]), "without cells"),                     # a category that no cell carries
    (dict(reference="3"), "without cells"),
    (dict(groups=["1"], reference="1"), "nothing to test"),
    (dict(corr_method="holm"), "holm"),
    (dict(genes=["a", "zz"]), "zz"),
    (dict(n_genes=0), "n_genes"),
])
def test_rank_genes_groups_argument_errors(no_library, kwargs, fragment):
    args = dict(groupby="cluster")
    args.update(kwargs)
    ad = _clustered()
    with pytest.raises(ValueError, match=fragment):
        tl.rank_genes_groups(ad, **args)
    assert ad.uns == {}


def test_rank_genes_groups_one_group_has_no_rest(no_library):
    ad = _clustered()
    ad.obs = pd.DataFrame({"cluster": ["x"] * 6})
    with pytest.raises(ValueError, match="every cell"):
        tl.rank_genes_groups(ad, "cluster")


def test_sub_group_tests_argument_errors(no_library):
    adata, props, _ = S.cohort(n_cells=300, n_genes=12, n_shifted=2)
    with pytest.raises(ValueError, match="both"):
        tl.wilcoxon_diff_expressions(adata, S.CELL, props, group1="Tumor 1", group2="Tumor 1")
    with pytest.raises(ValueError, match="Tumor 9"):
        tl.wilcoxon_diff_expressions(adata, S.CELL, props, group2="Tumor 9")
    with pytest.raises(KeyError):
        tl.wilcoxon_diff_expressions(adata, S.CELL, props, selected_genes=["g001", "nope"])
    with pytest.raises(KeyError):
        tl.kruskal_diff_expressions(adata, S.CELL, props[props["sampIeD"] != "s04"])
    with pytest.raises(ValueError, match="Tumor 9"):
        tl.kruskal_diff_expressions(adata, S.CELL, props, groups=["Tumor 1", "Tumor 9"])
    with pytest.raises(ValueError, match="twice"):
        tl.kruskal_diff_expressions(adata, S.CELL, props, groups=["Tumor 1", "Tumor 1"])
    with pytest.raises(ValueError, match="at least two"):
        tl.kruskal_diff_expressions(adata, S.CELL, props, groups=["Tumor 1"])
    one = props.assign(Predicted_Labels="same")
    with pytest.raises(ValueError, match="one label"):
        tl.kruskal_diff_expressions(adata, S.CELL, one)
