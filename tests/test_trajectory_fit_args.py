"""Trajectory model fits (K9): argument checks of the C ABI and of the Python faces, and the restatement's own agreement with
scikit-learn / scipy.  CPU only: every library call here is refused before the device is touched."""
import ctypes

import numpy as np
import pytest
from scipy import optimize, stats

import trajfit_restatement as R
from pilot_amd import _lib, engine, tl


def _rc(n=10, n_targets=3, ld=3, dtype=1, x=None, model=0, epsilon=1.35, pval_thr=0.05, null=None):
    L = _lib.load()
    Y = np.zeros(max(n, 1) * max(ld, 1) + 1)
    x = np.arange(max(n, 1), dtype=np.float64) if x is None else np.asarray(x, dtype=np.float64)
    out = _lib.TrajfitOut()
    ptrs = dict(Y=ctypes.c_void_p(Y.ctypes.data), x=_lib.dptr(x), out=ctypes.byref(out))
    if null:
        ptrs[null] = None
    return L.pilot_ot_trajectory_fits(ptrs["Y"], 0, dtype, n, n_targets, ld, ptrs["x"], model, epsilon, pval_thr, 0, ptrs["out"],
                                      None)


BAD = [
    dict(n=3),                                   # n < 4
    dict(n=0),
    dict(n_targets=-1),
    dict(n_targets=4, ld=3),                     # ld < n_targets
    dict(dtype=2),
    dict(model=2),
    dict(model=-1),
    dict(pval_thr=float("nan")),
    dict(epsilon=0.99),                          # sklearn's bound epsilon >= 1
    dict(epsilon=0.99, model=1),
    dict(epsilon=float("nan")),
    dict(epsilon=float("inf"), model=1),
    dict(x=np.ones(10)),                         # one distinct x
    dict(x=np.r_[np.ones(5), 2 * np.ones(5)]),   # two distinct x: x^2 is affine in x
    dict(x=np.r_[np.ones(5), 2 * np.ones(5)], model=1),
    dict(x=np.r_[np.arange(9.0), np.nan]),
    dict(x=np.r_[np.arange(9.0), np.inf]),
    dict(null="Y"),
    dict(null="x"),
    dict(null="out"),
]


@pytest.mark.parametrize("kw", BAD, ids=[str(b) for b in range(len(BAD))])
def test_c_abi_rejects_before_the_device(kw):
    assert _rc(**kw) == _lib.EINVAL
    assert _lib.load().pilot_ot_last_error()


def test_zero_targets_is_a_no_op():
    assert _rc(n_targets=0, ld=0) == _lib.OK


@pytest.mark.parametrize("kw", [dict(model="lasso"), dict(pval_thr=float("nan")), dict(epsilon=0.5), dict(model="huber", epsilon=0.5),
                                dict(x=np.ones(10)), dict(Y=np.ones(10)),
                                dict(x=np.arange(9.0)), dict(Y=np.ones((3, 4)), x=np.arange(3.0))])
def test_engine_rejects(kw):
    args = dict(Y=np.ones((10, 4)), x=np.arange(10.0))
    args.update(kw)
    model = args.pop("model", "ols")
    with pytest.raises(ValueError):
        engine.trajectory_fits(args.pop("Y"), args.pop("x"), model=model, **args)


def test_normalize_rejects():
    L = _lib.load()
    X = np.ones((4, 3), dtype=np.float32)
    out = np.empty((4, 3), dtype=np.float32)
    cols = np.array([0, 3], dtype=np.int32)
    assert L.pilot_ot_normalize_log1p(X.ctypes.data, 0, 4, 3, 1e4, _lib.iptr(cols), 2, out.ctypes.data) == _lib.EINVAL
    cols = np.array([0, 1], dtype=np.int32)
    assert L.pilot_ot_normalize_log1p(X.ctypes.data, 0, 4, 3, 0.0, _lib.iptr(cols), 2, out.ctypes.data) == _lib.EINVAL
    assert L.pilot_ot_normalize_log1p(X.ctypes.data, 3, 4, 3, 1e4, _lib.iptr(cols), 2, out.ctypes.data) == _lib.EINVAL


def test_cell_importance_names_both_pseudotime_sources():
    class A:
        uns = {}
    with pytest.raises(KeyError, match="pseudotime=.*uns\\['pseudotime'\\]"):
        tl.cell_importance(A())


def test_device_matrix_consumers_want_a_square_f64_matrix():
    D = engine.DeviceMatrix(0x1000, 10, shape=(10, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="N x N float64"):
        engine.silhouette_of_rows(D, np.zeros(10, dtype=int))
    with pytest.raises(ValueError, match="N x N float64"):
        engine.diffusion_map_from_kernel(D)
    with pytest.raises(ValueError, match="N x N float64"):
        engine.diffusion_kernel_of_rows(engine.DeviceMatrix(0x1000, 10, dtype=np.float32))


def test_genes_importance_rejects_an_unknown_model():
    with pytest.raises(ValueError):
        tl.genes_importance(object(), "T", model_type="Lasso")


def test_bh_adjustment_is_scipy_s():
    p = np.random.default_rng(3).random(57) ** 3
    np.testing.assert_allclose(tl._bh_adjust(p), stats.false_discovery_control(p, method="bh"), rtol=1e-14, atol=0)


# ---- the restatement against scikit-learn / scipy ------------------------------------------------------------------------
def _data(seed=0, n_samples=60, per=15):
    rng = np.random.default_rng(seed)
    x = np.repeat(np.arange(1, n_samples + 1), per).astype(np.float64)
    Y = np.stack([rng.poisson(1 + 0.04 * x * k).astype(np.float64) for k in range(4)] + [rng.standard_normal(x.size) + 1e-3 * x ** 2])
    return x, Y


@pytest.mark.parametrize("model", R.MODELS)
def test_ols_is_linear_regression(model):
    from sklearn.linear_model import LinearRegression
    x, Y = _data()
    for y in Y:
        f = R.fit_one(x, y, model)
        lr = LinearRegression().fit(R.design(x, model)[:, 1:], y)
        ref = np.r_[lr.intercept_, lr.coef_]
        np.testing.assert_allclose(f["params"], ref, rtol=1e-9, atol=1e-12)
        r2 = lr.score(R.design(x, model)[:, 1:], y)
        q = ref.size - 1
        assert abs(f["rsquared_adj"] - (1 - (1 - r2) * (x.size - 1) / (x.size - q - 1))) <= 1e-12


def test_pvalues_follow_the_t_distribution_and_pearson_is_scipy_s():
    x, Y = _data(1)
    y = Y[1]
    f = R.fit_one(x, y, "linear_quadratic")
    Z = R.design(x, "linear_quadratic")
    n, p = Z.shape
    e = y - Z @ f["params"]
    se = np.sqrt(e @ e / (n - p) * np.diag(np.linalg.inv(Z.T @ Z)))
    ref = 2 * (1 - stats.t.cdf(np.abs(f["params"] / se), n - p))
    np.testing.assert_allclose(f["pvalues"], ref, rtol=1e-6, atol=1e-12)       # (the direct inverse is the ill-conditioned one)
    r, pp = R.pearson(x, y)
    ref = stats.pearsonr(x, y)
    assert abs(r - ref[0]) <= 1e-15 and abs(pp - ref[1]) <= 1e-15


@pytest.mark.parametrize("model", R.MODELS)
def test_huber_is_the_optimum_and_matches_sklearn_where_it_converged(model):
    """The restatement's Huber optimum against L-BFGS-B on the rescaled problem (gtol 1e-13) and against scikit-learn's own fit,
    on zero-heavy log counts (most points outliers) and on Gaussian noise."""
    from sklearn.linear_model import HuberRegressor
    x, Y = _data(2, n_samples=40, per=10)
    Y = np.r_[np.log1p(Y[:4]), Y[4:]]
    compared = 0
    for y in Y:
        prm, sig, F, ok = R.huber(x, y, model)
        assert ok
        Z = R.design(x, model)
        s = np.abs(Z).max(axis=0)

        def obj(v):
            return R.huber_objective(x, y, model, v[:-1] / s, v[-1], 1.35)
        res = optimize.minimize(obj, np.r_[prm * s, sig] * (1 + 1e-3), method="L-BFGS-B",
                                bounds=[(None, None)] * s.size + [(R.SIGMA_MIN, None)],
                                options=dict(gtol=1e-13, ftol=1e-16, maxiter=20000))
        assert F <= res.fun * (1 + 1e-12)
        h = HuberRegressor(epsilon=1.35).fit(Z[:, 1:], y)
        Fs = R.huber_objective(x, y, model, np.r_[h.intercept_, h.coef_], h.scale_, 1.35)
        assert F <= Fs * (1 + 1e-12)
        # (an objective within 1e-9 of the optimum still leaves flat fits' coefficients free by ~1e-3: sqrt(2 dF / curvature))
        if Fs <= F * (1 + 1e-12):
            compared += 1
            np.testing.assert_allclose(prm, np.r_[h.intercept_, h.coef_], rtol=1e-5, atol=1e-5 * np.abs(prm).max())
