"""The regularised log transform (K24), the parts that need no device.

The restatement (tests/nb_rlog_restatement.py) is pinned on its own: its dense-Newton optimum against
scipy.optimize.minimize(L-BFGS-B) with the analytic gradient (to 1e-3 in log2 units: that is L-BFGS's own limit, the observed
worst is printed) and by its own residual (the dense Newton step left at the result, <= 1e-12); the arrowhead form -- the device's
iteration, vectorised -- against the dense one at m <= 130; the gradient and Hessian against finite differences; the weighted
quantile against a brute-force expansion of integer weights; the PCA tail against scikit-learn.  The product's host tails:
engine.nb_rlog_prior_var equals the restatement's, tl.pseudobulk_pca (engine.pca replaced by numpy's SVD in engine.pca's sign
convention) equals scikit-learn's VarianceThreshold + PCA to 1e-9, tl.rlog / tl.compute_pseudobulk_PCA run with the two device
calls replaced by the restatement.  pilot_ot_nb_dispersions_blind / pilot_ot_nb_rlog refuse every bad argument before any HIP
call, engine / tl raise before the library is touched, and engine.nb_dispersions(..., n_groups=1) is refused as before."""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest
from scipy import optimize

import nb_glm_restatement as RR
import nb_rlog_restatement as LR
from pilot_amd import _lib, engine, tl


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())


@functools.lru_cache(maxsize=None)
def _genes(m, G=27, seed=3):
    rng = np.random.default_rng(seed + m)
    s = RR.size_factors(rng, m)
    c, alpha, kind = LR.gene_classes(rng, s, G)
    for a in (s, c, alpha, kind):
        a.flags.writeable = False
    return s, c, alpha, kind


def _live(c, alpha):
    return np.flatnonzero(~np.isnan(alpha) & (c > 0).any(axis=0))


# ---- the restatement on its own ------------------------------------------------------------------------------------------------------
def test_gradient_and_hessian_are_the_derivatives_of_P():
    s, c, alpha, _ = _genes(12)
    rng = np.random.default_rng(0)
    lam = LR.ridge(0.5)
    for j in _live(c, alpha)[:9]:
        cj = c[:, j]
        b0, b = np.log(max(cj.mean(), 0.5)) + rng.normal(0, 0.3), rng.normal(0, 0.3, 12)
        x = np.append(b0, b)
        f = lambda v: LR.P(cj, s, alpha[j], lam, v[0], v[1:])
        g = LR.gradient(cj, s, alpha[j], lam, b0, b)
        # central differences of step 1e-4: the rounding of P, 4 ulp |P| / step, plus step^2 times a third derivative of the size of H
        step = 1e-4
        num = np.array([(f(x + step * e) - f(x - step * e)) / (2 * step) for e in np.eye(13)])
        scale = np.abs(g).max() + np.abs(LR.hessian(cj, s, alpha[j], lam, b0, b)).max()
        assert np.abs(num - g).max() <= 4 * 2.0 ** -52 * abs(f(x)) / step + step ** 2 * scale
        H = LR.hessian(cj, s, alpha[j], lam, b0, b)
        grad = lambda v: LR.gradient(cj, s, alpha[j], lam, v[0], v[1:])
        for i in range(13):
            e = np.zeros(13)
            e[i] = 1e-5
            col = -(grad(x + e) - grad(x - e)) / 2e-5
            assert np.abs(col - H[:, i]).max() <= 1e-6 * np.abs(H).max()
        assert np.linalg.eigvalsh(H).min() > 0                          # strictly concave


@pytest.mark.parametrize("prior_var", [0.05, 1.0])
def test_the_dense_optimum_is_the_l_bfgs_optimum(prior_var):
    s, c, alpha, kind = _genes(12)
    lam = LR.ridge(prior_var)
    want, intercept, left = LR.dense_rlog(c, s, alpha, prior_var)
    assert left.max() <= 1e-12, left.max()                               # the dense Newton step left at the result
    worst = 0.0
    for j in _live(c, alpha):
        cj = c[:, j]
        fun = lambda v: -LR.P(cj, s, alpha[j], lam, v[0], v[1:])
        jac = lambda v: -LR.gradient(cj, s, alpha[j], lam, v[0], v[1:])
        x0 = np.append(np.log((cj / s).mean()), np.zeros(12))
        for _ in range(2):                                              # (restarted once from its own result: a fresh memory)
            best = optimize.minimize(fun, x0, jac=jac, method="L-BFGS-B", options=dict(maxiter=5000, maxfun=50000, ftol=1e-15, gtol=1e-10))
            x0 = best.x
        got = (best.x[0] + best.x[1:]) / LR.LN2
        worst = max(worst, np.abs(got - want[:, j]).max(), abs(best.x[0] / LR.LN2 - intercept[j]))
        b0, b = LR.coefficients(want[:, j:j + 1], intercept[j:j + 1])
        assert -best.fun <= LR.P(cj, s, alpha[j], lam, b0[0], b[:, 0]) + 1e-9 * max(1.0, abs(best.fun))      # nothing lies above it
    print("\nL-BFGS-B against the dense Newton optimum: at most %.3g log2 units" % worst)
    assert worst <= 1e-3
    zero, dead = kind == LR.CLASSES.index("all zero"), np.isnan(alpha)
    assert (want[:, zero] == 0).all() and np.isnan(intercept[zero]).all() and np.isnan(want[:, dead]).all()


@pytest.mark.parametrize("m", [2, 3, 12, 65, 130])
@pytest.mark.parametrize("prior_var", [1e-3, 1.0, 50.0])
def test_the_arrowhead_iteration_ends_at_the_dense_optimum(m, prior_var):
    s, c, alpha, kind = _genes(m)
    got = LR.arrowhead_rlog(c, s, alpha, prior_var)
    want, intercept, left = LR.dense_rlog(c, s, alpha, prior_var)
    live = _live(c, alpha)
    assert left.max() <= 1e-12
    assert not got["flags"].any() and got["steps"][live].max() <= 16 and (got["steps"][live] >= 1).all()
    assert LR.dense_step_at(c, s, alpha, prior_var, got["rlog"], got["intercept"], live).max() <= 1e-12
    np.testing.assert_allclose(got["rlog"][:, live], want[:, live], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got["intercept"][live], intercept[live], rtol=0, atol=1e-11)
    d0, d = LR.arrowhead_step(c[:, live], s, alpha[live], prior_var, *LR.coefficients(got["rlog"][:, live], got["intercept"][live]))
    assert max(np.abs(d0).max(), np.abs(d).max()) <= 1e-12              # the two forms of the step agree that nothing is left
    rest = np.setdiff1d(np.arange(alpha.size), live)
    np.testing.assert_array_equal(got["rlog"][:, rest], want[:, rest])
    assert np.isnan(got["intercept"][rest]).all() and not got["steps"][rest].any()


def test_the_ridge_pulls_the_samples_towards_the_intercept():
    s, c, alpha, kind = _genes(12)
    nb = np.flatnonzero(kind == 0)
    spread = [np.ptp(LR.arrowhead_rlog(c[:, nb], s, alpha[nb], pv)["rlog"], axis=0) for pv in (1e-3, 1.0, 50.0)]
    assert (spread[0] < spread[1]).all() and (spread[1] < spread[2]).all()
    loose = LR.arrowhead_rlog(c[:, nb], s, alpha[nb], 1e4)["rlog"]       # an all but free fit is log2 of the normalised count
    big = c[:, nb] >= 50
    assert np.abs(loose - np.log2(np.maximum(c[:, nb], 0.5) / s[:, None]))[big].max() <= 0.02


def test_blind_dispersions_are_the_one_group_case_of_the_k22_restatement():
    rng = np.random.default_rng(4)
    s = RR.size_factors(rng, 6)
    c = RR.nb_class(rng, s, np.zeros(6, dtype=np.int64), 1, 30)
    c[:, 3] = 0.0
    x, L, mu = LR.blind_dispersions(c, s)
    assert np.isnan(x[3]) and np.isfinite(np.delete(x, 3)).all()
    np.testing.assert_array_equal(mu, np.maximum(s[:, None] * (c / s[:, None]).mean(axis=0)[None], RR.MIN_MU))
    assert (x[np.isfinite(x)] >= np.log(RR.MIN_DISP) - 1e-12).all() and (x[np.isfinite(x)] <= np.log(RR.max_disp(6)) + 1e-12).all()


# ---- the prior variance ----------------------------------------------------------------------------------------------------------------
def test_weighted_quantile_is_the_type_7_quantile_of_the_expanded_sample():
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 200):
        x = np.round(rng.exponential(1.0, n), 1)                         # (rounded: equal values occur)
        w = rng.integers(1, 6, n)
        for upper in (0.05, 0.5, 0.3):
            e = np.sort(np.repeat(x, w))
            o = 1.0 + (e.size - 1) * (1.0 - upper)
            low = int(np.floor(o))
            high = min(low + 1, e.size)
            want = (1 - o % 1.0) * e[low - 1] + (o % 1.0) * e[high - 1]
            got = LR.weighted_upper_quantile(x, w.astype(np.float64), upper)
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want))
            assert abs(got - np.quantile(e, 1.0 - upper)) <= 1e-12 * max(1.0, abs(want))


def test_engine_prior_var_is_the_restatement(no_library):
    for m, seed in ((3, 1), (12, 2), (130, 3)):
        rng = np.random.default_rng(seed)
        s = RR.size_factors(rng, m)
        c = RR.nb_class(rng, s, np.zeros(m, dtype=np.int64), 1, 150)
        c[:, 5] = 0.0
        mean = (c / s[:, None]).mean(axis=0)
        with np.errstate(divide="ignore"):
            fit = np.clip(0.05 + 2.0 / mean, RR.MIN_DISP, RR.max_disp(m))
        want = LR.prior_var(c, s, mean, fit)
        got = engine.nb_rlog_prior_var(c, s, mean, fit)
        print("\nm = %d: prior_var %.4g" % (m, got))
        assert abs(got - want) <= 1e-12 * want and 0.05 < got < 5.0
        assert engine.nb_rlog_prior_var(c.astype(np.float32), s, mean, fit) == got
    for bad in (dict(base_mean=mean[:-1]), dict(disp_fit=fit[:-1]), dict(size_factors=s[:-1]), dict(counts=c[0]),
                dict(base_mean=np.zeros(150)), dict(size_factors=-s)):
        with pytest.raises(ValueError):
            engine.nb_rlog_prior_var(**{**dict(counts=c, size_factors=s, base_mean=mean, disp_fit=fit), **bad})


# ---- the PCA tail ----------------------------------------------------------------------------------------------------------------------
def _numpy_pca(Y, n_comps=50, scale=True, max_value=10.0, cols=None, return_info=False):
    """engine.pca(scale=False) by numpy: the score of largest magnitude of every component positive, as the device returns it"""
    assert scale is False and not return_info
    Z = np.asarray(Y, dtype=np.float64)[:, cols]
    Z = Z - Z.mean(axis=0)
    U, sv, Vt = np.linalg.svd(Z, full_matrices=False)
    scores = U * sv[None]
    sign = np.sign(scores[np.abs(scores).argmax(axis=0), np.arange(scores.shape[1])])
    var = sv ** 2 / (Z.shape[0] - 1)
    return (scores * sign[None])[:, :n_comps], (Vt.T * sign[None])[:, :n_comps], var[:n_comps], (var / var.sum())[:n_comps]


def test_pseudobulk_pca_is_variance_threshold_then_sklearn_pca(monkeypatch):
    from sklearn.decomposition import PCA
    from sklearn.feature_selection import VarianceThreshold
    monkeypatch.setattr(engine, "pca", _numpy_pca)
    rng = np.random.default_rng(6)
    X = rng.normal(5.0, 1.0, (12, 80)) * rng.uniform(0.05, 1.5, 80)[None]
    X[:4, :10] += 3.0
    frame = pd.DataFrame(X, index=["s%d" % i for i in range(12)], columns=["g%d" % j for j in range(80)])
    for thr, k in ((0.2, 2), (0.0, 3), (0.5, 1)):
        kept = VarianceThreshold(thr).fit_transform(X)
        assert 3 < kept.shape[1] < 80 or thr == 0.0
        model = PCA(n_components=k)
        want = model.fit_transform(kept)
        scores, ratio = tl.pseudobulk_pca(frame, thr, k)
        assert list(scores.columns) == ["PC%d" % (i + 1) for i in range(k)] and list(scores.index) == list(frame.index)
        np.testing.assert_allclose(scores.to_numpy(), want, rtol=0, atol=1e-9)
        np.testing.assert_allclose(ratio, model.explained_variance_ratio_, rtol=0, atol=1e-9)
        mine, mine_ratio, cols = LR.pca_tail(X, thr, k)
        np.testing.assert_allclose(mine, want, rtol=0, atol=1e-9)
        np.testing.assert_allclose(mine_ratio, model.explained_variance_ratio_, rtol=0, atol=1e-9)
        assert cols.size == kept.shape[1]
    np.testing.assert_array_equal(tl.pseudobulk_pca(X)[0].to_numpy(), tl.pseudobulk_pca(frame)[0].to_numpy())


def test_pseudobulk_pca_refuses_before_the_library(no_library):
    X = np.random.default_rng(7).normal(0, 1, (6, 10))
    flat = np.ones((6, 10)) + 1e-3 * X
    for kw in (dict(rld=X[0]), dict(rld=flat), dict(variance_threshold=100.0), dict(n_components=0), dict(n_components=1.5),
               dict(n_components=True), dict(variance_threshold=-1.0), dict(variance_threshold="0.2"), dict(n_components=10),
               dict(rld=np.where(np.arange(10) == 3, np.nan, X))):
        with pytest.raises(ValueError):
            tl.pseudobulk_pca(**{**dict(rld=X, variance_threshold=0.2, n_components=2), **kw})


# ---- tl.rlog on the restatement ----------------------------------------------------------------------------------------------------
def _frame(m=12, G=60, seed=8):
    rng = np.random.default_rng(seed)
    s = RR.size_factors(rng, m)
    c = RR.nb_class(rng, s, np.zeros(m, dtype=np.int64), 1, G)
    c[:, 4] = 0.0
    return pd.DataFrame(c, index=["s%02d" % i for i in range(m)], columns=["g%03d" % j for j in range(G)])


def test_tl_rlog_is_the_host_tail_of_the_two_device_calls(monkeypatch):
    calls = []

    def blind(counts, size_factors, return_info=False):
        calls.append("blind")
        return LR.blind_dispersions(counts, size_factors)[0]

    def fit(counts, size_factors, dispersion, prior_var, on_device=False, return_info=False):
        calls.append("rlog")
        got = LR.arrowhead_rlog(counts, size_factors, dispersion, prior_var)
        return got["rlog"], {"intercept": got["intercept"], "steps": got["steps"], "flags": got["flags"], "n_not_converged": 0}

    monkeypatch.setattr(engine, "nb_dispersions_blind", blind)
    monkeypatch.setattr(engine, "nb_rlog", fit)
    counts = _frame()
    out = tl.rlog(counts)
    assert calls == ["blind", "rlog"]
    assert out.shape == counts.shape and list(out.index) == list(counts.index) and list(out.columns) == list(counts.columns)
    assert sorted(out.attrs) == ["dispFit", "intercept", "n_not_converged", "prior_var", "size_factors"]
    c = counts.to_numpy()
    sf = tl.deseq2_size_factors(counts).to_numpy()
    np.testing.assert_array_equal(out.attrs["size_factors"].to_numpy(), sf)
    mean = (c / sf[:, None]).mean(axis=0)
    x = LR.blind_dispersions(c, sf)[0]
    trend = engine.nb_clip(engine.nb_trend(mean, engine.nb_clip(np.exp(x), 12))[0], 12)
    np.testing.assert_array_equal(out.attrs["dispFit"].to_numpy(), trend)
    assert out.attrs["prior_var"] == LR.prior_var(c, sf, mean, trend) and 0.05 < out.attrs["prior_var"] < 5.0
    want, intercept, left = LR.dense_rlog(c, sf, trend, out.attrs["prior_var"])
    assert left.max() <= 1e-12
    np.testing.assert_allclose(out.to_numpy(), want, rtol=0, atol=1e-11)
    assert (out["g004"] == 0).all() and np.isnan(out.attrs["intercept"]["g004"])
    # the transform is a shrunken log2 of the normalised counts: close to it where the counts are large
    big = c.min(axis=0) > 200
    assert big.sum() >= 5 and np.abs(out.to_numpy()[:, big] - np.log2(c[:, big] / sf[:, None])).max() < 0.5
    # a given prior variance and size factors, and the mean trend
    given = tl.rlog(counts, size_factors=np.ones(12), fit_type="mean", prior_var=2.0)
    assert given.attrs["prior_var"] == 2.0 and (given.attrs["size_factors"] == 1.0).all() and given.attrs["dispFit"].nunique() == 1
    # the reference's function: the transpose, R's genes x samples
    meta = pd.DataFrame({"stage": ["T1"] * 5 + ["T2"] * 7}, index=counts.index)
    rld = tl.compute_pseudobulk_PCA(counts, meta)
    assert list(rld.index) == list(counts.columns) and list(rld.columns) == list(counts.index)
    np.testing.assert_array_equal(rld.to_numpy(), out.to_numpy().T)
    assert rld.attrs["prior_var"] == out.attrs["prior_var"]
    with pytest.raises(ValueError, match="cluster_metadata"):
        tl.compute_pseudobulk_PCA(counts, meta.iloc[::-1])


def test_tl_rlog_refuses_before_the_library(no_library):
    counts = _frame(6, 5)
    for kw in (dict(cluster_counts=counts.iloc[:1]), dict(cluster_counts=counts.iloc[:, :0]), dict(cluster_counts=np.ones(6)),
               dict(fit_type="local"), dict(prior_var=0.0), dict(prior_var=-1.0), dict(prior_var=np.nan), dict(prior_var=np.inf),
               dict(prior_var="1"), dict(prior_var=True), dict(size_factors=np.ones(5)), dict(size_factors=[1, 1, 0, 1, 1, 1]),
               dict(size_factors=[1, 1, np.nan, 1, 1, 1])):
        with pytest.raises(ValueError):
            tl.rlog(**{**dict(cluster_counts=counts), **kw})


# ---- the C entry points ----------------------------------------------------------------------------------------------------------------
GOOD = dict(y=True, dtype=1, m=6, genes=5, ld=5, sf=[1.0, 0.5, 2.0, 1.0, 1.5, 0.7], disp=[0.1] * 5, pv=1.0, out=True, ld_out=5, icpt=True)


def _call(which, **kw):
    a = dict(GOOD)
    a.update(kw)
    L = _lib.load()
    Y = np.ones((6, 8), dtype=np.float64)
    sf = None if a["sf"] is None else np.ascontiguousarray(a["sf"], dtype=np.float64)
    head = (ctypes.c_void_p(Y.ctypes.data) if a["y"] else None, 0, a["dtype"], a["m"], a["genes"], a["ld"], None if sf is None else _lib.dptr(sf))
    o1, o2, o3 = np.zeros(64), np.zeros(64), np.zeros(64)
    bad_row, bad_col = ctypes.c_longlong(5), ctypes.c_int(5)
    if which == "blind":
        rc = L.pilot_ot_nb_dispersions_blind(*head, _lib.dptr(o1) if a["out"] else None, _lib.dptr(o2), _lib.dptr(o3), ctypes.byref(bad_row),
                                             ctypes.byref(bad_col))
    else:
        disp = None if a["disp"] is None else np.ascontiguousarray(a["disp"], dtype=np.float64)
        i1, i2, n_bad = np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.int32), ctypes.c_int(7)
        rc = L.pilot_ot_nb_rlog(*head, None if disp is None else _lib.dptr(disp), a["pv"], ctypes.c_void_p(o1.ctypes.data) if a["out"] else None, 0,
                                a["ld_out"], _lib.dptr(o2) if a["icpt"] else None, _lib.iptr(i1), _lib.iptr(i2), ctypes.byref(n_bad),
                                ctypes.byref(bad_row), ctypes.byref(bad_col))
        assert n_bad.value == 0
    assert bad_row.value == -1 and bad_col.value == -1
    return rc, L.pilot_ot_last_error()


SHARED_REFUSALS = [
    (dict(y=False), b"NULL"), (dict(sf=None), b"NULL"), (dict(out=False), b"NULL"),
    (dict(genes=0, ld=0, ld_out=0), b"n_genes=0"), (dict(genes=-1), b"n_genes=-1"), (dict(ld=4), b"ld=4"), (dict(dtype=2), b"dtype"),
    (dict(dtype=-1), b"dtype"), (dict(m=1), b"m=1"), (dict(m=0), b"m=0"),
    (dict(sf=[1.0, 0.0, 2.0, 1.0, 1.5, 0.7]), b"size_factors[1]"), (dict(sf=[1.0, 0.5, -2.0, 1.0, 1.5, 0.7]), b"size_factors[2]"),
    (dict(sf=[1.0, 0.5, 2.0, np.nan, 1.5, 0.7]), b"size_factors[3]"), (dict(sf=[1.0, 0.5, 2.0, 1.0, np.inf, 0.7]), b"size_factors[4]"),
]


@pytest.mark.parametrize("which", ["blind", "rlog"])
@pytest.mark.parametrize("bad,fragment", SHARED_REFUSALS)
def test_entry_points_refuse_before_any_hip_call(which, bad, fragment):
    rc, msg = _call(which, **bad)
    assert rc == _lib.EINVAL and fragment in msg, (bad, msg)


@pytest.mark.parametrize("bad,fragment", [
    (dict(disp=None), b"NULL"), (dict(icpt=False), b"NULL"), (dict(ld_out=4), b"ld_out=4"),
    (dict(pv=0.0), b"prior_var"), (dict(pv=-1.0), b"prior_var"), (dict(pv=np.nan), b"prior_var"), (dict(pv=np.inf), b"prior_var"),
    (dict(disp=[0.1, 0.1, 9e-9, 0.1, 0.1]), b"dispersion[2]"), (dict(disp=[10.5] + [0.1] * 4), b"dispersion[0]"),
    (dict(disp=[0.1, np.inf, 0.1, 0.1, 0.1]), b"dispersion[1]"), (dict(disp=[0.1, 0.1, 0.1, -1.0, 0.1]), b"dispersion[3]"),
])
def test_rlog_refuses_its_own_arguments(bad, fragment):
    rc, msg = _call("rlog", **bad)
    assert rc == _lib.EINVAL and fragment in msg, (bad, msg)


def test_too_many_samples_are_refused_before_any_hip_call():
    L = _lib.load()
    m = L.pilot_ot_nb_glm_max_samples() + 1
    Y, sf, out, ints = np.ones((m, 1)), np.ones(m), np.zeros(m + 2), np.zeros(2, dtype=np.int32)
    rc = L.pilot_ot_nb_dispersions_blind(ctypes.c_void_p(Y.ctypes.data), 0, 1, m, 1, 1, _lib.dptr(sf), _lib.dptr(out), _lib.dptr(out[1:]), None,
                                         None, None)
    assert rc == _lib.ENOTSUP and b"staged in LDS" in L.pilot_ot_last_error()
    disp = np.full(1, 0.1)
    rc = L.pilot_ot_nb_rlog(ctypes.c_void_p(Y.ctypes.data), 0, 1, m, 1, 1, _lib.dptr(sf), _lib.dptr(disp), 1.0, ctypes.c_void_p(out.ctypes.data), 0,
                            1, _lib.dptr(out[m:]), _lib.iptr(ints), _lib.iptr(ints[1:]), None, None, None)
    assert rc == _lib.ENOTSUP and b"staged in LDS" in L.pilot_ot_last_error()
    with pytest.raises(NotImplementedError, match="samples"):
        engine.nb_dispersions_blind(Y, sf)
    with pytest.raises(NotImplementedError, match="samples"):
        engine.nb_rlog(Y, sf, disp, 1.0)
    assert 24 * (m - 1) <= 96 * 1024                                    # counts, log size factors and coefficients within the LDS


def test_good_arguments_get_as_far_as_the_device():
    want = _lib.OK if _lib.device_count() > 0 else _lib.EHIP
    for which, kw in (("blind", dict()), ("blind", dict(ld=8)), ("blind", dict(dtype=0, m=2)), ("rlog", dict()), ("rlog", dict(ld_out=7)),
                      ("rlog", dict(disp=[1e-8, 10.0, np.nan, 0.1, 0.1])), ("rlog", dict(m=2, sf=[1.0, 2.0]))):
        rc, msg = _call(which, **kw)
        assert rc == want, (which, kw, msg)


def test_symbols():
    for name in ("pilot_ot_nb_dispersions_blind", "pilot_ot_nb_rlog"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)
    assert LR.NOT_CONVERGED == _lib.NB_NOT_CONVERGED
    assert not [n for n in engine.ws_slot_names() if n.startswith("WS_NB_")
                and n not in ("WS_NB_Y", "WS_NB_INT", "WS_NB_SF", "WS_NB_BAD", "WS_NB_PRIOR", "WS_NB_OUT", "WS_NB_FIT_INT")]


# ---- engine ----------------------------------------------------------------------------------------------------------------------------
Y6, S6 = np.ones((6, 5)), np.array([1.0, 0.5, 2.0, 1.0, 1.5, 0.7])


@pytest.mark.parametrize("kw", [
    dict(counts=np.ones(6)), dict(counts=np.ones((6, 5), dtype=np.int64)), dict(counts=np.ones((6, 8))[:, :5]), dict(counts=np.ones((6, 0))),
    dict(counts=np.ones((1, 5)), size_factors=[1.0]), dict(size_factors=S6[:5]), dict(size_factors=[1.0, 0.0, 2.0, 1.0, 1.5, 0.7]),
    dict(size_factors=[1.0, np.nan, 2.0, 1.0, 1.5, 0.7]), dict(size_factors=-S6),
])
def test_engine_refuses_before_the_library(no_library, kw):
    a = dict(counts=Y6, size_factors=S6)
    a.update(kw)
    with pytest.raises(ValueError):
        engine.nb_dispersions_blind(**a)
    with pytest.raises(ValueError):
        engine.nb_rlog(dispersion=np.full(np.shape(a["counts"])[-1], 0.1), prior_var=1.0, **a)


def test_engine_refuses_its_own_arguments(no_library):
    for disp in (np.full(4, 0.1), np.array([0.1, 0.1, 9e-9, 0.1, 0.1]), np.array([0.1, 10.5, 0.1, 0.1, 0.1]), np.array([0.1, np.inf, 0.1, 0.1, 0.1])):
        with pytest.raises(ValueError):
            engine.nb_rlog(Y6, S6, disp, 1.0)
    for pv in (0.0, -1.0, np.nan, np.inf, "1", None, True, np.ones(2)):
        with pytest.raises(ValueError):
            engine.nb_rlog(Y6, S6, np.full(5, 0.1), pv)


def test_one_group_is_still_refused_by_the_grouped_calls(no_library):
    with pytest.raises(ValueError, match="n_groups=1"):
        engine.nb_dispersions(Y6, np.zeros(6, dtype=np.int32), 1, S6)
    with pytest.raises(ValueError, match="n_groups=1"):
        engine.nb_group_fits(Y6, np.zeros(6, dtype=np.int32), 1, S6, np.full(5, 0.1))


def test_one_group_is_still_refused_by_the_grouped_entry_point():
    L = _lib.load()
    Y, codes, sf, out = np.ones((6, 5)), np.zeros(6, dtype=np.int32), np.ones(6), np.zeros(10)
    rc = L.pilot_ot_nb_dispersions(ctypes.c_void_p(Y.ctypes.data), 0, 1, 6, 5, 5, _lib.iptr(codes), 1, _lib.dptr(sf), None, 0.0, _lib.dptr(out),
                                   _lib.dptr(out[5:]), None, None, None)
    assert rc == _lib.EINVAL and b"n_groups=1" in L.pilot_ot_last_error()
