"""The negative-binomial GLM (K22), the parts that need no device.

The restatement (tests/nb_glm_restatement.py) is pinned to scipy on its own: the likelihood against scipy.stats.nbinom.logpmf,
the Cox-Reid term against numpy.linalg.slogdet of the explicit intercept + indicator design, the grid maximiser against
scipy.optimize.minimize_scalar(bounded) on three sub-brackets, the group fits against scipy.optimize.minimize on the explicit
two-parameter GLM and inv(X^T W X).  The product's host tails: engine.nb_trend must satisfy the Gamma-GLM score equations on its
final gene set, engine.nb_prior_var and tl's outlier flags must equal the restatement's exactly (tl.deseq2_dispersions runs here
with engine.nb_dispersions replaced by the restatement).  pilot_ot_nb_dispersions / pilot_ot_nb_group_fits refuse every bad
argument before any HIP call (a box without a device returns PILOT_OT_EHIP from the first HIP call), and engine / tl raise before
the library is touched.

Two facts about the gene classes of test_gpu_nb_glm.py are checked here, as the design asks: the NB class resolves (parity rule 2)
on at least 95 % of its genes, and the constant-count class ends at the lower bound only up to the rounding of L -- see
test_constant_counts_end_next_to_the_lower_bound."""
import ctypes

import numpy as np
import pandas as pd
import pytest
from scipy import optimize, stats

import nb_glm_restatement as RR
from pilot_amd import _lib, engine, tl

CODES12 = np.repeat([0, 1, 2], [5, 4, 3])


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())


def _nb_cohort(G=200, seed=0):
    """the issue's NB class at m = 12, k = 3"""
    rng = np.random.default_rng(seed)
    s = RR.size_factors(rng, 12)
    return RR.nb_class(rng, s, CODES12, 3, G), s


@pytest.fixture(scope="module")
def cohort():
    c, s = _nb_cohort()
    x, L, mu = RR.dispersions(c, CODES12, 3, s)
    return c, s, x, L, mu


# ---- the restatement against scipy ---------------------------------------------------------------------------------------------------
def test_likelihood_is_the_negative_binomial_log_pmf(cohort):
    c, s, x, _, mu = cohort
    for shift in (-3.0, 0.0, 2.0):
        xs = np.clip(x + shift, np.log(RR.MIN_DISP), np.log(RR.max_disp(12)))
        alpha = np.exp(xs)[None]
        want = (stats.nbinom.logpmf(c, 1.0 / alpha, 1.0 / (1.0 + alpha * mu)) + RR.special.gammaln(c + 1.0)).sum(axis=0)
        got = sum(t.sum(axis=0) for t in RR.likelihood_terms(c, mu, xs))[:, 0]
        assert (np.abs(got - want) <= RR.bound(c, mu, 3, xs)).all()


def test_cox_reid_term_is_the_log_determinant_of_the_information(cohort):
    c, s, x, _, mu = cohort
    X = np.zeros((12, 3))
    X[:, 0] = 1.0
    X[CODES12 == 1, 1] = X[CODES12 == 2, 2] = 1.0
    got = RR.cox_reid(mu, CODES12, 3, x)[:, 0]
    for j in range(0, c.shape[1], 7):
        w = mu[:, j] / (1.0 + np.exp(x[j]) * mu[:, j])
        sign, want = np.linalg.slogdet(X.T @ (w[:, None] * X))
        assert sign == 1.0
        np.testing.assert_allclose(got[j], want, rtol=1e-12, atol=1e-12)


def test_grid_search_reaches_the_bounded_optimiser(cohort):
    """scipy may find a larger L only by the rounding noise of L itself (2 B: one B for each of the two evaluations), and on the
    genes the restatement resolves the two maximisers agree to 2e-4 in x, the tolerance the device is held to"""
    c, s, x, L, mu = cohort
    res = RR.resolved(c, mu, CODES12, 3, x)
    assert res.mean() >= 0.95                                      # the NB class of the device tests resolves: 0.99 measured
    B = RR.bound(c, mu, 3, x)
    edges = np.linspace(np.log(RR.MIN_DISP), np.log(RR.max_disp(12)), 4)
    for j in range(0, c.shape[1], 4):
        f = lambda v: -RR.objective(c[:, [j]], mu[:, [j]], CODES12, 3, np.array([v]))[0]
        best = min((optimize.minimize_scalar(f, bounds=(a, b), method="bounded", options={"xatol": 1e-10})
                    for a, b in zip(edges[:-1], edges[1:])), key=lambda r: r.fun)
        assert -best.fun - L[j] <= 2 * B[j], (j, -best.fun - L[j], B[j])
        if res[j]:
            assert abs(best.x - x[j]) <= 2e-4, (j, best.x, x[j])


def test_constant_counts_end_next_to_the_lower_bound():
    """No class of genes ends EXACTLY at log(minDisp): there r = 1e8, lgamma(c + r) and lgamma(r) are near 1.7e9 with an ulp of
    2.4e-7, and over the last rounds' grid spacings (3e-4 and below) the true L changes by less than that, so which grid point is
    'first largest' is decided by rounding.  rint(100 s_j), the class first proposed, ends up to 0.16 above the bound (measured
    over these shapes); the class used instead, rint(1e6 s_j), wins the first three rounds on slope and ends within 1e-3."""
    for m, sizes in ((12, [5, 4, 3]), (4, [2, 1, 1]), (3, [2, 1]), (65, [30, 20, 10, 4, 1]), (130, [100, 30])):
        s = RR.size_factors(np.random.default_rng(m), m)
        codes = np.repeat(np.arange(len(sizes)), sizes)
        x = RR.dispersions(np.rint(1e6 * s)[:, None], codes, len(sizes), s)[0]
        assert 0.0 <= x[0] - np.log(RR.MIN_DISP) <= 1e-3, (m, x[0] - np.log(RR.MIN_DISP))


def test_group_fits_are_the_two_parameter_glm(cohort):
    c, s, x, _, _ = cohort
    two = CODES12 < 2
    c2, s2, codes = c[two], s[two], CODES12[two]
    alpha = np.exp(x)
    q, w, flags = RR.group_fits(c2, codes, 2, s2, alpha)
    assert not flags.any()
    lfc, se, stat, p = RR.wald(q, w)
    X = np.stack([np.ones(codes.size), (codes == 1).astype(float)], axis=1)
    for j in range(0, c.shape[1], 9):
        a = alpha[j]

        def nll(beta):
            mu = s2 * np.exp(X @ beta)
            return -(stats.nbinom.logpmf(c2[:, j], 1.0 / a, 1.0 / (1.0 + a * mu))).sum()
        start = np.array([np.log(q[j, 0]) + 0.1, -0.1])
        fit = optimize.minimize(nll, start, method="BFGS", options={"gtol": 1e-10})
        fit = optimize.minimize(nll, fit.x, method="Nelder-Mead", options={"xatol": 1e-11, "fatol": 1e-15, "maxiter": 4000})
        np.testing.assert_allclose(fit.x[1] / np.log(2.0), lfc[j], rtol=0, atol=1e-7)
        mu = s2 * q[j, codes]
        W = mu / (1.0 + a * mu)
        cov = np.linalg.inv(X.T @ (W[:, None] * X))
        np.testing.assert_allclose(se[j], np.log2(np.e) * np.sqrt(cov[1, 1]), rtol=1e-12)
        for g in range(2):                                          # the score equation itself, against the scale of its terms
            sq = s2[codes == g] * q[j, g]
            terms = (c2[codes == g, j] - sq) / (1.0 + a * sq)
            assert abs(terms.sum()) <= 1e-12 * (np.abs(c2[codes == g, j]).sum() + sq.sum())


def test_group_fit_floors():
    s = np.array([0.5, 2.0, 1.0, 1.0, 1.5])
    codes = np.array([0, 0, 1, 1, 1])
    c = np.array([[0.0, 3.0, 0.0], [0.0, 5.0, 1.0], [4.0, 0.0, 7.0], [6.0, 0.0, 7.0], [9.0, 0.0, 7.0]])
    q, w, flags = RR.group_fits(c, codes, 2, s, np.array([0.1, 1e-8, np.nan]))
    assert flags.tolist() == [[RR.FLOORED, 0], [0, RR.FLOORED], [0, 0]]
    assert q[0, 0] == 0.25 and q[1, 1] == 0.5 / 1.5 and np.isnan(q[2]).all() and np.isnan(w[2]).all()
    assert w[0, 0] == 2 * 0.5 / (1 + 0.1 * 0.5)                      # both fitted means sit on minmu


# ---- the product's host tails ------------------------------------------------------------------------------------------------------
def _trend_inputs():
    c, s = _nb_cohort(G=400, seed=3)
    x, _, _ = RR.dispersions(c, CODES12, 3, s)
    return c, s, x, (c / s[:, None]).mean(axis=0)


def test_trend_satisfies_the_gamma_glm_score_equations():
    c, s, x, base_mean = _trend_inputs()
    disp = np.exp(x)
    fitted, info = engine.nb_trend(base_mean, disp, "parametric")
    a0, a1 = info["coefficients"]
    assert a0 > 0 and a1 > 0 and 1 <= info["passes"] <= 10 and info["fit_type"] == "parametric"
    np.testing.assert_array_equal(fitted, a0 + a1 / base_mean)
    used = info["used"]
    assert used.sum() >= 300 and (disp[used] >= 1e-6).all()
    y, mean = disp[used], base_mean[used]
    f = a0 + a1 / mean
    for weight in (1.0, 1.0 / mean):
        terms = (y - f) / (f * f) * weight
        assert abs(terms.sum()) <= 1e-8 * np.abs(terms).sum()
    ratio = y / f                                                   # the last fit's gene set is the band around the fit before it
    assert (ratio > 5e-5).all() and (ratio < 30).all()


def test_trend_mean_and_refusals():
    c, s, x, base_mean = _trend_inputs()
    disp = np.exp(x)
    disp[:5] = [np.nan, 1e-8, 5e-7, 1e-6, 2e-6]
    fitted, info = engine.nb_trend(base_mean, disp, "mean")
    used = RR.used_for_fit(disp)
    assert not used[:3].any() and used[3:5].all()
    np.testing.assert_array_equal(info["used"], used)
    assert info["coefficients"] == (disp[used].mean(), 0.0) and (fitted == disp[used].mean()).all()
    with pytest.raises(ValueError, match="fit_type"):
        engine.nb_trend(base_mean, disp, "local")
    with pytest.raises(ValueError, match="fit_type='parametric'"):     # a dispersion that RISES with the mean: a1 < 0
        engine.nb_trend(base_mean, 0.01 * base_mean, "parametric")
    with pytest.raises(ValueError, match="fit_type"):
        engine.nb_trend(base_mean, np.full(base_mean.size, 1e-8), "mean")
    with pytest.raises(ValueError):
        engine.nb_trend(base_mean[:-1], disp, "mean")


@pytest.mark.parametrize("fit_type", ["parametric", "mean"])
def test_trend_at_is_the_trend_the_fit_returned(fit_type):
    c, s, x, base_mean = _trend_inputs()
    disp = np.exp(x)
    base_mean[[0, 7]], base_mean[[3, 11]] = np.nan, 0.0                # genes without an estimate: the table's NaN mean, and a mean of 0
    disp[[0, 7, 3, 11]] = np.nan
    fitted, info = engine.nb_trend(base_mean, disp, fit_type)
    np.testing.assert_array_equal(engine.nb_trend_at(info, base_mean), fitted)
    assert np.isnan(fitted[[0, 7]]).all() and np.isfinite(np.delete(fitted, [0, 7, 3, 11])).all()
    assert (fitted[[3, 11]] == (np.inf if fit_type == "parametric" else info["coefficients"][0])).all()
    # only the fit type and the coefficients are read, and every mean is evaluated on its own
    bare = {"fit_type": info["fit_type"], "coefficients": info["coefficients"]}
    np.testing.assert_array_equal(engine.nb_trend_at(bare, base_mean[::-1]), fitted[::-1])
    np.testing.assert_array_equal(engine.nb_trend_at(bare, base_mean[5:6]), fitted[5:6])
    with pytest.raises(ValueError, match="fit_type"):
        engine.nb_trend_at({"fit_type": "local", "coefficients": (0.1, 1.0)}, base_mean)


def test_prior_variance_equals_the_restatement():
    c, s, x, base_mean = _trend_inputs()
    fitted, _ = engine.nb_trend(base_mean, np.exp(x), "parametric")
    x = x.copy()
    x[:3] = [np.nan, np.log(1e-8), np.log(5e-7)]
    for m, k in ((12, 3), (4, 2), (3, 2), (130, 5)):
        assert engine.nb_prior_var(x, np.log(fitted), m, k) == RR.prior_var(x, np.log(fitted), m, k)
    assert engine.nb_prior_var(x, x + 0.01, 12, 3)[0] == 0.25          # the floor
    with pytest.raises(ValueError):
        engine.nb_prior_var(x, np.log(fitted), 3, 3)
    with pytest.raises(ValueError):
        engine.nb_prior_var(x[:-1], np.log(fitted), 12, 3)


def test_dispersion_table_on_the_restatement(monkeypatch):
    """tl.deseq2_dispersions with the device call replaced by the restatement: the frame's host tail, outlier flags included"""
    c, s, _, _ = _trend_inputs()
    c = c[:, :150].copy()
    c[:, 7] = 0.0                                                   # a gene of zeros
    c[:, 11] = RR.nb_counts(np.random.default_rng(5), np.full(12, 300.0), 8.0)         # far above the trend: an outlier
    labels = np.array(["b", "a", "c"])[CODES12]                       # sorted labels: a < b < c, so group codes are 1, 0, 2

    def fake(counts, codes, n_groups, size_factors, log_prior_mean=None, prior_var=None, return_info=False):
        return RR.dispersions(counts, codes, n_groups, size_factors, log_prior_mean, prior_var)[0]
    monkeypatch.setattr(engine, "nb_dispersions", fake)
    frame = pd.DataFrame(c, index=["s%d" % i for i in range(12)], columns=["g%d" % j for j in range(150)])
    out = tl.deseq2_dispersions(frame, labels, size_factors=s)
    assert list(out.columns) == ["baseMean", "baseVar", "dispGeneEst", "dispFit", "dispMAP", "dispersion", "dispOutlier"]
    assert list(out.index) == list(frame.columns)
    codes = np.array([1, 0, 2])[CODES12]
    x = RR.dispersions(c, codes, 3, s)[0]
    q = c / s[:, None]
    live = ~np.isnan(x)
    assert not live[7] and live.sum() == 149
    np.testing.assert_array_equal(out["baseMean"].to_numpy()[live], q.mean(axis=0)[live])
    np.testing.assert_array_equal(out["baseVar"].to_numpy()[live], q.var(axis=0, ddof=1)[live])
    clip = lambda d: np.clip(d, RR.MIN_DISP, RR.max_disp(12))
    np.testing.assert_array_equal(out["dispGeneEst"].to_numpy(), clip(np.exp(x)))
    log_fit = np.log(out["dispFit"].to_numpy())
    pv, vld = RR.prior_var(x, log_fit, 12, 3)
    assert (out.attrs["prior_var"], out.attrs["var_log_disp"]) == (pv, vld)
    flags = RR.outliers(x, log_fit, vld)
    np.testing.assert_array_equal(out["dispOutlier"].to_numpy(), flags)
    assert flags[11] and not flags[7] and 1 <= flags.sum() <= 10
    x_map = RR.dispersions(c, codes, 3, s, log_fit, pv)[0]
    np.testing.assert_array_equal(out["dispMAP"].to_numpy(), clip(np.exp(x_map)))
    np.testing.assert_array_equal(out["dispersion"].to_numpy(), np.where(flags, clip(np.exp(x)), clip(np.exp(x_map))))
    assert out.iloc[7, :6].isna().all() and not out["dispOutlier"].iloc[7]
    assert out.attrs["trend"]["fit_type"] == "parametric"
    const = tl.deseq2_dispersions(frame, labels, size_factors=s, fit_type="mean")
    assert const["dispFit"].dropna().nunique() == 1
    default = tl.deseq2_dispersions(frame, labels)                  # the size factors of the table as passed
    np.testing.assert_array_equal(default["baseMean"].to_numpy()[live],
                                  (c / tl.deseq2_size_factors(frame).to_numpy()[:, None]).mean(axis=0)[live])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
GOOD = dict(y=True, dtype=1, m=6, genes=5, ld=5, codes=[0, 1, 0, 1, 1, 0], ng=2, sf=[1.0, 0.5, 2.0, 1.0, 1.5, 0.7], prior=None, pv=0.0,
            out=True, disp=[0.1] * 5)


def _call(which, **kw):
    a = dict(GOOD)
    a.update(kw)
    L = _lib.load()
    Y = np.ones((6, 8), dtype=np.float64)
    codes = None if a["codes"] is None else np.ascontiguousarray(a["codes"], dtype=np.int32)
    sf = None if a["sf"] is None else np.ascontiguousarray(a["sf"], dtype=np.float64)
    head = (ctypes.c_void_p(Y.ctypes.data) if a["y"] else None, 0, a["dtype"], a["m"], a["genes"], a["ld"],
            None if codes is None else _lib.iptr(codes), a["ng"], None if sf is None else _lib.dptr(sf))
    o1, o2 = np.zeros(64), np.zeros(64)
    if which == "dispersions":
        prior = None if a["prior"] is None else np.ascontiguousarray(a["prior"], dtype=np.float64)
        bad_row, bad_col = ctypes.c_longlong(5), ctypes.c_int(5)
        rc = L.pilot_ot_nb_dispersions(*head, None if prior is None else _lib.dptr(prior), a["pv"], _lib.dptr(o1) if a["out"] else None,
                                       _lib.dptr(o2), None, ctypes.byref(bad_row), ctypes.byref(bad_col))
        assert bad_row.value == -1 and bad_col.value == -1
    else:
        disp = None if a["disp"] is None else np.ascontiguousarray(a["disp"], dtype=np.float64)
        i1, i2, n_bad = np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.int32), ctypes.c_int(7)
        rc = L.pilot_ot_nb_group_fits(*head, None if disp is None else _lib.dptr(disp), _lib.dptr(o1) if a["out"] else None, _lib.dptr(o2),
                                      _lib.iptr(i1), _lib.iptr(i2), ctypes.byref(n_bad))
        assert n_bad.value == 0
    return rc, L.pilot_ot_last_error()


SHARED_REFUSALS = [
    (dict(y=False), b"NULL"), (dict(codes=None), b"NULL"), (dict(sf=None), b"NULL"), (dict(out=False), b"NULL"),
    (dict(genes=0, ld=0), b"n_genes=0"), (dict(ld=4), b"ld=4"), (dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"),
    (dict(m=1), b"m=1"), (dict(m=0), b"m=0"),
    (dict(ng=1), b"n_groups=1"), (dict(ng=6, codes=[0, 1, 2, 3, 4, 5]), b"n_groups=6"), (dict(ng=0), b"n_groups=0"),
    (dict(ng=3), b"group 2 has no sample"), (dict(codes=[1, 1, 1, 1, 1, 1]), b"group 0 has no sample"),
    (dict(codes=[0, 1, 2, 1, 1, 0]), b"codes[2]=2"), (dict(codes=[0, -1, 0, 1, 1, 0]), b"codes[1]=-1"),
    (dict(sf=[1.0, 0.0, 2.0, 1.0, 1.5, 0.7]), b"size_factors[1]"), (dict(sf=[1.0, 0.5, -2.0, 1.0, 1.5, 0.7]), b"size_factors[2]"),
    (dict(sf=[1.0, 0.5, 2.0, np.nan, 1.5, 0.7]), b"size_factors[3]"), (dict(sf=[1.0, 0.5, 2.0, 1.0, np.inf, 0.7]), b"size_factors[4]"),
]


@pytest.mark.parametrize("which", ["dispersions", "group_fits"])
@pytest.mark.parametrize("bad,fragment", SHARED_REFUSALS)
def test_entry_points_refuse_before_any_hip_call(which, bad, fragment):
    rc, msg = _call(which, **bad)
    assert rc == _lib.EINVAL and fragment in msg, (bad, msg)


@pytest.mark.parametrize("which,bad,fragment", [
    ("dispersions", dict(prior=[0.0] * 5, pv=0.0), b"prior_var"), ("dispersions", dict(prior=[0.0] * 5, pv=-1.0), b"prior_var"),
    ("dispersions", dict(prior=[0.0] * 5, pv=np.nan), b"prior_var"), ("dispersions", dict(prior=[0.0] * 5, pv=np.inf), b"prior_var"),
    ("group_fits", dict(disp=None), b"NULL"),
    ("group_fits", dict(disp=[0.1, 0.1, 9e-9, 0.1, 0.1]), b"dispersion[2]"), ("group_fits", dict(disp=[10.5] + [0.1] * 4), b"dispersion[0]"),
    ("group_fits", dict(disp=[0.1, np.inf, 0.1, 0.1, 0.1]), b"dispersion[1]"), ("group_fits", dict(disp=[0.1, 0.1, 0.1, -1.0, 0.1]), b"dispersion[3]"),
])
def test_entry_points_refuse_their_own_arguments(which, bad, fragment):
    rc, msg = _call(which, **bad)
    assert rc == _lib.EINVAL and fragment in msg, (bad, msg)


def test_too_many_samples_are_refused_before_any_hip_call():
    L = _lib.load()
    m = L.pilot_ot_nb_glm_max_samples() + 1
    assert m - 1 >= 4096 and engine.nb_glm_limits() == m - 1
    Y, codes, sf, out = np.ones((m, 1)), np.zeros(m, dtype=np.int32), np.ones(m), np.zeros(2)
    codes[::2] = 1
    rc = L.pilot_ot_nb_dispersions(ctypes.c_void_p(Y.ctypes.data), 0, 1, m, 1, 1, _lib.iptr(codes), 2, _lib.dptr(sf), None, 0.0,
                                   _lib.dptr(out), _lib.dptr(out[1:]), None, None, None)
    assert rc == _lib.ENOTSUP and b"staged in LDS" in L.pilot_ot_last_error()
    with pytest.raises(NotImplementedError, match="samples"):
        engine.nb_dispersions(Y, codes, 2, sf)
    assert 8 * (2 * (m - 1) + (m - 2)) <= 160 * 1024                # counts, fitted means and group means within the LDS


def test_good_arguments_get_as_far_as_the_device():
    want = _lib.OK if _lib.device_count() > 0 else _lib.EHIP
    for which, kw in (("dispersions", dict()), ("dispersions", dict(prior=[0.0] * 5, pv=0.5)), ("dispersions", dict(ld=8)),
                      ("dispersions", dict(ng=5, codes=[0, 1, 2, 3, 4, 4])), ("group_fits", dict()),
                      ("group_fits", dict(disp=[1e-8, 10.0, np.nan, 0.1, 0.1])), ("group_fits", dict(dtype=0))):
        rc, msg = _call(which, **kw)
        assert rc == want, (which, kw, msg)


def test_symbols():
    for name in ("pilot_ot_nb_dispersions", "pilot_ot_nb_group_fits", "pilot_ot_nb_glm_max_samples"):
        assert name in _lib.SYMBOLS
    assert (_lib.NB_NOT_CONVERGED, _lib.NB_FLOORED) == (RR.NOT_CONVERGED, RR.FLOORED) == (1, 2)


# ---- engine and tl --------------------------------------------------------------------------------------------------------------------
Y6 = np.ones((6, 5))
C6, S6 = np.array([0, 1, 0, 1, 1, 0]), np.array([1.0, 0.5, 2.0, 1.0, 1.5, 0.7])


@pytest.mark.parametrize("kw", [
    dict(counts=np.ones(6)), dict(counts=np.ones((6, 5), dtype=np.int64)), dict(counts=np.ones((6, 8))[:, :5]), dict(counts=np.ones((6, 0))),
    dict(counts=np.ones((1, 5)), codes=[0], size_factors=[1.0]),
    dict(n_groups=1), dict(n_groups=6), dict(n_groups=2.5), dict(n_groups=True), dict(n_groups=3),
    dict(codes=C6[:5]), dict(codes=C6.astype(float)), dict(codes=[0, 1, 0, 1, 2, 0]), dict(codes=[0, -1, 0, 1, 1, 0]), dict(codes=[1] * 6),
    dict(size_factors=S6[:5]), dict(size_factors=[1.0, 0.0, 2.0, 1.0, 1.5, 0.7]), dict(size_factors=[1.0, np.nan, 2.0, 1.0, 1.5, 0.7]),
    dict(size_factors=-S6),
])
def test_engine_refuses_before_the_library(no_library, kw):
    a = dict(counts=Y6, codes=C6, n_groups=2, size_factors=S6)
    a.update(kw)
    with pytest.raises(ValueError):
        engine.nb_dispersions(**a)
    with pytest.raises(ValueError):
        engine.nb_group_fits(dispersion=np.full(np.shape(a["counts"])[-1], 0.1), **a)


def test_engine_refuses_its_own_arguments(no_library):
    for kw in (dict(log_prior_mean=np.zeros(5)), dict(prior_var=1.0), dict(log_prior_mean=np.zeros(4), prior_var=1.0),
               dict(log_prior_mean=np.zeros(5), prior_var=0.0), dict(log_prior_mean=np.zeros(5), prior_var=np.nan),
               dict(log_prior_mean=np.zeros(5), prior_var=-1.0)):
        with pytest.raises(ValueError):
            engine.nb_dispersions(Y6, C6, 2, S6, **kw)
    for disp in (np.full(4, 0.1), np.array([0.1, 0.1, 9e-9, 0.1, 0.1]), np.array([0.1, 10.5, 0.1, 0.1, 0.1]),
                 np.array([0.1, np.inf, 0.1, 0.1, 0.1])):
        with pytest.raises(ValueError):
            engine.nb_group_fits(Y6, C6, 2, S6, disp)


def _de_inputs():
    counts = pd.DataFrame(np.arange(1.0, 31.0).reshape(6, 5), index=list("abcdef"), columns=["g%d" % j for j in range(5)])
    meta = pd.DataFrame({"Predicted_Labels": ["T1", "T2", "T1", "T3", "T2", "T1"], "stage": ["T1", "T2", "T1", "T3", "T2", "T1"]},
                        index=list("abcdef"))
    return counts, meta


def test_tl_refuses_before_the_library(no_library):
    counts, meta = _de_inputs()
    for g1, g2 in (("T1", "T9"), ("T9", "T1"), ("T1", "T1")):
        with pytest.raises(ValueError):
            tl.compute_pseudobulk_DE(counts, meta, group1=g1, group2=g2, cluster_col="Predicted_Labels")
    with pytest.raises(ValueError, match="cluster_col"):
        tl.compute_pseudobulk_DE(counts, meta, group1="T1", group2="T2", cluster_col="nope")
    with pytest.raises(ValueError, match="residual"):
        tl.compute_pseudobulk_DE(counts.iloc[[0, 3]], meta.iloc[[0, 3]], group1="T1", group2="T3", cluster_col="Predicted_Labels")
    with pytest.raises(ValueError):
        tl.deseq2_dispersions(counts, ["x", "y", "x", "y", "y"])
    with pytest.raises(ValueError):
        tl.deseq2_dispersions(counts, ["x"] * 6)
    with pytest.raises(ValueError):
        tl.deseq2_dispersions(counts, list("uvwxyz"))
    with pytest.raises(ValueError):
        tl.deseq2_dispersions(counts, ["x", "y", "x", "y", "y", "x"], size_factors=np.ones(5))
    with pytest.raises(ValueError):
        tl.deseq2_dispersions(np.ones(6), ["x", "y", "x", "y", "y", "x"])
