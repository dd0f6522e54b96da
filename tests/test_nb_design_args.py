"""The negative-binomial GLM for a general design (K26), the parts that need no device.

The restatement (tests/nb_design_restatement.py) is pinned to scipy on its own: its inner fit to scipy.optimize.minimize on the
penalised likelihood written with stats.nbinom.logpmf (1e-6, scipy's tolerance), its L to nbinom.logpmf and numpy's slogdet, its
covariance and log likelihood to numpy's inverse and nbinom.logpmf.  THE CAP THAT KEEPS THE PARITY TEST HONEST: on the (12, 4) case
the restatement alone must resolve at least 90 % of the NB-class genes, or "dispersions agree on the resolved genes" says little.
tl.deseq2_design: level order, scaling, every refusal.  tl.compute_pseudobulk_DE(covariates=...) runs with the two device calls
replaced by the restatement, against the host tail written out here.  The C entry points refuse every bad argument before any HIP
call; engine and tl raise before the library is touched."""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest
from scipy import optimize, stats

import nb_design_restatement as D
import nb_glm_restatement as RR
from pilot_amd import _lib, engine, tl


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())


@functools.lru_cache(maxsize=None)
def case_12_4(G=40):
    """the issue's prototype: m = 12, p = 4 (intercept, batch, scaled age, group), NB genes with planted coefficients; gene 0 has a
    group of zeros"""
    rng = np.random.default_rng(26)
    s = D.size_factors(rng, 12)
    X, kinds = D.make_design(rng, 12, 4)
    assert kinds == ["intercept", "batch", "age", "group"]
    c = D.nb_class(rng, s, X, kinds, G)
    c[X[:, -1] == 1, 0] = 0.0
    x, L = D.dispersions(c, X, s)
    # where the pins compare with stats.nbinom.logpmf they do so at max(alpha, 1e-3): at r = 1 / alpha = 1e8, where a gene without
    # overdispersion ends, scipy's logpmf carries an error of 1e-6 (it differences terms of size r)
    return dict(s=s, X=X, c=c, x=x, L=L, alpha=np.exp(x), alpha_pin=np.maximum(np.exp(x), 1e-3))


# ---- pins for the restatement -------------------------------------------------------------------------------------------------------
def test_the_inner_fit_is_scipys_minimum_of_the_penalised_likelihood():
    C = case_12_4()
    c, X, s, alpha = C["c"], C["X"], C["s"], C["alpha_pin"]
    beta, steps, conv = D.fit(c, X, s, alpha)
    assert conv.all() and steps.max() <= 60
    assert beta[0, -1] < -15                                             # the group of zeros: separation, held finite by the ridge
    worst = 0.0
    for g in range(c.shape[1]):
        def f(b):
            return -D.penalised_loglik(c[:, g], X, s, alpha[g], b)

        def jac(b):                                                       # d/d eta nbinom.logpmf = (c - mu) / (1 + alpha mu)
            mu = s * np.exp(X @ b)
            return -(X.T @ ((c[:, g] - mu) / (1.0 + alpha[g] * mu)) - D.RIDGE * b)

        def hess(b):
            mu = s * np.exp(X @ b)
            return (X * (mu * (1.0 + alpha[g] * c[:, g]) / (1.0 + alpha[g] * mu) ** 2)[:, None]).T @ X + D.RIDGE * np.eye(4)

        np.testing.assert_allclose(optimize.approx_fprime(beta[g] + 0.1, f, 1e-7), jac(beta[g] + 0.1), rtol=1e-4, atol=1e-4)
        start = np.array([np.log(max((c[:, g] / s).mean(), 0.5)), 0.0, 0.0, 0.0])
        got = optimize.minimize(f, start, jac=jac, hess=hess, method="trust-exact", options={"gtol": 1e-12, "maxiter": 2000})
        assert f(beta[g]) <= got.fun + 1e-9 * abs(got.fun)               # the restatement's point is at least as good
        worst = max(worst, np.abs(got.x - beta[g]).max())
    print("max |beta - scipy| = %.3g" % worst)
    assert worst <= 1e-6


def test_the_newton_step_vanishes_at_the_fit_and_nowhere_else():
    C = case_12_4()
    beta = D.fit(C["c"], C["X"], C["s"], C["alpha"])[0]
    assert np.abs(D.newton_step(C["c"], C["X"], C["s"], C["alpha"], beta)).max() <= 1e-12
    assert np.abs(D.newton_step(C["c"], C["X"], C["s"], C["alpha"], beta + 1e-6)).max() >= 1e-7


def test_L_is_logpmf_and_slogdet():
    C = case_12_4()
    c, X, s, x = C["c"], C["X"], C["s"], np.log(C["alpha_pin"])
    beta = D.fit(c, X, s, np.exp(x))[0]
    L = D.objective(c, X, s, x)
    seen = 0
    for g in range(c.shape[1]):
        mu = s * np.exp(X @ beta[g])
        if mu.min() < D.MIN_MU:
            continue
        seen += 1
        a = np.exp(x[g])
        w = mu / (1.0 + a * mu)
        want = (stats.nbinom.logpmf(c[:, g], 1.0 / a, 1.0 / (1.0 + a * mu)).sum() + RR.special.gammaln(c[:, g] + 1.0).sum()
                - 0.5 * np.linalg.slogdet((X * w[:, None]).T @ X)[1])
        assert abs(L[g] - want) <= 1e-9 * max(abs(want), 1.0), g
    assert seen >= 30
    # the floor: the gene with a group of zeros is evaluated at max(mu, 0.5)
    mu0 = s * np.exp(X @ beta[0])
    assert mu0.min() < 1e-4 and np.isfinite(L[0])
    prior = x + 0.3
    np.testing.assert_allclose(D.objective(c, X, s, x, prior, 0.7), L - 0.09 / 1.4, rtol=1e-12)


def test_final_fit_outputs_are_numpys_inverse_and_logpmf():
    C = case_12_4()
    c, X, s, alpha = C["c"], C["X"], C["s"], C["alpha_pin"]
    beta, cov, loglik = D.final_fit(c, X, s, alpha)
    for g in (0, 1, 7):
        mu = s * np.exp(X @ beta[g])
        fl = np.maximum(mu, 0.5)
        want = np.linalg.inv((X * (fl / (1.0 + alpha[g] * fl))[:, None]).T @ X + 1e-6 * np.eye(4))
        np.testing.assert_allclose(cov[g], want, rtol=1e-10)
        np.testing.assert_allclose(loglik[g], stats.nbinom.logpmf(c[:, g], 1.0 / alpha[g], 1.0 / (1.0 + alpha[g] * mu)).sum(), rtol=1e-10)
    zero = c.copy()
    zero[:, 3] = 0.0
    a = alpha.copy()
    a[5] = np.nan
    beta, cov, loglik = D.final_fit(zero, X, s, a)
    assert np.isnan(beta[[3, 5]]).all() and np.isnan(cov[[3, 5]]).all() and np.isnan(loglik[[3, 5]]).all() and np.isfinite(beta[4]).all()
    lfc, se, stat, p = D.wald(beta, cov, [0, 0, 0, 1])
    np.testing.assert_allclose(lfc[4], beta[4, 3] / np.log(2.0))
    np.testing.assert_allclose(se[4], np.sqrt(cov[4, 3, 3]) / np.log(2.0))
    np.testing.assert_allclose(p[4], 2 * stats.norm.sf(abs(lfc[4] / se[4])))


def test_the_restatement_alone_resolves_the_nb_class():
    """the cap: the prototype resolved 39 of 39"""
    C = case_12_4()
    res = D.resolved(C["c"], C["X"], C["s"], C["x"])
    nb = np.arange(1, 40)                                                 # (gene 0 carries the group of zeros)
    print("resolved %d of %d NB genes" % (res[nb].sum(), nb.size))
    assert res[nb].sum() >= 0.9 * nb.size


def test_one_factor_design_agrees_with_the_group_roots_within_the_ridge_bound():
    """X = [1, indicator]: beta0 = log q1 and beta0 + beta1 = log q2 of K22's group fits, up to the ridge's pull lambda |beta| / lambda_min"""
    rng = np.random.default_rng(3)
    m, G = 9, 30
    s = D.size_factors(rng, m)
    codes = (np.arange(m) >= 5).astype(int)
    X = np.stack([np.ones(m), codes.astype(float)], axis=1)
    c = RR.nb_class(rng, s, codes, 2, G)
    alpha = np.full(G, 0.2)
    beta = D.fit(c, X, s, alpha)[0]
    q, _, flags = RR.group_fits(c, codes, 2, s, alpha)
    ok = (flags == 0).all(axis=1)
    assert ok.sum() >= 25
    mu = s[:, None] * np.exp(X @ beta.T)
    w = mu * (1.0 + alpha[None] * c) / (1.0 + alpha[None] * mu) ** 2
    lam_min = np.array([np.linalg.eigvalsh((X * w[:, g][:, None]).T @ X)[0] for g in range(G)])
    limit = D.RIDGE * np.linalg.norm(beta, axis=1) / lam_min + 1e-9
    assert (np.abs(beta[:, 0] - np.log(q[:, 0]))[ok] <= limit[ok]).all()
    assert (np.abs(beta[:, 0] + beta[:, 1] - np.log(q[:, 1]))[ok] <= limit[ok]).all()


# ---- tl.deseq2_design -------------------------------------------------------------------------------------------------------------------
def _meta():
    idx = ["s%d" % i for i in range(10)]
    return pd.DataFrame({
        "Predicted_Labels": ["T1", "T2", "T1", "T2", "T3", "T1", "T2", "T1", "T2", "T2"],
        "batch": ["b10", "b2", "b2", "b10", "b2", "b9", "b9", "b10", "b2", "b9"],
        "sex": pd.Categorical(["m", "f", "f", "m", "f", "m", "f", "f", "m", "m"], categories=["m", "f"]),
        "smoker": [True, False, True, True, False, False, True, False, False, True],
        "age": [30.0, 41.0, 52.0, 38.0, 60.0, 45.0, 33.0, 58.0, 49.0, 36.0],
        "n": [1, 2, 3, 4, 5, 6, 7, 8, 9, 10],
        "flat": [2.0] * 10,
        "site": ["x"] * 10,
        "twin": ["u", "v", "u", "v", "w", "u", "v", "u", "v", "v"],
        "age2": [2 * a + 1 for a in [30.0, 41.0, 52.0, 38.0, 60.0, 45.0, 33.0, 58.0, 49.0, 36.0]],
    }, index=idx)


def test_design_columns_levels_and_scaling():
    meta = _meta()
    X, names, index = tl.deseq2_design(meta, "Predicted_Labels", "T1", "T2", ["batch", "age", "sex", "smoker", "n"])
    assert list(index) == [s for s in meta.index if s != "s4"]                     # T3 is not selected
    assert names == ["Intercept", "batch_b2", "batch_b9", "age", "sex_m", "smoker_True", "n", "Predicted_Labels_T2_vs_T1"]
    sub = meta.loc[index]
    assert X.dtype == np.float64 and X.shape == (9, 8) and (X[:, 0] == 1).all()
    # Python string order: "b10" < "b2" < "b9", "f" < "m" whatever the categorical's own order, "False" < "True"
    np.testing.assert_array_equal(X[:, 1], (sub["batch"] == "b2").to_numpy().astype(float))
    np.testing.assert_array_equal(X[:, 2], (sub["batch"] == "b9").to_numpy().astype(float))
    np.testing.assert_array_equal(X[:, 4], (sub["sex"] == "m").to_numpy().astype(float))
    np.testing.assert_array_equal(X[:, 5], sub["smoker"].to_numpy().astype(float))
    np.testing.assert_array_equal(X[:, 7], (sub["Predicted_Labels"] == "T2").to_numpy().astype(float))
    age = sub["age"].to_numpy()
    np.testing.assert_allclose(X[:, 3], (age - age.mean()) / age.std(ddof=1), rtol=1e-14)
    assert abs(X[:, 3].mean()) < 1e-14 and abs(X[:, 3].std(ddof=1) - 1) < 1e-14 and abs(X[:, 6].std(ddof=1) - 1) < 1e-14
    X2, names2, _ = tl.deseq2_design(meta, "Predicted_Labels", "T2", "T1", [])
    assert names2 == ["Intercept", "Predicted_Labels_T1_vs_T2"] and X2.shape == (9, 2)
    np.testing.assert_array_equal(X2[:, 1], 1.0 - X[:, 7])


@pytest.mark.parametrize("covariates,fragment", [
    (["flat"], "'flat' is constant"), (["site"], "'site' is constant"), (["nope"], "'nope' is not a column"),
    (["Predicted_Labels"], "'Predicted_Labels' is not a column"),
    (["age", "age2"], "'age2' is confounded with the columns before it"),
    (["batch", "twin"], "group column 'Predicted_Labels' is confounded"),
])
def test_design_refusals(covariates, fragment):
    with pytest.raises(ValueError, match=fragment):
        tl.deseq2_design(_meta(), "Predicted_Labels", "T1", "T2", covariates)


def test_design_refuses_missing_values_and_bad_groups():
    meta = _meta()
    meta.loc["s2", "age"] = np.nan
    with pytest.raises(ValueError, match="'age' has a missing value in sample 's2'"):
        tl.deseq2_design(meta, "Predicted_Labels", "T1", "T2", ["age"])
    tl.deseq2_design(meta, "Predicted_Labels", "T2", "T3", ["age"])                 # s2 is T1: not selected
    with pytest.raises(ValueError, match="both"):
        tl.deseq2_design(meta, "Predicted_Labels", "T1", "T1", [])
    with pytest.raises(ValueError, match="cluster_col"):
        tl.deseq2_design(meta, "stage", "T1", "T2", [])


def test_obs_columns_must_be_constant_within_a_sample():
    obs = pd.DataFrame({"sampleID": ["a", "a", "b", "b", "c"], "batch": ["x", "x", "y", "y", "x"], "age": [3.0, 3.0, 4.0, 5.0, 6.0]})

    class A:
        pass

    A.obs = obs
    got = tl._sample_constant_obs(A, "sampleID", ["batch"], pd.Index(["c", "a", "b"]))
    assert got["batch"].tolist() == ["x", "x", "y"] and got.index.tolist() == ["c", "a", "b"]
    with pytest.raises(ValueError, match=r"obs\['age'\] is not constant within sample 'b'"):
        tl._sample_constant_obs(A, "sampleID", ["batch", "age"], pd.Index(["a", "b", "c"]))
    with pytest.raises(ValueError, match="nope"):
        tl._sample_constant_obs(A, "sampleID", ["nope"], pd.Index(["a"]))


# ---- tl on the restatement ----------------------------------------------------------------------------------------------------------------
def _bh(p):
    order = np.argsort(p, kind="stable")
    scaled = p[order] * p.size / np.arange(1, p.size + 1)
    out = np.empty(p.size)
    out[order] = np.minimum(np.minimum.accumulate(scaled[::-1])[::-1], 1.0)
    return out


def design_table_by_hand(c, X, sf, fit_type="parametric"):
    """tl.deseq2_dispersions(design=X) from the engine calls: (frame columns as arrays, prior_var, var_log_disp)"""
    m, p = X.shape
    x = engine.nb_design_dispersions(c, X, sf)
    q = np.rint(c) / sf[:, None]
    base = np.where(np.isnan(x), np.nan, q.mean(axis=0))
    var = np.where(np.isnan(x), np.nan, q.var(axis=0, ddof=1))
    clip = lambda d: np.clip(d, RR.MIN_DISP, RR.max_disp(m))
    fit, _ = engine.nb_trend(base, clip(np.exp(x)), fit_type)
    pv, vld = RR.prior_var(x, np.log(fit), m, p)
    x_map = engine.nb_design_dispersions(c, X, sf, log_prior_mean=np.log(fit), prior_var=pv)
    flags = RR.outliers(x, np.log(fit), vld)
    return dict(baseMean=base, baseVar=var, dispGeneEst=clip(np.exp(x)), dispFit=fit, dispMAP=clip(np.exp(x_map)),
                dispersion=np.where(flags, clip(np.exp(x)), clip(np.exp(x_map))), dispOutlier=flags), pv, vld


def design_de_by_hand(counts, meta, group1, group2, cluster_col, covariates, test="wald", filtering_alpha=None):
    """tl.compute_pseudobulk_DE(covariates=...) from the engine calls and the host tail of step 6 written out"""
    X, names, index = tl.deseq2_design(meta, cluster_col, group1, group2, covariates)
    sub = counts.loc[index]
    c = np.ascontiguousarray(sub.to_numpy(dtype=np.float64))
    sf = tl.deseq2_size_factors(sub).to_numpy()
    table, _, _ = design_table_by_hand(c, X, sf)
    disp = table["dispersion"]
    beta, cov, loglik = engine.nb_design_fits(c, X, sf, disp)
    a = np.zeros(X.shape[1])
    a[-1] = 1.0
    lfc, se, stat, p = D.wald(beta, cov, a)
    if test == "lrt":
        stat, p = D.lrt(loglik, engine.nb_design_fits(c, np.ascontiguousarray(X[:, :-1]), sf, disp)[2])
    if filtering_alpha is None:
        padj = np.full(p.size, np.nan)
        padj[~np.isnan(p)] = _bh(p[~np.isnan(p)])
    else:
        padj = engine.independent_filtering(p, table["baseMean"], filtering_alpha)[0]
    frame = pd.DataFrame({"gene": np.asarray(sub.columns), "baseMean": table["baseMean"], "log2FoldChange": lfc, "lfcSE": se, "stat": stat,
                          "pvalue": p, "padj": padj, "dispersion": disp})
    return frame.iloc[np.argsort(padj, kind="stable")].reset_index(drop=True), X, names, beta


@functools.lru_cache(maxsize=None)
def pseudobulk_with_batch(G=60):
    """12 samples in three sub-groups (5, 4, 3) with a batch, a scaled age and a sex column, G NB genes with planted batch and age
    effects; gene 5 is zero everywhere, genes 9 and 10 are copies (tied padj)"""
    rng = np.random.default_rng(11)
    s = RR.size_factors(rng, 12)
    codes = rng.permutation(np.repeat(np.arange(3), (5, 4, 3)))
    batch = np.arange(12) % 2
    age = rng.normal(50.0, 10.0, 12)
    base = np.exp(rng.uniform(np.log(5.0), np.log(2000.0), G))
    effect = rng.normal(0.0, 0.5, G)[None] * batch[:, None] + rng.normal(0.0, 0.3, G)[None] * ((age - age.mean()) / age.std(ddof=1))[:, None]
    effect += np.where(rng.random(G) < 0.3, rng.normal(0.0, 1.0, G), 0.0)[None] * (codes == 1)[:, None]
    c = RR.nb_counts(rng, s[:, None] * base[None] * np.exp(effect), (0.05 + 2.0 / base)[None])
    c[:, 5] = 0.0
    c[:, 10] = c[:, 9]
    samples = ["s%02d" % i for i in range(12)]
    counts = pd.DataFrame(c, index=samples, columns=["g%03d" % j for j in range(G)])
    labels = np.array(["T1", "T2", "T3"])[codes]
    meta = pd.DataFrame({"Predicted_Labels": labels, "stage": labels, "batch": np.array(["A", "B"])[batch], "age": age}, index=samples)
    return counts, meta


def _fakes(monkeypatch):
    """the two device calls of the K26 route replaced by the restatement"""
    def dispersions(counts, design, size_factors, log_prior_mean=None, prior_var=None, return_info=False):
        return D.dispersions(np.asarray(counts), design, size_factors, log_prior_mean, prior_var)[0]

    def fits(counts, design, size_factors, dispersion, return_info=False):
        out = D.final_fit(np.asarray(counts), design, size_factors, dispersion)
        return out + ({"n_not_converged": 0},) if return_info else out

    monkeypatch.setattr(engine, "nb_design_dispersions", dispersions)
    monkeypatch.setattr(engine, "nb_design_fits", fits)


@pytest.mark.parametrize("test,filtering", [("wald", False), ("lrt", False), ("wald", True)])
def test_tl_design_route_on_the_restatement(monkeypatch, test, filtering):
    _fakes(monkeypatch)
    counts, meta = pseudobulk_with_batch()
    args = dict(group1="T1", group2="T2", cluster_col="Predicted_Labels")
    out = tl.compute_pseudobulk_DE(counts, meta, covariates=["batch", "age"], test=test, independent_filtering=filtering, alpha=0.1, **args)
    want, X, names, beta = design_de_by_hand(counts, meta, covariates=["batch", "age"], test=test, filtering_alpha=0.1 if filtering else None,
                                             **args)
    assert list(out.columns) == ["gene", "baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "padj", "dispersion"]
    pd.testing.assert_frame_equal(out, want, check_exact=True)
    assert out.attrs["test"] == test and out.attrs["n_not_converged"] == 0
    assert list(out.attrs["design"].columns) == names == ["Intercept", "batch_B", "age", "Predicted_Labels_T2_vs_T1"]
    np.testing.assert_array_equal(out.attrs["design"].to_numpy(), X)
    assert out.attrs["design"].index.tolist() == [s for s in counts.index if meta.loc[s, "stage"] != "T3"]
    np.testing.assert_array_equal(out.attrs["coefficients"].to_numpy(), beta)
    assert out.attrs["coefficients"].index.tolist() == counts.columns.tolist()
    assert ("independent_filtering" in out.attrs) == filtering
    assert out["gene"].iloc[-1] == "g005" and out.iloc[-1, 1:].isna().all()
    pos = {g: i for i, g in enumerate(out["gene"])}
    assert pos["g009"] + 1 == pos["g010"]
    if test == "lrt":                                                     # the fold change and its error stay the Wald ones
        wald = tl.compute_pseudobulk_DE(counts, meta, covariates=["batch", "age"], **args).set_index("gene")
        lrt = out.set_index("gene").loc[wald.index]
        pd.testing.assert_frame_equal(lrt[["log2FoldChange", "lfcSE", "dispersion"]], wald[["log2FoldChange", "lfcSE", "dispersion"]])
        live = wald["stat"].notna()
        assert (lrt["stat"][live] >= -1e-9).all()
        # asymptotically the same test: the two statistics agree in rank
        assert stats.spearmanr(lrt["stat"][live], wald["stat"][live] ** 2)[0] > 0.95


def test_tl_dispersions_with_a_design_on_the_restatement(monkeypatch):
    _fakes(monkeypatch)
    counts, meta = pseudobulk_with_batch()
    X, names, index = tl.deseq2_design(meta, "Predicted_Labels", "T1", "T3", ["batch"])
    sub = counts.loc[index]
    out = tl.deseq2_dispersions(sub, design=pd.DataFrame(X, index=index, columns=names))
    want, pv, vld = design_table_by_hand(np.ascontiguousarray(sub.to_numpy()), X, tl.deseq2_size_factors(sub).to_numpy())
    assert list(out.columns) == list(want)
    for name in want:
        np.testing.assert_array_equal(out[name].to_numpy(), want[name], err_msg=name)
    assert (out.attrs["prior_var"], out.attrs["var_log_disp"]) == (pv, vld)
    with pytest.raises(ValueError, match="groups and design"):
        tl.deseq2_dispersions(sub, np.zeros(len(sub)), design=X)


# ---- the C entry points ---------------------------------------------------------------------------------------------------------------------
X6 = [[1.0, 0.0, -1.0], [1.0, 1.0, 0.5], [1.0, 0.0, 0.2], [1.0, 1.0, 1.3], [1.0, 1.0, -0.7], [1.0, 0.0, 0.1]]
GOOD = dict(y=True, dtype=1, m=6, genes=5, ld=5, X=X6, p=3, sf=[1.0, 0.5, 2.0, 1.0, 1.5, 0.7], disp=[0.1] * 5, prior=None, pv=0.0, out=True)


def _call(which, **kw):
    a = dict(GOOD)
    a.update(kw)
    L = _lib.load()
    Y = np.ones((6, 8), dtype=np.float64)
    arr = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    X, sf, disp, prior = arr(a["X"]), arr(a["sf"]), arr(a["disp"]), arr(a["prior"])
    ptr = lambda v: None if v is None else _lib.dptr(v)
    d = [np.zeros(512) for _ in range(3)]
    i = [np.zeros(64, dtype=np.int32) for _ in range(2)]
    bad_row, bad_col, n_bad = ctypes.c_longlong(5), ctypes.c_int(5), ctypes.c_int(5)
    y = ctypes.c_void_p(Y.ctypes.data) if a["y"] else None
    if which == "dispersions":
        rc = L.pilot_ot_nb_design_dispersions(y, 0, a["dtype"], a["m"], a["genes"], a["ld"], ptr(X), a["p"], ptr(sf), ptr(prior), a["pv"],
                                              _lib.dptr(d[0]) if a["out"] else None, _lib.dptr(d[1]), _lib.dptr(d[2]), _lib.iptr(i[0]),
                                              _lib.iptr(i[1]), ctypes.byref(n_bad), ctypes.byref(bad_row), ctypes.byref(bad_col))
    else:
        rc = L.pilot_ot_nb_design_fits(y, 0, a["dtype"], a["m"], a["genes"], a["ld"], ptr(X), a["p"], ptr(sf), ptr(disp),
                                       _lib.dptr(d[0]) if a["out"] else None, _lib.dptr(d[1]), _lib.dptr(d[2]), _lib.iptr(i[0]), _lib.iptr(i[1]),
                                       ctypes.byref(n_bad), ctypes.byref(bad_row), ctypes.byref(bad_col))
    assert bad_row.value == -1 and bad_col.value == -1 and n_bad.value == 0
    return rc, L.pilot_ot_last_error()


def _wide(p):
    return [[1.0] + [float((j >> k) & 1) for k in range(p - 1)] for j in range(6)]


BAD = [
    (dict(y=False), b"NULL"), (dict(X=None), b"NULL"), (dict(sf=None), b"NULL"), (dict(out=False), b"NULL"),
    (dict(genes=0, ld=0), b"n_genes=0"), (dict(ld=4), b"ld=4"), (dict(dtype=2), b"dtype"), (dict(m=1), b"m=1"),
    (dict(sf=[1.0, 0.0, 2.0, 1.0, 1.5, 0.7]), b"size_factors[1]"), (dict(sf=[1.0, 0.5, 2.0, np.nan, 1.5, 0.7]), b"size_factors[3]"),
    (dict(p=1), b"p=1"), (dict(p=9), b"p=9"), (dict(p=0), b"p=0"), (dict(p=6, X=_wide(6)), b"no residual degree of freedom"),
    (dict(X=[[1.0, 0.0, -1.0]] * 3 + [[0.5, 1.0, 1.3]] + [[1.0, 1.0, 0.1]] * 2), b"X[3, 0]=0.5"),
    (dict(X=[[1.0, 0.0, -1.0]] * 4 + [[1.0, np.nan, 1.3]] + [[1.0, 1.0, 0.1]]), b"X[4, 1]"),
    (dict(X=[[1.0, 0.0, np.inf]] + [[1.0, 1.0, 0.1]] * 5), b"X[0, 2]"),
]


@pytest.mark.parametrize("bad,fragment", BAD + [(dict(prior=[0.0] * 5, pv=0.0), b"prior_var"), (dict(prior=[0.0] * 5, pv=np.inf), b"prior_var")])
def test_dispersions_entry_point_refuses_before_any_hip_call(bad, fragment):
    rc, msg = _call("dispersions", **bad)
    assert rc == _lib.EINVAL and fragment in msg, (bad, msg)


@pytest.mark.parametrize("bad,fragment", BAD + [(dict(disp=None), b"NULL"), (dict(disp=[0.1, 0.1, 9e-9, 0.1, 0.1]), b"dispersion[2]"),
                                                (dict(disp=[10.5] + [0.1] * 4), b"dispersion[0]")])
def test_fits_entry_point_refuses_before_any_hip_call(bad, fragment):
    rc, msg = _call("fits", **bad)
    assert rc == _lib.EINVAL and fragment in msg, (bad, msg)


def test_limits_and_too_many_samples():
    limits = engine.nb_design_limits()
    assert limits["max_cols"] == engine.NB_DESIGN_MAX_COLS == 8
    for p, limit in limits["max_samples"].items():
        assert 8 * limit * (2 + p) <= 96 * 1024 and (limit == 4096 or 8 * (limit + 1) * (2 + p) > 96 * 1024)
    assert limits["max_samples"][8] >= 1024
    assert _lib.load().pilot_ot_nb_design_max_samples(9) == _lib.EINVAL
    p = 3
    m = limits["max_samples"][p] + 1
    X = np.stack([np.ones(m), np.arange(m) % 2, np.sin(np.arange(m))], axis=1)
    rc, msg = _call("dispersions", m=m, X=X, sf=[1.0] * m, genes=1, ld=1)
    assert rc == _lib.ENOTSUP and b"staged in LDS" in msg
    with pytest.raises(NotImplementedError, match="samples"):
        engine.nb_design_dispersions(np.ones((m, 1)), X, np.ones(m))


def test_good_arguments_get_as_far_as_the_device():
    want = _lib.OK if _lib.device_count() > 0 else _lib.EHIP
    for which in ("dispersions", "fits"):
        for kw in (dict(), dict(ld=8), dict(dtype=0), dict(p=2, X=_wide(2)), dict(p=5, X=[[1.0, j % 2, j % 3 == 0, np.sin(j), j * j / 10.0] for j in range(6)]),
                   dict(disp=[1e-8, 10.0, np.nan, 0.1, 0.1]), dict(prior=[0.0, np.nan, 1.0, -1.0, 0.5], pv=0.5)):
            rc, msg = _call(which, **kw)
            assert rc == want, (which, kw, msg)


def test_symbols():
    for name in ("pilot_ot_nb_design_dispersions", "pilot_ot_nb_design_fits", "pilot_ot_nb_design_max_samples", "pilot_ot_nb_design_max_cols"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)
    assert (D.RIDGE, D.TOL, D.MAX_STEPS) == (engine.NB_DESIGN_RIDGE, 1e-10, 100)


# ---- engine and tl refuse on the host --------------------------------------------------------------------------------------------------------
Y6, S6 = np.ones((6, 5)), np.array([1.0, 0.5, 2.0, 1.0, 1.5, 0.7])
XA = np.array(X6)


@pytest.mark.parametrize("kw", [
    dict(counts=np.ones(6)), dict(counts=np.ones((6, 5), dtype=np.int64)), dict(counts=np.ones((6, 8))[:, :5]),
    dict(design=XA[:5]), dict(design=XA[:, 0]), dict(design=XA[:, :1]), dict(design=np.hstack([XA] * 3)), dict(design=XA.astype(str)),
    dict(design=np.hstack([XA, XA[:, 1:] ** 2, XA[:, 1:] ** 3])[:, :6]),                                      # m - p = 0
    dict(design=np.where(np.arange(3)[None] == 0, 2.0, XA)), dict(design=XA[:, ::-1]),                         # the first column is not ones
    dict(design=np.stack([XA[:, 0], XA[:, 1], 1.0 - XA[:, 1]], axis=1)),                                       # rank 2
    dict(design=np.stack([XA[:, 0], XA[:, 1], XA[:, 1] + 1e-10 * XA[:, 2]], axis=1)),                          # condition number > 1e8
    dict(design=np.where(np.arange(18).reshape(6, 3) == 7, np.nan, XA)),
    dict(size_factors=S6[:5]), dict(size_factors=[1.0, 0.0, 2.0, 1.0, 1.5, 0.7]), dict(size_factors=-S6),
])
def test_engine_refuses_before_the_library(no_library, kw):
    a = dict(counts=Y6, design=XA, size_factors=S6)
    a.update(kw)
    with pytest.raises(ValueError):
        engine.nb_design_dispersions(**a)
    with pytest.raises(ValueError):
        engine.nb_design_fits(dispersion=np.full(5, 0.1), **a)


@pytest.mark.parametrize("kw", [dict(log_prior_mean=np.zeros(5)), dict(prior_var=1.0), dict(log_prior_mean=np.zeros(4), prior_var=1.0),
                                dict(log_prior_mean=np.zeros(5), prior_var=0.0), dict(log_prior_mean=np.zeros(5), prior_var=np.nan)])
def test_engine_refuses_a_bad_prior_before_the_library(no_library, kw):
    with pytest.raises(ValueError):
        engine.nb_design_dispersions(Y6, XA, S6, **kw)


@pytest.mark.parametrize("disp", [np.full(4, 0.1), [0.1, 0.1, 9e-9, 0.1, 0.1], [0.1, np.inf, 0.1, 0.1, 0.1], [10.5, 0.1, 0.1, 0.1, 0.1]])
def test_engine_refuses_bad_dispersions_before_the_library(no_library, disp):
    with pytest.raises(ValueError):
        engine.nb_design_fits(Y6, XA, S6, disp)


def test_good_engine_arguments_reach_the_library(no_library):
    with pytest.raises(AssertionError, match="the library was touched"):
        engine.nb_design_dispersions(Y6, XA, S6)
    with pytest.raises(AssertionError, match="the library was touched"):
        engine.nb_design_fits(Y6, XA, S6, [0.1, np.nan, 1e-8, 10.0, 0.1])


def test_tl_refuses_before_the_library(no_library):
    counts, meta = pseudobulk_with_batch()
    args = dict(group1="T1", group2="T2", cluster_col="Predicted_Labels")
    for kw in (dict(test="LRT"), dict(test="score"), dict(test=None), dict(test=1), dict(test="lrt"), dict(test="lrt", covariates=[]),
               dict(covariates="batch"), dict(covariates=["batch", "batch"]), dict(covariates=[1])):
        with pytest.raises(ValueError):
            tl.compute_pseudobulk_DE(counts, meta, **args, **kw)
        with pytest.raises(ValueError):
            tl.get_pseudobulk_DE(None, None, "alpha", **kw)
    for kw in (dict(shrink="apeglm"), dict(outliers="deseq2"), dict(shrink="apeglm", outliers="deseq2", test="lrt")):
        with pytest.raises(NotImplementedError, match="K23"):
            tl.compute_pseudobulk_DE(counts, meta, covariates=["batch"], **args, **kw)
        with pytest.raises(NotImplementedError, match="K25"):
            tl.get_pseudobulk_DE(None, None, "alpha", covariates=["batch"], **kw)
    for covariates, fragment in ((["nope"], "not a column"), (["stage"], "confounded"), (["batch", "age", "stage"], "confounded")):
        with pytest.raises(ValueError, match=fragment):
            tl.compute_pseudobulk_DE(counts, meta, covariates=covariates, **args)
    wide = meta.copy()
    for k in range(7):
        wide["c%d" % k] = np.sin((k + 1.0) * np.arange(12))
    with pytest.raises(ValueError, match="columns"):                     # 9 design columns
        tl.compute_pseudobulk_DE(counts, wide, covariates=["c%d" % k for k in range(7)], **args)
    with pytest.raises(ValueError, match="residual degree of freedom"):   # T2 and T3: 7 samples, 7 columns
        tl.compute_pseudobulk_DE(counts, wide, covariates=["c%d" % k for k in range(5)], group1="T2", group2="T3", cluster_col="Predicted_Labels")
