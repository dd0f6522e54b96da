"""The negative-binomial GLM for a general design on the device (K26: engine.nb_design_dispersions, engine.nb_design_fits,
tl.compute_pseudobulk_DE(covariates=...), tl.deseq2_dispersions(design=...), tl.get_pseudobulk_DE) against the numpy / scipy
restatement (tests/nb_design_restatement.py, itself pinned to scipy in test_nb_design_args.py).

Shapes (m, p, G): (3, 2, 1) one residual degree of freedom; (4, 3, 63); (12, 4, 257); (65, 6, 64) and (130, 8, 65): samples and
genes across the 64-lane edge, the largest P.  Gene classes, by gene index mod 16: 0-9 NB with planted coefficients, 10 Poisson,
11 constant, 12 huge (means 2e6), 13 a group of zeros (separation), 14 a single non-zero count, 15 all zero.

Tolerances.
  Fits (K24's criterion): the result is DEFINED by the optimum, so the device's coefficients are held to it and not to another
  path's last iterate: the restatement's Newton step evaluated AT the device's beta has infinity norm <= 1e-9, one order above the
  stop rule 1e-10.  Sigma and the log likelihood are then held to the restatement AT THAT beta: Sigma to 1e-9 of its largest entry
  (an entry of an inverse can cancel to nothing, so the error is measured against the matrix; the floored weights keep X^T W X
  conditioned far below 1e7), the log likelihood within B = 64 ulp of the magnitudes added.  Step counts are printed, not asserted.
  Dispersions (K22's two-part rule): the grid search defines the maximiser, and two correct evaluations of L can pick different
  grid points only where L is flat to rounding.  (1) On EVERY gene the restatement's L at the device's x falls short of the
  restatement's own maximum by at most B = 64 * 2^-53 * (sum of the magnitudes added + 4 m + p^2).  (2) On the genes whose
  maximiser the restatement resolves (interior, L drops by more than 2 B at x -+ 1e-4) the dispersions agree to 2e-4 relative.
  One-factor cross-check against K22, an independent route: for X = [1, indicator] the ridge moves the optimum by at most
  lambda |beta| / lambda_min(X^T W X), so |beta0 - log q1| and |beta0 + beta1 - log q2| stay below that plus 1e-9."""
import functools
import itertools

import numpy as np
import pandas as pd
import pytest

import nb_design_restatement as D
import nb_glm_restatement as RR
from pilot_amd import _lib, engine, tl
from test_nb_design_args import design_de_by_hand, design_table_by_hand, pseudobulk_with_batch

pytestmark = pytest.mark.gpu

P_MAX = engine.NB_DESIGN_MAX_COLS
SHAPES = [(3, 2, 1), (4, 3, 63), (12, 4, 257), (65, 6, 64), (130, P_MAX, 65)]
KINDS = ["nb"] * 10 + ["poisson", "constant", "huge", "zero_group", "single", "zero"]
PRIOR_VAR = 0.6


@functools.lru_cache(maxsize=None)
def _case(m, p, G):
    rng = np.random.default_rng(1000 * m + 10 * p + G)
    s = D.size_factors(rng, m)
    X, names = D.make_design(rng, m, p)
    c = D.nb_class(rng, s, X, names, G)
    kind = np.array([KINDS[j % 16] for j in range(G)])
    group = X[:, -1] == 1
    for j in range(G):
        if kind[j] == "poisson":
            c[:, j] = rng.poisson(s * 40.0)
        elif kind[j] == "constant":
            c[:, j] = 11.0
        elif kind[j] == "huge":
            c[:, j] = D.nb_counts(rng, s * 2e6, 0.1)
        elif kind[j] == "zero_group":
            # (the ridge holds the separated coefficient where sum_{j in g} mu_j = lambda |beta_g|, about beta_0 + beta_g = -12: it is
            # below -15 when the other group's mean is above e^3.5, so this class is drawn around 300)
            c[:, j] = np.maximum(D.nb_counts(rng, s * 300.0, 0.1), 1.0)
            c[group, j] = 0.0
        elif kind[j] == "single":
            c[:, j] = 0.0
            c[int(rng.integers(m)), j] = 7.0
        elif kind[j] == "zero":
            c[:, j] = 0.0
    live = (c > 0).any(axis=0)
    prior = np.log(0.05 + 2.0 / np.maximum((c / s[:, None]).mean(axis=0), 1.0))
    x, L = D.dispersions(c, X, s)
    xp, Lp = D.dispersions(c, X, s, prior, PRIOR_VAR)
    out = dict(m=m, p=p, G=G, s=s, X=X, c=c, kind=kind, live=live, prior=prior, x=x, L=L, xp=xp, Lp=Lp,
               alpha=np.clip(np.exp(x), D.MIN_DISP, D.max_disp(m)))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_fits_against_the_restatement(shape):
    C = _case(*shape)
    c, X, s, live, kind = C["c"], C["X"], C["s"], C["live"], C["kind"]
    alpha = C["alpha"].copy()
    if C["G"] > 20:
        alpha[17] = np.nan                                               # a gene left out
    beta, cov, loglik, info = engine.nb_design_fits(c, X, s, alpha, return_info=True)
    assert beta.shape == (C["G"], C["p"]) and cov.shape == (C["G"], C["p"], C["p"]) and loglik.shape == (C["G"],)
    ok = live & ~np.isnan(alpha)
    for name, a in (("beta", beta), ("cov", cov), ("loglik", loglik)):
        np.testing.assert_array_equal(np.isnan(a).reshape(C["G"], -1).any(axis=1), ~ok, err_msg=name)
        assert np.isfinite(a[ok]).all(), name
    assert (info["steps"][~ok] == 0).all() and (info["flags"][~ok] == 0).all()
    assert info["n_not_converged"] == 0 and (info["flags"] == 0).all()
    print("steps: mean %.1f, max %d (%s)" % (info["steps"][ok].mean(), info["steps"].max(), kind[int(np.argmax(info["steps"]))]))
    np.testing.assert_array_equal(cov, np.swapaxes(cov, 1, 2))
    step = np.abs(D.newton_step(c[:, ok], X, s, alpha[ok], beta[ok])).max(axis=1)
    print("the restatement's Newton step at the device's beta: max %.3g" % step.max())
    assert (step <= 1e-9).all()
    want_cov, want_ll, B = D.fit_outputs(c[:, ok], X, s, alpha[ok], beta[ok])
    err = np.abs(cov[ok] - want_cov).max(axis=(1, 2)) / np.abs(want_cov).max(axis=(1, 2))
    print("Sigma: worst error %.3g of the largest entry; loglik: worst %.3g B" % (err.max(), (np.abs(loglik[ok] - want_ll) / B).max()))
    assert (err <= 1e-9).all()
    assert (np.abs(loglik[ok] - want_ll) <= B).all()
    sep = ok & (kind == "zero_group")
    if sep.any():                                                         # separation: the ridge keeps the optimum finite
        assert (beta[sep, -1] < -15).all() and np.isfinite(cov[sep]).all() and (info["flags"][sep] == 0).all()


@pytest.mark.parametrize("with_prior", [False, True], ids=["gene-wise", "MAP"])
@pytest.mark.parametrize("shape", SHAPES)
def test_dispersions_against_the_restatement(shape, with_prior):
    C = _case(*shape)
    c, X, s, live = C["c"], C["X"], C["s"], C["live"]
    prior, pv = (C["prior"], PRIOR_VAR) if with_prior else (None, None)
    want_x, want_L = (C["xp"], C["Lp"]) if with_prior else (C["x"], C["L"])
    x, info = engine.nb_design_dispersions(c, X, s, prior, pv, return_info=True)
    np.testing.assert_array_equal(np.isnan(x), ~live)
    np.testing.assert_array_equal(np.isnan(info["objective"]), ~live)
    np.testing.assert_array_equal(np.isnan(info["beta"]).any(axis=1), ~live)
    assert (info["steps"][~live] == 0).all() and info["n_not_converged"] == 0 and (info["flags"] == 0).all()
    lo, hi = np.log(D.MIN_DISP), np.log(D.max_disp(C["m"]))
    assert ((x[live] >= lo - 1e-12) & (x[live] <= hi + 1e-12)).all()
    print("inner Newton steps per lane and round: mean %.2f, worst gene %.2f" % (info["steps"][live].mean() / 384.0, info["steps"].max() / 384.0))
    cl, pl = c[:, live], None if prior is None else prior[live]
    B = D.bound(cl, X, s, x[live])
    at_device = D.objective(cl, X, s, x[live], pl, pv)
    short = want_L[live] - at_device
    print("shortfall of the restatement's L at the device's x: worst %.3g B; the device's own L differs by at most %.3g B"
          % ((short / B).max(), (np.abs(info["objective"][live] - at_device) / B).max()))
    assert (short <= B).all()
    assert (np.abs(info["objective"][live] - at_device) <= B).all()
    # the coefficients at the winner are the optimum at the winner's dispersion
    step = np.abs(D.newton_step(cl, X, s, np.exp(x[live]), info["beta"][live])).max()
    assert step <= 1e-9, step
    res = D.resolved(c, X, s, want_x, log_prior_mean=prior, prior_var=pv)
    nb = live & (C["kind"] == "nb")
    print("resolved %d of %d genes (%d of %d NB)" % (res.sum(), live.sum(), (res & nb).sum(), nb.sum()))
    if shape == (12, 4, 257):
        assert (res & nb).sum() >= 0.9 * nb.sum()
    rel = np.abs(np.exp(x[res]) - np.exp(want_x[res])) / np.exp(want_x[res])
    if rel.size:
        print("dispersions on the resolved genes: worst relative difference %.3g" % rel.max())
    assert (rel <= 2e-4).all()


def test_one_factor_design_against_the_group_fits():
    """K22 is an independent route: for X = [1, indicator] the K26 coefficients are its group roots up to the ridge's pull"""
    rng = np.random.default_rng(226)
    m, G = 13, 96
    s = D.size_factors(rng, m)
    codes = rng.permutation((np.arange(m) >= 7).astype(np.int32))
    X = np.stack([np.ones(m), codes.astype(np.float64)], axis=1)
    c = RR.nb_class(rng, s, codes, 2, G)
    alpha = np.exp(rng.uniform(np.log(1e-3), np.log(2.0), G))
    beta, cov, _ = engine.nb_design_fits(c, X, s, alpha)
    q, w, info = engine.nb_group_fits(c, codes, 2, s, alpha, return_info=True)
    ok = ((info["flags"] & _lib.NB_FLOORED) == 0).all(axis=1) & (c > 0).any(axis=0)
    assert ok.sum() >= 80
    mu = np.maximum(s[:, None] * np.exp(X @ beta.T), D.MIN_MU)
    W = mu / (1.0 + alpha[None] * mu)
    lam_min = np.array([np.linalg.eigvalsh((X * W[:, g][:, None]).T @ X)[0] for g in range(G)])
    limit = D.RIDGE * np.linalg.norm(beta, axis=1) / lam_min + 1e-9
    d1, d2 = np.abs(beta[:, 0] - np.log(q[:, 0])), np.abs(beta[:, 0] + beta[:, 1] - np.log(q[:, 1]))
    print("worst share of the ridge bound: %.3g" % np.maximum(d1 / limit, d2 / limit)[ok].max())
    assert (d1[ok] <= limit[ok]).all() and (d2[ok] <= limit[ok]).all()
    # and the covariance of an unfloored one-factor fit is K22's: Var(beta1) = 1 / W_1 + 1 / W_2 up to the ridge
    unfloored = ok & (mu > D.MIN_MU).all(axis=0)
    np.testing.assert_allclose(cov[unfloored, 1, 1], (1.0 / w[unfloored, 0] + 1.0 / w[unfloored, 1]), rtol=1e-4)


@pytest.mark.parametrize("shape", SHAPES[1:])
def test_same_bits_by_every_route(shape):
    C = _case(*shape)
    c, X, s, G, alpha = C["c"], C["X"], C["s"], C["G"], C["alpha"]
    small = np.minimum(c, 2.0 ** 24 - 1)                                  # float32 holds every count
    def both(Y, cols=slice(None)):
        x, info = engine.nb_design_dispersions(Y, X, s, return_info=True)
        beta, cov, ll, fi = engine.nb_design_fits(Y, X, s, alpha[cols], return_info=True)
        return [x, info["objective"], info["beta"], info["steps"], beta, cov, ll, fi["steps"]]

    def same(got, want, cols=slice(None)):
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b[cols])

    first = both(small)
    same(both(small), first)
    same(both(small.astype(np.float32)), first)
    dev = engine.DeviceMatrix.upload(small)
    same(both(dev), first)
    same(both(engine.DeviceMatrix.upload(small.astype(np.float32))), first)
    a, b = G // 3, min(G // 3 + 5, G)
    same(both(engine.device_columns(dev, a, b), slice(a, b)), first, slice(a, b))
    for j in sorted({0, G // 2, G - 1, 13 % G}):                          # a gene alone
        same(both(np.ascontiguousarray(small[:, j:j + 1]), slice(j, j + 1)), first, slice(j, j + 1))


def test_limits_and_bad_counts():
    limits = engine.nb_design_limits()
    assert limits["max_cols"] == P_MAX and limits["max_samples"][P_MAX] >= 1024
    m = limits["max_samples"][P_MAX]
    rng = np.random.default_rng(826)
    s = D.size_factors(rng, m)
    X, names = D.make_design(rng, m, P_MAX)
    c = np.concatenate([D.nb_class(rng, s, X, names, 1), np.zeros((m, 1))], axis=1)   # one gene pair: NB and all zero
    x, info = engine.nb_design_dispersions(c, X, s, return_info=True)
    want_x, want_L = D.dispersions(c, X, s)
    assert np.isnan(x[1]) and info["n_not_converged"] == 0
    at_device = D.objective(c[:, :1], X, s, x[:1])
    B = D.bound(c[:, :1], X, s, x[:1])
    print("m = %d: shortfall %.3g B, x %.6f against %.6f" % (m, (want_L[0] - at_device[0]) / B[0], x[0], want_x[0]))
    assert want_L[0] - at_device[0] <= B[0]
    if D.resolved(c, X, s, want_x)[0]:
        assert abs(np.exp(x[0]) - np.exp(want_x[0])) <= 2e-4 * np.exp(want_x[0])
    beta, cov, _ = engine.nb_design_fits(c, X, s, np.clip(np.exp(x), D.MIN_DISP, m))
    assert np.abs(D.newton_step(c[:, :1], X, s, np.exp(x[:1]), beta[:1])).max() <= 1e-9 and np.isnan(beta[1]).all()
    more = np.concatenate([c, c[:1]])
    X1, s1 = np.concatenate([X, X[:1]]), np.concatenate([s, s[:1]])       # one sample more
    with pytest.raises(NotImplementedError, match="staged in LDS"):
        engine.nb_design_dispersions(more, X1, s1)
    bad = c[:200].copy()
    bad[157, 1] = -1.0
    bad[33, 1] = np.nan
    with pytest.raises(ValueError, match=r"Y\[33, 1\]") as err:
        engine.nb_design_dispersions(bad, X[:200], s[:200])
    assert (err.value.row, err.value.col) == (33, 1)
    with pytest.raises(ValueError, match=r"Y\[33, 1\]"):
        engine.nb_design_fits(bad, X[:200], s[:200], np.full(2, 0.1))


# ---- tl ---------------------------------------------------------------------------------------------------------------------------
ARGS = dict(group1="T1", group2="T2", cluster_col="Predicted_Labels")


@pytest.mark.parametrize("test,filtering", [("wald", False), ("lrt", False), ("lrt", True)])
def test_compute_pseudobulk_DE_with_covariates_is_the_host_tail_of_the_engine_calls(test, filtering):
    counts, meta = pseudobulk_with_batch()
    out = tl.compute_pseudobulk_DE(counts, meta, covariates=["batch", "age"], test=test, independent_filtering=filtering, alpha=0.1, **ARGS)
    want, X, names, beta = design_de_by_hand(counts, meta, covariates=["batch", "age"], test=test, filtering_alpha=0.1 if filtering else None,
                                             **ARGS)
    assert list(out.columns) == ["gene", "baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "padj", "dispersion"]
    pd.testing.assert_frame_equal(out, want, check_exact=True)
    assert out.attrs["test"] == test and out.attrs["n_not_converged"] == 0 and list(out.attrs["design"].columns) == names
    np.testing.assert_array_equal(out.attrs["design"].to_numpy(), X)
    np.testing.assert_array_equal(out.attrs["coefficients"].to_numpy(), beta)
    padj = out["padj"].to_numpy()
    n_nan = int(np.isnan(padj).sum())
    assert (np.diff(padj[:len(padj) - n_nan]) >= 0).all() and np.isnan(padj[len(padj) - n_nan:]).all()
    assert out["gene"].iloc[-1] == "g005" and out.iloc[-1, 1:].isna().all()
    assert (out["padj"] < 0.1).sum() >= 3                                 # the planted group effects are found
    # the default route is untouched by the new arguments
    pd.testing.assert_frame_equal(tl.compute_pseudobulk_DE(counts, meta, covariates=None, test="wald", **ARGS),
                                  tl.compute_pseudobulk_DE(counts, meta, **ARGS), check_exact=True)


def test_deseq2_dispersions_with_a_design():
    counts, meta = pseudobulk_with_batch()
    X, names, index = tl.deseq2_design(meta, "Predicted_Labels", "T1", "T3", ["batch"])
    sub = counts.loc[index]
    out = tl.deseq2_dispersions(sub, design=X)
    want, pv, vld = design_table_by_hand(np.ascontiguousarray(sub.to_numpy()), X, tl.deseq2_size_factors(sub).to_numpy())
    assert list(out.columns) == ["baseMean", "baseVar", "dispGeneEst", "dispFit", "dispMAP", "dispersion", "dispOutlier"]
    for name in want:
        np.testing.assert_array_equal(out[name].to_numpy(), want[name], err_msg=name)
    assert (out.attrs["prior_var"], out.attrs["var_log_disp"]) == (pv, vld)
    assert out["dispersion"].between(1e-8, 10.0).sum() == len(out) - 1 and out.loc["g005"].isna()[:-1].all()


class _Adata:
    def __init__(self, X, obs, var_names):
        self.X, self.obs, self.var_names, self.uns = X, obs, var_names, {}


def test_get_pseudobulk_DE_with_covariates_returns_the_keyed_frames():
    """a synthetic AnnData whose per-sample sums of the cell type 'alpha' are the table: the covariates come from adata.obs"""
    counts, meta = pseudobulk_with_batch()
    rng = np.random.default_rng(8)
    rows, sample, cell = [], [], []
    for name in counts.index:
        total = counts.loc[name].to_numpy().astype(np.int64)
        n = 3 + int(rng.integers(4))
        rows.append(rng.multinomial(total, np.full(n, 1.0 / n)).T)
        sample += [name] * (n + 2)
        cell += ["alpha"] * n + ["beta"] * 2
        rows.append(rng.poisson(3.0, (2, total.size)))
    Xc = np.vstack(rows).astype(np.float32)
    shuffle = rng.permutation(Xc.shape[0])
    sample = np.array(sample, dtype=object)[shuffle]
    obs = pd.DataFrame({"cell_types": np.array(cell, dtype=object)[shuffle], "sampleID": sample,
                        "batch": meta.loc[sample, "batch"].to_numpy(), "age": meta.loc[sample, "age"].to_numpy()})
    adata = _Adata(Xc[shuffle], obs, list(counts.columns))
    props = meta[["Predicted_Labels"]]
    kw = dict(celltype_col="cell_types", sample_col="sampleID", cluster_col="Predicted_Labels")
    got_counts, got_meta = tl.pseudobulk_inputs(adata, props, "alpha", obs_columns=["batch", "age"], **kw)
    assert got_meta["batch"].tolist() == meta["batch"].tolist() and got_meta["age"].tolist() == meta["age"].tolist()
    plain = tl.pseudobulk_inputs(adata, props, "alpha", **kw)[1]
    assert list(plain.columns) == ["Predicted_Labels", "stage"]
    out = tl.get_pseudobulk_DE(adata, props, "alpha", covariates=["batch"], test="lrt", **kw)
    assert list(out) == ["T2vsT1", "T3vsT1", "T3vsT2"]
    live = counts.loc[:, (counts != 0).any(axis=0)]
    for (g1, g2), frame in zip(itertools.combinations(["T1", "T2", "T3"], 2), out.values()):
        want = tl.compute_pseudobulk_DE(live, meta, group1=g1, group2=g2, cluster_col="Predicted_Labels", covariates=["batch"], test="lrt")
        pd.testing.assert_frame_equal(frame, want, check_exact=True)
    uneven = obs.copy()
    uneven.loc[np.flatnonzero(sample == "s03")[0], "age"] += 1.0
    with pytest.raises(ValueError, match="not constant within sample 's03'"):
        tl.get_pseudobulk_DE(_Adata(adata.X, uneven, adata.var_names), props, "alpha", covariates=["age"], **kw)


def test_adjusting_for_batch_removes_batch_driven_hits():
    """the purpose: a strong batch effect, the batch unbalanced across the two groups, NO group effect.  Without the covariate the
    batch shows up as a group difference; with it the statistics shrink"""
    rng = np.random.default_rng(2626)
    m, G = 16, 150
    group = np.repeat([0, 1], 8)
    batch = np.array([0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1])    # 2 of 8 against 6 of 8
    s = RR.size_factors(rng, m)
    base = np.exp(rng.uniform(np.log(20.0), np.log(2000.0), G))
    c = RR.nb_counts(rng, s[:, None] * base[None] * np.exp(rng.normal(0.0, 1.0, G)[None] * batch[:, None]), (0.05 + 2.0 / base)[None])
    samples = ["s%02d" % i for i in range(m)]
    counts = pd.DataFrame(c, index=samples, columns=["g%03d" % j for j in range(G)])
    meta = pd.DataFrame({"Predicted_Labels": np.array(["T1", "T2"])[group], "batch": np.array(["A", "B"])[batch]}, index=samples)
    plain = tl.compute_pseudobulk_DE(counts, meta, **ARGS)
    adjusted = tl.compute_pseudobulk_DE(counts, meta, covariates=["batch"], **ARGS)
    med_plain, med_adjusted = plain["stat"].abs().median(), adjusted["stat"].abs().median()
    print("median |stat|: %.3f without the covariate, %.3f with it; padj < 0.05: %d and %d"
          % (med_plain, med_adjusted, (plain["padj"] < 0.05).sum(), (adjusted["padj"] < 0.05).sum()))
    assert med_adjusted < med_plain
    assert (adjusted["padj"] < 0.05).sum() <= (plain["padj"] < 0.05).sum()
    batch_effect = adjusted.attrs["coefficients"]["batch_B"]
    assert batch_effect.abs().median() > 0.3                              # the covariate's coefficient carries the effect
