"""The restatement of the shrunken fold change (tests/nb_shrink_restatement.py) pinned to scipy on its own, and the host-side
argument errors of engine.nb_shrink, tl.lfc_shrink and shrink="other", which are raised before the library is touched.  No GPU."""
import functools

import numpy as np
import pandas as pd
import pytest
from scipy import optimize, stats

import nb_glm_restatement as RR
import nb_shrink_restatement as SR
from pilot_amd import engine, tl


@functools.lru_cache(maxsize=None)
def _genes(G=40, m=12, seed=5):
    """G small NB genes in two groups (7 + 5 of 12), their dispersions, K22 fits and far ends"""
    rng = np.random.default_rng(seed)
    s = RR.size_factors(rng, m)
    codes = rng.permutation(np.repeat(np.arange(2), (m - 5, 5))).astype(np.int32)
    c = RR.nb_class(rng, s, codes, 2, G)
    alpha = np.clip(0.05 + 2.0 / np.maximum((c / s[:, None]).mean(axis=0), 1.0), RR.MIN_DISP, RR.max_disp(m))
    q, w, flags = RR.group_fits(c, codes, 2, s, alpha)
    return c, codes, s, alpha, q, w, flags, SR.far_end(q, flags)


def test_P_is_the_scipy_log_posterior_up_to_constants():
    c, codes, s, alpha, *_ = _genes()
    rng = np.random.default_rng(1)
    S = 0.3
    b0, b1 = rng.normal(3.0, 2.0, (alpha.size, 5)), rng.normal(0.0, 1.0, (alpha.size, 5))
    mu = s[:, None, None] * np.exp(b0[None] + (codes == 1)[:, None, None] * b1[None])
    r = 1.0 / alpha[None, :, None]
    full = (stats.nbinom.logpmf(c[:, :, None], r, 1.0 / (1.0 + alpha[None, :, None] * mu)).sum(axis=0) + stats.norm.logpdf(b0, 0.0, 15.0)
            + stats.t.logpdf(b1 / S, 1))
    diff = full - SR.P(c, codes, s, alpha, b0, b1, S)
    # the difference is a constant of the gene: lgamma terms, log pi, log(15 sqrt(2 pi))
    assert np.abs(diff - diff[:, :1]).max() <= 1e-9 * np.abs(full).max()
    assert np.array_equal(SR.P(c, codes, s, alpha, b0[:, 0], b1[:, 0], S), SR.P(c, codes, s, alpha, b0, b1, S)[:, 0])


def test_the_inner_solve_is_the_root_of_the_score_and_the_maximum_over_b0():
    c, codes, s, alpha, *_ = _genes()
    b1 = np.linspace(-3.0, 3.0, alpha.size)
    p, b0 = SR.profile(c, codes, s, alpha, b1, 0.3)
    lo, hi = SR.bracket(c, codes, s, b1[:, None])
    assert (SR.score(c, codes, s, alpha, lo * np.ones_like(b0[:, None]), b1[:, None]) > 0).all()
    assert (SR.score(c, codes, s, alpha, hi, b1[:, None]) < 0).all()
    for d in (-1e-6, 1e-6):
        assert (SR.P(c, codes, s, alpha, b0 + d, b1, 0.3) < p).all()
    f = SR.score(c, codes, s, alpha, b0[:, None], b1[:, None])[:, 0]
    w0, w1 = SR.weights(c, codes, s, alpha, b0, b1)
    assert (np.abs(f) <= 1e-9 * (w0 + w1)).all()                        # |score| / |its slope|: the root to 1e-9


@pytest.mark.parametrize("S", [0.3, 0.05])
def test_no_local_optimiser_beats_the_search(S):
    """Nelder-Mead from 0, from the MLE and from three random points never ends above the restatement's maximum by more than B"""
    c, codes, s, alpha, q, _, _, far = _genes()
    found = SR.search(c, codes, s, alpha, far, S)
    assert not found["flags"].any()
    B = SR.bound(c, codes, s, alpha, found["b0"], found["b1"], S)
    rng = np.random.default_rng(2)
    mle = np.log(q[:, 1]) - np.log(q[:, 0])
    worst = -np.inf
    for j in range(alpha.size):
        cj, aj = c[:, j:j + 1], alpha[j:j + 1]
        fun = lambda x: -SR.P(cj, codes, s, aj, np.array([x[0]]), np.array([x[1]]), S)[0]
        starts = [(np.log(q[j, 0]), 0.0), (np.log(q[j, 0]), mle[j])] + [(np.log(q[j, 0]) + rng.normal(), rng.normal(0, 1.5)) for _ in range(3)]
        for x0 in starts:
            best = optimize.minimize(fun, x0, method="Nelder-Mead", options=dict(xatol=1e-8, fatol=1e-12, maxiter=2000))
            worst = max(worst, (-best.fun - found["p"][j]) / B[j])
            assert -best.fun <= found["p"][j] + B[j], (j, x0, -best.fun - found["p"][j], B[j])
    print("\nthe best local optimum exceeds the search's by at most %.3g B" % worst)
    assert (np.abs(found["b1"]) <= np.abs(mle) + 1e-9).all() and (found["b1"] * mle >= 0).all()      # between 0 and the MLE


def test_posterior_sd_is_the_finite_difference_hessian():
    c, codes, s, alpha, q, _, _, far = _genes()
    S = 0.3
    found = SR.search(c, codes, s, alpha, far, S)
    b0, b1 = found["b0"], found["b1"]
    sd = SR.posterior_sd(b1, found["w0"], found["w1"], S)
    h = 1e-3                                                            # (error: h^2 / 12 of a fourth derivative + 4 ulp |P| / h^2, about 1e-4 of H)
    f = lambda d0, d1: -SR.P(c, codes, s, alpha, b0 + d0, b1 + d1, S)
    h00 = (f(h, 0) - 2 * f(0, 0) + f(-h, 0)) / h ** 2
    h11 = (f(0, h) - 2 * f(0, 0) + f(0, -h)) / h ** 2
    h01 = (f(h, h) - f(h, -h) - f(-h, h) + f(-h, -h)) / (4 * h ** 2)
    det = h00 * h11 - h01 ** 2
    ok = np.isfinite(sd)
    assert ok.sum() >= 30 and (det[ok] > 0).all()
    np.testing.assert_allclose(sd[ok], np.sqrt(h00 / det)[ok], rtol=1e-3)
    np.testing.assert_array_equal(engine.nb_posterior_sd(b1, found["w0"], found["w1"], S), sd)
    assert np.isnan(SR.posterior_sd(np.array([3.0]), np.array([1e-3]), np.array([1e-3]), 0.1)).all()    # not log-concave there


def test_prior_scale_is_the_top_of_the_marginal_likelihood():
    rng = np.random.default_rng(3)
    V = rng.uniform(0.01, 0.5, 400)
    for true_A, want_S in ((0.25, None), (4.0, 1.0)):
        D = rng.normal(0.0, np.sqrt(V + true_A))
        S, A = SR.prior_scale(D, np.sqrt(V))
        grid = np.exp(np.linspace(np.log(1e-6), np.log(400.0), 20001))
        ll = (-0.5 * np.log(V[None] + grid[:, None]) - 0.5 * D[None] ** 2 / (V[None] + grid[:, None])).sum(axis=1)
        top = grid[np.argmax(ll)]
        assert abs(np.log(A / top)) <= 2 * np.log(grid[1] / grid[0])
        assert abs(A - true_A) < 0.5 * true_A and S == (want_S or np.sqrt(A))
        assert engine.nb_prior_scale(D, np.sqrt(V)) == (S, A)
    assert SR.prior_scale(np.zeros(5), np.ones(5)) == (np.sqrt(1e-6), 1e-6)
    assert SR.prior_scale(np.full(5, 100.0), np.ones(5)) == (1.0, 400.0)
    # the genes with a NaN and the ones masked out do not count
    D2, se2 = np.append(D, [np.nan, 50.0]), np.append(np.sqrt(V), [0.1, 0.1])
    use = np.append(np.ones(D.size + 1, dtype=bool), False)
    assert engine.nb_prior_scale(D2, se2, use=use) == (S, A) == SR.prior_scale(D2, se2, use)
    with pytest.raises(ValueError, match="usable"):
        engine.nb_prior_scale(np.array([0.3, np.nan]), np.array([0.1, 0.1]))


def test_a_constructed_pair_has_two_maxima_and_one_gene_in_each_basin():
    _, codes, s, *_ = _genes()
    S = 0.02
    pair, alpha, ok = SR.bimodal_pair(s, codes, S)
    assert ok
    q, _, flags = RR.group_fits(pair, codes, 2, s, alpha)
    assert not flags.any()
    far = SR.far_end(q, flags)
    assert SR.two_maxima(pair, codes, s, alpha, far, S).all()
    found = SR.search(pair, codes, s, alpha, far, S)
    mle = np.abs(np.log(q[:, 1]) - np.log(q[:, 0]))
    assert abs(found["b1"][0]) < S and abs(found["b1"][1]) > 0.5 * mle[1]
    # both basins exist in both genes: a dense scan finds a local maximum on each side of the valley
    t = np.arcsinh(np.abs(far) / S)[:, None] * np.arange(2000) / 1999.0
    p, _ = SR.profile(pair, codes, s, alpha, SR.beta1_of(far, S, t), S)
    for j in range(2):
        peaks = np.flatnonzero((p[j, 1:-1] > p[j, :-2]) & (p[j, 1:-1] >= p[j, 2:])) + 1
        if p[j, 0] > p[j, 1]:
            peaks = np.append(0, peaks)
        assert peaks.size >= 2
        assert abs(t[j, peaks[np.argmax(p[j, peaks])]] - found["t"][j]) <= 2 * t[j, 1]      # the search ends on the higher one
    # a search from the wrong basin's side alone would have missed it: the two tops differ by more than B
    B = SR.bound(pair, codes, s, alpha, found["b0"], found["b1"], S)
    assert (B < 1e-9).all()


def test_far_end_follows_the_group_fits():
    q = np.array([[2.0, 8.0], [8.0, 2.0], [1.0, 1.0], [0.25, 40.0]])
    flags = np.array([[0, 0], [0, 0], [0, 0], [RR.FLOORED, 0]], dtype=np.int32)
    want = np.array([np.log(4.0) + 1, -np.log(4.0) - 1, 1.0, 30.0])
    np.testing.assert_allclose(SR.far_end(q, flags), want, rtol=1e-15)
    lfc = np.append(np.log(q[:, 1]) - np.log(q[:, 0]), np.nan)
    np.testing.assert_array_equal(engine.nb_far_end(lfc, np.append((flags != 0).any(axis=1), False)), np.append(SR.far_end(q, flags), 1.0))


# ---- argument errors, all before the library is loaded ---------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(engine._lib, "load", refuse)


def test_nb_shrink_refuses_bad_arguments_on_the_host(no_library):
    c, codes, s, alpha, _, _, _, far = _genes()
    good = dict(counts=c, codes=codes, size_factors=s, dispersion=alpha, far_end=far, prior_scale=0.3)
    bad = [dict(prior_scale=0.0), dict(prior_scale=-1.0), dict(prior_scale=np.inf), dict(prior_scale=np.nan), dict(intercept_scale=0.0),
           dict(intercept_scale=np.nan), dict(far_end=np.where(np.arange(far.size) == 3, np.inf, far)),
           dict(far_end=np.where(np.arange(far.size) == 3, np.nan, far)), dict(far_end=far[:-1]), dict(dispersion=alpha[:-1]),
           dict(dispersion=np.where(np.arange(alpha.size) == 2, 0.0, alpha)), dict(dispersion=np.full(alpha.size, 13.0)),
           dict(codes=np.zeros(codes.size, dtype=np.int32)), dict(codes=np.ones(codes.size, dtype=np.int32)),
           dict(codes=np.where(np.arange(codes.size) == 0, 2, codes)), dict(codes=codes[:-1]), dict(codes=codes.astype(float)),
           dict(size_factors=np.where(np.arange(s.size) == 1, 0.0, s)), dict(size_factors=s[:-1]),
           dict(counts=c[:2], codes=np.array([0, 1]), size_factors=s[:2]), dict(counts=c.astype(np.int64)), dict(counts=c[:, :0])]
    for change in bad:
        with pytest.raises(ValueError):
            engine.nb_shrink(**{**good, **change})


def _frame(genes):
    n = len(genes)
    de = pd.DataFrame({"gene": genes, "baseMean": np.ones(n), "log2FoldChange": np.linspace(-1, 1, n), "lfcSE": np.full(n, 0.3),
                       "stat": np.zeros(n), "pvalue": np.ones(n), "padj": np.ones(n), "dispersion": np.full(n, 0.1)})
    de.attrs.update(size_factors=pd.Series(np.ones(4)), floored=pd.Series(np.zeros(n, dtype=bool), index=genes))
    return de


def test_lfc_shrink_refuses_bad_arguments_on_the_host(no_library):
    genes = ["a", "b", "c"]
    counts = pd.DataFrame(np.ones((4, 3)), columns=genes)
    groups = np.array([0, 0, 1, 1])
    de = _frame(genes)
    lacking = _frame(genes)
    del lacking.attrs["floored"]
    shrunk = _frame(genes)
    shrunk["lfcMLE"] = 0.0
    bad = [dict(groups=groups[:-1]), dict(groups=np.array([0, 0, 1, 2])), dict(groups=np.zeros(4, dtype=int)), dict(groups=np.ones(4, dtype=bool)),
           dict(groups=np.array([0.0, 0.0, 1.0, 1.0])), dict(groups=np.array(["a", "a", "b", "b"])), dict(de=de.drop(columns="dispersion")),
           dict(de=lacking), dict(de=shrunk), dict(de=_frame(["a", "b", "d"])), dict(de=_frame(["a", "b"])), dict(de=_frame(["a", "b", "b"])),
           dict(de=None), dict(prior_scale=0.0), dict(prior_scale=-0.1), dict(prior_scale=np.nan), dict(prior_scale="apeglm"),
           dict(cluster_counts=np.ones(4))]
    for change in bad:
        with pytest.raises(ValueError):
            tl.lfc_shrink(**{**dict(cluster_counts=counts, groups=groups, de=de, prior_scale=None), **change})


def test_an_unknown_shrink_is_refused_before_device_work(no_library):
    counts = pd.DataFrame(np.ones((4, 3)), columns=["a", "b", "c"], index=list("wxyz"))
    meta = pd.DataFrame({"stage": ["T1", "T1", "T2", "T2"]}, index=list("wxyz"))
    for shrink in ("other", "ashr", "normal", True, 1):
        with pytest.raises(ValueError, match="shrink"):
            tl.compute_pseudobulk_DE(counts, meta, group1="T1", group2="T2", cluster_col="stage", shrink=shrink)
        with pytest.raises(ValueError, match="shrink"):
            tl.get_pseudobulk_DE(None, None, "alpha", shrink=shrink)
