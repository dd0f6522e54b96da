"""Cook's outlier handling and independent filtering (K25), the parts that need no device.

The restatement (tests/nb_cooks_restatement.py) is pinned where something independent exists here: its trimmed mean to
scipy.stats.trim_mean, its cutoff to scipy.stats.f.ppf, its loop Benjamini-Hochberg to tl._bh_adjust, its design-matrix hat
diagonal to the closed form w_j / sum_group w.  lowess has NO independent implementation on this machine (statsmodels is not
installed and there is no R): engine.lowess and the loop restatement are checked against each other and by three properties -- a
straight line is reproduced to 1e-12, one gross outlier is ignored after the robustness iterations, and f = 1 with iters = 0 is
the weighted least-squares line with tricube weights computed here -- and that is all the pinning there is.
engine.independent_filtering equals the loop restatement exactly on seeded tables; engine.nb_replacements equals the loop;
tl.compute_pseudobulk_DE(outliers="deseq2") runs with the three device calls replaced by the restatements, against the host
tail written out here.  pilot_ot_nb_cooks refuses every bad argument before any HIP call; engine and tl raise before the library
is touched."""
import ctypes

import numpy as np
import pandas as pd
import pytest
from scipy import stats

import nb_cooks_restatement as CR
import nb_glm_restatement as RR
from pilot_amd import _lib, engine, tl


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())


# ---- pins for the restatement -------------------------------------------------------------------------------------------------------
def test_trimmed_mean_is_scipy_trim_mean():
    rng = np.random.default_rng(0)
    for n in range(1, 80):
        x = rng.gamma(2.0, 10.0, n)
        for r in (CR.Fraction(1, 3), CR.Fraction(1, 4), CR.Fraction(1, 8), CR.BASE_TRIM):
            drop = (n * r.numerator) // r.denominator
            want = stats.trim_mean(x, (drop + 0.5) / n)                 # (a proportion inside the step: no float product on its edge)
            assert abs(CR.tm(x, r) - want) <= 1e-14 * abs(want), (n, r)
            if int(float(r) * n) == drop:                               # and with the ratio itself wherever its float product agrees
                assert abs(CR.tm(x, r) - stats.trim_mean(x, float(r))) <= 1e-14 * abs(want), (n, r)
    assert CR.tm([5.0, 1.0, 100.0], CR.Fraction(1, 3)) == 5.0           # trim 1/3 of three keeps the median
    assert [CR.trim_rule(n)[1] for n in (1, 3, 4, 23, 24, 4096)] == [2.04, 2.04, 1.86, 1.86, 1.51, 1.51]


def test_cutoff_is_the_f_quantile():
    for m, p in ((10, 2), (16, 2), (14, 3), (4096, 2)):
        assert engine.nb_cooks_cutoff(m, p) == CR.cutoff(m, p) == float(stats.f.ppf(0.99, p, m - p))
    for m, p in ((2, 2), (5, 0), (5.5, 2), (True, 1)):
        with pytest.raises(ValueError):
            engine.nb_cooks_cutoff(m, p)


def test_loop_bh_is_tl_bh():
    rng = np.random.default_rng(1)
    for n in (1, 2, 17, 300):
        p = rng.random(n) ** 3
        p[rng.random(n) < 0.2] = p[0]                                   # ties
        np.testing.assert_array_equal(CR.bh(p), tl._bh_adjust(p))
        np.testing.assert_array_equal(engine.bh_adjust(p), tl._bh_adjust(p))


def test_hat_diagonal_is_the_weight_over_its_group_sum():
    rng = np.random.default_rng(2)
    codes = rng.permutation(np.repeat(np.arange(3), (3, 4, 7)))
    w = rng.gamma(2.0, 1.0, 14)
    want = w / np.bincount(codes, weights=w)[codes]
    np.testing.assert_allclose(CR.hat_diagonal(w, codes, 3), want, rtol=1e-12)


# ---- lowess ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", [engine.lowess, CR.lowess], ids=["engine", "loop"])
def test_lowess_properties(fit):
    x = np.linspace(0.1, 0.95, 50)
    line = 3.0 - 2.0 * x
    assert np.abs(fit(x, line, 0.2) - line).max() <= 1e-12
    assert np.abs(fit(x, line, 2.0 / 3.0, 0) - line).max() <= 1e-12
    # one gross outlier.  On an EXACT line the median residual is 0 and the iterations stop, as in R, so the line carries a little
    # noise (sd 0.01); and the span is 1/2: at 1/5 every neighbour in the outlier's ten-point window is pulled so far by the first
    # pass that all of them lose their weight with it, which is lowess's known behaviour, not a fault of either statement
    bumped = line + np.random.default_rng(6).normal(0.0, 0.01, x.size)
    bumped[20] += 500.0
    assert np.abs(fit(x, bumped, 0.5, 0) - line).max() > 10.0            # without the robustness iterations the outlier pulls
    assert np.abs(fit(x, bumped, 0.5, 3) - line).max() <= 0.05          # with them it has weight 0: the line, within the noise
    # f = 1, iters = 0: per point the weighted least-squares line with tricube weights over the whole range
    rng = np.random.default_rng(3)
    y = np.sin(4 * x) + rng.normal(0, 0.1, x.size)
    got = fit(x, y, 1.0, 0)
    for i in range(x.size):
        r = np.abs(x - x[i])
        h = r.max()
        w = np.where(r <= 0.999 * h, (1.0 - (r / h) ** 3) ** 3, 0.0)
        w[r <= 0.001 * h] = 1.0
        slope, intercept = np.polyfit(x, y, 1, w=np.sqrt(w))
        assert abs(got[i] - (intercept + slope * x[i])) <= 1e-10


def test_engine_lowess_is_the_loop():
    rng = np.random.default_rng(4)
    for n, f in ((50, 0.2), (50, 0.5), (7, 0.2), (2, 1.0)):
        x = np.sort(rng.random(n))
        y = np.rint(200 * np.exp(-3 * x) + rng.normal(0, 5, n))
        np.testing.assert_allclose(engine.lowess(x, y, f), CR.lowess(x, y, f), rtol=0, atol=1e-10)
    for bad in (dict(x=[0, 1], y=[1]), dict(x=[1, 0], y=[0, 1]), dict(x=[0, np.nan], y=[0, 1]), dict(x=[0, 1], y=[0, 1], f=0),
                dict(x=[0, 1], y=[0, 1], f=1.5), dict(x=[0, 1], y=[0, 1], iters=-1), dict(x=[0, 1], y=[0, 1], iters=1.5), dict(x=[0], y=[0])):
        with pytest.raises(ValueError):
            engine.lowess(**bad)


# ---- independent filtering ---------------------------------------------------------------------------------------------------------------
def _table(seed, G, n_true, zero_share=0.1):
    rng = np.random.default_rng(seed)
    mean = np.exp(rng.uniform(np.log(0.5), np.log(5000.0), G))
    p = rng.random(G)
    true = rng.choice(G, n_true, replace=False)
    p[true] = rng.random(n_true) ** 6 * np.minimum(1.0, 20.0 / mean[true])        # power grows with the mean
    mean[rng.random(G) < zero_share] = np.nan                          # genes of zeros: no mean, no p-value
    p[np.isnan(mean)] = np.nan
    p[rng.random(G) < 0.02] = np.nan                                   # and a few flagged ones with a mean
    return p, mean


@pytest.mark.parametrize("seed,G,n_true", [(0, 400, 80), (1, 1000, 150), (2, 300, 40), (3, 60, 30)])
def test_engine_filtering_is_the_loop(seed, G, n_true):
    p, mean = _table(seed, G, n_true)
    padj, info = engine.independent_filtering(p, mean, 0.05)
    want, winfo = CR.independent_filtering(p, mean, 0.05, fit_lowess=engine.lowess)
    np.testing.assert_array_equal(padj, want)
    np.testing.assert_array_equal(info["num_rej"], winfo["num_rej"])
    assert info["num_rej"].dtype.kind == "i" and isinstance(info["chosen"], int) and info["chosen"] == winfo["chosen"]
    assert info["filter_threshold"] == winfo["filter_threshold"]
    np.testing.assert_array_equal(info["theta"], winfo["theta"])
    assert info["num_rej"].max() > 10 and info["lowess"] is not None
    # with the loop's own lowess the choice is the same (the two fits agree far inside the gaps between the counts)
    assert CR.independent_filtering(p, mean, 0.05)[1]["chosen"] == info["chosen"]
    below = np.where(np.isnan(mean), 0.0, mean) < info["filter_threshold"]
    assert np.isnan(padj[below | np.isnan(p)]).all() and not np.isnan(padj[~below & ~np.isnan(p)]).any()


def test_filtering_returns_plain_bh_when_little_is_rejected():
    rng = np.random.default_rng(5)
    p, mean = rng.random(200), np.exp(rng.uniform(0, 8, 200))
    p[:4] = 1e-9
    padj, info = engine.independent_filtering(p, mean, 0.05)
    assert info["num_rej"].max() <= 10 and info["chosen"] == 0 and info["lowess"] is None and info["theta"][0] == 0.0
    np.testing.assert_array_equal(padj, tl._bh_adjust(p))
    # everything a gene of zeros: one column, theta = [0]
    padj, info = engine.independent_filtering(np.full(5, np.nan), np.full(5, np.nan), 0.05)
    assert info["theta"].tolist() == [0.0] and np.isnan(padj).all()
    for bad in (dict(pvalue=p, base_mean=mean[:5]), dict(pvalue=p, base_mean=mean, alpha=0.0), dict(pvalue=p, base_mean=mean, alpha=1.0),
                dict(pvalue=p, base_mean=mean, alpha="0.05"), dict(pvalue=p[:0], base_mean=mean[:0])):
        with pytest.raises(ValueError):
            engine.independent_filtering(**bad)


# ---- replacements and the tl tail on the restatement ---------------------------------------------------------------------------------------
def test_replacements_are_the_loop():
    C = CR.case(11, (3, 7), 27)
    W = C["want"]
    rows = engine.nb_replacements(C["c"], C["codes"], C["s"], W["D"], C["cutoff"], W["trimmed_base"], 7)
    want = CR.replacements(C["c"], C["codes"], C["s"], W["D"], C["cutoff"], W["trimmed_base"], 7)
    assert [tuple(r) for r in rows.tolist()] == want and len(want) >= 3
    assert (np.bincount(C["codes"])[C["codes"]][rows["sample"]] >= 7).all()
    np.testing.assert_array_equal(np.bincount(rows["gene"], minlength=C["G"]), W["n_replace"])
    for bad in (dict(D=W["D"][:, :5]), dict(trimmed_base=W["trimmed_base"][:5]), dict(cutoff=0.0), dict(min_replace=2),
                dict(codes=C["codes"][:5]), dict(size_factors=-C["s"])):
        a = dict(counts=C["c"], codes=C["codes"], size_factors=C["s"], D=W["D"], cutoff=C["cutoff"], trimmed_base=W["trimmed_base"], min_replace=7)
        a.update(bad)
        with pytest.raises(ValueError):
            engine.nb_replacements(**a)


def _fakes(monkeypatch):
    def dispersions(counts, codes, n_groups, size_factors, log_prior_mean=None, prior_var=None, return_info=False):
        return RR.dispersions(counts, codes, n_groups, size_factors, log_prior_mean, prior_var)[0]

    def group_fits(counts, codes, n_groups, size_factors, dispersion, return_info=False):
        q, w, flags = RR.group_fits(counts, codes, n_groups, size_factors, dispersion)
        return (q, w, {"flags": flags, "steps": np.zeros_like(flags), "n_not_converged": 0}) if return_info else (q, w)

    def cooks(counts, codes, n_groups, size_factors, dispersion, q, cutoff, min_replace=7, return_distances=False):
        out = CR.cooks(counts, codes, n_groups, size_factors, dispersion, q, cutoff, min_replace)
        out.pop("D_scale")
        if not return_distances:
            out.pop("D")
        return out
    monkeypatch.setattr(engine, "nb_dispersions", dispersions)
    monkeypatch.setattr(engine, "nb_group_fits", group_fits)
    monkeypatch.setattr(engine, "nb_cooks", cooks)


def planted_table(n0, n1, G=90, seed=31):
    """a `_pseudobulk`-style pair: n0 + n1 samples (T1, T2), G NB genes; g003 and g017 carry one count x 300 (in T2 and T1), g020 a
    planted 0 among counts around 1000, g025 a single non-zero count (in T2), g030 a count x 300 in T1 that stays below every
    count of T2 (a distance past the cutoff with three or more larger counts: not to be flagged); returns (counts, meta, planted
    {gene: [samples]})"""
    rng = np.random.default_rng(seed + n0)
    m = n0 + n1
    s = RR.size_factors(rng, m)
    codes = rng.permutation(np.repeat(np.arange(2), (n0, n1)))
    c = RR.nb_class(rng, s, codes, 2, G)
    samples = ["s%02d" % i for i in range(m)]
    first = lambda g, skip=0: int(np.flatnonzero(codes == g)[skip])
    c[:, 3] = np.rint(s * 80.0 * np.exp(rng.normal(0, 0.1, m)))
    c[:, 17] = np.rint(s * 40.0 * np.exp(rng.normal(0, 0.1, m)))
    c[first(1), 3] *= 300.0
    c[first(0, 1), 17] *= 300.0
    c[:, 20] = np.rint(s * 1000.0 * np.exp(rng.normal(0, 0.05, m)))
    c[first(1, 2), 20] = 0.0
    c[:, 25] = 0.0
    c[first(1, 1), 25] = 5000.0
    c[:, 30] = np.rint(s * np.where(codes == 1, 20000.0, 10.0) * np.exp(rng.normal(0, 0.1, m)))
    c[first(0, 2), 30] *= 300.0
    planted = {"g003": [samples[first(1)]], "g017": [samples[first(0, 1)]], "g025": [samples[first(1, 1)]]}
    counts = pd.DataFrame(c, index=samples, columns=["g%03d" % j for j in range(G)])
    labels = np.array(["T1", "T2"])[codes]
    meta = pd.DataFrame({"Predicted_Labels": labels, "stage": labels}, index=samples)
    return counts, meta, planted


def outliers_by_hand(counts, meta, plain, independent_filtering=False, alpha=0.05):
    """tl.compute_pseudobulk_DE(outliers="deseq2") from the engine calls and the host tail written out;
    plain: the frame without outlier handling, whose attrs carry the first fit's table.  Returns (frame, replaced rows)"""
    codes = (meta["Predicted_Labels"] == "T2").to_numpy().astype(np.int32)
    c = np.ascontiguousarray(counts.to_numpy(dtype=np.float64))
    m, G = c.shape
    sf = plain.attrs["size_factors"].to_numpy()
    table = plain.attrs["dispersions"]
    disp, base = table["dispersion"].to_numpy().copy(), table["baseMean"].to_numpy().copy()
    cut = float(stats.f.ppf(0.99, 2, m - 2))
    q, w = engine.nb_group_fits(c, codes, 2, sf, disp)
    q, w = q.copy(), w.copy()
    first = engine.nb_cooks(c, codes, 2, sf, disp, q, cut)
    max_cooks, n_above = first["max_cooks"].copy(), first["n_above"].copy()
    rep = np.flatnonzero(first["n_replace"] > 0)
    rows = []
    if rep.size:
        sub = np.ascontiguousarray(c[:, rep])
        second = engine.nb_cooks(sub, codes, 2, sf, disp[rep], q[rep], cut, return_distances=True)
        rows = CR.replacements(sub, codes, sf, second["D"], cut, second["trimmed_base"])
        new = sub.copy()
        for j, i, _, value in rows:
            new[i, j] = value
        x = engine.nb_dispersions(new, codes, 2, sf)
        nbase = np.where(np.isnan(x), np.nan, (new / sf[:, None]).mean(axis=0))
        a0, a1 = table.attrs["trend"]["coefficients"]
        with np.errstate(divide="ignore", invalid="ignore"):
            log_fit = np.log(a0 + a1 / nbase)
        x_map = engine.nb_dispersions(new, codes, 2, sf, log_prior_mean=log_fit, prior_var=table.attrs["prior_var"])
        clip = lambda d: np.clip(d, RR.MIN_DISP, RR.max_disp(m))
        ndisp = np.where(RR.outliers(x, log_fit, table.attrs["var_log_disp"]), clip(np.exp(x)), clip(np.exp(x_map)))
        q[rep], w[rep] = engine.nb_group_fits(new, codes, 2, sf, ndisp)
        disp[rep], base[rep] = ndisp, nbase
        live = ~np.isnan(ndisp)
        max_cooks[rep], n_above[rep] = np.nan, 0
        if live.any():
            third = engine.nb_cooks(np.ascontiguousarray(new[:, live]), codes, 2, sf, ndisp[live], q[rep][live], cut, return_distances=True)
            max_cooks[rep[live]], n_above[rep[live]] = CR.refit_max_cooks(new[:, live], codes, third["D"])
        rows = [(counts.columns[rep[j]], counts.index[i], was, value) for j, i, was, value in rows]
    lfc, se, stat, p = RR.wald(q, w)
    with np.errstate(invalid="ignore"):
        flagged = (max_cooks > cut) & (n_above < 3)
    p[flagged] = np.nan
    if independent_filtering:
        padj = CR.independent_filtering(p, base, alpha, fit_lowess=engine.lowess)[0]
    else:
        padj = np.full(G, np.nan)
        padj[~np.isnan(p)] = CR.bh(p[~np.isnan(p)])
    replace = np.zeros(G, dtype=bool)
    replace[rep] = True
    frame = pd.DataFrame({"gene": np.asarray(counts.columns), "baseMean": base, "log2FoldChange": lfc, "lfcSE": se, "stat": stat, "pvalue": p,
                          "padj": padj, "dispersion": disp, "maxCooks": max_cooks, "cooksOutlier": flagged, "replace": replace})
    return frame.iloc[np.argsort(padj, kind="stable")].reset_index(drop=True), rows


def check_planted(out, plain, planted, replaceable):
    """what the issue asks of the planted genes, for 5 + 5 (nothing replaceable) and 8 + 8 (everything replaceable)"""
    at = out.set_index("gene")
    was = plain.set_index("gene")
    assert not at.loc["g020", "cooksOutlier"] and not at.loc["g030", "cooksOutlier"]
    replaced = out.attrs["replaced"]
    assert list(replaced.columns) == ["gene", "sample", "count", "replacement"]
    if not replaceable:
        for g in planted:
            assert at.loc[g, "cooksOutlier"] and np.isnan(at.loc[g, "pvalue"]) and np.isnan(at.loc[g, "padj"]) and not at.loc[g, "replace"]
        assert len(replaced) == 0 and not at["replace"].any()
        assert at.loc["g030", "maxCooks"] > out.attrs["cooks_cutoff"]     # a distance past the cutoff under three or more larger counts
        keep = ~at["cooksOutlier"].to_numpy()
        np.testing.assert_array_equal(at["pvalue"].to_numpy()[keep], was.loc[at.index, "pvalue"].to_numpy()[keep])
        assert at["cooksOutlier"].sum() <= len(planted) + 3
    else:
        for g, samples in planted.items():
            assert at.loc[g, "replace"] and not at.loc[g, "cooksOutlier"]
            assert replaced.loc[replaced["gene"] == g, "sample"].tolist() == samples
        assert np.isnan(at.loc[list(planted), "maxCooks"]).all()       # every group replaceable: nothing left to flag
        for g in ("g003", "g017"):
            assert abs(at.loc[g, "log2FoldChange"]) < abs(was.loc[g, "log2FoldChange"])
        assert at.loc["g025", ["baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "padj", "dispersion"]].isna().all()
        assert set(replaced["gene"]) >= set(planted) and len(set(replaced["gene"])) <= len(planted) + 4    # (g020, g030, chance)
        assert (replaced["replacement"] == np.trunc(replaced["replacement"])).all()


@pytest.mark.parametrize("n0,n1", [(5, 5), (8, 8)])
def test_tl_outliers_on_the_restatement(monkeypatch, n0, n1):
    _fakes(monkeypatch)
    counts, meta, planted = planted_table(n0, n1, G=60)
    args = dict(group1="T1", group2="T2", cluster_col="Predicted_Labels")
    plain = tl.compute_pseudobulk_DE(counts, meta, **args)
    assert list(plain.columns) == ["gene", "baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "padj", "dispersion"]
    assert not {"cooks_cutoff", "replaced", "independent_filtering"} & set(plain.attrs)
    pd.testing.assert_frame_equal(tl.compute_pseudobulk_DE(counts, meta, outliers=None, independent_filtering=False, alpha=0.3, **args), plain,
                                  check_exact=True)
    out = tl.compute_pseudobulk_DE(counts, meta, outliers="deseq2", **args)
    assert list(out.columns) == list(plain.columns) + ["maxCooks", "cooksOutlier", "replace"]
    assert out.attrs["cooks_cutoff"] == CR.cutoff(n0 + n1, 2)
    want, rows = outliers_by_hand(counts, meta, plain)
    pd.testing.assert_frame_equal(out, want, check_exact=True)
    assert [tuple(r) for r in out.attrs["replaced"].itertuples(index=False)] == rows
    check_planted(out, plain, planted, replaceable=n0 >= 7)
    both = tl.compute_pseudobulk_DE(counts, meta, outliers="deseq2", independent_filtering=True, alpha=0.1, **args)
    pd.testing.assert_frame_equal(both, outliers_by_hand(counts, meta, plain, True, 0.1)[0], check_exact=True)
    assert both.attrs["independent_filtering"]["theta"].size in (1, 50)
    # filtering alone, and on a frame already made
    alone = tl.compute_pseudobulk_DE(counts, meta, independent_filtering=True, **args)
    assert list(alone.columns) == list(plain.columns)
    later = tl.independent_filtering(plain, 0.05)
    pd.testing.assert_frame_equal(later, alone, check_exact=True)
    assert later.attrs["independent_filtering"]["chosen"] == alone.attrs["independent_filtering"]["chosen"]
    np.testing.assert_array_equal(alone.set_index("gene").loc[plain["gene"], "pvalue"].to_numpy(), plain["pvalue"].to_numpy())
    # the per-gene table of the refitted state
    codes = (meta["Predicted_Labels"] == "T2").to_numpy()
    per_gene = tl.deseq2_cooks(counts, codes, out)
    assert list(per_gene.index) == list(counts.columns) and per_gene.attrs["cooks_cutoff"] == out.attrs["cooks_cutoff"]
    if n0 < 7:
        assert (per_gene["n_replace"] == 0).all()
        np.testing.assert_array_equal(per_gene["max_cooks"].to_numpy(), out.set_index("gene").loc[counts.columns, "maxCooks"].to_numpy())


def frozen_fit_is_the_identity(counts, meta, monkeypatch):
    """the property that lets the refit be the first fit's own function: fitted again on the SAME counts with the trend and the
    two prior widths of the first table frozen, every column of the table, q, w and the flags come back bit for bit -- and neither
    the trend nor the prior variance is estimated on the way.  (Also run on the device: tests/test_gpu_nb_cooks.py.)"""
    codes = (meta["Predicted_Labels"] == "T2").to_numpy().astype(np.int32)
    counts = counts.copy()
    counts[["g040", "g041"]] = 0                                        # (the planted table has no gene of zeros: two all-NaN rows)
    c, genes = tl._nb_counts(counts, "frozen_fit")
    sf = tl.deseq2_size_factors(counts).to_numpy()
    first = tl._nb_fit(c, genes, codes, sf, "parametric")
    assert first.table.loc[["g040", "g041"]].drop(columns="dispOutlier").isna().all(axis=None) and np.isnan(first.q[[40, 41]]).all()
    assert first.table["dispersion"].notna().sum() == 58 and first.table["dispOutlier"].any()    # both kinds of final value

    def estimated(*a, **k):
        raise AssertionError("the frozen fit estimated its trend or its prior variance")
    monkeypatch.setattr(engine, "nb_trend", estimated)
    monkeypatch.setattr(engine, "nb_prior_var", estimated)
    again = tl._nb_fit(c, genes, codes, sf, None, frozen=first.table.attrs)
    pd.testing.assert_frame_equal(again.table, first.table, check_exact=True)
    assert list(again.table.dtypes) == list(first.table.dtypes)
    for name in ("q", "w", "flags"):
        np.testing.assert_array_equal(getattr(again, name), getattr(first, name))
    assert again.table.attrs["trend"] is first.table.attrs["trend"]
    assert (again.table.attrs["prior_var"], again.table.attrs["var_log_disp"]) == (first.table.attrs["prior_var"], first.table.attrs["var_log_disp"])
    # and written over its own rows, at any positions, it changes nothing
    rep = np.array([1, 25, 40])
    sub = tl._NBFit(first.table.iloc[rep], first.q[rep], first.w[rep], first.flags[rep])
    patched = first.with_rows(rep, sub)
    pd.testing.assert_frame_equal(patched.table, first.table, check_exact=True)
    assert patched.table is not first.table and patched.q is not first.q and np.array_equal(patched.q, first.q, equal_nan=True)


def test_a_frozen_fit_of_the_same_counts_is_the_first_fit(monkeypatch):
    _fakes(monkeypatch)
    counts, meta, _ = planted_table(8, 8, G=60)
    frozen_fit_is_the_identity(counts, meta, monkeypatch)


@pytest.mark.parametrize("n0,n1", [(5, 5), (8, 8)])
def test_outliers_make_no_device_call_they_did_not_make_before(monkeypatch, n0, n1):
    """the device calls of compute_pseudobulk_DE(outliers="deseq2"), in order, with the number of genes each is given: the first
    fit, the distances, and -- where a gene has a replacement -- the distances of those r genes, their refit, and the distances of
    the l of them that still have a dispersion"""
    _fakes(monkeypatch)
    calls = []

    def recording(name, fake):
        def call(counts, *a, **kw):
            calls.append((name, np.shape(counts)[1]) + ((kw.get("return_distances", False),) if name == "nb_cooks" else ()))
            return fake(counts, *a, **kw)
        return call
    for name in ("nb_dispersions", "nb_group_fits", "nb_cooks"):
        monkeypatch.setattr(engine, name, recording(name, getattr(engine, name)))
    counts, meta, _ = planted_table(n0, n1, G=60)
    out = tl.compute_pseudobulk_DE(counts, meta, group1="T1", group2="T2", cluster_col="Predicted_Labels", outliers="deseq2")
    G = 60
    want = [("nb_dispersions", G), ("nb_dispersions", G), ("nb_group_fits", G), ("nb_cooks", G, False)]
    r = int(out["replace"].sum())
    live = int((out["replace"] & out["dispersion"].notna()).sum())
    if n0 < 7:
        assert r == 0
    else:
        assert 1 <= live < r                                            # (g025 is emptied by its replacement)
        want += [("nb_cooks", r, True), ("nb_dispersions", r), ("nb_dispersions", r), ("nb_group_fits", r), ("nb_cooks", live, True)]
    assert calls == want


# ---- the C entry point --------------------------------------------------------------------------------------------------------------------
GOOD = dict(y=True, dtype=1, m=6, genes=5, ld=5, codes=[0, 1, 0, 1, 1, 0], ng=2, sf=[1.0, 0.5, 2.0, 1.0, 1.5, 0.7], disp=[0.1] * 5,
            q=[[1.0, 2.0]] * 5, cutoff=3.0, min_replace=7, out=True, D=False, ld_D=5)


def _call(**kw):
    a = dict(GOOD)
    a.update(kw)
    L = _lib.load()
    Y = np.ones((6, 8), dtype=np.float64)
    arr = lambda v, t: None if v is None else np.ascontiguousarray(v, dtype=t)
    codes, sf, disp, q = arr(a["codes"], np.int32), arr(a["sf"], np.float64), arr(a["disp"], np.float64), arr(a["q"], np.float64)
    ptr = lambda v, f: None if v is None else f(v)
    d = [np.zeros(64) for _ in range(3)]
    i = [np.zeros(64, dtype=np.int32) for _ in range(3)]
    Dbuf = np.zeros(64)
    bad_row, bad_col = ctypes.c_longlong(5), ctypes.c_int(5)
    rc = L.pilot_ot_nb_cooks(ctypes.c_void_p(Y.ctypes.data) if a["y"] else None, 0, a["dtype"], a["m"], a["genes"], a["ld"], ptr(codes, _lib.iptr),
                             a["ng"], ptr(sf, _lib.dptr), ptr(disp, _lib.dptr), ptr(q, _lib.dptr), a["cutoff"], a["min_replace"],
                             _lib.dptr(d[0]) if a["out"] else None, _lib.dptr(d[1]), _lib.iptr(i[0]), _lib.iptr(i[1]), _lib.iptr(i[2]),
                             _lib.dptr(d[2]), ctypes.c_void_p(Dbuf.ctypes.data) if a["D"] else None, 0, a["ld_D"], ctypes.byref(bad_row),
                             ctypes.byref(bad_col))
    assert bad_row.value == -1 and bad_col.value == -1
    return rc, L.pilot_ot_last_error()


@pytest.mark.parametrize("bad,fragment", [
    (dict(y=False), b"NULL"), (dict(codes=None), b"NULL"), (dict(sf=None), b"NULL"), (dict(out=False), b"NULL"), (dict(disp=None), b"NULL"),
    (dict(q=None), b"NULL"),
    (dict(genes=0, ld=0), b"n_genes=0"), (dict(ld=4), b"ld=4"), (dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"),
    (dict(m=1), b"m=1"), (dict(m=0), b"m=0"),
    (dict(ng=1), b"n_groups=1"), (dict(ng=6, codes=[0, 1, 2, 3, 4, 5]), b"n_groups=6"), (dict(ng=0), b"n_groups=0"),
    (dict(ng=3, q=[[1.0, 2.0, 3.0]] * 5), b"group 2 has no sample"), (dict(codes=[1, 1, 1, 1, 1, 1]), b"group 0 has no sample"),
    (dict(codes=[0, 1, 2, 1, 1, 0]), b"codes[2]=2"), (dict(codes=[0, -1, 0, 1, 1, 0]), b"codes[1]=-1"),
    (dict(sf=[1.0, 0.0, 2.0, 1.0, 1.5, 0.7]), b"size_factors[1]"), (dict(sf=[1.0, 0.5, -2.0, 1.0, 1.5, 0.7]), b"size_factors[2]"),
    (dict(sf=[1.0, 0.5, 2.0, np.nan, 1.5, 0.7]), b"size_factors[3]"), (dict(sf=[1.0, 0.5, 2.0, 1.0, np.inf, 0.7]), b"size_factors[4]"),
    (dict(disp=[0.1, 0.1, 9e-9, 0.1, 0.1]), b"dispersion[2]"), (dict(disp=[10.5] + [0.1] * 4), b"dispersion[0]"),
    (dict(disp=[0.1, np.inf, 0.1, 0.1, 0.1]), b"dispersion[1]"), (dict(disp=[0.1, 0.1, 0.1, -1.0, 0.1]), b"dispersion[3]"),
    (dict(cutoff=0.0), b"cutoff"), (dict(cutoff=-1.0), b"cutoff"), (dict(cutoff=np.nan), b"cutoff"), (dict(cutoff=np.inf), b"cutoff"),
    (dict(min_replace=2), b"min_replace=2"), (dict(min_replace=0), b"min_replace=0"), (dict(min_replace=-7), b"min_replace=-7"),
    (dict(D=True, ld_D=4), b"ld_D=4"),
    (dict(q=[[1.0, 2.0]] * 3 + [[1.0, 0.0]] + [[1.0, 2.0]]), b"q[3, 1]"), (dict(q=[[-1.0, 2.0]] + [[1.0, 2.0]] * 4), b"q[0, 0]"),
    (dict(q=[[1.0, 2.0]] * 4 + [[np.nan, 2.0]]), b"q[4, 0]"), (dict(q=[[1.0, np.inf]] + [[1.0, 2.0]] * 4), b"q[0, 1]"),
])
def test_entry_point_refuses_before_any_hip_call(bad, fragment):
    rc, msg = _call(**bad)
    assert rc == _lib.EINVAL and fragment in msg, (bad, msg)


def test_too_many_samples_are_refused_before_any_hip_call():
    L = _lib.load()
    limit = L.pilot_ot_nb_glm_max_samples()
    assert limit >= 4096 and 8 * (2 * 4096 + 4096) <= 96 * 1024          # counts, normalised counts and the sort buffer at 4096
    rc, msg = _call(m=limit + 1, codes=[0, 1] * ((limit + 1) // 2) + [0], sf=[1.0] * (limit + 1), genes=1, ld=1, disp=[0.1], q=[[1.0, 2.0]])
    assert rc == _lib.ENOTSUP and b"staged in LDS" in msg
    m = limit + 1
    with pytest.raises(NotImplementedError, match="samples"):
        engine.nb_cooks(np.ones((m, 1)), np.arange(m) % 2, 2, np.ones(m), np.full(1, 0.1), np.ones((1, 2)), 3.0)


def test_good_arguments_get_as_far_as_the_device():
    want = _lib.OK if _lib.device_count() > 0 else _lib.EHIP
    for kw in (dict(), dict(ld=8), dict(dtype=0), dict(D=True), dict(D=True, ld_D=7), dict(min_replace=3), dict(ld_D=0),
               dict(disp=[1e-8, 10.0, np.nan, 0.1, 0.1], q=[[1.0, 2.0]] * 2 + [[np.nan, -1.0]] + [[1.0, 2.0]] * 2),
               dict(ng=5, codes=[0, 1, 2, 3, 4, 4], q=[[1.0] * 5] * 5)):
        rc, msg = _call(**kw)
        assert rc == want, (kw, msg)


def test_symbols():
    assert "pilot_ot_nb_cooks" in _lib.SYMBOLS and hasattr(_lib.load(), "pilot_ot_nb_cooks")
    assert (engine.NB_COOKS_MIN_REPLACE, engine.NB_COOKS_MIN_GROUP) == (CR.MIN_REPLACE, CR.MIN_GROUP) == (7, 3)
    assert not [n for n in engine.ws_slot_names() if n.startswith("WS_NB_")
                and n not in ("WS_NB_Y", "WS_NB_INT", "WS_NB_SF", "WS_NB_BAD", "WS_NB_PRIOR", "WS_NB_OUT", "WS_NB_FIT_INT")]


# ---- engine and tl refuse on the host -------------------------------------------------------------------------------------------------------
Y6 = np.ones((6, 5))
C6, S6 = np.array([0, 1, 0, 1, 1, 0]), np.array([1.0, 0.5, 2.0, 1.0, 1.5, 0.7])


@pytest.mark.parametrize("kw", [
    dict(counts=np.ones(6)), dict(counts=np.ones((6, 5), dtype=np.int64)), dict(counts=np.ones((6, 8))[:, :5]),
    dict(n_groups=1), dict(n_groups=6), dict(n_groups=2.5), dict(n_groups=True), dict(n_groups=3),
    dict(codes=C6[:5]), dict(codes=C6.astype(float)), dict(codes=[0, 1, 0, 1, 2, 0]), dict(codes=[0, -1, 0, 1, 1, 0]), dict(codes=[1] * 6),
    dict(size_factors=S6[:5]), dict(size_factors=[1.0, 0.0, 2.0, 1.0, 1.5, 0.7]), dict(size_factors=-S6),
    dict(dispersion=np.full(4, 0.1)), dict(dispersion=[0.1, 0.1, 9e-9, 0.1, 0.1]), dict(dispersion=[0.1, np.inf, 0.1, 0.1, 0.1]),
    dict(q=np.ones((5, 3))), dict(q=np.ones(5)), dict(q=np.zeros((5, 2))), dict(q=-np.ones((5, 2))), dict(q=np.full((5, 2), np.nan)),
    dict(q=np.full((5, 2), np.inf)),
    dict(cutoff=0.0), dict(cutoff=-2.0), dict(cutoff=np.nan), dict(cutoff=np.inf), dict(cutoff="3"), dict(cutoff=None), dict(cutoff=True),
    dict(min_replace=2), dict(min_replace=0), dict(min_replace=7.5), dict(min_replace=True),
    dict(return_distances="host"), dict(return_distances=2),
])
def test_engine_refuses_before_the_library(no_library, kw):
    a = dict(counts=Y6, codes=C6, n_groups=2, size_factors=S6, dispersion=np.full(5, 0.1), q=np.ones((5, 2)), cutoff=3.0)
    a.update(kw)
    with pytest.raises(ValueError):
        engine.nb_cooks(**a)


def test_a_nan_dispersion_excuses_its_q(no_library):
    disp, q = np.array([0.1, np.nan, 0.1, 0.1, 0.1]), np.ones((5, 2))
    q[1] = np.nan
    with pytest.raises(AssertionError, match="the library was touched"):   # every check passed
        engine.nb_cooks(Y6, C6, 2, S6, disp, q, 3.0)


def test_tl_refuses_before_the_library(no_library):
    counts = pd.DataFrame(np.arange(1.0, 31.0).reshape(6, 5), index=list("abcdef"), columns=["g%d" % j for j in range(5)])
    meta = pd.DataFrame({"Predicted_Labels": ["T1", "T2", "T1", "T3", "T2", "T1"]}, index=list("abcdef"))
    args = dict(group1="T1", group2="T2", cluster_col="Predicted_Labels")
    for kw in (dict(outliers="cooks"), dict(outliers=True), dict(outliers="DESeq2"), dict(outliers=7), dict(alpha=0.0), dict(alpha=1.0),
               dict(alpha=-0.1), dict(alpha=np.nan), dict(alpha="0.05"), dict(alpha=None), dict(independent_filtering="yes"),
               dict(independent_filtering=1), dict(outliers="deseq2", alpha=2.0)):
        with pytest.raises(ValueError):
            tl.compute_pseudobulk_DE(counts, meta, **args, **kw)
        with pytest.raises(ValueError):
            tl.get_pseudobulk_DE(None, None, "alpha", **kw)
    frame = pd.DataFrame({"gene": counts.columns, "baseMean": 1.0, "pvalue": 0.5, "padj": 0.5, "dispersion": 0.1})
    frame.attrs["size_factors"] = pd.Series(np.ones(6), index=counts.index)
    for bad in (dict(de=frame.drop(columns="pvalue")), dict(de=None), dict(alpha=0.0), dict(alpha=1.5), dict(alpha="x")):
        a = dict(de=frame, alpha=0.05)
        a.update(bad)
        with pytest.raises(ValueError):
            tl.independent_filtering(**a)


def _intake_inputs():
    counts = pd.DataFrame(np.arange(1.0, 31.0).reshape(6, 5), index=list("abcdef"), columns=["g%d" % j for j in range(5)])
    frame = pd.DataFrame({"gene": counts.columns, "baseMean": 1.0, "log2FoldChange": np.linspace(-1, 1, 5), "lfcSE": 0.3, "stat": 0.0,
                          "pvalue": 0.5, "padj": 0.5, "dispersion": [0.1, 0.2, 0.3, 0.4, 0.5]})
    frame.attrs.update(size_factors=pd.Series(np.ones(6), index=counts.index), floored=pd.Series(np.zeros(5, dtype=bool), index=counts.columns))
    return counts, np.array([0, 1, 0, 1, 1, 0]), frame


def _with(frame, **attrs):
    out = frame.copy()
    out.attrs.update(attrs)
    return out


def _renamed(frame, names):
    out = frame.copy()
    out["gene"] = names
    return out


@pytest.mark.parametrize("who", ["lfc_shrink", "deseq2_cooks"])
def test_both_readers_of_a_de_frame_refuse_it_the_same_way(no_library, who):
    """what tl.lfc_shrink and tl.deseq2_cooks check of (cluster_counts, groups, de) alike: each refusal in the caller's own name,
    before the library is touched.  (The cases deseq2_cooks had in test_tl_refuses_before_the_library live here; what only
    lfc_shrink refuses is in tests/test_nb_shrink_args.py.)"""
    counts, codes, frame = _intake_inputs()
    fn = getattr(tl, who)
    bare = frame.copy()
    bare.attrs = {}
    replaced = lambda **kw: pd.DataFrame({**dict(gene=["g1"], sample=["c"], count=[12.0], replacement=[3.0]), **kw})
    bad = [
        (dict(groups=codes[:5]), "groups has shape"), (dict(groups=codes + 1), "groups must be 0 / 1 or boolean"),
        (dict(groups=codes.astype(float)), "groups must be 0 / 1 or boolean"),
        (dict(de=frame.drop(columns="dispersion")), "de must be a frame of compute_pseudobulk_DE"),
        (dict(de=None), "de must be a frame of compute_pseudobulk_DE"),
        (dict(de=bare), "de.attrs lacks 'size_factors'" if who == "lfc_shrink" else "de must be a frame of compute_pseudobulk_DE"),
        (dict(de=frame.iloc[:4]), "the genes of de are not the columns"),
        (dict(de=_renamed(frame, ["g0", "g1", "g2", "g3", "g9"])), "the genes of de are not the columns"),
        (dict(de=_renamed(frame, ["g0", "g1", "g2", "g3", "g3"])), "the genes of de are not the columns"),
        (dict(cluster_counts=counts.rename(columns={"g4": "g3"})), "the genes of de are not the columns"),
        (dict(de=_with(frame, replaced=replaced(sample=["z"]))), "names a gene or a sample"),
        (dict(de=_with(frame, replaced=replaced(gene=["g7"]))), "names a gene or a sample"),
        (dict(de=_with(frame, replaced=replaced(count=[13.0]))), "records other counts"),
    ]
    for change, text in bad:
        with pytest.raises(ValueError) as err:
            fn(**{**dict(cluster_counts=counts, groups=codes, de=frame), **change})
        assert str(err.value).startswith(who + ": ") and text in str(err.value), (change, str(err.value))
    with pytest.raises(ValueError, match="size_factors has shape"):
        fn(counts, codes, _with(frame, size_factors=np.ones(5)))
    if who == "deseq2_cooks":
        with pytest.raises(ValueError, match="min_replace=2"):
            fn(counts, codes, frame, min_replace=2)
        with pytest.raises(ValueError, match="a samples x genes frame"):     # the table is looked at before min_replace
            fn(np.ones(6), codes, frame, min_replace=2)
    # a frame in another row order is no refusal (compute_pseudobulk_DE orders its rows by padj): every check passes, with the
    # recorded replacement too, and the dispersions are read in the table's order
    shuffled = _with(frame.iloc[[3, 0, 4, 2, 1]].reset_index(drop=True), replaced=replaced())
    with pytest.raises(AssertionError, match="the library was touched"):
        fn(counts, codes, shuffled)
    c, genes, samples, got_codes, sf, at, disp = tl._nb_de_intake(who, counts, codes, shuffled, ["gene", "dispersion"], ["size_factors"])
    assert disp.tolist() == [0.1, 0.2, 0.3, 0.4, 0.5] and shuffled["gene"].to_numpy()[at].tolist() == list(counts.columns)
    assert c[2, 1] == 3.0 and c.sum() == counts.to_numpy().sum() - 9.0 and got_codes.dtype == np.int32 and sf.dtype == np.float64
    assert list(genes) == list(counts.columns) and list(samples) == list(counts.index)
