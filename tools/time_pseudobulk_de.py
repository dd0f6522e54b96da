#!/usr/bin/env python3
"""Time of the negative-binomial GLM kernels (K22: engine.nb_dispersions, engine.nb_group_fits) beside the vectorised numpy /
scipy restatement (tests/nb_glm_restatement.py) on the same host.

Table: genes x samples of the tests' NB generator (base mean log-uniform on [2, 3000], alpha = 0.05 + 2 / base, 20 % fold
changes), two groups of m / 2 samples, float32 in HBM (a DeviceMatrix), at --samples sizes (default 24 and 600) and --genes
(default 20 000).  Per size, after one warm-up call of each, the host clock around ``nb_dispersions`` (gene-wise, then with a
prior: the MAP pass) and around ``nb_group_fits`` -- each call ends in device-to-host copies of its results -- best of --reps.
``lgamma-free``: the same call on a table of the same shape whose counts are zero but for one sample a gene; there the kernel takes
its c = 0 path for all but one sample (log1p, one division and the running sums: everything it does except the two lgamma and the
log of a positive count), which prices the arithmetic around lgamma.  Host: the restatement on --host-genes of the genes (default
200), scaled by genes / host-genes and reported as such.  No DESeq2 timing exists where this library is built.
Writes OUT/rate.txt (--out, default profiles/pseudobulk_de/).

--shrink: instead, the shrunken fold change (K23: engine.nb_shrink) beside the dispersion pass on the same tables: both are one
wave per gene and six 64-point rounds over LDS-staged samples; nb_shrink replaces two lgamma a sample by an inner Newton loop of
divides.  The dispersions come from one MAP-less pass, the far ends from nb_group_fits, the prior scale from
engine.nb_prior_scale.  ``nb_dispersions`` and ``nb_shrink`` alternate in one loop, best of --reps each; the mean inner steps a
lane and round (from the call's ``steps``) go beside the times so that the ratio can be read.  Host: the vectorised restatement
(tests/nb_shrink_restatement.py) on --host-genes genes, scaled.  Writes OUT/shrink_rate.txt.

--rlog: instead, the regularised log transform (K24: engine.nb_rlog, on_device=True) beside the dispersion pass on the same tables:
both are one wave per gene over LDS-staged samples; the dispersion pass evaluates 6 x 64 x m likelihood terms with lgamma a gene,
nb_rlog about (iterations + halvings) x m terms in three passes, spread over the lanes.  The dispersions are the trend of one
blind pass (engine.nb_dispersions_blind, engine.nb_trend), the prior variance engine.nb_rlog_prior_var's.  ``nb_dispersions`` and
``nb_rlog`` alternate in one loop, best of --reps each; the mean iterations a gene go beside the times.  Host: the vectorised
restatement of the same iteration (tests/nb_rlog_restatement.py) on --host-genes genes, scaled.  Writes OUT/rlog_rate.txt.

--cooks: instead, the Cook's-distance pass (K25: engine.nb_cooks on the whole table, no distances returned) beside the dispersion
pass on the same tables: both are one wave per gene over LDS-staged samples; nb_cooks is one staged pass plus five bitonic sorts a
gene (all samples, and each group's values and squared deviations).  --outlier-share of the genes (default 2 %) get one count
x 200, so that the refit has something to do.  The dispersions come from one MAP-less pass, the fits from
nb_group_fits.  ``nb_dispersions`` and ``nb_cooks`` alternate in one loop, best of --reps each.  Then, once, what
``outliers="deseq2"`` adds for the genes with a replacement: the gathered call with distances, the replacements, two dispersion
passes, the group fits and the last distance call on those genes only, with the share of genes that took part.  Host: the
restatement (tests/nb_cooks_restatement.py) on --host-genes genes, scaled.  Writes OUT/cooks_rate.txt.

--design: instead, the GLM for a general design (K26: engine.nb_design_dispersions, engine.nb_design_fits) at --design-cols columns
(default 4: intercept, batch, scaled age, group; the tests' generator with planted coefficients) beside K22's pass for the group
column alone on the same table: both searches are one wave per gene and six 64-point rounds over LDS-staged samples;
nb_design_dispersions adds an inner Newton fit of p coefficients at every grid point (two passes over the samples a step, one for
the normal equations and one for the line search).  ``nb_dispersions`` and ``nb_design_dispersions`` alternate in one loop, and so
do ``nb_group_fits`` and ``nb_design_fits``, best of --reps each; the mean inner steps a lane and round go beside the ratio.  Host:
the vectorised restatement (tests/nb_design_restatement.py) on --host-genes genes, scaled.  Writes OUT/design_rate.txt.

--design-shrink: instead, the shrunken coefficient under a general design (K27: engine.nb_design_shrink) at --design-cols columns
beside K26's dispersion pass on the same table: both are one wave per gene and six 64-point rounds over LDS-staged samples with an
inner Newton fit at every grid point -- of p coefficients there, of p - 1 here, warm-started from the lane's own last point.  The
dispersions are one MAP-less pass, the maximum-likelihood coefficients nb_design_fits', the prior scale nb_prior_scale's.
``nb_design_dispersions`` and ``nb_design_shrink`` alternate in one loop, best of --reps each; the mean inner steps a lane and
round of both go beside the ratio.  Host: the restatement (tests/nb_design_shrink_restatement.py) on --host-genes genes, scaled.
Writes OUT/design_shrink_rate.txt.

--design-cooks: instead, the Cook's-distance pass under a general design (K28: engine.nb_design_cooks on the whole table, no
distances returned) at 4 columns beside K25's ``nb_cooks`` for the group column alone and beside ``nb_design_fits`` on the same
table: K28 is K25's staged pass and sorts plus one pass for the Gram matrix, a Cholesky inverse and the hat diagonals, with the rows
of X read from global memory.  Two designs a shape: (intercept, batch, scaled age, group), whose cells are single samples (two
sorts of all samples a gene), and (intercept, batch, centre, group), all indicators, whose eight cells are sorted one by one.
--outlier-share of the genes get one count x 200.  The three calls alternate in one loop, best of --reps each.  Host: the
restatement (tests/nb_design_cooks_restatement.py) on --host-genes genes, scaled.  Writes OUT/design_cooks_rate.txt."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pseudobulk_de"))
    ap.add_argument("--samples", type=int, nargs="+", default=[24, 600])
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--host-genes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shrink", action="store_true")
    ap.add_argument("--rlog", action="store_true")
    ap.add_argument("--cooks", action="store_true")
    ap.add_argument("--design", action="store_true")
    ap.add_argument("--design-shrink", action="store_true")
    ap.add_argument("--design-cooks", action="store_true")
    ap.add_argument("--design-cols", type=int, default=4, help="--design, --design-shrink: the columns of the design matrix")
    ap.add_argument("--outlier-share", type=float, default=0.02, help="--cooks: the share of genes that get one count x 200")
    a = ap.parse_args()
    if a.shrink + a.rlog + a.cooks + a.design + a.design_shrink + a.design_cooks > 1:
        ap.error("--shrink, --rlog, --cooks, --design, --design-shrink and --design-cooks are separate runs")
    import nb_glm_restatement as RR
    from pilot_amd import _lib, engine

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def best_of(fn):
        fn()
        best = np.inf
        for _ in range(a.reps):
            t = time.perf_counter()
            out = fn()
            best = min(best, time.perf_counter() - t)
        return best, out

    say("%s; %s; at most %d samples a gene" % (_lib.device_name(), time.strftime("%Y-%m-%d"), engine.nb_glm_limits()))
    for m in (a.samples if a.shrink else ()):
        import nb_shrink_restatement as SR
        rng = np.random.default_rng(m)
        s = RR.size_factors(rng, m)
        codes = (np.arange(m) % 2).astype(np.int32)
        c = RR.nb_class(rng, s, codes, 2, a.genes)
        D = engine.DeviceMatrix.upload(c.astype(np.float32))
        alpha = engine.nb_clip(np.exp(engine.nb_dispersions(D, codes, 2, s)), m)
        q, w, fit = engine.nb_group_fits(D, codes, 2, s, alpha, return_info=True)
        floored = ((fit["flags"] & _lib.NB_FLOORED) != 0).any(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            lfc, se = np.log(q[:, 1]) - np.log(q[:, 0]), np.sqrt(1.0 / w[:, 0] + 1.0 / w[:, 1])
        S, A = engine.nb_prior_scale(lfc, se, use=~floored)
        far = engine.nb_far_end(lfc, floored)
        engine.nb_dispersions(D, codes, 2, s)
        engine.nb_shrink(D, codes, s, alpha, far, S)
        t_disp = t_shrink = np.inf
        for _ in range(a.reps):                                         # the two calls alternate
            t0 = time.perf_counter()
            engine.nb_dispersions(D, codes, 2, s)
            t1 = time.perf_counter()
            b0, b1, info = engine.nb_shrink(D, codes, s, alpha, far, S, return_info=True)
            t2 = time.perf_counter()
            t_disp, t_shrink = min(t_disp, t1 - t0), min(t_shrink, t2 - t1)
        live = ~np.isnan(alpha)
        say("case %d genes x %d samples, float32 in HBM, 2 groups; prior scale %.4g (prior variance %.4g), %d floored genes"
            % (a.genes, m, S, A, floored.sum()))
        say("  nb_shrink %.2f ms, nb_dispersions (gene-wise) %.2f ms beside it: ratio %.2f; best of %d, alternating"
            % (1e3 * t_shrink, 1e3 * t_disp, t_shrink / t_disp, a.reps))
        say("  inner steps a lane and round: mean %.2f, largest gene mean %.2f; %d at bound, %d not converged"
            % (info["steps"][live].mean() / 384.0, info["steps"][live].max() / 384.0, info["n_at_bound"], info["n_not_converged"]))
        h = min(a.host_genes, a.genes)
        t0 = time.perf_counter()
        found = SR.search(c[:, :h], codes, s, alpha[:h], far[:h], S)
        t_host = time.perf_counter() - t0
        res = SR.resolved(c[:, :h], codes, s, alpha[:h], far[:h], S, found)
        say("  host restatement on %d genes: %.2f s; scaled by %d / %d: %.0f s; device against it on the resolved genes (%d): t off by "
            "at most %.2g" % (h, t_host, a.genes, h, t_host * a.genes / h, res.sum(),
                              np.abs(SR.t_of(b1[:h][res], S) - found["t"][res]).max(initial=0)))
        del D
    for m in (a.samples if a.rlog else ()):
        import nb_rlog_restatement as LR
        rng = np.random.default_rng(m)
        s = RR.size_factors(rng, m)
        codes = (np.arange(m) % 2).astype(np.int32)
        c = RR.nb_class(rng, s, codes, 2, a.genes)
        D = engine.DeviceMatrix.upload(c.astype(np.float32))
        x = engine.nb_dispersions_blind(D, s)
        mean = (c / s[:, None]).mean(axis=0)
        fit = engine.nb_clip(engine.nb_trend(mean, engine.nb_clip(np.exp(x), m))[0], m)
        pv = engine.nb_rlog_prior_var(c, s, mean, fit)
        engine.nb_dispersions(D, codes, 2, s)
        engine.nb_rlog(D, s, fit, pv, on_device=True)
        t_disp = t_rlog = np.inf
        for _ in range(a.reps):                                         # the two calls alternate
            t0 = time.perf_counter()
            engine.nb_dispersions(D, codes, 2, s)
            t1 = time.perf_counter()
            R, info = engine.nb_rlog(D, s, fit, pv, on_device=True, return_info=True)
            t2 = time.perf_counter()
            t_disp, t_rlog = min(t_disp, t1 - t0), min(t_rlog, t2 - t1)
        live = np.isfinite(info["intercept"])
        say("case %d genes x %d samples, float32 in HBM, result kept in HBM; prior variance %.4g" % (a.genes, m, pv))
        say("  nb_rlog %.2f ms, nb_dispersions (gene-wise, 2 groups) %.2f ms beside it: ratio %.2f; best of %d, alternating"
            % (1e3 * t_rlog, 1e3 * t_disp, t_rlog / t_disp, a.reps))
        say("  iterations a gene: mean %.2f, largest %d; %d not converged" % (info["steps"][live].mean(), info["steps"].max(), info["n_not_converged"]))
        h = min(a.host_genes, a.genes)
        t0 = time.perf_counter()
        ref = LR.arrowhead_rlog(c[:, :h], s, fit[:h], pv)
        t_host = time.perf_counter() - t0
        got = engine.download(R)[:, :h]
        say("  host restatement (vectorised numpy) on %d genes: %.1f ms; scaled by %d / %d: %.2f s; device against it: rlog off by at most "
            "%.2g" % (h, 1e3 * t_host, a.genes, h, t_host * a.genes / h, np.abs(got - ref["rlog"]).max()))
        del D, R
    for m in (a.samples if a.cooks else ()):
        import nb_cooks_restatement as CR
        rng = np.random.default_rng(m)
        s = RR.size_factors(rng, m)
        codes = (np.arange(m) % 2).astype(np.int32)
        c = RR.nb_class(rng, s, codes, 2, a.genes)
        planted = rng.choice(a.genes, int(round(a.outlier_share * a.genes)), replace=False)      # one count x 200 in each of these genes
        at = rng.integers(0, m, planted.size)
        c[at, planted] = np.maximum(c[at, planted], 5.0) * 200.0
        D = engine.DeviceMatrix.upload(c.astype(np.float32))
        x = engine.nb_dispersions(D, codes, 2, s)
        alpha = engine.nb_clip(np.exp(x), m)
        q, _ = engine.nb_group_fits(D, codes, 2, s, alpha)
        cut = engine.nb_cooks_cutoff(m, 2)
        engine.nb_cooks(D, codes, 2, s, alpha, q, cut)
        t_disp = t_cooks = np.inf
        for _ in range(a.reps):                                         # the two calls alternate
            t0 = time.perf_counter()
            engine.nb_dispersions(D, codes, 2, s)
            t1 = time.perf_counter()
            ck = engine.nb_cooks(D, codes, 2, s, alpha, q, cut)
            t2 = time.perf_counter()
            t_disp, t_cooks = min(t_disp, t1 - t0), min(t_cooks, t2 - t1)
        say("case %d genes x %d samples, float32 in HBM, 2 groups, one count x 200 planted in %d genes; cutoff qf(0.99, 2, %d) = %.4g"
            % (a.genes, m, planted.size, m - 2, cut))
        say("  nb_cooks %.2f ms, nb_dispersions (gene-wise) %.2f ms beside it: ratio %.3f; best of %d, alternating"
            % (1e3 * t_cooks, 1e3 * t_disp, t_cooks / t_disp, a.reps))
        with np.errstate(invalid="ignore"):
            say("  %d genes with max_cooks past the cutoff, %d with a replacement (%.2f %% of the table)"
                % ((ck["max_cooks"] > cut).sum(), (ck["n_replace"] > 0).sum(), 100.0 * (ck["n_replace"] > 0).mean()))
        rep = np.flatnonzero(ck["n_replace"] > 0)
        if rep.size:
            t0 = time.perf_counter()
            sub = np.ascontiguousarray(c[:, rep])
            second = engine.nb_cooks(sub, codes, 2, s, alpha[rep], q[rep], cut, return_distances=True)
            rows = engine.nb_replacements(sub, codes, s, second["D"], cut, second["trimmed_base"])
            new = sub.copy()
            new[rows["sample"], rows["gene"]] = rows["replacement"]
            xn = engine.nb_dispersions(new, codes, 2, s)
            engine.nb_dispersions(new, codes, 2, s, log_prior_mean=np.where(np.isnan(xn), np.nan, x[rep]), prior_var=0.6)
            an = engine.nb_clip(np.exp(xn), m)
            qn, _ = engine.nb_group_fits(new, codes, 2, s, an)
            engine.nb_cooks(new, codes, 2, s, an, qn, cut, return_distances=True)
            say("  the refit of those %d genes (host table; gathered distances, %d replacements, two dispersion passes, group fits, "
                "distances again): %.2f ms, once" % (rep.size, rows.size, 1e3 * (time.perf_counter() - t0)))
        h = min(a.host_genes, a.genes)
        t0 = time.perf_counter()
        ref = CR.cooks(c[:, :h], codes, 2, s, alpha[:h], q[:h], cut)
        t_host = time.perf_counter() - t0
        with np.errstate(invalid="ignore", divide="ignore"):
            off = np.abs(ck["max_cooks"][:h] - ref["max_cooks"]) / ref["max_cooks"]
        say("  host restatement (numpy, a loop over genes) on %d genes: %.1f ms; scaled by %d / %d: %.2f s; device against it: max_cooks off "
            "by at most %.2g relative, arg_max equal on %d of %d"
            % (h, 1e3 * t_host, a.genes, h, t_host * a.genes / h, np.nanmax(off), (ck["arg_max"][:h] == ref["arg_max"]).sum(), h))
        del D
    for m in (a.samples if a.design else ()):
        import nb_design_restatement as DR
        rng = np.random.default_rng(m)
        s = RR.size_factors(rng, m)
        X, kinds = DR.make_design(rng, m, a.design_cols)
        codes = X[:, -1].astype(np.int32)
        c = DR.nb_class(rng, s, X, kinds, a.genes)
        D = engine.DeviceMatrix.upload(c.astype(np.float32))
        x22 = engine.nb_dispersions(D, codes, 2, s)
        x26, info = engine.nb_design_dispersions(D, X, s, return_info=True)
        a22, a26 = engine.nb_clip(np.exp(x22), m), engine.nb_clip(np.exp(x26), m)
        engine.nb_group_fits(D, codes, 2, s, a22)
        engine.nb_design_fits(D, X, s, a26)
        t = np.full(4, np.inf)
        for _ in range(a.reps):                                         # the calls alternate
            t0 = time.perf_counter()
            engine.nb_dispersions(D, codes, 2, s)
            t1 = time.perf_counter()
            engine.nb_design_dispersions(D, X, s)
            t2 = time.perf_counter()
            engine.nb_group_fits(D, codes, 2, s, a22)
            t3 = time.perf_counter()
            beta, cov, ll, fit = engine.nb_design_fits(D, X, s, a26, return_info=True)
            t4 = time.perf_counter()
            t = np.minimum(t, [t1 - t0, t2 - t1, t3 - t2, t4 - t3])
        live = ~np.isnan(x26)
        say("case %d genes x %d samples, float32 in HBM, design of %d columns (%s)" % (a.genes, m, a.design_cols, ", ".join(kinds)))
        say("  nb_design_dispersions %.2f ms, nb_dispersions (gene-wise, the group column alone) %.2f ms beside it: ratio %.2f; best of %d, "
            "alternating" % (1e3 * t[1], 1e3 * t[0], t[1] / t[0], a.reps))
        say("  inner Newton steps a lane and round: mean %.2f, largest gene mean %.2f; %d genes with a fit that did not converge"
            % (info["steps"][live].mean() / 384.0, info["steps"][live].max() / 384.0, info["n_not_converged"]))
        say("  nb_design_fits %.2f ms, nb_group_fits %.2f ms beside it: ratio %.2f; steps a gene: mean %.1f, largest %d; %d not converged"
            % (1e3 * t[3], 1e3 * t[2], t[3] / t[2], fit["steps"][live].mean(), fit["steps"].max(), fit["n_not_converged"]))
        h = min(a.host_genes, a.genes)
        t0 = time.perf_counter()
        xh = DR.dispersions(c[:, :h], X, s)[0]
        t_host = time.perf_counter() - t0
        res = DR.resolved(c[:, :h], X, s, xh)
        say("  host restatement (vectorised numpy) on %d genes: dispersions %.2f s; scaled by %d / %d: %.0f s; device against it on the "
            "resolved genes (%d): dispersion off by at most %.2g relative"
            % (h, t_host, a.genes, h, t_host * a.genes / h, res.sum(), np.abs(np.expm1(x26[:h][res] - xh[res])).max(initial=0)))
        del D
    for m in (a.samples if a.design_shrink else ()):
        import nb_design_restatement as DR
        import nb_design_shrink_restatement as KR
        rng = np.random.default_rng(m)
        s = RR.size_factors(rng, m)
        X, kinds = DR.make_design(rng, m, a.design_cols)
        c = DR.nb_class(rng, s, X, kinds, a.genes)
        D = engine.DeviceMatrix.upload(c.astype(np.float32))
        x26, disp = engine.nb_design_dispersions(D, X, s, return_info=True)
        alpha = engine.nb_clip(np.exp(x26), m)
        mle, cov, _ = engine.nb_design_fits(D, X, s, alpha)
        bk = mle[:, -1]
        with np.errstate(invalid="ignore"):
            S, A = engine.nb_prior_scale(bk, np.sqrt(cov[:, -1, -1]), use=np.isfinite(bk) & (np.abs(bk) < 10))
        far = engine.nb_design_far_end(bk)
        engine.nb_design_shrink(D, X, s, alpha, mle, far, S)
        t = np.full(2, np.inf)
        for _ in range(a.reps):                                         # the calls alternate
            t0 = time.perf_counter()
            engine.nb_design_dispersions(D, X, s)
            t1 = time.perf_counter()
            beta, info = engine.nb_design_shrink(D, X, s, alpha, mle, far, S, return_info=True)
            t2 = time.perf_counter()
            t = np.minimum(t, [t1 - t0, t2 - t1])
        live = ~np.isnan(beta[:, -1])
        say("case %d genes x %d samples, float32 in HBM, design of %d columns (%s), prior scale %.3f"
            % (a.genes, m, a.design_cols, ", ".join(kinds), S))
        say("  nb_design_shrink %.2f ms, nb_design_dispersions (gene-wise) %.2f ms beside it: ratio %.2f; best of %d, alternating"
            % (1e3 * t[1], 1e3 * t[0], t[1] / t[0], a.reps))
        say("  inner Newton steps a lane and round: nb_design_shrink mean %.2f, largest gene mean %.2f; nb_design_dispersions mean %.2f; "
            "%d genes at the bound, %d with a fit that did not converge"
            % (info["steps"][live].mean() / 384.0, info["steps"][live].max() / 384.0, disp["steps"][live].mean() / 384.0, info["n_at_bound"],
               info["n_not_converged"]))
        h = min(a.host_genes, a.genes)
        t0 = time.perf_counter()
        found = KR.search(c[:, :h], X, s, alpha[:h], far[:h], S, a.design_cols - 1, start=mle[:h])
        t_host = time.perf_counter() - t0
        res = KR.resolved(c[:, :h], X, s, alpha[:h], far[:h], S, a.design_cols - 1, found)
        say("  host restatement (vectorised numpy) on %d genes: %.2f s; scaled by %d / %d: %.0f s; device against it on the resolved genes "
            "(%d): t off by at most %.2g"
            % (h, t_host, a.genes, h, t_host * a.genes / h, res.sum(),
               np.abs(KR.t_of(beta[:h, -1], S) - found["t"])[res].max(initial=0)))
        del D
    for m, kinds in ((m, kinds) for m in (a.samples if a.design_cooks else ()) for kinds in (("intercept", "batch", "age", "group"),
                                                                                             ("intercept", "batch", "centre", "group"))):
        import nb_design_cooks_restatement as KR
        import nb_design_restatement as DR
        rng = np.random.default_rng(m)
        s = RR.size_factors(rng, m)
        age = rng.normal(0.0, 1.0, m)
        cols = {"intercept": np.ones(m), "batch": rng.permutation(np.arange(m) % 2).astype(np.float64), "age": (age - age.mean()) / age.std(ddof=1),
                "centre": rng.permutation(np.arange(m) // 2 % 2).astype(np.float64), "group": rng.permutation(np.arange(m) >= (m + 1) // 2).astype(np.float64)}
        X = np.ascontiguousarray(np.stack([cols[k] for k in kinds], axis=1))
        codes = X[:, -1].astype(np.int32)
        c = DR.nb_class(rng, s, X, ["batch" if k == "centre" else k for k in kinds], a.genes)
        hit = rng.choice(a.genes, int(round(a.outlier_share * a.genes)), replace=False)
        row = rng.integers(0, m, hit.size)
        c[row, hit] = np.maximum(c[row, hit], 5.0) * 200.0
        D = engine.DeviceMatrix.upload(c.astype(np.float32))
        a22 = engine.nb_clip(np.exp(engine.nb_dispersions(D, codes, 2, s)), m)
        a26 = engine.nb_clip(np.exp(engine.nb_design_dispersions(D, X, s)), m)
        q, _ = engine.nb_group_fits(D, codes, 2, s, a22)
        beta, _, _ = engine.nb_design_fits(D, X, s, a26)
        cut2, cutp = engine.nb_cooks_cutoff(m, 2), engine.nb_cooks_cutoff(m, X.shape[1])
        engine.nb_cooks(D, codes, 2, s, a22, q, cut2)
        engine.nb_design_cooks(D, X, s, a26, beta, cutp)
        t = np.full(3, np.inf)
        for _ in range(a.reps):                                         # the calls alternate
            t0 = time.perf_counter()
            engine.nb_cooks(D, codes, 2, s, a22, q, cut2)
            t1 = time.perf_counter()
            engine.nb_design_fits(D, X, s, a26)
            t2 = time.perf_counter()
            ck = engine.nb_design_cooks(D, X, s, a26, beta, cutp)
            t3 = time.perf_counter()
            t = np.minimum(t, [t1 - t0, t2 - t1, t3 - t2])
        n_cells = engine.nb_design_cells(X)[1]
        say("case %d genes x %d samples, float32 in HBM, design of %d columns (%s): %d cells; one count x 200 planted in %d genes; cutoff "
            "qf(0.99, %d, %d) = %.3f" % (a.genes, m, X.shape[1], ", ".join(kinds), n_cells, hit.size, X.shape[1], m - X.shape[1], cutp))
        say("  nb_design_cooks %.2f ms; nb_cooks (the group column alone) %.2f ms beside it: ratio %.2f; nb_design_fits %.2f ms: "
            "nb_design_cooks / (nb_cooks + nb_design_fits) = %.2f; best of %d, alternating"
            % (1e3 * t[2], 1e3 * t[0], t[2] / t[0], 1e3 * t[1], t[2] / (t[0] + t[1]), a.reps))
        with np.errstate(invalid="ignore"):
            say("  %d genes with max_cooks past the cutoff, %d with a replacement" % ((ck["max_cooks"] > cutp).sum(), (ck["n_replace"] > 0).sum()))
        h = min(a.host_genes, a.genes)
        t0 = time.perf_counter()
        want = KR.cooks(c[:, :h], X, s, a26[:h], np.nan_to_num(beta[:h]), cutp)
        t_host = time.perf_counter() - t0
        live = ~np.isnan(want["alpha_robust"])
        say("  host restatement (numpy, a loop over genes) on %d genes: %.1f ms; scaled by %d / %d: %.2f s; device against it: alpha_robust "
            "off by at most %.2g relative, arg_max equal on %d of %d"
            % (h, 1e3 * t_host, a.genes, h, t_host * a.genes / h,
               np.abs(ck["alpha_robust"][:h][live] / want["alpha_robust"][live] - 1.0).max(initial=0),
               (ck["arg_max"][:h] == want["arg_max"]).sum(), h))
        del D
    for m in (() if a.shrink or a.rlog or a.cooks or a.design or a.design_shrink or a.design_cooks else a.samples):
        rng = np.random.default_rng(m)
        s = RR.size_factors(rng, m)
        codes = (np.arange(m) % 2).astype(np.int32)
        c = RR.nb_class(rng, s, codes, 2, a.genes)
        D = engine.DeviceMatrix.upload(c.astype(np.float32))
        t_gene, x = best_of(lambda: engine.nb_dispersions(D, codes, 2, s))
        prior = np.log(0.05 + 2.0 / np.maximum((c / s[:, None]).mean(axis=0), 1e-3))
        t_map, x_map = best_of(lambda: engine.nb_dispersions(D, codes, 2, s, log_prior_mean=prior, prior_var=0.6))
        alpha = engine.nb_clip(np.exp(x_map), m)
        t_fit, fits = best_of(lambda: engine.nb_group_fits(D, codes, 2, s, alpha, return_info=True))
        sparse = np.zeros((m, a.genes), dtype=np.float32)
        sparse[rng.integers(0, m, a.genes), np.arange(a.genes)] = 1.0 + rng.integers(0, 40, a.genes)
        Z = engine.DeviceMatrix.upload(sparse)
        t_free, _ = best_of(lambda: engine.nb_dispersions(Z, codes, 2, s))
        say("case %d genes x %d samples, float32 in HBM, 2 groups" % (a.genes, m))
        say("  nb_dispersions %.2f ms gene-wise, %.2f ms with the prior; nb_group_fits %.2f ms (at most %d steps, %d not converged); "
            "best of %d" % (1e3 * t_gene, 1e3 * t_map, 1e3 * t_fit, fits[2]["steps"].max(), fits[2]["n_not_converged"], a.reps))
        evals = a.genes * m * 64.0 * 6
        say("  %.3g likelihood terms a call: %.1f ps a term on the whole device; lgamma-free table %.2f ms: the "
            "full call is %.1f x it" % (evals, 1e12 * t_gene / evals, 1e3 * t_free, t_gene / t_free))
        h = min(a.host_genes, a.genes)
        t0 = time.perf_counter()
        xh = RR.dispersions(c[:, :h], codes, 2, s)[0]
        t_host = time.perf_counter() - t0
        t0 = time.perf_counter()
        RR.group_fits(c[:, :h], codes, 2, s, np.exp(xh))
        t_host_fit = time.perf_counter() - t0
        res = RR.resolved(c[:, :h], RR.fitted_mu(c[:, :h], codes, 2, s), codes, 2, xh)
        say("  host restatement on %d genes: dispersions %.2f s, group fits (200 bisection steps) %.2f s; scaled by %d / %d: %.0f s and "
            "%.0f s; device against it on the resolved genes (%d): dispersion off by at most %.2g relative"
            % (h, t_host, t_host_fit, a.genes, h, t_host * a.genes / h, t_host_fit * a.genes / h, res.sum(),
               np.abs(np.expm1(x[:h][res] - xh[res])).max(initial=0)))
        del D, Z
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "shrink_rate.txt" if a.shrink else "rlog_rate.txt" if a.rlog else "cooks_rate.txt" if a.cooks else "design_rate.txt" if a.design else "design_shrink_rate.txt" if a.design_shrink else "design_cooks_rate.txt" if a.design_cooks else "rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
