#!/usr/bin/env python3
"""Generate tests/golden/gene_cluster_*.npz by RUNNING THE REFERENCE's infer_gene_cluster_differentiation
(pilotpy/tools/Gene_cluster_specific.py) on a small synthetic cohort.  CPU only; needs the reference checkout (see gen_golden.py).

Two shims, both only for what this environment lacks: ``multipletests`` (statsmodels is not installed) is a Benjamini-Hochberg
restatement, set as ``F.multipletests`` and ``F.smf.multitest``; ``mean_squared_error(..., squared=False)`` lost its keyword
in scikit-learn 1.6 and is restated.  The genes_importance tables (inputs) come from tests/trajfit_restatement.py with a Treat2
column, the cells' expression is normalised log counts (stored; the tests call with ``normalize=False``).  Both are stored as the
reference reads them back from its CSV files.

Recorded: the inputs, the output frame, a SHA-256 of every resample the reference drew (np.random.choice wrapped), every
bootstrap beta, each row's mean curve and table2 choice with its adjusted-R^2 margin, and per row the largest relative gap of a
scikit-learn Huber fit (bootstraps and the chosen table2 fit) above the optimum of its objective (tests/bootfit_restatement.py)."""
import hashlib
import os
import sys
import tempfile
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

import bootfit_restatement as BR  # noqa: E402
import gen_golden  # noqa: E402
import trajfit_restatement as TR  # noqa: E402

SEED = 20261015
CELL_TYPES = ["alpha", "beta", "gamma", "delta"]
CELL_COUNTS = {"alpha": 70, "beta": 45, "gamma": 30, "delta": 9}    # delta: fewer than 10 cells


def cohort(rng, n_samples=8, n_genes=18):
    """cells x genes counts with a per-cell-type trend over the samples' Time_score 1..n_samples"""
    genes = ["g%02d" % k for k in range(n_genes)]
    rows = []
    for c in CELL_TYPES:
        n = CELL_COUNTS[c]
        smp = np.sort(np.r_[np.arange(n_samples), rng.integers(0, n_samples, n - n_samples)])[:n] if n >= n_samples else \
            np.sort(rng.choice(n_samples, n, replace=False))
        for s in rng.permutation(smp):
            rows.append((c, "s%d" % s, int(s) + 1))
    obs = pd.DataFrame(rows, columns=["cell_types", "sampleID", "t"])
    t = obs["t"].to_numpy(dtype=np.float64)
    base = rng.uniform(1.0, 6.0, n_genes)
    slope = {c: rng.normal(0.0, 0.25, n_genes) for c in CELL_TYPES}
    curv = {c: rng.normal(0.0, 0.03, n_genes) for c in CELL_TYPES}
    mu = np.stack([base * np.exp(slope[c] * (ti - 4.5) / 4 + curv[c] * (ti - 4.5) ** 2) for c, ti in zip(obs["cell_types"], t)])
    X = rng.poisson(mu).astype(np.float64)
    X[:, 0] = rng.poisson(3.0, X.shape[0])            # a flat gene
    return obs.drop(columns="t"), X, genes


def main():
    rng = np.random.default_rng(SEED)
    obs, counts, genes = cohort(rng)
    orders = pd.DataFrame({"sampleID": ["s%d" % s for s in range(8)], "Time_score": np.arange(1, 9, dtype=np.int64)})
    Xn = TR.normalize_log1p(counts)
    pos = {s: i for i, s in enumerate(orders["sampleID"])}

    # genes_importance-style tables (restatement, Huber, p_val 1), then a few genes dropped per cell type
    tables, cells = {}, {}
    for c in CELL_TYPES:
        sel = np.flatnonzero(obs["cell_types"].to_numpy() == c)
        sel = sel[np.argsort([pos[s] for s in obs["sampleID"].to_numpy()[sel]], kind="stable")]
        x = orders["Time_score"].to_numpy()[[pos[s] for s in obs["sampleID"].to_numpy()[sel]]]
        res = [TR.best_model(x.astype(np.float64), Xn[sel, g], pval_thr=1.0, kind="huber") for g in range(len(genes))]
        rows, _ = TR.table(res, genes, "Gene ID", 1.0)
        tab = pd.DataFrame(rows)
        keep = rng.random(len(tab)) > 0.3
        tables[c] = tab[keep].reset_index(drop=True)
        cells[c] = (sel, x)
    cluster_names = ["beta", "alpha", "delta", "gamma"]
    gene_list = np.unique(np.concatenate([tables[c]["Gene ID"].to_numpy() for c in cluster_names]))

    T = gen_golden.import_reference()
    import pilotpy.tools.Gene_cluster_specific as GC
    import pilotpy.tools.Gene_cluster_specific_functions as F
    from sklearn.linear_model import HuberRegressor

    def multipletests(p, method="fdr_bh"):
        assert method == "fdr_bh"
        from pilot_amd.tl import _bh_adjust
        return None, _bh_adjust(p)
    F.multipletests = multipletests
    F.smf.multitest = type("mt", (), {"multipletests": staticmethod(multipletests)})
    F.mean_squared_error = lambda y, pr, squared=True: float(np.sqrt(np.mean((np.asarray(y) - np.asarray(pr)) ** 2)))

    log = []                    # every HuberRegressor fit: (phase, func, X, y, params, scale, epsilon)
    draws = []
    phase = ["boot"]

    class RecHuber(HuberRegressor):
        def fit(self, X, y, sample_weight=None):
            r = super().fit(X, y, sample_weight)
            log.append(dict(phase=phase[0], X=np.array(X, dtype=np.float64), y=np.array(y, dtype=np.float64),
                            params=np.r_[self.intercept_, self.coef_], scale=float(self.scale_), eps=float(self.epsilon)))
            return r
    F.HuberRegressor = RecHuber
    fits2 = []
    orig_best = F._fit_best_model_

    def best_wrapped(target, data, pval_thr=0.05, model_type="HuberRegressor", fun_types=["linear", "linear_quadratic", "quadratic"]):
        phase[0] = "table2"
        inner = []
        orig_fit = F._fit_model_

        def fit_rec(func_type, X, y, model_type):
            r = orig_fit(func_type, X, y, model_type)
            inner.append((func_type, float(r["rsquared_adj"]), np.asarray(r["pvalues"], dtype=np.float64), len(log) - 1))
            return r
        F._fit_model_ = fit_rec
        try:
            tab = orig_best(target, data, pval_thr=pval_thr, model_type=model_type, fun_types=fun_types)
        finally:
            F._fit_model_ = orig_fit
            phase[0] = "boot"
        fits2.append(dict(ybar=np.asarray(target.values[0], dtype=np.float64), inner=inner,
                          chosen=None if tab is None else str(tab.iloc[0, 3])))
        return tab
    GC._fit_best_model_ = best_wrapped
    captured = []
    orig_ext = GC.extend_stats

    def ext_wrapped(all_stats, path_to_results, *a, **k):
        r = orig_ext(all_stats, path_to_results, *a, **k)
        captured.append(r)
        return r
    GC.extend_stats = ext_wrapped
    orig_choice = np.random.choice

    def choice_rec(*a, **k):
        r = orig_choice(*a, **k)
        draws.append(np.asarray(r, dtype=np.int64))
        return r

    with tempfile.TemporaryDirectory() as tmp:
        for c in CELL_TYPES:
            os.makedirs(os.path.join(tmp, "Markers", c))
            tables[c].to_csv(os.path.join(tmp, "Markers", c, "Whole_expressions.csv"))
            sel, x = cells[c]
            d = pd.DataFrame(Xn[sel], columns=genes)
            d["Time_score"] = x
            os.makedirs(os.path.join(tmp, "cells"), exist_ok=True)
            d.to_csv(os.path.join(tmp, "cells", c + ".csv"), index=False)
            # what the reference reads back (pandas' default float parser is not always correctly rounded): the fixture's inputs
            tables[c] = pd.read_csv(os.path.join(tmp, "Markers", c, "Whole_expressions.csv"), index_col=0)
            Xn[sel] = pd.read_csv(os.path.join(tmp, "cells", c + ".csv"))[genes].to_numpy(dtype=np.float64)
        np.random.seed(SEED % 2 ** 31)
        np.random.choice = choice_rec
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                GC.infer_gene_cluster_differentiation(list(gene_list), cluster_names, start=1, end=8, path_to_results=tmp)
        finally:
            np.random.choice = orig_choice
    out = captured[0].reset_index(drop=True)
    print(out.head(12).to_string())

    # per Wald row: bootstrap betas (50 x 6), table2 choice, margin, largest sklearn gap above the optimum
    boots = [f for f in log if f["phase"] == "boot"]
    R = len(fits2)
    assert len(boots) == 100 * R, (len(boots), R)
    pline = np.linspace(1, 8, 20)
    fill = {"linear": lambda p: [p[0], p[1], 0.0], "quadratic": lambda p: [p[0], 0.0, p[1]],
            "linear_quadratic": lambda p: [p[0], p[1], p[2]]}
    B6 = np.zeros((R, 50, 6))
    gap = np.zeros(R)
    eps_ok = np.ones(R, dtype=bool)
    ch2 = np.full(R, -1)
    prm2 = np.full((R, 3), np.nan)
    margin = np.full(R, np.inf)
    wald_rows = [k for k in range(len(out)) if not (out["waldStat"][k] == 1 and out["df"][k] == 1 and out["pvalue"][k] == 0.0
                                                    and out["FC"][k] == 0.0)]
    assert len(wald_rows) == R
    cell_x = {}
    for j in range(R):
        c = out["cluster"][wald_rows[j]]
        xs = np.sort(cells[c][1], kind="quicksort")
        cell_x[c] = xs
        eps_ok[j] = all(f["eps"] == 1.35 for f in boots[100 * j:100 * j + 100])
        t2 = fits2[j]
        elig = [(fn, r2) for fn, r2, pv, _ in t2["inner"] if np.all(pv <= 1.0)]
        best = max(r2 for _, r2 in elig)
        ch2[j] = TR.MODELS.index(t2["chosen"])
        for fn, r2 in elig:
            if fn != t2["chosen"]:
                margin[j] = min(margin[j], abs(best - r2))
        i2 = [li for fn, _, _, li in t2["inner"] if fn == t2["chosen"]][0]
        prm2[j, :len(log[i2]["params"])] = log[i2]["params"]
        chk = [(log[i2], t2["chosen"], pline)]
        g, c = out["gene"][wald_rows[j]], out["cluster"][wald_rows[j]]
        f1 = tables[c][tables[c]["Gene ID"] == g]["Fitted function"].values[0]
        for side, fn, xb in ((0, f1, cell_x[c]), (1, t2["chosen"], pline)):
            for b in range(50):
                f = boots[100 * j + 50 * side + b]
                B6[j, b, 3 * side:3 * side + 3] = fill[fn](f["params"])
                chk.append((f, fn, xb))
        worst = 0.0
        for f, fn, xb in chk:
            xr = f["X"][:, 0] if fn != "quadratic" else np.sqrt(f["X"][:, 0])
            _, _, Fopt = BR.huber_opt(xb, xr, f["y"], fn)
            Fs = BR.objective(xr, f["y"], fn, f["params"], f["scale"])
            worst = max(worst, (Fs - Fopt) / abs(Fopt))
        gap[j] = worst
    digest = hashlib.sha256(b"".join(d.tobytes() for d in draws)).hexdigest()
    sizes = np.array([d.size for d in draws[::50]], dtype=np.int64)
    print("rows", len(out), "wald rows", R, "held (gap <= 1e-9, margin > 1e-9):", int(((gap <= 1e-9) & (margin > 1e-9) & eps_ok).sum()))

    tab_cols = ["Gene ID", "Expression pattern", "Slope", "Fitted function", "Intercept", "Treat", "Treat2", "adjusted P-value",
                "R-squared", "mod_rsquared_adj"]
    blob = dict(
        seed=SEED % 2 ** 31, start=1, end=8, n_points=20, fc_thr=1.5, eigen_thresh=1e-8,
        X=Xn, counts=counts, genes=np.array(genes), cell_types=obs["cell_types"].to_numpy().astype(str),
        sample_ids=obs["sampleID"].to_numpy().astype(str), order_samples=orders["sampleID"].to_numpy().astype(str),
        order_times=orders["Time_score"].to_numpy(), cluster_names=np.array(cluster_names), gene_list=gene_list.astype(str),
        draw_sha256=digest, draw_sizes=sizes,
        boot=B6, t2_chosen=ch2, t2_params=prm2, t2_margin=margin, t2_ybar=np.stack([f["ybar"] for f in fits2]),
        sk_gap=gap, eps_ok=eps_ok, wald_rows=np.array(wald_rows),
        out_gene=out["gene"].to_numpy().astype(str), out_cluster=out["cluster"].to_numpy().astype(str),
        out_pattern=out["Expression pattern"].to_numpy().astype(str),
        **{"out_" + k: out[k].to_numpy(dtype=np.float64) for k in ["waldStat", "df", "pvalue", "FC", "fit-pvalue", "fit-rsquared",
                                                                   "fit-mod-rsquared"]},
    )
    for c in CELL_TYPES:
        for k in tab_cols:
            v = tables[c][k].to_numpy()
            blob["table_%s_%s" % (c, k)] = v.astype(str) if v.dtype == object else v
    np.savez_compressed(os.path.join(HERE, "gene_cluster_4types.npz"), **blob)
    print("wrote gene_cluster_4types.npz", digest)


if __name__ == "__main__":
    main()
