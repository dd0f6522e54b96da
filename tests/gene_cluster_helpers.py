"""Shared by the gene-cluster differentiation tests: the reference fixture (tests/golden/gene_cluster_4types.npz, written by
tests/golden/gen_gene_cluster_golden.py) as inputs for tl, a synthetic counts cohort, and a pure host restatement of
tl.infer_gene_cluster_differentiation built from the same draws (bootstrap fits: bootfit_restatement; mean-curve fits:
trajfit_restatement; the Wald step: tl._gcd_wald, itself held to the reference by test_gene_cluster_diff_args.py)."""
import os

import numpy as np
import pandas as pd

import bootfit_restatement as BR
import trajfit_restatement as TR
from pilot_amd import tl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gene_cluster_4types.npz")
TABLE_COLUMNS = ["Gene ID", "Expression pattern", "Slope", "Fitted function", "Intercept", "Treat", "Treat2", "adjusted P-value",
                 "R-squared", "mod_rsquared_adj"]


class Cohort:
    def __init__(self, X, obs, var_names, uns):
        self.X, self.obs, self.var_names, self.uns = X, obs, var_names, uns


def load_fixture():
    z = dict(np.load(GOLDEN, allow_pickle=False))
    obs = pd.DataFrame({"cell_types": z["cell_types"], "sampleID": z["sample_ids"]})
    orders = pd.DataFrame({"sampleID": z["order_samples"], "Time_score": z["order_times"]})
    ad = Cohort(z["X"], obs, list(z["genes"]), dict(orders=orders))
    tables = {}
    for c in sorted(set(z["cell_types"])):
        tables[c] = pd.DataFrame({k: z["table_%s_%s" % (c, k)] for k in TABLE_COLUMNS})
    return z, ad, tables


def counts_cohort(seed=5, n_samples=12, n_genes=10, types=(("A", 0.5), ("B", 0.3), ("C", 0.2))):
    """cells x genes Poisson counts with per-type trends; a genes_importance-style table per type (host restatement, Huber,
    p_val 1) with some genes dropped, so genes appear in 0 .. 3 types"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(6, 14, n_samples)
    sample = np.repeat(np.arange(n_samples), sizes)
    names = [t for t, _ in types]
    ctype = rng.choice(names, sample.size, p=[p for _, p in types])
    perm = rng.permutation(sample.size)
    sample, ctype = sample[perm], ctype[perm]
    time = rng.permutation(n_samples)
    eff = {t: rng.normal(0, 1.0, n_genes) for t in names}
    lam = np.stack([4.0 * np.exp(eff[c] * time[s] / n_samples) for c, s in zip(ctype, sample)])
    X = rng.poisson(lam).astype(np.float64)
    obs = pd.DataFrame({"cell_types": ctype, "sampleID": ["s%d" % s for s in sample]})
    orders = pd.DataFrame({"sampleID": ["s%d" % s for s in np.argsort(time)], "Time_score": np.arange(1, n_samples + 1)})
    genes = ["g%d" % i for i in range(n_genes)]
    ad = Cohort(X, obs, genes, dict(orders=orders))
    Xn = TR.normalize_log1p(X)
    tables = {}
    for t in names:
        rows, x = tl._cell_rows(ad, t, "sampleID", "cell_types", orders, "Time_score")
        res = [TR.best_model(x, Xn[rows, g], pval_thr=1.0, kind="huber") for g in range(n_genes)]
        tab = pd.DataFrame(TR.table(res, genes, "Gene ID", 1.0)[0])
        tables[t] = tab[rng.random(len(tab)) > 0.25].reset_index(drop=True)
    return ad, tables


def host_restatement(ad, tables, seed, cluster_names=None, n_points=20, start=1, end=20, fc_thr=1.5, eigen_thresh=1e-8,
                     n_bootstraps=50, normalize=True):
    """The whole computation on the host from RandomState(seed): returns (frame, dict of per Wald row arrays: ``margin`` (the
    table2 choice's margin), ``table2`` (its model), ``boot`` (B x 6 bootstrap betas))."""
    cluster_names = list(tables) if cluster_names is None else list(cluster_names)
    gene_list = np.unique(np.concatenate([tables[c]["Gene ID"].to_numpy() for c in cluster_names]))
    rs = np.random.RandomState(seed)
    pline = np.linspace(start, end, n_points)
    cut = np.log(np.power(2, np.log2(fc_thr)))
    orders = ad.uns["orders"]
    X = np.asarray(ad.X, dtype=np.float64)
    Xn = TR.normalize_log1p(X) if normalize else X

    def row(c, g):
        t = tables[c]
        return t[t["Gene ID"] == g].iloc[0]
    out, margins, t2s, boots = [], [], [], []
    for g in gene_list:
        cl = [c for c in cluster_names if (tables[c]["Gene ID"] == g).any()]
        if len(cl) == 1:
            r = row(cl[0], g)
            out.append([g, cl[0], 1.0, 1, 0.0, 0.0, r["Expression pattern"], r["adjusted P-value"], r["R-squared"],
                        r["mod_rsquared_adj"]])
            continue
        for c in cl:
            r1 = row(c, g)
            f1 = r1["Fitted function"]
            curve1 = tl._gcd_features(f1, pline, False) @ tl._gcd_params(r1)
            ybar = np.mean(np.stack([tl._gcd_features(row(o, g)["Fitted function"], pline, False) @ tl._gcd_params(row(o, g))
                                     for o in cl if o != c]), axis=0)
            bm = TR.best_model(pline, ybar, pval_thr=1.0, kind="huber")
            margins.append(bm["margin"])
            f2 = TR.MODELS[bm["chosen"]]
            p2 = bm["fits"][bm["chosen"]]["params"]
            curve2 = tl._gcd_features(f2, pline, False) @ p2
            rows, x = tl._cell_rows(ad, c, "sampleID", "cell_types", orders, "Time_score")
            o = np.argsort(x.astype(orders["Time_score"].dtype), kind="quicksort")
            x, y = x[o], Xn[rows[o], list(ad.var_names).index(g)]
            boot = np.zeros((n_bootstraps, 6))
            for b in range(n_bootstraps):
                idx = rs.randint(0, x.size, x.size)
                boot[b, :3] = tl._gcd_fill_betas(f1, BR.huber_opt(x, x[idx], y, f1)[0])
            for b in range(n_bootstraps):
                idx = rs.randint(0, n_points, n_points)
                boot[b, 3:] = tl._gcd_fill_betas(f2, BR.huber_opt(pline, pline[idx], ybar, f2)[0])
            betas = tl._gcd_fill_betas(f1, tl._gcd_params(r1)) + tl._gcd_fill_betas(f2, p2)
            t2s.append(f2)
            boots.append(boot)
            w, df, pv = tl._gcd_wald(tl._gcd_features(f1, pline, True), tl._gcd_features(f2, pline, True), betas, boot, cut,
                                     eigen_thresh)
            out.append([g, c, w, df, pv, np.log2(curve1.mean()) - np.log2(curve2.mean()), r1["Expression pattern"],
                        r1["adjusted P-value"], r1["R-squared"], r1["mod_rsquared_adj"]])
    return pd.DataFrame(out, columns=tl._GCD_COLUMNS), dict(margin=np.array(margins), table2=t2s, boot=np.array(boots))
