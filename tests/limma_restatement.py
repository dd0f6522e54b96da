"""An independent restatement, with numpy / pandas / scipy on the host, of what pilot_amd computes for the patient sub-group
workflow (K12): group moments, scanpy's seurat-flavour highly variable genes, limma's lmFit -> eBayes -> topTable for PILOT's
design and for a two-group design, and Welch's t per cell type.  Not collected by pytest.

It shares no code and no algebra with the package: moments are numpy two-pass sums in float64; lmFit solves the explicit design
matrix with ``np.linalg.lstsq`` and takes the residuals of the fitted values (the package uses closed forms in the group
moments); Welch's t is ``scipy.stats.ttest_ind(equal_var=False)``.  eBayes and the HVG rule follow limma's ``fitFDist`` /
``squeezeVar`` / ``trigammaInverse`` and scanpy's ``_highly_variable_genes_single_batch`` as documented; neither package is
installed here, so both are UNPINNED restatements."""
import numpy as np
import pandas as pd
from scipy import special, stats


def group_moments(Y, codes, n_groups, transform=None, cols=None):
    """(count, mean, m2) per group and column: two passes in float64"""
    Y = np.asarray(Y)
    if cols is not None:
        Y = Y[:, np.asarray(cols)]
    V = Y.astype(np.float64)
    if transform == "expm1":
        V = np.expm1(V)
    codes = np.asarray(codes)
    count = np.zeros(n_groups, dtype=np.int64)
    mean = np.full((n_groups, V.shape[1]), np.nan)
    m2 = np.full((n_groups, V.shape[1]), np.nan)
    for g in range(n_groups):
        R = V[codes == g]
        count[g] = R.shape[0]
        if R.shape[0]:
            mean[g] = R.sum(axis=0) / R.shape[0]
            m2[g] = ((R - mean[g]) ** 2).sum(axis=0)
    return count, mean, m2


def highly_variable_genes(X, n_top_genes=2000, n_bins=20):
    """scanpy's flavor='seurat' rule for one batch; X holds log1p values"""
    V = np.expm1(np.asarray(X, dtype=np.float64))
    mean = V.mean(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        var = ((V - mean) ** 2).sum(axis=0) / (V.shape[0] - 1)
        mean[mean == 0] = 1e-12
        dispersion = var / mean
        dispersion[dispersion == 0] = np.nan
        dispersion = np.log(dispersion)
    mean = np.log1p(mean)
    df = pd.DataFrame({"means": mean, "dispersions": dispersion})
    df["mean_bin"] = pd.cut(df["means"], bins=n_bins)
    grouped = df.groupby("mean_bin", observed=False)["dispersions"]
    disp_mean_bin = grouped.mean()
    disp_std_bin = grouped.std(ddof=1)
    one_gene_per_bin = disp_std_bin.isnull()
    disp_std_bin[one_gene_per_bin] = disp_mean_bin[one_gene_per_bin].values
    disp_mean_bin[one_gene_per_bin] = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        df["dispersions_norm"] = (df["dispersions"].values - disp_mean_bin[df["mean_bin"]].values) / disp_std_bin[df["mean_bin"]].values
    dn = df["dispersions_norm"].values
    ranked = dn[~np.isnan(dn)]
    ranked[::-1].sort()
    n_top = min(n_top_genes, ranked.size)
    cutoff = ranked[n_top - 1]
    df["highly_variable"] = np.nan_to_num(dn) >= cutoff
    df.attrs["cutoff"] = float(cutoff)
    return df.drop(columns="mean_bin")


def trigamma_inverse(x):
    if x > 1e7:
        return 1.0 / np.sqrt(x)
    if x < 1e-6:
        return 1.0 / x
    y = 0.5 + 1.0 / x
    it = 0
    while True:
        it += 1
        tri = special.polygamma(1, y)
        dif = tri * (1.0 - tri / x) / special.polygamma(2, y)
        y = y + dif
        if -dif / y < 1e-8 or it > 50:
            return float(y)


def fit_f_dist(s2, df):
    """limma's fitFDist without covariate: (scale s0^2, df0)"""
    x = np.maximum(np.asarray(s2, dtype=np.float64), 0.0)
    m = np.median(x)
    if m == 0:
        raise ValueError("more than half of the residual variances are exactly zero")
    x = np.maximum(x, 1e-5 * m)
    e = np.log(x) - special.digamma(df / 2.0) + np.log(df / 2.0)
    emean = e.mean()
    evar = ((e - emean) ** 2).sum() / (e.size - 1) - special.polygamma(1, df / 2.0)
    if evar > 0:
        df0 = 2.0 * trigamma_inverse(float(evar))
        s20 = np.exp(emean + special.digamma(df0 / 2.0) - np.log(df0 / 2.0))
    else:
        df0 = np.inf
        s20 = np.exp(emean)
    return float(s20), float(df0)


def lm_fit(Y, design):
    """lmFit for a full-rank design without weights: coefficients (p x G), unscaled stdev (p), sigma^2 (G), residual df"""
    Y = np.asarray(Y, dtype=np.float64)
    X = np.asarray(design, dtype=np.float64)
    beta = np.linalg.lstsq(X, Y, rcond=None)[0]
    resid = Y - X @ beta
    df = X.shape[0] - np.linalg.matrix_rank(X)
    return beta, np.sqrt(np.diag(np.linalg.inv(X.T @ X))), (resid ** 2).sum(axis=0) / df, float(df)


def bh(p):
    p = np.asarray(p, dtype=np.float64)
    order = np.argsort(p, kind="stable")
    ranked = p[order] * p.size / np.arange(1, p.size + 1)
    adj = np.minimum(np.minimum.accumulate(ranked[::-1])[::-1], 1.0)
    out = np.empty_like(adj)
    out[order] = adj
    return out


def diff_expressions(values, labels, group1, group2, design="reference"):
    """values: cells x genes; labels: one sub-group label per cell.  A dict of per-gene arrays plus df_prior and s2_prior."""
    labels = np.asarray(labels, dtype=object)
    keep = (labels == group1) | (labels == group2)
    Y, lab = np.asarray(values, dtype=np.float64)[keep], labels[keep]
    if design == "reference":                                     # unclass(as.factor(labels)): 1 for the name sorting first
        first = sorted([group1, group2])[0]
        X = np.where(lab == first, 1.0, 2.0)[:, None]
        coef = 0
    else:
        X = np.column_stack([np.ones(lab.size), (lab == group1).astype(np.float64)])
        coef = 1
    beta, unscaled, s2, df = lm_fit(Y, X)
    s20, df0 = fit_f_dist(s2, df)
    s2_post = np.full_like(s2, s20) if np.isinf(df0) else (df0 * s20 + df * s2) / (df0 + df)
    t = beta[coef] / (unscaled[coef] * np.sqrt(s2_post))
    df_total = min(df + df0, s2.size * df)
    p = 2.0 * stats.t.sf(np.abs(t), df_total)
    return {"logFC": beta[coef], "AveExpr": Y.mean(axis=0), "t": t, "P.Value": p, "adj.P.Val": bh(p), "df_prior": df0, "s2_prior": s20}


def welch_table(proportions, cell_types, labels, group1, group2):
    a, b = proportions[proportions[labels] == group1], proportions[proportions[labels] == group2]
    res = [stats.ttest_ind(a[c], b[c], equal_var=False) for c in cell_types]
    adj = bh([r[1] for r in res])
    out = pd.DataFrame({"cell_type": list(cell_types), "adjPval": adj, "-logPval": -np.log(adj), "score": [r[0] for r in res]})
    return out.sort_values(by=["score", "-logPval"], ascending=[False, False])
