"""Host restatements for the pseudobulk tests (K14), written independently of pilot_amd: the grouped sum by np.add.at on float64,
the reference's pandas expressions (plot/pseudobulk_DE_analysis.py:590-610) on the dense frame, and DESeq2's median-of-ratios
size factors as an explicit loop per sample.  No device, no pilot_amd import."""
import math

import numpy as np
import pandas as pd


def group_sums(Y, codes, n_groups, cols=None):
    """(count int64[n_groups], sums float64[n_groups, n_sel]); rows with a negative code enter nothing"""
    Y = np.asarray(Y)
    codes = np.asarray(codes)
    if cols is not None:
        Y = Y[:, np.asarray(cols, dtype=np.int64)]
    used = np.flatnonzero(codes >= 0)
    count = np.bincount(codes[used], minlength=n_groups).astype(np.int64)
    sums = np.zeros((n_groups, Y.shape[1]), dtype=np.float64)
    np.add.at(sums, codes[used], Y[used].astype(np.float64))
    return count, sums


def abs_sums(Y, codes, n_groups, cols=None):
    """sum |y| per group and column: the scale of the rounding bound of a sum"""
    return group_sums(np.abs(np.asarray(Y, dtype=np.float64)), codes, n_groups, cols)[1]


def aggr_counts(adata, celltype_col="cell_types", sample_col="sampleID"):
    """the reference's lines 591-594 on the dense matrix (adata.to_df() is DataFrame(X, columns=var_names))"""
    X = adata.X.toarray() if hasattr(adata.X, "toarray") else np.asarray(adata.X)
    counts_df = pd.DataFrame(X, columns=list(adata.var_names))
    counts_df[[celltype_col, sample_col]] = adata.obs[[celltype_col, sample_col]].values
    return counts_df.groupby([celltype_col, sample_col]).sum()


def pseudobulk_inputs(aggr, proportion_df, cell_type, cluster_col="Predicted_Labels", remove_samples=()):
    """the reference's lines 597-610 on its aggr_counts"""
    cluster_counts = aggr.loc[cell_type]
    cluster_metadata = proportion_df.loc[cluster_counts.index.values].copy()
    cluster_metadata["stage"] = cluster_metadata[cluster_col].values
    if remove_samples is not None:
        for sample in remove_samples:
            if sample in cluster_metadata.index:
                cluster_metadata = cluster_metadata.drop(index=sample)
            if sample in cluster_counts.index:
                cluster_counts = cluster_counts.drop(index=sample)
    cluster_metadata = cluster_metadata.loc[cluster_counts.index]
    cluster_counts = cluster_counts.loc[:, (cluster_counts != 0).any(axis=0)]
    return cluster_counts, cluster_metadata


def _log(x):
    """numpy's logarithm of one value (the C library's may differ from it in the last bit, which is all of a 1e-15 bound)"""
    return float(np.log(np.float64(x)))


def size_factors(counts):
    """estimateSizeFactorsForMatrix(round(t(counts))) with DESeq2's defaults, one sample at a time: the genes whose rounded count
    is positive in every sample, per sample the median of log(count) - mean over samples of log(count), exponentiated"""
    c = [[float(round(float(v))) for v in row] for row in np.asarray(counts, dtype=np.float64)]   # Python's round: half to even, as R's
    n_s, n_g = len(c), len(c[0])
    usable = [g for g in range(n_g) if all(c[s][g] > 0 for s in range(n_s))]
    if not usable:
        raise ValueError("every gene contains at least one zero")
    log_gm = {g: sum(_log(c[s][g]) for s in range(n_s)) / n_s for g in usable}
    out = []
    for s in range(n_s):
        ratios = sorted(_log(c[s][g]) - log_gm[g] for g in usable)
        m = len(ratios)
        med = ratios[m // 2] if m % 2 else 0.5 * (ratios[m // 2 - 1] + ratios[m // 2])
        out.append(math.exp(med))
    return np.asarray(out)
