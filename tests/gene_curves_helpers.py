"""Shared by the gene curve clustering tests: the reference fixture (tests/golden/gene_curves_1type.npz, written by
tests/golden/gen_gene_curves_golden.py) as inputs for tl and for the restatement (tests/curves_restatement.py)."""
import os

import numpy as np
import pandas as pd

import curves_restatement as CR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gene_curves_1type.npz")
TABLE_COLUMNS = ["Gene ID", "Expression pattern", "Slope", "Fitted function", "Intercept", "Treat", "Treat2", "adjusted P-value",
                 "R-squared", "mod_rsquared_adj"]


class Cohort:
    def __init__(self, X, obs, var_names, uns):
        self.X, self.obs, self.var_names, self.uns = X, obs, var_names, uns


def load():
    return dict(np.load(GOLDEN, allow_pickle=False))


def table(g):
    return pd.DataFrame({k: g["table_" + k] for k in TABLE_COLUMNS})


def adata(g, X=None):
    """the fixture's cells as the duck-typed AnnData tl reads (X: another form of the same matrix, e.g. float32 or CSR)"""
    obs = pd.DataFrame({"cell_types": np.full(g["sample_ids"].size, str(g["cell"])), "sampleID": g["sample_ids"]})
    orders = pd.DataFrame({"sampleID": g["order_samples"], "Time_score": g["order_times"]})
    return Cohort(g["X"] if X is None else X, obs, list(g["genes"]), dict(orders=orders))


def restated_inputs(g, thr=None, pthr=None, X=None):
    """(selected table, times, sd T x G, params G x 3, model names) of the restatement on the fixture's inputs"""
    sel = CR.select(table(g), thr=float(g["thr"]) if thr is None else thr, pthr=float(g["pthr"]) if pthr is None else pthr)
    genes = list(g["genes"])
    cols = [genes.index(x) for x in sel["Gene ID"]]
    times, sd = CR.segment_std((g["X"] if X is None else X)[:, cols], g["cell_times"])
    return sel, times, sd, sel[["Intercept", "Treat", "Treat2"]].to_numpy(dtype=np.float64), list(sel["Fitted function"])
