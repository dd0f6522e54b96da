"""Shared by the patient sub-group tests (K12): a synthetic cohort as the duck-typed AnnData tl reads, and its proportions frame."""
import numpy as np
import pandas as pd

GROUPS = ("Tumor 1", "Tumor 2", "Tumor 3")
CELL = "alpha"


class Cohort:
    def __init__(self, X, obs, var_names):
        self.X, self.obs, self.var_names, self.uns = X, obs, var_names, {}


def cohort(seed=0, n_cells=4400, n_genes=400, n_shifted=40, equal_variance=False, id_column="sampIeD"):
    """12 samples (6 / 5 / 1 over the three labels), about 10 in 11 cells of type CELL and the rest 'beta', log1p-scale float32
    values: log1p of gamma-Poisson counts with ``n_shifted`` genes shifted between the first two groups and gene 3 constant 0
    (``equal_variance``: standard normal values instead, the same true variance for every gene, no constant gene).
    Returns (adata, proportions, labels per cell)."""
    rng = np.random.default_rng(seed)
    samples = ["s%02d" % i for i in range(12)]
    label = dict(zip(samples, [GROUPS[0]] * 6 + [GROUPS[1]] * 5 + [GROUPS[2]]))
    sample = rng.choice(samples, n_cells)
    cell = np.where(rng.random(n_cells) < 1.0 / 11.0, "beta", CELL)
    lab = np.array([label[s] for s in sample], dtype=object)
    if equal_variance:
        X = rng.standard_normal((n_cells, n_genes))
    else:
        lam = np.maximum(rng.lognormal(0.5, 1.0, n_genes), 0.3)
        fold = np.ones((n_cells, n_genes))
        shifted = rng.choice(np.arange(4, n_genes), n_shifted, replace=False)
        fold[np.ix_(lab == GROUPS[1], shifted)] = rng.uniform(1.5, 3.0, n_shifted) ** rng.choice([-1.0, 1.0], n_shifted)
        X = np.log1p(rng.poisson(lam * fold * rng.gamma(2.0, 0.5, (n_cells, 1))))
        X[:, 3] = 0.0
    obs = pd.DataFrame({"cell_types": cell.astype(object), "sampleID": sample.astype(object)})
    props = pd.DataFrame({id_column: samples, "Predicted_Labels": [label[s] for s in samples]})
    adata = Cohort(np.ascontiguousarray(X, dtype=np.float32), obs, ["g%03d" % j for j in range(n_genes)])
    return adata, props, lab


def cell_values(adata):
    """(values of the cells of CELL, their rows)"""
    rows = np.flatnonzero(np.asarray(adata.obs["cell_types"]) == CELL)
    X = adata.X[rows]
    return np.asarray(X.toarray() if hasattr(X, "toarray") else X), rows
