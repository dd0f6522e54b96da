#!/usr/bin/env python3
"""Generate tests/golden/gene_curves_1type.npz by RUNNING THE REFERENCE's get_noised_curves, cluster_genes_curves and
compute_curves_activities (pilotpy/plot/gene_selection_analysis.py) on a small synthetic cohort.  CPU only; needs the reference
checkout (see gen_golden.py).

The reference reads Results_PILOT/cells/<cell>.csv and Results_PILOT/Markers/<cell>/Whole_expressions.csv: both are written
into a temporary directory in that layout and the fixture stores them AS READ BACK (pandas' default float parser is not always
correctly rounded).  One shim, for what this environment lacks: ``np.asfarray`` (adjust_p_values calls it) left numpy in 2.0 and
is restated as ``np.asarray(., dtype=float)``.  The genes_importance-style table comes from tests/trajfit_restatement.py (OLS,
p_val 1) with a Treat2 column that is NaN on the two-coefficient fits, so ``fillna(0)`` has work to do.

The cohort holds: all three fitted functions; genes removed by the R-squared filter alone and by the p-value filter alone; a
time point with a single cell (its std is NaN: the whole noised entry becomes 0); a gene whose noised curve is constant (all
coefficients 0: scale 0 becomes 1); more than one flat cluster at scaler_value 0.4 and 0.65 (asserted below).

Recorded: the inputs, the three frames of get_noised_curves, the clusters (complete linkage) at 0.4 and 0.65 on the noised
curves, and compute_curves_activities' frame for the 0.4 clusters."""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

import gen_golden  # noqa: E402
import trajfit_restatement as TR  # noqa: E402

SEED = 20261017
CELL = "alpha"
N_SAMPLES, N_GENES = 12, 48
THR, PTHR = 0.1, 0.05


def cohort(rng):
    """cells of one cell type over 12 samples (Time_score 1..12); sample s6 has a single cell"""
    genes = ["g%02d" % k for k in range(N_GENES)]
    per = rng.integers(8, 20, N_SAMPLES)
    per[6] = 1
    smp = np.repeat(np.arange(N_SAMPLES), per)
    t = smp + 1.0
    base = rng.uniform(1.0, 6.0, N_GENES)
    slope = rng.normal(0.0, 0.9, N_GENES)
    curv = rng.normal(0.0, 0.05, N_GENES)
    kind = rng.integers(0, 3, N_GENES)                 # 0: trend, 1: curved, 2: pure curvature
    slope[kind == 2] = 0.0
    curv[kind == 0] = 0.0
    slope[:6] = rng.normal(0.0, 0.03, 6)               # a few nearly flat genes: weak fits for the two filters to remove
    curv[:6] = 0.0
    mu = base * np.exp(slope * (t[:, None] - 6.5) / 6 + curv * ((t[:, None] - 6.5) ** 2 - 12.0))
    X = rng.poisson(mu).astype(np.float64)
    X[:, N_GENES - 1] = 0.0                            # a gene without counts (its table row is written by hand below)
    return ["s%d" % s for s in smp], t, X, genes


def main():
    rng = np.random.default_rng(SEED)
    samples, t, counts, genes = cohort(rng)
    Xn = TR.normalize_log1p(counts)
    res = [TR.best_model(t, Xn[:, g], pval_thr=1.0, kind="ols") for g in range(N_GENES - 1)]
    rows, _ = TR.table(res, genes[:-1], "Gene ID", 1.0)
    tab = pd.DataFrame(rows)
    assert "Treat2" in tab.columns and tab["Treat2"].isna().any()
    flat = {c: np.nan for c in tab.columns}
    flat.update({"Gene ID": genes[-1], "Expression pattern": "linear up", "Slope": 0.0, "Fitted function": "linear", "Intercept": 0.0,
                 "Treat": 0.0, "adjusted P-value": 0.01, "R-squared": 0.5, "mod_rsquared_adj": 0.5})
    tab = pd.concat([tab, pd.DataFrame([flat])], ignore_index=True)

    gen_golden.import_reference()
    if not hasattr(np, "asfarray"):
        np.asfarray = lambda a, dtype=float: np.asarray(a, dtype=dtype)
    import pilotpy.plot.gene_selection_analysis as GS

    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "Markers", CELL))
        os.makedirs(os.path.join(tmp, "cells"))
        tab.to_csv(os.path.join(tmp, "Markers", CELL, "Whole_expressions.csv"))
        d = pd.DataFrame(Xn, columns=genes)
        d["sampleID"] = samples
        d["Time_score"] = t.astype(np.int64)
        d.to_csv(os.path.join(tmp, "cells", CELL + ".csv"))
        tab = pd.read_csv(os.path.join(tmp, "Markers", CELL, "Whole_expressions.csv"), index_col=0)
        back = pd.read_csv(os.path.join(tmp, "cells", CELL + ".csv"), index_col=0)
        Xn = back[genes].to_numpy(dtype=np.float64)
        curves, noised, names = GS.get_noised_curves(None, CELL, "R-squared", "adjusted P-value", THR, PTHR, tmp)
        cl = {sv: GS.cluster_genes_curves(noised, "complete", "correlation", sv) for sv in (0.4, 0.65)}
        act = GS.compute_curves_activities(noised, cl[0.4].copy(), names, CELL, tmp)

    filled = tab.fillna(0)
    low_r2 = np.abs(filled["R-squared"]) < THR
    high_p = filled["adjusted P-value"] > PTHR
    sel = filled[~low_r2 & ~high_p]
    assert (low_r2 & ~high_p).any() and (high_p & ~low_r2).any(), "each filter must remove a gene on its own"
    assert set(sel["Fitted function"]) == set(TR.MODELS), set(sel["Fitted function"])
    assert list(curves.index) == list(sel["Gene ID"]) and genes[-1] in curves.index
    assert (np.bincount(t.astype(int)) == 1).any()
    g_flat = list(curves.index).index(genes[-1])
    assert np.all(noised.to_numpy()[g_flat] == 0.0)
    for sv in cl:
        assert cl[sv]["cluster"].nunique() > 1, (sv, cl[sv]["cluster"].nunique())
    print("selected %d of %d genes; clusters: %d at 0.4, %d at 0.65" % (len(sel), len(tab), cl[0.4]["cluster"].nunique(),
                                                                       cl[0.65]["cluster"].nunique()))

    tab_cols = ["Gene ID", "Expression pattern", "Slope", "Fitted function", "Intercept", "Treat", "Treat2", "adjusted P-value",
                "R-squared", "mod_rsquared_adj"]
    blob = dict(
        cell=np.asarray(CELL), thr=THR, pthr=PTHR, X=Xn, counts=counts, genes=np.array(genes), sample_ids=np.array(samples),
        cell_times=t, order_samples=np.array(["s%d" % s for s in range(N_SAMPLES)]),
        order_times=np.arange(1, N_SAMPLES + 1, dtype=np.int64),
        selected=np.array(list(curves.index)), times=names.index.to_numpy(dtype=np.float64),
        time_samples=names["sampleID"].to_numpy().astype(str),
        scaled_curves=curves.to_numpy(), scaled_noised_curves=noised.to_numpy(),
        noised_columns=np.array(list(noised.columns)).astype(str),
        clusters_040=cl[0.4]["cluster"].to_numpy(), clusters_065=cl[0.65]["cluster"].to_numpy(),
        act_index=np.array(list(act.index)),
        **{"act_" + k: act[k].to_numpy(dtype=np.float64) for k in act.columns},
    )
    for k in tab_cols:
        v = tab[k].to_numpy()
        blob["table_" + k] = v.astype(str) if v.dtype == object else v
    np.savez_compressed(os.path.join(HERE, "gene_curves_1type.npz"), **blob)
    print("wrote gene_curves_1type.npz")


if __name__ == "__main__":
    main()
