"""Patient sub-group detection on the device (K12: tl.highly_variable_genes, extract_cells_from_gene_expression_for_clustering,
compute_diff_expressions, cell_type_diff_two_sub_patient_groups) against the independent host restatement
(tests/limma_restatement.py: two-pass moments, lstsq on the explicit design, scipy's Welch test).

Cohort (tests/subgroup_helpers.py): 12 samples under 3 sub-group labels (one sample carries the third), about 4 000 cells of the
cell type and 400 beyond it, 400 genes of log1p-scale float32 values, 40 genes shifted between the two groups compared, gene 3
constant 0.  Bounds: logFC and AveExpr are means of at most 4 000 float64 terms in a fixed chunked order (test_gpu_group_moments:
a few hundred u) and are held to 1e-11 relative; the prior (df_prior, s2_prior) and t pass through log, digamma and a Newton
iteration stopped at 1e-8 of a quadratically convergent step, and are held to 1e-9 relative; p-values are held to 1e-8 relative
wherever the restatement's exceeds 1e-300, below which both sides must be 0 or denormal-small alike (<= 1e-300).  Relative
bounds on a difference of means (a two-group logFC) and on a logarithm (an HVG dispersion) only mean something away from 0, so
the seeds are chosen, and it is asserted on the restatement alone, that no logFC lies within 1e-4 of 0 without being 0 and no
dispersion within 0.05 of 0."""
import functools

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import limma_restatement as LR
import subgroup_helpers as S
import trajfit_restatement as TR
from pilot_amd import engine, tl

pytestmark = pytest.mark.gpu

G1, G2 = S.GROUPS[0], S.GROUPS[1]
COHORT_SEED = 19               # a seed at which no gene's two-group logFC is nearly 0 (asserted below)
EQUAL_VARIANCE_SEED = 2        # a seed at which the restatement's evar <= 0 (asserted below)


@functools.lru_cache(maxsize=None)
def _cohort(equal_variance=False):
    adata, props, lab = S.cohort(seed=EQUAL_VARIANCE_SEED if equal_variance else COHORT_SEED, equal_variance=equal_variance)
    values, rows = S.cell_values(adata)
    return adata, props, values, lab[rows]


@functools.lru_cache(maxsize=None)
def _restated(design, equal_variance=False):
    _, _, values, lab = _cohort(equal_variance)
    return LR.diff_expressions(values, lab, G1, G2, design)


@functools.lru_cache(maxsize=None)
def _restated_hvg(n_top):
    return LR.highly_variable_genes(_cohort()[2], n_top)


def _rel(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got - want)[ok]
    scale = np.abs(want)[ok]
    worst = float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), err), initial=0.0))
    print("%s: max rel err %.3e (tol %g)" % (what, worst, tol))
    assert worst <= tol, what


def _check_table(res, want, genes, what):
    assert list(res.columns) == ["logFC", "AveExpr", "t", "P.Value", "adj.P.Val"] and list(res.index) == list(genes)
    _rel(res["logFC"], want["logFC"], 1e-11, what + " logFC")
    _rel(res["AveExpr"], want["AveExpr"], 1e-11, what + " AveExpr")
    if np.isinf(want["df_prior"]):
        assert np.isinf(res.attrs["df_prior"])
    else:
        _rel(res.attrs["df_prior"], want["df_prior"], 1e-9, what + " df_prior")
    _rel(res.attrs["s2_prior"], want["s2_prior"], 1e-9, what + " s2_prior")
    _rel(res["t"], want["t"], 1e-9, what + " t")
    for col in ("P.Value", "adj.P.Val"):
        big = want[col] > 1e-300
        _rel(res[col].values[big], want[col][big], 1e-8, what + " " + col)
        assert (res[col].values[~big] <= 1e-300).all()


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
@pytest.mark.parametrize("design", ["reference", "two_group"])
def test_designs_against_restatement(design, sparse):
    adata, props, values, lab = _cohort()
    want = _restated(design)
    assert np.isfinite(want["df_prior"]) and (want["adj.P.Val"] < 0.01).sum() >= 30 and want["t"][3] == 0.0
    # a logFC is a difference of two means of size <= 4, each good to a few u: 1e-11 relative needs |logFC| >= 1e-4 (or exactly 0)
    assert np.abs(want["logFC"][want["logFC"] != 0]).min() > 1e-4 and np.abs(want["AveExpr"]).max() < 4.0
    ad = S.Cohort(sp.csr_matrix(adata.X), adata.obs, adata.var_names) if sparse else adata
    res = tl.compute_diff_expressions(ad, S.CELL, props, highly_variable_genes_=False, design=design)
    _check_table(res, want, adata.var_names, design)
    if design == "two_group":                                      # positive = higher in group1; swapping the groups flips the sign
        m1, m2 = values[lab == G1].astype(np.float64).mean(axis=0), values[lab == G2].astype(np.float64).mean(axis=0)
        assert (np.sign(res["logFC"].values) == np.sign(m1 - m2)).all()
        back = tl.compute_diff_expressions(ad, S.CELL, props, group1=G2, group2=G1, highly_variable_genes_=False, design=design)
        assert np.array_equal(back["logFC"].values, -res["logFC"].values) and np.array_equal(back["P.Value"].values, res["P.Value"].values)
    else:                                                          # x follows the names' order, not the argument order
        back = tl.compute_diff_expressions(ad, S.CELL, props, group1=G2, group2=G1, highly_variable_genes_=False, design=design)
        assert np.array_equal(back["logFC"].values, res["logFC"].values)


def test_cells_left_out_lie_on_another_scale(design="two_group"):
    """the cells a call leaves out -- the other cell types, and within the cell type the patients of neither group -- hold values
    1e6 times the others' (raw counts beside log1p values): the table is the restatement's on the same matrix within the bounds
    above.  The other cell types never reach the device; the third label's cells do, as skipped rows of K12, and two of the 30
    row slices the host makes of these 3 963 cells (n // 128 on any device of 8 or more CUs, the rule restated in
    tests/test_gpu_group_moments.py) begin with one."""
    adata, props, _, _ = _cohort()
    lab = S.cohort(seed=COHORT_SEED)[2]
    rows = S.cell_values(adata)[1]
    out = np.asarray(adata.obs["cell_types"]) != S.CELL
    out |= (lab != G1) & (lab != G2)
    X = adata.X.copy()
    X[out] *= np.float32(1e6)
    scaled = S.Cohort(X, adata.obs, adata.var_names)
    n, skipped = rows.size, out[rows]
    starts = [n // (n // 128) * s + n % (n // 128) * s // (n // 128) for s in range(n // 128)]
    assert out.sum() > 600 and skipped.sum() > 300 and skipped[starts].sum() >= 2
    assert np.isfinite(X).all() and X[out].max() >= 1e5 * X[~out].max() and np.array_equal(X[~out], adata.X[~out])
    want = LR.diff_expressions(X[rows], lab[rows], G1, G2, design)
    assert all(np.array_equal(want[k], _restated(design)[k]) for k in ("logFC", "t"))     # the restatement never sees those cells
    res = tl.compute_diff_expressions(scaled, S.CELL, props, highly_variable_genes_=False, design=design)
    _check_table(res, want, adata.var_names, design + ", cells left out scaled by 1e6")


@pytest.mark.parametrize("id_column", ["sampleID", None])
def test_sample_ids_from_the_other_places(id_column):
    adata, props, _, _ = _cohort()
    props = props.rename(columns={"sampIeD": id_column}) if id_column else props.set_index("sampIeD")
    res = tl.compute_diff_expressions(adata, S.CELL, props.sample(frac=1.0, random_state=1), highly_variable_genes_=False)
    _check_table(res, _restated("reference"), adata.var_names, "ids from %s" % (id_column or "the index"))


@pytest.mark.parametrize("design", ["reference", "two_group"])
def test_infinite_prior(design):
    """every gene has the same true variance: the restatement's evar is <= 0 at this seed, so df0 = inf and s2_post = s0^2"""
    adata, props, _, _ = _cohort(True)
    want = _restated(design, True)
    assert np.isinf(want["df_prior"])
    res = tl.compute_diff_expressions(adata, S.CELL, props, highly_variable_genes_=False, design=design)
    _check_table(res, want, adata.var_names, design + ", df0 = inf")


def test_highly_variable_genes():
    adata, _, values, _ = _cohort()
    want = _restated_hvg(120)
    dn = want["dispersions_norm"].values
    assert np.isnan(dn[3]) and 100 <= want["highly_variable"].sum() <= 125
    assert np.nanmin(np.abs(want["dispersions"].values)) > 0.05    # log(var / mean) is compared relatively: none near 0
    assert np.nanmin(np.abs(dn - want.attrs["cutoff"])[dn != want.attrs["cutoff"]]) > 1e-9      # nothing else near the cut-off
    assert np.abs(np.nan_to_num(dn)[np.isnan(dn)] - want.attrs["cutoff"]).min(initial=1.0) > 1e-9
    got = tl.highly_variable_genes(np.ascontiguousarray(values), 120)
    assert list(got.columns) == ["means", "dispersions", "dispersions_norm", "highly_variable"] and len(got) == values.shape[1]
    _rel(got["means"], want["means"], 1e-11, "HVG means")
    _rel(got["dispersions"], want["dispersions"], 1e-11, "HVG dispersions")
    assert np.array_equal(got["highly_variable"].values, want["highly_variable"].values)
    on_device = tl.highly_variable_genes(engine.DeviceMatrix.upload(values), 120)
    assert on_device.equals(got)


def test_more_top_genes_than_finite_dispersions():
    _, _, values, _ = _cohort()
    want = _restated_hvg(5000)
    finite = ~np.isnan(want["dispersions_norm"].values)
    assert finite.sum() < values.shape[1] < 5000
    got = tl.highly_variable_genes(np.ascontiguousarray(values), 5000)
    assert np.array_equal(got["highly_variable"].values, want["highly_variable"].values) and got["highly_variable"].values[finite].all()


def test_diff_expressions_over_the_highly_variable_genes():
    adata, props, values, lab = _cohort()
    keep = np.flatnonzero(_restated_hvg(120)["highly_variable"].values)
    genes = np.asarray(adata.var_names)[keep]
    want = LR.diff_expressions(values[:, keep], lab, G1, G2, "two_group")
    res = tl.compute_diff_expressions(adata, S.CELL, props, n_top_genes=120, design="two_group")
    _check_table(res, want, genes, "over 120 HVGs")
    pick = [genes[40], genes[2], genes[77]]                         # selected_genes: their order, their own prior
    sub = tl.compute_diff_expressions(adata, S.CELL, props, selected_genes=pick, n_top_genes=120, design="two_group")
    _check_table(sub, LR.diff_expressions(values[:, keep[[40, 2, 77]]], lab, G1, G2, "two_group"), pick, "three selected genes")
    outside = [g for g in adata.var_names if g not in set(genes)][0]
    with pytest.raises(KeyError):
        tl.compute_diff_expressions(adata, S.CELL, props, selected_genes=[outside], n_top_genes=120)


def test_extract_cells_frame():
    adata, _, values, _ = _cohort()
    rows = S.cell_values(adata)[1]
    samples = list(np.asarray(adata.obs["sampleID"])[rows])
    plain = tl.extract_cells_from_gene_expression_for_clustering(adata, "sampleID", "cell_types", [S.CELL, "beta"], normalization=False)
    assert list(plain.columns) == list(adata.var_names) + ["sampleID"] and list(plain["sampleID"]) == samples
    assert np.array_equal(plain[list(adata.var_names)].to_numpy(), values)
    keep = np.flatnonzero(_restated_hvg(120)["highly_variable"].values)
    hv = tl.extract_cells_from_gene_expression_for_clustering(adata, "sampleID", "cell_types", [S.CELL], normalization=False,
                                                               n_top_genes=120, highly_variable_genes_=True)
    assert list(hv.columns) == [adata.var_names[j] for j in keep] + ["sampleID"]
    assert np.array_equal(hv.drop(columns="sampleID").to_numpy(), values[:, keep]) and list(hv["sampleID"]) == samples
    # normalised: float32 roundings of a float64 evaluation, held to two float32 ulps of the restated values
    counts = S.Cohort(np.expm1(adata.X.astype(np.float64)).round().astype(np.float32), adata.obs, adata.var_names)
    normed = tl.extract_cells_from_gene_expression_for_clustering(counts, "sampleID", "cell_types", [S.CELL])
    restated = TR.normalize_log1p(counts.X[rows])
    got = normed.drop(columns="sampleID").to_numpy()
    assert got.dtype == np.float32 and np.abs(got - restated).max() <= 2.4e-7 * np.abs(restated).max()
    assert (got[:, 3] == 0).all()


def test_cell_type_diff_two_sub_patient_groups():
    rng = np.random.default_rng(6)
    types = ["ct%d" % k for k in range(9)]
    P = rng.dirichlet(np.full(9, 3.0), 30)
    lab = np.array([G1] * 13 + [G2] * 12 + [S.GROUPS[2]] * 5, dtype=object)
    P[lab == G2, :3] *= 1.6
    P /= P.sum(axis=1, keepdims=True)
    frame = pd.DataFrame(P, columns=types)
    frame["Predicted_Labels"] = lab
    frame = frame.sample(frac=1.0, random_state=3).reset_index(drop=True)
    want = LR.welch_table(frame, types, "Predicted_Labels", G1, G2)
    assert np.diff(np.sort(want["score"].values)).min() > 1e-6 and (want["adjPval"] < 0.05).any()
    got = tl.cell_type_diff_two_sub_patient_groups(frame, types, group1=G1, group2=G2)
    assert list(got.columns) == ["cell_type", "adjPval", "-logPval", "score"]
    assert list(got["cell_type"]) == list(want["cell_type"]) and list(got.index) == list(want.index)
    _rel(got["score"], want["score"], 1e-11, "Welch score")
    _rel(got["adjPval"], want["adjPval"], 1e-9, "Welch adjPval")
    _rel(got["-logPval"], want["-logPval"], 1e-9, "Welch -logPval")
