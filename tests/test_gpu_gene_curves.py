"""Gene curve clustering on the device (K11: engine.segment_std, fitted_curves, linkage_of_rows, flat_clusters,
curve_activities; tl.get_noised_curves, cluster_genes_curves, compute_curves_activities, genes_selection_analysis) against the
restatement with pandas / scipy / scikit-learn (tests/curves_restatement.py) and the reference-executed fixture
tests/golden/gene_curves_1type.npz.

Bounds.  Segment std: a segment of m rows is summed as 8 strided slices of m / 8 terms and an 8-term merge, twice (mean, squared
deviations), so the sum of squares carries about (m / 8 + 11) u relative, u = 1.1e-16: 4e-15 at m = 220, the longest segment
here, halved by the square root -- held to 1e-12 absolute on O(1) values.  Standardised curves: T-term sums, T u = 3e-14 at
T = 300, on values of at most sqrt(T): 1e-12 absolute.  Merge heights and d.max(): 1e-11 relative (a T-term sum of squares is
good to T u, halved by the root).  Z's structure, sizes and the flat labels are compared exactly where the restatement's
consecutive sorted heights differ by more than 1e-9 relative, none is within 1e-9 of the cut, AND no merge of the restatement is
ambiguous (curves_restatement.merge_margins: at every merge the next-nearest third cluster is more than 1e-9 relative farther
than the merge height); all three are computed with scipy alone and asserted for every input meant for exact comparison.  The
third condition is needed because distinct heights do not make a tree unique: the fixture's constant gene has the standardised
row 0, at distance sqrt(T) from every other row, so which cluster it joins at height sqrt(T) hangs on the last bit of the
inputs -- scipy itself renumbers the 0.4 clusters in 113 of 200 perturbations of the fixture's curves by 1e-15 and changes the
0.65 partition in the same 113, with every height unchanged.  Where a merge is ambiguous the sorted heights are compared, and
the partition (labels up to a bijection) at the cuts below the lowest ambiguous merge, where it is still determined.  The
rounded activity columns are compared exactly where no unrounded restatement value is within 1e-9 of a rounding boundary
(asserted)."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import curves_restatement as CR
import gene_curves_helpers as H
import trajfit_restatement as TR
from pilot_amd import engine, tl

pytestmark = pytest.mark.gpu

METHODS = ["complete", "average", "weighted", "single"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _standardised(seed, G, T):
    """standardised noised curves of the restatement from a synthetic table and synthetic spreads (one NaN time point)"""
    rng = np.random.default_rng(seed)
    params, names, times = CR.synthetic_table(rng, G, T)
    sd = rng.uniform(0.2, 1.5, (T, G))
    sd[T // 3] = np.nan
    return params, names, times, sd, CR.noised_curves(params, names, times, sd)


# ---- K11a -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_cells,T,n_genes", [(150, 12, 24), (5000, 60, 130), (50000, 300, 500)])
def test_segment_std_against_groupby(dtype, n_cells, T, n_genes):
    rng = np.random.default_rng(n_cells + T)
    Y, t = CR.synthetic_cells(rng, n_cells, T, n_genes, dtype)
    keep = np.ones(n_cells, dtype=bool)
    one = np.flatnonzero(t == 2.0)
    keep[one[1:]] = False                                          # time point 2 keeps a single cell
    Y, t = np.ascontiguousarray(Y[keep]), t[keep]
    times, first = np.unique(t, return_index=True)
    offsets = np.r_[first, t.size]
    _, want = CR.segment_std(Y, t)
    got = engine.segment_std(Y, offsets)
    assert got.shape == want.shape == (T, n_genes)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[1]).all() and np.isnan(got).sum() == n_genes
    err = np.nanmax(np.abs(got - want))
    print("segment_std %s cells=%d T=%d genes=%d longest segment %d: max abs err %.3e" % (np.dtype(dtype).name, n_cells, T, n_genes,
                                                                                       np.diff(offsets).max(), err))
    assert err <= 1e-12
    cols = rng.permutation(n_genes)[:max(1, n_genes // 3)].astype(np.int32)
    sub = engine.segment_std(Y, offsets, cols=cols)
    assert _same(sub, got[:, cols])
    dY = engine.DeviceMatrix.upload(Y)
    assert _same(engine.segment_std(dY, offsets), got) and _same(engine.segment_std(Y, offsets), got)
    assert _same(engine.download(engine.segment_std(dY, offsets, cols=cols, device=True)), sub)
    part = engine.segment_std(Y, offsets[3:8])                     # segments that do not start at row 0
    assert _same(part, got[3:7])


def test_segment_std_host_rows_from_an_offset():
    """segments that start at row 3 with a column selection: the host route copies rows 3..10 only and shifts the offsets, the
    DeviceMatrix route reads them in place -- the same bits, NaN for the one-row segment in both"""
    rng = np.random.default_rng(3)
    Y = rng.standard_normal((12, 9)).astype(np.float32)
    offsets, cols = [3, 5, 6, 11], [8, 0, 4]
    host = engine.segment_std(Y, offsets, cols=cols)
    dev = engine.segment_std(engine.DeviceMatrix.upload(Y), offsets, cols=cols)
    assert host.shape == (3, 3) and _same(host, dev)
    assert np.isnan(host[1]).all() and np.isfinite(host[[0, 2]]).all()
    want = np.stack([Y[3:5].astype(np.float64).std(axis=0, ddof=1), Y[6:11].astype(np.float64).std(axis=0, ddof=1)])[:, cols]
    assert np.abs(host[[0, 2]] - want).max() <= 1e-12
    assert _same(engine.download(engine.segment_std(Y, offsets, cols=cols, device=True)), host)


# ---- curves ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,T", [(1, 2), (50, 24), (2000, 120), (4000, 300)])
def test_fitted_curves_against_standard_scaler(G, T):
    params, names, times, sd, (sc, sn) = _standardised(G * 7 + T, G, T)
    got_c = engine.fitted_curves(params, names, times)
    got_n = engine.fitted_curves(params, names, times, noise=sd)
    e_c, e_n = np.abs(got_c - sc).max(), np.abs(got_n - sn).max()
    print("fitted_curves G=%d T=%d: max abs err %.3e (plain), %.3e (noised)" % (G, T, e_c, e_n))
    assert e_c <= 1e-12 and e_n <= 1e-12
    assert (got_n[:, T // 3] == sn[:, T // 3]).all() or np.abs(got_n[:, T // 3] - sn[:, T // 3]).max() <= 1e-12
    dev = engine.fitted_curves(params, names, times, noise=engine.DeviceMatrix.upload(sd), device=True)
    assert _same(engine.download(dev), got_n) and _same(engine.fitted_curves(params, names, times, noise=sd), got_n)


def test_fitted_curves_fixture():
    """the fixture's frames (reference-executed; the restatement reproduces them exactly, test_gene_curves_args.py)"""
    g = H.load()
    sel, times, sd, params, models = H.restated_inputs(g)
    got_sd = engine.segment_std(g["X"], np.r_[np.unique(g["cell_times"], return_index=True)[1], g["cell_times"].size],
                                cols=[list(g["genes"]).index(x) for x in sel["Gene ID"]])
    assert np.array_equal(np.isnan(got_sd), np.isnan(sd)) and np.nanmax(np.abs(got_sd - sd)) <= 1e-12
    got_c = engine.fitted_curves(params, models, times)
    got_n = engine.fitted_curves(params, models, times, noise=got_sd)
    assert np.abs(got_c - g["scaled_curves"]).max() <= 1e-12 and np.abs(got_n - g["scaled_noised_curves"]).max() <= 1e-12
    flat = list(g["selected"]).index(str(g["genes"][-1]))
    assert (got_n[flat] == 0.0).all() and (got_c[flat] == 0.0).all()      # scale 0 became 1


# ---- K11b -----------------------------------------------------------------------------------------------------------------------
def _labels_agree(got, want, exact, determined):
    """exactly; or as a partition where the cut lies below every ambiguous merge; or not at all (the heights are compared)"""
    if exact:
        assert np.array_equal(got, want)
    elif determined:
        assert CR.same_partition(got, want)


def _check_linkage(curves, method, cuts=(0.4, 0.65)):
    Zr, dmax_r = CR.linkage(curves, method)
    Z, dmax, info = engine.linkage_of_rows(curves, method, return_info=True)
    G = curves.shape[0]
    assert Z.shape == (G - 1, 4) and info["chain_steps"] < 4 * G
    assert abs(dmax - dmax_r) <= 1e-11 * dmax_r
    rel = np.abs(np.sort(Z[:, 2]) - np.sort(Zr[:, 2])) / np.sort(Zr[:, 2])
    assert (np.diff(Z[:, 2]) >= 0).all()
    exact, determined = CR.comparable(curves, method, cuts)
    print("linkage %s G=%d T=%d: heights rel err %.3e, d.max rel err %.3e, chain steps %d, exact comparison: %s"
          % (method, G, curves.shape[1], rel.max(), abs(dmax - dmax_r) / dmax_r, info["chain_steps"], exact))
    assert rel.max() <= 1e-11
    for c in cuts:
        want = CR.sch.fcluster(Zr, c * dmax_r, "distance")
        got = engine.flat_clusters(Z, c * dmax)
        _labels_agree(got, want, exact, c in determined)
    if exact:
        assert np.array_equal(Z[:, :2], Zr[:, :2]) and np.array_equal(Z[:, 3], Zr[:, 3])
    return Z, dmax, exact


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("G,T", [(2, 5), (3, 4), (65, 17), (300, 24), (2000, 120), (4000, 300)])
def test_linkage_against_scipy(method, G, T):
    _, _, _, _, (_, sn) = _standardised(G + T, G, T)
    Z, dmax, exact = _check_linkage(sn, method)
    if G in (300, 2000, 4000):                         # the probe sizes of the issue satisfied the condition: so must these
        assert exact
    Z2, dmax2 = engine.linkage_of_rows(engine.DeviceMatrix.upload(sn), method)
    Z3, dmax3 = engine.linkage_of_rows(sn, method)
    assert _same(Z2, Z) and _same(Z3, Z) and dmax2 == dmax == dmax3


@pytest.mark.parametrize("method", METHODS)
def test_linkage_fixture(method):
    g = H.load()
    curves = g["scaled_noised_curves"]
    nz = curves[(curves != 0).any(axis=1)]
    Z, dmax, exact = _check_linkage(np.ascontiguousarray(nz), method)
    assert exact
    # with the constant gene: its row is 0, equidistant from every other row -- the merge that takes it in is ambiguous
    Z, dmax, exact = _check_linkage(curves, method)
    if method == "complete":
        ex, determined = CR.comparable(curves, method, (0.4, 0.65))
        assert not ex and determined == [0.4]
        _labels_agree(engine.flat_clusters(Z, 0.4 * dmax), g["clusters_040"], ex, True)


def test_linkage_with_exact_ties_gives_the_same_heights_and_partition():
    """duplicate rows: zero heights and tied merges; structure may differ from scipy's, heights and partition may not"""
    rng = np.random.default_rng(3)
    base = rng.standard_normal((40, 6))
    Y = np.ascontiguousarray(np.repeat(base, 3, axis=0)[rng.permutation(120)])
    for method in METHODS:
        Zr, dmax_r = CR.linkage(Y, method)
        Z, dmax = engine.linkage_of_rows(Y, method)
        assert np.allclose(np.sort(Z[:, 2]), np.sort(Zr[:, 2]), rtol=1e-11, atol=0.0) and dmax == pytest.approx(dmax_r, rel=1e-11)
        assert (Z[:80, 2] == 0.0).all() and Z[-1, 3] == 120
        assert CR.same_partition(engine.flat_clusters(Z, 0.0), CR.sch.fcluster(Zr, 0.0, "distance"))


# ---- activities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,T", [(24, 12), (300, 24), (4000, 300)])
def test_curve_activities_against_restatement(G, T):
    _, _, times, _, (_, sn) = _standardised(G * 3 + T, G, T)
    times = np.cumsum(np.random.default_rng(T).uniform(0.5, 2.0, T))            # uneven time points
    want = CR.activities_raw(sn, times)
    margin = min(CR.rounding_margin(want[:, j]) for j in range(4))
    assert margin > 1e-9, margin
    got = engine.curve_activities(sn, times)
    print("curve_activities G=%d T=%d: max abs err %s, rounding margin %.2e" % (G, T, np.abs(got - want).max(axis=0), margin))
    assert np.array_equal(np.round(got, 2), np.round(want, 2))
    assert _same(engine.curve_activities(engine.DeviceMatrix.upload(sn), times), got) and _same(engine.curve_activities(sn, times), got)
    labels = np.ones(G, dtype=np.int64)
    frame = tl.compute_curves_activities(pd.DataFrame(sn, index=["g%d" % i for i in range(G)]),
                                         pd.DataFrame({"Gene ID": ["g%d" % i for i in range(G)], "cluster": labels}),
                                         pd.DataFrame({"sampleID": ["s"] * T}, index=pd.Index(times, name="Time_score")))
    ref = CR.activities(sn, times, labels)
    assert list(frame.columns) == list(ref)
    for k in ("Terminal_logFC", "Transient_logFC", "Switching_time", "area", "cluster"):
        assert np.array_equal(frame[k].to_numpy(dtype=np.float64), ref[k]), k
    for k in ("Terminal_pvalue", "Terminal_adjPvalue"):
        assert np.abs(frame[k].to_numpy(dtype=np.float64) - ref[k]).max() <= 1e-12, k


# ---- tl -------------------------------------------------------------------------------------------------------------------------
def _check_frames_against_fixture(g, curves, noised, names, tol=1e-12, want=None):
    want_c, want_n = (g["scaled_curves"], g["scaled_noised_curves"]) if want is None else want
    assert list(curves.index) == list(g["selected"]) == list(noised.index) and curves.index.name == "Gene ID"
    assert np.array_equal(np.asarray(curves.columns, dtype=np.float64), g["times"])
    assert list(noised.columns) == list(g["noised_columns"]) and noised.columns.name == "sampleID"
    assert np.array_equal(names.index.to_numpy(dtype=np.float64), g["times"]) and names.index.name == "Time_score"
    assert list(names["sampleID"]) == list(g["time_samples"])
    e_c, e_n = np.abs(curves.to_numpy() - want_c).max(), np.abs(noised.to_numpy() - want_n).max()
    print("tl.get_noised_curves: max abs err %.3e (curves), %.3e (noised)" % (e_c, e_n))
    assert e_c <= tol and e_n <= tol


@pytest.mark.parametrize("form", ["dense", "csr"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tl_chain_on_the_fixture(dtype, form):
    g = H.load()
    X = g["X"].astype(dtype)
    ad = H.adata(g, sp.csr_matrix(X) if form == "csr" else X)
    tab = H.table(g)
    if dtype == np.float64:
        want = None
    else:                                              # float32 cells: the restatement on the same float32 values
        sel, times, sd, params, models = H.restated_inputs(g, X=X.astype(np.float64))
        want = CR.noised_curves(params, models, times, sd)
    curves, noised, names = tl.get_noised_curves(ad, str(g["cell"]), tab, normalize=False)
    _check_frames_against_fixture(g, curves, noised, names, want=want)
    want_n = g["scaled_noised_curves"] if want is None else want[1]
    exact, determined = CR.comparable(want_n, "complete", (0.4, 0.65))
    assert not exact and determined == [0.4]           # the constant gene's merge is ambiguous (module docstring)
    for sv, key in ((0.4, "clusters_040"), (0.65, "clusters_065")):
        gc = tl.cluster_genes_curves(noised, scaler_value=sv)
        assert list(gc.columns) == ["Gene ID", "cluster"] and list(gc["Gene ID"]) == list(g["selected"])
        _labels_agree(gc["cluster"].to_numpy(), CR.clusters(want_n, "complete", sv), exact, sv in determined)
        if dtype == np.float64:
            _labels_agree(gc["cluster"].to_numpy(), g[key], exact, sv in determined)
    out = tl.genes_selection_analysis(ad, str(g["cell"]), tab, table_filter_thr=float(g["thr"]), normalize=False)
    assert sorted(out) == ["curves", "curves_activities", "genes_clusters", "noised_curves", "pseudotime_sample_names"]
    assert _same(out["noised_curves"].to_numpy(), noised.to_numpy()) and _same(out["curves"].to_numpy(), curves.to_numpy())
    _labels_agree(out["genes_clusters"]["cluster"].to_numpy(), CR.clusters(want_n, "complete", 0.4), exact, True)
    act = out["curves_activities"]
    assert list(act.index) == list(g["selected"]) and list(act.columns) == tl._ACTIVITY_COLUMNS
    raw = CR.activities_raw(want_n, g["times"])
    assert min(CR.rounding_margin(raw[:, j]) for j in range(4)) > 1e-9
    ref = CR.activities(want_n, g["times"], CR.clusters(want_n, "complete", 0.4))
    for k in ("Terminal_logFC", "Transient_logFC", "Switching_time", "area"):
        assert np.array_equal(act[k].to_numpy(dtype=np.float64), ref[k]), k
        if dtype == np.float64:
            assert np.array_equal(act[k].to_numpy(dtype=np.float64), g["act_" + k]), k
    assert np.array_equal(act["cluster"].to_numpy(), out["genes_clusters"]["cluster"].to_numpy())
    _labels_agree(act["cluster"].to_numpy(), ref["cluster"], exact, True)
    for k in ("Terminal_pvalue", "Terminal_adjPvalue"):
        assert np.abs(act[k].to_numpy(dtype=np.float64) - ref[k]).max() <= 1e-12, k
    # a separate call of the three functions on frames gives what the chained call gave, and so does a second chained call
    gc = tl.cluster_genes_curves(noised, scaler_value=0.4)
    act2 = tl.compute_curves_activities(noised, gc, names)
    assert act2.equals(act)
    again = tl.genes_selection_analysis(ad, str(g["cell"]), tab, table_filter_thr=float(g["thr"]), normalize=False)
    assert again["curves_activities"].equals(act) and _same(again["noised_curves"].to_numpy(), noised.to_numpy())


@pytest.mark.parametrize("method", METHODS)
def test_tl_clusters_exactly_without_the_constant_gene(method):
    """the fixture's table without its constant gene: no merge is ambiguous (asserted), so the cluster numbers of
    cluster_genes_curves and of the chained call are the restatement's -- which is the reference on these inputs -- exactly"""
    g = H.load()
    ad = H.adata(g)
    tab = H.table(g)
    tab = tab[tab["Gene ID"] != str(g["genes"][-1])]
    keep = g["selected"] != str(g["genes"][-1])
    want_n = g["scaled_noised_curves"][keep]                       # (each gene's curve does not depend on the other genes)
    exact, determined = CR.comparable(want_n, method, (0.4, 0.65))
    assert exact and determined == [0.4, 0.65]
    curves, noised, names = tl.get_noised_curves(ad, str(g["cell"]), tab, normalize=False)
    assert list(noised.index) == list(g["selected"][keep]) and np.abs(noised.to_numpy() - want_n).max() <= 1e-12
    for sv in (0.4, 0.65):
        want = CR.clusters(want_n, method, sv)
        gc = tl.cluster_genes_curves(noised, cluster_method=method, scaler_value=sv)
        assert np.array_equal(gc["cluster"].to_numpy(), want) and len(set(want)) > (method != "single")
        out = tl.genes_selection_analysis(ad, str(g["cell"]), tab, table_filter_thr=float(g["thr"]), cluster_method=method,
                                          scaler_value=sv, normalize=False)
        assert np.array_equal(out["genes_clusters"]["cluster"].to_numpy(), want)
        assert np.array_equal(out["curves_activities"]["cluster"].to_numpy(), want)


def test_tl_normalises_counts_like_genes_importance():
    """normalize=True from the counts: the device's normalize_total + log1p against its restatement (a few ulp apart on O(1)
    values, passed on by the spreads at a tenth: far inside 1e-12)"""
    g = H.load()
    ad = H.adata(g, g["counts"])
    Xn = TR.normalize_log1p(g["counts"])
    sel, times, sd, params, models = H.restated_inputs(g, X=Xn)
    want = CR.noised_curves(params, models, times, sd)
    curves, noised, names = tl.get_noised_curves(ad, str(g["cell"]), H.table(g))
    _check_frames_against_fixture(g, curves, noised, names, want=want)


def test_tl_without_treat2_and_filters():
    g = H.load()
    ad = H.adata(g)
    tab = H.table(g)
    two = tab[tab["Fitted function"] != "linear_quadratic"]
    a = tl.get_noised_curves(ad, str(g["cell"]), two.drop(columns="Treat2"), normalize=False)
    b = tl.get_noised_curves(ad, str(g["cell"]), two, normalize=False)
    assert a[0].equals(b[0]) and a[1].equals(b[1]) and len(a[0]) > 2
    loose = tl.get_noised_curves(ad, str(g["cell"]), tab, table_filter_thr=0.0, table_filter_pval_thr=1.0, normalize=False)
    assert len(loose[0]) == len(tab) > len(g["selected"])
    one = tab[tab["Gene ID"] == g["selected"][0]]
    out = tl.genes_selection_analysis(ad, str(g["cell"]), one, normalize=False)
    assert list(out["genes_clusters"]["cluster"]) == [1] and out["curves_activities"].shape == (1, 7)


def test_tl_chain_at_size():
    """G = 1500 selected of 2000 genes, T = 150, 20 000 float32 cells: the chained call against the restatement's chain"""
    rng = np.random.default_rng(11)
    n_genes, G, T, n_cells = 2000, 1500, 150, 20000
    Y, t = CR.synthetic_cells(rng, n_cells, T, n_genes, np.float32)
    params, names, times = CR.synthetic_table(rng, n_genes, T)
    genes = ["g%04d" % i for i in range(n_genes)]
    r2 = np.where(np.arange(n_genes) < G, 0.5, 0.01)
    order = rng.permutation(n_genes)
    tab = pd.DataFrame({"Gene ID": np.asarray(genes)[order], "Fitted function": names[order], "Intercept": params[order, 0],
                        "Treat": params[order, 1], "Treat2": np.where(names[order] == "linear_quadratic", params[order, 2], np.nan),
                        "adjusted P-value": 0.01, "R-squared": r2[order]})
    obs = pd.DataFrame({"cell_types": "c", "sampleID": ["s%d" % int(v) for v in t]})
    orders = pd.DataFrame({"sampleID": ["s%d" % v for v in range(1, T + 1)], "Time_score": np.arange(1, T + 1)})
    ad = H.Cohort(Y, obs, genes, dict(orders=orders))
    sel = CR.select(tab, thr=0.05)
    cols = [genes.index(x) for x in sel["Gene ID"]]
    _, sd = CR.segment_std(Y[:, cols].astype(np.float64), t)
    sc, sn = CR.noised_curves(sel[["Intercept", "Treat", "Treat2"]].fillna(0).to_numpy(), list(sel["Fitted function"]), times, sd)
    Zr, dmax_r = CR.linkage(sn, "complete")
    assert CR.comparable(sn, "complete", (0.4,)) == (True, [0.4])
    raw = CR.activities_raw(sn, times)
    assert min(CR.rounding_margin(raw[:, j]) for j in range(4)) > 1e-9
    out = tl.genes_selection_analysis(ad, "c", tab, normalize=False)
    assert list(out["noised_curves"].index) == list(sel["Gene ID"]) and len(sel) == G
    e_c, e_n = np.abs(out["curves"].to_numpy() - sc).max(), np.abs(out["noised_curves"].to_numpy() - sn).max()
    print("chain at size: max abs err %.3e (curves), %.3e (noised)" % (e_c, e_n))
    assert e_c <= 1e-12 and e_n <= 1e-12
    labels = CR.sch.fcluster(Zr, 0.4 * dmax_r, "distance")
    assert np.array_equal(out["genes_clusters"]["cluster"].to_numpy(), labels) and len(set(labels)) > 1
    ref = CR.activities(sn, times, labels)
    act = out["curves_activities"]
    for k in ("Terminal_logFC", "Transient_logFC", "Switching_time", "area", "cluster"):
        assert np.array_equal(act[k].to_numpy(dtype=np.float64), ref[k]), k
    for k in ("Terminal_pvalue", "Terminal_adjPvalue"):
        assert np.abs(act[k].to_numpy(dtype=np.float64) - ref[k]).max() <= 1e-12, k
