"""K21 on the device: engine.rank_sums (rs_dense_scan_kernel, rs_csr_scan_kernel, rs_rank_kernel) against scipy.stats.rankdata and
np.unique column by column (tests/rank_sums_restatement.py), and what tl builds on it against scipy.stats.mannwhitneyu / kruskal.

The rule is integer, so count, rank_sums and ties must EQUAL the restatement, with no tolerance, by four routes that must also
equal one another: a dense float32 array, the same values as float64, and a DeviceCSR of each.  Every matrix is made in float32
and widened, so the two precisions order and tie alike.  The float64 tail (z, U, H, p) is held to rtol = 1e-12: the expressions
agree with scipy bit for bit on the CPU, the margin only frees the order of operations.

w, W, T = pilot_ot_rank_sums_wave_max(), _wg_max(), _sort_tile(): the bin ladder puts a column on either side of each."""
import functools

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
from scipy import stats

import rank_sums_restatement as RR
import subgroup_helpers as S
from pilot_amd import engine, tl

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)


def _routes(Y32, sparse_forms=None):
    """name -> what engine.rank_sums takes.  sparse_forms: name -> scipy CSR of Y32 to upload besides the canonical one."""
    out = {}
    for dt in DTYPES:
        Y = np.ascontiguousarray(Y32, dtype=dt)
        out["dense %s" % np.dtype(dt).name] = Y
        out["csr %s" % np.dtype(dt).name] = engine.DeviceCSR.upload(sp.csr_matrix(Y))
        for name, M in (sparse_forms or {}).items():
            out["csr %s %s" % (np.dtype(dt).name, name)] = engine.DeviceCSR.upload(M.astype(dt))
    return out


def _exact(Y32, codes, n_groups, cols=None, sparse_forms=None, what=""):
    assert Y32.dtype == np.float32
    want = RR.rank_sums(Y32.astype(np.float64), codes, n_groups, cols)
    for name, route in _routes(Y32, sparse_forms).items():
        got = engine.rank_sums(route, codes, n_groups, cols=cols)
        assert [a.dtype for a in got] == [np.int64, np.float64, np.int64], (what, name)
        for a, b, part in zip(got, want, ("count", "rank_sums", "ties")):
            np.testing.assert_array_equal(a, b, err_msg="%s, %s: %s differs from the restatement" % (what, name, part))
    return want


def _codes(rng, n, n_groups, unused=0.2, empty=None):
    codes = rng.integers(0, n_groups, n)
    if empty is not None:
        codes[codes == empty] = (empty + 1) % n_groups
    codes[rng.random(n) < unused] = -1
    return codes


def test_heavy_ties():
    rng = np.random.default_rng(1)
    Y = rng.poisson(0.7, (300, 40)).astype(np.float32)
    codes = _codes(rng, 300, 5, empty=3)
    count, R, ties = _exact(Y, codes, 5, what="Poisson(0.7)")
    assert count[3] == 0 and (R[3] == 0).all() and (ties > 0).all()


def _with_stored_zeros(Y32, rng):
    """a CSR of Y32 that also stores some of its zeros, as 0.0 and as -0.0"""
    mask = (Y32 != 0) | ((Y32 == 0) & (rng.random(Y32.shape) < 0.5))
    M = sp.csr_matrix(mask.astype(np.float32))
    r, c = M.nonzero()
    data = Y32[r, c].copy()
    zero = np.flatnonzero(data == 0)
    assert zero.size > 20
    data[zero[::2]] = -0.0
    M.data[:] = data
    assert (M.data == 0).sum() == zero.size and np.signbit(M.data[M.data == 0]).any()
    return M


def _unsorted(M):
    """the same matrix with every row's entries stored in reverse column order"""
    indices, data = M.indices.copy(), M.data.copy()
    for i in range(M.shape[0]):
        a, b = M.indptr[i], M.indptr[i + 1]
        indices[a:b], data[a:b] = indices[a:b][::-1].copy(), data[a:b][::-1].copy()
    U = sp.csr_matrix((data, indices, M.indptr.copy()), shape=M.shape)
    assert not U.has_sorted_indices
    return U


def test_negatives_and_zeros_mid_order():
    rng = np.random.default_rng(2)
    Y = np.round(rng.standard_normal((300, 40)), 1).astype(np.float32)
    Y[rng.random(Y.shape) < 0.3] = 0.0
    Y[5, 7] = -0.0                                                  # a dense -0.0 ties with the zeros too
    assert (Y < 0).any(axis=0).all() and (Y == 0).any(axis=0).all() and (Y > 0).any(axis=0).all()
    codes = _codes(rng, 300, 4)
    stored = _with_stored_zeros(Y, rng)
    _exact(Y, codes, 4, sparse_forms={"stored zeros": stored, "unsorted": _unsorted(stored)}, what="rounded normals")


def test_edge_columns():
    rng = np.random.default_rng(3)
    n = 257
    Y = np.zeros((n, 5), dtype=np.float32)
    Y[:, 1] = 3.0                                                   # all equal, every entry stored in the CSR
    Y[100, 2] = -2.5                                                # a single non-zero
    Y[:, 3] = rng.permutation(n) - 40.0                             # every value distinct (one of them 0)
    Y[:, 4] = rng.permutation(n) + 1.0                              # distinct and no zero
    codes = _codes(rng, n, 3, unused=0.1)
    codes[100] = 0                                                  # the single non-zero sits in a used row
    count, R, ties = _exact(Y, codes, 3, what="edge columns")
    N = int(count.sum())
    assert ties[0] == ties[1] == N ** 3 - N and ties[3] == ties[4] == 0
    np.testing.assert_array_equal(R[:, 0], count * (N + 1) / 2)
    np.testing.assert_array_equal(R[:, 0], R[:, 1])
    z, U = engine.rank_sum_z(count, R, ties, tie_correct=True)
    assert (z[:, :2] == 0).all()
    H, p, df = engine.kruskal_h(count, R, ties)
    assert np.isnan(H[:2]).all() and np.isnan(p[:2]).all() and np.isfinite(H[2:]).all() and df == 2


def test_bin_ladder():
    """Columns with exactly L non-zero used entries for L on either side of every bin limit, the values 1..9 so that runs of
    equal values cross every tile and run boundary.  N = 2W + 2 used rows; five unused rows lie among them and hold non-zero
    values in the long columns.  One more column has W + 1 entries of both signs."""
    w, W, T = engine.rank_sums_limits()
    assert 2 <= w < W and T >= 2 and W & (W - 1) == 0 and T & (T - 1) == 0
    rng = np.random.default_rng(4)
    N, unused = 2 * W + 2, 5
    n = N + unused
    codes = rng.integers(0, 7, n)
    skipped = rng.choice(n, unused, replace=False)
    codes[skipped] = -1
    used = np.flatnonzero(codes >= 0)
    lengths = [0, 1, 2, w - 1, w, w + 1, W - 1, W, W + 1, max(W, T) + 1, 2 * W + 1, N]
    Y = np.zeros((n, len(lengths) + 1), dtype=np.float32)
    for j, L in enumerate(lengths + [W + 1]):
        rows = rng.choice(used, L, replace=False)
        Y[rows, j] = rng.integers(1, 10, L)
        if L > W:
            Y[skipped, j] = rng.integers(1, 10, unused)
    Y[Y[:, -1] != 0, -1] *= rng.choice([-1.0, 1.0], int((Y[:, -1] != 0).sum()))
    assert [int((Y[used, j] != 0).sum()) for j in range(len(lengths))] == lengths
    count, R, ties = _exact(Y, codes, 7, what="bin ladder")
    np.testing.assert_array_equal(R.sum(axis=0), np.full(Y.shape[1], N * (N + 1) / 2))


def test_invariants():
    rng = np.random.default_rng(5)
    Y = np.round(rng.standard_normal((2048, 6)) * 2).astype(np.float32)
    for n_groups, codes in ((1, np.zeros(2048, dtype=np.int64)), (1024, rng.permutation(2048) % 1024), (1024, rng.integers(0, 1024, 2048))):
        count, R, ties = _exact(Y, codes, n_groups, what="n_groups=%d" % n_groups)
        N = 2048
        assert count.sum() == N
        np.testing.assert_array_equal(R.sum(axis=0), np.full(6, N * (N + 1) / 2))
    codes = np.where(np.arange(2048) == 77, 1, 0)                   # a group of one row
    codes[::3] = -1
    codes[77] = 1
    count, R, ties = _exact(Y, codes, 2, what="a group of one")
    N = int(count.sum())
    assert count[1] == 1
    np.testing.assert_array_equal(R.sum(axis=0), np.full(6, N * (N + 1) / 2))


def test_column_selection_windows_and_repeats():
    rng = np.random.default_rng(6)
    n, G = 500, 30
    Y = rng.poisson(1.5, (n, G)).astype(np.float32) * rng.choice([-1.0, 1.0, 1.0], (n, G)).astype(np.float32)
    codes = _codes(rng, n, 6)
    cols = rng.permutation(G)[:17]
    want = _exact(Y, codes, 6, cols=cols, what="a shuffled subset")
    full = RR.rank_sums(Y, codes, 6)
    np.testing.assert_array_equal(want[1], full[1][:, cols])
    for dt in DTYPES:
        wide = np.full((n, G + 5), 7.0, dtype=dt)                   # the columns beside the window must stay out
        wide[:, 3:3 + G] = Y
        window = engine.device_columns(engine.DeviceMatrix.upload(wide), 3, 3 + G)
        for c, ref in ((None, full), (cols, want)):
            first = engine.rank_sums(window, codes, 6, cols=c)
            again = engine.rank_sums(window, codes, 6, cols=c)
            for a, b, r in zip(first, again, ref):
                np.testing.assert_array_equal(a, r)
                np.testing.assert_array_equal(a, b)
    S_ = engine.DeviceCSR.upload(sp.csr_matrix(Y))
    for a, b in zip(S_.rank_sums(codes, 6, cols=cols), S_.rank_sums(codes, 6, cols=cols)):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_values(bad):
    rng = np.random.default_rng(7)
    n, G = 200, 12
    Y = rng.poisson(1.0, (n, G)).astype(np.float32)
    codes = _codes(rng, n, 3)
    codes[[20, 150]] = 1
    codes[[10, 30]] = -1
    cols = np.array([9, 2, 5, 7])
    quiet = Y.copy()
    quiet[10, 5] = quiet[30, 2] = bad                              # an unused row of selected columns
    quiet[20, 3] = bad                                             # a used row of a column that is not selected
    loud = quiet.copy()
    loud[150, 2] = loud[20, 5] = loud[20, 2] = bad                 # first: position 1 of cols (column 2), then the lowest row
    for dt in DTYPES:
        for make in (lambda A: A, lambda A: engine.DeviceCSR.upload(sp.csr_matrix(A))):
            got = engine.rank_sums(make(quiet.astype(dt)), codes, 3, cols=cols)
            want = RR.rank_sums(np.where(np.isfinite(quiet), quiet, 0.0), codes, 3, cols)
            for a, b in zip(got, want):
                np.testing.assert_array_equal(a, b)
            with pytest.raises(ValueError, match=r"Y\[20, 2\]"):
                engine.rank_sums(make(loud.astype(dt)), codes, 3, cols=cols)


# ---- tl.rank_genes_groups ---------------------------------------------------------------------------------------------------------
class _Adata:
    def __init__(self, X, obs, var_names):
        self.X, self.obs, self.var_names, self.uns = X, obs, var_names, {}


@functools.lru_cache(maxsize=None)
def _clusters():
    """600 cells x 50 genes of log1p Poisson counts, 4 clusters; gene 10 + k is planted in cluster k, gene 49 copies gene 48"""
    rng = np.random.default_rng(8)
    cluster = rng.integers(0, 4, 600)
    lam = np.tile(rng.uniform(0.3, 2.0, 50), (600, 1))
    for k in range(4):
        lam[cluster == k, 10 + k] = 12.0
    X = np.log1p(rng.poisson(lam)).astype(np.float32)
    X[:, 49] = X[:, 48]
    X.setflags(write=False)
    return X, cluster


def _adata(sparse):
    X, cluster = _clusters()
    obs = pd.DataFrame({"cluster": pd.Categorical([str(k) for k in cluster])})
    return _Adata(sp.csr_matrix(X) if sparse else X, obs, ["g%02d" % j for j in range(50)])


def _by_gene(frame, group):
    sub = frame[frame["group"] == group]
    assert len(sub) == 50
    return sub.set_index("names").loc[["g%02d" % j for j in range(50)]]


@pytest.mark.parametrize("sparse", [False, True])
def test_rank_genes_groups_against_scipy(sparse):
    X, cluster = _clusters()
    X64 = X.astype(np.float64)
    ad = _adata(sparse)
    corrected = tl.rank_genes_groups(ad, "cluster", tie_correct=True, key_added="corrected")
    plain = tl.rank_genes_groups(ad, "cluster")
    assert list(plain.columns) == ["group", "names", "scores", "pvals", "pvals_adj", "logfoldchanges"]
    count, R, ties = RR.rank_sums(X64, cluster, 4)
    z = RR.z_scores(count, R, ties, False)
    for k in range(4):
        inside = cluster == k
        want_p = np.array([stats.mannwhitneyu(X64[inside, j], X64[~inside, j], use_continuity=False, method="asymptotic").pvalue
                           for j in range(50)])
        got = _by_gene(corrected, str(k))
        np.testing.assert_allclose(got["pvals"].values, want_p, rtol=1e-12, atol=0)
        got = _by_gene(plain, str(k))
        np.testing.assert_allclose(got["pvals"].values, 2.0 * stats.norm.sf(np.abs(z[k])), rtol=1e-12, atol=0)
        np.testing.assert_allclose(got["scores"].values, z[k], rtol=1e-6, atol=0)
        assert got["scores"].values.dtype == np.float32
        mean_in, mean_out = X64[inside].mean(axis=0), X64[~inside].mean(axis=0)
        want_lfc = np.log2((np.expm1(mean_in) + 1e-9) / (np.expm1(mean_out) + 1e-9))
        np.testing.assert_allclose(got["logfoldchanges"].values, want_lfc, rtol=1e-6, atol=0)
        m = 50
        p_sorted = np.sort(want_p)                                  # Benjamini-Hochberg by hand on scipy's p-values
        bh = np.minimum(np.minimum.accumulate((p_sorted * m / np.arange(1, m + 1))[::-1])[::-1], 1.0)
        np.testing.assert_allclose(np.sort(_by_gene(corrected, str(k))["pvals_adj"].values), bh, rtol=1e-12, atol=0)
        # the order rule: descending score, equal scores in gene order; the planted gene first
        sub = plain[plain["group"] == str(k)]
        assert sub["names"].iloc[0] == "g%02d" % (10 + k)
        s = sub["scores"].values
        assert (s[:-1] >= s[1:]).all()
        where = list(sub["names"])
        assert where.index("g49") == where.index("g48") + 1        # equal columns, equal scores: gene order decides


def test_rank_genes_groups_reference_group_and_layout():
    X, cluster = _clusters()
    X64 = X.astype(np.float64)
    ad = _adata(True)
    frame = tl.rank_genes_groups(ad, "cluster", groups=["2", "0", "3"], reference="3", n_genes=7, tie_correct=True,
                                 corr_method="bonferroni")
    res = ad.uns["rank_genes_groups"]
    assert res["params"] == {"groupby": "cluster", "reference": "3", "method": "wilcoxon", "use_raw": False, "layer": None,
                             "corr_method": "bonferroni", "tie_correct": True}
    kinds = {"names": np.dtype("O"), "scores": np.float32, "pvals": np.float64, "pvals_adj": np.float64, "logfoldchanges": np.float32}
    assert set(res) == set(kinds) | {"params"}
    for key, kind in kinds.items():
        assert res[key].dtype.names == ("2", "0") and res[key].shape == (7,), key
        assert all(res[key].dtype[f] == kind for f in ("2", "0")), key
    assert len(frame) == 14 and list(frame["group"]) == ["2"] * 7 + ["0"] * 7
    for k in (2, 0):
        a, b = X64[cluster == k], X64[cluster == 3]
        names = list(res["names"][str(k)])
        assert names[0] == "g%02d" % (10 + k)
        j = [int(name[1:]) for name in names]
        want = np.array([stats.mannwhitneyu(a[:, c], b[:, c], use_continuity=False, method="asymptotic").pvalue for c in j])
        np.testing.assert_allclose(res["pvals"][str(k)], want, rtol=1e-12, atol=0)
        np.testing.assert_allclose(res["pvals_adj"][str(k)], np.minimum(want * 50, 1.0), rtol=1e-12, atol=0)
        np.testing.assert_array_equal(frame[frame["group"] == str(k)]["pvals"].values, res["pvals"][str(k)])
        want_lfc = np.log2((np.expm1(a.mean(axis=0)) + 1e-9) / (np.expm1(b.mean(axis=0)) + 1e-9))[j]
        np.testing.assert_allclose(res["logfoldchanges"][str(k)], want_lfc, rtol=1e-6, atol=0)
    # the last gene of g13's own cluster against it: the most negative score
    last = tl.rank_genes_groups(ad, "cluster", groups=["0"], reference="3", key_added="other")
    assert "other" in ad.uns and last["names"].iloc[-1] == "g13" and last["scores"].iloc[-1] < -10


# ---- the sub-group tests ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cohort():
    return S.cohort(seed=3, n_cells=1500, n_genes=80, n_shifted=10)


def _sparse_twin(adata):
    return S.Cohort(sp.csr_matrix(adata.X), adata.obs, adata.var_names)


@pytest.mark.parametrize("sparse", [False, True])
def test_wilcoxon_diff_expressions_against_scipy(sparse):
    adata, props, lab = _cohort()
    values, rows = S.cell_values(adata)
    values, lab = values.astype(np.float64), lab[rows]
    a, b = values[lab == S.GROUPS[0]], values[lab == S.GROUPS[1]]
    res = tl.wilcoxon_diff_expressions(_sparse_twin(adata) if sparse else adata, S.CELL, props, highly_variable_genes_=False)
    assert list(res.columns) == ["logFC", "AveExpr", "U", "z", "P.Value", "adj.P.Val"] and list(res.index) == list(adata.var_names)
    live = [j for j in range(80) if j != 3]
    want = [stats.mannwhitneyu(a[:, j], b[:, j], use_continuity=False, method="asymptotic") for j in live]
    np.testing.assert_array_equal(res["U"].values[live], [r.statistic for r in want])
    np.testing.assert_allclose(res["P.Value"].values[live], [r.pvalue for r in want], rtol=1e-12, atol=0)
    assert res["z"].values[3] == 0 and res["P.Value"].values[3] == 1           # the constant gene
    n1, n2 = len(a), len(b)
    mu, N = n1 * n2 / 2.0, n1 + n2
    for j in live[:10]:                                             # z restated from scipy's U and rankdata's ties
        t = np.unique(np.concatenate([a[:, j], b[:, j]]), return_counts=True)[1].astype(np.float64)
        s = np.sqrt(n1 * n2 / 12.0 * ((N + 1) - (t ** 3 - t).sum() / (N * (N - 1))))
        np.testing.assert_allclose(res["z"].values[j], (res["U"].values[j] - mu) / s, rtol=1e-12, atol=0)
    np.testing.assert_allclose(res["logFC"].values, a.mean(axis=0) - b.mean(axis=0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(res["AveExpr"].values, np.concatenate([a, b]).mean(axis=0), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(res["adj.P.Val"].values, tl._bh_adjust(res["P.Value"].values), rtol=0, atol=0)
    plain = tl.wilcoxon_diff_expressions(adata, S.CELL, props, highly_variable_genes_=False, tie_correct=False,
                                         selected_genes=["g010", "g002"])
    assert list(plain.index) == ["g010", "g002"]
    assert (np.abs(plain["z"].values) < np.abs(res["z"].loc[["g010", "g002"]].values)).all()      # no tie term: a larger variance


@pytest.mark.parametrize("sparse", [False, True])
def test_kruskal_diff_expressions_against_scipy(sparse):
    adata, props, lab = _cohort()
    values, rows = S.cell_values(adata)
    values, lab = values.astype(np.float64), lab[rows]
    parts = [values[lab == g] for g in S.GROUPS]
    res = tl.kruskal_diff_expressions(_sparse_twin(adata) if sparse else adata, S.CELL, props, highly_variable_genes_=False)
    assert list(res.columns) == ["H", "df", "P.Value", "adj.P.Val"] + ["mean(%s)" % g for g in S.GROUPS]
    live = [j for j in range(80) if j != 3]
    want = [stats.kruskal(*(p[:, j] for p in parts)) for j in live]
    np.testing.assert_allclose(res["H"].values[live], [r.statistic for r in want], rtol=1e-12, atol=0)
    np.testing.assert_allclose(res["P.Value"].values[live], [r.pvalue for r in want], rtol=1e-12, atol=0)
    assert (res["df"] == 2).all() and np.isnan(res["H"].values[3]) and np.isnan(res["adj.P.Val"].values[3])
    np.testing.assert_array_equal(res["adj.P.Val"].values[live], tl._bh_adjust(res["P.Value"].values[live]))
    for g, p in zip(S.GROUPS, parts):
        np.testing.assert_allclose(res["mean(%s)" % g].values, p.mean(axis=0), rtol=1e-12, atol=1e-15)
    two = tl.kruskal_diff_expressions(adata, S.CELL, props, groups=[S.GROUPS[2], S.GROUPS[0]], highly_variable_genes_=False)
    want = [stats.kruskal(parts[2][:, j], parts[0][:, j]) for j in live]
    np.testing.assert_allclose(two["H"].values[live], [r.statistic for r in want], rtol=1e-12, atol=0)
    assert (two["df"] == 1).all() and list(two.columns[-2:]) == ["mean(%s)" % S.GROUPS[2], "mean(%s)" % S.GROUPS[0]]


def _diff_expressions_as_before(adata, props, n_top_genes):
    """compute_diff_expressions(design='reference', group1 = GROUPS[0], group2 = GROUPS[1]) step by step as its body read before
    the selection was factored out"""
    genes = np.asarray(list(adata.var_names), dtype=object)
    label_of = tl._sample_labels(props, "Predicted_Labels")
    rows = tl._cell_type_rows(adata, "cell_types", S.CELL)
    samples = np.asarray(adata.obs["sampleID"])[rows]
    labels = np.asarray([label_of[s] for s in samples], dtype=object)
    codes = np.where(labels == S.GROUPS[0], 0, np.where(labels == S.GROUPS[1], 1, -1)).astype(np.int32)
    D = tl._cell_type_matrix(adata, rows, False)
    cols = np.flatnonzero(tl.highly_variable_genes(D, n_top_genes)["highly_variable"].values)
    count, mean, m2 = engine.group_moments(D, codes, 2, cols=cols.astype(np.int32))
    G = cols.size
    logfc, ave, rss, df, unscaled = tl._two_group_fit(count, mean, m2, "reference", 0)
    s2 = rss / df
    s2_prior, df_prior = tl._ebayes_prior(s2, df)
    s2_post = np.full(G, s2_prior) if np.isinf(df_prior) else (df_prior * s2_prior + df * s2) / (df_prior + df)
    t = logfc / (unscaled * np.sqrt(s2_post))
    df_total = min(df + df_prior, G * df)
    p = 2.0 * (stats.norm.sf(np.abs(t)) if np.isinf(df_total) else stats.t.sf(np.abs(t), df_total))
    return pd.DataFrame({"logFC": logfc, "AveExpr": ave, "t": t, "P.Value": p, "adj.P.Val": tl._bh_adjust(p)},
                        index=pd.Index(genes[cols], name="gene"))


@pytest.mark.parametrize("sparse", [False, True])
def test_compute_diff_expressions_keeps_its_bits(sparse):
    adata, props, _ = _cohort()
    ad = _sparse_twin(adata) if sparse else adata
    got = tl.compute_diff_expressions(ad, S.CELL, props, n_top_genes=40)
    want = _diff_expressions_as_before(ad, props, 40)
    assert 30 <= len(want) < 80
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    assert all(np.array_equal(got[c].values.view(np.uint64), want[c].values.view(np.uint64)) for c in got.columns)
