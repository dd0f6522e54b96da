"""Gene-cluster differentiation (K10): argument checks of the C ABI and of the Python faces, and the host stages held to the
reference-executed fixture tests/golden/gene_cluster_4types.npz (draws, the Wald step, the gene-list selection).  CPU only:
every library call here is refused before the device is touched."""
import ctypes
import hashlib

import numpy as np
import pandas as pd
import pytest

import gene_cluster_helpers as H
from pilot_amd import _lib, engine, tl


def _rc(n=6, n_cols=2, ld=2, dtype=1, x=None, P=2, cols=(0, 1), models=(0, 2), B=3, idx=None, epsilon=1.35, null=None):
    L = _lib.load()
    Y = np.zeros(max(n, 1) * max(ld, 1) + 1)
    x = np.arange(max(n, 1), dtype=np.float64) if x is None else np.asarray(x, dtype=np.float64)
    cols = np.asarray(cols, dtype=np.int32)
    models = np.asarray(models, dtype=np.int32)
    idx = np.zeros(max(P * n * B, 1), dtype=np.int32) if idx is None else np.asarray(idx, dtype=np.int32)
    params = np.empty(max(P * B * 3, 1))
    ptrs = dict(Y=ctypes.c_void_p(Y.ctypes.data), x=_lib.dptr(x), cols=_lib.iptr(cols), models=_lib.iptr(models),
                idx=_lib.iptr(idx), params=_lib.dptr(params))
    if null:
        ptrs[null] = None
    return L.pilot_ot_bootstrap_huber_fits(ptrs["Y"], 0, dtype, n, n_cols, ld, ptrs["x"], P, ptrs["cols"], ptrs["models"], B,
                                           ptrs["idx"], epsilon, ptrs["params"], None, None, None, None)


BAD = [
    dict(n=0),
    dict(n_cols=0),
    dict(ld=1),                                   # ld < n_cols
    dict(dtype=2),
    dict(P=-1),
    dict(B=0),
    dict(epsilon=0.99),
    dict(epsilon=float("nan")),
    dict(x=[0, 1, 2, np.nan, 4, 5]),
    dict(cols=(0, 2)),                            # column outside Y
    dict(cols=(-1, 0)),
    dict(models=(0, 3)),
    dict(models=(-1, 0)),
    dict(idx=np.r_[np.zeros(35), 6].astype(np.int32)),    # an index = n
    dict(idx=np.r_[-1, np.zeros(35)].astype(np.int32)),
    dict(null="Y"), dict(null="x"), dict(null="params"), dict(null="cols"), dict(null="models"), dict(null="idx"),
]


@pytest.mark.parametrize("kw", BAD)
def test_c_abi_rejects_before_the_device(kw):
    assert _rc(**kw) == _lib.EINVAL
    assert _lib.load().pilot_ot_last_error()


def test_zero_problems_is_a_no_op():
    assert _rc(P=0, idx=np.zeros(1)) == _lib.OK


@pytest.mark.parametrize("bad", ["shape", "models", "x"])
def test_engine_rejects(bad):
    Y = np.zeros((6, 2))
    x, cols, models, idx = np.arange(6.0), [0, 1], [0, 1], np.zeros((2, 6, 4), dtype=np.int32)
    if bad == "shape":
        idx = idx[:, :5]
    elif bad == "models":
        models = [0]
    else:
        x = np.arange(5.0)
    with pytest.raises(ValueError):
        engine.bootstrap_huber_fits(Y, x, cols, models, idx)


@pytest.fixture(scope="module")
def fixture():
    return H.load_fixture()


@pytest.mark.parametrize("kw,exc", [(dict(n_points=2), ValueError), (dict(n_bootstraps=1), ValueError),
                                    (dict(start=5, end=5), ValueError), (dict(fc_thr=0.0), ValueError),
                                    (dict(cluster_names=["alpha", "nope"]), KeyError)])
def test_infer_rejects_before_device_work(fixture, kw, exc):
    _, ad, tables = fixture
    with pytest.raises(exc):
        tl.infer_gene_cluster_differentiation(ad, tables, **kw)


def test_infer_rejects_a_table_without_the_columns(fixture):
    _, ad, tables = fixture
    t = dict(tables)
    t["alpha"] = t["alpha"].drop(columns="mod_rsquared_adj")
    with pytest.raises(ValueError, match="mod_rsquared_adj"):
        tl.infer_gene_cluster_differentiation(ad, t)


def test_draws_reproduce_the_reference_resamples(fixture):
    z, _, _ = fixture
    sizes = [int(s) for s in z["draw_sizes"]]
    draws = tl._gcd_draws(np.random.RandomState(int(z["seed"])), sizes, 50)
    digest = hashlib.sha256(b"".join(d[:, b].astype(np.int64).tobytes() for d in draws for b in range(50))).hexdigest()
    assert digest == str(z["draw_sha256"])
    np.random.seed(int(z["seed"]))                 # the global legacy stream gives the same draws
    again = tl._gcd_draws(np.random.mtrand._rand, sizes, 50)
    assert all(np.array_equal(a, b) for a, b in zip(draws, again))


def test_wald_stage_reproduces_the_reference(fixture):
    """Fed the reference's bootstrap betas and table2 fits, the host stage gives its df exactly and its waldStat / pvalue / FC to
    1e-12 relative, absolute below 1 (a Wald statistic near 0 is rounding noise of a rank-deficient quadratic form -- the
    reference reports values like -7.8e-4 -- so its floor is absolute); about a third of the rows are bit-equal, the rest differ
    in the last bits of the 20 x 20 matrix products."""
    z, ad, tables = fixture
    pline = np.linspace(int(z["start"]), int(z["end"]), int(z["n_points"]))
    cut = np.log(np.power(2, np.log2(float(z["fc_thr"]))))
    bit_equal = 0
    for j, k in enumerate(z["wald_rows"]):
        g, c = z["out_gene"][k], z["out_cluster"][k]
        t = tables[c]
        r1 = t[t["Gene ID"] == g].iloc[0]
        f1 = r1["Fitted function"]
        f2 = H.TR.MODELS[int(z["t2_chosen"][j])]
        p2 = z["t2_params"][j]
        betas = tl._gcd_fill_betas(f1, tl._gcd_params(r1)) + tl._gcd_fill_betas(f2, p2)
        w, df, pv = tl._gcd_wald(tl._gcd_features(f1, pline, True), tl._gcd_features(f2, pline, True), betas, z["boot"][j], cut,
                                 float(z["eigen_thresh"]))
        curve1 = np.matmul(tl._gcd_features(f1, pline, False), tl._gcd_params(r1))
        curve2 = np.matmul(tl._gcd_features(f2, pline, False), p2[:3 if f2 == "linear_quadratic" else 2])
        fc = np.log2(curve1.mean()) - np.log2(curve2.mean())
        assert df == z["out_df"][k]
        for mine, ref in ((w, z["out_waldStat"][k]), (pv, z["out_pvalue"][k]), (fc, z["out_FC"][k])):
            assert abs(mine - ref) <= 1e-12 * max(abs(ref), 1.0), (g, c, mine, ref)
        bit_equal += (w == z["out_waldStat"][k]) and (pv == z["out_pvalue"][k]) and (fc == z["out_FC"][k])
    print("Wald rows bit-equal to the reference: %d of %d" % (bit_equal, len(z["wald_rows"])))


def test_mean_curves_are_the_reference_s(fixture):
    """the mean curve each table2 fit saw (the reference's RNA_target_clusters.mean()) from the tables, bit for bit"""
    z, ad, tables = fixture
    pline = np.linspace(int(z["start"]), int(z["end"]), int(z["n_points"]))
    names = list(z["cluster_names"])
    for j, k in enumerate(z["wald_rows"]):
        g, c = z["out_gene"][k], z["out_cluster"][k]
        others = [o for o in names if o != c and (tables[o]["Gene ID"] == g).any()]
        cs = [np.matmul(tl._gcd_features(tables[o][tables[o]["Gene ID"] == g].iloc[0]["Fitted function"], pline, False),
                        tl._gcd_params(tables[o][tables[o]["Gene ID"] == g].iloc[0])) for o in others]
        assert np.array_equal(np.mean(np.stack(cs), axis=0), z["t2_ybar"][j]), (g, c)


def test_gene_selection_is_the_reference_s():
    """sort_values(sort, ascending=[True, True, False]).groupby('Expression pattern').head(n), np.unique over cell types; ties
    keep table order (pandas' sort of several keys is stable)"""
    t = pd.DataFrame({"Gene ID": ["a", "b", "c", "d", "e", "f", "g"],
                      "Expression pattern": ["linear up", "linear up", "linear down", "linear up", "linear down", "quadratic up",
                                             "linear up"],
                      "adjusted P-value": [0.01, 0.01, 0.2, 0.001, 0.2, 0.5, 0.01],
                      "R-squared": [0.3, 0.5, 0.1, 0.2, 0.4, 0.9, 0.5]})
    u = t.assign(**{"Gene ID": ["h", "a", "i", "j", "k", "l", "m"]})
    got = tl._gcd_select_genes({"X": t, "Y": u}, ["X", "Y"], ["Expression pattern", "adjusted P-value", "R-squared"], 2)
    # X: linear down -> e, c (R^2 desc); linear up -> d (p 0.001), then b (p 0.01, R^2 0.5 before a's 0.3; g ties b, later);
    # quadratic up -> f.  Y likewise with its names: k, i, j, a, l.
    assert list(got) == sorted({"e", "c", "d", "b", "f", "k", "i", "j", "a", "l"})


def test_wrapper_rejects_unknown_cellnames(fixture):
    _, ad, tables = fixture
    with pytest.raises(KeyError):
        tl.gene_cluster_differentiation(ad, tables, cellnames=["nope"])
