"""Trajectory model fits on the device (K9: pilot_ot_trajectory_fits, engine.trajectory_fits, tl.cell_importance,
tl.genes_importance) against the numpy / scipy restatement (tests/trajfit_restatement.py) and scikit-learn."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import trajfit_restatement as R
from conftest import GOLDEN_REAL, load_golden
from pilot_amd import _lib, engine, tl

pytestmark = pytest.mark.gpu

MARGIN = 1e-9


def _genes_like(n_samples=200, per=25, n_targets=2000, seed=0, dtype=np.float32):
    """counts-like: ~n_samples * per cells, time = the sample's rank, many zeros; one all-zero target"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(per // 2, 3 * per // 2 + 1, n_samples)
    x = np.repeat(np.arange(1, n_samples + 1), sizes).astype(np.float64)
    t = x / n_samples
    base = rng.gamma(0.3, 1.0, n_targets)
    a, b = rng.normal(0, 1.5, n_targets), rng.normal(0, 1.5, n_targets)
    lam = base[None, :] * np.exp(a[None, :] * t[:, None] + b[None, :] * (t[:, None] - 0.5) ** 2)
    Y = rng.poisson(lam).astype(dtype)
    Y[:, 7] = 0
    return x, Y


def _scale(x, Y, model):
    """per-coefficient scale: the size that moves the predictions by the target's rms"""
    Z = R.design(x, model)
    rms = np.sqrt(np.mean(np.asarray(Y, dtype=np.float64) ** 2, axis=0))
    return rms[:, None] / np.abs(Z).max(axis=0)[None, :]


def _compare_ols(x, Y, pval_thr=0.05, modify_r2=False):
    """Params to 1e-9 relative, with a floor: 1e-9 of the coefficient size that moves the predictions by the target's rms
    (_scale), so a coefficient that is ~0 is held in absolute terms; R^2 and p-values to 1e-11 absolute."""
    got = engine.trajectory_fits(Y, x, model="ols", pval_thr=pval_thr, modify_r2=modify_r2)
    Yd = np.asarray(Y, dtype=np.float64)
    T = Yd.shape[1]
    inside = 0
    for m, model in enumerate(R.MODELS):
        sc = _scale(x, Yd, model)
        for t in range(T):
            f = R.fit_one(x, Yd[:, t], model)
            p = f["params"].size
            d = np.abs(got["params"][t, m, :p] - f["params"])
            assert np.all(d <= 1e-9 * np.maximum(np.abs(f["params"]), sc[t])), (t, model, got["params"][t, m], f["params"])
            if p == 2:
                assert np.isnan(got["params"][t, m, 2]) and np.isnan(got["pvalues"][t, m, 2])
            for k in ("rsquared_adj", "mod_rsquared_adj"):
                a, b = got[k][t, m], f[k]
                assert (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= 1e-11, (t, model, k, a, b)
            a, b = got["pvalues"][t, m, :p], f["pvalues"]
            assert np.all((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= 1e-11)), (t, model, a, b)
    for t in range(T):
        ref = R.best_model(x, Yd[:, t], pval_thr=pval_thr, modify_r2=modify_r2)
        r, pp = ref["pearson"]
        if np.isnan(r):
            assert np.isnan(got["pearson_r"][t]) and np.isnan(got["pearson_p"][t])
        else:
            assert abs(got["pearson_r"][t] - r) <= 1e-12 and abs(got["pearson_p"][t] - pp) <= 1e-11, (t, got["pearson_p"][t], pp)
        assert got["zero_fraction"][t] == np.mean(Yd[:, t] == 0)
        assert abs(got["mean"][t] - Yd[:, t].mean()) <= 1e-12 * max(1.0, abs(Yd[:, t].mean()))
        if ref["margin"] <= MARGIN:
            inside += 1
            continue
        assert got["chosen"][t] == ref["chosen"], (t, got["chosen"][t], ref["chosen"])
        if ref["chosen"] >= 0:
            m = ref["chosen"]
            pat = tl._PATTERNS[m][got["pattern"][t]]
            assert pat == ref["pattern"]
            span = np.abs(R.design(np.array([x.min(), x.max()]), R.MODELS[m]) @ np.abs(ref["fits"][m]["params"])).max()
            assert abs(got["slope"][t] - ref["slope"]) <= 1e-9 * span / (x.max() - x.min())
        else:
            assert got["pattern"][t] == -1 and np.isnan(got["slope"][t])
        if not np.any(Yd[:, t]):
            assert got["chosen"][t] == -1
    assert inside <= 0.001 * T, "%d of %d targets inside the deciding margin" % (inside, T)
    return got


@pytest.fixture(scope="module")
def kidney():
    g = load_golden(GOLDEN_REAL)
    pt = np.random.default_rng(11).permutation(g["proportions"].shape[0]).astype(np.float64) * 0.37
    return g, pt


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ols_kidney_proportions(kidney, dtype):
    g, pt = kidney
    order = np.argsort(pt, kind="stable")
    _compare_ols(np.arange(1, pt.size + 1, dtype=np.float64), g["proportions"][order].astype(dtype), pval_thr=1.0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ols_genes_like(dtype):
    x, Y = _genes_like(dtype=dtype)
    got = _compare_ols(x, Y)
    assert got["chosen"][7] == -1 and (got["chosen"] >= 0).sum() > 100


@pytest.mark.parametrize("n,T", [(4, 3), (5, 70), (37, 129)])
def test_ols_shape_edges(n, T):
    rng = np.random.default_rng(n * T)
    x = rng.permutation(n).astype(np.float64) * 2.5 - 3.0
    Y = rng.random((n, T)) + np.outer(x, rng.normal(size=T)) * 0.3
    _compare_ols(x, Y, pval_thr=0.5)


def test_ols_long_time_axis():
    rng = np.random.default_rng(5)
    n = 200_000
    x = np.sort(rng.random(n)) * 50.0
    Y = (rng.poisson(2.0, (n, 64)) + np.outer(np.sin(x / 8.0), np.arange(64) / 16.0)).astype(np.float32)
    _compare_ols(x, Y)


def test_modified_r2_selection():
    x, Y = _genes_like(n_samples=60, per=12, n_targets=130, seed=4)
    _compare_ols(x, Y, modify_r2=True)


def _log_counts(n_samples, per, n_targets, seed):
    """genes_importance's Huber input: log1p of counts with library-size noise, genes with zero fraction <= 0.95 (its filter)"""
    x, Y = _genes_like(n_samples=n_samples, per=per, n_targets=n_targets, seed=seed, dtype=np.float64)
    Y = np.log1p(Y * (1 + 0.1 * np.random.default_rng(seed + 100).random(Y.shape)))
    return x, Y[:, ~((Y == 0).mean(axis=0) > 0.95)]


def _huber_check(x, Y, epsilon=1.35):
    """every (target, model): objective <= the host optimum x (1 + 1e-10); coefficients within 1e-6 relative of it, with the
    floor of _compare_ols (1e-6 of the coefficient size that moves the predictions by the target's rms)"""
    got, info = engine.trajectory_fits(Y, x, model="huber", epsilon=epsilon, return_info=True)
    assert info["not_converged"] == 0 and not info["flags"].any()
    for m, model in enumerate(R.MODELS):
        sc = _scale(x, Y, model)
        for t in range(Y.shape[1]):
            prm, sig, F, ok = R.huber(x, Y[:, t], model, epsilon)
            assert ok
            p = prm.size
            Fd = R.huber_objective(x, Y[:, t], model, got["params"][t, m, :p], info["sigma"][t, m], epsilon)
            assert Fd <= F * (1 + 1e-10), (t, model, Fd, F)
            d = np.abs(got["params"][t, m, :p] - prm)
            assert np.all(d <= 1e-6 * np.maximum(np.abs(prm), sc[t])), (t, model, got["params"][t, m], prm)
    return got, info


def test_huber_is_the_optimum():
    x, Y = _log_counts(80, 12, 150, 2)
    assert Y.shape[1] > 50 and (Y == 0).mean() > 0.4
    _huber_check(x, Y)
    _huber_check(x, Y[:, :40], epsilon=2.0)
    x, Y = _log_counts(200, 25, 40, 3)
    _huber_check(x, Y.astype(np.float32).astype(np.float64))


def test_huber_table_values_match_the_restatement():
    x, Y = _log_counts(60, 12, 60, 5)
    got = engine.trajectory_fits(Y, x, model="huber")
    for t in range(Y.shape[1]):
        ref = R.best_model(x, Y[:, t], kind="huber")
        for m in range(3):
            f = ref["fits"][m]
            p = f["params"].size
            assert np.all(np.abs(got["pvalues"][t, m, :p] - f["pvalues"]) <= 1e-7)
            assert abs(got["rsquared_adj"][t, m] - f["rsquared_adj"]) <= 1e-9
        if ref["margin"] > 1e-6:
            assert got["chosen"][t] == ref["chosen"]


def test_huber_agrees_with_sklearn_where_sklearn_is_at_the_optimum():
    from sklearn.linear_model import HuberRegressor
    x, Y = _log_counts(40, 10, 16, 3)
    rng = np.random.default_rng(1)                           # + Gaussian targets: where scikit-learn's fit reaches the optimum
    Y = np.c_[Y, 1 + 0.02 * x[:, None] * rng.normal(size=8) + rng.standard_normal((x.size, 8))]
    got, info = engine.trajectory_fits(Y, x, model="huber", return_info=True)
    compared = 0
    for m, model in enumerate(R.MODELS):
        Z = R.design(x, model)
        for t in range(Y.shape[1]):
            h = HuberRegressor().fit(Z[:, 1:], Y[:, t])
            ref = np.r_[h.intercept_, h.coef_]
            p = ref.size
            Fs = R.huber_objective(x, Y[:, t], model, ref, h.scale_, 1.35)
            Fd = R.huber_objective(x, Y[:, t], model, got["params"][t, m, :p], info["sigma"][t, m], 1.35)
            assert Fd <= Fs * (1 + 1e-12)
            # (within 1e-9 of the optimum a flat fit's coefficients are still free by ~1e-3; 1e-12 pins them)
            if Fs <= Fd * (1 + 1e-12):
                compared += 1
                np.testing.assert_allclose(got["params"][t, m, :p], ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    assert compared >= 10


def test_huber_not_converged_is_flagged_and_ineligible():
    x, Y = _log_counts(50, 10, 20, 6)
    _lib.test_switch("PILOT_OT_TRAJFIT_MAX_ITER", 1)
    try:
        got, info = engine.trajectory_fits(Y, x, model="huber", pval_thr=1.0, return_info=True)
    finally:
        _lib.test_switch("PILOT_OT_TRAJFIT_MAX_ITER", None)
    flagged = (info["flags"] & _lib.TRAJFIT_NOT_CONVERGED) != 0
    assert info["not_converged"] == flagged.sum() > 0
    for t in range(Y.shape[1]):
        if flagged[t].all():
            assert got["chosen"][t] == -1
        elif got["chosen"][t] >= 0:
            assert not flagged[t, got["chosen"][t]]
    full, info2 = engine.trajectory_fits(Y, x, model="huber", pval_thr=1.0, return_info=True)
    assert info2["not_converged"] == 0 and (info2["steps"] > 1).any()
    assert np.all(np.isnan(engine.trajectory_fits(Y, x, return_info=True)[1]["sigma"]))


@pytest.mark.parametrize("dtype,model", [(np.float32, "ols"), (np.float64, "ols"), (np.float32, "huber"), (np.float64, "huber")])
def test_repeated_calls_routes_and_chunks_give_identical_bits(dtype, model):
    x, Y = _genes_like(n_samples=60, per=10, n_targets=300, seed=8, dtype=dtype)
    if model == "huber":
        Y = np.log1p(Y)
    kw = dict(model=model, return_info=True)
    a = engine.trajectory_fits(Y, x, **kw)
    b = engine.trajectory_fits(Y, x, **kw)
    c = engine.trajectory_fits(engine.DeviceMatrix.upload(Y), x, **kw)
    _lib.test_switch("PILOT_OT_TRAJFIT_CHUNK_TARGETS", 64)
    try:
        d = engine.trajectory_fits(Y, x, **kw)
    finally:
        _lib.test_switch("PILOT_OT_TRAJFIT_CHUNK_TARGETS", None)
    wide = np.zeros((Y.shape[0], Y.shape[1] + 9), dtype=Y.dtype)
    wide[:, 3:3 + Y.shape[1]] = Y
    e = engine.trajectory_fits(wide[:, 3:3 + Y.shape[1]], x, **kw)      # ld > targets
    for other in (b, c, d, e):
        for u, v in zip(a, other):
            for k in u:
                np.testing.assert_array_equal(u[k], v[k], err_msg=k)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("model", ["ols", "huber"])
def test_host_view_staged_in_chunks_gives_the_bits_of_its_copy(model):
    """A row-strided host view goes to the library where it lies, with its own leading dimension; with 64 targets per chunk its 70
    columns are staged twice, the second time from an offset.  The kernel receives the packed values of the contiguous copy either
    way, so every output has the copy's bits (NaNs by position: the comparison is of the bit patterns)."""
    rng = np.random.default_rng(12)
    x = np.array([1, 1, 2, 3, 3, 4, 5, 6, 6, 7, 8, 9], dtype=np.float64)
    W = np.log1p(rng.poisson(1.0 + 0.3 * x[:, None], (12, 96))).astype(np.float32)
    view = W[:, 5:5 + 70]
    assert not view.flags.c_contiguous and engine._dense_arg(view, "Y", mode="strided").ld == 96
    kw = dict(model=model, return_info=True)
    _lib.test_switch("PILOT_OT_TRAJFIT_CHUNK_TARGETS", 64)
    try:
        got = engine.trajectory_fits(view, x, **kw)
        want = engine.trajectory_fits(np.ascontiguousarray(view), x, **kw)
    finally:
        _lib.test_switch("PILOT_OT_TRAJFIT_CHUNK_TARGETS", None)
    assert got[1].pop("not_converged") == want[1].pop("not_converged")
    for u, v in zip(got, want):
        for k in u:
            assert np.array_equal(_bits(u[k]), _bits(v[k])), k
    assert got[0]["params"].shape == (70, 3, 3) and np.isnan(got[0]["params"][:, 0, 2]).all()


# ---- the AnnData level ---------------------------------------------------------------------------------------------------
class _Uns:
    def __init__(self, uns):
        self.uns = uns


def test_cell_importance_kidney(kidney):
    g, pt = kidney
    samples = [str(s) for s in g["samples"]]
    cells = [str(c) for c in g["cells"]]
    ad = _Uns(dict(proportions={s: g["proportions"][i] for i, s in enumerate(samples)},
                   annot=pd.DataFrame({"cell_type": cells}), pseudotime=pt))
    table = tl.cell_importance(ad)
    order = np.argsort(pt, kind="stable")
    x = np.arange(1, len(samples) + 1, dtype=np.float64)
    P = g["proportions"][order]
    res = [R.best_model(x, P[:, k], pval_thr=1.0) for k in range(P.shape[1])]
    assert all(r["margin"] > MARGIN for r in res)
    rows, names = R.table(res, cells, "Cell name", 1.0)
    assert ad.uns["cellnames"] == names
    assert list(table["Cell name"]) == [r["Cell name"] for r in rows]
    assert list(table["Expression pattern"]) == [r["Expression pattern"] for r in rows]
    assert list(table["Fitted function"]) == [r["Fitted function"] for r in rows]
    for col in ("R-squared", "mod_rsquared_adj", "adjusted P-value"):
        np.testing.assert_allclose(table[col].to_numpy(), [r[col] for r in rows], rtol=0, atol=1e-11)
    exp = pd.DataFrame({"sampleID": np.asarray(samples, dtype=object)[order], "Time_score": np.arange(1, len(samples) + 1)})
    pd.testing.assert_frame_equal(ad.uns["orders"], exp)
    # the same through an explicit pseudotime
    ad2 = _Uns(dict(proportions=ad.uns["proportions"], annot=ad.uns["annot"]))
    pd.testing.assert_frame_equal(tl.cell_importance(ad2, pseudotime=pt), table)


class _Cohort:
    def __init__(self, X, obs, var_names, uns):
        self.X, self.obs, self.var_names, self.uns = X, obs, var_names, uns


def _counts_cohort(sparse, seed=21):
    rng = np.random.default_rng(seed)
    n_samples, n_genes = 40, 90
    sizes = rng.integers(8, 25, n_samples)
    sample = np.repeat(np.arange(n_samples), sizes)
    ctype = rng.choice(["T", "B"], sample.size, p=[0.7, 0.3])
    perm = rng.permutation(sample.size)                      # cells of a sample not contiguous in obs
    sample, ctype = sample[perm], ctype[perm]
    time = rng.permutation(n_samples)
    lam = rng.gamma(0.5, 2.0, n_genes)[None, :] * np.exp(np.outer(time[sample] / n_samples, rng.normal(0, 2, n_genes)))
    X = rng.poisson(lam).astype(np.float64)
    X[:, :5] *= rng.random((X.shape[0], 5)) < 0.03           # mostly-zero genes, dropped by the 0.95 rule
    obs = pd.DataFrame({"cell_types": ctype, "sampleID": ["s%d" % s for s in sample]})
    orders = pd.DataFrame({"sampleID": ["s%d" % s for s in np.argsort(time)], "Time_score": np.arange(1, n_samples + 1)})
    return _Cohort(sp.csr_matrix(X) if sparse else X, obs, ["g%d" % i for i in range(n_genes)], dict(orders=orders))


@pytest.mark.parametrize("model_type", ["LinearRegression", "HuberRegressor"])
def test_genes_importance_counts_cohort(model_type):
    ad = _counts_cohort(False)
    table = tl.genes_importance(ad, "T", model_type=model_type, p_value=0.05)
    table_csr = tl.genes_importance(_counts_cohort(True), "T", model_type=model_type, p_value=0.05)
    pd.testing.assert_frame_equal(table, table_csr)
    # the restatement: cells in orders' sample order, normalised, genes with zero fraction <= 0.95
    pos = {s: i for i, s in enumerate(ad.uns["orders"]["sampleID"])}
    cells = np.flatnonzero(ad.obs["cell_types"].to_numpy() == "T")
    cells = cells[np.argsort([pos[s] for s in ad.obs["sampleID"].to_numpy()[cells]], kind="stable")]
    x = np.array([pos[s] + 1 for s in ad.obs["sampleID"].to_numpy()[cells]], dtype=np.float64)
    X = ad.X[cells]
    keep = ~((X == 0).mean(axis=0) > 0.95)
    assert (~keep).sum() >= 3
    Yn = R.normalize_log1p(X)[:, keep]
    names = np.asarray(ad.var_names)[keep]
    kind = "ols" if model_type == "LinearRegression" else "huber"
    res = [R.best_model(x, Yn[:, k], pval_thr=0.05, kind=kind) for k in range(Yn.shape[1])]
    assert sum(r["margin"] <= (MARGIN if kind == "ols" else 1e-6) for r in res) == 0
    rows, _ = R.table(res, names, "Gene ID", 0.05)
    assert len(rows) > 5
    assert list(table["Gene ID"]) == [r["Gene ID"] for r in rows]
    assert list(table["Expression pattern"]) == [r["Expression pattern"] for r in rows]
    for col in ("R-squared", "adjusted P-value"):
        np.testing.assert_allclose(table[col].to_numpy(), [r[col] for r in rows], rtol=0, atol=1e-11 if kind == "ols" else 1e-8)
    np.testing.assert_array_equal(table["proportion"].to_numpy(), (X[:, keep] == 0).mean(axis=0)[[list(names).index(g) for g in table["Gene ID"]]])
    assert table["Slope"].dtype == np.float64 and table["Intercept"].dtype == np.float64
