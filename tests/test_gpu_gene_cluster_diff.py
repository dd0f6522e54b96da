"""Gene-cluster differentiation on the device (K10: pilot_ot_bootstrap_huber_fits, engine.bootstrap_huber_fits,
tl.infer_gene_cluster_differentiation, tl.gene_cluster_differentiation) against the numpy restatement of the penalised Huber
optimum (tests/bootfit_restatement.py), a pure host restatement of the whole computation from the same draws, and the
reference-executed fixture tests/golden/gene_cluster_4types.npz."""
import numpy as np
import pandas as pd
import pytest

import bootfit_restatement as BR
import gene_cluster_helpers as H
from pilot_amd import _lib, engine, tl

pytestmark = pytest.mark.gpu


def _problem(rng, n, B, dtype, n_cols=4, models=(0, 1, 2), distinct=None):
    x = np.sort(rng.integers(1, 9, n)).astype(np.float64)
    x[:3] = [1.0, 4.0, 8.0][:min(3, n)]
    Y = np.log1p(rng.poisson(2.0 + 0.4 * x[:, None], (n, n_cols))).astype(dtype)
    P = len(models)
    idx = rng.integers(0, n, (P, n, B)).astype(np.int32)
    if distinct is not None:                       # resamples drawn from `distinct` base positions only
        pick = np.array([0, n - 1][:distinct]) if distinct <= 2 else None
        idx = pick[rng.integers(0, pick.size, (P, n, B))].astype(np.int32)
    cols = rng.integers(0, n_cols, P).astype(np.int32)
    return Y, x, cols, np.asarray(models, dtype=np.int32), idx


def _check_against_restatement(Y, x, cols, models, idx, params, info, well_conditioned=True):
    worst_obj, worst_prm = 0.0, 0.0
    for q in range(cols.size):
        f = BR.MODELS[models[q]]
        y = Y[:, cols[q]].astype(np.float64)
        for b in range(idx.shape[2]):
            xr = x[idx[q, :, b]]
            p_ref, s_ref, F_ref = BR.huber_opt(x, xr, y, f)
            F_dev = BR.objective(xr, y, f, params[q, b], info["sigma"][q, b])
            worst_obj = max(worst_obj, (F_dev - F_ref) / abs(F_ref))
            assert F_dev <= F_ref * (1 + 1e-10) + 1e-300, (f, q, b, F_dev, F_ref)
            p = 3 if f == "linear_quadratic" else 2
            assert np.isnan(params[q, b, p:]).all() and np.isfinite(params[q, b, :p]).all()
            if well_conditioned and np.unique(xr).size >= 3 + (f == "linear_quadratic"):
                scale = np.abs(p_ref).max()
                worst_prm = max(worst_prm, np.abs(params[q, b, :p] - p_ref).max() / scale)
    assert (info["flags"] == 0).all() and info["not_converged"] == 0
    return worst_obj, worst_prm


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,B", [(3, 1), (5, 65), (20, 50), (20, 64), (3000, 2)])
def test_bootfit_against_restatement(dtype, n, B):
    rng = np.random.default_rng(n * 100 + B)
    Y, x, cols, models, idx = _problem(rng, n, B, dtype)
    params, info = engine.bootstrap_huber_fits(Y, x, cols, models, idx, return_info=True)
    assert params.shape == (3, B, 3)
    obj, prm = _check_against_restatement(Y, x, cols, models, idx, params, info)
    assert prm <= 1e-6, prm
    print("n=%d B=%d %s: objective <= restatement x (1 + %.1e), params %.1e" % (n, B, np.dtype(dtype).name, obj, prm))


@pytest.mark.parametrize("distinct", [1, 2])
def test_bootfit_degenerate_resamples(distinct):
    """resamples with 1 or 2 distinct times: still the penalised optimum, finite, not flagged"""
    rng = np.random.default_rng(distinct)
    Y, x, cols, models, idx = _problem(rng, 20, 50, np.float64, distinct=distinct)
    assert all(np.unique(x[idx[q, :, b]]).size <= distinct for q in range(3) for b in range(50))
    params, info = engine.bootstrap_huber_fits(Y, x, cols, models, idx, return_info=True)
    _check_against_restatement(Y, x, cols, models, idx, params, info, well_conditioned=False)


def test_bootfit_bit_identical_routes():
    rng = np.random.default_rng(7)
    Y, x, cols, models, idx = _problem(rng, 300, 50, np.float32, n_cols=6, models=(0, 1, 2, 1, 0, 2, 2))
    a = engine.bootstrap_huber_fits(Y, x, cols, models, idx)
    b = engine.bootstrap_huber_fits(Y, x, cols, models, idx)
    c = engine.bootstrap_huber_fits(engine.DeviceMatrix.upload(Y), x, cols, models, idx)
    _lib.test_switch("PILOT_OT_BOOTFIT_CHUNK_PROBLEMS", 2)
    try:
        d = engine.bootstrap_huber_fits(Y, x, cols, models, idx)
    finally:
        _lib.test_switch("PILOT_OT_BOOTFIT_CHUNK_PROBLEMS", None)
    for other in (b, c, d):
        assert np.array_equal(a.view(np.uint64), other.view(np.uint64))


def test_bootfit_host_view_gives_the_bits_of_its_copy():
    """a row-strided host view (its own leading dimension, copied packed by the library), its contiguous copy and an upload of
    that copy: the kernel reads the same values each time"""
    rng = np.random.default_rng(10)
    Y, x, cols, models, idx = _problem(rng, 10, 3, np.float64, n_cols=7, models=(0, 1, 2, 1))
    W = rng.standard_normal((10, 12))
    W[:, 2:9] = Y
    view = W[:, 2:9]
    assert not view.flags.c_contiguous and engine._dense_arg(view, "Y", mode="strided").ld == 12
    copy = np.ascontiguousarray(view)
    a, ia = engine.bootstrap_huber_fits(view, x, cols, models, idx, return_info=True)
    b, ib = engine.bootstrap_huber_fits(copy, x, cols, models, idx, return_info=True)
    c, ic = engine.bootstrap_huber_fits(engine.DeviceMatrix.upload(copy), x, cols, models, idx, return_info=True)
    assert a.shape == (4, 3, 3) and np.isfinite(a[:, :, :2]).all()
    for other, info in ((b, ib), (c, ic)):
        assert np.array_equal(a.view(np.uint64), other.view(np.uint64))
        assert np.array_equal(ia["sigma"].view(np.uint64), info["sigma"].view(np.uint64))
        assert np.array_equal(ia["steps"], info["steps"]) and np.array_equal(ia["flags"], info["flags"])


def test_bootfit_not_converged_flag():
    rng = np.random.default_rng(3)
    Y, x, cols, models, idx = _problem(rng, 40, 8, np.float64)
    _lib.test_switch("PILOT_OT_TRAJFIT_MAX_ITER", 0)
    try:
        _, info = engine.bootstrap_huber_fits(Y, x, cols, models, idx, return_info=True)
    finally:
        _lib.test_switch("PILOT_OT_TRAJFIT_MAX_ITER", None)
    assert info["not_converged"] == int((info["flags"] != 0).sum()) > 0


@pytest.mark.parametrize("n", [5, 20, 67])
def test_identity_bootstrap_is_the_trajectory_fit(n):
    """A bootstrap whose index vector is the identity is K9's Huber fit of that column and model: the two kernels carry the same
    Newton loop and run it from two starts (K9: the OLS fit, K10: the penalised least-squares fit).  Both reach the optimum by
    the objective criterion; their coefficients are held to 2e-6 of the largest, the sum of the 1e-6 each entry is held to
    against its own restatement."""
    Y, x, cols, models, _ = _problem(np.random.default_rng(n), n, 2, np.float64)
    idx = np.ascontiguousarray(np.broadcast_to(np.arange(n, dtype=np.int32)[None, :, None], (3, n, 2)))
    params, info = engine.bootstrap_huber_fits(Y, x, cols, models, idx, return_info=True)
    fits, finfo = engine.trajectory_fits(Y, x, model="huber", return_info=True)
    assert np.array_equal(params[:, 0].view(np.uint64), params[:, 1].view(np.uint64))
    assert np.array_equal(np.ascontiguousarray(info["sigma"][:, 0]).view(np.uint64),
                          np.ascontiguousarray(info["sigma"][:, 1]).view(np.uint64))
    assert np.array_equal(info["steps"][:, 0], info["steps"][:, 1])
    assert not info["flags"].any() and info["not_converged"] == 0
    assert not finfo["flags"].any() and finfo["not_converged"] == 0
    for q in range(cols.size):
        f, c, m = BR.MODELS[models[q]], cols[q], models[q]
        y = Y[:, c]
        p_ref, _, F_ref = BR.huber_opt(x, x, y, f)
        p = p_ref.size
        boot, traj = params[q, 0], fits["params"][c, m]
        F_boot = BR.objective(x, y, f, boot, info["sigma"][q, 0])
        F_traj = BR.objective(x, y, f, traj, finfo["sigma"][c, m])
        diff = np.abs(boot[:p] - traj[:p]).max() / np.abs(p_ref).max()
        print("n=%d %s: objective / optimum - 1: bootstrap %.1e, trajectory %.1e; params differ by %.1e of the largest"
              % (n, f, F_boot / F_ref - 1, F_traj / F_ref - 1, diff))
        assert F_boot <= F_ref * (1 + 1e-10) and F_traj <= F_ref * (1 + 1e-10), (f, q, F_boot, F_traj, F_ref)
        assert diff <= 2e-6, (f, q, boot, traj)


# ---- end to end -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cohort():
    return H.counts_cohort()


def test_e2e_counts_cohort_against_host_restatement(cohort):
    """Every column against the host restatement from the same draws.

    Tolerances, derived: the bootstrap fits on both sides are the same optima (objective within 1e-10, params to ~1e-9 on
    these fits; the restatement normalises with differently ordered f64 sums), so the bootstrap betas are held to 1e-6 relative
    to each row's largest |beta| and FC (a smooth function of the table fits) to 1e-9.  waldStat and pvalue are NOT a smooth
    function of the betas: the reference's halfCovInv takes ROWS of the eigenvector matrix of a rank-deficient 20 x 20 matrix,
    so they mix in its null-space eigenvectors, whose basis is arbitrary -- a 3e-10 change of the betas moved waldStat by 40 %
    with both sides restated on the host.  They are therefore held bit for bit to the host Wald step fed the device's own betas,
    and df (the rank, robust) exactly.  Rows whose mean-curve choice is decided by less than 1e-9 in adjusted R^2 (the mean curve
    is a polynomial of degree <= 2, so exact-fit ties are common), or where the two sides chose differently (an exact fit the
    device flags not converged is ineligible), are counted, not compared."""
    ad, tables = cohort
    frame, info = tl.infer_gene_cluster_differentiation(ad, tables, random_state=11, return_info=True)
    ref, rinfo = H.host_restatement(ad, tables, 11)
    assert list(frame.columns) == tl._GCD_COLUMNS
    assert frame[["gene", "cluster"]].equals(ref[["gene", "cluster"]])
    assert info["wald_rows"] >= 6 and info["rows"] > info["wald_rows"]
    assert info["not_converged_rows"] == 0 and info["no_table2_rows"] == 0
    for k in ["Expression pattern", "fit-pvalue", "fit-rsquared", "fit-mod-rsquared"]:
        assert (frame[k].to_numpy() == ref[k].to_numpy()).all(), k
    single = (frame["waldStat"] == 1.0) & (frame["pvalue"] == 0.0) & (frame["FC"] == 0.0)
    assert frame[single].reset_index(drop=True).equals(ref[single.to_numpy()].reset_index(drop=True).astype(frame.dtypes.to_dict()))
    wald = np.flatnonzero(~single.to_numpy())
    same = np.array([a == b for a, b in zip(info["table2"], rinfo["table2"])])
    sel = (rinfo["margin"] > 1e-9) & same
    held = wald[sel]
    print("Wald rows %d, held %d (table2 ties %d, other table2 choice %d, table2 fits flagged %s); draws %.3f s, device %.3f s, "
          "Wald %.3f s" % (wald.size, held.size, (rinfo["margin"] <= 1e-9).sum(), (~same).sum(),
                           info["table2_not_converged"].sum(axis=0).tolist(), info["draw_s"], info["device_s"], info["wald_s"]))
    assert held.size >= 3
    scale = np.abs(rinfo["boot"][sel]).max(axis=(1, 2))[:, None, None]
    dev_boot = info["boot"][sel]
    assert (np.abs(dev_boot - rinfo["boot"][sel]) <= 1e-6 * scale).all(), np.abs(dev_boot - rinfo["boot"][sel]).max()
    assert (frame["df"].to_numpy()[held] == ref["df"].to_numpy()[held]).all()
    np.testing.assert_allclose(frame["FC"].to_numpy()[held], ref["FC"].to_numpy()[held].astype(np.float64), rtol=1e-9, atol=1e-12)
    # the Wald step on the device's betas, bit for bit
    pline = np.linspace(1, 20, 20)
    cut = np.log(np.power(2, np.log2(1.5)))
    for j, k in enumerate(wald):
        g, c = frame["gene"][k], frame["cluster"][k]
        r1 = tables[c][tables[c]["Gene ID"] == g].iloc[0]
        f1, f2 = r1["Fitted function"], info["table2"][j]
        betas = tl._gcd_fill_betas(f1, tl._gcd_params(r1)) + tl._gcd_fill_betas(f2, info["table2_params"][j])
        w, df, pv = tl._gcd_wald(tl._gcd_features(f1, pline, True), tl._gcd_features(f2, pline, True), betas, info["boot"][j],
                                 cut, 1e-8)
        assert (w, df, pv) == (frame["waldStat"][k], frame["df"][k], frame["pvalue"][k]), (g, c)
    for k in ["waldStat", "df", "pvalue", "FC", "fit-pvalue"]:
        assert np.issubdtype(frame[k].dtype, np.number), k


def test_e2e_seed_forms_agree(cohort):
    ad, tables = cohort
    a = tl.infer_gene_cluster_differentiation(ad, tables, random_state=4)
    b = tl.infer_gene_cluster_differentiation(ad, tables, random_state=4)
    np.random.seed(4)
    c = tl.infer_gene_cluster_differentiation(ad, tables)
    pd.testing.assert_frame_equal(a, b)
    pd.testing.assert_frame_equal(a, c)
    d = tl.infer_gene_cluster_differentiation(ad, tables, random_state=5)
    assert not d["waldStat"].equals(a["waldStat"])


def test_e2e_not_converged_rows_are_nan(cohort):
    ad, tables = cohort
    _lib.test_switch("PILOT_OT_TRAJFIT_MAX_ITER", 0)
    try:
        frame, info = tl.infer_gene_cluster_differentiation(ad, tables, random_state=1, return_info=True)
    finally:
        _lib.test_switch("PILOT_OT_TRAJFIT_MAX_ITER", None)
    assert info["not_converged_rows"] + info["no_table2_rows"] == info["wald_rows"] > 0
    wald = ~((frame["waldStat"] == 1.0) & (frame["pvalue"] == 0.0) & (frame["FC"] == 0.0))
    assert frame.loc[wald, "waldStat"].isna().all() and frame.loc[wald, "pvalue"].isna().all()


def test_wrapper_matches_infer(cohort):
    ad, tables = cohort
    a = tl.gene_cluster_differentiation(ad, tables, cellnames=["A"], number_genes=2, random_state=9)
    genes = tl._gcd_select_genes(tables, ["A"], ["Expression pattern", "adjusted P-value", "R-squared"], 2)
    b = tl.infer_gene_cluster_differentiation(ad, tables, gene_list=genes, start=1, end=12, random_state=9)
    pd.testing.assert_frame_equal(a, b)


def test_e2e_reference_fixture():
    """Against the reference's own run (tests/golden/gen_gene_cluster_golden.py).  Row order, gene, cluster, Expression pattern
    and fit-* exact, df exact on every single-cell-type row.  scikit-learn's Huber fits stop short of the optimum (K9,
    DESIGN.md: on this fixture every row has a bootstrap fit at least 2e-5 above it, the median row 2.5 %), so df / waldStat /
    pvalue / FC are held (df exact, the rest rtol 1e-6) only on rows where every scikit-learn bootstrap fit and the table2 fit
    reached the optimum within 1e-9 relative and the table2 choice is decided by more than 1e-9.  The early stops also give a
    direction of the Wald matrix a variance the optimum does not have (an exactly linear mean curve's x^2 coefficient), so df
    can be lower here, and waldStat moves by O(1) with any change of the betas (the eigenvector-row quirk, see the test above);
    the other rows are counted and printed."""
    z, ad, tables = H.load_fixture()
    frame = tl.infer_gene_cluster_differentiation(ad, tables, gene_list=list(z["gene_list"]),
                                                  cluster_names=list(z["cluster_names"]), start=int(z["start"]), end=int(z["end"]),
                                                  n_points=int(z["n_points"]), random_state=int(z["seed"]), normalize=False)
    assert (frame["gene"].to_numpy() == z["out_gene"]).all()
    assert (frame["cluster"].to_numpy() == z["out_cluster"]).all()
    assert (frame["Expression pattern"].to_numpy() == z["out_pattern"]).all()
    for k in ["fit-pvalue", "fit-rsquared", "fit-mod-rsquared"]:
        assert np.array_equal(frame[k].to_numpy(), z["out_" + k]), k
    w = z["wald_rows"]
    single = np.setdiff1d(np.arange(len(frame)), w)
    assert np.array_equal(frame["df"].to_numpy(dtype=np.float64)[single], z["out_df"][single])
    held = w[(z["sk_gap"] <= 1e-9) & (z["t2_margin"] > 1e-9) & z["eps_ok"]]
    assert np.array_equal(frame["df"].to_numpy(dtype=np.float64)[held], z["out_df"][held])
    print("fixture: df differs on %d of %d Wald rows" % ((frame["df"].to_numpy()[w] != z["out_df"][w]).sum(), w.size))
    for k in ["waldStat", "pvalue", "FC"]:
        np.testing.assert_allclose(frame[k].to_numpy()[held], z["out_" + k][held], rtol=1e-6, atol=1e-10, err_msg=k)
    rel = np.abs(frame["waldStat"].to_numpy()[w] - z["out_waldStat"][w]) / np.maximum(np.abs(z["out_waldStat"][w]), 1e-300)
    print("fixture: %d rows, %d Wald rows, %d held; not held: median |dWald| / Wald %.2e (scikit-learn gap median %.2e)"
          % (len(frame), w.size, held.size, np.median(rel), np.median(z["sk_gap"])))
    # exact-fit ties in table2 (with two cell types the mean curve IS one curve): the reference picks the first model in
    # linear, linear_quadratic, quadratic order among the tied adjusted R^2 (a strict >), as the device's rule does
    ties = z["t2_margin"] == 0.0
    print("table2 exact ties: %d, reference choices %s" % (ties.sum(), z["t2_chosen"][ties].tolist()))
