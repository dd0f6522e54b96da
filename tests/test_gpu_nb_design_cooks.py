"""Cook's distances under a general design on the device (K28, pilot_ot_nb_design_cooks) against the numpy restatement
(tests/nb_design_cooks_restatement.py: the cells from a dict of row bytes, np.sort and fsum, the hat diagonal from a long-double
refined solve of the explicit X^T W X + lambda I), given the SAME coefficients and dispersions, and tl.outliers_design against its
host tail written out from the engine calls (test_nb_design_cooks_args.py: outliers_design_by_hand).

Tolerances.  The integers -- arg_max, n_above, n_replace, which counts are replaced and by what -- are exact: the generator keeps only
genes whose distances stay 1e-6 (relative) clear of the cutoff, whose replacements stay 1e-9 clear of an integer and whose Jacobi-scaled
Gram matrix has cond_2 <= 1e3, all checked on the restatement when the case is built.  alpha_robust, max_cooks and trimmed_base to
1e-10 relative (K25's derivation: sums of at most 4096 terms of one sign, m 2^-53 <= 4.5e-13, a margin of about 200).  H to
max(1e-10, 100 p kappa 2^-53) relative, kappa the Jacobi-scaled cond_2 of the gene's M: the backward error of a Cholesky solve is
about p 2^-53 in the scaled matrix, so its forward error p kappa 2^-53, with K25's margin of about 100.  D to that tolerance times
(1 + 2 h / (1 - h)), the logarithmic derivative of h / (1 - h)^2, plus 1e-10, both of the same expression with |c - mu| replaced by
c + mu (mu comes from the same coefficients on both sides).  The worst measured value of each is printed."""
import functools

import numpy as np
import pandas as pd
import pytest

import nb_cooks_restatement as CR
import nb_design_cooks_restatement as KR
import nb_glm_restatement as RR
from pilot_amd import engine, tl
from test_nb_design_cooks_args import ARGS, hold_outliers_frame, hold_to_k25, planted_table_with_batch, ridge_pull

pytestmark = pytest.mark.gpu

RTOL = 1e-10
GENES = (1, 63, 65)
INTS = ("arg_max", "n_above", "n_replace")
FLOATS = ("alpha_robust", "max_cooks", "trimmed_base")
KEYS = INTS + FLOATS + ("D", "H")


def _case(key, G):
    return KR.first_genes(KR.design_case(key), G)


def _run(Y, C, cols=slice(None), distances=True):
    got = engine.nb_design_cooks(Y, C["X"], C["s"], C["alpha"][cols], C["beta"][cols], C["cutoff"], C["min_replace"], return_distances=distances)
    for name in ("D", "H"):
        if isinstance(got.get(name), engine.DeviceMatrix):
            got[name] = engine.download(got[name])
    return got


def _h_tolerance(C):
    """per gene, relative"""
    with np.errstate(invalid="ignore"):
        return np.maximum(RTOL, 100.0 * C["p"] * C["want"]["kappa"] * 2.0 ** -53)


def _hold_hat(C, got):
    """H and the identity sum_j h_j = p - lambda tr(M^-1), to the kappa-scaled bound; D to it times (1 + 2 h / (1 - h)) plus 1e-10"""
    want = C["want"]
    H, Hw, D, Dw, scale = got["H"], want["H"], got["D"], want["D"], want["D_scale"]
    np.testing.assert_array_equal(np.isnan(H), np.isnan(Hw))
    np.testing.assert_array_equal(np.isnan(D), np.isnan(Dw))
    live = ~np.isnan(Hw).any(axis=0)
    if not live.any():
        return
    tol = _h_tolerance(C)[None, live]
    H, Hw, D, Dw, scale = H[:, live], Hw[:, live], D[:, live], Dw[:, live], scale[:, live]
    err = np.abs(H - Hw) / Hw
    print("H: worst error %.3g of its tolerance (%.3g relative)" % ((err / tol).max(), err.max()))
    assert (err <= tol).all() and (H > 0).all() and (H < 1).all()
    total = np.abs(H.sum(axis=0) - (C["p"] - want["ridge_trace"][live])) / C["p"]
    print("sum h: worst error %.3g of its tolerance" % (total / tol[0]).max())
    assert (total <= tol[0]).all()
    d_tol = tol * (1.0 + 2.0 * Hw / (1.0 - Hw)) + RTOL
    err = np.abs(D - Dw) / scale
    print("D: worst error %.3g of its tolerance (%.3g of the c + mu form)" % ((err / d_tol).max(), err.max()))
    assert (err <= d_tol).all()


def _hold(C, got):
    want = C["want"]
    for name in INTS:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
        assert got[name].dtype == np.int32
    for name in FLOATS:
        np.testing.assert_array_equal(np.isnan(got[name]), np.isnan(want[name]), err_msg=name)
        live = ~np.isnan(want[name])
        err, size = np.abs(got[name][live] - want[name][live]), np.abs(want[name][live])
        print("%s: worst relative error %.3g" % (name, (err[size > 0] / size[size > 0]).max() if (size > 0).any() else 0.0))
        assert (err <= RTOL * size).all(), name
    _hold_hat(C, got)
    rows = engine.nb_replacements(C["c"], C["cells"], C["s"], got["D"], C["cutoff"], got["trimmed_base"], C["min_replace"])
    assert [tuple(r) for r in rows.tolist()] == KR.replacements(C["c"], C["cells"], C["s"], want["D"], C["cutoff"], want["trimmed_base"],
                                                                 C["min_replace"])
    dead = np.isnan(C["alpha"]) | ~(C["c"] > 0).any(axis=0)
    assert np.isnan(got["D"][:, dead]).all() and np.isnan(got["H"][:, dead]).all() and (got["arg_max"][dead] == -1).all()
    assert not got["n_above"][dead].any() and not np.isnan(got["D"][:, ~dead]).any()
    return rows


@pytest.mark.parametrize("G", GENES)
@pytest.mark.parametrize("key", KR.DESIGN_KEYS, ids=str)
def test_design_cooks_against_the_restatement(key, G):
    C = _case(key, G)
    got = _run(np.ascontiguousarray(C["c"]), C)
    rows = _hold(C, got)
    without = _run(np.ascontiguousarray(C["c"]), C, distances=False)      # the full-table call: no D, no H, the same bits
    assert "D" not in without and "H" not in without
    for name in INTS + FLOATS:
        np.testing.assert_array_equal(without[name], got[name], err_msg=name)
    size = C["sizes"]
    if key[0] == "numeric":                                              # every cell one sample: the fallback variance, nothing to replace or flag
        assert np.isnan(got["max_cooks"]).all() and (got["arg_max"] == -1).all() and not got["n_replace"].any() and len(rows) == 0
        live = ~np.isnan(C["alpha"]) & (C["c"] > 0).any(axis=0)
        assert live[0] and not np.isnan(got["alpha_robust"][live]).any()
    else:
        small = size[C["cells"]] < 3
        live = ~np.isnan(got["max_cooks"])
        assert not small[got["arg_max"][live]].any()                     # a cell below 3 never holds the maximum
        if size.max() >= 7 and G > 2:
            assert len(rows) >= 1                                        # the planted outliers of a replaceable cell are found
        if size.max() < 7:
            assert len(rows) == 0 and not got["n_replace"].any()


def test_a_near_confounded_design_is_held_to_the_scaled_bound_only():
    """two design columns that nearly coincide: kappa about 1e8, so H and D are held to 100 p kappa 2^-53, about 1e-5, and nothing else"""
    X = KR.near_confounded_design(np.random.default_rng(5))
    C = KR.case(99, X, 24, max_cond=np.inf)
    kappa = C["want"]["kappa"]
    assert 5e7 < np.nanmin(kappa) and np.nanmax(kappa) < 1e9 and np.linalg.cond(X) < engine.NB_DESIGN_MAX_COND
    _hold_hat(C, _run(np.ascontiguousarray(C["c"]), C))


@pytest.mark.parametrize("key,G", [(("cells", (3, 7, 4, 6)), 63), (("cells", (64, 66)), 65), (("numeric", 8, 65), 65)], ids=str)
def test_same_bits_by_every_route(key, G):
    C = _case(key, G)
    c = C["c"]
    assert c.max() < 2 ** 24                                           # float32 holds every count
    first = _run(np.ascontiguousarray(c), C)
    wide = np.full((C["m"], G + 7), 3.0)
    wide[:, 3:3 + G] = c
    W = engine.DeviceMatrix.upload(wide)
    routes = {"again": np.ascontiguousarray(c), "float32": c.astype(np.float32), "device": engine.DeviceMatrix.upload(c),
              "device float32": engine.DeviceMatrix.upload(c.astype(np.float32)), "window": engine.device_columns(W, 3, 3 + G)}
    for name, Y in routes.items():
        other = _run(Y, C)
        for key_ in KEYS:
            np.testing.assert_array_equal(first[key_], other[key_], err_msg="%s: %s" % (name, key_))
    other = _run(engine.DeviceMatrix.upload(c), C, distances="device")   # D and H left in HBM
    for key_ in KEYS:
        np.testing.assert_array_equal(first[key_], other[key_], err_msg="D and H on the device: %s" % key_)
    for j in list(range(len(KR.CLASSES))) + [G - 1]:                      # a gene alone, as in its batch: one of every class
        alone = _run(engine.device_columns(W, 3 + j, 4 + j), C, slice(j, j + 1))
        for key_ in ("D", "H"):
            np.testing.assert_array_equal(first[key_][:, j:j + 1], alone[key_], err_msg="gene %d alone: %s" % (j, key_))
        for key_ in INTS + FLOATS:
            np.testing.assert_array_equal(first[key_][j:j + 1], alone[key_], err_msg="gene %d alone: %s" % (j, key_))


@pytest.mark.parametrize("sizes", [(3, 7), (2, 5), (64, 66)], ids=lambda s: "%dx%d" % s)
def test_one_factor_design_against_k25_on_the_device(sizes):
    """nb_design_cooks on [1, indicator] and nb_cooks on the same genes: the same integers and replacements, the floats within the
    ridge's pull (test_nb_design_cooks_args.hold_to_k25)"""
    C = KR.design_case(("cells", sizes))
    X, s, alpha, c = C["X"], C["s"], C["alpha"], np.ascontiguousarray(C["c"])
    codes = X[:, 1].astype(np.int32)
    np.testing.assert_array_equal(codes, C["cells"] if X[0, 1] == 0 else 1 - C["cells"])
    q, _ = engine.nb_group_fits(c, codes, 2, s, alpha)
    live = ~np.isnan(alpha) & (c > 0).any(axis=0)
    q[~live & ~np.isnan(alpha)] = 1.0                                  # (a gene of zeros: any positive q passes the check, the kernel leaves it out)
    k25 = engine.nb_cooks(c, codes, 2, s, alpha, q, C["cutoff"], return_distances=True)
    k25["D_scale"] = CR.cooks(c, codes, 2, s, alpha, q, C["cutoff"])["D_scale"]
    got = _run(c, C)
    pull = np.full(C["G"], np.nan)
    pull[live] = ridge_pull(X, s, alpha[live], C["beta"][live])
    print("worst share of the ridge bound: %.3g" % hold_to_k25(got, k25, pull))
    rows = engine.nb_replacements(c, C["cells"], s, got["D"], C["cutoff"], got["trimmed_base"])
    rows25 = engine.nb_replacements(c, codes, s, k25["D"], C["cutoff"], k25["trimmed_base"])
    assert rows.tolist() == rows25.tolist() and (len(rows) >= 1) == (max(sizes) >= 7)


def test_results_do_not_depend_on_the_scratch():
    """the workspace guard (tests/test_gpu_ws_guard.py) over the new call: it takes K22's slots and no new one"""
    C = _case(("cells", (3, 7, 4, 6)), 63)
    flat = lambda got: [np.asarray(got[key]) for key in KEYS]
    run = lambda: flat(_run(np.ascontiguousarray(C["c"]), C)) + flat(_run(C["c"].astype(np.float32), C, distances="device"))
    plain = run()
    with engine.ws_guard() as guard:
        guarded = run()
    assert guard.damage is None, guard.damage
    assert {"WS_NB_Y", "WS_NB_INT", "WS_NB_SF", "WS_NB_BAD", "WS_NB_PRIOR", "WS_NB_OUT", "WS_NB_FIT_INT"} <= guard.seen
    for a, b in zip(plain, guarded):
        assert a.tobytes() == b.tobytes()
    assert engine.ws_guard_report() == (set(), None)


def test_bad_counts():
    C = _case(("cells", (3, 7)), 63)
    for value, row, col in ((-1.0, 2, 5), (np.nan, 0, 62), (np.inf, 3, 0)):
        Y = np.array(C["c"])
        Y[row, col] = value
        with pytest.raises(ValueError, match=r"Y\[%d, %d\]" % (row, col)) as err:
            _run(Y, C)
        assert (err.value.row, err.value.col) == (row, col)


# ---- tl ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frames(n, test):
    counts, meta, planted = planted_table_with_batch(n, n, G=40)
    plain = tl.compute_pseudobulk_DE(counts, meta, covariates=["batch"], test=test, **ARGS)
    return counts, meta, planted, plain, tl.outliers_design(counts, plain)


@pytest.mark.parametrize("test,n", [("wald", 7), ("wald", 14), ("lrt", 14)], ids=["wald-flaggable", "wald-replaceable", "lrt-replaceable"])
def test_outliers_design_is_the_host_tail_of_the_engine_calls(test, n):
    counts, meta, planted, plain, out = _frames(n, test)
    assert list(plain.attrs["design"].columns) == ["Intercept", "batch_B", "Predicted_Labels_T2_vs_T1"]
    sizes = np.bincount(engine.nb_design_cells(plain.attrs["design"].to_numpy())[0])
    assert sorted(sizes) == ([3, 3, 4, 4] if n == 7 else [7, 7, 7, 7])
    hold_outliers_frame(out, plain, counts, planted, replaceable=n >= 14)
    assert out.attrs["n_not_converged"] == 0
    both = tl.outliers_design(counts, plain, independent_filtering=True, alpha=0.1)
    assert "independent_filtering" in both.attrs and both["cooksOutlier"].sum() == out["cooksOutlier"].sum()
    table = tl.deseq2_cooks_design(counts, out)
    assert list(table.index) == list(counts.columns) and table.attrs["cooks_cutoff"] == out.attrs["cooks_cutoff"]
    if n < 14:
        np.testing.assert_array_equal(table["max_cooks"].to_numpy(), out.set_index("gene").loc[counts.columns, "maxCooks"].to_numpy())
        for g, samples in planted.items():
            assert table.loc[g, "arg_max"] == samples[0]


def test_a_clean_table_returns_the_old_columns_bit_for_bit():
    counts, meta, _ = planted_table_with_batch(7, 7, G=40)
    clean = counts.drop(columns=["g003", "g017", "g020", "g025", "g030"])
    plain = tl.compute_pseudobulk_DE(clean, meta, covariates=["batch"], **ARGS)
    out = tl.outliers_design(clean, plain)
    assert not out["replace"].any() and not out["cooksOutlier"].any() and len(out.attrs["replaced"]) == 0
    pd.testing.assert_frame_equal(out[list(plain.columns)], plain, check_exact=True)
    pd.testing.assert_frame_equal(out.attrs["dispersions"], plain.attrs["dispersions"], check_exact=True)
    pd.testing.assert_frame_equal(out.attrs["coefficients"], plain.attrs["coefficients"], check_exact=True)


def test_lfc_shrink_design_after_the_outliers_fits_the_replaced_counts():
    counts, meta, planted, plain, out = _frames(14, "wald")
    assert len(out.attrs["replaced"]) >= 3
    shrunk = tl.lfc_shrink_design(counts, out)
    by_hand = counts.copy()
    for gene, sample, was, value in out.attrs["replaced"].itertuples(index=False):
        assert by_hand.loc[sample, gene] == was
        by_hand.loc[sample, gene] = value
    bare = out.copy()
    bare.attrs = {k: v for k, v in out.attrs.items() if k != "replaced"}
    want = tl.lfc_shrink_design(by_hand, bare)
    pd.testing.assert_frame_equal(shrunk, want, check_exact=True)
    assert shrunk.attrs["prior_scale"] == want.attrs["prior_scale"]
    at = shrunk.set_index("gene")
    assert np.isnan(at.loc["g025", "log2FoldChange"]) and abs(at.loc["g003", "log2FoldChange"]) < 0.5
