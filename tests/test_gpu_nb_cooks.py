"""Cook's distances on the device (K25, pilot_ot_nb_cooks) against the numpy restatement (tests/nb_cooks_restatement.py: np.sort
and fsum where the device sorts in LDS and closes a butterfly, the hat diagonal from the explicit design matrix), given the SAME
group fits q and dispersions, and tl.compute_pseudobulk_DE(outliers=..., independent_filtering=...) against its host tail written
out from the engine calls (test_nb_cooks_args.py: outliers_by_hand).

Tolerances.  The integers -- arg_max, n_above, n_replace, which counts are replaced and by what -- are exact: the generator keeps
only genes whose distances stay 1e-6 (relative) clear of the cutoff and whose replacements stay 1e-9 clear of an integer, both
checked on the restatement when the case is built.  alpha_robust, max_cooks and trimmed_base to 1e-10 relative: the sums are at
most m = 4096 terms of one sign, m 2^-53 <= 4.5e-13, with a margin of about 200 for the chained operations.  Each D_j to 1e-10 of
the same expression with |c - mu| replaced by c + mu: the conditioning of that subtraction (mu comes from the same q on both
sides, so this bounds the rounding of the rest)."""
import functools

import numpy as np
import pandas as pd
import pytest

import nb_cooks_restatement as CR
import nb_glm_restatement as RR
from pilot_amd import engine, tl
from test_nb_cooks_args import check_planted, frozen_fit_is_the_identity, outliers_by_hand, planted_table

pytestmark = pytest.mark.gpu

RTOL = 1e-10
SIZES = [(2, 5), (3, 3), (3, 7), (4, 6), (7, 7), (23, 24), (1, 63), (32, 32), (64, 66)]
GENES = (1, 63, 65)
INTS = ("arg_max", "n_above", "n_replace")
FLOATS = ("alpha_robust", "max_cooks", "trimmed_base")


@functools.lru_cache(maxsize=None)
def _case(sizes, G):
    return CR.case(1000 * sum(sizes) + 7 * len(sizes) + G, sizes, G)


def _run(Y, C, cols=slice(None), distances=True):
    got = engine.nb_cooks(Y, C["codes"], C["k"], C["s"], C["alpha"][cols], C["q"][cols], C["cutoff"], C["min_replace"],
                          return_distances=distances)
    if isinstance(got.get("D"), engine.DeviceMatrix):
        got["D"] = engine.download(got["D"])
    return got


def _hold(C, got):
    want = C["want"]
    for name in INTS:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
        assert got[name].dtype == np.int32
    for name in FLOATS:
        np.testing.assert_array_equal(np.isnan(got[name]), np.isnan(want[name]), err_msg=name)
        live = ~np.isnan(want[name])
        err, size = np.abs(got[name][live] - want[name][live]), np.abs(want[name][live])      # (a trimmed mean of zeros is 0 on both sides)
        print("%s: worst relative error %.3g" % (name, (err[size > 0] / size[size > 0]).max() if (size > 0).any() else 0.0))
        assert (err <= RTOL * size).all(), name
    D, Dw, scale = got["D"], want["D"], want["D_scale"]
    np.testing.assert_array_equal(np.isnan(D), np.isnan(Dw))
    live = ~np.isnan(Dw)
    if live.any():
        err = np.abs(D[live] - Dw[live]) / scale[live]
        print("D: worst error %.3g of the c + mu form" % err.max())
        assert (err <= RTOL).all()
    rows = engine.nb_replacements(C["c"], C["codes"], C["s"], D, C["cutoff"], got["trimmed_base"], C["min_replace"])
    assert [tuple(r) for r in rows.tolist()] == CR.replacements(C["c"], C["codes"], C["s"], Dw, C["cutoff"], want["trimmed_base"],
                                                                 C["min_replace"])
    dead = np.isnan(C["alpha"]) | ~(C["c"] > 0).any(axis=0)
    assert np.isnan(D[:, dead]).all() and (got["arg_max"][dead] == -1).all() and not got["n_above"][dead].any()
    return rows


@pytest.mark.parametrize("G", GENES)
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "%dx%d" % s)
def test_cooks_against_the_restatement(sizes, G):
    C = _case(sizes, G)
    got = _run(np.ascontiguousarray(C["c"]), C)
    rows = _hold(C, got)
    without = _run(np.ascontiguousarray(C["c"]), C, distances=False)      # the full-table call: no D, the same bits
    assert "D" not in without
    for name in INTS + FLOATS:
        np.testing.assert_array_equal(without[name], got[name], err_msg=name)
    size = np.bincount(C["codes"])
    if size.min() < 3 <= size.max() and G > 2:
        assert np.isnan(got["D"][size[C["codes"]] == 1]).all()           # a group of one has no distance
        small = size[C["codes"]] < 3
        live = ~np.isnan(got["max_cooks"])
        assert not small[got["arg_max"][live]].any()                     # and a group below 3 never holds the maximum
    if size.max() >= 7 and G > 2:
        assert len(rows) >= 1                                            # the planted outliers of a replaceable group are found
    if size.max() < 7:
        assert len(rows) == 0 and not got["n_replace"].any()


def test_classes_behave_as_described():
    C = _case((3, 7), 63)
    got, kind = C["want"], C["kind"]
    name = lambda n: kind == CR.CLASSES.index(n)
    assert (got["n_replace"][name("two outliers")] >= 1).any() and (got["n_replace"][name("outlier in a replaceable group")] == 1).all()
    assert (got["n_replace"][name("outlier in a flaggable group")] == 0).all()
    assert (got["max_cooks"][name("outlier in a flaggable group")] > C["cutoff"]).all()
    assert (got["n_above"][name("planted zero")] >= 3).all()
    assert np.isnan(got["max_cooks"][name("zeros") | name("nan dispersion")]).all()
    assert (got["trimmed_base"][name("single count")] == 0).all()


def test_three_groups():
    C = _case((3, 4, 7), 63)
    _hold(C, _run(np.ascontiguousarray(C["c"]), C))


def test_no_group_of_three():
    """two groups of 2: trimmed_base only"""
    C = _case((2, 2), 9)
    got = _run(np.ascontiguousarray(C["c"]), C)
    _hold(C, got)
    assert np.isnan(got["max_cooks"]).all() and np.isnan(got["D"]).all() and (got["arg_max"] == -1).all()
    assert not np.isnan(got["trimmed_base"][:7]).any()


@pytest.mark.parametrize("sizes,G", [((3, 7), 63), ((64, 66), 65)], ids=["3x7", "64x66"])
def test_same_bits_by_every_route(sizes, G):
    C = _case(sizes, G)
    c = C["c"]
    assert c.max() < 2 ** 24                                           # float32 holds every count
    keys = INTS + FLOATS + ("D",)
    first = _run(np.ascontiguousarray(c), C)
    wide = np.full((C["m"], G + 7), 3.0)
    wide[:, 3:3 + G] = c
    W = engine.DeviceMatrix.upload(wide)
    routes = {"again": np.ascontiguousarray(c), "float32": c.astype(np.float32), "device": engine.DeviceMatrix.upload(c),
              "device float32": engine.DeviceMatrix.upload(c.astype(np.float32)), "window": engine.device_columns(W, 3, 3 + G)}
    for name, Y in routes.items():
        other = _run(Y, C)
        for key in keys:
            np.testing.assert_array_equal(first[key], other[key], err_msg="%s: %s" % (name, key))
    other = _run(engine.DeviceMatrix.upload(c), C, distances="device")   # D left in HBM
    for key in keys:
        np.testing.assert_array_equal(first[key], other[key], err_msg="D on the device: %s" % key)
    for j in list(range(len(CR.CLASSES))) + [G - 1]:                      # a gene alone, as in its batch: one of every class
        alone = _run(engine.device_columns(W, 3 + j, 4 + j), C, slice(j, j + 1))
        np.testing.assert_array_equal(first["D"][:, j:j + 1], alone["D"], err_msg="gene %d alone" % j)
        for key in INTS + FLOATS:
            np.testing.assert_array_equal(first[key][j:j + 1], alone[key], err_msg="gene %d alone: %s" % (j, key))


def test_results_do_not_depend_on_the_scratch():
    """the workspace guard (tests/test_gpu_ws_guard.py) over the new call: it takes K22's slots and no new one"""
    C = _case((4, 6), 63)
    flat = lambda got: [np.asarray(got[key]) for key in INTS + FLOATS + ("D",)]
    run = lambda: flat(_run(np.ascontiguousarray(C["c"]), C)) + flat(_run(C["c"].astype(np.float32), C, distances="device"))
    plain = run()
    with engine.ws_guard() as guard:
        guarded = run()
    assert guard.damage is None, guard.damage
    assert {"WS_NB_Y", "WS_NB_INT", "WS_NB_SF", "WS_NB_BAD", "WS_NB_PRIOR", "WS_NB_OUT", "WS_NB_FIT_INT"} <= guard.seen
    for a, b in zip(plain, guarded):
        assert a.tobytes() == b.tobytes()
    assert engine.ws_guard_report() == (set(), None)


def test_the_largest_sample_count():
    """m = the limit, two groups: the whole LDS layout (counts, normalised counts, a 4096-entry sort buffer)"""
    m = engine.nb_glm_limits()
    C = _case((m - 1500, 1500), 2)
    _hold(C, _run(np.ascontiguousarray(C["c"]), C))
    with pytest.raises(NotImplementedError):
        engine.nb_cooks(np.ones((m + 1, 1)), np.arange(m + 1) % 2, 2, np.ones(m + 1), np.full(1, 0.1), np.ones((1, 2)), 3.0)


def test_bad_counts():
    C = _case((4, 6), 63)
    for value, row, col in ((-1.0, 2, 5), (np.nan, 0, 62), (np.inf, 3, 0)):
        Y = np.array(C["c"])
        Y[row, col] = value
        with pytest.raises(ValueError, match=r"Y\[%d, %d\]" % (row, col)) as err:
            _run(Y, C)
        assert (err.value.row, err.value.col) == (row, col)


# ---- tl ---------------------------------------------------------------------------------------------------------------------------
ARGS = dict(group1="T1", group2="T2", cluster_col="Predicted_Labels")


@functools.lru_cache(maxsize=None)
def _frames(n0, n1):
    counts, meta, planted = planted_table(n0, n1)
    plain = tl.compute_pseudobulk_DE(counts, meta, **ARGS)
    return counts, meta, planted, plain, tl.compute_pseudobulk_DE(counts, meta, outliers="deseq2", **ARGS)


@pytest.mark.parametrize("n0,n1", [(5, 5), (8, 8)])
def test_compute_pseudobulk_DE_with_outliers_is_the_host_tail_of_the_engine_calls(n0, n1):
    counts, meta, planted, plain, out = _frames(n0, n1)
    assert list(plain.columns) == ["gene", "baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "padj", "dispersion"]
    assert not {"cooks_cutoff", "replaced", "independent_filtering"} & set(plain.attrs)
    default = tl.compute_pseudobulk_DE(counts, meta, outliers=None, independent_filtering=False, **ARGS)
    pd.testing.assert_frame_equal(default, plain, check_exact=True)
    assert list(out.columns) == list(plain.columns) + ["maxCooks", "cooksOutlier", "replace"]
    want, rows = outliers_by_hand(counts, meta, plain)
    pd.testing.assert_frame_equal(out, want, check_exact=True)
    assert [tuple(r) for r in out.attrs["replaced"].itertuples(index=False)] == rows
    assert out.attrs["cooks_cutoff"] == CR.cutoff(n0 + n1, 2) and out.attrs["n_not_converged"] == 0
    check_planted(out, plain, planted, replaceable=n0 >= 7)
    both = tl.compute_pseudobulk_DE(counts, meta, outliers="deseq2", independent_filtering=True, alpha=0.1, **ARGS)
    pd.testing.assert_frame_equal(both, outliers_by_hand(counts, meta, plain, True, 0.1)[0], check_exact=True)
    alone = tl.compute_pseudobulk_DE(counts, meta, independent_filtering=True, **ARGS)
    pd.testing.assert_frame_equal(alone, tl.independent_filtering(plain), check_exact=True)
    assert list(alone.columns) == list(plain.columns) and "independent_filtering" in alone.attrs


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_frozen_fit_of_the_same_counts_is_the_first_fit(monkeypatch, dtype):
    # 8 + 8 samples x 60 genes: the smallest table of the suite with a replaceable group (min_replace = 7), genes of zeros included
    counts, meta, _ = planted_table(8, 8, G=60)
    frozen_fit_is_the_identity(counts.astype(dtype), meta, monkeypatch)


def test_lfc_shrink_with_outliers_is_lfc_shrink_on_the_replaced_counts():
    counts, meta, planted, plain, out = _frames(8, 8)
    shrunk = tl.compute_pseudobulk_DE(counts, meta, outliers="deseq2", shrink="apeglm", **ARGS)
    codes = (meta["Predicted_Labels"] == "T2").to_numpy()
    by_hand = counts.copy()
    for gene, sample, was, value in out.attrs["replaced"].itertuples(index=False):
        assert by_hand.loc[sample, gene] == was
        by_hand.loc[sample, gene] = value
    bare = out.copy()
    bare.attrs = {k: v for k, v in out.attrs.items() if k != "replaced"}
    want = tl.lfc_shrink(by_hand, codes, bare)
    pd.testing.assert_frame_equal(shrunk, want, check_exact=True)
    assert shrunk.attrs["prior_scale"] == want.attrs["prior_scale"]
    at = shrunk.set_index("gene")
    assert np.isnan(at.loc["g025", "log2FoldChange"]) and abs(at.loc["g003", "log2FoldChange"]) < 0.5


def test_deseq2_cooks_table():
    counts, meta, planted, plain, out = _frames(5, 5)
    codes = (meta["Predicted_Labels"] == "T2").to_numpy()
    table = tl.deseq2_cooks(counts, codes, plain)
    assert list(table.columns) == ["alpha_robust", "max_cooks", "arg_max", "n_above", "n_replace", "trimmed_base"]
    at = out.set_index("gene").loc[counts.columns]
    np.testing.assert_array_equal(table["max_cooks"].to_numpy(), at["maxCooks"].to_numpy())
    for g, samples in planted.items():
        assert table.loc[g, "arg_max"] == samples[0]
