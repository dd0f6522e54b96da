"""Gene curve clustering (K11), the parts that need no device: the restatement (tests/curves_restatement.py) against the
reference-executed fixture tests/golden/gene_curves_1type.npz, the host restatement of fcluster, and the argument errors of the
engine and tl functions, all raised before any device work."""
import numpy as np
import pandas as pd
import pytest
import scipy.cluster.hierarchy as sch

import curves_restatement as CR
import gene_curves_helpers as H
from pilot_amd import _lib, engine, tl


def test_restatement_reproduces_the_reference_fixture():
    """The fixture stores the reference's inputs as it read them back from its CSV files, so the restatement sees identical
    arrays.  Measured here on the CPU: max |restatement - fixture| = 0.0 for the scaled curves, the scaled noised curves and
    every activity column, and the clusters are equal -- the restatement IS the reference on these inputs, bit for bit.  Ten
    times that is still 0, so the comparison is exact; the device tests then hold the engine to the fixture with the bound they
    use against the restatement (1e-12)."""
    g = H.load()
    sel, times, sd, params, models = H.restated_inputs(g)
    assert list(sel["Gene ID"]) == list(g["selected"])
    assert set(models) == set(CR.MODELS)
    assert np.isnan(sd).any(axis=1).sum() == 1                    # the time point with a single cell
    assert np.array_equal(times, g["times"])
    sc, sn = CR.noised_curves(params, models, times, sd)
    d_curves, d_noised = np.abs(sc - g["scaled_curves"]).max(), np.abs(sn - g["scaled_noised_curves"]).max()
    print("restatement vs fixture: curves %.3e, noised %.3e" % (d_curves, d_noised))
    assert d_curves == 0.0 and d_noised == 0.0
    assert (sn == 0.0).all(axis=1).sum() == 1                     # the constant gene: scale 0 became 1
    for sv, key in ((0.4, "clusters_040"), (0.65, "clusters_065")):
        assert np.array_equal(CR.clusters(sn, "complete", sv), g[key]) and len(set(g[key])) > 1
    act = CR.activities(sn, times, g["clusters_040"])
    for k, v in act.items():
        assert np.array_equal(v, g["act_" + k]), k


def test_fixture_filters_remove_genes():
    g = H.load()
    tab = H.table(g).fillna(0)
    low, high = np.abs(tab["R-squared"]) < float(g["thr"]), tab["adjusted P-value"] > float(g["pthr"])
    assert (low & ~high).any() and (high & ~low).any()
    assert tab.shape[0] - (low | high).sum() == len(g["selected"])


@pytest.mark.parametrize("method", ["complete", "average", "weighted", "single"])
def test_flat_clusters_is_fcluster(method):
    rng = np.random.default_rng(5)
    for n in (2, 3, 7, 60, 400):
        X = rng.standard_normal((n, 9))
        d = sch.distance.pdist(X)
        Z = sch.linkage(d, method)
        for f in (0.0, 0.1, 0.4, 0.65, 0.99, 1.0, 1.2):
            assert np.array_equal(engine.flat_clusters(Z, f * d.max()), sch.fcluster(Z, f * d.max(), "distance")), (n, f)
    with pytest.raises(ValueError):
        engine.flat_clusters(np.zeros((3, 3)), 1.0)


@pytest.mark.parametrize("method", ["centroid", "median", "ward"])
def test_unsupported_methods_raise_before_device_work(method):
    curves = pd.DataFrame(np.random.default_rng(0).standard_normal((5, 4)), index=list("abcde"))
    with pytest.raises(NotImplementedError):
        engine.linkage_of_rows(curves.to_numpy(), method)
    with pytest.raises(NotImplementedError):
        tl.cluster_genes_curves(curves, cluster_method=method)
    with pytest.raises(NotImplementedError):
        tl.genes_selection_analysis(None, "alpha", None, cluster_method=method)
    with pytest.raises(ValueError):
        tl.cluster_genes_curves(curves, cluster_method="no-such-method")


def test_linkage_shape_errors():
    with pytest.raises(ValueError):
        engine.linkage_of_rows(np.zeros((1, 4)))
    with pytest.raises(ValueError):
        engine.linkage_of_rows(np.full((3, 4), np.nan))
    L = _lib.load()
    Y, Z = np.zeros((4, 3)), np.zeros((3, 4))
    big = _lib.LINKAGE_MAX_G + 1
    assert L.pilot_ot_linkage_of_rows(Y.ctypes.data, 0, big, 3, 1, _lib.dptr(Z), None, None) == _lib.EINVAL
    assert b"HBM" in L.pilot_ot_last_error()
    assert L.pilot_ot_linkage_of_rows(Y.ctypes.data, 0, 4, 3, 7, _lib.dptr(Z), None, None) == _lib.ENOTSUP
    assert L.pilot_ot_linkage_of_rows(Y.ctypes.data, 0, 1, 3, 1, _lib.dptr(Z), None, None) == _lib.EINVAL


@pytest.mark.parametrize("times", [[1.0], [1.0, 1.0, 2.0], [1.0, 3.0, 2.0], []])
def test_times_must_increase(times):
    curves = pd.DataFrame(np.zeros((3, len(times))), index=list("abc"))
    names = pd.DataFrame({"sampleID": ["s"] * len(times)}, index=pd.Index(times, name="Time_score", dtype=np.float64))
    clusters = pd.DataFrame({"Gene ID": list("abc"), "cluster": [1, 1, 1]})
    with pytest.raises(ValueError, match="increasing"):
        engine.curve_activities(curves.to_numpy().reshape(3, len(times)), times)
    with pytest.raises(ValueError, match="increasing"):
        tl.compute_curves_activities(curves, clusters, names)
    with pytest.raises(ValueError, match="increasing"):
        CR.activities_raw(curves.to_numpy().reshape(3, len(times)), np.asarray(times))
    out = np.zeros((3, 4))
    t = np.asarray(times + [0.0], dtype=np.float64)              # (never empty for the pointer)
    rc = _lib.load().pilot_ot_curve_activities(out.ctypes.data, 0, 3, len(times), _lib.dptr(t), _lib.dptr(out))
    assert rc == _lib.EINVAL


@pytest.mark.parametrize("n", [0, 1])
def test_fewer_than_two_genes_is_one_cluster(n):
    curves = pd.DataFrame(np.zeros((n, 5)), index=["g%d" % i for i in range(n)])
    out = tl.cluster_genes_curves(curves)                         # no device call: the reference's except ValueError path
    assert list(out.columns) == ["Gene ID", "cluster"] and list(out["cluster"]) == [1] * n
    assert list(CR.clusters(curves.to_numpy())) == [1] * n


def test_segment_std_and_curve_argument_errors():
    L = _lib.load()
    Y, out = np.zeros((4, 3)), np.zeros((2, 3))
    off = np.array([0, 3, 2], dtype=np.int64)
    lp = off.ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_longlong))
    assert L.pilot_ot_segment_std(Y.ctypes.data, 0, 1, 4, 3, 3, lp, 2, None, 3, out.ctypes.data, 0) == _lib.EINVAL
    assert b"decrease" in L.pilot_ot_last_error()
    off[:] = [0, 2, 5]
    assert L.pilot_ot_segment_std(Y.ctypes.data, 0, 1, 4, 3, 3, lp, 2, None, 3, out.ctypes.data, 0) == _lib.EINVAL
    with pytest.raises(ValueError):
        engine.fitted_curves(np.zeros((3, 2)), [0, 1, 2], [1.0, 2.0])
    with pytest.raises(ValueError):
        engine.fitted_curves(np.zeros((3, 3)), [0, 1], [1.0, 2.0])
    with pytest.raises(ValueError):
        engine.fitted_curves(np.zeros((3, 3)), [0, 1, 5], [1.0, 2.0])
    with pytest.raises(ValueError):
        engine.fitted_curves(np.zeros((2, 3)), ["linear", "quadratic"], [1.0, 2.0], noise=np.zeros((3, 2)))


def test_table_without_treat2_is_read_as_zero():
    """genes_importance drops Treat2 when no fit has three coefficients; the reference raises KeyError on such a table, this
    package reads Treat2 = 0.  Without a device the call gets past the table and fails in the device call, loudly."""
    g = H.load()
    adata = H.adata(g)
    tab = H.table(g)
    tab = tab[tab["Fitted function"] != "linear_quadratic"].drop(columns="Treat2")
    if _lib.device_count() > 0:
        curves, noised, names = tl.get_noised_curves(adata, str(g["cell"]), tab, normalize=False)
        assert curves.shape[0] == noised.shape[0] > 0
    else:
        with pytest.raises(_lib.PilotOTError):
            tl.get_noised_curves(adata, str(g["cell"]), tab, normalize=False)
