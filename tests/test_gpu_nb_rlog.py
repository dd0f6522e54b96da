"""The regularised log transform on the device (K24: engine.nb_dispersions_blind, engine.nb_rlog, tl.rlog,
tl.compute_pseudobulk_PCA, tl.pseudobulk_pca) against the numpy / scipy restatement (tests/nb_rlog_restatement.py, itself pinned
to scipy in test_nb_rlog_args.py).

Cases: m in {2, 3, 63, 64, 65, 130} samples (one partial wave, exactly one, wrap by one, two full passes plus two), G in
{1, 63, 65} genes, prior variance in {1e-3, 0.05, 1, 50}; every value of each appears, m = 65 with every prior variance.  Gene
classes, dealt round-robin (nb_rlog_restatement.gene_classes), the dispersions given as inputs: NB (K22's generator), alpha =
minDisp, alpha = 10, means of 2e6, a single non-zero count of 1 .. 40, a single 50 000 among zeros, mean 0.3, all zero, a NaN
dispersion.

Parity, for EVERY live gene: P is strictly concave, so the device's point is held to the optimum itself, not to a path.  (1) The
restatement's dense Newton step at the device's (beta0, beta) is <= 1e-9 in every coordinate; (2) rlog and intercept are within
1e-8 of the restatement's dense-Newton optimum (whose own residual is <= 1e-12).  Both margins are over the device's 1e-10 stopping
rule under quadratic convergence.  flags are zero, steps <= 40 (the restatement of the same iteration needs <= 16: a condition
on the generator).  All-zero genes give 0 and a NaN intercept, NaN-dispersion genes NaN.  The measured residual of every class is
printed.  The tl frames must equal, bit for bit, the host tail recomputed here from the engine calls."""
import functools

import numpy as np
import pandas as pd
import pytest

import nb_glm_restatement as RR
import nb_rlog_restatement as LR
from pilot_amd import engine, tl
from test_gpu_nb_shrink import _Adata, _pseudobulk

pytestmark = pytest.mark.gpu

CASES = [(2, 63, 1.0), (3, 1, 0.05), (63, 65, 1e-3), (64, 63, 50.0), (65, 63, 1e-3), (65, 65, 0.05), (65, 63, 1.0), (65, 65, 50.0),
         (130, 65, 1.0)]


@functools.lru_cache(maxsize=None)
def _case(m, G, prior_var):
    rng = np.random.default_rng(1000 * m + G)
    s = RR.size_factors(rng, m)
    c, alpha, kind = LR.gene_classes(rng, s, G)
    want, intercept, left = LR.dense_rlog(c, s, alpha, prior_var)
    assert left.max() <= 1e-12                                          # the reference is at its own optimum
    for a in (c, s, alpha, kind, want, intercept):
        a.flags.writeable = False
    return dict(m=m, G=G, pv=prior_var, c=c, s=s, alpha=alpha, kind=kind, want=want, intercept=intercept)


def _ids(case):
    return "m%d-G%d-pv%g" % case


def _hold(c, s, alpha, prior_var, got, info, step_at, want=None, kind=None):
    """the two parity conditions, the flags and the genes left out; step_at(genes) -> the largest Newton step left at each"""
    dead = np.isnan(alpha)
    zero = ~dead & (c == 0).all(axis=0)
    live = np.flatnonzero(~dead & ~zero)
    assert np.isnan(got[:, dead]).all() and np.isnan(info["intercept"][dead]).all()
    assert (got[:, zero] == 0).all() and np.isnan(info["intercept"][zero]).all()
    assert not info["steps"][dead | zero].any() and not info["flags"].any() and info["n_not_converged"] == 0
    if not live.size:
        return
    assert np.isfinite(got[:, live]).all() and np.isfinite(info["intercept"][live]).all()
    assert (info["steps"][live] >= 1).all() and info["steps"][live].max() <= 40, info["steps"].max()
    left = step_at(live)
    off = np.zeros(live.size) if want is None else np.maximum(np.abs(got[:, live] - want[0][:, live]).max(axis=0),
                                                              np.abs(info["intercept"][live] - want[1][live]))
    classes = {"all": np.ones(live.size, dtype=bool)} if kind is None else {LR.CLASSES[k]: kind[live] == k for k in np.unique(kind[live])}
    print()
    for name, sel in classes.items():
        print("%-13s %3d genes: Newton step left %.3g, off the optimum by %.3g log2 units, at most %d iterations"
              % (name, sel.sum(), left[sel].max(), off[sel].max(), info["steps"][live][sel].max()))
    assert (left <= 1e-9).all(), left.max()
    assert (off <= 1e-8).all(), off.max()


# ---- engine.nb_rlog ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_rlog_against_the_restatement(case):
    C = _case(*case)
    c, s, alpha, pv = C["c"], C["s"], C["alpha"], C["pv"]
    got, info = engine.nb_rlog(c, s, alpha, pv, return_info=True)
    assert got.shape == c.shape and got.dtype == np.float64
    _hold(c, s, alpha, pv, got, info, lambda genes: LR.dense_step_at(c, s, alpha, pv, got, info["intercept"], genes),
          (C["want"], C["intercept"]), C["kind"])
    np.testing.assert_array_equal(engine.nb_rlog(c, s, alpha, pv), got)


def _all(Y, C, cols=slice(None), **kw):
    out, info = engine.nb_rlog(Y, C["s"], C["alpha"][cols], C["pv"], return_info=True, **kw)
    if isinstance(out, engine.DeviceMatrix):
        out = engine.download(out)
    return [out, info["intercept"], info["steps"], info["flags"]]


@pytest.mark.parametrize("case", [CASES[0], CASES[5]], ids=_ids)
def test_same_bits_by_every_route(case):
    C = _case(*case)
    c, G = C["c"], C["G"]
    assert c.max() < 2 ** 24                                           # float32 holds every count
    first = _all(np.ascontiguousarray(c), C)
    wide = np.full((C["m"], G + 7), 3.0)
    wide[:, 3:3 + G] = c
    D = engine.DeviceMatrix.upload(wide)
    routes = {"again": np.ascontiguousarray(c), "float32": c.astype(np.float32), "device": engine.DeviceMatrix.upload(c),
              "device float32": engine.DeviceMatrix.upload(c.astype(np.float32)), "window": engine.device_columns(D, 3, 3 + G)}
    for name, Y in routes.items():
        for a, b in zip(first, _all(Y, C)):
            np.testing.assert_array_equal(a, b, err_msg=name)
    for a, b in zip(first, _all(engine.DeviceMatrix.upload(c.astype(np.float32)), C, on_device=True)):
        np.testing.assert_array_equal(a, b, err_msg="on_device")
    for j in (0, 8, G - 1):                                            # a gene alone, as in its batch
        alone = _all(engine.device_columns(D, 3 + j, 4 + j), C, slice(j, j + 1))
        np.testing.assert_array_equal(first[0][:, j:j + 1], alone[0], err_msg="gene %d alone" % j)
        for a, b in zip(first[1:], alone[1:]):
            np.testing.assert_array_equal(a[j:j + 1], b, err_msg="gene %d alone" % j)


def test_results_do_not_depend_on_the_scratch():
    """the workspace guard (tests/test_gpu_ws_guard.py) over the two new calls: they take K22's slots and no new one"""
    C = _case(*CASES[2])
    run = lambda: engine.nb_dispersions_blind(C["c"], C["s"], return_info=True) + tuple(_all(np.ascontiguousarray(C["c"]), C)) \
        + tuple(_all(C["c"].astype(np.float32), C, on_device=True))
    plain = run()
    with engine.ws_guard() as guard:
        guarded = run()
    assert guard.damage is None, guard.damage
    assert {"WS_NB_Y", "WS_NB_INT", "WS_NB_SF", "WS_NB_BAD", "WS_NB_PRIOR", "WS_NB_OUT", "WS_NB_FIT_INT"} <= guard.seen
    flat = lambda r: [np.asarray(a) for x in r for a in (x.values() if isinstance(x, dict) else [x])]
    for a, b in zip(flat(plain), flat(guarded)):
        assert a.tobytes() == b.tobytes()
    assert engine.ws_guard_report() == (set(), None)


# ---- limits and refusals ----------------------------------------------------------------------------------------------------------
def test_the_largest_sample_count():
    """m = the limit: the whole LDS layout, four genes (NB, NB at minDisp, a single count, all zero), held by the residual with the
    restatement's vectorised arrowhead step (itself held to the dense form at m <= 130 in test_nb_rlog_args.py)"""
    m = engine.nb_glm_limits()
    rng = np.random.default_rng(24)
    s = RR.size_factors(rng, m)
    c = RR.nb_class(rng, s, np.zeros(m, dtype=np.int64), 1, 4)
    alpha = np.clip(0.05 + 2.0 / np.maximum((c / s[:, None]).mean(axis=0), 1.0), RR.MIN_DISP, 10.0)
    alpha[1] = RR.MIN_DISP
    c[:, 2] = 0.0
    c[rng.integers(m), 2] = 17.0
    c[:, 3] = 0.0
    got, info = engine.nb_rlog(c, s, alpha, 1.0, return_info=True)

    def step_at(genes):
        d0, d = LR.arrowhead_step(c[:, genes], s, alpha[genes], 1.0, *LR.coefficients(got[:, genes], info["intercept"][genes]))
        return np.maximum(np.abs(d0), np.abs(d).max(axis=0))

    _hold(c, s, alpha, 1.0, got, info, step_at)
    ref = LR.arrowhead_rlog(c, s, alpha, 1.0)
    assert np.abs(got - ref["rlog"]).max() <= 1e-8
    with pytest.raises(NotImplementedError):
        engine.nb_rlog(np.ones((m + 1, 2)), np.ones(m + 1), np.full(2, 0.1), 1.0)
    with pytest.raises(NotImplementedError):
        engine.nb_dispersions_blind(np.ones((m + 1, 2)), np.ones(m + 1))


def test_bad_counts_and_left_out_genes():
    C = _case(*CASES[4])
    for value, row, col in ((-1.0, 2, 5), (np.nan, 0, 62), (np.inf, 1, 0), (-0.6, 1, 1)):
        Y = np.array(C["c"])
        Y[row, col] = value
        with pytest.raises(ValueError, match=r"Y\[%d, %d\]" % (row, col)) as err:
            engine.nb_rlog(Y, C["s"], C["alpha"], C["pv"])
        assert (err.value.row, err.value.col) == (row, col)
        with pytest.raises(ValueError, match=r"Y\[%d, %d\]" % (row, col)) as err:
            engine.nb_dispersions_blind(Y, C["s"])
        assert (err.value.row, err.value.col) == (row, col)
    alpha = np.array(C["alpha"])
    alpha[[0, 4]] = np.nan                                              # a NaN dispersion leaves its gene out, whatever its counts
    got, info = engine.nb_rlog(C["c"], C["s"], alpha, C["pv"], return_info=True)
    np.testing.assert_array_equal(np.isnan(got).all(axis=0), np.isnan(alpha))
    keep = ~np.isnan(alpha)
    np.testing.assert_array_equal(got[:, keep], engine.nb_rlog(C["c"], C["s"], C["alpha"], C["pv"])[:, keep])


# ---- engine.nb_dispersions_blind --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 12, 65])
def test_blind_dispersions_against_the_restatement(m):
    """K22's two-part criterion with one group: the objective of every gene, the dispersion of the resolved ones"""
    rng = np.random.default_rng(300 + m)
    s = RR.size_factors(rng, m)
    c, _, kind = LR.gene_classes(rng, s, 65)
    codes = np.zeros(m, dtype=np.int64)
    want, _, mu = LR.blind_dispersions(c, s)
    got, info = engine.nb_dispersions_blind(c, s, return_info=True)
    dead = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), dead)
    np.testing.assert_array_equal(dead, (c == 0).all(axis=0))
    live = ~dead
    cl, mul = c[:, live], mu[:, live]
    B = RR.bound(cl, mul, 1, want[live])
    at_got = RR.objective(cl, mul, codes, 1, got[live])
    short = RR.objective(cl, mul, codes, 1, want[live]) - at_got
    res = RR.resolved(c, mu, codes, 1, want)
    rel = np.abs(np.expm1(got[res] - want[res]))
    print("\nobjective shortfall / B: max %.3g; device objective off by at most %.3g B; resolved %d of %d genes, dispersion off by at most "
          "%.3g relative" % ((short / B).max(), (np.abs(info["objective"][live] - at_got) / B).max(), res.sum(), live.sum(),
                             rel.max(initial=0)))
    assert (short <= B).all() and (np.abs(info["objective"][live] - at_got) <= B).all()
    assert (rel <= 2e-4).all()
    np.testing.assert_allclose(info["base_mean"], (c / s[:, None]).mean(axis=0), rtol=m * 2.0 ** -52, atol=0)
    np.testing.assert_array_equal(engine.nb_dispersions_blind(c.astype(np.float32), s), got)
    with pytest.raises(ValueError, match="n_groups=1"):                 # the grouped call refuses one group, as before
        engine.nb_dispersions(c, codes.astype(np.int32), 1, s)


# ---- tl ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rld():
    counts, meta = _pseudobulk()
    return counts, meta, tl.rlog(counts)


def test_tl_rlog_is_the_host_tail_of_the_engine_calls():
    counts, meta, out = _rld()
    c = np.ascontiguousarray(counts.to_numpy(dtype=np.float64))
    sf = tl.deseq2_size_factors(counts).to_numpy()
    x = engine.nb_dispersions_blind(c, sf)
    mean = (c / sf[:, None]).mean(axis=0)
    fit = engine.nb_clip(engine.nb_trend(mean, engine.nb_clip(np.exp(x), 12))[0], 12)
    pv = engine.nb_rlog_prior_var(c, sf, mean, fit)
    values, info = engine.nb_rlog(c, sf, fit, pv, return_info=True)
    want = pd.DataFrame(values, index=counts.index, columns=counts.columns)
    pd.testing.assert_frame_equal(out, want, check_exact=True)
    assert out.attrs["prior_var"] == pv == LR.prior_var(c, sf, mean, fit) and 0.05 < pv < 5.0
    np.testing.assert_array_equal(out.attrs["dispFit"].to_numpy(), fit)
    np.testing.assert_array_equal(out.attrs["intercept"].to_numpy(), info["intercept"])
    np.testing.assert_array_equal(out.attrs["size_factors"].to_numpy(), sf)
    assert out.attrs["n_not_converged"] == 0
    # against the restatement from the same trend
    ref, _, left = LR.dense_rlog(c, sf, fit, pv)
    assert left.max() <= 1e-12 and np.abs(out.to_numpy() - ref).max() <= 1e-8
    # the reference's function: R's genes x samples frame
    rld = tl.compute_pseudobulk_PCA(counts, meta)
    assert list(rld.index) == list(counts.columns) and list(rld.columns) == list(counts.index)
    np.testing.assert_array_equal(rld.to_numpy(), out.to_numpy().T)
    given = tl.rlog(counts, size_factors=sf, prior_var=pv)
    pd.testing.assert_frame_equal(given, out, check_exact=True)


def test_pseudobulk_pca_is_sklearn_of_the_downloaded_matrix_and_separates_the_sub_groups():
    from sklearn.decomposition import PCA
    from sklearn.feature_selection import VarianceThreshold
    counts, meta, out = _rld()
    scores, ratio = tl.pseudobulk_pca(out)
    assert list(scores.columns) == ["PC1", "PC2"] and list(scores.index) == list(counts.index)
    model = PCA(n_components=2)
    want = model.fit_transform(VarianceThreshold(0.2).fit_transform(out.to_numpy()))
    np.testing.assert_allclose(scores.to_numpy(), want, rtol=0, atol=1e-9)
    np.testing.assert_allclose(ratio, model.explained_variance_ratio_, rtol=0, atol=1e-9)
    again, _ = tl.pseudobulk_pca(tl.compute_pseudobulk_PCA(counts, meta).T)
    pd.testing.assert_frame_equal(again, scores, check_exact=True)
    # the planted sub-groups: T1 and T3 lie further apart in the PC1 / PC2 plane than either is wide
    xy = scores.to_numpy()
    t1, t3 = xy[(meta["Predicted_Labels"] == "T1").to_numpy()], xy[(meta["Predicted_Labels"] == "T3").to_numpy()]
    gap = np.linalg.norm(t1.mean(axis=0) - t3.mean(axis=0))
    spread = max(np.linalg.norm(t - t.mean(axis=0), axis=1).max() for t in (t1, t3))
    print("\nT1 / T3 centres %.3g apart, largest distance from a group's own centre %.3g" % (gap, spread))
    assert gap > spread
    with pytest.raises(ValueError, match="n_components"):
        tl.pseudobulk_pca(out, variance_threshold=1e6)


def test_get_pseudobulk_DE_is_unchanged():
    """the frames of the pairwise runs carry the bits they had before rlog existed: recomputed pair by pair, with and without it"""
    counts, meta = _pseudobulk()
    before = tl.compute_pseudobulk_DE(counts, meta, group1="T1", group2="T3", cluster_col="Predicted_Labels")
    tl.rlog(counts)
    after = tl.compute_pseudobulk_DE(counts, meta, group1="T1", group2="T3", cluster_col="Predicted_Labels")
    pd.testing.assert_frame_equal(after, before, check_exact=True)
    rng = np.random.default_rng(8)
    rows, sample = [], []
    for name in counts.index:
        total = counts.loc[name].to_numpy().astype(np.int64)
        n = 3 + int(rng.integers(4))
        rows.append(rng.multinomial(total, np.full(n, 1.0 / n)).T)
        sample += [name] * n
    obs = pd.DataFrame({"cell_types": np.full(len(sample), "alpha", dtype=object), "sampleID": np.array(sample, dtype=object)})
    adata = _Adata(np.vstack(rows).astype(np.float32), obs, list(counts.columns))
    out = tl.get_pseudobulk_DE(adata, meta[["Predicted_Labels", "frac"]], "alpha")
    assert list(out) == ["T2vsT1", "T3vsT1", "T3vsT2"]
    pd.testing.assert_frame_equal(out["T3vsT1"], before, check_exact=True)
    cluster_counts, cluster_metadata = tl.pseudobulk_inputs(adata, meta[["Predicted_Labels", "frac"]], "alpha")
    rld = tl.compute_pseudobulk_PCA(cluster_counts, cluster_metadata)
    np.testing.assert_array_equal(rld.to_numpy(), _rld()[2].to_numpy().T)          # the route of the tutorial ends at the same matrix
