"""The negative-binomial GLM on the device (K22: engine.nb_dispersions, engine.nb_group_fits, tl.deseq2_dispersions,
tl.compute_pseudobulk_DE, tl.get_pseudobulk_DE) against the numpy / scipy restatement (tests/nb_glm_restatement.py, itself pinned
to scipy in test_nb_glm_args.py).

Shapes: m in {3 (2 + 1), 4, 12, 65, 130} samples in k in {2, 3, 5} unequal groups (one-sample groups among them, the codes
shuffled), G in {1, 63, 64, 65, 257} genes.  Gene classes, dealt round-robin: NB (the design's generator), Poisson, constant
rint(1e6 s_j) (ends next to minDisp; see test_nb_glm_args.py for why no class ends exactly on it), NB with alpha = 30 (runs into
maxDisp), means of 2e6 (the lgamma difference cancels), one group all zero, a single non-zero count, all zero.

Parity of nb_dispersions has two parts, because L is flat to rounding on some genes and two correct searches may then return
different x.  (1) For EVERY gene the restatement's objective at the device's x may fall short of its value at the restatement's x
by at most B = 64 * 2^-53 * (sum_j [|lgamma(c + r)| + |lgamma(r)| + |(c + r) log1p(a mu)| + |c log(a mu)|] + 4 m + k): 64 ulp (a
few per library function plus the summation) of the magnitudes actually added, plus one per term for where lgamma crosses zero.
(2) On the genes the restatement resolves (interior, L drops by more than 2 B at x -+ 1e-4) the dispersions agree to 2e-4
relative.  nb_group_fits is fed the restatement's dispersions, so errors do not compound: q and w to 1e-9 relative (1000 x the
1e-12 stop rule; the root is well conditioned), floors and flags exactly.  The tl frames must equal, bit for bit, the host tail
recomputed here from the engine calls' outputs."""
import functools
import itertools

import numpy as np
import pandas as pd
import pytest
from scipy import stats

import nb_glm_restatement as RR
from pilot_amd import engine, tl

pytestmark = pytest.mark.gpu

SHAPES = [(3, (2, 1), 1), (4, (2, 1, 1), 63), (12, (5, 4, 3), 257), (65, (30, 20, 10, 4, 1), 64), (130, (100, 30), 65)]
CLASSES = ["nb", "poisson", "constant", "alpha30", "huge", "zero group", "single", "all zero"]


def _counts(rng, s, codes, k, G):
    """G genes of the classes above, class j % 8 for gene j"""
    m = s.size
    base = np.exp(rng.uniform(np.log(2.0), np.log(3000.0), G))
    c = RR.nb_class(rng, s, codes, k, G)
    kind = np.arange(G) % len(CLASSES)
    mean = s[:, None] * base[None]
    for j in range(G):
        what = CLASSES[kind[j]]
        if what == "poisson":
            c[:, j] = rng.poisson(mean[:, j])
        elif what == "constant":
            c[:, j] = np.rint(1e6 * s)
        elif what == "alpha30":
            c[:, j] = RR.nb_counts(rng, mean[:, j], 30.0)
        elif what == "huge":
            c[:, j] = RR.nb_counts(rng, 2e6 * s, 0.01)
        elif what == "zero group":
            c[codes == j % k, j] = 0.0
        elif what == "single":
            c[:, j] = 0.0
            c[rng.integers(m), j] = 1.0 + rng.integers(40)
        elif what == "all zero":
            c[:, j] = 0.0
    return c, kind


@functools.lru_cache(maxsize=None)
def _case(m, sizes, G):
    rng = np.random.default_rng(1000 * m + G)
    k = len(sizes)
    s = RR.size_factors(rng, m)
    codes = rng.permutation(np.repeat(np.arange(k), sizes)).astype(np.int32)
    c, kind = _counts(rng, s, codes, k, G)
    x, L, mu = RR.dispersions(c, codes, k, s)
    base = (c / s[:, None]).mean(axis=0)
    with np.errstate(divide="ignore"):
        prior = np.where(np.isnan(x), np.nan, np.log(0.05 + 2.0 / base))
    xp, Lp, _ = RR.dispersions(c, codes, k, s, prior, 0.6)
    for a in (c, s, codes, x, L, mu, prior, xp, Lp):
        a.flags.writeable = False
    return dict(m=m, k=k, G=G, c=c, s=s, codes=codes, kind=kind, x=x, L=L, mu=mu, prior=prior, xp=xp, Lp=Lp)


def _ids(shape):
    return "m%d-k%d-G%d" % (shape[0], len(shape[1]), shape[2])


# ---- engine.nb_dispersions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prior", [False, True], ids=["gene-wise", "MAP"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_dispersions_against_the_restatement(shape, with_prior):
    C = _case(*shape)
    c, s, codes, k, mu = C["c"], C["s"], C["codes"], C["k"], C["mu"]
    prior, pv = (C["prior"], 0.6) if with_prior else (None, None)
    want = C["xp"] if with_prior else C["x"]
    got, info = engine.nb_dispersions(c, codes, k, s, log_prior_mean=prior, prior_var=pv, return_info=True)
    dead = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), dead)
    np.testing.assert_array_equal(np.isnan(info["objective"]), dead)
    np.testing.assert_array_equal(dead, (c == 0).all(axis=0))
    assert dead[C["kind"] == CLASSES.index("all zero")].all()
    live = ~dead
    if not live.any():
        return
    cl, mul = c[:, live], mu[:, live]
    pl = None if prior is None else prior[live]
    lo, hi = np.log(RR.MIN_DISP), np.log(RR.max_disp(C["m"]))
    assert (got[live] >= lo - 1e-14).all() and (got[live] <= hi + 1e-14).all()      # the grid's ends: the bounds up to an ulp
    # (1) the objective, every gene
    B = RR.bound(cl, mul, k, want[live])
    at_want = RR.objective(cl, mul, codes, k, want[live], pl, pv)
    at_got = RR.objective(cl, mul, codes, k, got[live], pl, pv)
    short = at_want - at_got
    print("\nobjective shortfall / B: max %.3g (gene class %s); device objective off by at most %.3g B"
          % ((short / B).max(), CLASSES[C["kind"][live][np.argmax(short / B)]], (np.abs(info["objective"][live] - at_got) / B).max()))
    assert (short <= B).all(), (short / B).max()
    assert (np.abs(info["objective"][live] - at_got) <= B).all()       # what the device reports is L at its x
    # (2) the dispersion, resolved genes
    res = RR.resolved(c, mu, codes, k, want, 1e-4, prior, pv)
    rel = np.abs(np.expm1(got[res] - want[res]))
    print("resolved %d of %d genes; dispersion off by at most %.3g relative" % (res.sum(), live.sum(), rel.max() if res.any() else 0.0))
    assert (rel <= 2e-4).all()
    # the normalised group means: one add per sample against numpy's pairwise sums
    np.testing.assert_allclose(info["fitted_mean"], RR.group_means(c, codes, k, s), rtol=C["m"] * 2.0 ** -52, atol=0)


def test_classes_behave_as_described():
    C = _case(*SHAPES[2])
    x, kind = C["x"], C["kind"]
    lo, hi = np.log(RR.MIN_DISP), np.log(RR.max_disp(C["m"]))
    res = RR.resolved(C["c"], C["mu"], C["codes"], C["k"], x)
    assert res[kind == 0].mean() >= 0.95                                # the NB class is held by rule 2
    assert (x[kind == CLASSES.index("constant")] - lo <= 1e-3).all()
    assert (x[kind == CLASSES.index("alpha30")] >= hi - 1.0).mean() >= 0.5


# ---- engine.nb_group_fits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_group_fits_against_the_restatement(shape):
    C = _case(*shape)
    c, s, codes, k = C["c"], C["s"], C["codes"], C["k"]
    alpha = np.clip(np.exp(C["x"]), RR.MIN_DISP, RR.max_disp(C["m"]))
    want_q, want_w, want_flags = RR.group_fits(c, codes, k, s, alpha)
    q, w, info = engine.nb_group_fits(c, codes, k, s, alpha, return_info=True)
    dead = np.isnan(alpha)
    assert np.isnan(q[dead]).all() and np.isnan(w[dead]).all() and not info["flags"][dead].any() and not info["steps"][dead].any()
    np.testing.assert_array_equal(info["flags"], want_flags)           # nothing unconverged; the floors where the restatement's are
    assert info["n_not_converged"] == 0 and info["steps"].max() <= 100
    live = ~dead
    print("\nq off by at most %.3g, w by %.3g relative; at most %d steps"
          % (np.abs(q[live] / want_q[live] - 1).max(initial=0), np.abs(w[live] / want_w[live] - 1).max(initial=0), info["steps"].max()))
    np.testing.assert_allclose(q[live], want_q[live], rtol=1e-9, atol=0)
    np.testing.assert_allclose(w[live], want_w[live], rtol=1e-9, atol=0)
    floored = (want_flags & RR.FLOORED) != 0
    np.testing.assert_array_equal(q[floored], want_q[floored])          # a floor is the same number
    if C["G"] >= 63:
        assert floored.any()
    plain = engine.nb_group_fits(c, codes, k, s, alpha)
    np.testing.assert_array_equal(plain[0], q)
    np.testing.assert_array_equal(plain[1], w)


# ---- same bits --------------------------------------------------------------------------------------------------------------------
def _both(Y, C, alpha):
    x, info = engine.nb_dispersions(Y, C["codes"], C["k"], C["s"], log_prior_mean=C["prior"], prior_var=0.6, return_info=True)
    q, w, fit = engine.nb_group_fits(Y, C["codes"], C["k"], C["s"], alpha, return_info=True)
    return [x, info["objective"], info["fitted_mean"], q, w, fit["steps"], fit["flags"]]


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=_ids)
def test_same_bits_by_every_route(shape):
    C = _case(*shape)
    c, G = C["c"], C["G"]
    assert c.max() < 2 ** 24                                           # float32 holds every count
    alpha = np.clip(np.exp(C["x"]), RR.MIN_DISP, RR.max_disp(C["m"]))
    first = _both(np.ascontiguousarray(c), C, alpha)
    wide = np.full((C["m"], G + 7), 3.0)
    wide[:, 3:3 + G] = c
    D = engine.DeviceMatrix.upload(wide)
    routes = {"again": np.ascontiguousarray(c), "float32": c.astype(np.float32), "device": engine.DeviceMatrix.upload(c),
              "device float32": engine.DeviceMatrix.upload(c.astype(np.float32)), "window": engine.device_columns(D, 3, 3 + G)}
    for name, Y in routes.items():
        for a, b in zip(first, _both(Y, C, alpha)):
            np.testing.assert_array_equal(a, b, err_msg=name)


# ---- limits and refusals ----------------------------------------------------------------------------------------------------------
def test_limits_and_bad_counts():
    limit = engine.nb_glm_limits()
    assert limit >= 4096
    m = limit + 1
    with pytest.raises(NotImplementedError):
        engine.nb_dispersions(np.ones((m, 2)), np.arange(m) % 2, 2, np.ones(m))
    C = _case(*SHAPES[1])
    for value, row, col in ((-1.0, 2, 5), (np.nan, 0, 62), (np.inf, 3, 0), (-0.6, 1, 1)):
        Y = np.array(C["c"])
        Y[row, col] = value
        with pytest.raises(ValueError, match=r"Y\[%d, %d\]" % (row, col)) as err:
            engine.nb_dispersions(Y, C["codes"], C["k"], C["s"])
        assert (err.value.row, err.value.col) == (row, col)
        with pytest.raises(ValueError, match=r"Y\[%d, %d\]" % (row, col)):
            engine.nb_group_fits(Y, C["codes"], C["k"], C["s"], np.full(C["G"], 0.1))
    Y = np.array(C["c"])
    Y[1, 1] = -0.4                                                      # rounds to a count of zero
    engine.nb_dispersions(Y, C["codes"], C["k"], C["s"])
    Y[3, 7] = Y[0, 9] = -5.0                                            # the first one: the lowest column, then the lowest row
    with pytest.raises(ValueError, match=r"Y\[3, 7\]"):
        engine.nb_dispersions(Y, C["codes"], C["k"], C["s"])


def test_the_largest_sample_count():
    """m = the limit, k = 3: the whole LDS layout of one gene (one class each of NB and all zero), against the restatement"""
    m = engine.nb_glm_limits()
    rng = np.random.default_rng(22)
    s = RR.size_factors(rng, m)
    codes = rng.permutation(np.repeat(np.arange(3), (m - 1001, 1000, 1))).astype(np.int32)
    c = np.zeros((m, 2))
    c[:, 0] = RR.nb_class(rng, s, codes, 3, 1)[:, 0]
    want, _, mu = RR.dispersions(c, codes, 3, s)
    got = engine.nb_dispersions(c, codes, 3, s)
    assert np.isnan(got[1]) and np.isnan(want[1])
    B = RR.bound(c[:, :1], mu[:, :1], 3, want[:1])
    short = RR.objective(c[:, :1], mu[:, :1], codes, 3, want[:1]) - RR.objective(c[:, :1], mu[:, :1], codes, 3, got[:1])
    print("\nshortfall %.3g B" % (short[0] / B[0]))
    assert short[0] <= B[0]
    if RR.resolved(c, mu, codes, 3, want)[0]:
        assert abs(np.expm1(got[0] - want[0])) <= 2e-4


# ---- tl ---------------------------------------------------------------------------------------------------------------------------
def _bh(p):
    order = np.argsort(p, kind="stable")
    scaled = p[order] * p.size / np.arange(1, p.size + 1)
    out = np.empty(p.size)
    out[order] = np.minimum(np.minimum.accumulate(scaled[::-1])[::-1], 1.0)
    return out


def _de_by_hand(counts, meta, group1, group2, cluster_col):
    """tl.compute_pseudobulk_DE from the engine calls and the host tail written out"""
    keep = ((meta[cluster_col] == group1) | (meta[cluster_col] == group2)).to_numpy()
    sub = counts.loc[meta.index[keep]]
    codes = (meta[cluster_col][keep] == group2).to_numpy().astype(np.int32)
    c = np.ascontiguousarray(sub.to_numpy(dtype=np.float64))
    sf = tl.deseq2_size_factors(sub).to_numpy()
    m = c.shape[0]
    x = engine.nb_dispersions(c, codes, 2, sf)
    q = np.rint(c) / sf[:, None]
    base = np.where(np.isnan(x), np.nan, q.mean(axis=0))
    clip = lambda d: np.clip(d, RR.MIN_DISP, RR.max_disp(m))
    fit, _ = engine.nb_trend(base, clip(np.exp(x)), "parametric")
    pv, vld = engine.nb_prior_var(x, np.log(fit), m, 2)
    x_map = engine.nb_dispersions(c, codes, 2, sf, log_prior_mean=np.log(fit), prior_var=pv)
    disp = np.where(RR.outliers(x, np.log(fit), vld), clip(np.exp(x)), clip(np.exp(x_map)))
    qh, w = engine.nb_group_fits(c, codes, 2, sf, disp)
    with np.errstate(divide="ignore", invalid="ignore"):
        lfc = np.log2(qh[:, 1]) - np.log2(qh[:, 0])
        se = np.log2(np.e) * np.sqrt(1.0 / w[:, 0] + 1.0 / w[:, 1])
        stat = lfc / se
    p = 2.0 * stats.norm.sf(np.abs(stat))
    padj = np.full(p.size, np.nan)
    padj[~np.isnan(p)] = _bh(p[~np.isnan(p)])
    frame = pd.DataFrame({"gene": np.asarray(sub.columns), "baseMean": base, "log2FoldChange": lfc, "lfcSE": se, "stat": stat, "pvalue": p,
                          "padj": padj, "dispersion": disp})
    return frame.iloc[np.argsort(padj, kind="stable")].reset_index(drop=True)


@functools.lru_cache(maxsize=None)
def _pseudobulk():
    """12 samples in three sub-groups (5, 4, 3), 120 NB genes; gene 5 is zero in T1 and T2, genes 9 and 10 are copies (tied padj)"""
    rng = np.random.default_rng(7)
    s = RR.size_factors(rng, 12)
    codes = rng.permutation(np.repeat(np.arange(3), (5, 4, 3)))
    c = RR.nb_class(rng, s, codes, 3, 120)
    c[codes < 2, 5] = 0.0
    c[:, 10] = c[:, 9]
    samples = ["s%02d" % i for i in range(12)]
    counts = pd.DataFrame(c, index=samples, columns=["g%03d" % j for j in range(120)])
    labels = np.array(["T1", "T2", "T3"])[codes]
    meta = pd.DataFrame({"Predicted_Labels": labels, "stage": labels, "frac": rng.random(12)}, index=samples)
    return counts, meta


@pytest.mark.parametrize("group1,group2", [("T1", "T2"), ("T1", "T3"), ("T2", "T3")])
def test_compute_pseudobulk_DE_is_the_host_tail_of_the_engine_calls(group1, group2):
    counts, meta = _pseudobulk()
    out = tl.compute_pseudobulk_DE(counts, meta, group1=group1, group2=group2, cluster_col="Predicted_Labels")
    assert list(out.columns) == ["gene", "baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "padj", "dispersion"]
    pd.testing.assert_frame_equal(out, _de_by_hand(counts, meta, group1, group2, "Predicted_Labels"), check_exact=True)
    padj = out["padj"].to_numpy()
    n_nan = int(np.isnan(padj).sum())
    assert (np.diff(padj[:len(padj) - n_nan]) >= 0).all() and np.isnan(padj[len(padj) - n_nan:]).all()      # arrange(padj): NaN last
    pos = {g: i for i, g in enumerate(out["gene"])}
    assert pos["g009"] + 1 == pos["g010"]                               # ties keep the gene order
    if "T3" not in (group1, group2):
        assert n_nan == 1 and out["gene"].iloc[-1] == "g005" and out.iloc[-1, 1:].isna().all()
    else:
        assert n_nan == 0
    disp = out.attrs["dispersions"]
    assert disp.index.tolist() == counts.columns.tolist() and disp["dispersion"].between(1e-8, 10.0).sum() == 120 - n_nan
    assert out.attrs["n_not_converged"] == 0
    # the other way round: the fold change and the statistic change sign, nothing else changes
    back = tl.compute_pseudobulk_DE(counts, meta, group1=group2, group2=group1, cluster_col="Predicted_Labels")
    pd.testing.assert_frame_equal(back.drop(columns=["log2FoldChange", "stat"]), out.drop(columns=["log2FoldChange", "stat"]),
                                  check_exact=True)
    live = ~np.isnan(padj)
    np.testing.assert_array_equal(back["log2FoldChange"].to_numpy()[live], -out["log2FoldChange"].to_numpy()[live])
    np.testing.assert_array_equal(back["stat"].to_numpy()[live], -out["stat"].to_numpy()[live])
    # a true fold change is found: the genes the generator moved most between the two groups lead the table
    assert (out["padj"] < 0.05).sum() >= 3


def test_deseq2_dispersions_frame():
    counts, meta = _pseudobulk()
    out = tl.deseq2_dispersions(counts, meta["stage"].to_numpy())
    assert list(out.columns) == ["baseMean", "baseVar", "dispGeneEst", "dispFit", "dispMAP", "dispersion", "dispOutlier"]
    c, sf = counts.to_numpy(), tl.deseq2_size_factors(counts).to_numpy()
    codes = np.unique(meta["stage"].to_numpy(), return_inverse=True)[1].astype(np.int32)
    x = engine.nb_dispersions(c, codes, 3, sf)
    clip = lambda d: np.clip(d, RR.MIN_DISP, RR.max_disp(12))
    np.testing.assert_array_equal(out["dispGeneEst"].to_numpy(), clip(np.exp(x)))
    q = c / sf[:, None]
    np.testing.assert_array_equal(out["baseMean"].to_numpy(), q.mean(axis=0))
    np.testing.assert_array_equal(out["baseVar"].to_numpy(), q.var(axis=0, ddof=1))
    fit, trend = engine.nb_trend(q.mean(axis=0), clip(np.exp(x)), "parametric")
    np.testing.assert_array_equal(out["dispFit"].to_numpy(), fit)
    assert out.attrs["trend"]["coefficients"] == trend["coefficients"]
    pv, vld = RR.prior_var(x, np.log(fit), 12, 3)
    assert (out.attrs["prior_var"], out.attrs["var_log_disp"]) == (pv, vld)
    flags = RR.outliers(x, np.log(fit), vld)
    np.testing.assert_array_equal(out["dispOutlier"].to_numpy(), flags)
    x_map = engine.nb_dispersions(c, codes, 3, sf, log_prior_mean=np.log(fit), prior_var=pv)
    np.testing.assert_array_equal(out["dispersion"].to_numpy(), np.where(flags, clip(np.exp(x)), clip(np.exp(x_map))))
    shrunk = np.abs(np.log(out["dispMAP"]) - np.log(out["dispFit"])) <= np.abs(np.log(out["dispGeneEst"]) - np.log(out["dispFit"])) + 1e-6
    assert shrunk.all()                                                 # the prior pulls every estimate towards the trend


class _Adata:
    def __init__(self, X, obs, var_names):
        self.X, self.obs, self.var_names, self.uns = X, obs, var_names, {}


def test_get_pseudobulk_DE_returns_the_keyed_frames():
    """a synthetic AnnData whose per-sample sums of the cell type 'alpha' are the table above: every sample's counts are dealt over
    its cells, and cells of a second type ride along"""
    counts, meta = _pseudobulk()
    rng = np.random.default_rng(8)
    rows, sample, cell = [], [], []
    for name in counts.index:
        total = counts.loc[name].to_numpy().astype(np.int64)
        n = 3 + int(rng.integers(4))
        share = rng.multinomial(total, np.full(n, 1.0 / n)).T              # n cells x genes, summing to the sample's counts
        rows.append(share)
        sample += [name] * (n + 2)
        cell += ["alpha"] * n + ["beta"] * 2
        rows.append(rng.poisson(3.0, (2, total.size)))
    X = np.vstack(rows).astype(np.float32)
    shuffle = rng.permutation(X.shape[0])
    obs = pd.DataFrame({"cell_types": np.array(cell, dtype=object)[shuffle], "sampleID": np.array(sample, dtype=object)[shuffle]})
    adata = _Adata(X[shuffle], obs, list(counts.columns))
    props = meta[["Predicted_Labels", "frac"]]
    out = tl.get_pseudobulk_DE(adata, props, "alpha", celltype_col="cell_types", sample_col="sampleID", cluster_col="Predicted_Labels")
    assert list(out) == ["T2vsT1", "T3vsT1", "T3vsT2"]
    for (g1, g2), frame in zip(itertools.combinations(["T1", "T2", "T3"], 2), out.values()):
        pd.testing.assert_frame_equal(frame, tl.compute_pseudobulk_DE(counts, meta, group1=g1, group2=g2, cluster_col="Predicted_Labels"),
                                      check_exact=True)
    dropped = tl.get_pseudobulk_DE(adata, props, "alpha", remove_samples=["s00"])
    assert list(dropped) == ["T2vsT1", "T3vsT1", "T3vsT2"] and len(dropped["T2vsT1"]) == 120
    for key in dropped:                                                 # only the pairs that held the sample change
        held = meta.loc["s00", "Predicted_Labels"] in key
        assert dropped[key]["baseMean"].equals(out[key]["baseMean"]) == (not held)
