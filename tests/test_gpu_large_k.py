"""Large-K parity: the fallback solvers up to their stated limit K = 2048 and the pre-pass / cost matrix up to 4096, each held to
an fp64 reference that does not share its code -- the C oracle (POT's loop, the network simplex), scipy's pdist, numpy's
median, a closed-form W1 on the line and the numpy restatement of POT's sinkhorn_stabilized.  The K values sit on both sides
of every point where a kernel's launch geometry changes shape:

* sinkhorn_generic_kernel (generic_kernels.hpp): the number of waves that share one output block (nsplit) halves as K grows;
* emd_generic_kernel (emd_generic_kernel.hpp): its LDS passes the 64 KiB that a launch gets without hipFuncSetAttribute;
* cost_matrix_kernel: its LDS (2 K + D doubles) passes 64 KiB at K = 4096;
* the resident workgroups of both fallback solvers are reused for a second pair once the pairs outnumber them."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import scipy.spatial.distance as ssd

from oracle import oracle as O
from pilot_amd import _lib, engine, multi, tl
from pilot_amd.synthetic import make_cells, make_problem
from test_gpu_transport_plans import _cost, _histograms, pot_sinkhorn_stabilized

pytestmark = pytest.mark.gpu

ORACLE_THREADS = 16


def _by_row(fn, P, M, *args, **kw):
    """An oracle grid with its rows run side by side: the oracle deals pairs to its threads 16 at a time, so a grid of 16 or
    fewer pairs would otherwise run on one thread.  Each row is the oracle's own call (row_begin = i, one thread)."""
    N = P.shape[0]
    with ThreadPoolExecutor(min(N, ORACLE_THREADS)) as ex:
        rows = list(ex.map(lambda i: fn(P, M, *args, row_begin=i, row_end=i + 1, n_threads=1, **kw), range(N)))
    if isinstance(rows[0], tuple):
        E = np.concatenate([r[0] for r in rows])
        return E, {k: np.concatenate([r[1][k] for r in rows]) for k in rows[0][1]}
    return np.concatenate(rows)


def _ns_grid(P, M):
    return _by_row(O.emd_grid, P, M, fast="ns")


def _sinkhorn_oracle(P, M, reg):
    return _by_row(O.sinkhorn_grid, P, M, reg, return_info=True)


def _nonsym_cost(K, seed):
    M = np.random.default_rng(seed).random((K, K))
    return M / M.max()


# ================================================================================================ A. Sinkhorn, K2g regimes
GENERIC_WAVES, LDS_BYTES = 16, 160 * 1024


def _nsplit(K):
    """run_generic (pilot_ot_sinkhorn.hip): 8 vectors of K doubles, nsplit rows of K partial sums, GENERIC_WAVES reduction doubles and a
    16-byte queue slot must fit 160 KiB of LDS -- lds(ns) = 8 ((8 + ns) K + 16) + 16 -- with nsplit the largest power of two
    <= 16 that fits.  16 -> 8 after K = 852, 8 -> 4 after 1278, 4 -> 2 after 1705, 2 -> 1 after 2046."""
    ns = GENERIC_WAVES
    while ns > 1 and 8 * ((8 + ns) * K + GENERIC_WAVES) + 16 > LDS_BYTES:
        ns //= 2
    return ns


K2G = [257, 852, 853, 1278, 1279, 1705, 1706, 2046, 2047, 2048]
K2G_NONSYM = (853, 1706, 2047)
K2G_SMALL_REG = (852, 1278, 1279, 2046, 2047)          # one K in each nsplit regime


def test_the_k_values_straddle_every_nsplit_boundary():
    last = [K for K in range(257, 2048) if _nsplit(K) != _nsplit(K + 1)]
    assert last == [852, 1278, 1705, 2046]
    for K in last:
        assert K in K2G and K + 1 in K2G
    assert sorted({_nsplit(K) for K in K2G}) == [1, 2, 4, 8, 16]
    assert sorted({_nsplit(K) for K in K2G_SMALL_REG}) == [1, 2, 4, 8, 16]


def _assert_pot_literal(Eg, ig, Eo, io, tol):
    assert np.isfinite(Eg).all()
    np.testing.assert_array_equal(ig["iters"], io["iters"])
    for bit in (1, 2, 4, 8):
        np.testing.assert_array_equal(ig["flags"] & bit, io["flags"] & bit)
    assert np.all((ig["flags"] & _lib.FLAG_F64) > 0)
    assert np.abs(Eg - Eo).max() <= tol, np.abs(Eg - Eo).max()


@pytest.mark.parametrize("K", K2G)
def test_sinkhorn_generic_regimes_reg_01(K, switches):
    """reg 0.1 on make_problem costs (and a random non-symmetric cost at three K): every update count, flag and error of the
    oracle, values to 1e-12.  At K = 1279 and 2048 one and three resident workgroups (each running several pairs in turn), row
    shards and (1279) a two-shard run must give the default launch's bits: a pair's arithmetic does not depend on where it runs."""
    N = 5 if K <= 1279 else 4
    P, M = make_problem(N, K, 6, seed=K, cells_per_patient=3000)
    costs = [M] + ([_nonsym_cost(K, K)] if K in K2G_NONSYM else [])
    for Mc in costs:
        Eo, io = _sinkhorn_oracle(P, Mc, 0.1)
        Eg, ig = engine.sinkhorn_grid(P, Mc, 0.1, return_info=True)
        _assert_pot_literal(Eg, ig, Eo, io, 1e-12)
        np.testing.assert_allclose(ig["err"], io["err"], rtol=1e-6, atol=1e-13)
    if K not in (1279, 2048):
        return
    Eg, ig = engine.sinkhorn_grid(P, M, 0.1, return_info=True)
    for wgs in ("1", "3"):
        switches.setenv("PILOT_OT_GENERIC_WGS", wgs)
        try:
            Ew, iw = engine.sinkhorn_grid(P, M, 0.1, return_info=True)
        finally:
            switches.delenv("PILOT_OT_GENERIC_WGS")
        np.testing.assert_array_equal(Ew, Eg)
        for k in ("iters", "err", "flags"):
            np.testing.assert_array_equal(iw[k], ig[k])
    for rb, re_, rs in ((0, N, 2), (1, N, 3), (N - 1, N, 1)):
        np.testing.assert_array_equal(engine.sinkhorn_grid(P, M, 0.1, row_begin=rb, row_end=re_, row_step=rs), Eg[rb:re_:rs])
    if K == 1279:
        Em, im = multi.sinkhorn_grid_multi(P, M, 0.1, devices=[0, 0], return_info=True)
        np.testing.assert_array_equal(Em, Eg)
        np.testing.assert_array_equal(im["iters"], ig["iters"])
        np.testing.assert_array_equal(im["flags"], ig["flags"])


@pytest.mark.parametrize("K", K2G_SMALL_REG)
def test_sinkhorn_generic_regimes_reg_001(K):
    """reg 0.01: the diagonal pairs run the full 1000 updates, the others absorb and leave by POT's NaN revert (flags 2 | 8) --
    the bounds of test_generic_kernel_is_pot_literal_including_absorption_and_tiny_reg, in every nsplit regime."""
    P, M = make_problem(3, K, 6, seed=K, cells_per_patient=3000)
    Eo, io = _sinkhorn_oracle(P, M, 0.01)
    Eg, ig = engine.sinkhorn_grid(P, M, 0.01, return_info=True)
    _assert_pot_literal(Eg, ig, Eo, io, 1e-10)
    assert ((io["flags"] & O.FLAG_ABSORBED) > 0).any()


# ================================================================================================ B. exact OT, K3g
def _assert_exact(P, M, tol=1e-12, **kw):
    Eg = engine.emd_grid(P, M, **kw)
    Eo = _ns_grid(P, M)
    assert np.abs(Eg - Eo).max() <= tol, np.abs(Eg - Eo).max()
    return Eg


@pytest.mark.parametrize("K", [933, 934, 1500, 2048])
def test_exact_generic_on_both_sides_of_64_kib(K):
    """emd_grid_kernel's fallback at K > 256, against the network simplex: its LDS (70 K + 192 bytes) passes 64 KiB at K = 934.
    A symmetric cost with equal masses (auto: upper triangle + mirror; all), then a non-symmetric cost with sparse histograms
    of unequal mass (empty bins on both sides)."""
    N = 4 if K < 2048 else 3
    P, M = make_problem(N, K, 6, seed=K, cells_per_patient=3000)
    assert engine.equal_masses(P)
    Ea = _assert_exact(P, M, mode="auto")
    Eall = _assert_exact(P, M, mode="all")
    np.testing.assert_array_equal(np.triu(Ea), np.triu(Eall))
    rng = np.random.default_rng(K + 1)
    Ps = rng.random((N, K))
    Ps[rng.random((N, K)) < 0.5] = 0.0
    Ps[:, 0] = 0.5
    Ps *= rng.uniform(0.5, 2.0, size=(N, 1)) / Ps.sum(1, keepdims=True)
    _assert_exact(Ps, _nonsym_cost(K, K + 2))


def _w1_on_the_line(a, b, x):
    """W1 between a and b * sum(a) / sum(b) on points x (cost |x_i - x_j|): the sum over the sorted distinct points of
    |A - B| times the gap to the next point, A and B the cumulative masses."""
    b = b * (a.sum() / b.sum())
    pts = np.unique(x)
    ma = np.array([math.fsum(a[x == p]) for p in pts])
    mb = np.array([math.fsum(b[x == p]) for p in pts])
    terms, A, B = [], 0.0, 0.0
    for k in range(len(pts) - 1):
        A = math.fsum([A, ma[k]])
        B = math.fsum([B, mb[k]])
        terms.append(abs(A - B) * float(pts[k + 1] - pts[k]))
    return math.fsum(terms)


@pytest.mark.parametrize("K", [934])
def test_exact_generic_against_closed_form_w1_on_a_line(K):
    """Centroids on a line at a dozen integer points: most off-diagonal costs are zero and the searches meet ties everywhere.
    W1 has a closed form there, independent of any solver.  (K = 2048 is left out: with ties this heavy a 3 x 3 grid there
    took about five minutes on the MI355X, against 17 s at K = 934.)"""
    rng = np.random.default_rng(K)
    x = rng.integers(0, 12, size=K).astype(np.float64)
    M = np.abs(x[:, None] - x[None, :])
    N = 3
    P = rng.random((N, K))
    P[rng.random((N, K)) < 0.3] = 0.0
    P *= rng.uniform(0.5, 2.0, size=(N, 1)) / P.sum(1, keepdims=True)
    Eg = engine.emd_grid(P, M)
    for i in range(N):
        for j in range(N):
            W = _w1_on_the_line(P[i], P[j], x)
            assert abs(Eg[i, j] - W) <= 1e-12 * max(1.0, W), (i, j, Eg[i, j], W)


def test_exact_generic_reuses_its_flow_slabs():
    """K = 300, N = 40: 820 upper-triangle pairs (1600 in mode 'all') for at most 512 resident workgroups, so workgroups solve a
    second pair in the flow slab of their first.  Every pair against the network simplex; row shards give the same bits."""
    N, K = 40, 300
    P, M = make_problem(N, K, 6, seed=300, cells_per_patient=3000)
    Eo = O.emd_grid(P, M, fast="ns", n_threads=ORACLE_THREADS)
    Ea = engine.emd_grid(P, M)
    assert np.abs(Ea - Eo).max() <= 1e-12
    Eall = engine.emd_grid(P, M, mode="all")
    assert np.abs(Eall - Eo).max() <= 1e-12
    for rb, re_, rs in ((0, N, 3), (1, N, 7), (N - 1, N, 1)):
        np.testing.assert_array_equal(engine.emd_grid(P, M, mode="all", row_begin=rb, row_end=re_, row_step=rs), Eall[rb:re_:rs])


def test_exact_refuses_k_2049():
    P, M = make_problem(2, 2049, 4, seed=1, cells_per_patient=500)
    with pytest.raises(NotImplementedError, match="2049"):
        engine.emd_grid(P, M)


# ================================================================================================ C. transport plans
@pytest.mark.parametrize("K", [934, 1500, 2048])
def test_exact_plans_at_large_k(K):
    """A feasible plan whose value is the LP optimum is an optimal plan: Gamma >= 0, its margins are a and the rescaled b, its
    <M, Gamma> is the reported value, the grid's value bit for bit, and the network simplex's to 1e-12."""
    N = 3
    P = _histograms(N, K, K)
    M = _cost(K, K)
    pr = np.array([[0, 1], [1, 2], [2, 0], [1, 1]])
    G, info = engine.transport_plans(P, M, pr, return_info=True)
    vals = info["values"]
    E = engine.emd_grid(P, M, mode="all")
    Eo = _ns_grid(P, M)
    for t, (i, j) in enumerate(pr):
        a, b = P[i], P[j] * (P[i].sum() / P[j].sum())
        g = G[t]
        assert (g >= 0).all()
        np.testing.assert_allclose(g.sum(1), a, rtol=1e-12, atol=1e-12 * a.max())
        np.testing.assert_allclose(g.sum(0), b, rtol=1e-12, atol=1e-12 * b.max())
        assert abs((M * g).sum() - vals[t]) <= 1e-12 * max(1.0, abs(vals[t]))
        assert vals[t] == E[i, j], "pair %d (%d, %d): plan value %r, grid %r" % (t, i, j, vals[t], E[i, j])
        assert abs(vals[t] - Eo[i, j]) <= 1e-12
    assert (info["flags"] == 0).all() and (info["iters"] >= 0).all()


@pytest.mark.parametrize("K", [853, 1279, 2047])
def test_entropic_plans_at_large_k(K):
    N = 3
    P = _histograms(N, K, 3 * K, zeros=False, unequal=False)
    M = _cost(K, K)
    pr = np.array([[i, j] for i in range(N) for j in range(N)])
    G, info = engine.transport_plans(P, M, pr, regularized="reg", reg=0.1, return_info=True)
    E, ginfo = engine.sinkhorn_grid(P, M, 0.1, precision="generic", return_info=True)
    for t, (i, j) in enumerate(pr):
        assert info["values"][t] == E[i, j] and info["iters"][t] == ginfo["iters"][i, j] and info["flags"][t] == ginfo["flags"][i, j]
    t = 1
    i, j = pr[t]
    ref, _ = pot_sinkhorn_stabilized(P[i], P[j], M, 0.1)
    assert np.abs(G[t] - ref).max() <= 1e-10 * ref.max()
    assert abs(info["values"][t] - (M * G[t]).sum()) <= 1e-12 * max(1.0, abs(info["values"][t]))


def test_group_sums_at_k_1279_are_the_host_loop_bit_for_bit(switches):
    N, K, n = 4, 1279, 8
    P = _histograms(N, K, 11 * K, zeros=False, unequal=False)
    M = _cost(K, K)
    pr = np.array([[i, j] for i in range(N) for j in range(N)])[:n]
    groups = np.array([0, 1, 0, 2, 2, 0, 1, 0])
    per = engine.transport_plans(P, M, pr, regularized="reg")
    want = np.zeros((3, K, K))
    for t in range(n):
        want[groups[t]] += per[t]
    np.testing.assert_array_equal(engine.transport_plans(P, M, pr, regularized="reg", groups=groups), want)
    switches.setenv("PILOT_OT_PLAN_CHUNK_PAIRS", "3")    # partial sums carried across chunks
    try:
        np.testing.assert_array_equal(engine.transport_plans(P, M, pr, regularized="reg", groups=groups), want)
    finally:
        switches.delenv("PILOT_OT_PLAN_CHUNK_PAIRS")


# ================================================================================================ D. cost matrix
COST_SHAPES = [(4096, 1), (4096, 2), (4093, 7), (4000, 200), (2, 4096), (300, 4096)]


@pytest.mark.parametrize("metric", ["cosine", "euclidean", "sqeuclidean", "cityblock", "chebyshev", "correlation", "seuclidean"])
@pytest.mark.parametrize("K,D", COST_SHAPES)
def test_cost_matrix_up_to_4096(metric, K, D):
    """cost_matrix_kernel holds 2 K + D doubles of row statistics and variances in LDS: beyond 64 KiB whenever 2 K + D > 8192."""
    X = np.random.default_rng(K + D).standard_normal((K, D))
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = ssd.squareform(ssd.pdist(X, metric=metric))
    got = engine.pdist_square(X, metric=metric)
    np.testing.assert_allclose(got, ref, rtol=1e-13, atol=1e-14)
    assert np.array_equal(got, got.T, equal_nan=True) and np.all(np.diag(got) == 0)


def test_cost_matrix_mahalanobis_at_4096():
    X = np.random.default_rng(7).standard_normal((4096, 3))
    ref = ssd.squareform(ssd.pdist(X, metric="mahalanobis"))
    got = engine.pdist_square(X, metric="mahalanobis")
    np.testing.assert_allclose(got, ref, rtol=1e-13, atol=1e-14)
    assert np.array_equal(got, got.T) and np.all(np.diag(got) == 0)


# ================================================================================================ E. pre-pass
def _cohort(C, D, K, dtype, seed):
    """Cells with ties and signed zeros; type 0 has one cell, type 1 two, type K - 1 none."""
    rng = np.random.default_rng(seed)
    X = np.round(rng.standard_normal((C, D)) * 4) / 4
    X[rng.random((C, D)) < 0.05] = 0.0
    X[rng.random((C, D)) < 0.05] *= -0.0
    X = X.astype(dtype)
    cc = rng.integers(2, K - 1, size=C).astype(np.int32)
    cc[:3] = [0, 1, 1]
    return X, cc


def _assert_medians(got, X, cc, K):
    order = np.argsort(cc, kind="stable")
    bounds = np.searchsorted(cc[order], np.arange(K + 1))
    for k in range(K):
        rows = X[order[bounds[k]:bounds[k + 1]]]
        if len(rows) == 0:
            assert np.isnan(got[k]).all()
        else:
            np.testing.assert_array_equal(got[k], np.median(rows, axis=0).astype(np.float64))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("K", [1000, 4096])
def test_centroid_medians_small_and_general_path(K, dtype, switches):
    """A cohort small enough for the one-launch selection (C x K x D <= 3.2e7) and the sixteen-launch radix select on it."""
    D = 3 if K == 1000 else 1
    C = int(3.2e7 // (K * D))
    X, cc = _cohort(C, D, K, dtype, K + D)
    fast = engine.centroid_medians(X, cc, K)
    _assert_medians(fast, X, cc, K)
    switches.setenv("PILOT_OT_NO_SMALL_MEDIANS", "1")
    try:
        slow = engine.centroid_medians(X, cc, K)
    finally:
        switches.delenv("PILOT_OT_NO_SMALL_MEDIANS")
    np.testing.assert_array_equal(slow, fast)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("K", [1000, 4096])
def test_prepass_at_large_k(K, dtype, switches):
    """EmbeddingUpload.prepass (the device-resident embedding: above its 4 MB threshold): medians bit-equal to np.median per
    type, proportions bit-equal to the bincount restatement of test_proportions_kernel_large_and_ragged."""
    C, D, N = 200_000, 6, 37
    X, cc = _cohort(C, D, K, dtype, 3 * K)
    sc = np.random.default_rng(K).integers(0, N, size=C).astype(np.int32)
    counts = np.bincount(sc.astype(np.int64) * K + cc, minlength=N * K).reshape(N, K).astype(np.float64)
    prior = counts.sum(0) / (C - 1) * 0.2
    want = np.stack([(counts[n] + prior) / (sum(counts[n]) + sum(prior)) for n in range(N)])
    for general in (False, True):
        if general:
            switches.setenv("PILOT_OT_NO_SMALL_MEDIANS", "1")
        up = engine.EmbeddingUpload(X)
        try:
            assert up.thread is not None
            P, first, cen = up.prepass(cc, sc, N, K, n_total=C)
        finally:
            up.close()
            switches.delenv("PILOT_OT_NO_SMALL_MEDIANS")
        np.testing.assert_array_equal(P, want)
        np.testing.assert_array_equal(first, [int(np.argmax(sc == n)) for n in range(N)])
        _assert_medians(cen, X, cc, K)


# ================================================================================================ F. end to end
@pytest.mark.parametrize("mode", ["unreg", "reg"])
def test_wasserstein_distance_with_a_thousand_cell_types(mode, tmp_path, monkeypatch):
    """tl.wasserstein_distance with ~1000 cell types against the oracle chain cluster_representations -> cost_matrix -> exact
    grid (network simplex) or Sinkhorn grid.  At K > 256 precision 'auto' runs the POT-literal f64 kernel (FLAG_F64 on every
    pair): 1e-12 in both modes."""
    monkeypatch.chdir(tmp_path)
    ad = make_cells(6, 1000, 10, seed=4, cells_per_patient=4000)
    kw = dict(regularized=mode, reg=0.1)
    tl.wasserstein_distance(ad, emb_matrix="X_pca", **kw)
    obs = ad.obs
    clu, cells = O.cluster_representations(obs["cell_types"], obs["sampleID"])
    cost, _, _ = O.cost_matrix(ad.obsm["X_pca"], obs["cell_types"])
    K = len(cells)
    assert K >= 950
    P = np.stack(list(clu.values()))
    M = cost / cost.max()
    np.testing.assert_array_equal(np.stack(list(ad.uns["proportions"].values())), P)
    np.testing.assert_allclose(ad.uns["cost"].to_numpy(), cost, rtol=0, atol=1e-13 * cost.max())
    if mode == "unreg":
        Eo = _ns_grid(P, M)
    else:
        Eo, io = _sinkhorn_oracle(P, M, 0.1)
        Eg, ig = engine.sinkhorn_grid(P, ad.uns["cost"].to_numpy() / ad.uns["cost"].to_numpy().max(), 0.1, return_info=True)
        assert np.all((ig["flags"] & _lib.FLAG_F64) > 0)
        np.testing.assert_array_equal(ad.uns["EMD"], Eg)
        np.testing.assert_array_equal(ig["iters"], io["iters"])
    assert np.abs(ad.uns["EMD"] - Eo).max() <= 1e-12
