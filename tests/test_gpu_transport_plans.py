"""Transport plans on the device (engine.transport_plans, tl.transport_plans, tl.group_transport), held to the oracle,
scipy's LP solver, a numpy restatement of POT's sinkhorn_stabilized, and the pair grid's own values."""
import numpy as np
import pytest

from conftest import GOLDEN_REAL, golden_adata, load_golden
from oracle import oracle as O
from pilot_amd import _lib, engine, tl

pytestmark = pytest.mark.gpu


def _histograms(N, K, seed, zeros=True, unequal=True):
    rng = np.random.default_rng(seed)
    P = rng.random((N, K)) + 0.05
    if zeros:
        P[rng.random((N, K)) < 0.15] = 0.0           # empty bins in some histograms
        P[:, 0] = np.maximum(P[:, 0], 0.05)
    P /= P.sum(1, keepdims=True)
    if unequal:
        P *= rng.uniform(0.5, 2.0, size=(N, 1))       # unequal masses: POT's pre-step b *= sum(a) / sum(b)
    return P


def _cost(K, seed):
    rng = np.random.default_rng(seed + 1000)
    X = rng.standard_normal((K, 6))
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    return D / D.max()


def _pairs(N, n, seed):
    rng = np.random.default_rng(seed + 7)
    pr = rng.integers(0, N, size=(n, 2))
    pr[: min(3, n), 1] = pr[: min(3, n), 0]          # diagonal pairs
    return pr


# ------------------------------------------------------------------------------------------------ exact
def _linprog_value(a, b, M):
    from scipy.optimize import linprog
    K = len(a)
    A = np.zeros((2 * K, K * K))
    for i in range(K):
        A[i, i * K:(i + 1) * K] = 1.0
        A[K + i, i::K] = 1.0
    r = linprog(M.ravel(), A_eq=A, b_eq=np.concatenate([a, b]), bounds=(0, None), method="highs",
                options=dict(primal_feasibility_tolerance=1e-10, dual_feasibility_tolerance=1e-10))
    assert r.status == 0
    return r.fun


@pytest.mark.parametrize("K", [3, 14, 30, 50, 100, 256, 300, 600])
def test_exact_plans(K, switches):
    N = 10 if K <= 256 else 6
    P = _histograms(N, K, K)
    M = _cost(K, K)
    pr = _pairs(N, 24 if K <= 256 else 8, K)
    G, info = engine.transport_plans(P, M, pr, return_info=True)
    assert G.shape == (len(pr), K, K)
    vals = info["values"]
    if K <= 16:
        switches.setenv("PILOT_OT_EMD_MULTI", "0")         # the one-pair-per-wave kernel, the one plan mode runs
    try:
        E = engine.emd_grid(P, M, mode="all")
    finally:
        switches.delenv("PILOT_OT_EMD_MULTI")
    n_ref = 0
    for t, (i, j) in enumerate(pr):
        a, b = P[i], P[j] * (P[i].sum() / P[j].sum())
        g = G[t]
        assert (g >= 0).all()
        np.testing.assert_allclose(g.sum(1), a, rtol=1e-12, atol=1e-12 * a.max())
        np.testing.assert_allclose(g.sum(0), b, rtol=1e-12, atol=1e-12 * b.max())
        assert abs((M * g).sum() - vals[t]) <= 1e-12 * max(1.0, abs(vals[t]))
        assert vals[t] == E[i, j], "pair %d (%d, %d): plan value %r, grid %r" % (t, i, j, vals[t], E[i, j])
        if K <= 256 or t < 3:                             # (the CPU references are slow at K = 300, 600)
            assert abs(vals[t] - O.emd2(P[i], P[j], M)) <= 1e-12
            n_ref += 1
        if K <= 100 and t < 6:
            assert abs(vals[t] - _linprog_value(a, b, M)) <= 1e-12
    assert n_ref >= 3
    assert (info["flags"] == 0).all() and (info["iters"] >= 0).all()


# ------------------------------------------------------------------------------------------------ entropic
def pot_sinkhorn_stabilized(a, b, M, reg, numItermax=1000, tau=1e3, stopThr=1e-9, print_period=20):
    """POT 0.9 ot.bregman.sinkhorn_stabilized (warmstart None, log False), restated in numpy: (Gamma, iterations)."""
    dim_a, dim_b = len(a), len(b)
    alpha, beta = np.zeros(dim_a), np.zeros(dim_b)
    u, v = np.full(dim_a, 1.0 / dim_a), np.full(dim_b, 1.0 / dim_b)

    def get_K(alpha, beta):
        return np.exp(-(M - alpha.reshape((dim_a, 1)) - beta.reshape((1, dim_b))) / reg)

    def get_Gamma(alpha, beta, u, v):
        return np.exp(-(M - alpha.reshape((dim_a, 1)) - beta.reshape((1, dim_b))) / reg
                      + np.log(u.reshape((dim_a, 1))) + np.log(v.reshape((1, dim_b))))

    Kg = get_K(alpha, beta)
    err, cpt = 1.0, 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        while True:
            uprev, vprev = u, v
            v = b / (Kg.T @ u)
            u = a / (Kg @ v)
            if np.abs(u).max() > tau or np.abs(v).max() > tau:
                alpha, beta = alpha + reg * np.log(u), beta + reg * np.log(v)
                u, v = np.full(dim_a, 1.0 / dim_a), np.full(dim_b, 1.0 / dim_b)
                Kg = get_K(alpha, beta)
            if cpt % print_period == 0:
                err = np.linalg.norm(get_Gamma(alpha, beta, u, v).sum(0) - b)
            stop = err <= stopThr or cpt + 1 >= numItermax
            if np.any(np.isnan(u)) or np.any(np.isnan(v)):
                u, v = uprev, vprev
                break
            cpt += 1
            if stop:
                break
        return get_Gamma(alpha, beta, u, v), cpt


@pytest.mark.parametrize("K", [3, 30, 50, 130, 300])
@pytest.mark.parametrize("reg", [1.0, 0.1, 0.01])
def test_entropic_plans(K, reg):
    N = 5
    P = _histograms(N, K, 3 * K, zeros=False, unequal=False)
    M = _cost(K, K)
    pr = np.array([[i, j] for i in range(N) for j in range(N)])
    G, info = engine.transport_plans(P, M, pr, regularized="reg", reg=reg, return_info=True)
    E, ginfo = engine.sinkhorn_grid(P, M, reg, precision="generic", return_info=True)
    for t, (i, j) in enumerate(pr):
        assert info["values"][t] == E[i, j] and info["iters"][t] == ginfo["iters"][i, j] and info["flags"][t] == ginfo["flags"][i, j]
    for t in range(0, len(pr), 6):                    # (the numpy restatement takes a while per pair at small reg)
        i, j = pr[t]
        ref, _ = pot_sinkhorn_stabilized(P[i], P[j], M, reg)
        v_or = O.sinkhorn2(P[i], P[j], M, reg)
        assert abs((M * ref).sum() - v_or) <= 1e-13 * max(1.0, abs(v_or)), "restatement vs oracle.sinkhorn2"
        assert np.abs(G[t] - ref).max() <= 1e-10 * ref.max()
        assert abs(info["values"][t] - (M * G[t]).sum()) <= 1e-12 * max(1.0, abs(info["values"][t]))


@pytest.mark.parametrize("K", [30, 130])
def test_entropic_plans_that_stop_at_num_iter_max(K):
    N, reg, cap = 4, 0.01, 30
    P = _histograms(N, K, 5 * K, zeros=False, unequal=False)
    M = _cost(K, K)
    pr = np.array([[i, j] for i in range(N) for j in range(N) if i != j])
    G, info = engine.transport_plans(P, M, pr, regularized="reg", reg=reg, num_iter_max=cap, return_info=True)
    E, ginfo = engine.sinkhorn_grid(P, M, reg, num_iter_max=cap, precision="generic", return_info=True)
    assert (info["iters"] == cap).all() and not (info["flags"] & _lib.FLAG_CONVERGED).any()
    for t, (i, j) in enumerate(pr):
        assert info["values"][t] == E[i, j] and info["iters"][t] == ginfo["iters"][i, j] and info["flags"][t] == ginfo["flags"][i, j]
        ref, _ = pot_sinkhorn_stabilized(P[i], P[j], M, reg, numItermax=cap)
        assert np.abs(G[t] - ref).max() <= 1e-10 * ref.max()


# ------------------------------------------------------------------------------------------------ groups
def _host_group_sum(plans, groups, G):
    acc = np.zeros((G,) + plans.shape[1:])
    for t in range(len(plans)):
        acc[groups[t]] += plans[t]
    return acc


@pytest.mark.parametrize("mode", ["unreg", "reg"])
@pytest.mark.parametrize("K", [30, 300])
def test_group_sums_are_the_host_loop_bit_for_bit(mode, K, switches):
    N = 12 if K <= 256 else 6
    n = 150 if K <= 256 else 20
    P = _histograms(N, K, 11 * K, zeros=(mode == "unreg"), unequal=(mode == "unreg"))
    M = _cost(K, K)
    pr = _pairs(N, n, K)
    groups = np.random.default_rng(K).integers(0, 5, size=n)
    groups[groups == 3] = 2                              # group 3 has no pair: its sum is 0
    per = engine.transport_plans(P, M, pr, regularized=mode)
    want = _host_group_sum(per, groups, 5)
    got = engine.transport_plans(P, M, pr, regularized=mode, groups=groups)
    np.testing.assert_array_equal(got, want)
    assert (got[3] == 0).all()
    np.testing.assert_array_equal(engine.transport_plans(P, M, pr, regularized=mode, groups=groups), got)
    switches.setenv("PILOT_OT_PLAN_CHUNK_PAIRS", "7")    # many chunks: partial sums carried across them
    try:
        np.testing.assert_array_equal(engine.transport_plans(P, M, pr, regularized=mode, groups=groups), want)
        np.testing.assert_array_equal(engine.transport_plans(P, M, pr, regularized=mode), per)
    finally:
        switches.delenv("PILOT_OT_PLAN_CHUNK_PAIRS")


def test_full_size_group_300x300_at_k50():
    N, K = 600, 50
    P = _histograms(N, K, 50, zeros=False, unequal=False)
    M = _cost(K, 50)
    src, dst = np.arange(300), np.arange(300, 600)
    pr = np.stack(np.meshgrid(src, dst, indexing="ij"), -1).reshape(-1, 2)          # 90 000 pairs: 1.8 GB of plans
    got = engine.transport_plans(P, M, pr, groups=np.zeros(len(pr), dtype=np.int64))
    acc = np.zeros((K, K))
    for c0 in range(0, len(pr), 10000):                  # the host sum in list order, 10 000 plans at a time
        for g in engine.transport_plans(P, M, pr[c0:c0 + 10000]):
            acc += g
    np.testing.assert_array_equal(got[0], acc)
    np.testing.assert_allclose(acc.sum(1), 300 * P[:300].sum(0), rtol=1e-12)


# ------------------------------------------------------------------------------------------------ tl level
def _run_distance(name, mode):
    g = load_golden(name)
    ad, cell_col = golden_adata(g)
    kw = dict(clusters_col=cell_col, sample_col="sampleID", status="status", regularized=mode, reg=0.1)
    if str(g["data_type"]) != "scRNA":
        tl.wasserstein_distance(ad, data_type="Pathomics", **kw)
    else:
        tl.wasserstein_distance(ad, emb_matrix="X_pca", **kw)
    return ad


@pytest.mark.parametrize("name", ["c2s_100x30x30", GOLDEN_REAL])
@pytest.mark.parametrize("mode", ["unreg", "reg"])
def test_tl_plans_reproduce_the_emd_matrix(name, mode, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ad = _run_distance(name, mode)
    uns = ad.uns
    keys = list(uns["proportions"].keys())
    rng = np.random.default_rng(3)
    idx = [(0, 0)] + [tuple(int(x) for x in rng.integers(0, len(keys), 2)) for _ in range(12)]
    before = set(uns.keys())
    frames = tl.transport_plans(ad, [(keys[i], keys[j]) for i, j in idx], regularized=mode, reg=0.1)
    assert set(uns.keys()) == before
    cost = uns["cost"].to_numpy()
    Mn = cost / cost.max()
    tol = 1e-12 if mode == "unreg" else 1e-5
    for (i, j), f in zip(idx, frames):
        assert list(f.index) == list(uns["cost"].index) and list(f.columns) == list(uns["cost"].columns)
        assert abs((Mn * f.to_numpy()).sum() - uns["EMD"][i, j]) <= tol


@pytest.mark.parametrize("name", ["c2s_100x30x30", GOLDEN_REAL])
def test_tl_group_transport(name, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ad = _run_distance(name, "unreg")
    uns = ad.uns
    labels = np.asarray(uns["real_labels"], dtype=object)
    statuses = list(dict.fromkeys(labels.tolist()))
    assert len(statuses) >= 2
    P = np.stack(list(uns["proportions"].values()))
    s, t = statuses[0], statuses[1]
    before = set(uns.keys())
    f = tl.group_transport(ad, s, t)
    assert set(uns.keys()) == before
    assert list(f.index) == list(uns["cost"].index) and list(f.columns) == list(uns["cost"].columns)
    np.testing.assert_allclose(f.to_numpy().sum(1), P[labels == s].mean(0), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(f.to_numpy().sum(0), P[labels == t].mean(0), rtol=1e-12, atol=1e-14)
    fr = tl.group_transport(ad, s, t, regularized="reg", reg=0.1)
    np.testing.assert_allclose(fr.to_numpy().sum(0), P[labels == t].mean(0), rtol=1e-6, atol=1e-8)
    with pytest.raises(ValueError, match="no sample has status"):
        tl.group_transport(ad, s, "no-such-status")
