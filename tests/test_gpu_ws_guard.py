"""The workspace guard (include/pilot_ot.h, "PILOT_OT_WS_GUARD"; DESIGN.md, "The workspace pool"): no result may depend on what a
pooled device temporary held before it was handed out, and no kernel may touch it past the bytes requested.

Every case is one or a few ``engine`` calls at the smallest shape that reaches every slot and every carve region of an entry point.
It runs plain, then under ``engine.ws_guard()``: there every hand-out is filled with 0xFF (float and double NaN, int -1) and
followed by a canary.  The outputs must keep the plain run's BYTES (so NaNs compare by position and payload), the canaries must be
intact, and the slots the case declares must have been handed out.  That the plain outputs are right is what the entry points' own
tests establish against the restatements; nothing is re-derived here.

CASES: name -> (callable returning a tuple of arrays, the slot names it declares).  tests/test_ws_guard_args.py holds the union
of the declared slots to the library's own list, so a slot no case reaches is a failure there.  Limits come from the library's
getters and test switches; the two constants it has no getter for are restated beside their use.
"""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp

import louvain_graphs as LG
import principal_tree_clouds as PC
import silhouette_cohorts as SC
from pilot_amd import _lib, engine, tl

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)


@contextlib.contextmanager
def _switch(**switches):
    for name, value in switches.items():
        _lib.test_switch(name, value)
    try:
        yield
    finally:
        for name in switches:
            _lib.test_switch(name, None)


def _flat(*results):
    """every array of nested tuples / dicts / namedtuples, in order"""
    out = []
    for r in results:
        if isinstance(r, dict):
            out += _flat(*(r[k] for k in sorted(r)))
        elif isinstance(r, (tuple, list)):
            out += _flat(*r)
        elif isinstance(r, engine.DeviceMatrix):
            out.append(engine.download(r))
        elif r is not None:
            out.append(np.asarray(r))
    return out


# ---- pre-pass ------------------------------------------------------------------------------------------------------------------
def _cells(C, D, K, dtype, seed, empty=None):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(C, D)).astype(dtype)
    code = rng.integers(0, K, C).astype(np.int32)
    if empty is not None:
        code[code == empty] = (empty + 1) % K
    return X, code


def _medians(C, D, K, empty=None, **switches):
    def run():
        with _switch(**switches):
            return _flat(*(engine.centroid_medians(*_cells(C, D, K, dt, 3, empty), K) for dt in DTYPES))
    return run


def _proportions_fallback():
    # 700 samples shuffled over 5000 cells: a block's rows span more samples than its LDS bins hold, the counts' global fallback
    rng = np.random.default_rng(4)
    C, N, K = 5000, 700, 6
    return _flat(engine.proportions_and_first_rows(rng.integers(0, K, C), rng.permutation(np.arange(C) % N), N, K))


def _embedding_prepass():
    out = []
    for dt, C, D, K, sw in ((np.float32, 9, 2, 4, {}), (np.float64, 5000, 3, 40, {"PILOT_OT_NO_SMALL_MEDIANS": "1"})):
        X, code = _cells(C, D, K, dt, 5)
        sample = (np.arange(C) % 7).astype(np.int32)
        up = engine.EmbeddingUpload.__new__(engine.EmbeddingUpload)
        up.SMALL_BYTES = 0                                         # (the resident embedding, whatever its size)
        up.__init__(X)
        try:
            with _switch(**sw):
                out += _flat(up.prepass(code, sample, 7, K), up.medians(code, K))
        finally:
            up.close()
    return out


# ---- cost, consumers, plans, diffusion map -------------------------------------------------------------------------------------
def _pdist(metric):
    def run():
        X = np.random.default_rng(6).uniform(0.1, 1.0, size=(7, 3))
        return _flat(engine.pdist_square(X, metric))
    return run


def _cohort_matrix(N=65):
    rng = np.random.default_rng(8)
    pts = rng.normal(size=(N, 3)) + 4.0 * (np.arange(N) % 3)[:, None]
    E = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    return E, np.arange(N) % 3


def _consumers(device):
    def run():
        E, labels = _cohort_matrix()
        A = engine.DeviceMatrix.upload(E) if device else E
        out = [engine.silhouette_of_rows(A, labels, metric="cosine", normalize_by_max=True, return_samples=True),
               engine.diffusion_kernel_of_rows(A, k=9, epsilon=0.5)]
        if not device:
            D = engine.row_distances(E, "euclidean", normalize_by_max=True)
            out += [D, engine.row_distances(E, "cosine"), engine.silhouette_precomputed(D, labels, return_samples=True),
                    engine.knn_gaussian_kernel(D, k=9, epsilon=0.5)]
            with _switch(PILOT_OT_SIL_UNSTAGED="1"):
                out.append(engine.silhouette_precomputed(D, labels, return_samples=True))
        return _flat(out)
    return run


def _plan_inputs(N, K):
    rng = np.random.default_rng(9)
    P = rng.dirichlet(np.ones(K), size=N)
    M = np.abs(rng.normal(size=(K, K)))
    M = M + M.T
    np.fill_diagonal(M, 0.0)
    pairs = np.array([(i, j) for i in range(N) for j in range(N) if i < j][:7])
    return P, M / M.max(), pairs


def _plans(regularized, groups=False, N=6, K=5, **switches):
    def run():
        P, M, pairs = _plan_inputs(N, K)
        with _switch(**switches):
            return _flat(engine.transport_plans(P, M, pairs, regularized, reg=0.1, return_info=True,
                                                groups=np.arange(len(pairs)) % 2 if groups else None))
    return run


EMD_ONE_WAVE_MAX_K = 256      # (abi_common.hpp EMD_MAX_K, no getter: above it the exact plans take the generic kernel and its row minima)


def _diffmap():
    E, _ = _cohort_matrix(40)
    Kmat = engine.diffusion_kernel_of_rows(E, k=8, epsilon=0.5)[1]
    return _flat(engine.diffusion_map_from_kernel(Kmat, n_evecs=3, epsilon=0.5, return_info=True),
                 engine.diffusion_map_of_rows(E, n_evecs=3, epsilon=0.5, k=8, return_info=True),
                 engine.diffusion_map_of_rows(engine.DeviceMatrix.upload(E), n_evecs=3, epsilon=0.5, k=8, return_info=True))


# ---- model fits, curves ----------------------------------------------------------------------------------------------------------
def _fit_data(n=12, T=70, dtype=np.float32):
    rng = np.random.default_rng(10)
    x = np.sort(rng.uniform(0, 10, n))
    Y = (rng.normal(size=(n, T)) + 0.3 * x[:, None] * rng.normal(size=T)).astype(dtype)
    Y[:, 3] = 2.0                                                # a constant target
    return Y, x


def _trajfit():
    out = []
    with _switch(PILOT_OT_TRAJFIT_CHUNK_TARGETS="64"):             # 70 targets: two chunks staged
        for dt in DTYPES:
            Y, x = _fit_data(dtype=dt)
            out += _flat(engine.trajectory_fits(Y, x, "ols", return_info=True), engine.trajectory_fits(Y, x, "huber", return_info=True))
    return out


def _normalize_log1p():
    rng = np.random.default_rng(11)
    out = []
    for dt in DTYPES:
        X = rng.integers(0, 30, (13, 21)).astype(dt)
        cols = np.array([20, 0, 7, 7], dtype=np.int32)
        res = np.empty((13, cols.size), dtype=dt)
        tl._lib_check_normalize(X, cols, res)
        out.append(res)
    return out


def _bootfit():
    rng = np.random.default_rng(12)
    out = []
    with _switch(PILOT_OT_BOOTFIT_CHUNK_PROBLEMS="2"):             # 3 problems: two chunks
        for dt in DTYPES:
            Y, x = _fit_data(12, 5, dt)
            idx = rng.integers(0, 12, (3, 12, 70))                # 70 bootstraps: two blocks of lanes, the second partly idle
            out += _flat(engine.bootstrap_huber_fits(Y, x, [4, 0, 2], [0, 1, 2], idx, return_info=True))
    return out


def _curves():
    rng = np.random.default_rng(13)
    G, T = 33, 9
    Y = rng.normal(size=(50, G)).astype(np.float32)
    offsets = np.array([2, 7, 8, 20, 20, 31, 36, 41, 46, 50])      # T segments; one of one row, one empty
    sd = engine.segment_std(Y, offsets)
    sd_cols = engine.segment_std(Y, offsets, cols=[5, 1, 32])
    params = rng.normal(size=(G, 3))
    model = np.arange(G) % 3
    times = np.linspace(0.0, 1.0, T)
    curves = engine.fitted_curves(params, model, times, noise=sd)
    plain = engine.fitted_curves(params, model, times)
    out = [sd, sd_cols, curves, plain, engine.curve_activities(curves, times)]
    for method in ("single", "complete", "average", "weighted"):
        out.append(engine.linkage_of_rows(plain, method))
    return _flat(out)


# ---- moments, CSR, group sums, PCA ---------------------------------------------------------------------------------------------
GM_MIN_SLICE_ROWS = 128       # (moments_kernels.hpp, no getter; restated as tests/test_gpu_group_moments.py does)


def _counts_matrix(n, G, dtype, seed, density=0.4):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 40, (n, G)) * (rng.uniform(size=(n, G)) < density)).astype(dtype)


def _moments_dense():
    n = 2 * GM_MIN_SLICE_ROWS + 1                                   # two slices: partials and the join
    out = []
    for dt in DTYPES:
        Y = _counts_matrix(n, 20, dt, 14)
        codes = np.arange(n) % 4 - 1                               # -1: skipped rows; 3 groups in a stride of 4
        out += _flat(engine.group_moments(Y, codes, 3), engine.group_moments(Y, codes, 3, transform="expm1", cols=[19, 0, 4]))
    return out


def _csr():
    n = engine.csr_slice_rows() + 1                                 # two slices of the column-form build
    out = []
    for dt in DTYPES:
        Y = _counts_matrix(n, 11, dt, 15, 0.2)
        codes = np.arange(n) % 3
        A = engine.DeviceCSR.upload(sp.csr_matrix(Y))
        try:
            A.normalize_log1p()
            A.build_columns()
            out += _flat(A.column_nnz(), A.group_moments(codes, 3), A.group_moments(codes, 3, cols=[10, 2]), A.densify(),
                         A.densify(cols=[9, 0, 3]))
        finally:
            A.close()
    return out


def _group_sums(sparse):
    def run():
        n = engine.group_sums_slice_rows() + 1 + 5                  # L + 1 rows in group 0 (a partial and the join), 5 in group 2, none in 1
        codes = np.r_[np.zeros(n - 5, dtype=int), np.full(5, 2)]
        out = []
        for dt in DTYPES:
            Y = _counts_matrix(n, engine.group_sums_col_block() + 3 if sparse else 9, dt, 16, 0.1 if sparse else 0.6)
            A = engine.DeviceCSR.upload(sp.csr_matrix(Y)) if sparse else Y
            try:
                out += _flat(engine.group_sums(A, codes, 3), engine.group_sums(A, codes, 3, cols=[4, 0, 4]))
            finally:
                if sparse:
                    A.close()
        return out
    return run


def _pca(sparse):
    def run():
        rng = np.random.default_rng(17)
        out = []
        for dt in DTYPES:
            Y = (_counts_matrix(60, 20, np.float64, 17, 0.5) * rng.uniform(0.5, 1.5, 20)).astype(dt)
            A = engine.DeviceCSR.upload(sp.csr_matrix(Y)) if sparse else Y
            try:
                out += _flat(engine.pca(A, 3, return_info=True), engine.pca(A, 3, scale=False, cols=np.arange(19, 3, -1), return_info=True))
            finally:
                if sparse:
                    A.close()
        return out
    return run


# ---- neighbours, communities, silhouette, principal tree -------------------------------------------------------------------------
def _knn(D, metrics=("euclidean", "cosine")):
    def run():
        X = np.random.default_rng(18).normal(size=(300, D))
        out = []
        for dt in DTYPES:
            for metric in metrics:
                out += _flat(engine.knn(X.astype(dt), 5, metric), engine.knn(X.astype(dt), 5, metric, rows=(7, 40)))
        return out
    return run


def _knn_smooth():
    X = np.random.default_rng(19).normal(size=(300, 4))
    X[5] = X[6]                                                    # a zero distance: rho skips it
    return _flat(engine.knn_smooth(engine.knn(X, 5)[1], 6))


def _communities(fn, graph, coarsens=False, **switches):
    def run():
        with _switch(**switches):
            labels, info = getattr(engine, fn)(graph(), return_info=True)
        assert info["levels"] >= 2 or not coarsens, "the case must coarsen at least once"
        return _flat(labels, {k: np.float64(v) for k, v in info.items()})
    return run


def _silhouette_points():
    points, group, _ = SC.cohort("three_groups")
    out = []
    for dt in DTYPES:
        for metric in ("euclidean", "cosine"):
            out += _flat(engine.silhouette_samples((points + 1.0).astype(dt), group, metric, return_score=True)[0])
    return out


def _principal_tree():
    out = []
    for dt in DTYPES:
        name, n, m, seed = PC.FITS[0]
        X, Y0, S, centre = PC.fit_case(name, n, m, seed, dt)
        fits = engine.elastic_fit(X, np.stack([Y0, Y0[::-1]]), np.stack([S, S]), centre)
        edges = [(a, a + 1) for a in range(m - 1)]
        out += _flat(tuple(fits), engine.point_moments(X), engine.tree_pseudotime(X, fits.nodes[0], edges, source=0))
    return out


# ---- rank sums, negative-binomial fits -----------------------------------------------------------------------------------------
def _rank_sums(sparse):
    def run():
        w, W, T = engine.rank_sums_limits()
        lengths = (0, w, W, max(W, T) + 1)                          # one column per bin; the last is no power of two: padded records
        n = lengths[-1] + 3
        rng = np.random.default_rng(20)
        codes = np.arange(n) % 3
        codes[-3:] = -1                                            # skipped rows
        out = []
        for dt in DTYPES:
            Y = np.zeros((n, len(lengths)), dtype=dt)
            for j, L in enumerate(lengths):
                Y[:L, j] = rng.integers(1, 50, L)                  # ties everywhere
            A = engine.DeviceCSR.upload(sp.csr_matrix(Y)) if sparse else Y
            try:
                out += _flat(engine.rank_sums(A, codes, 3), engine.rank_sums(A, codes, 3, cols=[3, 1]))
            finally:
                if sparse:
                    A.close()
        return out
    return run


def _nb():
    rng = np.random.default_rng(21)
    m, k, G = 12, 3, 65
    codes = np.arange(m) % k
    sf = rng.uniform(0.5, 2.0, m)
    out = []
    for dt in DTYPES:
        Y = rng.poisson(rng.uniform(1, 60, G) * sf[:, None]).astype(dt)
        Y[:, 7] = 0                                                # a gene of zeros: NaN
        x, info = engine.nb_dispersions(Y, codes, k, sf, return_info=True)
        xp = engine.nb_dispersions(Y, codes, k, sf, log_prior_mean=np.where(np.isnan(x), 0.0, x) + 0.1, prior_var=0.5)
        disp = engine.nb_clip(np.exp(x), m)
        two = codes % 2
        far = np.where(np.arange(G) % 2, 3.0, -3.0)
        out += _flat(x, info, xp, engine.nb_group_fits(Y, codes, k, sf, disp, return_info=True),
                     engine.nb_shrink(Y, two, sf, disp, far, prior_scale=0.7, return_info=True))
    return out


CASES = {
    "medians_one_launch": (_medians(9, 2, 4, empty=2), ["WS_PREPASS_X", "WS_PREPASS"]),
    "medians_general": (_medians(5000, 3, 40, PILOT_OT_NO_SMALL_MEDIANS="1"), ["WS_PREPASS_X", "WS_PREPASS"]),
    "medians_windowed": (_medians(500, 70, 2, PILOT_OT_NO_SMALL_MEDIANS="1"), ["WS_PREPASS_X", "WS_PREPASS"]),
    "proportions_global_fallback": (_proportions_fallback, ["WS_PREPASS"]),
    "embedding_prepass": (_embedding_prepass, ["WS_PREPASS"]),
    "pdist_cosine": (_pdist("cosine"), ["WS_COST_X", "WS_COST_C"]),
    "pdist_seuclidean": (_pdist("seuclidean"), ["WS_COST_X", "WS_COST_C"]),
    "pdist_mahalanobis": (_pdist("mahalanobis"), ["WS_COST_X", "WS_COST_C", "WS_COST_AUX"]),
    "pdist_jensenshannon": (_pdist("jensenshannon"), ["WS_COST_X", "WS_COST_C"]),
    "consumers_host": (_consumers(False), ["WS_CONS_E", "WS_CONS_D", "WS_CONS_MAX", "WS_CONS_LABELS", "WS_CONS_SIZES", "WS_CONS_SCORES",
                                           "WS_CONS_K"]),
    "consumers_device": (_consumers(True), ["WS_CONS_D", "WS_CONS_MAX", "WS_CONS_LABELS", "WS_CONS_SIZES", "WS_CONS_SCORES", "WS_CONS_K"]),
    "plans_exact": (_plans("unreg"), ["WS_PLAN_P", "WS_PLAN_M", "WS_PLAN_PI", "WS_PLAN_PJ", "WS_PLAN_VAL", "WS_PLAN_IT", "WS_PLAN_FL",
                                      "WS_PLAN_Q", "WS_PLAN_PLANS", "WS_PLAN_SLAB"]),
    "plans_entropic": (_plans("reg"), ["WS_PLAN_P", "WS_PLAN_M", "WS_PLAN_PI", "WS_PLAN_PJ", "WS_PLAN_VAL", "WS_PLAN_IT", "WS_PLAN_FL",
                                       "WS_PLAN_Q", "WS_PLAN_PLANS", "WS_PLAN_KWS"]),
    "plans_group_means_exact": (_plans("unreg", True, PILOT_OT_PLAN_CHUNK_PAIRS="4"), ["WS_PLAN_ACC", "WS_PLAN_GOFF", "WS_PLAN_GIDX"]),
    "plans_group_means_entropic": (_plans("reg", True, PILOT_OT_PLAN_CHUNK_PAIRS="4"), ["WS_PLAN_ACC", "WS_PLAN_GOFF", "WS_PLAN_GIDX"]),
    "plans_exact_generic": (_plans("unreg", N=5, K=EMD_ONE_WAVE_MAX_K + 1), ["WS_PLAN_SLAB", "WS_PLAN_ROWMIN"]),
    "diffusion_map": (_diffmap, ["WS_DM_S", "WS_DM_V", "WS_DM_VEC", "WS_DM_Z", "WS_DM_PSI", "WS_DM_E", "WS_DM_D", "WS_DM_K", "WS_DM_MAX",
                                 "WS_DM_OUT"]),
    "trajectory_fits": (_trajfit, ["WS_TF_U", "WS_TF_Y", "WS_TF_OUT"]),
    "normalize_log1p": (_normalize_log1p, ["WS_TF_Y", "WS_TF_OUT", "WS_TF_COLS"]),
    "bootstrap_huber_fits": (_bootfit, ["WS_BOOT_U", "WS_BOOT_OUT", "WS_BOOT_IDX", "WS_BOOT_Y"]),
    "curves": (_curves, ["WS_CV_Y", "WS_CV_IN", "WS_CV_AUX", "WS_CV_OUT", "WS_CV_BMAX", "WS_CV_CHAIN", "WS_CV_Z"]),
    "group_moments_dense": (_moments_dense, ["WS_GM_Y", "WS_GM_AUX", "WS_GM_PART", "WS_GM_COUNT", "WS_GM_OUT"]),
    "csr": (_csr, ["WS_CSR_COUNTS", "WS_CSR_TOTAL", "WS_CSR_CODES", "WS_CSR_COLS", "WS_CSR_OUT"]),
    "group_sums_dense": (_group_sums(False), ["WS_GS_Y", "WS_GS_AUX", "WS_GS_PART", "WS_GS_OUT"]),
    "group_sums_csr": (_group_sums(True), ["WS_GS_AUX", "WS_GS_PART", "WS_GS_OUT"]),
    "pca_dense": (_pca(False), ["WS_PCA_V", "WS_PCA_VEC", "WS_PCA_Z", "WS_PCA_PCS", "WS_PCA_SCORES", "WS_PCA_STATS", "WS_PCA_COLS", "WS_PCA_Y",
                                "WS_PCA_S", "WS_PCA_PARTW", "WS_GM_Y", "WS_GM_OUT"]),
    "pca_csr": (_pca(True), ["WS_PCA_V", "WS_PCA_VEC", "WS_PCA_Z", "WS_PCA_PCS", "WS_PCA_SCORES", "WS_PCA_STATS", "WS_PCA_COLS", "WS_PCA_POS",
                             "WS_PCA_SIDX", "WS_PCA_SVAL", "WS_PCA_CSVAL", "WS_CSR_OUT"]),
    "knn": (_knn(8), ["WS_KNN_X", "WS_KNN_UNIT", "WS_KNN_FLAGS", "WS_KNN_BEST_D", "WS_KNN_BEST_I", "WS_KNN_OUT_D", "WS_KNN_OUT_I"]),
    "knn_wide_rows": (_knn(_lib.ELASTIC_MAX_D + 1, ("cosine",)), ["WS_KNN_X", "WS_KNN_UNIT", "WS_KNN_BEST_D", "WS_KNN_BEST_I"]),
    "knn_smooth": (_knn_smooth, ["WS_KNN_SM_IN", "WS_KNN_SM_OUT"]),
    "louvain": (_communities("louvain", LG.ring_of_cliques, True), ["WS_LV_VAL0", "WS_LV_VAL1", "WS_LV_DEG0", "WS_LV_DEG1", "WS_LV_IDX0", "WS_LV_IDX1",
                                                              "WS_LV_TOT", "WS_LV_SUMS", "WS_LV_INT", "WS_LV_FLAG", "WS_LV_ECOMM", "WS_LV_NKEYS",
                                                              "WS_LV_EKEYS", "WS_LV_CNT"]),
    "leiden": (_communities("leiden", LG.ring_of_cliques, True), ["WS_LV_INT", "WS_LV_NKEYS", "WS_LV_EKEYS", "WS_LD_INT", "WS_LD_DBL"]),
    # node 0 of hub() has 150 neighbours: above the one-wave limit; the switch puts it in the long bin and others in the workgroup bin
    "louvain_hub": (_communities("louvain", LG.hub), ["WS_LV_INT", "WS_LV_ECOMM"]),
    "louvain_hub_bins": (_communities("louvain", LG.hub, PILOT_OT_LOUVAIN_BINS="4,32"), ["WS_LV_INT", "WS_LV_ECOMM"]),
    "leiden_hub_bins": (_communities("leiden", LG.hub, PILOT_OT_LOUVAIN_BINS="4,32"), ["WS_LD_INT", "WS_LD_DBL", "WS_LV_ECOMM"]),
    "silhouette_points": (_silhouette_points, ["WS_SIL_X", "WS_SIL_UNIT", "WS_SIL_FLAGS", "WS_SIL_SORTED", "WS_SIL_ORDER", "WS_SIL_OFFSETS",
                                               "WS_SIL_OUT"]),
    "principal_tree": (_principal_tree, ["WS_PT_X", "WS_PT_FLAGS", "WS_PT_Y", "WS_PT_YT", "WS_PT_S", "WS_PT_CENTRE", "WS_PT_STATE", "WS_PT_ITERS",
                                         "WS_PT_ENERGY", "WS_PT_COUNTS", "WS_PT_SUMS", "WS_PT_PCOUNTS", "WS_PT_PSUMS", "WS_PT_PMSE", "WS_PT_PART",
                                         "WS_PT_OUT"]),
    "rank_sums_dense": (_rank_sums(False), ["WS_RS_Y", "WS_RS_INT", "WS_RS_LL", "WS_RS_REC", "WS_RS_OUT"]),
    "rank_sums_csr": (_rank_sums(True), ["WS_RS_INT", "WS_RS_LL", "WS_RS_REC", "WS_RS_OUT", "WS_CSR_COUNTS", "WS_CSR_TOTAL"]),
    "nb_glm": (_nb, ["WS_NB_Y", "WS_NB_INT", "WS_NB_SF", "WS_NB_BAD", "WS_NB_PRIOR", "WS_NB_OUT", "WS_NB_FIT_INT"]),
}


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("name", sorted(CASES))
def test_results_do_not_depend_on_the_scratch(name):
    run, slots = CASES[name]
    plain = run()
    with engine.ws_guard() as guard:
        guarded = run()
    seen, damage = guard.result
    assert len(plain) == len(guarded) and len(plain) > 0
    for i, (a, b) in enumerate(zip(plain, guarded)):
        assert a.dtype == b.dtype and a.shape == b.shape, "output %d" % i
        differ = np.flatnonzero((_bytes(a).reshape(a.size, -1) != _bytes(b).reshape(b.size, -1)).any(axis=1))
        assert differ.size == 0, "output %d of %s read scratch nobody wrote: %d of %d elements change under the guard, the first is %d" % (
            i, name, differ.size, a.size, differ[0])
    assert damage is None, "an access past the request: (slot, offset past the request, request bytes) = %r" % (damage,)
    assert set(slots) <= seen, "declared slots not handed out: %s" % sorted(set(slots) - seen)
    # guard off: the switch is cleared, and a plain call makes no guard fill
    run()
    assert engine.ws_guard_report() == (set(), None)


def test_guard_selftest_names_the_damaged_slot():
    """the control: a guard that could not see a damaged canary would pass every case above"""
    Y = _counts_matrix(9, 4, np.float32, 1)
    with engine.ws_guard("selftest") as guard:
        engine.group_sums(Y, np.arange(9) % 2, 2)
    seen, damage = guard.result
    assert damage == ("WS_GS_Y", 7, Y.nbytes)                    # the first slot group_sums takes: the staged matrix, all of it requested
    assert "WS_GS_Y" in seen
    with engine.ws_guard() as guard:                               # and the record does not outlive its report
        engine.group_sums(Y, np.arange(9) % 2, 2)
    assert guard.damage is None and "WS_GS_OUT" in guard.seen
