"""K15 on the device: engine.pca / DeviceCSR.pca (pca_kernels.hpp, the shared Lanczos step) and tl.pca / tl.extract_annot_expression
against tests/pca_restatement.py, which forms the standardised matrix densely in float64 and takes np.linalg.svd of it.

Inputs: Poisson counts from a low-rank gamma model (as many factors as components are tested, strengths 1 .. 0.45, so the wanted
part of the spectrum is separated), with an all-zero gene (sigma -> 1), a gene expressed in one cell (its z of about sqrt(n) is
clipped at max_value), an empty row and, in every third row, indices stored in descending order.  Shapes: 257 x 70, k = 6 (the
basis becomes complete; rows not a multiple of 64); 1100 x 300, k = 12 (three 512-row slices of the column form); 700 x 1300,
k = 8 (more columns than the 1024 basis vectors: only the residual test can end the run).

Condition on every input, asserted on the restatement alone (``_reference``): the smallest relative gap
(lambda_c - lambda_{c+1}) / lambda_0 over the tested components is >= 1e-3, and with scaling at least one entry is clipped.

Bounds.  A Ritz pair is accepted at a residual of 1e-12 lambda_0, so an eigenvector is off by at most residual / gap =
1e-12 / 1e-3 = 1e-9 in angle, and a score column by that times the largest singular direction it can leak into; f64 rounding of
the sums (a few hundred terms, 1e-13 relative) is far inside.  Scores and PCs: per column <= 1e-8 max|reference column|.
Eigenvalues converge with the square of the vector error: variance and variance_ratio <= 1e-10 of the leading one.  The sparse
and the dense route are held to each other by the same bounds.

The gap condition keeps repeated eigenvalues out of those inputs.  The orthogonal designs further down are the inputs where wanted
eigenvalues repeat exactly or nearly (test_repeated_eigenvalues_are_found), held to contracts that do not need a gap: the variances
with their multiplicity, residuals, orthonormality and the projector of every eigenvalue cluster inside the first k."""
import functools

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import pca_restatement as PR
from pilot_amd import _lib, engine, tl

pytestmark = pytest.mark.gpu

SHAPES = {"complete": (257, 70, 6, 2), "slices": (1100, 300, 12, 3), "wide": (700, 1300, 8, 1)}     # n, D, k, seed
MODES = {"scaled": dict(scale=True, max_value=10.0), "raw": dict(scale=False), "unclipped": dict(scale=True, max_value=None)}
TOL_VEC, TOL_VAR, MIN_GAP = 1e-8, 1e-10, 1e-3


@functools.lru_cache(maxsize=None)
def _counts(shape):
    n, D, k, seed = SHAPES[shape]
    rng = np.random.default_rng(seed)
    L = rng.gamma(1.0, 1.0, (n, k)) * np.linspace(1.0, 0.45, k)
    W = rng.gamma(0.4, 1.0, (k, D))
    K = rng.poisson(0.25 * (L @ W)).astype(np.float64)
    K[:, 3] = 0.0                                                  # a gene nobody expresses
    K[:, 5] = 0.0
    K[n // 3, 5] = 4.0                                             # a gene one cell expresses
    K[7, :] = 0.0                                                  # a cell without counts
    K.setflags(write=False)
    return K


def _csr(K, dtype):
    """K as CSR with the indices of every third row in descending order"""
    indptr, indices, data = [0], [], []
    for i in range(K.shape[0]):
        js = np.flatnonzero(K[i])
        if i % 3 == 0:
            js = js[::-1]
        indices.append(js)
        data.append(K[i, js])
        indptr.append(indptr[-1] + js.size)
    X = sp.csr_matrix((np.concatenate(data).astype(dtype), np.concatenate(indices).astype(np.int32), np.array(indptr, dtype=np.int64)),
                      shape=K.shape)
    assert not X.has_sorted_indices and X.dtype == dtype
    return X


def _subset(shape):
    """two thirds of the columns in scrambled order, the two special genes among them"""
    D = SHAPES[shape][1]
    perm = np.random.default_rng(99).permutation(D)
    cols = perm[: 2 * D // 3]
    cols = np.concatenate([cols, [c for c in (3, 5) if c not in cols]]).astype(np.int64)
    return cols[np.random.default_rng(98).permutation(cols.size)]


def _gap(all_var, k):
    return float(((all_var[:k] - all_var[1:k + 1]) / all_var[0]).min())


@functools.lru_cache(maxsize=None)
def _reference(shape, mode, subset=False):
    K, k = _counts(shape), SHAPES[shape][2]
    cols = _subset(shape) if subset else None
    kw = MODES[mode]
    ref = PR.pca(K, k, kw["scale"], kw.get("max_value"), cols=cols)
    gap = _gap(ref[4], k)
    print("%s / %s%s: min relative gap %.2e" % (shape, mode, " / subset" if subset else "", gap))
    assert gap >= MIN_GAP
    if mode == "scaled":
        assert PR.clipped(K, 10.0, cols) >= 1
    return ref[:4]


def _worst(got, want):
    """(scores, pcs: max over the columns of |diff| / max|reference column|; variance, ratio: |diff| / leading)"""
    out = []
    for g, w in zip(got[:2], want[:2]):
        assert g.shape == w.shape and g.dtype == np.float64
        out.append(float((np.abs(g - w).max(axis=0) / np.abs(w).max(axis=0)).max()))
    for g, w in zip(got[2:4], want[2:4]):
        assert g.shape == w.shape and g.dtype == np.float64
        out.append(float(np.abs(g - w).max() / w[0]))
    return out


def _check(got, want, what):
    e = _worst(got, want)
    print("%s: scores %.2e, PCs %.2e (tol %.0e); variance %.2e, ratio %.2e (tol %.0e)" % (what, e[0], e[1], TOL_VEC, e[2], e[3], TOL_VAR))
    assert e[0] <= TOL_VEC and e[1] <= TOL_VEC and e[2] <= TOL_VAR and e[3] <= TOL_VAR, what


def _run(shape, dtype, route, mode="scaled", cols=None, **kw):
    K, k = _counts(shape), SHAPES[shape][2]
    if route == "sparse":
        Y = engine.DeviceCSR.upload(_csr(K, dtype))
    elif route == "device":
        Y = engine.DeviceMatrix.upload(K.astype(dtype))
    else:
        Y = np.ascontiguousarray(K.astype(dtype))
    return engine.pca(Y, n_comps=k, cols=cols, **MODES[mode], **kw)


def _bits(out):
    return [np.ascontiguousarray(a).view(np.uint64) for a in out[:4]]


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


@pytest.mark.parametrize("route", ["sparse", "dense"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_parity(shape, dtype, route):
    got = _run(shape, dtype, route, return_info=True)
    info = got[4]
    print("%s %s %s: %d Lanczos steps" % (shape, np.dtype(dtype).name, route, info["steps"]))
    assert info["converged"] and not info["rank_deficient"] and info["flags"] == 0
    n, D, k, _ = SHAPES[shape]
    assert k <= info["steps"] <= min(D, 1024)
    if shape == "wide":
        assert info["steps"] < 1024                               # the residual test ended it, not the basis cap
    _check(got, _reference(shape, "scaled"), "%s %s %s" % (shape, np.dtype(dtype).name, route))
    at = np.abs(got[0]).argmax(axis=0)
    assert (got[0][at, np.arange(k)] > 0).all()                    # the sign rule
    assert np.abs(got[1].T @ got[1] - np.eye(k)).max() <= 1e-12    # orthonormal directions


@pytest.mark.parametrize("route", ["sparse", "dense"])
@pytest.mark.parametrize("mode", ["raw", "unclipped"])
@pytest.mark.parametrize("shape", ["complete", "slices"])
def test_scale_modes(shape, mode, route):
    _check(_run(shape, np.float64, route, mode), _reference(shape, mode), "%s %s %s" % (shape, mode, route))


@pytest.mark.parametrize("route", ["sparse", "dense", "device"])
@pytest.mark.parametrize("shape", ["complete", "slices"])
def test_column_subset_in_scrambled_order(shape, route):
    cols = _subset(shape)
    assert not (np.diff(cols) > 0).all() and {3, 5} <= set(cols.tolist())
    got = _run(shape, np.float32, route, cols=cols)
    assert got[1].shape == (cols.size, SHAPES[shape][2])
    _check(got, _reference(shape, "scaled", True), "%s subset %s" % (shape, route))


def test_device_columns_view():
    """a column window of a DeviceMatrix, its leading dimension the parent's"""
    K, k = _counts("complete"), 5
    D = engine.DeviceMatrix.upload(np.ascontiguousarray(K))
    got = engine.pca(engine.device_columns(D, 2, 50), n_comps=k)
    ref = PR.pca(K[:, 2:50], k)
    assert _gap(ref[4], k) >= MIN_GAP
    _check(got, ref[:4], "device_columns")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_routes_agree(shape):
    a, b = _run(shape, np.float64, "sparse"), _run(shape, np.float64, "dense")
    _check(a, b, "%s sparse against dense" % shape)


@pytest.mark.parametrize("route", ["sparse", "dense"])
@pytest.mark.parametrize("shape", ["complete", "slices"])
def test_repeated_calls_and_both_dtypes_give_the_same_bits(shape, route):
    """counts are float32-representable and all arithmetic is float64"""
    a = _run(shape, np.float64, route)
    assert _same_bits(a, _run(shape, np.float64, route))
    assert _same_bits(a, _run(shape, np.float32, route))
    if route == "dense":
        assert _same_bits(a, _run(shape, np.float64, "device"))


def test_one_handle_serves_several_calls_and_stays_as_it_was():
    K = _counts("complete")
    S = engine.DeviceCSR.upload(_csr(K, np.float32))
    a = S.pca(n_comps=6)
    nnz = S.column_nnz()
    b = S.pca(n_comps=6)
    assert _same_bits(a, b) and np.array_equal(nnz, (K != 0).sum(axis=0))
    assert np.array_equal(engine.download(S.densify()), K.astype(np.float32))
    lead = S.pca(n_comps=2)                                        # fewer components: the same leading ones
    _check(lead, tuple(x[..., :2] for x in _reference("complete", "scaled")), "k = 2")


def _rank_one(n=90, D=24):
    """two identical latent factors and nothing else: every standardised column is the same vector"""
    rng = np.random.default_rng(4)
    l = rng.gamma(1.0, 1.0, n)
    l[::5] = 0.0
    w = rng.gamma(2.0, 1.0, D) + 0.5
    return np.stack([l, l], axis=1) @ np.stack([w, w], axis=0)


@pytest.mark.parametrize("route", ["sparse", "dense"])
def test_a_rank_deficient_matrix_is_refused(route):
    Y = _rank_one()
    assert np.linalg.matrix_rank(PR.standardise(Y) - PR.standardise(Y).mean(0)) == 1
    arg = engine.DeviceCSR.upload(sp.csr_matrix(Y)) if route == "sparse" else Y
    with pytest.raises(ValueError, match="rank"):
        engine.pca(arg, n_comps=3)
    out = engine.pca(arg, n_comps=3, return_info=True)
    assert out[4]["rank_deficient"] and out[4]["flags"] & _lib.PCA_RANK_DEFICIENT
    one = engine.pca(arg, n_comps=1)                               # within the rank: fine
    ref = PR.pca(Y, 1)
    _check(one, ref[:4], "rank one, k = 1")
    with pytest.raises(ValueError, match="rank"):                  # constant columns: nothing to find
        engine.pca(np.ones((10, 6)), n_comps=2)


def test_small_basis_is_not_converged(switches):
    switches.setenv("PILOT_OT_PCA_BASIS", "14")
    out = _run("wide", np.float32, "sparse", return_info=True)
    assert not out[4]["converged"] and out[4]["flags"] & _lib.PCA_NOT_CONVERGED and out[4]["steps"] == 14
    with pytest.raises(ValueError, match="converge"):
        _run("wide", np.float32, "sparse")
    switches.delenv("PILOT_OT_PCA_BASIS")
    assert _run("wide", np.float32, "sparse", return_info=True)[4]["converged"]


# ---- repeated eigenvalues: orthogonal designs ------------------------------------------------------------------------------------
# Columns 1 .. D of the Sylvester matrix of order 64 are orthogonal, have zero sum and entries +-1, so Y = (H[:, 1:D+1] + 1) * s has
# entries 0 or 2 s_j (exact in float32 for integer s, true zeros in the CSR), centres to H * s and has Zc^T Zc = 64 diag(s^2) exactly:
# the variances are 64 s_j^2 / 63 with every multiplicity known.  A Krylov space grown from one vector holds one direction per
# distinct eigenvalue, so these are the inputs a single-vector Lanczos run gets wrong unless it looks for hidden copies.
def _sylvester64():
    H = np.array([[1.0]])
    for _ in range(6):
        H = np.kron(H, np.array([[1.0, 1.0], [1.0, -1.0]]))
    return H


DESIGNS = {
    "pairs": (3, 3, 2, 2, 1, 1, 1, 1, 1, 1),
    "null": (4, 3, 0, 3, 2, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0),                    # three all-zero columns among the others
    "near-6": (3, 3 * (1 - 1e-6), 2, 1, 1, 1, 1, 1),
    "near-9": (3, 3 * (1 - 1e-9), 2, 1, 1, 1, 1, 1),
}
DESIGN_CASES = ([("pairs", k, False, dt) for k in (1, 2, 3, 4) for dt in (np.float32, np.float64)]
                + [("null", k, False, dt) for k in (2, 3) for dt in (np.float32, np.float64)]
                + [(d, k, False, np.float64) for d in ("near-6", "near-9") for k in (2, 3)]
                + [("pairs", k, True, dt) for k in (2, 5) for dt in (np.float32, np.float64)])


@functools.lru_cache(maxsize=None)
def _design(name, scale):
    """(Y, A = Zc^T Zc of the restatement's float64 Z, Zc, every reference variance sorted, eigenvectors of A to match)"""
    s = np.array(DESIGNS[name], dtype=np.float64)
    D = s.size
    H = _sylvester64()
    Y = (H[:, 1:D + 1] + 1.0) * s[None, :]
    if scale:
        want = np.ones(D)                                          # every column has unit variance: A = 63 I
    else:
        want = np.sort(64.0 * s ** 2 / 63.0)[::-1]
    all_var = PR.pca(Y, 1, scale, 10.0 if scale else None)[4]
    assert all_var.shape == (D,)
    assert (np.abs(all_var - want) <= 1e-13 * np.where(want > 0, want, want[0])).all(), (all_var, want)
    Z = PR.standardise(Y, scale, 10.0)
    Zc = Z - Z.mean(axis=0)
    A = Zc.T @ Zc
    if not scale:
        assert np.array_equal(A, np.diag(64.0 * s ** 2)) or name.startswith("near")
    lam, vec = np.linalg.eigh(A)
    for a in (Y, A, Zc, want, vec):
        a.setflags(write=False)
    return Y, A, Zc, want, vec[:, ::-1]


def _clusters_within(lam, k, gap):
    """index ranges [a, b) of the descending spectrum lam: maximal runs whose members are mutually closer than gap, that lie
    wholly inside the first k, and that are at least gap away from everything else"""
    out, a = [], 0
    while a < k:
        b = a + 1
        while b < lam.size and lam[b - 1] - lam[b] < gap:
            b += 1
        if b <= k and lam[a] - lam[b - 1] < gap:
            out.append((a, b))
        a = b
    return out


def _design_arg(Y, route, dtype):
    if route == "sparse":
        X = sp.csr_matrix(Y.astype(dtype))
        assert X.nnz == int((Y != 0).sum())
        return engine.DeviceCSR.upload(X)
    return np.ascontiguousarray(Y.astype(dtype))


@pytest.mark.parametrize("route", ["sparse", "dense"])
@pytest.mark.parametrize("name,k,scale,dtype", DESIGN_CASES)
def test_repeated_eigenvalues_are_found(name, k, scale, dtype, route):
    """Every contract of test_parity on inputs whose wanted eigenvalues repeat (or nearly do), where a column of the answer is
    defined only up to a rotation inside its eigenspace: the variances with their multiplicity, orthonormal directions that are
    eigenvectors (residual <= 1e-10 lambda_0: the solver's 1e-12 with the factor 100 the diffusion-map tests allow for the
    reference product), scores = Zc pcs, the sign rule, and for every cluster of eigenvalues inside the first k the projector."""
    Y, A, Zc, want, vec = _design(name, scale)
    n, D = Y.shape
    if dtype == np.float32:
        assert np.array_equal(Y.astype(np.float32).astype(np.float64), Y)
    kw = dict(scale=True, max_value=10.0) if scale else dict(scale=False)
    scores, pcs, variance, ratio, info = engine.pca(_design_arg(Y, route, dtype), n_comps=k, return_info=True, **kw)
    what = "%s k=%d scale=%s %s %s" % (name, k, scale, np.dtype(dtype).name, route)
    print("%s: %d Lanczos steps, flags %d, variance %s" % (what, info["steps"], info["flags"], variance))
    assert info["converged"] and not info["rank_deficient"] and info["flags"] == 0, (what, info)
    e_var = np.abs(variance - want[:k]).max() / want[0]
    e_ratio = np.abs(ratio - want[:k] / want.sum()).max() / (want[0] / want.sum())
    lam = variance * (n - 1)
    resid = np.abs(A @ pcs - pcs * lam[None, :]).max() / lam[0]
    ortho = np.abs(pcs.T @ pcs - np.eye(k)).max()
    proj = Zc @ pcs
    e_scores = (np.abs(scores - proj).max(axis=0) / np.abs(proj).max(axis=0)).max()
    print("%s: variance %.2e, ratio %.2e (tol %.0e); residual %.2e (1e-10); orthonormal %.2e (1e-12); scores %.2e (tol %.0e)"
          % (what, e_var, e_ratio, TOL_VAR, resid, ortho, e_scores, TOL_VEC))
    assert e_var <= TOL_VAR and e_ratio <= TOL_VAR, what
    assert ortho <= 1e-12 and resid <= 1e-10, what
    assert e_scores <= TOL_VEC, what
    at = np.abs(scores).argmax(axis=0)
    assert (scores[at, np.arange(k)] > 0).all(), what              # the sign rule
    for a, b in _clusters_within(want * (n - 1), k, MIN_GAP * want[0] * (n - 1)):
        e_proj = np.abs(pcs[:, a:b] @ pcs[:, a:b].T - vec[:, a:b] @ vec[:, a:b].T).max()
        print("%s: cluster [%d, %d): projector %.2e (tol %.0e)" % (what, a, b, e_proj, TOL_VEC))
        assert e_proj <= TOL_VEC, what


def test_cluster_rule_of_the_design_cases():
    """the clusters the projector check sees, on the reference alone: a cut cluster is left to the residual check"""
    gap = MIN_GAP * 9.0
    lam = np.array([9.0, 9.0, 4.0, 4.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    assert [_clusters_within(lam, k, gap) for k in (1, 2, 3, 4)] == [[], [(0, 2)], [(0, 2)], [(0, 2), (2, 4)]]
    assert _clusters_within(np.array([16.0, 9.0, 9.0, 4.0, 1.0]), 2, gap) == [(0, 1)]
    assert _clusters_within(np.ones(10), 5, gap) == []


@pytest.mark.parametrize("route", ["sparse", "dense"])
def test_a_breakdown_without_room_to_verify_is_not_converged(route, switches):
    """Three basis vectors hold the three distinct eigenvalues of the pairs design and nothing can look behind them: the call must
    say so instead of returning (9, 4) for the variances (9, 9)."""
    Y = _design("pairs", False)[0]
    switches.setenv("PILOT_OT_PCA_BASIS", "3")
    out = engine.pca(_design_arg(Y, route, np.float64), n_comps=2, scale=False, return_info=True)
    print("basis 3, %s: %d steps, flags %d, variance %s" % (route, out[4]["steps"], out[4]["flags"], out[2]))
    assert not out[4]["converged"] and out[4]["flags"] & _lib.PCA_NOT_CONVERGED
    with pytest.raises(ValueError):
        engine.pca(_design_arg(Y, route, np.float64), n_comps=2, scale=False)


def test_non_finite_values_on_the_device_are_refused():
    K = _counts("complete").copy()
    K[11, 20] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        engine.pca(engine.DeviceMatrix.upload(K), n_comps=3)
    X = _csr(K, np.float64)
    with pytest.raises(ValueError, match="non-finite"):
        engine.DeviceCSR.upload(X).pca(n_comps=3)
    cols = np.array([c for c in range(K.shape[1]) if c != 20])
    _check(engine.DeviceCSR.upload(X).pca(n_comps=3, cols=cols), PR.pca(K, 3, cols=cols)[:4], "the NaN column left out")


# ---- tl -------------------------------------------------------------------------------------------------------------------------
class _Adata:
    def __init__(self, X, obs, var_names):
        self.X, self.obs, self.var_names = X, obs, var_names
        self.obsm, self.varm, self.uns = {}, {}, {}


def _adata(kind, dtype=np.float32, shape="slices"):
    K = _counts(shape)
    n, D = K.shape
    rng = np.random.default_rng(8)
    obs = pd.DataFrame({"ct": rng.choice(["T", "B", "NK"], n), "sample": rng.choice(["p1", "p2", "p3"], n),
                        "state": rng.choice(["case", "control"], n)}, index=["cell%d" % i for i in range(n)])
    X = _csr(K, dtype) if kind == "sparse" else np.ascontiguousarray(K.astype(dtype))
    return _Adata(X, obs, ["g%d" % j for j in range(D)]), K


def _tl_check(ad, ref, k, cols, key="X_pca"):
    sc = ad.obsm[key]
    assert sc.dtype == np.float32 and sc.shape == (ad.X.shape[0], k)
    colmax = np.abs(ref[0]).max(axis=0)
    assert (np.abs(sc - ref[0]) <= (TOL_VEC + 2.0 ** -24) * colmax).all()        # the f64 bound and one rounding to float32
    PCs = ad.varm["PCs"]
    assert PCs.dtype == np.float64 and PCs.shape == (ad.X.shape[1], k)
    used = np.zeros(ad.X.shape[1], dtype=bool)
    used[cols if cols is not None else slice(None)] = True
    assert (PCs[~used] == 0.0).all()
    got = (ref[0], PCs[used] if cols is None else PCs[cols], ad.uns["pca"]["variance"], ad.uns["pca"]["variance_ratio"])
    _check(got, ref, "tl.pca")
    assert set(ad.uns["pca"]) == {"variance", "variance_ratio"}


@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_tl_pca_writes_what_scanpy_writes(kind, monkeypatch):
    ad, K = _adata(kind)
    k = SHAPES["slices"][2]
    if kind == "sparse":
        def boom(self, *a, **kw):
            raise AssertionError("the sparse matrix was made dense on the host")
        for cls in {type(ad.X), sp.csr_matrix}:
            monkeypatch.setattr(cls, "toarray", boom)
            monkeypatch.setattr(cls, "todense", boom)
        before = (ad.X.indptr.copy(), ad.X.indices.copy(), ad.X.data.copy())
    else:
        before = ad.X.copy()
    out = tl.pca(ad, n_comps=k)
    assert out is ad.obsm["X_pca"] and set(ad.obsm) == {"X_pca"} and set(ad.varm) == {"PCs"} and set(ad.uns) == {"pca"}
    _tl_check(ad, _reference("slices", "scaled"), k, None)
    # a gene selection, by name and by mask, under another key
    cols = np.sort(_subset("slices"))
    mask = np.zeros(K.shape[1], dtype=bool)
    mask[cols] = True
    tl.pca(ad, n_comps=k, genes=mask, key_added="X_sel")
    ref = PR.pca(K, k, cols=cols)
    assert _gap(ref[4], k) >= MIN_GAP
    _tl_check(ad, ref[:4], k, cols, "X_sel")
    by_mask = ad.obsm["X_sel"].copy()
    names = [ad.var_names[j] for j in _subset("slices")]           # scrambled: varm rows still land on their genes
    tl.pca(ad, n_comps=k, genes=names, key_added="X_sel")
    _tl_check(ad, PR.pca(K, k, cols=_subset("slices"))[:4], k, _subset("slices"), "X_sel")
    assert (np.abs(ad.obsm["X_sel"] - by_mask) <= 2 * (TOL_VEC + 2.0 ** -24) * np.abs(by_mask).max(axis=0)).all()
    if kind == "sparse":
        assert all(np.array_equal(a, b) for a, b in zip(before, (ad.X.indptr, ad.X.indices, ad.X.data)))
    else:
        assert np.array_equal(before, ad.X)


@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_tl_pca_normalizes_on_the_device_copy_only(kind):
    ad, K = _adata(kind)
    k = 6
    data_before = ad.X.data.copy() if kind == "sparse" else ad.X.copy()
    tl.pca(ad, n_comps=k, normalize=True, target_sum=1e4)
    S = engine.DeviceCSR.upload(_csr(K, np.float32)).normalize_log1p(1e4)
    Yn = engine.download(S.densify())
    assert Yn.dtype == np.float32 and Yn.max() > 1.0
    ref = PR.pca(Yn, k)
    gap = _gap(ref[4], k)
    print("normalised: min relative gap %.2e" % gap)
    assert gap >= MIN_GAP
    _tl_check(ad, ref[:4], k, None)
    assert np.array_equal(data_before, ad.X.data if kind == "sparse" else ad.X)


def test_extract_annot_expression():
    ad, K = _adata("sparse", shape="complete")
    columns = ["ct", "sample", "state", "X_emb"]
    ad.obsm["X_emb"] = np.arange(ad.X.shape[0] * 3, dtype=np.float32).reshape(-1, 3)
    data, annot = tl.extract_annot_expression(ad, columns=columns)
    assert list(data.columns) == ["PCA_1", "PCA_2", "PCA_3"] and np.array_equal(data.values, ad.obsm["X_emb"])
    assert list(annot.columns) == ["cell_types", "sampleID", "status"] and len(annot) == ad.X.shape[0]
    assert list(annot["cell_types"]) == list(ad.obs["ct"]) and list(annot["status"]) == list(ad.obs["state"])
    assert list(ad.obs.columns) == ["ct", "sample", "state"] and "X_pca" not in ad.obsm
    data, annot = tl.extract_annot_expression(ad, columns=columns, reduction=True, max_value=8, target_sum=5e3)
    k = 50                                                         # scanpy's default, below min(257, 70) - 1
    assert list(data.columns) == ["PCA_%d" % i for i in range(1, k + 1)] and data.shape == (ad.X.shape[0], k)
    assert list(annot.columns) == ["cell_types", "sampleID", "status"]
    other, _ = _adata("sparse", shape="complete")
    want = tl.pca(other, n_comps=k, normalize=True, target_sum=5e3, scale=True, max_value=8)
    assert np.array_equal(data.values, want) and np.array_equal(ad.obsm["X_pca"], want)
    assert np.array_equal(ad.varm["PCs"], other.varm["PCs"])
