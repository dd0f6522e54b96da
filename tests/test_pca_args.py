"""Principal components (K15), the parts that need no device.  The C ABI refuses every argument it can judge before any HIP call (a
box without a device returns PILOT_OT_EHIP from the first HIP call, so PILOT_OT_EINVAL shows the check came first), and engine.pca /
DeviceCSR.pca / tl.pca / tl.extract_annot_expression raise before the library is touched (the library handle is replaced by an
object that fails the test on any use).  The restatement is checked against an eigen-decomposition of the covariance matrix."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import pca_restatement as PR
from pilot_amd import _lib, engine, tl


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def _dense_rc(n=10, n_cols_total=6, ld=None, dtype=1, cols=None, n_sel=None, scale=1, max_value=10.0, n_comps=2, null=None):
    L = _lib.load()
    Y = np.ones((max(n, 1), max(n_cols_total, 1)))
    out = np.zeros(max(n, 1) * 64 + 64 * 64)
    info = np.zeros(2, dtype=np.int32)
    cols = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32)
    n_sel = (n_cols_total if cols is None else cols.size) if n_sel is None else n_sel
    p = dict(Y=ctypes.c_void_p(Y.ctypes.data), scores=_lib.dptr(out), pcs=_lib.dptr(out), variance=_lib.dptr(out), ratio=_lib.dptr(out),
             info=_lib.iptr(info))
    if null:
        p[null] = None
    rc = L.pilot_ot_pca(p["Y"], 0, dtype, n, n_cols_total, n_cols_total if ld is None else ld, None if cols is None else _lib.iptr(cols),
                        n_sel, scale, max_value, n_comps, p["scores"], p["pcs"], p["variance"], p["ratio"], p["info"])
    return rc, L.pilot_ot_last_error()


@pytest.mark.parametrize("bad,fragment", [
    (dict(n=1, n_comps=1), b"at least 2 rows"),
    (dict(n=0, n_comps=1), b"at least 2 rows"),
    (dict(n_comps=0), b"n_comps"),
    (dict(n_comps=6), b"n_comps"),                                 # columns - 1 = 5
    (dict(n=4, n_comps=4), b"n_comps"),                            # n - 1 = 3
    (dict(n=200, n_cols_total=100, n_comps=65), b"n_comps"),       # the cap of 64
    (dict(cols=[0, 1, 2], n_comps=3), b"n_comps"),                 # the selection counts, not the matrix
    (dict(cols=[0, 6]), b"outside [0, 6)"),
    (dict(cols=[-1, 2, 3]), b"outside [0, 6)"),
    (dict(cols=[4, 2, 4]), b"repeats"),
    (dict(n_sel=3), b"n_sel"),                                     # without cols: all of them
    (dict(scale=2), b"scale"),
    (dict(max_value=0.0), b"max_value"),
    (dict(max_value=-1.0), b"max_value"),
    (dict(max_value=float("nan")), b"max_value"),
    (dict(scale=0, max_value=-1.0), b"max_value"),
    (dict(dtype=2), b"dtype"),
    (dict(ld=5), b"ld"),
    (dict(n_cols_total=0, n_sel=0), b"n_cols_total"),
    (dict(null="Y"), b"NULL"), (dict(null="scores"), b"NULL"), (dict(null="pcs"), b"NULL"), (dict(null="variance"), b"NULL"),
    (dict(null="ratio"), b"NULL"), (dict(null="info"), b"NULL"),
])
def test_c_abi_refuses_before_any_hip_call(bad, fragment):
    rc, msg = _dense_rc(**bad)
    assert rc == _lib.EINVAL and fragment in msg, (bad, msg)


def test_good_arguments_get_as_far_as_the_device():
    for kw in (dict(), dict(max_value=float("inf")), dict(cols=[5, 0, 3], n_comps=2), dict(scale=0)):
        rc, msg = _dense_rc(**kw)
        assert rc == (_lib.OK if _lib.device_count() > 0 else _lib.EHIP), (kw, msg)


def test_sparse_entry_point_refuses_a_null_handle_and_is_declared():
    L = _lib.load()
    out, info = np.zeros(64), np.zeros(2, dtype=np.int32)
    rc = L.pilot_ot_csr_pca(None, None, 4, 1, 10.0, 2, _lib.dptr(out), _lib.dptr(out), _lib.dptr(out), _lib.dptr(out), _lib.iptr(info))
    assert rc == _lib.EINVAL and b"NULL" in L.pilot_ot_last_error()
    assert "pilot_ot_csr_pca" in _lib.SYMBOLS and "pilot_ot_pca" in _lib.SYMBOLS
    assert (_lib.PCA_NOT_CONVERGED, _lib.PCA_RANK_DEFICIENT) == (1, 2)


# ---- engine ---------------------------------------------------------------------------------------------------------------------
Y = np.arange(60, dtype=np.float64).reshape(10, 6) % 7


@pytest.fixture
def shell(no_library):
    """a DeviceCSR of 10 x 6 around a handle that must never be used"""
    S = engine.DeviceCSR(ctypes.c_void_p(0x1000), (10, 6), np.float32, 7)
    yield S
    S.h = None


BAD_KW = [
    dict(n_comps=0), dict(n_comps=6), dict(n_comps=-1), dict(n_comps=2.5), dict(n_comps=True), dict(n_comps=float("nan")),
    dict(n_comps=3, cols=[0, 1, 2]),                               # columns - 1 = 2
    dict(cols=[0, 6]), dict(cols=[-1, 2, 3]), dict(cols=[[0, 1, 2]]), dict(cols=[0.0, 1.0, 2.0]), dict(cols=[1, 2, 1]),
    dict(max_value=0), dict(max_value=-3.0), dict(max_value=float("nan")), dict(max_value="10"), dict(max_value=[10.0]),
    dict(scale=False, max_value=-1.0),
]


@pytest.mark.parametrize("kw", BAD_KW)
def test_engine_pca_argument_errors(no_library, shell, kw):
    args = dict(n_comps=2)
    args.update(kw)
    for arg in (Y, Y.astype(np.float32), engine.DeviceMatrix(0x1000, 10, shape=(10, 6)), shell):
        with pytest.raises(ValueError):
            engine.pca(arg, **args)
    with pytest.raises(ValueError):
        shell.pca(**args)


def test_engine_pca_shapes_and_values(no_library, shell):
    for arg in (np.ones((1, 6)), engine.DeviceMatrix(0x1000, 1, shape=(1, 6)), engine.DeviceCSR(ctypes.c_void_p(0x1000), (1, 6), np.float32, 0)):
        with pytest.raises(ValueError, match="at least 2 rows"):
            engine.pca(arg, n_comps=1)
        if isinstance(arg, engine.DeviceCSR):
            arg.h = None
    with pytest.raises(ValueError, match="n_comps"):               # 200 x 100: the cap of 64
        engine.pca(np.ones((200, 100)), n_comps=65)
    for bad in (np.nan, np.inf, -np.inf):
        Z = Y.copy()
        Z[3, 4] = bad
        with pytest.raises(ValueError, match="non-finite"):
            engine.pca(Z, n_comps=2)
        with pytest.raises(ValueError, match="non-finite"):
            engine.pca(Z, n_comps=2, cols=[4, 1, 0])
        with pytest.raises(AssertionError, match="touched"):       # the bad column is not selected: every check passes
            engine.pca(Z, n_comps=2, cols=[5, 1, 0])
    for arg in (Y.astype(np.int64), Y[:, ::2], Y.ravel(), [[1.0, 2.0], [3.0, 4.0], [5.0, 7.0]], None, sp.csr_matrix(Y)):
        with pytest.raises(ValueError):
            engine.pca(arg, n_comps=1)
    for good in (dict(), dict(max_value=None), dict(scale=False), dict(cols=[5, 0, 3])):
        with pytest.raises(AssertionError, match="touched"):       # every check passed: the call is the first use of the library
            engine.pca(Y, n_comps=2, **good)
        with pytest.raises(AssertionError, match="touched"):
            shell.pca(n_comps=2, **good)


# ---- tl -------------------------------------------------------------------------------------------------------------------------
class _Adata:
    def __init__(self, X):
        self.X = X
        self.var_names = ["g%d" % j for j in range(X.shape[1])]
        self.obs = pd.DataFrame({"a": ["x"] * X.shape[0], "b": ["y"] * X.shape[0], "c": ["z"] * X.shape[0]})
        self.obsm, self.varm, self.uns = {"X_pca": np.ones((X.shape[0], 2), dtype=np.float32)}, {}, {}


@pytest.mark.parametrize("sparse", [False, True])
def test_tl_pca_checks_first(no_library, sparse):
    ad = _Adata(sp.csr_matrix(Y) if sparse else Y.copy())
    for kw in (dict(n_comps=0), dict(n_comps=2.5), dict(max_value=0), dict(max_value=-1), dict(target_sum=0), dict(target_sum=float("inf")),
               dict(genes=["g1", "nope", "g2"]), dict(genes=np.ones(5, dtype=bool)), dict(genes=[["g1", "g2"]]),
               dict(genes=["g1", "g2", "g1"]), dict(genes=["g1"])):
        with pytest.raises(ValueError):
            tl.pca(ad, **{**dict(n_comps=2), **kw})
    with pytest.raises(ValueError, match="n_comps"):               # beyond the cap of 64 nothing is lowered
        tl.pca(_Adata(np.ones((100, 80))), n_comps=70)
    bad = Y.copy()
    bad[2, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        tl.pca(_Adata(sp.csr_matrix(bad) if sparse else bad), n_comps=2)
    assert set(ad.obsm) == {"X_pca"} and not ad.varm and not ad.uns
    # n_comps at or above min(cells, genes) is lowered to one below it, as scanpy does: the call then reaches the library
    with pytest.raises(AssertionError, match="touched"):
        tl.pca(ad)


def test_extract_annot_expression_without_a_device(no_library):
    ad = _Adata(Y.copy())
    with pytest.raises(NotImplementedError, match="reclustering"):
        tl.extract_annot_expression(ad, columns=["a", "b", "c", "X_pca"], reclustering=True, reduction=True)
    with pytest.raises(NotImplementedError):
        tl.extract_annot_expression(ad, columns=["a", "b", "c", "X_pca"], reclustering=True)
    data, annot = tl.extract_annot_expression(ad, columns=["a", "b", "c", "X_pca"])
    assert list(data.columns) == ["PCA_1", "PCA_2"] and data.shape == (10, 2)
    assert list(annot.columns) == ["cell_types", "sampleID", "status"] and list(annot["sampleID"]) == ["y"] * 10
    assert list(ad.obs.columns) == ["a", "b", "c"]
    with pytest.raises(ValueError, match="max_value"):
        tl.extract_annot_expression(ad, columns=["a", "b", "c", "X_pca"], reduction=True, max_value=0)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_agrees_with_the_covariance_eigenproblem():
    rng = np.random.default_rng(0)
    K = rng.poisson(rng.gamma(0.5, 2.0, (40, 9))).astype(np.float64)
    K[:, 2] = 0.0                                                  # sigma -> 1
    K[:, 4] = 0.0
    K[6, 4] = 3.0                                                  # z = 39 / sqrt(40) = 6.2 > 5: clipped
    Z = PR.standardise(K, True, 5.0)
    assert Z.max() == 5.0 and Z[6, 4] == 5.0 and (Z[:, 2] == 0.0).all() and PR.clipped(K, 5.0) == 1
    low = PR.standardise(K, True, 0.5)
    assert low.max() == 0.5 and low.min() < -0.5                   # the lower side is not clipped
    sd = K.std(axis=0, ddof=1)
    assert np.allclose(PR.standardise(K, True, None)[:, 0], (K[:, 0] - K[:, 0].mean()) / sd[0], rtol=0, atol=1e-14)
    scores, pcs, var, ratio, all_var = PR.pca(K, 3, True, 5.0)
    lam, vec = np.linalg.eigh(np.cov(Z, rowvar=False))
    assert np.allclose(var, lam[::-1][:3], rtol=1e-12) and np.allclose(ratio, var / np.trace(np.cov(Z, rowvar=False)), rtol=1e-12)
    assert np.allclose(np.abs(pcs.T @ vec[:, ::-1][:, :3]), np.eye(3), atol=1e-10)
    assert np.allclose(scores, (Z - Z.mean(0)) @ pcs, atol=1e-12) and np.allclose(scores.var(axis=0, ddof=1), var, rtol=1e-12)
    at = np.abs(scores).argmax(axis=0)
    assert (scores[at, np.arange(3)] > 0).all()
    raw = PR.pca(K, 2, False)
    assert np.allclose(raw[2], np.linalg.eigvalsh(np.cov(K, rowvar=False))[::-1][:2], rtol=1e-12)
    sub = PR.pca(K, 2, True, 5.0, cols=[7, 0, 5])
    assert sub[1].shape == (3, 2) and np.allclose(sub[0], PR.pca(K[:, [7, 0, 5]], 2, True, 5.0)[0])
