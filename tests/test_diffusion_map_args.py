"""Diffusion map (K8): argument checks of the C ABI and of the Python faces, the restatement's own consistency.  CPU only:
every call here is refused before the device is touched."""
import ctypes

import numpy as np
import pytest

from pilot_amd import _lib, engine, tl


def _dev_rc(N, epsilon=1.0, alpha=0.5, n_evecs=2, null=None):
    """pilot_ot_diffusion_map_dev with placeholder pointers (never dereferenced: the call is refused first)."""
    L = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    info = np.zeros(2, dtype=np.int32)
    ptrs = dict(K=fake, dmap=fake, evecs=fake, evals=fake, info=_lib.iptr(info))
    if null:
        ptrs[null] = None
    return L.pilot_ot_diffusion_map_dev(ptrs["K"], N, epsilon, alpha, n_evecs, ptrs["dmap"], ptrs["evecs"], ptrs["evals"],
                                        ptrs["info"], None)


def _rows_rc(N, k=64, epsilon=1.0, alpha=0.5, n_evecs=2, null=None):
    L = _lib.load()
    n = max(N, 1)
    E = np.ones((n, n))
    out = np.zeros(n * 64 + 64)
    info = np.zeros(2, dtype=np.int32)
    ptrs = dict(E=ctypes.c_void_p(E.ctypes.data), dmap=_lib.dptr(out), evals=_lib.dptr(out), info=_lib.iptr(info))
    if null:
        ptrs[null] = None
    return L.pilot_ot_diffusion_map_of_rows(ptrs["E"], 0, N, k, epsilon, alpha, n_evecs, ptrs["dmap"], None, ptrs["evals"],
                                            ptrs["info"])


BAD = [
    dict(N=1, n_evecs=1),                       # N < 2
    dict(N=0, n_evecs=1),
    dict(N=10, n_evecs=0),                      # n_evecs < 1
    dict(N=10, n_evecs=10),                     # n_evecs > N - 1
    dict(N=200, n_evecs=65),                    # n_evecs > 64
    dict(N=10, epsilon=0.0),                    # epsilon <= 0
    dict(N=10, epsilon=-1.0),
    dict(N=10, epsilon=float("nan")),           # epsilon not finite
    dict(N=10, epsilon=float("inf")),
    dict(N=10, alpha=float("nan")),             # alpha not finite
    dict(N=10, alpha=float("-inf")),
]


@pytest.mark.parametrize("kw", BAD)
def test_c_abi_refuses_out_of_range_arguments(kw):
    assert _dev_rc(**kw) == _lib.EINVAL
    assert _rows_rc(**kw) == _lib.EINVAL
    assert _lib.load().pilot_ot_last_error()


@pytest.mark.parametrize("null", ["K", "dmap", "evals", "info"])
def test_dev_entry_refuses_null_pointers(null):
    assert _dev_rc(10, null=null) == _lib.EINVAL


@pytest.mark.parametrize("null", ["E", "dmap", "evals", "info"])
def test_rows_entry_refuses_null_pointers(null):
    assert _rows_rc(10, null=null) == _lib.EINVAL


@pytest.mark.parametrize("k", [0, -3])
def test_rows_entry_refuses_k_below_one(k):
    assert _rows_rc(10, k=k) == _lib.EINVAL and b"k=" in _lib.load().pilot_ot_last_error()


ENGINE_BAD = [
    dict(N=1, n_evecs=1), dict(N=10, n_evecs=0), dict(N=10, n_evecs=10), dict(N=200, n_evecs=65), dict(N=10, epsilon=0.0),
    dict(N=10, epsilon=-2.0), dict(N=10, epsilon=float("nan")), dict(N=10, epsilon=float("inf")), dict(N=10, alpha=float("nan")),
]


@pytest.mark.parametrize("kw", ENGINE_BAD)
def test_engine_refuses_out_of_range_arguments(kw):
    kw = dict(kw)
    N = kw.pop("N")
    E = np.ones((N, N))
    with pytest.raises(ValueError):
        engine.diffusion_map_of_rows(E, **kw)
    with pytest.raises(ValueError):
        engine.diffusion_map_from_kernel(E, **kw)


def test_engine_refuses_k_below_one():
    with pytest.raises(ValueError):
        engine.diffusion_map_of_rows(np.ones((10, 10)), k=0)


@pytest.mark.parametrize("eps", ["bgh", "bgh_generous", b"bgh", None, [1.0]])
def test_bandwidth_selection_is_not_implemented(eps):
    with pytest.raises(NotImplementedError):
        engine.diffusion_map_of_rows(np.ones((10, 10)), epsilon=eps)
    with pytest.raises(NotImplementedError):
        engine.diffusion_map_from_kernel(np.ones((10, 10)), epsilon=eps)
    ad = type("A", (), {})()
    ad.uns = {"EMD": np.ones((10, 10))}
    with pytest.raises(NotImplementedError):
        tl.diffusion_map(ad, epsilon=eps)
    assert set(ad.uns) == {"EMD"}


def test_tl_diffusion_map_needs_the_emd():
    ad = type("A", (), {})()
    ad.uns = {}
    with pytest.raises(KeyError):
        tl.diffusion_map(ad)


def test_header_declares_the_flags():
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "pilot_ot.h")).read()
    assert "#define PILOT_OT_DIFFMAP_NOT_CONVERGED %d" % _lib.DIFFMAP_NOT_CONVERGED in text
    assert "#define PILOT_OT_DIFFMAP_DEGENERATE %d" % _lib.DIFFMAP_DEGENERATE in text


def test_restatement_is_pydiffmap_s_similarity_identity():
    """The device form rests on P being similar to S = D^-1/2 A D^-1/2: the restatement's eigs(L) against eigh(S) on a small
    random point cloud (the identity of DESIGN.md K8)."""
    import diffmap_restatement as R
    rng = np.random.default_rng(0)
    X = rng.random((120, 5))
    K = R.knn_kernel(X, 16, 0.5)
    dmap, evecs, evals = R.diffusion_map_from_kernel(K, 0.5, 0.5, 3)
    mu = R.mu_spectrum(K, 0.5)
    np.testing.assert_allclose(evals, (mu[1:4] - 1.0) / 0.5, rtol=0, atol=1e-12)
    P, _ = R.markov_operator(K, 0.5)
    res = np.abs(P @ evecs - evecs * (evals * 0.5 + 1.0)).max()
    assert res <= 1e-12
    np.testing.assert_allclose(np.linalg.norm(evecs, axis=0), 1.0, atol=1e-12)
    np.testing.assert_allclose(dmap, evecs * np.sqrt(-1.0 / evals), rtol=0, atol=1e-15)
