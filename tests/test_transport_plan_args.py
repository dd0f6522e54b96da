"""Argument checks of the transport-plan entry point (pilot_ot_transport_plans / engine.transport_plans): every rejection is
reported before the device is touched, so these run on a box without a GPU."""
import ctypes

import numpy as np
import pytest

from pilot_amd import _lib, engine

N, K = 5, 4


def _inputs():
    rng = np.random.default_rng(0)
    P = rng.random((N, K))
    P /= P.sum(1, keepdims=True)
    M = rng.random((K, K))
    np.fill_diagonal(M, 0.0)
    return P, M


def _call(P=None, M=None, Nv=N, Kv=K, regularized=0, reg=0.1, pi=(0,), pj=(1,), n_pairs=None, groups=None, n_groups=1,
          null=()):
    """pilot_ot_transport_plans through ctypes; `null` names the pointer arguments passed as NULL."""
    L = _lib.load()
    P0, M0 = _inputs()
    P = P0 if P is None else P
    M = M0 if M is None else M
    pi = np.asarray(pi, dtype=np.int32)
    pj = np.asarray(pj, dtype=np.int32)
    n = len(pi) if n_pairs is None else n_pairs
    g = None if groups is None else np.asarray(groups, dtype=np.int32)
    out = np.full(max(n, n_groups if g is not None else 0, 1) * max(Kv, 1) ** 2 if Kv <= 64 else 1, -7.0)
    vals = np.full(max(n, 1), -7.0)
    ptr = {"P": _lib.dptr(P), "M": _lib.dptr(M), "pair_i": _lib.iptr(pi), "pair_j": _lib.iptr(pj), "plans": _lib.dptr(out)}
    for k in null:
        ptr[k] = None
    rc = L.pilot_ot_transport_plans(ptr["P"], Nv, Kv, ptr["M"], regularized, reg, 1000, 1e-9, 1e3, 20, ptr["pair_i"],
                                    ptr["pair_j"], n, None if g is None else _lib.iptr(g), n_groups, ptr["plans"],
                                    _lib.dptr(vals), None, None)
    return rc, L.pilot_ot_last_error().decode(), out, vals


@pytest.mark.parametrize("name", ["P", "M", "pair_i", "pair_j", "plans"])
def test_null_pointer(name):
    rc, msg, _, _ = _call(null=(name,))
    assert rc == _lib.EINVAL and msg == "NULL pointer"


@pytest.mark.parametrize("Nv,Kv", [(0, K), (-1, K), (N, 0), (N, -3)])
def test_non_positive_shape(Nv, Kv):
    rc, msg, _, _ = _call(Nv=Nv, Kv=Kv)
    assert rc == _lib.EINVAL and msg == "N=%d K=%d must be positive" % (Nv, Kv)


@pytest.mark.parametrize("pi,pj", [((0, N), (1, 1)), ((0, 1), (-1, 1)), ((-2,), (0,)), ((3,), (N + 4,))])
def test_pair_out_of_range(pi, pj):
    rc, msg, _, _ = _call(pi=pi, pj=pj)
    t = next(k for k in range(len(pi)) if not (0 <= pi[k] < N and 0 <= pj[k] < N))
    assert rc == _lib.EINVAL and msg == "pair %d = (%d, %d) out of range for N=%d" % (t, pi[t], pj[t], N)


@pytest.mark.parametrize("groups,n_groups", [((0, 2), 2), ((-1, 0), 1), ((0, 5), 3)])
def test_group_out_of_range(groups, n_groups):
    rc, msg, _, _ = _call(pi=(0, 1), pj=(1, 2), groups=groups, n_groups=n_groups)
    t = next(k for k in range(len(groups)) if not (0 <= groups[k] < n_groups))
    assert rc == _lib.EINVAL and msg == "group %d of pair %d out of range for n_groups=%d" % (groups[t], t, n_groups)


def test_no_groups_with_a_group_list():
    rc, msg, _, _ = _call(groups=(0,), n_groups=0)
    assert rc == _lib.EINVAL and msg == "n_groups=0 must be positive"


@pytest.mark.parametrize("reg", [0.0, -0.5, float("inf"), float("nan")])
def test_bad_reg_in_entropic_mode(reg):
    rc, msg, _, _ = _call(regularized=1, reg=reg)
    assert rc == _lib.EINVAL and msg == "reg=%g must be positive and finite" % reg


def test_unknown_mode():
    rc, msg, _, _ = _call(regularized=2)
    assert rc == _lib.EINVAL and msg == "regularized=2 must be 0 (exact) or 1 (entropic)"


@pytest.mark.parametrize("Kv", [2049, 4096])
def test_too_many_cell_types(Kv):
    P = np.full((N, Kv), 1.0 / Kv)
    M = np.zeros((1, 1))                     # (never read: the shape check comes first)
    rc, msg, _, _ = _call(P=P, M=M, Kv=Kv)
    assert rc == _lib.ENOTSUP and msg == "transport plans: K=%d > 2048 cell types" % Kv and "K=%d" % Kv in msg


def test_no_pairs_writes_nothing():
    rc, _, out, vals = _call(pi=(), pj=(), n_pairs=0)
    assert rc == _lib.OK
    assert (out == -7.0).all() and (vals == -7.0).all()


# ---- the same rejections through engine.transport_plans (EINVAL -> ValueError, ENOTSUP -> NotImplementedError) ----
def test_engine_rejections():
    P, M = _inputs()
    with pytest.raises(ValueError, match=r"pilot_ot: pair 1 = \(0, 5\) out of range for N=5"):
        engine.transport_plans(P, M, [[0, 1], [0, 5]])
    with pytest.raises(ValueError, match=r"pilot_ot: pair 0 = \(-1, 2\) out of range for N=5"):
        engine.transport_plans(P, M, [[-1, 2]])
    with pytest.raises(ValueError, match=r"pilot_ot: group -1 of pair 1 out of range for n_groups=1"):
        engine.transport_plans(P, M, [[0, 1], [1, 2]], groups=[0, -1])
    for reg in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="pilot_ot: reg=%s must be positive and finite" % ("%g" % reg)):
            engine.transport_plans(P, M, [[0, 1]], regularized="reg", reg=reg)
    with pytest.raises(NotImplementedError, match="pilot_ot: transport plans: K=2100 > 2048 cell types"):
        engine.transport_plans(np.full((2, 2100), 1 / 2100), np.zeros((2100, 2100)), [[0, 1]])
    with pytest.raises(ValueError, match="pairs must be an"):
        engine.transport_plans(P, M, [[0, 1, 2]])
    with pytest.raises(ValueError, match="groups must be"):
        engine.transport_plans(P, M, [[0, 1]], groups=[0, 1])
    assert engine.transport_plans(P, M, np.zeros((0, 2), dtype=np.int64)).shape == (0, K, K)
    G, info = engine.transport_plans(P, M, np.zeros((0, 2), dtype=np.int64), groups=np.zeros(0, dtype=np.int64), return_info=True)
    assert G.shape == (0, K, K) and info["values"].shape == (0,)


def test_symbol_is_listed():
    assert "pilot_ot_transport_plans" in _lib.SYMBOLS and hasattr(_lib.load(), "pilot_ot_transport_plans")
