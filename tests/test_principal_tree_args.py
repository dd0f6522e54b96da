"""The principal tree's argument checks (engine.elastic_fit / principal_tree / tree_pseudotime, tl.fit_principal_graph and the C
ABI under them) and the numpy restatement's own properties.  CPU only: every refusal here comes before any device work, which on
a machine without a device is what makes it a ValueError and not a PilotOTError."""
import ctypes

import numpy as np
import pytest

import principal_tree_clouds as C
import principal_tree_restatement as R
from pilot_amd import _lib, engine, tl

X = np.ascontiguousarray(C.cloud("y", 60, 2))
CENTRE = X.mean(axis=0)
Y0 = X[:4].copy()
S = C.path_springs(4)


def _abi_fit(X=X, dtype=1, n=None, D=None, ld=None, B=1, m=4, Y0=Y0, S=S, centre=CENTRE, max_iter=10, eps=0.01, null=None):
    """pilot_ot_elastic_fit_batch with one argument changed; returns (rc, message)"""
    L = _lib.load()
    n = X.shape[0] if n is None else n
    D = X.shape[1] if D is None else D
    out = dict(Y=np.empty((B if B > 0 else 1, m, D if 0 < D <= 64 else 1)), energy=np.empty((max(B, 1), 2)), iters=np.empty(max(B, 1), dtype=np.int32),
               flags=np.empty(max(B, 1), dtype=np.int32), counts=np.empty((max(B, 1), m), dtype=np.int32),
               sums=np.empty((max(B, 1), m, D if 0 < D <= 64 else 1)))
    args = dict(X=ctypes.c_void_p(X.ctypes.data), Y0=_lib.dptr(np.ascontiguousarray(Y0)), S=_lib.dptr(np.ascontiguousarray(S)),
                centre=_lib.dptr(np.ascontiguousarray(centre)), Y=_lib.dptr(out["Y"]), energy=_lib.dptr(out["energy"]),
                iters=_lib.iptr(out["iters"]), flags=_lib.iptr(out["flags"]), counts=_lib.iptr(out["counts"]), sums=_lib.dptr(out["sums"]))
    if null:
        args[null] = None
    rc = L.pilot_ot_elastic_fit_batch(args["X"], 0, dtype, n, D, D if ld is None else ld, B, m, args["Y0"], args["S"], args["centre"], max_iter,
                                      eps, args["Y"], args["energy"], args["iters"], args["flags"], args["counts"], args["sums"])
    return rc, L.pilot_ot_last_error().decode()


def _bad(a, where=0):
    a = np.array(a, dtype=np.float64)
    a.flat[where] = np.nan
    return a


@pytest.mark.parametrize("null", ["X", "Y0", "S", "centre", "Y", "energy", "iters", "flags", "counts", "sums"])
def test_abi_refuses_a_null_pointer(null):
    rc, msg = _abi_fit(null=null)
    assert rc == _lib.EINVAL and "NULL" in msg


@pytest.mark.parametrize("kw, word", [(dict(D=0), "D=0"), (dict(D=65), "D=65"), (dict(m=1), "m=1"), (dict(m=66), "m=66"), (dict(B=0), "B=0"),
                                      (dict(max_iter=0), "max_iter"), (dict(eps=-1e-3), "eps"), (dict(eps=float("nan")), "eps"),
                                      (dict(Y0=_bad(Y0, 3)), "start position"), (dict(S=_bad(S, 5)), "spring"),
                                      (dict(centre=_bad(CENTRE, 1)), "centre"), (dict(dtype=2), "dtype"), (dict(ld=1), "ld"), (dict(n=0), "n=0")])
def test_abi_einval_before_any_hip_call(kw, word):
    if kw.get("m", 4) != 4:
        m = kw["m"]
        kw = dict(kw, Y0=np.zeros((max(m, 1), 2)), S=np.zeros((max(m, 1), max(m, 1))))
    rc, msg = _abi_fit(**kw)
    assert rc == _lib.EINVAL and word in msg, (rc, msg)


def test_abi_moments_and_projection_checks():
    L = _lib.load()
    mean, cross = np.empty(2), np.empty((2, 2))
    xp = ctypes.c_void_p(X.ctypes.data)
    assert L.pilot_ot_point_moments(None, 0, 1, 60, 2, 2, _lib.dptr(mean), _lib.dptr(cross)) == _lib.EINVAL
    assert L.pilot_ot_point_moments(xp, 0, 1, 60, 2, 2, None, _lib.dptr(cross)) == _lib.EINVAL
    assert L.pilot_ot_point_moments(xp, 0, 1, 60, 65, 65, _lib.dptr(mean), _lib.dptr(cross)) == _lib.EINVAL
    assert L.pilot_ot_point_moments(xp, 0, 1, 1 << 31, 2, 2, _lib.dptr(mean), _lib.dptr(cross)) == _lib.ENOTSUP
    nodes, edges, base = Y0.copy(), np.array([[0, 1], [1, 2], [2, 3]], dtype=np.int32), np.zeros(4)
    pt, d2, e, t = np.empty(60), np.empty(60), np.empty(60, dtype=np.int32), np.empty(60)

    def proj(nodes=nodes, m=4, ne=3, edges=edges, base=base, pt=pt):
        return L.pilot_ot_tree_projection(xp, 0, 1, 60, 2, 2, m, _lib.dptr(nodes), ne, _lib.iptr(edges), _lib.dptr(base),
                                          None if pt is None else _lib.dptr(pt), _lib.dptr(d2), _lib.iptr(e), _lib.dptr(t))
    assert proj(pt=None) == _lib.EINVAL
    assert proj(m=66) == _lib.EINVAL and proj(m=1) == _lib.EINVAL
    assert proj(ne=0) == _lib.EINVAL and proj(ne=4) == _lib.EINVAL
    assert proj(edges=np.array([[0, 1], [1, 2], [2, 4]], dtype=np.int32)) == _lib.EINVAL and b"edge 2" in L.pilot_ot_last_error()
    assert proj(nodes=_bad(nodes)) == _lib.EINVAL and proj(base=_bad(base)) == _lib.EINVAL


def test_symbols_are_declared():
    for name in ("pilot_ot_elastic_fit_batch", "pilot_ot_point_moments", "pilot_ot_tree_projection"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)


@pytest.mark.parametrize("call", [
    lambda: engine.elastic_fit(X, Y0, S, CENTRE, max_iter=0),
    lambda: engine.elastic_fit(X, Y0, S, CENTRE, max_iter=2.5),
    lambda: engine.elastic_fit(X, Y0, S, CENTRE, eps=-1.0),
    lambda: engine.elastic_fit(X, _bad(Y0), S, CENTRE),
    lambda: engine.elastic_fit(X, Y0, _bad(S), CENTRE),
    lambda: engine.elastic_fit(X, Y0, S, _bad(CENTRE)),
    lambda: engine.elastic_fit(X, Y0[:, :1], S, CENTRE),
    lambda: engine.elastic_fit(X, Y0, S[:3, :3], CENTRE),
    lambda: engine.elastic_fit(X, Y0[:1], S[:1, :1], CENTRE),
    lambda: engine.elastic_fit(X, np.zeros((66, 2)), np.zeros((66, 66)), CENTRE),
    lambda: engine.elastic_fit(np.zeros((10, 65)), np.zeros((3, 65)), C.path_springs(3), np.zeros(65)),
    lambda: engine.elastic_fit(X[0], Y0, S, CENTRE),
    lambda: engine.principal_tree(X, n_nodes=2),
    lambda: engine.principal_tree(X, n_nodes=65),
    lambda: engine.principal_tree(X, n_nodes=8.0),
    lambda: engine.principal_tree(X, lam=-0.1),
    lambda: engine.principal_tree(X, mu=float("inf")),
    lambda: engine.principal_tree(X, max_iter=0),
    lambda: engine.principal_tree(X, eps=-1),
    lambda: engine.principal_tree(X[:1]),
    lambda: engine.principal_tree(np.zeros((10, 65))),
    lambda: engine.principal_tree(np.zeros((0, 2))),
    lambda: engine.tree_pseudotime(X, Y0, [(0, 1), (1, 2)]),
    lambda: engine.tree_pseudotime(X, Y0, [(0, 1), (1, 2), (0, 2)]),
    lambda: engine.tree_pseudotime(X, Y0, [(0, 1), (1, 2), (2, 4)]),
    lambda: engine.tree_pseudotime(X, Y0, [(0, 1), (1, 2), (2, 3)], source=4),
    lambda: engine.tree_pseudotime(X, Y0, [(0, 1), (1, 2), (2, 3)], source=-1),
    lambda: engine.tree_pseudotime(X, _bad(Y0), [(0, 1), (1, 2), (2, 3)]),
    lambda: engine.tree_pseudotime(X, np.zeros((4, 3)), [(0, 1), (1, 2), (2, 3)]),
])
def test_engine_refuses_before_any_device_work(call):
    with pytest.raises(ValueError):
        call()


def test_tl_alias_and_missing_embedding():
    assert tl.fit_pricipla_graph is tl.fit_principal_graph

    class A:
        uns = {}
    with pytest.raises(KeyError, match="embedding"):
        tl.fit_principal_graph(A())
    with pytest.raises(ValueError):
        tl.fit_principal_graph(A(), NumNodes=2, X=X)
    assert A.uns == {}


def test_springs_match_the_restatement():
    edges = [(0, 1), (1, 2), (1, 3), (3, 4)]
    assert np.array_equal(engine.tree_springs(5, edges, 0.01, 0.1), R.springs(5, edges, 0.01, 0.1))
    assert np.array_equal(engine.tree_springs(4, [(0, 1), (1, 2), (2, 3)]), C.path_springs(4))
    S5 = R.springs(5, edges)
    assert np.allclose(S5, S5.T) and np.abs(S5.sum(axis=1)).max() < 1e-17 and np.linalg.eigvalsh(S5).min() > -1e-17


def test_candidate_lists_match_the_restatement():
    rng = np.random.default_rng(0)
    Y, edges = rng.normal(size=(6, 3)), [(0, 1), (1, 2), (1, 3), (3, 4), (3, 5)]
    cnt, s = np.array([3, 0, 2, 0, 1, 4]), rng.normal(size=(6, 3))
    for mine, ref in ((engine._grow_candidates(Y, edges, cnt, s), R.grow(Y, edges, cnt, s)),
                      (engine._shrink_candidates(Y, edges), R.shrink(Y, edges))):
        assert len(mine) == len(ref)
        for (ya, ea, _), (yb, eb) in zip(mine, ref):
            assert np.array_equal(ya, yb) and [tuple(e) for e in ea] == [tuple(e) for e in eb]
            assert R.is_tree(len(ya), ea)


def test_orientation_matches_the_restatement():
    rng = np.random.default_rng(1)
    Y, edges = rng.normal(size=(6, 2)), [(0, 1), (2, 1), (1, 3), (4, 3), (3, 5)]
    for source in (0, 3, 5):
        e1, b1 = engine.tree_orientation(Y, edges, source)
        e2, b2 = R.orient(Y, edges, source)
        assert np.array_equal(e1, e2) and np.allclose(b1, b2, rtol=1e-15, atol=0)


@pytest.mark.parametrize("name, n, m, seed", C.FITS)
def test_restatement_energy_never_rises(name, n, m, seed):
    Xc, Yc, Sc, c = C.fit_case(name, n, m, seed, np.float64)
    f = R.fit(Xc, Yc, Sc, c)
    tr = np.array(f["trace"])
    assert len(tr) == f["iters"] + 1 and (np.diff(tr) <= 1e-14 * tr[:-1]).all(), tr


@pytest.mark.parametrize("name, n, M, seed", [c for c in C.TREES if c[1] <= 150])
def test_restatement_returns_a_tree(name, n, M, seed):
    Y, edges, info = R.tree(C.cloud(name, n, seed), M)
    assert Y.shape[0] == M and edges.shape == (M - 1, 2) and R.is_tree(M, edges)
    assert len(info["winners"]) == 3 * (M - 2) + 1
    with pytest.raises(ValueError, match="coincide"):
        R.start(np.ones((5, 2)))
