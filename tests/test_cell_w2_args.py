"""Argument checks of the cell-level W2 entry points that return before any HIP call (CPU only: no device needed).
pilot_ot_cell_cohort_create: NULL pointers, N / D out of range, an empty patient, a patient over the LDS limit
(3 max_n + 48 floats <= 160 KiB: max_n <= 13 637).  pilot_ot_cell_w2_grid_multi: the checks before hipGetDeviceCount."""
import ctypes

import numpy as np

from pilot_amd import _lib

MAX_CELLS = 13637            # (160 * 1024 / 4 - 48) / 3


def _create(X, offs, N, D):
    L = _lib.load()
    h = ctypes.c_void_p()
    xp = None if X is None else ctypes.c_void_p(X.ctypes.data)
    op = None if offs is None else ctypes.c_void_p(offs.ctypes.data)
    rc = L.pilot_ot_cell_cohort_create(xp, op, N, D, ctypes.byref(h))
    if h.value:
        L.pilot_ot_cell_cohort_destroy(h)
    return rc, L.pilot_ot_last_error().decode()


def test_cell_cohort_create_rejects_bad_arguments():
    X = np.zeros((8, 65), dtype=np.float32)
    offs = np.array([0, 3, 8], dtype=np.int64)
    L = _lib.load()
    assert L.pilot_ot_cell_cohort_create(None, ctypes.c_void_p(offs.ctypes.data), 2, 4, ctypes.byref(ctypes.c_void_p())) == _lib.EINVAL
    assert _create(X, None, 2, 4)[0] == _lib.EINVAL
    assert L.pilot_ot_cell_cohort_create(ctypes.c_void_p(X.ctypes.data), ctypes.c_void_p(offs.ctypes.data), 2, 4, None) == _lib.EINVAL
    for N, D in ((0, 4), (-1, 4), (2, 0), (2, -3)):
        rc, msg = _create(X, offs, N, D)
        assert rc == _lib.EINVAL and "must be positive" in msg, (N, D, msg)
    rc, msg = _create(X, offs, 2, 65)
    assert rc == _lib.ENOTSUP and "D=65" in msg
    for bad in ([0, 3, 3, 8], [0, 0, 8], [0, 5, 3, 8]):          # an empty patient (last, first) and a negative size
        o = np.array(bad, dtype=np.int64)
        rc, msg = _create(X, o, len(bad) - 1, 4)
        assert rc == _lib.EINVAL and "cells" in msg, (bad, msg)


def test_cell_cohort_create_lds_limit():
    D = 2
    X = np.zeros((MAX_CELLS + 1 + 5, D), dtype=np.float32)
    over = np.array([0, 5, 5 + MAX_CELLS + 1], dtype=np.int64)
    rc, msg = _create(X, over, 2, D)
    assert rc == _lib.ENOTSUP and "%d cells" % (MAX_CELLS + 1) in msg and "LDS" in msg
    # the largest patient that fits passes the check: on a box without a device the call fails only at the first HIP call
    at = np.array([0, 5, 5 + MAX_CELLS], dtype=np.int64)
    rc, msg = _create(X, at, 2, D)
    assert rc in (_lib.OK, _lib.EHIP), msg
    if rc == _lib.EHIP:
        assert "LDS" not in msg


def test_cell_w2_grid_multi_checks_before_the_device():
    L = _lib.load()
    X = np.zeros((8, 4), dtype=np.float32)
    offs = np.array([0, 3, 8], dtype=np.int64)
    w2 = np.zeros((2, 2))
    it = np.zeros((2, 2), dtype=np.int32)
    err = np.zeros((2, 2))
    dev = np.zeros(65, dtype=np.int32)

    def call(Xp, op, N, devp, n_dev, w2p):
        return L.pilot_ot_cell_w2_grid_multi(Xp, op, N, 4, 1.0, 0.1, 1000, 1e-9, 10, 0.0, devp, n_dev, w2p,
                                             _lib.iptr(it), _lib.dptr(err))
    xp, op = ctypes.c_void_p(X.ctypes.data), ctypes.c_void_p(offs.ctypes.data)
    assert call(None, op, 2, _lib.iptr(dev), 1, _lib.dptr(w2)) == _lib.EINVAL
    assert call(xp, None, 2, _lib.iptr(dev), 1, _lib.dptr(w2)) == _lib.EINVAL
    assert call(xp, op, 2, None, 1, _lib.dptr(w2)) == _lib.EINVAL
    assert call(xp, op, 2, _lib.iptr(dev), 1, None) == _lib.EINVAL
    for n_dev in (0, -1, 65):
        assert call(xp, op, 2, _lib.iptr(dev), n_dev, _lib.dptr(w2)) == _lib.EINVAL
        assert "n_devices=%d" % n_dev in L.pilot_ot_last_error().decode()
    for N in (0, -2):
        assert call(xp, op, N, _lib.iptr(dev), 1, _lib.dptr(w2)) == _lib.EINVAL
        assert "N=%d" % N in L.pilot_ot_last_error().decode()


def test_c_oracle_follows_the_numpy_oracle():
    """The GPU parity tests use oracle.cell_w2_c (C / OpenMP) for speed: it takes the numpy oracle's updates, also with a
    far-out cell, a capped count, another check period and a stop threshold it reaches."""
    from oracle import oracle as O
    rng = np.random.default_rng(2)
    X, Y = rng.standard_normal((23, 7)), rng.standard_normal((31, 7)) + 0.4
    Xf = X.copy()
    Xf[0, 3] += 300.0
    for A, kw in ((X, {}), (Xf, {}), (X, dict(numItermax=2)), (X, dict(check_period=7, stopThr=1e-6)), (Xf, dict(stopThr=1e-5))):
        for reg in (0.5, 0.05):
            v, i = O.cell_w2(A, Y, 3.0, reg, return_info=True, **kw)
            vc, ic = O.cell_w2_c(A, Y, 3.0, reg, n_threads=3, return_info=True, **kw)
            assert ic["iters"] == i["iters"]
            assert abs(vc - v) <= 1e-12 * max(1.0, abs(v)) and abs(ic["err"] - i["err"]) <= 1e-12 + 1e-9 * i["err"]
