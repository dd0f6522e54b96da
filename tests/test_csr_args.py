"""Sparse matrices on the device (K13), the parts that need no device.  pilot_ot_csr_upload refuses every malformed CSR before any
HIP call (a box without a device returns PILOT_OT_EHIP from the first HIP call, so PILOT_OT_EINVAL shows the check came first), the
other entry points refuse the arguments they can judge without a matrix, and engine.DeviceCSR raises ValueError before the library
is touched (the library handle is replaced by an object that fails the test on any use).  The checks that need a live handle -- a
code reaching n_groups, a column out of range, through ctypes -- are in tests/test_gpu_csr.py."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from pilot_amd import _lib, engine

LLP = ctypes.POINTER(ctypes.c_longlong)


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())


def _upload(indptr, indices, data, dtype=1, n_rows=None, n_cols=4, handle=True):
    L = _lib.load()
    indptr = None if indptr is None else np.ascontiguousarray(indptr, dtype=np.int64)
    indices = None if indices is None else np.ascontiguousarray(indices, dtype=np.int32)
    data = None if data is None else np.ascontiguousarray(data, dtype=np.float64)
    h = ctypes.c_void_p()
    rc = L.pilot_ot_csr_upload(None if indptr is None else indptr.ctypes.data_as(LLP), None if indices is None else _lib.iptr(indices),
                               None if data is None else ctypes.c_void_p(data.ctypes.data), dtype,
                               (indptr.size - 1 if indptr is not None else 2) if n_rows is None else n_rows, n_cols,
                               ctypes.byref(h) if handle else None)
    msg = L.pilot_ot_last_error()
    if rc == _lib.OK:                                              # (a device is present and the matrix was fine)
        L.pilot_ot_csr_destroy(h)
    return rc, msg


GOOD = dict(indptr=[0, 2, 3], indices=[3, 0, 1], data=[1.0, 2.0, 3.0])


@pytest.mark.parametrize("bad,fragment", [
    (dict(indptr=None), b"NULL"),
    (dict(handle=False), b"NULL"),
    (dict(indices=None), b"NULL"),
    (dict(data=None), b"NULL"),
    (dict(dtype=2), b"dtype"),
    (dict(n_rows=-1), b"n_rows"),
    (dict(n_cols=0), b"n_cols"),
    (dict(indptr=[1, 2, 3]), b"indptr[0]"),
    (dict(indptr=[0, 3, 2]), b"non-decreasing"),
    (dict(indices=[3, 0, 4]), b"outside [0, 4)"),
    (dict(indices=[3, 0, -1]), b"outside [0, 4)"),
    (dict(indices=[3, 3, 1]), b"duplicate"),
])
def test_upload_refuses_before_any_hip_call(bad, fragment):
    args = dict(GOOD)
    args.update(bad)
    rc, msg = _upload(**args)
    assert rc == _lib.EINVAL and fragment in msg, (bad, msg)


def test_a_good_matrix_gets_as_far_as_the_device():
    rc, msg = _upload(**GOOD)
    assert rc == (_lib.OK if _lib.device_count() > 0 else _lib.EHIP), msg
    rc, msg = _upload(indptr=[0, 0, 0], indices=None, data=None)    # no stored values: the two arrays may be NULL
    assert rc == (_lib.OK if _lib.device_count() > 0 else _lib.EHIP), msg


def test_the_other_entry_points_refuse_what_they_can_judge_without_a_matrix():
    L = _lib.load()
    count, mean, m2 = np.zeros(8, dtype=np.int64), np.zeros(8), np.zeros(8)
    codes = np.zeros(4, dtype=np.int32)
    for ts in (0.0, -1.0, float("nan"), float("inf")):
        assert L.pilot_ot_csr_normalize_log1p(None, ts) == _lib.EINVAL and b"target_sum" in L.pilot_ot_last_error()
    assert L.pilot_ot_csr_normalize_log1p(None, 1e4) == _lib.EINVAL and b"NULL" in L.pilot_ot_last_error()

    def moments(ng=2, transform=0):
        return L.pilot_ot_csr_group_moments(None, _lib.iptr(codes), ng, None, 1, transform, count.ctypes.data_as(LLP), _lib.dptr(mean),
                                            _lib.dptr(m2))
    for ng in (0, 9, -1):
        assert moments(ng=ng) == _lib.EINVAL and b"n_groups" in L.pilot_ot_last_error()
    assert moments(transform=2) == _lib.EINVAL and b"transform" in L.pilot_ot_last_error()
    assert moments() == _lib.EINVAL and b"NULL" in L.pilot_ot_last_error()
    assert L.pilot_ot_csr_column_nnz(None, count.ctypes.data_as(LLP)) == _lib.EINVAL and b"NULL" in L.pilot_ot_last_error()
    assert L.pilot_ot_csr_densify(None, None, 1, None) == _lib.EINVAL and b"NULL" in L.pilot_ot_last_error()
    assert L.pilot_ot_csr_build_columns(None) == _lib.EINVAL and b"NULL" in L.pilot_ot_last_error()
    assert L.pilot_ot_csr_destroy(None) == _lib.OK
    assert L.pilot_ot_csr_slice_rows() == engine.csr_slice_rows() >= 64
    for name in ("upload", "destroy", "normalize_log1p", "column_nnz", "group_moments", "densify"):
        assert "pilot_ot_csr_" + name in _lib.SYMBOLS


# ---- engine ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", [
    np.zeros((3, 4)),                                              # dense
    [[0.0, 1.0]],
    sp.csc_matrix(np.eye(3)),                                      # sparse, but not CSR
    sp.coo_matrix(np.eye(3)),
    None,
])
def test_upload_takes_only_csr(no_library, X):
    with pytest.raises(ValueError):
        engine.DeviceCSR.upload(X)


def test_upload_refuses_non_numeric_data_and_no_columns(no_library):
    with pytest.raises(ValueError):
        engine.DeviceCSR.upload(sp.csr_matrix(np.eye(3)).astype(np.complex128))
    with pytest.raises(ValueError):
        engine.DeviceCSR.upload(sp.csr_matrix((3, 0)))


@pytest.fixture
def shell(no_library):
    """a DeviceCSR of 6 x 5 around a handle that must never be used"""
    S = engine.DeviceCSR(ctypes.c_void_p(0x1000), (6, 5), np.float32, 7)
    yield S
    S.h = None                                                     # (nothing to destroy)


CODES = np.array([0, 1, 0, 1, -1, 0])


@pytest.mark.parametrize("kwargs", [
    dict(codes=CODES[:5]),                                        # length different from n
    dict(codes=CODES.reshape(2, 3)),
    dict(codes=CODES.astype(np.float64)),
    dict(codes=np.array([0, 1, 2, 1, -1, 0])),                    # a code >= n_groups
    dict(n_groups=0), dict(n_groups=9), dict(n_groups=2.5), dict(n_groups=True),
    dict(cols=[0, 5]), dict(cols=[-1]), dict(cols=[[0, 1]]), dict(cols=[0.0]),
    dict(transform="log1p"),
])
def test_group_moments_argument_errors(shell, kwargs):
    args = dict(codes=CODES, n_groups=2)
    args.update(kwargs)
    with pytest.raises(ValueError):
        shell.group_moments(**args)
    with pytest.raises(ValueError):                                # the module-level function forwards a DeviceCSR
        engine.group_moments(shell, **args)


def test_the_other_methods_check_first(shell):
    for ts in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="target_sum"):
            shell.normalize_log1p(ts)
    for cols in ([0, 5], [-1], [[0, 1]], [0.5], [1, 1]):
        with pytest.raises(ValueError):
            shell.densify(cols)
    assert shell.shape == (6, 5) and shell.dtype == np.float32 and shell.nnz == 7
    with pytest.raises(AssertionError, match="touched"):           # every check passed: the call is the first use of the library
        shell.group_moments(CODES, 2, cols=[4, 0])


def test_upload_leaves_a_non_canonical_input_unmodified():
    """duplicate entries and unsorted rows: the duplicates are summed in a copy (whether or not a device then takes it)"""
    indptr, indices = np.array([0, 3, 3, 5], dtype=np.int32), np.array([2, 0, 2, 1, 1], dtype=np.int32)
    data = np.array([1, 2, 3, 4, 5], dtype=np.int64)
    X = sp.csr_matrix((data.copy(), indices.copy(), indptr.copy()), shape=(3, 4))
    assert not X.has_canonical_format
    try:
        S = engine.DeviceCSR.upload(X)
    except _lib.PilotOTError:
        assert _lib.device_count() == 0
    else:
        assert S.shape == (3, 4) and S.dtype == np.float32 and S.nnz == 3
        S.close()
    assert X.nnz == 5 and X.data.dtype == np.int64
    assert np.array_equal(X.indptr, indptr) and np.array_equal(X.indices, indices) and np.array_equal(X.data, data)
    Y = sp.csr_matrix((np.array([1.0, 2.0]), np.array([3, 1]), np.array([0, 2])), shape=(1, 4))     # unsorted only
    before = (Y.indices.copy(), Y.data.copy())
    try:
        engine.DeviceCSR.upload(Y).close()
    except _lib.PilotOTError:
        assert _lib.device_count() == 0
    assert np.array_equal(Y.indices, before[0]) and np.array_equal(Y.data, before[1])
