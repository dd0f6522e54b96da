"""The argument helpers every engine function shares, without a device: engine._dense_arg (the one place a matrix argument becomes
ABI arguments) in its three modes, the moment-argument checks behind both group_moments entry points, and the P / M check.  The
library handle is replaced by an object that fails the test on any use, so every refusal is shown to come before the library."""
import ctypes

import numpy as np
import pytest

from pilot_amd import _lib, engine


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())


T = 5
W = np.arange(8 * 16, dtype=np.float32).reshape(8, 16)
VIEW = W[:, 3:3 + T]


def test_dense_arg_on_a_host_view(no_library):
    d = engine._dense_arg(VIEW, "Y", mode="strided")                # passed where it lies, with the parent's leading dimension
    assert (d.on_dev, d.rows, d.cols, d.ld, d.dtype) == (0, 8, T, 16, np.float32)
    assert d.ptr.value == VIEW.ctypes.data and d.keep is VIEW
    d = engine._dense_arg(VIEW, "Y")                               # the default: a packed copy
    assert (d.on_dev, d.rows, d.cols, d.ld, d.dtype) == (0, 8, T, T, np.float32)
    assert d.ptr.value == d.keep.ctypes.data != VIEW.ctypes.data
    assert d.keep.flags.c_contiguous and np.array_equal(d.keep, VIEW)
    with pytest.raises(ValueError, match=r"Y must be C-contiguous \(np.ascontiguousarray\), got strides \(64, 4\)"):
        engine._dense_arg(VIEW, "Y", mode="strict")
    # what the strided mode cannot pass as it is becomes a packed copy: a column stride, a reversed row order
    for V in (W[:, ::2], W[::-1, 3:3 + T], W.T):
        d = engine._dense_arg(V, "Y", mode="strided")
        assert d.ld == d.cols == V.shape[1] and d.keep.flags.c_contiguous and np.array_equal(d.keep, V)
    d = engine._dense_arg(W[::2, 3:3 + T], "Y", mode="strided")      # every other row: still one stride
    assert d.ld == 32 and d.rows == 4 and d.ptr.value == W.ctypes.data + 3 * 4
    assert engine._dense_arg(W[:1, 3:3 + T], "Y", mode="strided").ld == T        # a single row has no stride to speak of


@pytest.mark.parametrize("mode", ["packed", "strided"])
def test_dense_arg_converts_other_dtypes(no_library, mode):
    A = np.arange(12, dtype=np.int64).reshape(3, 4)
    d = engine._dense_arg(A, "Y", mode=mode)
    assert d.dtype == np.float64 and d.ld == 4 and np.array_equal(d.keep, A.astype(np.float64))
    d = engine._dense_arg(A.astype(np.float32), "Y", (np.float64,), mode=mode)      # the f64-only callers convert float32 too
    assert d.dtype == np.float64
    with pytest.raises(ValueError, match="Y must be 2-D, got"):
        engine._dense_arg(A[0], "Y", mode=mode)
    with pytest.raises(ValueError, match=r"Y must be 2-D \(observations x targets\), got \(4,\)"):
        engine._dense_arg(A[0], "Y", mode=mode, axes=" (observations x targets)")


def test_dense_arg_strict_refuses_what_it_would_have_to_convert(no_library):
    text = "Y: a 2-D float32 / float64 numpy array or a DeviceMatrix, got"
    for bad in (np.zeros((3, 4), dtype=np.int64), np.zeros((3, 4), dtype=np.float16), np.zeros(4), [[0.0, 1.0]]):
        with pytest.raises(ValueError, match=text):
            engine._dense_arg(bad, "Y", mode="strict")
    A = np.zeros((3, 4), dtype=np.float32)
    d = engine._dense_arg(A, "Y", mode="strict")
    assert d.keep is A and (d.rows, d.cols, d.ld) == (3, 4, 4)


def test_dense_arg_device_matrices(no_library):
    D = engine.DeviceMatrix(0x1000, 6, shape=(6, 5), dtype=np.float32)
    V = engine.device_columns(D, 1, 4)
    for mode in ("packed", "strided", "strict"):
        d = engine._dense_arg(D, "Y", mode=mode)
        assert (d.ptr.value, d.on_dev, d.rows, d.cols, d.ld, d.dtype) == (0x1000, 1, 6, 5, 5, np.float32)
    d = engine._dense_arg(V, "Y", mode="strict")                    # columns in place: the parent's width is the leading dimension
    assert (d.ptr.value, d.on_dev, d.rows, d.cols, d.ld) == (0x1000 + 4, 1, 6, 3, 5)
    for mode in ("packed", "strided"):                             # ... and only group_moments' route takes them
        with pytest.raises(ValueError, match="Y must be 2-D"):
            engine._dense_arg(V, "Y", mode=mode)
    with pytest.raises(ValueError):
        engine.trajectory_fits(V, np.arange(6.0))
    with pytest.raises(ValueError):
        engine.segment_std(V, [0, 6])
    with pytest.raises(AssertionError, match="touched"):           # group_moments gets as far as the library with it
        engine.group_moments(V, np.zeros(6, dtype=int), 1)
    # the f64-only callers refuse a float32 DeviceMatrix
    with pytest.raises(ValueError, match=r"noise: a 2-D float64 DeviceMatrix, got \(6, 5\) float32"):
        engine.fitted_curves(np.zeros((5, 3)), [0] * 5, np.arange(6.0), noise=D)
    with pytest.raises(ValueError, match=r"Y: a 2-D float64 DeviceMatrix, got \(6, 5\) float32"):
        engine.linkage_of_rows(D)
    with pytest.raises(ValueError, match=r"curves: a 2-D float64 DeviceMatrix, got \(6, 5\) float32"):
        engine.curve_activities(D, np.arange(5.0))
    with pytest.raises(ValueError, match=r"Y: a 2-D float32 / float64 DeviceMatrix, got \(6, 5\) float16"):
        engine.trajectory_fits(engine.DeviceMatrix(0x1000, 6, shape=(6, 5), dtype=np.float16), np.arange(6.0))


# ---- group_moments: the dense and the sparse entry point share their checks -----------------------------------------------------
CODES = np.array([0, 1, 0, 1, -1, 0])
BAD_MOMENT_ARGS = [                                               # tests/test_csr_args.py::test_group_moments_argument_errors
    dict(codes=CODES[:5]),
    dict(codes=CODES.reshape(2, 3)),
    dict(codes=CODES.astype(np.float64)),
    dict(codes=np.array([0, 1, 2, 1, -1, 0])),
    dict(n_groups=0), dict(n_groups=9), dict(n_groups=2.5), dict(n_groups=True),
    dict(cols=[0, 5]), dict(cols=[-1]), dict(cols=[[0, 1]]), dict(cols=[0.0]),
    dict(transform="log1p"),
]


@pytest.mark.parametrize("kwargs", BAD_MOMENT_ARGS, ids=[str(i) for i in range(len(BAD_MOMENT_ARGS))])
def test_both_group_moments_refuse_identically(no_library, kwargs):
    args = dict(codes=CODES, n_groups=2)
    args.update(kwargs)
    S = engine.DeviceCSR(ctypes.c_void_p(0x1000), (6, 5), np.float32, 7)
    try:
        with pytest.raises(ValueError) as sparse:
            S.group_moments(**args)
    finally:
        S.h = None                                                 # (nothing to destroy)
    with pytest.raises(ValueError) as dense:
        engine.group_moments(np.zeros((6, 5), dtype=np.float32), **args)
    assert type(sparse.value) is type(dense.value) is ValueError
    assert str(sparse.value) == str(dense.value) != ""


# ---- the P / M check --------------------------------------------------------------------------------------------------------------
def test_pair_inputs(no_library):
    P, M = np.full((5, 4), 0.25), np.ones((3, 3))
    text = r"shape mismatch: P \(5, 4\), M \(3, 3\)"
    with pytest.raises(ValueError, match=text):
        engine._pair_inputs(P, M)
    for call in (lambda: engine.sinkhorn_grid(P, M, 0.1), lambda: engine.emd_grid(P, M),
                 lambda: engine.transport_plans(P, M, [[0, 1]]), lambda: engine.DevicePlan(P, M)):
        with pytest.raises(ValueError, match=text):
            call()
    P2, M2, N, K = engine._pair_inputs(P.astype(np.float32).tolist(), np.ones((4, 4), dtype=np.int32))
    assert (N, K) == (5, 4) and P2.dtype == M2.dtype == np.float64 and P2.flags.c_contiguous
    with pytest.raises(ValueError, match="M contains NaN or inf"):
        engine._pair_inputs(P, np.full((4, 4), np.nan))
    with pytest.raises(ValueError, match="E must be square"):
        engine._square(np.zeros((3, 4)), "E")
