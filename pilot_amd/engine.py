"""NumPy-level face of the device engine (host buffers in, host buffers out).

These are the array-level operators ``tl.wasserstein_d`` / ``tl.cost_matrix`` are built on; they go
straight to ``libpilot_ot.so`` through ctypes.  No torch, no CPU fallback.
"""
from __future__ import annotations

import collections
import ctypes
import os

import numpy as np

from . import _lib

# POT defaults of ot.sinkhorn2 / sinkhorn_stabilized (what Trajectory.py:515 runs with)
NUM_ITER_MAX = 1000
STOP_THR = 1e-9
TAU = 1e3
CHECK_PERIOD = 20


def _as_f64(x, name):
    a = np.ascontiguousarray(x, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError("%s contains NaN or inf" % name)
    return a


class _Closing:
    """``close()`` when the object goes, whatever a constructor that failed half-way left behind"""

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ws_slot_names():
    """names of the workspace pool's slots, in slot order (no device needed)"""
    L = _lib.load()
    return [L.pilot_ot_ws_slot_name(i).decode() for i in range(L.pilot_ot_ws_slot_count())]


def ws_guard_report(reset=False):
    """``(seen names, damage)`` of the calling thread's workspace guard: the slots handed out under guard since the last reset and
    ``None`` or ``(slot name, first damaged offset past the request, request bytes)``"""
    L = _lib.load()
    names = ws_slot_names()
    seen = (ctypes.c_ubyte * len(names))()
    slot, off, req = ctypes.c_int(-1), ctypes.c_longlong(0), ctypes.c_longlong(0)
    _lib.check(L.pilot_ot_ws_guard_report(seen, ctypes.byref(slot), ctypes.byref(off), ctypes.byref(req), int(bool(reset))))
    damage = None if slot.value < 0 else (names[slot.value], off.value, req.value)
    return {n for n, s in zip(names, seen) if s}, damage


class ws_guard:
    """TEST HOOK: run the body with the workspace guard on (``PILOT_OT_WS_GUARD``, include/pilot_ot.h).  Entering resets the calling
    thread's report and sets the switch; leaving checks every canary, stores ``(seen names, damage or None)`` in ``result`` (also
    ``seen`` and ``damage``), resets the report and clears the switch.  ``mode="selftest"`` damages one canary byte on purpose."""

    def __init__(self, mode="1"):
        self.mode, self.result, self.seen, self.damage = mode, None, None, None

    def __enter__(self):
        ws_guard_report(reset=True)
        _lib.test_switch("PILOT_OT_WS_GUARD", self.mode)
        return self

    def __exit__(self, *exc):
        try:
            self.result = ws_guard_report(reset=True)
            self.seen, self.damage = self.result
        finally:
            _lib.test_switch("PILOT_OT_WS_GUARD", None)
        return False


def _square(A, name):
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("%s must be square, got %s" % (name, A.shape))
    return A


def _pair_inputs(P, M):
    """the pair grid's inputs: ``(P, M, N, K)`` with P (N x K) and M (K x K) finite float64"""
    P, M = _as_f64(P, "P"), _as_f64(M, "M")
    if P.ndim != 2 or M.ndim != 2 or M.shape[0] != M.shape[1] or M.shape[0] != P.shape[1]:
        raise ValueError("shape mismatch: P %s, M %s" % (P.shape, M.shape))
    return (P, M) + P.shape


def _code_columns(cell_code, sample_code, n_total, n_rows=None):
    """the two per-cell code columns as int32 (one entry per row of the embedding where ``n_rows`` is given) and n_total"""
    cc = np.ascontiguousarray(cell_code, dtype=np.int32)
    sc = np.ascontiguousarray(sample_code, dtype=np.int32)
    if n_rows is None:
        if cc.shape != sc.shape or cc.ndim != 1:
            raise ValueError("cell_code and sample_code must be 1-D arrays of equal length")
    elif cc.shape != (n_rows,) or sc.shape != cc.shape:
        raise ValueError("cell_code and sample_code must have one entry per row of X")
    return cc, sc, cc.size if n_total is None else int(n_total)


def _embedding_arg(X):
    """``(X, dtype code)``: the C x D embedding contiguous in its own dtype if that is float32, else as float64"""
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("X must be 2-D (cells, dims)")
    if X.dtype != np.float32:
        X = X.astype(np.float64, copy=False)
    return np.ascontiguousarray(X), _lib.dtype_code(X.dtype)


def n_rows_of(N, row_begin, row_end, row_step):
    return len(range(row_begin, N if row_end is None else row_end, row_step))


def sinkhorn_grid(P, M, reg, num_iter_max=NUM_ITER_MAX, stop_thr=STOP_THR, tau=TAU,
                  check_period=CHECK_PERIOD, precision="auto", f32_floor_ulps=0.0,
                  row_begin=0, row_end=None, row_step=1, return_info=False):
    """Entropic OT cost <Gamma, M> for ordered pairs (selected rows x all N columns).

    Device replacement of the loop at pilotpy/tools/Trajectory.py:512-515; each pair follows
    ``ot.sinkhorn2(P[i], P[j], M, reg, method="sinkhorn_stabilized")``.

    P : (N, K) proportion vectors; M : (K, K) cost (already divided by its max).
    Returns float64 (n_rows, N) and, with ``return_info``, a dict of iters / err / flags arrays.
    """
    P, M, N, K = _pair_inputs(P, M)
    if precision not in _lib.PREC:
        raise ValueError("precision must be one of %s" % sorted(_lib.PREC))
    row_end = N if row_end is None else int(row_end)
    n_rows = n_rows_of(N, row_begin, row_end, row_step)
    emd = np.empty((n_rows, N), dtype=np.float64)
    L = _lib.load()
    sym = int(np.array_equal(M, M.T))
    if return_info:
        iters = np.empty((n_rows, N), dtype=np.int32)
        err = np.empty((n_rows, N), dtype=np.float64)
        flags = np.empty((n_rows, N), dtype=np.int32)
        pi, pe, pf = _lib.iptr(iters), _lib.dptr(err), _lib.iptr(flags)
    else:                                  # only the matrix travels back
        pi = pe = pf = None
    _lib.check(L.pilot_ot_sinkhorn_grid(
        _lib.dptr(P), N, K, _lib.dptr(M), float(reg), int(num_iter_max), float(stop_thr), float(tau),
        int(check_period), _lib.PREC[precision], float(f32_floor_ulps), sym,
        int(row_begin), row_end, int(row_step), _lib.dptr(emd), pi, pe, pf))
    if return_info:
        return emd, dict(iters=iters, err=err, flags=flags)
    return emd


def pdist_square(centroids, metric="cosine"):
    """Square pairwise-distance matrix of the K centroids (device replacement of
    ``squareform(pdist(centroids, metric))``, pilotpy/tools/Trajectory.py:468-469)."""
    X = _as_f64(centroids, "centroids")
    if X.ndim != 2:
        raise ValueError("centroids must be 2-D (K, D)")
    if metric not in _lib.METRICS:
        raise NotImplementedError("metric %r: the device kernel implements scipy's pdist names %s" % (metric, sorted(_lib.METRICS)))
    K, D = X.shape
    out = np.zeros((K, K), dtype=np.float64)
    aux = None
    if metric == "mahalanobis":
        # scipy's own preparation (scipy/spatial/distance.py::_validate_mahalanobis_kwargs): VI = inv(cov(X^T))^T on the host
        if K <= D:
            raise ValueError("The number of observations (%d) is too small; the covariance matrix is singular. For observations "
                             "with %d dimensions, at least %d observations are required." % (K, D, D + 1))
        aux = np.ascontiguousarray(np.linalg.inv(np.atleast_2d(np.cov(X.T))).T, dtype=np.float64)
    _lib.check(_lib.load().pilot_ot_cost_matrix_ex(_lib.dptr(X), K, D, _lib.METRICS[metric], _lib.dptr(aux) if aux is not None else None,
                                                   _lib.dptr(out)))
    return out


def proportions(cell_code, sample_code, n_samples, n_types, regulizer=0.2, normalization=True, n_total=None):
    """N x K smoothed cell-type proportions from per-cell integer codes (device histogram; replaces the pandas
    loops of Cluster_Representations, pilotpy/tools/Trajectory.py:400-430).  Bit-identical to the reference."""
    cc, sc, n_total = _code_columns(cell_code, sample_code, n_total)
    P = np.zeros((n_samples, n_types), dtype=np.float64)
    _lib.check(_lib.load().pilot_ot_proportions(_lib.iptr(cc), _lib.iptr(sc), cc.size, n_total, int(n_samples),
                                                int(n_types), float(regulizer), int(bool(normalization)), _lib.dptr(P)))
    return P


def proportions_and_first_rows(cell_code, sample_code, n_samples, n_types, regulizer=0.2, normalization=True, n_total=None):
    """:func:`proportions` plus, from the same pass over the codes, the first row of every sample (int64, -1: none) --
    the row ``return_real_labels`` reads (pilotpy/tools/Trajectory.py:617-642)."""
    cc, sc, n_total = _code_columns(cell_code, sample_code, n_total)
    P = np.zeros((n_samples, n_types), dtype=np.float64)
    first = np.full(n_samples, -1, dtype=np.int64)
    _lib.check(_lib.load().pilot_ot_proportions_ex(
        _lib.iptr(cc), _lib.iptr(sc), cc.size, n_total, int(n_samples), int(n_types), float(regulizer), int(bool(normalization)),
        _lib.dptr(P), _lib.lptr(first)))
    return P, first


def label_codes(ids, max_uniques=1 << 16, n_threads=None):
    """``(codes int32, first_rows int64)``: the labels of one column numbered in order of first appearance, -1 = missing
    (host pass of ``libpilot_ot.so``, ``pilot_ot_label_codes``: what ``Series.unique()`` and the per-label masks of
    pilotpy/tools/Trajectory.py:402-425 amount to).  ``ids``: 1-D contiguous int8/int16/int32 (negative = missing: the codes
    of a pandas Categorical) or uint64 (opaque identities, 0 = missing).  ``None`` when the column holds more than
    ``max_uniques`` distinct labels (the caller then takes another route)."""
    ids = np.ascontiguousarray(ids)
    if ids.ndim != 1 or ids.dtype not in (np.int8, np.int16, np.int32, np.uint64):
        raise ValueError("ids must be a 1-D int8 / int16 / int32 / uint64 array")
    if n_threads is None:
        n_threads = max(1, min(4, (os.cpu_count() or 2) // 2))
    codes = np.empty(ids.size, dtype=np.int32)
    first = np.empty(int(max_uniques), dtype=np.int64)
    n_u = ctypes.c_int(0)
    rc = _lib.load().pilot_ot_label_codes(ctypes.c_void_p(ids.ctypes.data), ids.itemsize, ids.size, int(max_uniques), int(n_threads),
                                          _lib.iptr(codes), _lib.lptr(first), ctypes.byref(n_u))
    if rc == _lib.ENOTSUP:
        return None
    _lib.check(rc)
    return codes, first[:n_u.value]


class EmbeddingUpload(_Closing):
    """The C x D embedding on its way to the device: the copy runs on a helper thread (ctypes releases the GIL) while the
    caller factorises the label columns; :meth:`medians` joins it and runs the device radix select.

    A SMALL embedding (below ``SMALL_BYTES``: the reference test's own cohort is 1.3 MB) is not worth a thread, a device
    allocation and the ``hipFree`` that synchronises the device at the end -- 0.4 ms of a 2.8 ms call: it goes up inside
    :meth:`medians`, through the calling thread's buffer pool (``pilot_ot_centroid_medians`` on the host array)."""

    SMALL_BYTES = 4 << 20

    def __init__(self, X):
        import threading
        self.X, self.dt = _embedding_arg(X)
        self.L = _lib.load()
        self.h = ctypes.c_void_p()
        self.err = None
        dev = ctypes.c_int(0)
        _lib.check(self.L.pilot_ot_get_device(ctypes.byref(dev)))
        self.device = dev.value
        self.thread = None
        if self.X.nbytes < self.SMALL_BYTES:
            return

        def work():
            try:
                _lib.check(self.L.pilot_ot_set_device(self.device))      # (a new host thread starts on device 0)
                _lib.check(self.L.pilot_ot_embedding_upload(ctypes.c_void_p(self.X.ctypes.data), self.dt, self.X.shape[0],
                                                            self.X.shape[1], ctypes.byref(self.h)))
            except BaseException as e:      # re-raised by the caller's thread in medians()
                self.err = e

        self.thread = threading.Thread(target=work, name="pilot_ot_embedding_upload")
        self.thread.start()

    def medians(self, cell_code, n_types):
        if self.thread is None:
            return centroid_medians(self.X, cell_code, n_types)
        self.thread.join()
        if self.err is not None:
            raise self.err
        cc = np.ascontiguousarray(cell_code, dtype=np.int32)
        if cc.shape != (self.X.shape[0],):
            raise ValueError("cell_code must have one entry per row of X")
        out = np.zeros((int(n_types), self.X.shape[1]), dtype=np.float64)
        _lib.check(self.L.pilot_ot_centroid_medians_dev(self.h, _lib.iptr(cc), int(n_types), _lib.dptr(out)))
        return out

    def prepass(self, cell_code, sample_code, n_samples, n_types, regulizer=0.2, normalization=True, n_total=None):
        """``(P, first_rows, centroids)`` -- :func:`proportions_and_first_rows` and :meth:`medians` from ONE upload of the two
        code columns (``pilot_ot_prepass_dev``): the same bits as the separate calls, a third of their transfers."""
        if self.thread is None:
            P, first = proportions_and_first_rows(cell_code, sample_code, n_samples, n_types, regulizer=regulizer,
                                                  normalization=normalization, n_total=n_total)
            return P, first, centroid_medians(self.X, cell_code, n_types)
        self.thread.join()
        if self.err is not None:
            raise self.err
        cc, sc, n_total = _code_columns(cell_code, sample_code, n_total, n_rows=self.X.shape[0])
        P = np.zeros((int(n_samples), int(n_types)), dtype=np.float64)
        first = np.full(int(n_samples), -1, dtype=np.int64)
        cen = np.zeros((int(n_types), self.X.shape[1]), dtype=np.float64)
        _lib.check(self.L.pilot_ot_prepass_dev(self.h, _lib.iptr(cc), _lib.iptr(sc), n_total, int(n_samples), int(n_types),
                                               float(regulizer), int(bool(normalization)), _lib.dptr(P), _lib.lptr(first),
                                               _lib.dptr(cen)))
        return P, first, cen

    def close(self):
        if self.thread is not None:
            self.thread.join()
        if self.h:
            self.L.pilot_ot_embedding_destroy(self.h)
            self.h = ctypes.c_void_p()


def centroid_medians(X, cell_code, n_types):
    """K x D per-cell-type column-wise medians of the C x D embedding (device radix select; replaces
    ``data[annot.cell_type == k].median(axis=0)``, pilotpy/tools/Trajectory.py:465-466).  float32 / float64 input is
    processed in its own dtype, like pandas."""
    X, dt = _embedding_arg(X)
    cc = np.ascontiguousarray(cell_code, dtype=np.int32)
    if cc.shape != (X.shape[0],):
        raise ValueError("cell_code must have one entry per row of X")
    out = np.zeros((int(n_types), X.shape[1]), dtype=np.float64)
    _lib.check(_lib.load().pilot_ot_centroid_medians(ctypes.c_void_p(X.ctypes.data), dt, X.shape[0], X.shape[1],
                                                     _lib.iptr(cc), int(n_types), _lib.dptr(out)))
    return out


def _cell_inputs(X, offsets):
    X = np.ascontiguousarray(X, dtype=np.float32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if X.ndim != 2 or offsets.ndim != 1 or offsets.size < 2 or offsets[0] != 0 or offsets[-1] != X.shape[0]:
        raise ValueError("X must be (C, D) and offsets (N + 1,) with offsets[0] = 0, offsets[-1] = C")
    if not np.all(np.isfinite(X)):
        raise ValueError("X contains NaN or inf")
    return X, offsets


class CellCohort(_Closing):
    """Device-resident cell clouds for the cell-level W2 extension (``pilot_ot_cell_cohort_*``): the cells stay in HBM as
    fp16 / bf16 operand pieces across calls, a call moves only result rows."""

    def __init__(self, X, offsets):
        X, offsets = _cell_inputs(X, offsets)
        self.N, self.D = offsets.size - 1, X.shape[1]
        self.cells_per_patient = np.diff(offsets)
        self.L = _lib.load()
        self.h = ctypes.c_void_p()
        _lib.check(self.L.pilot_ot_cell_cohort_create(ctypes.c_void_p(X.ctypes.data), ctypes.c_void_p(offsets.ctypes.data),
                                                      self.N, self.D, ctypes.byref(self.h)))
        self.last_kernel_ms = None

    def w2_grid(self, scale, reg, num_iter_max=1000, stop_thr=1e-9, check_period=10, f32_floor_ulps=0.0,
                row_begin=0, row_end=None, row_step=1, return_info=False):
        row_end = self.N if row_end is None else int(row_end)
        n_rows = n_rows_of(self.N, row_begin, row_end, row_step)
        w2 = np.zeros((n_rows, self.N), dtype=np.float64)
        iters = np.zeros((n_rows, self.N), dtype=np.int32)
        err = np.zeros((n_rows, self.N), dtype=np.float64)
        ms = ctypes.c_float(0.0)
        _lib.check(self.L.pilot_ot_cell_w2_grid_cohort(self.h, float(scale), float(reg), int(num_iter_max), float(stop_thr),
                                                       int(check_period), float(f32_floor_ulps), int(row_begin), row_end,
                                                       int(row_step), _lib.dptr(w2), _lib.iptr(iters), _lib.dptr(err),
                                                       ctypes.byref(ms)))
        self.last_kernel_ms = float(ms.value)
        pieces = ctypes.c_int(0)
        _lib.check(self.L.pilot_ot_cell_cohort_pieces(self.h, ctypes.byref(pieces)))
        self.last_pieces = pieces.value           # 2: fp16 operand pieces (3 piece products per tile), 3: bf16 (6)
        if return_info:
            return w2, dict(iters=iters, err=err)
        return w2

    def close(self):
        if self.h:
            self.L.pilot_ot_cell_cohort_destroy(self.h)
            self.h = ctypes.c_void_p()


def cell_w2_grid(X, offsets, scale, reg, num_iter_max=1000, stop_thr=1e-9, check_period=10, f32_floor_ulps=0.0,
                 row_begin=0, row_end=None, row_step=1, return_info=False, devices=None):
    """EXTENSION (not in the reference; BASELINE config 5): entropic W2 cost between patients' raw cell clouds.

    X: (C, D) float32 embedding with every patient's cells contiguous; offsets: (N + 1,) row ranges.  Pair (i, j):
    uniform weights, cost |x - y|^2 / scale, log-domain Sinkhorn with POT ``sinkhorn_log`` control flow; returns the
    (n_rows, N) matrix of <Gamma, C>.  ``devices=[...]``: the full grid with its rows dealt round-robin over several GPUs."""
    X, offsets = _cell_inputs(X, offsets)
    N = offsets.size - 1
    if devices is not None:
        if row_begin != 0 or row_end not in (None, N) or row_step != 1:
            raise ValueError("devices=[...] computes the full grid")
        dev = np.ascontiguousarray([int(d) for d in devices], dtype=np.int32)
        w2 = np.zeros((N, N), dtype=np.float64)
        iters = np.zeros((N, N), dtype=np.int32)
        err = np.zeros((N, N), dtype=np.float64)
        _lib.check(_lib.load().pilot_ot_cell_w2_grid_multi(
            ctypes.c_void_p(X.ctypes.data), ctypes.c_void_p(offsets.ctypes.data), N, X.shape[1], float(scale), float(reg),
            int(num_iter_max), float(stop_thr), int(check_period), float(f32_floor_ulps), _lib.iptr(dev), len(dev),
            _lib.dptr(w2), _lib.iptr(iters), _lib.dptr(err)))
        return (w2, dict(iters=iters, err=err)) if return_info else w2
    co = CellCohort(X, offsets)
    try:
        return co.w2_grid(scale, reg, num_iter_max=num_iter_max, stop_thr=stop_thr, check_period=check_period,
                          f32_floor_ulps=f32_floor_ulps, row_begin=row_begin, row_end=row_end, row_step=row_step,
                          return_info=return_info)
    finally:
        co.close()


class DevicePlan(_Closing):
    """Device-resident pair-grid problem: P, M and the outputs live in HBM across calls.

    Used by ``bench.py`` (inputs resident before the timed region) and by the multi-GPU driver.
    Device memory comes from the library's own allocator (no torch needed); pointers can equally
    be torch ``data_ptr()`` values when the caller wants torch to own the buffers.
    """

    def __init__(self, P, M, n_rows_max=None):
        P, M, self.N, self.K = _pair_inputs(P, M)
        self.sym = int(np.array_equal(M, M.T))
        self.L = _lib.load()
        self._bufs = []
        self.plan = ctypes.c_void_p()
        _lib.check(self.L.pilot_ot_plan_create(self.N, self.K, ctypes.byref(self.plan)))
        # the device entry point cannot see max(M): the plan carries it, and every range decision (what AUTO means, the
        # fp16-split domain, the hand-over thresholds) is taken on max(M) / reg -- M need not be normalised
        self.max_cost = float(M.max()) if M.size else 1.0
        if not (self.max_cost > 0.0 and np.isfinite(self.max_cost)):
            self.max_cost = 1.0            # (an all-zero / NaN cost: every range decision as for the normalised cost, never a stale value)
        _lib.check(self.L.pilot_ot_plan_set_max_cost(self.plan, self.max_cost))
        self.n_rows_max = self.N if n_rows_max is None else n_rows_max
        n_out = self.n_rows_max * self.N
        self._bufs = [_DeviceBuffer.holding(P), _DeviceBuffer.holding(M)] + [_DeviceBuffer(b * n_out) for b in (8, 8, 4, 4)]
        self.dP, self.dM, self.dE, self.dErr, self.dIt, self.dFl = (buf.ptr for buf in self._bufs)

    def run(self, reg, row_begin=0, row_end=None, row_step=1, precision="auto", num_iter_max=NUM_ITER_MAX,
            stop_thr=STOP_THR, tau=TAU, check_period=CHECK_PERIOD, f32_floor_ulps=0.0, stream=None,
            d_emd=None):
        """Enqueue one pass over the selected rows (asynchronous)."""
        row_end = self.N if row_end is None else row_end
        if n_rows_of(self.N, row_begin, row_end, row_step) > self.n_rows_max:
            raise ValueError("row selection exceeds the plan's n_rows_max")
        _lib.check(self.L.pilot_ot_sinkhorn_grid_dev(
            self.plan, self.dP, self.dM, float(reg), int(num_iter_max), float(stop_thr), float(tau),
            int(check_period), _lib.PREC[precision], float(f32_floor_ulps), self.sym,
            int(row_begin), int(row_end), int(row_step),
            self.dE if d_emd is None else ctypes.c_void_p(d_emd), self.dIt, self.dErr, self.dFl,
            ctypes.c_void_p(stream) if stream else None))

    def enable_timing(self, enable=True):
        """HIP events around the pair-grid kernels of every call (``True``) or of every n-th call (``enable=n``)."""
        _lib.check(self.L.pilot_ot_plan_enable_timing(self.plan, int(enable)))

    def enable_graph(self, enable=True):
        """Replay repeated identical `run` calls as one hipGraph launch (pilot_ot_plan_enable_graph)."""
        _lib.check(self.L.pilot_ot_plan_enable_graph(self.plan, int(enable)))

    def kernel_times_ms(self, max_n=64):
        """(main_ms, track_ms) float arrays of the most recent timed calls (sync the stream first)."""
        a = (ctypes.c_float * max_n)()
        b = (ctypes.c_float * max_n)()
        n = ctypes.c_int(0)
        _lib.check(self.L.pilot_ot_plan_kernel_times(self.plan, max_n, a, b, ctypes.byref(n)))
        return np.array(a[:n.value]), np.array(b[:n.value])

    def sync(self, stream=None):
        _lib.check(self.L.pilot_ot_stream_sync(ctypes.c_void_p(stream) if stream else None))

    def device_matrix(self):
        """The N x N result of the last full-grid run as it sits in HBM (sync first), for the device-side consumers."""
        if self.n_rows_max != self.N:
            raise ValueError("the plan holds a row shard, not the full matrix")
        return DeviceMatrix(self.dE, self.N, owner=self)

    def fetch(self, n_rows=None):
        n_rows = self.n_rows_max if n_rows is None else n_rows

        def rows(ptr, dtype):
            return download(DeviceMatrix(ptr, self.N, shape=(n_rows, self.N), dtype=dtype))
        return rows(self.dE, np.float64), dict(iters=rows(self.dIt, np.int32), err=rows(self.dErr, np.float64),
                                               flags=rows(self.dFl, np.int32))

    def close(self):
        for buf in self._bufs:
            buf.free()
        self._bufs = []
        if self.plan:
            self.L.pilot_ot_plan_destroy(self.plan)
            self.plan = ctypes.c_void_p()


def equal_masses(P, rtol=1e-12):
    """ot.emd2 rescales b to the mass of a, so emd2(a, b) = sum(a) * W(a / sum a, b / sum b): the matrix of a symmetric cost
    is symmetric only when every histogram carries the same mass (to rounding)."""
    s = np.asarray(P, dtype=np.float64).sum(1)
    return s.size == 0 or float(s.max() - s.min()) <= rtol * max(float(np.abs(s).max()), 1e-300)


def emd_grid(P, M, row_begin=0, row_end=None, row_step=1, mode="auto", return_info=False):
    """Exact OT cost for ordered pairs (device replacement of the ``ot.emd2`` loop,
    pilotpy/tools/Trajectory.py:507-511).

    mode: "all" solves every (row, column) pair; "upper" only column >= row (rest left 0);
    "mirror" = upper + device-side mirroring (full square grid only); "auto" picks "mirror"
    when M is exactly symmetric, all histograms carry the same mass (see equal_masses) and the full grid is requested,
    else "all".
    """
    P, M, N, K = _pair_inputs(P, M)
    row_end = N if row_end is None else int(row_end)
    full = (row_begin == 0 and row_end == N and row_step == 1)
    if mode == "auto":
        mode = "mirror" if (full and np.array_equal(M, M.T) and equal_masses(P)) else "all"
    modes = {"all": _lib.EMD_ALL, "upper": _lib.EMD_UPPER, "mirror": _lib.EMD_MIRROR}
    if mode not in modes:
        raise ValueError("mode must be one of %s" % sorted(modes))
    n_rows = n_rows_of(N, row_begin, row_end, row_step)
    emd = np.zeros((n_rows, N), dtype=np.float64)
    n_aug = np.zeros((n_rows, N), dtype=np.int32)
    _lib.check(_lib.load().pilot_ot_emd_grid(_lib.dptr(P), N, K, _lib.dptr(M), modes[mode], int(row_begin), row_end,
                                             int(row_step), _lib.dptr(emd), _lib.iptr(n_aug)))
    if (n_aug < 0).any():
        raise _lib.PilotOTError("exact-EMD kernel: augmentation guard tripped on %d pairs" % int((n_aug < 0).sum()))
    if return_info:
        return emd, dict(n_aug=n_aug)
    return emd


def transport_plans(P, M, pairs, regularized="unreg", reg=0.1, groups=None, return_info=False,
                    num_iter_max=NUM_ITER_MAX, stop_thr=STOP_THR, tau=TAU, check_period=CHECK_PERIOD):
    """Optimal couplings Gamma (K x K) of the ordered pairs ``pairs`` (extension: POT's ``ot.emd`` / ``ot.sinkhorn``
    return them, the pair grid keeps only <M, Gamma>).  Rows of a plan are the cell types of ``P[i]``, columns those of
    ``P[j]``.

    regularized == "unreg": the plan of ``ot.emd(a, b * sum(a) / sum(b), M)`` -- *an* optimum: the LP's value is unique,
    its plan need not be.  Anything else: ``ot.sinkhorn(a, b, M, reg, method="sinkhorn_stabilized")`` in f64, POT's
    loop step by step (the kernel of ``sinkhorn_grid(precision="generic")``), whatever precision a grid would run in.

    pairs : (n, 2) int array of (i, j).  groups : optional int array of length n; with it the result is (G, K, K),
    G = max(groups) + 1, the sum of the plans of each group's pairs added in list order (bit-reproducible); without it
    (n, K, K).  ``return_info`` adds a dict: values (<M, Gamma> per pair, what the pair grid returns), iters (exact:
    augmentations; entropic: iterations) and flags (entropic: the PILOT_OT_FLAG_* bits of the grid; exact: 0).
    """
    P, M, N, K = _pair_inputs(P, M)
    pairs = np.asarray(pairs)
    if pairs.size == 0:
        pairs = pairs.reshape(0, 2)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or not np.issubdtype(pairs.dtype, np.integer):
        raise ValueError("pairs must be an (n, 2) integer array, got %s %s" % (pairs.shape, pairs.dtype))
    n = pairs.shape[0]
    if n and (pairs.min() < -2**31 or pairs.max() >= 2**31):
        raise ValueError("pair index out of range for N=%d" % N)
    pi = np.ascontiguousarray(pairs[:, 0], dtype=np.int32)
    pj = np.ascontiguousarray(pairs[:, 1], dtype=np.int32)
    if groups is not None:
        groups = np.asarray(groups)
        if groups.shape != (n,) or not np.issubdtype(groups.dtype, np.integer):
            raise ValueError("groups must be an integer array of length %d, got %s %s" % (n, groups.shape, groups.dtype))
        if n and (groups.min() < -2**31 or groups.max() >= 2**31 - 1):
            raise ValueError("group id out of range")
        G = max(int(groups.max()) + 1, 1) if n else 0
        gp = np.ascontiguousarray(groups, dtype=np.int32)
        plans = np.zeros((G, K, K), dtype=np.float64)
    else:
        G, gp = 0, None
        plans = np.zeros((n, K, K), dtype=np.float64)
    values = np.zeros(n, dtype=np.float64)
    iters = np.zeros(n, dtype=np.int32)
    flags = np.zeros(n, dtype=np.int32)
    exact = regularized == "unreg"
    _lib.check(_lib.load().pilot_ot_transport_plans(
        _lib.dptr(P), N, K, _lib.dptr(M), 0 if exact else 1, float(reg), int(num_iter_max), float(stop_thr), float(tau),
        int(check_period), _lib.iptr(pi), _lib.iptr(pj), n, None if gp is None else _lib.iptr(gp), max(G, 1),
        _lib.dptr(plans), _lib.dptr(values), _lib.iptr(iters), _lib.iptr(flags)))
    if exact and (iters < 0).any():
        raise _lib.PilotOTError("exact-EMD kernel: augmentation guard tripped on %d pairs" % int((iters < 0).sum()))
    if return_info:
        return plans, dict(values=values, iters=iters, flags=flags)
    return plans


# ---- consumers of the finished matrix ------------------------------------------------------------
def row_distances(E, metric="euclidean", normalize_by_max=False):
    """Distances between the ROWS of the N x N matrix E (of E / E.max() with ``normalize_by_max``) on the device: the points
    pilotpy's diffusion map (pilotpy/plot/ploting.py:95-110) and silhouette scores (pilotpy/tools/Trajectory.py:592-612)
    work with.  metric: "euclidean" (scipy cdist) or "cosine" (sklearn cosine_distances)."""
    E = _square(_as_f64(E, "E"), "E")
    if metric not in _lib.ROW_METRICS:
        raise NotImplementedError("row metric %r: the device kernel implements %s" % (metric, sorted(_lib.ROW_METRICS)))
    D = np.empty_like(E)
    _lib.check(_lib.load().pilot_ot_row_distances(_lib.dptr(E), E.shape[0], int(bool(normalize_by_max)),
                                                  _lib.ROW_METRICS[metric], _lib.dptr(D)))
    return D


def silhouette_precomputed(D, labels, return_samples=False):
    """``sklearn.metrics.silhouette_score(D, labels, metric="precomputed")`` on the device (labels of any hashable type)."""
    D = _square(_as_f64(D, "D"), "D")
    codes, n_clusters = _label_codes(labels, D.shape[0])
    score = ctypes.c_double(0.0)
    samples = np.empty(D.shape[0], dtype=np.float64)
    _lib.check(_lib.load().pilot_ot_silhouette(_lib.dptr(D), _lib.iptr(codes), D.shape[0], n_clusters, ctypes.byref(score),
                                               _lib.dptr(samples)))
    return (score.value, samples) if return_samples else score.value


def _label_codes(labels, n):
    uniq, codes = np.unique(np.asarray(labels), return_inverse=True)
    if codes.shape != (n,):
        raise ValueError("one label per sample expected")
    return np.ascontiguousarray(codes, dtype=np.int32), len(uniq)


_Dense = collections.namedtuple("_Dense", "ptr on_dev rows cols ld dtype keep")


def _dense_arg(Y, name, dtypes=(np.float32, np.float64), mode="packed", axes=""):
    """The one place a matrix argument becomes ABI arguments: pointer, is_device, rows, columns, leading dimension, dtype and
    what keeps the pointer valid, of a 2-D numpy array or :class:`DeviceMatrix` of one of ``dtypes``.  A host array of another
    dtype is converted to float64; then ``mode="packed"`` passes it C-contiguous and ``"strided"`` leaves a view with a unit
    column stride and a row stride of whole items as it is, with its own ``ld``.  ``"strict"`` converts and copies nothing:
    anything but a C-contiguous ndarray of ``dtypes`` is refused, and :func:`device_columns` of a DeviceMatrix is taken too."""
    kinds = " / ".join(np.dtype(d).name for d in dtypes)
    if isinstance(Y, (DeviceMatrix, _DeviceColumns) if mode == "strict" else DeviceMatrix):
        if len(Y.shape) != 2 or Y.dtype not in dtypes:
            raise ValueError("%s: a 2-D %s DeviceMatrix, got %s %s" % (name, kinds, Y.shape, Y.dtype))
        return _Dense(ctypes.c_void_p(Y.ptr), 1, Y.shape[0], Y.shape[1], getattr(Y, "ld", Y.shape[1]), Y.dtype, Y)
    if mode == "strict":
        if not isinstance(Y, np.ndarray) or Y.ndim != 2 or Y.dtype not in dtypes:
            raise ValueError("%s: a 2-D %s numpy array or a DeviceMatrix, got %s %s"
                             % (name, kinds, getattr(Y, "shape", type(Y).__name__), getattr(Y, "dtype", "")))
        if not Y.flags.c_contiguous:
            raise ValueError("%s must be C-contiguous (np.ascontiguousarray), got strides %s" % (name, Y.strides))
    else:
        Y = np.asarray(Y)
        if Y.ndim != 2:
            raise ValueError("%s must be 2-D%s, got %s" % (name, axes, Y.shape))
        if Y.dtype not in dtypes:
            Y = Y.astype(np.float64)
        if mode != "strided" or Y.strides[1] != Y.itemsize or Y.strides[0] % Y.itemsize or Y.strides[0] < 0:
            Y = np.ascontiguousarray(Y)
    ld = Y.strides[0] // Y.itemsize if mode == "strided" and Y.shape[0] > 1 else Y.shape[1]
    return _Dense(ctypes.c_void_p(Y.ctypes.data), 0, Y.shape[0], Y.shape[1], ld, Y.dtype, Y)


def _matrix_arg(E, name="E"):
    """:func:`_dense_arg` of a square float64 matrix: a finite numpy array or a device-resident result (DeviceMatrix)"""
    if isinstance(E, DeviceMatrix):
        _square_f64(E, name)
    else:
        E = _square(_as_f64(E, name), name)
    return _dense_arg(E, name, (np.float64,))


def _square_f64(D, name):
    """the consumers of the pair-grid matrix read an N x N float64 DeviceMatrix"""
    if D.shape != (D.N, D.N) or D.dtype != np.float64:
        raise ValueError("%s: an N x N float64 DeviceMatrix, got %s %s" % (name, D.shape, D.dtype))


class DeviceMatrix:
    """An N x N fp64 matrix that lives in HBM (e.g. ``DevicePlan.device_matrix()`` after a full-grid run, or
    ``multi.MultiPlan.device_matrix()``): the consumers below take it without a trip through host memory."""

    def __init__(self, ptr, N, owner=None, shape=None, dtype=np.float64):
        self.ptr = int(ptr.value if isinstance(ptr, ctypes.c_void_p) else ptr)
        self.N = int(N)
        self.owner = owner            # keeps the allocation alive
        self.shape = (self.N, self.N) if shape is None else tuple(int(v) for v in shape)   # (rows, columns), row-major, dense
        self.dtype = np.dtype(dtype)

    @classmethod
    def upload(cls, A):
        """A copy of the 2-D float32 / float64 array A in HBM (freed with the returned object)."""
        A = np.asarray(A)
        if A.ndim != 2 or A.dtype not in (np.float32, np.float64):
            raise ValueError("upload: a 2-D float32 / float64 array, got %s %s" % (A.shape, A.dtype))
        buf = _DeviceBuffer.holding(A)
        return cls(buf.ptr, A.shape[0], owner=buf, shape=A.shape, dtype=A.dtype)


class _DeviceBuffer(_Closing):
    """The owner of a pilot_ot_dev_alloc allocation, released by :meth:`free` or when the object goes."""

    def __init__(self, nbytes):
        self.ptr = ctypes.c_void_p()
        _lib.check(_lib.load().pilot_ot_dev_alloc(ctypes.byref(self.ptr), max(int(nbytes), 1)))

    @classmethod
    def holding(cls, A):
        """a buffer that holds the bytes of the array A (made C-contiguous): this module's host-to-device copy"""
        A = np.ascontiguousarray(A)
        buf = cls(A.nbytes)
        _lib.check(_lib.load().pilot_ot_memcpy_h2d(buf.ptr, A.ctypes.data, A.nbytes))
        return buf

    def free(self):
        if self.ptr:
            _lib.load().pilot_ot_dev_free(self.ptr)
            self.ptr = ctypes.c_void_p()

    close = free


def silhouette_of_rows(E, labels, metric="cosine", normalize_by_max=False, return_samples=False):
    """``sklearn.metrics.silhouette_score(E, labels, metric=metric)`` with the ROWS of E as the points -- what
    ``Sil_computing`` does (pilotpy/tools/Trajectory.py:592-612): row distances and silhouette chained on the device, only the
    N per-sample scores come back.  E: numpy array or :class:`DeviceMatrix`."""
    E = _matrix_arg(E)
    N = E.rows
    if metric not in _lib.ROW_METRICS:
        raise NotImplementedError("row metric %r: the device kernel implements %s" % (metric, sorted(_lib.ROW_METRICS)))
    codes, n_clusters = _label_codes(labels, N)
    score = ctypes.c_double(0.0)
    samples = np.empty(N, dtype=np.float64)
    _lib.check(_lib.load().pilot_ot_silhouette_of_rows(E.ptr, E.on_dev, N, int(bool(normalize_by_max)), _lib.ROW_METRICS[metric],
                                                       _lib.iptr(codes), n_clusters, ctypes.byref(score), _lib.dptr(samples)))
    return (score.value, samples) if return_samples else score.value


def diffusion_kernel_of_rows(E, k=64, epsilon=1.0, return_distances=True):
    """The dense part of ``pl.trajectory`` (pilotpy/plot/ploting.py:95-110) chained on the device: E / E.max() -> Euclidean row
    distances -> pydiffmap's k-nearest-neighbour Gaussian kernel.  Returns ``(D, Kmat)`` (``D`` None unless asked for)."""
    E = _matrix_arg(E)
    N = E.rows
    D = np.empty((N, N), dtype=np.float64) if return_distances else None
    Kmat = np.empty((N, N), dtype=np.float64)
    _lib.check(_lib.load().pilot_ot_diffusion_kernel_of_rows(E.ptr, E.on_dev, N, int(k), float(epsilon),
                                                             _lib.dptr(D) if D is not None else None, _lib.dptr(Kmat)))
    return D, Kmat


def knn_gaussian_kernel(D, k=64, epsilon=1.0):
    """Kernel matrix of pydiffmap's ``DiffusionMap.from_sklearn(epsilon=, k=)`` from row distances D: exp(-d^2 / (4 eps)) on
    every row's k nearest rows (itself included), 0 elsewhere (pilotpy/plot/ploting.py:109-110)."""
    D = _square(_as_f64(D, "D"), "D")
    Kmat = np.empty_like(D)
    _lib.check(_lib.load().pilot_ot_knn_kernel(_lib.dptr(D), D.shape[0], int(k), float(epsilon), _lib.dptr(Kmat)))
    return Kmat


# ---- diffusion map (pl.trajectory's embedding, pilotpy/plot/ploting.py:95-110) ---------------------------------------------
def _diffmap_check(N, n_evecs, epsilon, alpha):
    """pydiffmap's epsilon may be a bandwidth-selection rule ('bgh', 'bgh_generous'); only a number is implemented.  The numeric
    ranges are the library's (PILOT_OT_EINVAL), checked here too so a host kernel is refused before it is uploaded."""
    if isinstance(epsilon, (str, bytes)) or isinstance(epsilon, bool) or not np.isscalar(epsilon) or not np.isreal(epsilon):
        raise NotImplementedError("epsilon=%r: only a numeric epsilon is implemented (no bandwidth selection)" % (epsilon,))
    epsilon, alpha = float(epsilon), float(alpha)
    if N < 2:
        raise ValueError("a diffusion map needs at least 2 points, got N=%d" % N)
    if not 1 <= int(n_evecs) <= min(N - 1, 64):
        raise ValueError("n_evecs=%d outside [1, min(N - 1, 64)]" % n_evecs)
    if not (epsilon > 0.0 and np.isfinite(epsilon)):
        raise ValueError("epsilon=%g must be positive and finite" % epsilon)
    if not np.isfinite(alpha):
        raise ValueError("alpha=%g must be finite" % alpha)
    return int(n_evecs), epsilon, alpha


def _diffmap_result(dmap, evecs, evals, info, return_info):
    steps, flags = int(info[0]), int(info[1])
    out = dict(steps=steps, flags=flags, converged=not flags & _lib.DIFFMAP_NOT_CONVERGED,
               degenerate=bool(flags & _lib.DIFFMAP_DEGENERATE))
    if return_info:
        return dmap, evecs, evals, out
    if flags & _lib.DIFFMAP_DEGENERATE:
        raise ValueError("diffusion map: eigenvalue 1 of the Markov matrix is repeated (a disconnected neighbour graph)")
    if flags & _lib.DIFFMAP_NOT_CONVERGED:
        raise ValueError("diffusion map: Lanczos did not converge in %d steps" % steps)
    return dmap, evecs, evals


def diffusion_map_of_rows(E, n_evecs=2, epsilon=1.0, alpha=0.5, k=64, return_info=False):
    """pl.trajectory's embedding (pilotpy/plot/ploting.py:95-110) on the device: pydiffmap's
    ``DiffusionMap.from_sklearn(n_evecs, epsilon, alpha, k).fit_transform(E / E.max())`` -- row distances, k-nearest-neighbour
    Gaussian kernel, alpha-normalised Markov matrix, its leading eigenpairs (Lanczos) and the diffusion coordinates.
    E: numpy array or :class:`DeviceMatrix`.  Returns ``(dmap, evecs, evals)``: N x n_evecs, N x n_evecs, n_evecs (eigenvalues
    of (P - I) / epsilon, descending, the trivial 0 dropped).  A repeated eigenvalue 1 (disconnected graph) or no convergence
    raises ValueError; with ``return_info`` nothing is raised and a fourth item, ``dict(steps, flags, converged, degenerate)``,
    tells."""
    E = _matrix_arg(E)
    N = E.rows
    n_evecs, epsilon, alpha = _diffmap_check(N, n_evecs, epsilon, alpha)
    dmap = np.empty((N, n_evecs), dtype=np.float64)
    evecs = np.empty((N, n_evecs), dtype=np.float64)
    evals = np.empty(n_evecs, dtype=np.float64)
    info = np.zeros(2, dtype=np.int32)
    _lib.check(_lib.load().pilot_ot_diffusion_map_of_rows(E.ptr, E.on_dev, N, int(k), epsilon, float(alpha), n_evecs, _lib.dptr(dmap),
                                                          _lib.dptr(evecs), _lib.dptr(evals), _lib.iptr(info)))
    return _diffmap_result(dmap, evecs, evals, info, return_info)


def diffusion_map_from_kernel(Kmat, n_evecs=2, epsilon=1.0, alpha=0.5, return_info=False):
    """The eigen-part of the diffusion map from a non-negative N x N kernel matrix (numpy array or :class:`DeviceMatrix`), e.g.
    :func:`knn_gaussian_kernel`'s: symmetrised max(K, K^T), alpha-normalised, Lanczos on the device.  Same returns as
    :func:`diffusion_map_of_rows`."""
    K = _matrix_arg(Kmat, "Kmat")
    N = K.rows
    n_evecs, epsilon, alpha = _diffmap_check(N, n_evecs, epsilon, alpha)
    info = np.zeros(2, dtype=np.int32)
    bufs = []
    try:
        dK = K.ptr
        if not K.on_dev:
            bufs.append(_DeviceBuffer.holding(K.keep))
            dK = bufs[0].ptr
        out = [_device_result(N, n_evecs), _device_result(N, n_evecs), _device_result(1, n_evecs)]
        bufs += [D.owner for D in out]
        _lib.check(_lib.load().pilot_ot_diffusion_map_dev(dK, N, epsilon, alpha, n_evecs, *(ctypes.c_void_p(D.ptr) for D in out),
                                                          _lib.iptr(info), None))
        dmap, evecs, evals = download(out[0]), download(out[1]), download(out[2])[0]
    finally:
        for buf in bufs:
            buf.free()
    return _diffmap_result(dmap, evecs, evals, info, return_info)


# ---- trajectory model fits (pilotpy's fit_best_model, tools/Cell_gene_selection.py) --------------------------
TRAJFIT_MODELS = ("linear", "linear_quadratic", "quadratic")


def _fit_inputs(Y, x):
    """``Y`` (observations x targets) and the time ``x`` of the model fits as ``(Y, x, n, T)``: the dense argument, float64
    times, and the two sizes."""
    x = _as_f64(np.ravel(x), "x")
    Y = _dense_arg(Y, "Y", mode="strided", axes=" (observations x targets)")
    n, T = Y.rows, Y.cols
    if x.size != n:
        raise ValueError("x has %d values, Y has %d observations" % (x.size, n))
    return Y, x, n, T


def trajectory_fits(Y, x, model="ols", epsilon=1.35, pval_thr=0.05, modify_r2=False, return_info=False):
    """The three trajectory models of every target column of ``Y`` (n observations x targets, float32 / float64, a numpy
    array or a :class:`DeviceMatrix`) against the time ``x`` (n values), on the device: ``linear`` [x], ``linear_quadratic``
    [x, x^2] and ``quadratic`` [x^2], each with an intercept, fitted by OLS (``model="ols"``, LinearRegression) or to the
    optimum of scikit-learn's HuberRegressor objective (``model="huber"``, ``epsilon``, alpha 1e-4), then pilotpy's statistics
    and model choice (include/pilot_ot.h, "trajectory model fits").  Returns a dict of arrays: ``params`` and ``pvalues``
    (targets x 3 models x 3; the third slot NaN for the two-coefficient models), ``rsquared_adj``, ``mod_rsquared_adj``
    (targets x 3), ``chosen`` (index into :data:`TRAJFIT_MODELS`, -1 when no model is eligible), ``slope``, ``pattern``
    (bit 0: params[1] < 0, bit 1: params[2] < 0; -1 with no choice), ``pearson_r``, ``pearson_p``, ``zero_fraction``,
    ``mean``.  With ``return_info`` a second dict: ``sigma``, ``steps``, ``flags`` (targets x 3; Huber scale, Newton steps,
    ``_lib.TRAJFIT_NOT_CONVERGED`` bits) and ``not_converged`` (the flagged count)."""
    if model not in ("ols", "huber"):
        raise ValueError("model=%r must be 'ols' or 'huber'" % (model,))
    Y, x, n, T = _fit_inputs(Y, x)
    fits = dict(params=np.empty((T, 3, 3)), pvalues=np.empty((T, 3, 3)), rsquared_adj=np.empty((T, 3)),
                mod_rsquared_adj=np.empty((T, 3)), chosen=np.empty(T, dtype=np.int32), slope=np.empty(T),
                pattern=np.empty(T, dtype=np.int32), pearson_r=np.empty(T), pearson_p=np.empty(T), zero_fraction=np.empty(T),
                mean=np.empty(T))
    info = dict(sigma=np.empty((T, 3)), steps=np.empty((T, 3), dtype=np.int32), flags=np.empty((T, 3), dtype=np.int32))
    out = _lib.TrajfitOut()
    for name, arr in list(fits.items()) + list(info.items()):
        ct = ctypes.c_int if arr.dtype == np.int32 else ctypes.c_double
        setattr(out, name, arr.ctypes.data_as(ctypes.POINTER(ct)))
    nnc = ctypes.c_int(0)
    _lib.check(_lib.load().pilot_ot_trajectory_fits(
        Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), n, T, Y.ld, _lib.dptr(x),
        _lib.TRAJFIT_HUBER if model == "huber" else _lib.TRAJFIT_OLS, float(epsilon), float(pval_thr), int(bool(modify_r2)),
        ctypes.byref(out), ctypes.byref(nnc)))
    if return_info:
        info["not_converged"] = nnc.value
        return fits, info
    return fits


def bootstrap_huber_fits(Y, x, cols, models, idx, epsilon=1.35, return_info=False):
    """Batched bootstrap Huber fits on the device (K10; include/pilot_ot.h, "bootstrap Huber fits"): problem q fits column
    ``cols[q]`` of ``Y`` (n observations x targets, float32 / float64, a numpy array or a :class:`DeviceMatrix`) with the
    trajectory model ``models[q]`` (an index into :data:`TRAJFIT_MODELS`) B times, fit b regressing that column, in its own
    order, on the resampled times ``x[idx[q, :, b]]`` (``idx``: problems x n x B ints in [0, n), observation-major; only x is
    resampled, as in pilotpy's gene_cluster_differentiation).  Each fit is the optimum of scikit-learn's HuberRegressor objective
    (``epsilon``, alpha 1e-4) by K9's method.  Returns ``params`` (problems x B x 3, on [1, f(x)]; the third slot NaN for the
    two-coefficient models); with ``return_info`` also a dict of ``sigma``, ``steps``, ``flags`` (problems x B) and
    ``not_converged`` (the count flagged ``_lib.TRAJFIT_NOT_CONVERGED``)."""
    Y, x, n, T = _fit_inputs(Y, x)
    cols = np.ascontiguousarray(np.ravel(cols), dtype=np.int32)
    models = np.ascontiguousarray(np.ravel(models), dtype=np.int32)
    idx = np.asarray(idx)
    if idx.ndim != 3 or idx.shape[0] != cols.size or idx.shape[1] != n:
        raise ValueError("idx must be problems x n x B = %d x %d x B, got %s" % (cols.size, n, idx.shape))
    if models.size != cols.size:
        raise ValueError("models has %d entries for %d problems" % (models.size, cols.size))
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    P, B = cols.size, idx.shape[2]
    params = np.empty((P, B, 3))
    info = dict(sigma=np.empty((P, B)), steps=np.empty((P, B), dtype=np.int32), flags=np.empty((P, B), dtype=np.int32))
    nnc = ctypes.c_int(0)
    _lib.check(_lib.load().pilot_ot_bootstrap_huber_fits(
        Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), n, T, Y.ld, _lib.dptr(x), P, _lib.iptr(cols), _lib.iptr(models), B,
        _lib.iptr(idx), float(epsilon), _lib.dptr(params), _lib.dptr(info["sigma"]), _lib.iptr(info["steps"]),
        _lib.iptr(info["flags"]), ctypes.byref(nnc)))
    if return_info:
        info["not_converged"] = nnc.value
        return params, info
    return params


# ---- gene curve clustering (K11; pilotpy's genes_selection_analysis, plot/gene_selection_analysis.py) ------------------------
LINKAGE_METHODS = tuple(_lib.LINKAGE_METHODS)
_LINKAGE_UNSUPPORTED = ("centroid", "median", "ward")


def _device_result(rows, cols):
    buf = _DeviceBuffer(rows * cols * 8)
    return DeviceMatrix(buf.ptr, rows, owner=buf, shape=(rows, cols), dtype=np.float64)


def _result_matrix(rows, cols, on_device):
    """a rows x cols float64 result for a call that writes either to the host or into HBM: ``(numpy array or DeviceMatrix, the
    pointer the call is given)``"""
    out = _device_result(rows, cols) if on_device else np.empty((rows, cols), dtype=np.float64)
    return out, ctypes.c_void_p(out.ptr if on_device else out.ctypes.data)


def download(D):
    """The contents of a :class:`DeviceMatrix` as a numpy array."""
    out = np.empty(D.shape, dtype=D.dtype)
    if out.size:
        _lib.check(_lib.load().pilot_ot_memcpy_d2h(out.ctypes.data, ctypes.c_void_p(D.ptr), out.nbytes))
    return out


def segment_std(Y, offsets, cols=None, device=False):
    """K11a: the sample standard deviation (ddof 1, what pandas' ``groupby(...).std()`` gives) of every selected column of ``Y``
    (rows x columns, float32 / float64, numpy array or :class:`DeviceMatrix`) over each contiguous row segment
    ``offsets[s]:offsets[s + 1]``.  Returns segments x columns float64 (a :class:`DeviceMatrix` with ``device=True``); a segment
    of one row gives NaN.  Two passes in f64 (mean, then squared deviations), sums in a fixed order."""
    Y = _dense_arg(Y, "Y")
    n_cols = Y.cols
    offsets = np.ascontiguousarray(np.ravel(offsets), dtype=np.int64)
    if offsets.size < 1:
        raise ValueError("offsets needs at least one entry")
    S = offsets.size - 1
    if cols is not None:
        cols = np.ascontiguousarray(np.ravel(cols), dtype=np.int32)
    n_sel = n_cols if cols is None else cols.size
    out, out_ptr = _result_matrix(S, n_sel, device)
    _lib.check(_lib.load().pilot_ot_segment_std(
        Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, n_cols, Y.ld, _lib.lptr(offsets), S,
        None if cols is None else _lib.iptr(cols), n_sel, out_ptr, int(device)))
    return out


# ---- group moments (K12; what pilotpy's patient sub-group workflow needs of a cells x genes matrix) ---------------------------
GROUP_MOMENTS_MAX_GROUPS = 8
_GM_TRANSFORMS = {None: 0, "expm1": 1}


class _DeviceColumns:
    """Columns ``start:stop`` of a 2-D :class:`DeviceMatrix`, in place: the same rows with the parent's leading dimension.  Only
    :func:`group_moments` reads one (made by :func:`device_columns`)."""

    def __init__(self, parent, start, stop):
        if len(parent.shape) != 2 or not 0 <= start < stop <= parent.shape[1]:
            raise ValueError("columns %d:%d of a DeviceMatrix of shape %s" % (start, stop, parent.shape))
        self.parent, self.ld = parent, parent.shape[1]
        self.ptr = parent.ptr + int(start) * parent.dtype.itemsize
        self.shape, self.dtype = (parent.shape[0], int(stop - start)), parent.dtype


def device_columns(D, start, stop):
    """A view of the columns ``start:stop`` of the :class:`DeviceMatrix` D for :func:`group_moments` (no copy; the leading
    dimension stays D's)."""
    return _DeviceColumns(D, int(start), int(stop))


def _moment_args(n, n_total, codes, n_groups, transform, cols, max_groups=GROUP_MOMENTS_MAX_GROUPS):
    """group_moments' and group_sums' arguments checked on the host: (codes int32, n_groups, cols int32 or None)"""
    if transform not in _GM_TRANSFORMS:
        raise ValueError("transform=%r must be None or 'expm1'" % (transform,))
    if isinstance(n_groups, bool) or int(n_groups) != n_groups or not 1 <= n_groups <= max_groups:
        raise ValueError("n_groups=%r must be an integer in 1..%d" % (n_groups, max_groups))
    n_groups = int(n_groups)
    if n_total < 1:
        raise ValueError("Y has no columns")
    codes = np.asarray(codes)
    if codes.ndim != 1 or codes.size != n:
        raise ValueError("codes has shape %s for %d rows" % (codes.shape, n))
    if codes.dtype.kind not in "iu":
        raise ValueError("codes must be integers, got %s" % codes.dtype)
    if n and int(codes.max()) >= n_groups:
        raise ValueError("codes reach %d with n_groups=%d" % (int(codes.max()), n_groups))
    codes = np.ascontiguousarray(np.maximum(codes, -1), dtype=np.int32)
    if cols is not None:
        cols = np.asarray(cols)
        if cols.ndim != 1 or cols.dtype.kind not in "iu":
            raise ValueError("cols: a 1-D array of column indices, got %s %s" % (cols.shape, cols.dtype))
        if cols.size and (int(cols.min()) < 0 or int(cols.max()) >= n_total):
            raise ValueError("cols outside [0, %d)" % n_total)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
    return codes, n_groups, cols


class DeviceCSR(_Closing):
    """K13: a sparse rows x columns matrix resident in HBM as CSR (include/pilot_ot.h, "sparse matrices"): what ``adata.X`` is in
    real scRNA-seq data.  Made by :meth:`upload`; the dense matrix is never formed unless :meth:`densify` is asked for some
    columns.  ``shape``, ``dtype`` (float32 / float64) and ``nnz`` (stored entries) describe it.  The column-major copy the
    per-column calls read is built on the device by the first of them and dropped by :meth:`normalize_log1p`."""

    def __init__(self, handle, shape, dtype, nnz):
        self.h, self.shape, self.dtype, self.nnz = handle, tuple(int(v) for v in shape), np.dtype(dtype), int(nnz)

    @classmethod
    def upload(cls, X, rows=None):
        """``X``: a scipy CSR matrix or array (anything else: ValueError); ``rows``: an optional row selection, taken on the host
        (``X[rows]``).  Integer and bool data become float32.  Duplicate entries are summed in a copy, the caller's matrix is never
        modified; indices within a row may come unsorted."""
        import scipy.sparse as sp
        if not sp.issparse(X) or X.format != "csr":
            raise ValueError("DeviceCSR.upload: a scipy CSR matrix or array, got %s" % type(X).__name__)
        if rows is not None:
            X = X[np.asarray(rows)]
        if X.ndim != 2 or X.shape[1] < 1:
            raise ValueError("DeviceCSR.upload: a 2-D matrix with at least one column, got shape %s" % (X.shape,))
        if X.shape[0] >= 2 ** 31 or X.shape[1] >= 2 ** 31:
            raise ValueError("DeviceCSR.upload: shape %s needs more than 32-bit row / column indices" % (X.shape,))
        if not X.has_canonical_format:           # unsorted rows go up as they are; duplicates are summed, in a copy
            summed = X.copy()
            summed.sum_duplicates()
            if summed.nnz != X.nnz:
                X = summed
        data = X.data
        if data.dtype not in (np.float32, np.float64):
            if data.dtype.kind not in "biuf":
                raise ValueError("DeviceCSR.upload: numeric data, got %s" % data.dtype)
            data = data.astype(np.float32)
        data = np.ascontiguousarray(data)
        indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(X.indices, dtype=np.int32)
        h = ctypes.c_void_p()
        _lib.check(_lib.load().pilot_ot_csr_upload(
            _lib.lptr(indptr), _lib.iptr(indices), ctypes.c_void_p(data.ctypes.data), _lib.dtype_code(data.dtype), X.shape[0], X.shape[1],
            ctypes.byref(h)))
        return cls(h, X.shape, data.dtype, indices.size)

    def _handle(self):
        if not self.h:
            raise ValueError("the DeviceCSR was closed")
        return self.h

    def normalize_log1p(self, target_sum=1e4):
        """In place: scanpy's ``normalize_total(target_sum)`` then ``log1p`` on the stored values (zeros stay implicit), with the
        expressions of the dense ``pilot_ot_normalize_log1p``: counts give the same bits by either route."""
        if not (float(target_sum) > 0.0 and np.isfinite(target_sum)):
            raise ValueError("target_sum=%r must be positive" % (target_sum,))
        _lib.check(_lib.load().pilot_ot_csr_normalize_log1p(self._handle(), float(target_sum)))
        return self

    def build_columns(self):
        """Build the column-major copy now (the per-column calls build it on first use)."""
        _lib.check(_lib.load().pilot_ot_csr_build_columns(self._handle()))

    def column_nnz(self):
        """int64 per column: the stored values that are != 0 (``(dense != 0).sum(0)``)."""
        out = np.empty(self.shape[1], dtype=np.int64)
        _lib.check(_lib.load().pilot_ot_csr_column_nnz(self._handle(), _lib.lptr(out)))
        return out

    def group_moments(self, codes, n_groups, transform=None, cols=None):
        """:func:`group_moments` of the matrix, read from the column form: ``(count, mean, m2)``."""
        codes, n_groups, cols = _moment_args(self.shape[0], self.shape[1], codes, n_groups, transform, cols)
        n_sel = self.shape[1] if cols is None else cols.size
        count = np.empty(n_groups, dtype=np.int64)
        mean, m2 = np.empty((n_groups, n_sel)), np.empty((n_groups, n_sel))
        _lib.check(_lib.load().pilot_ot_csr_group_moments(
            self._handle(), _lib.iptr(codes), n_groups, None if cols is None else _lib.iptr(cols), n_sel, _GM_TRANSFORMS[transform],
            _lib.lptr(count), _lib.dptr(mean), _lib.dptr(m2)))
        return count, mean, m2

    def group_sums(self, codes, n_groups, cols=None):
        """:func:`group_sums` of the matrix, read from the row form (the column form is not needed and not built, so this also
        follows :meth:`normalize_log1p` at no extra cost): ``(count, sums)``."""
        codes, n_groups, cols = _moment_args(self.shape[0], self.shape[1], codes, n_groups, None, cols, GROUP_SUMS_MAX_GROUPS)
        n_sel = self.shape[1] if cols is None else cols.size
        count, sums = np.empty(n_groups, dtype=np.int64), np.empty((n_groups, n_sel))
        _lib.check(_lib.load().pilot_ot_csr_group_sums(
            self._handle(), _lib.iptr(codes), n_groups, None if cols is None else _lib.iptr(cols), n_sel, _lib.lptr(count), _lib.dptr(sums)))
        return count, sums

    def rank_sums(self, codes, n_groups, cols=None):
        """:func:`rank_sums` of the matrix, read from the column form: only a column's stored non-zero entries are sorted, the
        zeros (implicit or stored) are one run.  ``(count, rank_sums, ties)``."""
        codes, n_groups, cols, n_sel = _rank_sums_args(self.shape[0], self.shape[1], codes, n_groups, cols)
        return _rank_sums_call("pilot_ot_csr_rank_sums", (self._handle(),), codes, n_groups, cols, n_sel)

    def densify(self, cols=None):
        """A rows x len(cols) :class:`DeviceMatrix` of the matrix's dtype holding the columns ``cols`` (distinct, any order;
        default: all), dense in HBM."""
        if cols is not None:
            cols = np.asarray(cols)
            if cols.ndim != 1 or (cols.size and cols.dtype.kind not in "iu"):
                raise ValueError("cols: a 1-D array of column indices, got %s %s" % (cols.shape, cols.dtype))
            if cols.size and (int(cols.min()) < 0 or int(cols.max()) >= self.shape[1]):
                raise ValueError("cols outside [0, %d)" % self.shape[1])
            if np.unique(cols).size != cols.size:
                raise ValueError("cols names a column twice")
            cols = np.ascontiguousarray(cols, dtype=np.int32)
        n, n_sel = self.shape[0], self.shape[1] if cols is None else cols.size
        h = self._handle()
        buf = _DeviceBuffer(n * n_sel * self.dtype.itemsize)
        _lib.check(_lib.load().pilot_ot_csr_densify(h, None if cols is None else _lib.iptr(cols), n_sel, buf.ptr))
        return DeviceMatrix(buf.ptr, n, owner=buf, shape=(n, n_sel), dtype=self.dtype)

    def pca(self, n_comps=50, scale=True, max_value=10.0, cols=None, return_info=False):
        """:func:`pca` of the matrix: the forward product reads the row form, the transposed one the column form."""
        n, n_total = self.shape
        k, scale, max_value, cols, n_sel = _pca_args(n, n_total, n_comps, scale, max_value, cols)
        out = _pca_outputs(n, n_sel, k)
        _lib.check(_lib.load().pilot_ot_csr_pca(self._handle(), None if cols is None else _lib.iptr(cols), n_sel, scale, max_value, k,
                                                *(_lib.dptr(a) for a in out[:4]), _lib.iptr(out[4])))
        return _pca_result(out, return_info)

    def close(self):
        if self.h:
            _lib.load().pilot_ot_csr_destroy(self.h)
            self.h = ctypes.c_void_p()


def csr_slice_rows():
    """Rows per slice of :class:`DeviceCSR`'s column-form build."""
    return int(_lib.load().pilot_ot_csr_slice_rows())


def group_moments(Y, codes, n_groups, transform=None, cols=None):
    """K12: per group and selected column, the count, the float64 mean and the centred sum of squares ``sum (t(y) - mean)^2`` of
    the rows of ``Y`` with ``codes == g`` (include/pilot_ot.h, "group moments").  ``Y``: rows x columns, a C-contiguous float32 /
    float64 numpy array, a :class:`DeviceMatrix` (one upload can serve several calls) or :func:`device_columns` of one.
    ``codes``: one int per row, ``0 .. n_groups - 1`` or negative for a row to skip; ``n_groups`` in 1..8.  ``transform``: None or
    ``"expm1"`` (taken in float64).  ``cols``: the selected columns in any order (default: all).  Returns ``(count, mean, m2)``:
    ``n_groups`` int64 and two ``n_groups x columns`` float64 arrays; an empty group gives 0 and NaN, a group of one row m2 = 0.
    One pass over Y; sums in a fixed order, so a repeated call and the host and device routes return the same bits.  Every
    argument is checked before any device work (ValueError).  A :class:`DeviceCSR` is forwarded to its own method."""
    if isinstance(Y, DeviceCSR):
        return Y.group_moments(codes, n_groups, transform=transform, cols=cols)
    Y = _dense_arg(Y, "Y", mode="strict")
    n_total = Y.cols
    codes, n_groups, cols = _moment_args(Y.rows, n_total, codes, n_groups, transform, cols)
    n_sel = n_total if cols is None else cols.size
    count = np.empty(n_groups, dtype=np.int64)
    mean, m2 = np.empty((n_groups, n_sel)), np.empty((n_groups, n_sel))
    _lib.check(_lib.load().pilot_ot_group_moments(
        Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, n_total, Y.ld, _lib.iptr(codes), n_groups,
        None if cols is None else _lib.iptr(cols), n_sel, _GM_TRANSFORMS[transform], _lib.lptr(count), _lib.dptr(mean), _lib.dptr(m2)))
    return count, mean, m2


# ---- group sums (K14; the pseudobulk counts of pilotpy's get_pseudobulk_DE) ----------------------------------------------------
GROUP_SUMS_MAX_GROUPS = 2 ** 20


def group_sums_slice_rows():
    """Rows per slice of :func:`group_sums`: a group's rows are added in ascending order within slices of this many, the slices
    in order."""
    return int(_lib.load().pilot_ot_group_sums_slice_rows())


def group_sums_col_block():
    """Selected columns per wave of :meth:`DeviceCSR.group_sums` (its float64 accumulators in LDS)."""
    return int(_lib.load().pilot_ot_group_sums_col_block())


def group_sums(Y, codes, n_groups, cols=None):
    """K14: per group and selected column, the float64 sum of the rows of ``Y`` with ``codes == g``, and the number of such rows
    (include/pilot_ot.h, "group sums").  ``Y``, ``codes`` and ``cols`` are :func:`group_moments`'s; ``n_groups`` in 1..2^20.
    Returns ``(count, sums)``: ``n_groups`` int64 and an ``n_groups x columns`` float64 array.  A row with a negative code enters
    nothing, whatever it holds; a group without rows gives count 0 and sums 0.0.  One pass over the used rows, added in an order
    that depends on ``codes`` alone: a repeated call and the host and device routes return the same bits.  Every argument is
    checked before any device work (ValueError).  A :class:`DeviceCSR` is forwarded to its own method."""
    if isinstance(Y, DeviceCSR):
        return Y.group_sums(codes, n_groups, cols=cols)
    Y = _dense_arg(Y, "Y", mode="strict")
    n_total = Y.cols
    codes, n_groups, cols = _moment_args(Y.rows, n_total, codes, n_groups, None, cols, GROUP_SUMS_MAX_GROUPS)
    n_sel = n_total if cols is None else cols.size
    count, sums = np.empty(n_groups, dtype=np.int64), np.empty((n_groups, n_sel))
    _lib.check(_lib.load().pilot_ot_group_sums(
        Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, n_total, Y.ld, _lib.iptr(codes), n_groups,
        None if cols is None else _lib.iptr(cols), n_sel, _lib.lptr(count), _lib.dptr(sums)))
    return count, sums


# ---- rank sums (K21; the Wilcoxon rank-sum test of scanpy's rank_genes_groups and the Kruskal-Wallis test) ---------------------
RANK_SUMS_MAX_GROUPS = 1024
RANK_SUMS_MAX_ROWS = 2 ** 21 - 1


def rank_sums_limits():
    """``(wave_max, wg_max, sort_tile)`` of :func:`rank_sums`: a column with at most ``wave_max`` non-zero used entries is ranked
    by one wave, up to ``wg_max`` by one workgroup in LDS, a longer one in HBM through LDS tiles of ``sort_tile`` records."""
    L = _lib.load()
    return int(L.pilot_ot_rank_sums_wave_max()), int(L.pilot_ot_rank_sums_wg_max()), int(L.pilot_ot_rank_sums_sort_tile())


def _rank_sums_args(n, n_total, codes, n_groups, cols):
    """rank_sums' arguments checked on the host: (codes int32, n_groups, cols int32 or None, selected columns)"""
    codes, n_groups, cols = _moment_args(n, n_total, codes, n_groups, None, cols, RANK_SUMS_MAX_GROUPS)
    used = int(np.count_nonzero(codes >= 0))
    if used > RANK_SUMS_MAX_ROWS:
        raise NotImplementedError("rank_sums: %d used rows; the tie term t^3 - t is exact up to %d" % (used, RANK_SUMS_MAX_ROWS))
    return codes, n_groups, cols, n_total if cols is None else cols.size


def _rank_sums_call(symbol, head, codes, n_groups, cols, n_sel):
    count, ties = np.empty(n_groups, dtype=np.int64), np.empty(n_sel, dtype=np.int64)
    rank2 = np.empty((n_groups, n_sel), dtype=np.int64)
    bad_row, bad_col = ctypes.c_longlong(-1), ctypes.c_int(-1)
    _lib.check(getattr(_lib.load(), symbol)(
        *head, _lib.iptr(codes), n_groups, None if cols is None else _lib.iptr(cols), n_sel, _lib.lptr(count), _lib.lptr(rank2),
        _lib.lptr(ties), ctypes.byref(bad_row), ctypes.byref(bad_col)))
    return count, rank2 * 0.5, ties


def rank_sums(Y, codes, n_groups, cols=None):
    """K21: per selected column of ``Y``, the ranks of the used rows (``codes >= 0``; N of them) summed per group
    (include/pilot_ot.h, "rank sums").  ``Y``, ``codes`` and ``cols`` are :func:`group_moments`'s; ``n_groups`` in 1..1024.  Within
    a column equal values share the mean of their positions (``scipy.stats.rankdata(method="average")``); ``-0.0 == 0.0``, and in
    a :class:`DeviceCSR` a stored zero ties with the implicit ones.  Returns ``(count, rank_sums, ties)``: ``n_groups`` int64, an
    ``n_groups x columns`` float64 array of exact multiples of 1/2, and per column the int64 ``sum(t^3 - t)`` over its runs of
    equal values.  The device works in integers alone, so the dense route, the sparse route and a repeated call return the same
    arrays.  More than 2^21 - 1 used rows: NotImplementedError; a NaN or infinity in a used row of a selected column: ValueError
    naming the first one; every other argument is checked before any device work (ValueError).  :func:`rank_sum_z` and
    :func:`kruskal_h` turn the result into test statistics."""
    if isinstance(Y, DeviceCSR):
        return Y.rank_sums(codes, n_groups, cols=cols)
    Y = _dense_arg(Y, "Y", mode="strict")
    codes, n_groups, cols, n_sel = _rank_sums_args(Y.rows, Y.cols, codes, n_groups, cols)
    return _rank_sums_call("pilot_ot_rank_sums", (Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, Y.cols, Y.ld), codes, n_groups, cols,
                           n_sel)


def _rank_results(count, rank_sums, ties):
    count = np.asarray(count, dtype=np.float64)
    R, ties = np.asarray(rank_sums, dtype=np.float64), np.asarray(ties, dtype=np.float64)
    if count.ndim != 1 or R.ndim != 2 or R.shape[0] != count.size or ties.shape != R.shape[1:]:
        raise ValueError("count %s, rank_sums %s and ties %s are not one rank_sums result" % (count.shape, R.shape, ties.shape))
    return count, R, ties, float(count.sum())


def rank_sum_z(count, rank_sums, ties, tie_correct=False):
    """The Wilcoxon rank-sum (Mann-Whitney) statistics of every group against the other used rows, from :func:`rank_sums`'s
    result; pure numpy.  ``z = (R_g - n_g (N + 1) / 2) / sqrt(n_g (N - n_g) / 12 * ((N + 1) - c ties / (N (N - 1))))`` with
    c = 1 for ``tie_correct`` and 0 without, and ``U = R_g - n_g (n_g + 1) / 2``; the two-sided p-value is
    ``2 * scipy.stats.norm.sf(abs(z))``.  With the correction these are the values of
    ``scipy.stats.mannwhitneyu(use_continuity=False, method="asymptotic")``.  Where the variance is zero (an all-equal column, an
    empty group, a group holding every row) z = 0.  Returns ``(z, U)``, both ``n_groups x columns``."""
    count, R, ties, N = _rank_results(count, rank_sums, ties)
    n = count[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        spread = (N + 1) - (ties / (N * (N - 1)) if tie_correct else 0.0)
        z = (R - n * (N + 1) / 2) / np.sqrt(n * (N - n) / 12 * spread)
    z[~np.isfinite(z)] = 0.0
    return z, R - n * (n + 1) / 2


def kruskal_h(count, rank_sums, ties):
    """The Kruskal-Wallis test over the groups that have rows, from :func:`rank_sums`'s result; numpy and scipy.
    ``H = (12 / (N (N + 1)) * sum_g R_g^2 / n_g - 3 (N + 1)) / (1 - ties / (N^3 - N))``, ``p = chi2.sf(H, df)``, ``df`` = those
    groups - 1: the values of ``scipy.stats.kruskal``.  An all-equal column gives H = p = NaN, as scipy does.  Returns
    ``(H, p, df)``."""
    from scipy import stats
    count, R, ties, N = _rank_results(count, rank_sums, ties)
    ssbn = np.zeros(R.shape[1])
    for g in np.flatnonzero(count > 0):
        ssbn += R[g] ** 2 / count[g]
    df = int(np.count_nonzero(count > 0)) - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        correction = 1.0 - ties / (N ** 3 - N)
        H = (12.0 / (N * (N + 1)) * ssbn - 3 * (N + 1)) / correction
    H[correction == 0] = np.nan
    return H, stats.chi2.sf(H, df), df


# ---- PERMANOVA (K29; Anderson 2001, vegan's adonis2 with marginal terms: DESIGN.md K29) ------------------------------------------
PERMANOVA_EPS = float(np.sqrt(2.0 ** -52))
PERMANOVA_RANK_TOL = 1e-10


def permanova_limits():
    """``(max_n, chunk, tile_cols, row_block)`` of :func:`permanova_ss`: the most samples the LDS sort of the permutation kernel
    takes, the permutations one pass processes (fewer when ``65536 / columns`` is fewer; the test switch
    ``PILOT_OT_PERMANOVA_CHUNK`` lowers it), the columns a workgroup of the quadratic-form kernel owns and the rows of A it reads."""
    v = [ctypes.c_int(0) for _ in range(4)]
    _lib.check(_lib.load().pilot_ot_permanova_limits(*[ctypes.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def permanova_basis(X):
    """The model terms of :func:`permanova_ss` from variables: ``X`` maps a name to one value per sample (a dict, a pandas
    DataFrame, or a list of arrays named "0", "1", ...).  A variable of a numeric or boolean dtype is itself; any other is
    categorical and becomes the indicators of all its levels but the first, the levels being ``sorted`` as Python strings.
    Every term is centred and replaced by the Q of its thin QR (numpy); a column whose R diagonal is below ``1e-10 max |R_ii|``
    is dropped.  A term with no variation (``max |R_ii| <= 1e-10`` times the norm of its uncentred columns: one level, a constant)
    has rank 0 and raises ValueError naming it, as does a missing or non-finite value.  Returns ``(Q, terms)``: ``n x c`` float64
    and the ``len(X) + 1`` int32 column offsets of the terms."""
    if hasattr(X, "columns") and hasattr(X, "__getitem__") and not isinstance(X, dict):
        X = {str(c): np.asarray(X[c]) for c in X.columns}
    elif not isinstance(X, dict):
        X = {str(i): np.asarray(v) for i, v in enumerate(X)}
    if not X:
        raise ValueError("permanova_basis: no variable")
    blocks, terms, n = [], [0], None
    for name, values in X.items():
        v = np.asarray(values)
        if v.ndim != 1 or (n is not None and v.shape[0] != n) or v.shape[0] < 1:
            raise ValueError("permanova_basis: %r must hold one value per sample, got shape %s" % (name, v.shape))
        n = v.shape[0]
        if v.dtype.kind in "biuf":
            M = v.astype(np.float64).reshape(n, 1)
            if not np.all(np.isfinite(M)):
                raise ValueError("permanova_basis: %r has a missing or non-finite value" % (name,))
        else:
            if any(x is None or (isinstance(x, float) and x != x) for x in v.tolist()):
                raise ValueError("permanova_basis: %r has a missing value" % (name,))
            labels = np.array([str(x) for x in v.tolist()], dtype=object)
            levels = sorted(set(labels.tolist()))
            M = np.stack([(labels == lev).astype(np.float64) for lev in levels[1:]], axis=1) if len(levels) > 1 else np.zeros((n, 0))
        scale = float(np.sqrt((M * M).sum()))
        Mc = M - M.mean(axis=0, keepdims=True) if M.shape[1] else M
        Qt, R = np.linalg.qr(Mc) if M.shape[1] else (Mc, np.zeros((0, 0)))
        d = np.abs(np.diag(R))
        if d.size == 0 or not d.max() > PERMANOVA_RANK_TOL * scale:
            raise ValueError("permanova_basis: term %r has rank 0 (a single level or a constant)" % (name,))
        Qt = Qt[:, d >= PERMANOVA_RANK_TOL * d.max()]
        blocks.append(Qt)
        terms.append(terms[-1] + Qt.shape[1])
    return np.ascontiguousarray(np.concatenate(blocks, axis=1)), np.asarray(terms, dtype=np.int32)


def _permanova_window(n_perm, seed, start):
    n_perm, seed, start = int(n_perm), int(seed), int(start)
    if n_perm < 0:
        raise ValueError("n_perm=%d permutations" % n_perm)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed=%d must be in [0, 2^64)" % seed)
    if not 0 <= start <= n_perm:
        raise ValueError("start=%d must be in [0, n_perm=%d]" % (start, n_perm))
    return n_perm, seed, start


def _permanova_samples(n, strata, who):
    n = int(n)
    if n < 1:
        raise ValueError("%s: n=%d samples" % (who, n))
    max_n = permanova_limits()[0]
    if n > max_n:
        raise ValueError("%s: n=%d samples do not fit the LDS sort of the permutation kernel (at most %d)" % (who, n, max_n))
    if strata is None:
        return n, None
    codes, _ = _label_codes(strata, n)
    return n, codes


def permanova_permutations(n, n_perm, seed=0, strata=None, start=0):
    """K29's permutations ``start .. n_perm`` of ``n`` samples, generated on the device: an ``(n_perm + 1 - start) x n`` int32
    array whose row ``b - start`` is the permutation ``p`` with ``Z_b[i, :] = Q[p[i], :]``.  Permutation 0 is the identity; for
    b >= 1 the rows are ordered by ``(stratum, Philox4x32-10 key, index)`` and dealt to the rows ordered by ``(stratum, index)``
    (DESIGN.md K29), so a permutation is uniform within ``strata`` (one label per sample; None: one stratum) and a function of
    ``(seed, b, n, strata)`` alone.  ValueError before any device work: n outside 1 .. ``permanova_limits()[0]``, a negative seed
    or one beyond 2^64 - 1, ``start`` outside ``[0, n_perm]``, strata of another length."""
    n_perm, seed, start = _permanova_window(n_perm, seed, start)
    n, codes = _permanova_samples(n, strata, "permanova_permutations")
    out = np.empty((n_perm + 1 - start, n), dtype=np.int32)
    _lib.check(_lib.load().pilot_ot_permanova_permutations(n, None if codes is None else _lib.iptr(codes), seed, start, out.shape[0],
                                                           _lib.iptr(out)))
    return out


def permanova_ss(D, Q, terms, n_perm, seed=0, rows=None, strata=None, start=0, return_times=False):
    """K29: the sums of squares of PERMANOVA's model terms under permutations ``start .. n_perm`` (0 is the observed design).
    ``D``: an N x N float32 / float64 numpy array or :class:`DeviceMatrix` of dissimilarities; ``rows``: the ascending indices
    of the n samples used (None: all).  ``s_ij = (D_ij + D_ji) / 2``, ``s_ii = 0``, ``A_ij = -0.5 s_ij s_ij`` in float64.
    ``Q`` (n x c float64) and ``terms`` (offsets) are :func:`permanova_basis`'s: centred columns, orthonormal within a term.
    Returns ``(ss_total, ss)``: ``-(1/n) sum_ij A_ij`` and the ``(n_perm + 1 - start) x terms`` array ``ss[b - start, t] = sum
    over the term's columns of Z_b[:, c]^T A Z_b[:, c]`` with :func:`permanova_permutations`' ``Z_b``.  Permutation b's values
    have the same bits alone, in any batch, at any ``start`` and under any chunking.  ``return_times=True`` adds a dict of the
    device milliseconds of the ``prepare``, ``permute`` and ``quadratic`` kernels.
    ValueError before any device work: D not square, rows not ascending inside it, more than ``permanova_limits()[0]`` samples, Q
    not n x c float64, terms not strictly ascending offsets from 0 to c, a column of Q that is not centred, a bad seed or
    ``start``, strata of another length.  ValueError naming the entry: a NaN or infinity between two used samples."""
    n_perm, seed, start = _permanova_window(n_perm, seed, start)
    Dm = _dense_arg(D, "D", mode="strided")
    if Dm.rows != Dm.cols:
        raise ValueError("D must be samples x samples, got %d x %d" % (Dm.rows, Dm.cols))
    if rows is not None:
        rows = np.ascontiguousarray(rows)
        if rows.ndim != 1 or rows.dtype.kind not in "iu" or rows.size < 1:
            raise ValueError("rows: a 1-D array of at least one integer index, got %s %s" % (rows.shape, rows.dtype))
        if rows.min() < 0 or rows.max() >= Dm.rows or np.any(np.diff(rows.astype(np.int64)) <= 0):
            raise ValueError("rows must be ascending indices inside [0, %d)" % Dm.rows)
        rows = rows.astype(np.int32)
    n, codes = _permanova_samples(Dm.rows if rows is None else rows.size, strata, "permanova_ss")
    if not isinstance(Q, np.ndarray) or Q.ndim != 2 or Q.dtype != np.float64 or Q.shape[0] != n or Q.shape[1] < 1:
        raise ValueError("Q: an n x c float64 array with n=%d rows, got %s %s" % (n, getattr(Q, "shape", type(Q).__name__),
                                                                                  getattr(Q, "dtype", "")))
    Q = np.ascontiguousarray(Q)
    terms = np.ascontiguousarray(terms, dtype=np.int32)
    c = Q.shape[1]
    if terms.ndim != 1 or terms.size < 2 or terms[0] != 0 or terms[-1] != c or np.any(np.diff(terms) <= 0):
        raise ValueError("terms: strictly ascending column offsets from 0 to c=%d, got %s" % (c, terms.tolist()))
    if not np.all(np.isfinite(Q)):
        raise ValueError("Q has a NaN or an infinity")
    off = np.abs(Q.sum(axis=0)) > 1e-8 * (1.0 + np.abs(Q).sum(axis=0))
    if off.any():
        raise ValueError("column %d of Q is not centred (sum %g): permanova_basis centres the terms" % (int(np.flatnonzero(off)[0]),
                                                                                                       Q.sum(axis=0)[off][0]))
    n_terms, count = terms.size - 1, n_perm + 1 - start
    ss_total = ctypes.c_double(0.0)
    ss = np.empty((count, n_terms), dtype=np.float64)
    bad_row, bad_col = ctypes.c_longlong(-1), ctypes.c_longlong(-1)
    ms = (ctypes.c_float * 3)()
    _lib.check(_lib.load().pilot_ot_permanova(
        Dm.ptr, Dm.on_dev, _lib.dtype_code(Dm.dtype), Dm.rows, Dm.ld, None if rows is None else _lib.iptr(rows), n, _lib.dptr(Q), c,
        _lib.iptr(terms), n_terms, None if codes is None else _lib.iptr(codes), seed, start, count, ctypes.byref(ss_total), _lib.dptr(ss),
        ctypes.byref(bad_row), ctypes.byref(bad_col), ms if return_times else None))
    if return_times:
        return ss_total.value, ss, dict(zip(("prepare", "permute", "quadratic"), (float(v) for v in ms)))
    return ss_total.value, ss


def permanova_f(ss_total, ss, terms, n):
    """``F[b, t] = (ss / q_t) / ((ss_total - ss) / (n - q_t - 1))`` of :func:`permanova_ss`'s result, ``q_t`` the columns of term t."""
    q = np.diff(np.asarray(terms, dtype=np.int64)).astype(np.float64)
    ss = np.asarray(ss, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (ss / q) / ((float(ss_total) - ss) / (float(n) - q - 1.0))


def permanova_p(F):
    """``p_t = (1 + #{b >= 1: F[b, t] >= F[0, t] - EPS}) / (1 + n_perm)`` with ``EPS = sqrt(2^-52)``, every term against the same
    permutations; ``F`` from :func:`permanova_f` of a run with ``start=0``."""
    F = np.asarray(F, dtype=np.float64)
    return (1.0 + np.count_nonzero(F[1:] >= F[0] - PERMANOVA_EPS, axis=0)) / float(F.shape[0])


# ---- negative-binomial GLM (K22; DESeq2's model for the one-factor design of pilotpy's compute_pseudobulk_DE) ------------------
NB_MIN_DISP = 1e-8
NB_MIN_MU = 0.5


def nb_max_disp(m):
    """``maxDisp = max(10, m)`` of m samples"""
    return float(max(10, int(m)))


def nb_clip(disp, m):
    """``disp`` clipped to [minDisp, maxDisp]: the end points of :func:`nb_dispersions`' grid are the logs of the bounds, which
    ``exp`` returns to within an ulp.  NaN stays."""
    return np.clip(disp, NB_MIN_DISP, nb_max_disp(m))


def nb_glm_limits():
    """The most samples :func:`nb_dispersions` takes: a gene's counts and fitted means are staged in LDS."""
    return int(_lib.load().pilot_ot_nb_glm_max_samples())


def _nb_blind_args(m, n_genes, size_factors, groups=None):
    """the samples of an NB call checked on the host: the size factors as float64.  ``groups``: what a grouped call checks of its
    own, between the shape and the size factors (which refusal comes first is behaviour)"""
    if n_genes < 1:
        raise ValueError("counts has no columns")
    if m < 2:
        raise ValueError("counts has %d rows: at least 2 samples" % m)
    if groups is not None:
        groups()
    sf = np.ascontiguousarray(size_factors, dtype=np.float64)
    if sf.shape != (m,):
        raise ValueError("size_factors has shape %s for %d samples" % (sf.shape, m))
    if not (np.isfinite(sf).all() and (sf > 0).all()):
        raise ValueError("size_factors must be positive and finite")
    return sf


def _nb_args(m, n_genes, codes, n_groups, size_factors):
    """the design arguments of the grouped NB calls checked on the host: (codes int32, n_groups, size factors float64)"""
    if isinstance(n_groups, bool) or int(n_groups) != n_groups:
        raise ValueError("n_groups=%r must be an integer" % (n_groups,))
    n_groups = int(n_groups)

    def groups():
        if not 2 <= n_groups <= m - 1:
            raise ValueError("n_groups=%d must be in [2, m - 1 = %d]: a residual degree of freedom is needed" % (n_groups, m - 1))
        c = np.asarray(codes)
        if c.ndim != 1 or c.size != m:
            raise ValueError("codes has shape %s for %d samples" % (c.shape, m))
        if c.dtype.kind not in "iu":
            raise ValueError("codes must be integers, got %s" % c.dtype)
        if int(c.min()) < 0 or int(c.max()) >= n_groups:
            raise ValueError("codes outside [0, %d)" % n_groups)
        count = np.bincount(c, minlength=n_groups)
        if (count == 0).any():
            raise ValueError("group %d has no sample" % int(np.flatnonzero(count == 0)[0]))

    sf = _nb_blind_args(m, n_genes, size_factors, groups)
    return np.ascontiguousarray(codes, dtype=np.int32), n_groups, sf


def _nb_dispersion_arg(dispersion, n_genes, m, shape_checked=False):
    """one dispersion per gene as float64, each NaN (the gene is left out) or in [NB_MIN_DISP, nb_max_disp(m)].  ``shape_checked``:
    the caller has refused a wrong shape in words of its own"""
    alpha = np.ascontiguousarray(dispersion, dtype=np.float64)
    if not shape_checked and alpha.shape != (n_genes,):
        raise ValueError("dispersion has shape %s for %d genes" % (alpha.shape, n_genes))
    given = alpha[~np.isnan(alpha)]
    if given.size and not (given.min() >= NB_MIN_DISP and given.max() <= nb_max_disp(m)):
        raise ValueError("dispersion outside [%g, %g]" % (NB_MIN_DISP, nb_max_disp(m)))
    return alpha


def _positive_finite_arg(name, v):
    """the scalar ``v`` as a float: a positive finite number, no string, bool or array"""
    if isinstance(v, (str, bytes, bool)) or not np.isscalar(v) or not (np.isfinite(v) and v > 0):
        raise ValueError("%s=%r must be positive and finite" % (name, v))
    return float(v)


def _nb_sample_limit(name, m):
    """``name``'s refusal of more samples than a gene can stage in LDS (the first call that loads the library)"""
    limit = nb_glm_limits()
    if m > limit:
        raise NotImplementedError("%s: %d samples; a gene is staged in LDS, at most %d" % (name, m, limit))


def _nb_call(fn, *args):
    """``fn(*args, &bad_row, &bad_col)`` checked; the ValueError of a bad count carries its position as ``row`` and ``col``"""
    bad_row, bad_col = ctypes.c_longlong(-1), ctypes.c_int(-1)
    try:
        _lib.check(fn(*args, ctypes.byref(bad_row), ctypes.byref(bad_col)))
    except ValueError as err:
        err.row, err.col = int(bad_row.value), int(bad_col.value)
        raise


def nb_dispersions(counts, codes, n_groups, size_factors, log_prior_mean=None, prior_var=None, return_info=False):
    """K22: per gene (column) of ``counts`` (samples x genes, float32 / float64 numpy array, :class:`DeviceMatrix` or
    :func:`device_columns` window; c = rint(counts)) the log dispersion of the negative-binomial model with one mean per group
    (include/pilot_ot.h, "negative-binomial GLM"): the maximiser, by six rounds of a 64-point grid over
    [log 1e-8, log max(10, m)], of the Cox-Reid adjusted profile likelihood at the fitted means
    ``mu_j = max(s_j * mean_{i in g(j)} c_i / s_i, 0.5)`` -- with ``log_prior_mean`` (one per gene) and ``prior_var`` minus
    ``(x - log_prior_mean)^2 / (2 prior_var)``, the MAP estimate.  A global search, not DESeq2's line search.  ``codes``: the group
    of every sample, each of 0 .. n_groups - 1 used, ``2 <= n_groups <= m - 1``; ``size_factors`` positive.  Returns the float64
    log dispersions; with ``return_info`` also a dict: ``objective`` (the likelihood there) and ``fitted_mean`` (genes x groups,
    the normalised group means).  A gene of zeros gives NaN.  The same bits from a repeated call, from float32 and float64 storage
    and from host and device matrices.  More than :func:`nb_glm_limits` samples: NotImplementedError; a negative or non-finite
    count: ValueError naming its row and column; every other argument is checked before any device work (ValueError)."""
    Y = _dense_arg(counts, "counts", mode="strict")
    codes, n_groups, sf = _nb_args(Y.rows, Y.cols, codes, n_groups, size_factors)
    if (log_prior_mean is None) != (prior_var is None):
        raise ValueError("log_prior_mean and prior_var come together")
    if log_prior_mean is not None:
        log_prior_mean = np.ascontiguousarray(log_prior_mean, dtype=np.float64)
        if log_prior_mean.shape != (Y.cols,):
            raise ValueError("log_prior_mean has shape %s for %d genes" % (log_prior_mean.shape, Y.cols))
        prior_var = float(prior_var)
        if not (np.isfinite(prior_var) and prior_var > 0):
            raise ValueError("prior_var=%r must be positive and finite" % (prior_var,))
    _nb_sample_limit("nb_dispersions", Y.rows)
    x, objective = np.empty(Y.cols), np.empty(Y.cols)
    fitted = np.empty((Y.cols, n_groups)) if return_info else None
    _nb_call(_lib.load().pilot_ot_nb_dispersions,
             Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, Y.cols, Y.ld, _lib.iptr(codes), n_groups, _lib.dptr(sf),
             None if log_prior_mean is None else _lib.dptr(log_prior_mean), 0.0 if prior_var is None else prior_var, _lib.dptr(x),
             _lib.dptr(objective), None if fitted is None else _lib.dptr(fitted))
    return (x, {"objective": objective, "fitted_mean": fitted}) if return_info else x


def nb_group_fits(counts, codes, n_groups, size_factors, dispersion, return_info=False):
    """K22: per (gene, group) the maximum-likelihood normalised mean ``q`` of the negative-binomial model at the gene's
    ``dispersion`` -- the root of ``sum_{j in g} (c_j - s_j q) / (1 + alpha s_j q) = 0``, raised to ``0.5 / max_{j in g} s_j`` if
    below -- and ``w = sum_{j in g} mu_j / (1 + alpha mu_j)`` with ``mu_j = max(s_j q, 0.5)``, the diagonal of ``X^T W X`` by
    group (include/pilot_ot.h).  ``counts``, ``codes``, ``n_groups`` and ``size_factors`` are :func:`nb_dispersions`'s;
    ``dispersion``: one per gene in [1e-8, max(10, m)], NaN leaves the gene out (NaN results).  Returns ``(q, w)``, both genes x
    groups; with ``return_info`` also a dict: ``steps``, ``flags`` (``_lib.NB_NOT_CONVERGED``, ``_lib.NB_FLOORED``) and
    ``n_not_converged``.  Errors as :func:`nb_dispersions` (no limit on the samples)."""
    Y = _dense_arg(counts, "counts", mode="strict")
    codes, n_groups, sf = _nb_args(Y.rows, Y.cols, codes, n_groups, size_factors)
    alpha = _nb_dispersion_arg(dispersion, Y.cols, Y.rows)
    q, w = np.empty((Y.cols, n_groups)), np.empty((Y.cols, n_groups))
    steps, flags = np.empty((Y.cols, n_groups), dtype=np.int32), np.empty((Y.cols, n_groups), dtype=np.int32)
    bad = ctypes.c_int(0)
    _lib.check(_lib.load().pilot_ot_nb_group_fits(
        Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, Y.cols, Y.ld, _lib.iptr(codes), n_groups, _lib.dptr(sf), _lib.dptr(alpha),
        _lib.dptr(q), _lib.dptr(w), _lib.iptr(steps), _lib.iptr(flags), ctypes.byref(bad)))
    return (q, w, {"steps": steps, "flags": flags, "n_not_converged": bad.value}) if return_info else (q, w)


def _nb_used(disp):
    """the genes the trend and the prior variance are fitted on: a gene-wise estimate of at least 100 minDisp"""
    disp = np.asarray(disp, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(disp) & (disp >= 100 * NB_MIN_DISP)


def nb_trend(base_mean, disp, fit_type="parametric"):
    """The dispersion trend over the genes with ``disp >= 1e-6`` (step 4 of DESIGN.md K22); pure numpy.  ``"parametric"``:
    DESeq2's ``a0 + a1 / base_mean`` from (0.1, 1): every pass keeps the genes with ``1e-4 < disp / fitted < 15`` and fits a
    Gamma-family identity-link GLM on them by IRLS (weights 1 / fitted^2, run until the coefficients move by less than 1e-14
    relative), until ``sum(log(new / old)^2) < 1e-6``.  A non-positive coefficient or more than 10 passes: ValueError (DESeq2
    falls back to a local regression there; here ask for ``fit_type="mean"``).  ``"mean"``: one constant, the mean of the used
    estimates.  Returns ``(fitted, info)``: the trend at every gene's ``base_mean`` and a dict with ``fit_type``,
    ``coefficients`` (a0, a1), ``used`` (the mask of the last fit) and ``passes``."""
    mean, disp = np.asarray(base_mean, dtype=np.float64), np.asarray(disp, dtype=np.float64)
    if mean.ndim != 1 or mean.shape != disp.shape:
        raise ValueError("base_mean %s and disp %s: one of each per gene" % (mean.shape, disp.shape))
    if fit_type not in ("parametric", "mean"):
        raise ValueError("fit_type=%r must be 'parametric' or 'mean'" % (fit_type,))
    use = _nb_used(disp)
    if not use.any():
        raise ValueError("fit_type=%r: no gene has a dispersion estimate of at least %g" % (fit_type, 100 * NB_MIN_DISP))
    if fit_type == "mean":
        info = {"fit_type": "mean", "coefficients": (float(disp[use].mean()), 0.0), "used": use, "passes": 0}
        return nb_trend_at(info, mean), info
    failed = "fit_type='parametric': the dispersion trend a0 + a1 / mean did not fit (%s); use fit_type='mean'"
    inv = np.zeros_like(mean)
    inv[use] = 1.0 / mean[use]
    coefs = np.array([0.1, 1.0])
    for passes in range(1, 11):
        ratio = np.where(use, disp, np.nan) / (coefs[0] + coefs[1] * inv)
        with np.errstate(invalid="ignore"):
            good = use & (ratio > 1e-4) & (ratio < 15)
        if np.count_nonzero(good) < 2:
            raise ValueError(failed % "fewer than two genes within 1e-4 < disp / fitted < 15")
        y, z = disp[good], inv[good]
        new = coefs.copy()
        for _ in range(200):
            f = new[0] + new[1] * z
            if not (f > 0).all():
                raise ValueError(failed % "a fitted value is not positive")
            wt = 1.0 / (f * f)
            s0, s1, s2, t0, t1 = wt.sum(), (wt * z).sum(), (wt * z * z).sum(), (wt * y).sum(), (wt * z * y).sum()
            det = s0 * s2 - s1 * s1
            nxt = np.array([(t0 * s2 - t1 * s1) / det, (s0 * t1 - s1 * t0) / det])
            moved = np.abs(nxt - new).max() <= 1e-14 * np.abs(nxt).max()
            new = nxt
            if moved:
                break
        if not (np.isfinite(new).all() and (new > 0).all()):
            raise ValueError(failed % ("a coefficient is not positive: %r" % (tuple(new),)))
        change = float((np.log(new / coefs) ** 2).sum())
        coefs = new
        if change < 1e-6:
            break
    else:
        raise ValueError(failed % "more than 10 passes")
    info = {"fit_type": "parametric", "coefficients": (float(coefs[0]), float(coefs[1])), "used": good, "passes": passes}
    return nb_trend_at(info, mean), info


def nb_trend_at(info, base_mean):
    """The trend :func:`nb_trend` fitted (its ``info``: ``fit_type`` and ``coefficients`` (a0, a1) are read) at every
    ``base_mean``; pure numpy.  ``"parametric"``: ``a0 + a1 / base_mean`` (infinite at 0); ``"mean"``: a0 wherever the mean is
    finite; NaN for a NaN mean.  What :func:`nb_trend` returns as ``fitted``, and what a refit of some genes reads when the trend
    of the first fit stays."""
    mean = np.asarray(base_mean, dtype=np.float64)
    a0, a1 = info["coefficients"]
    if info["fit_type"] == "mean":
        return np.where(np.isfinite(mean), a0, np.nan)
    if info["fit_type"] != "parametric":
        raise ValueError("fit_type=%r must be 'parametric' or 'mean'" % (info["fit_type"],))
    with np.errstate(divide="ignore", invalid="ignore"):
        return a0 + a1 / mean


def nb_prior_var(log_disp, log_trend, m, k):
    """The width of the log-normal dispersion prior (step 5 of DESIGN.md K22); numpy and scipy.  Over the genes with
    ``exp(log_disp) >= 1e-6``: ``rho = log_disp - log_trend``, ``var_log_disp = (1.4826 median|rho - median rho|)^2`` and
    ``prior_var = max(var_log_disp - trigamma((m - k) / 2), 0.25)`` -- the same formula for ``m - k <= 3``, where DESeq2
    simulates.  Returns ``(prior_var, var_log_disp)``."""
    from scipy import special
    x, t = np.asarray(log_disp, dtype=np.float64), np.asarray(log_trend, dtype=np.float64)
    if x.ndim != 1 or x.shape != t.shape:
        raise ValueError("log_disp %s and log_trend %s: one of each per gene" % (x.shape, t.shape))
    if m - k < 1:
        raise ValueError("m=%d samples in k=%d groups leave no residual degree of freedom" % (m, k))
    with np.errstate(over="ignore", invalid="ignore"):
        use = _nb_used(np.exp(x)) & np.isfinite(t)
    if not use.any():
        raise ValueError("no gene has a dispersion estimate of at least %g" % (100 * NB_MIN_DISP))
    rho = x[use] - t[use]
    var_log_disp = float((1.4826 * np.median(np.abs(rho - np.median(rho)))) ** 2)
    return max(var_log_disp - float(special.polygamma(1, (m - k) / 2.0)), 0.25), var_log_disp


# ---- negative-binomial GLM for a general design (K26; covariates beside the group: `~ batch + stage`) -------------------------------
NB_DESIGN_MAX_COLS = 8
NB_DESIGN_RIDGE = 1e-6
NB_DESIGN_MAX_COND = 1e8


def nb_design_limits():
    """What the K26 calls take: ``{"max_cols": the most design columns, "max_samples": {p: the most samples
    :func:`nb_design_dispersions` takes with p columns}}`` (a gene's counts, log size factors and design rows are staged in LDS)."""
    L = _lib.load()
    max_cols = int(L.pilot_ot_nb_design_max_cols())
    return {"max_cols": max_cols, "max_samples": {p: int(L.pilot_ot_nb_design_max_samples(p)) for p in range(2, max_cols + 1)}}


def _nb_design_arg(design, m):
    """the design matrix of a K26 call checked on the host: C-contiguous float64 m x p, its first column ones, ``2 <= p <=
    NB_DESIGN_MAX_COLS``, ``m - p >= 1``, full column rank and a condition number of at most 1e8"""
    X = np.asarray(design)
    if X.ndim != 2 or X.shape[0] != m:
        raise ValueError("design has shape %s for %d samples: one row per sample" % (X.shape, m))
    if X.dtype.kind not in "biuf":
        raise ValueError("design must be numeric, got %s" % X.dtype)
    X = np.ascontiguousarray(X, dtype=np.float64)
    p = X.shape[1]
    if not 2 <= p <= NB_DESIGN_MAX_COLS:
        raise ValueError("design has %d columns: an intercept and 1 to %d more" % (p, NB_DESIGN_MAX_COLS - 1))
    if m - p < 1:
        raise ValueError("m=%d samples and p=%d design columns leave no residual degree of freedom" % (m, p))
    if not np.isfinite(X).all():
        raise ValueError("design holds a non-finite value")
    if not (X[:, 0] == 1.0).all():
        raise ValueError("the first design column must be ones (the intercept)")
    rank = int(np.linalg.matrix_rank(X))
    if rank != p:
        raise ValueError("design has rank %d, fewer than its %d columns" % (rank, p))
    cond = float(np.linalg.cond(X))
    if not cond <= NB_DESIGN_MAX_COND:
        raise ValueError("design has condition number %.3g, more than %g: rescale its columns" % (cond, NB_DESIGN_MAX_COND))
    return X


def nb_design_dispersions(counts, design, size_factors, log_prior_mean=None, prior_var=None, return_info=False):
    """K26: :func:`nb_dispersions` for a general ``design`` (m x p, the first column ones, ``2 <= p <= NB_DESIGN_MAX_COLS``,
    ``m - p >= 1``, full column rank, condition number <= 1e8) instead of groups: per gene (column) of ``counts`` the log dispersion
    that maximises, by the same six rounds of a 64-point grid, the Cox-Reid adjusted PROFILE likelihood (include/pilot_ot.h,
    "negative-binomial GLM for a general design") -- at every grid point the coefficients are fitted again (the maximiser of the
    negative-binomial likelihood with the ridge 1e-6 on every coefficient, ``mu_j = s_j exp(x_j^T beta)``), the likelihood is taken at
    ``max(mu_j, 0.5)`` and the adjustment is ``1/2 log det X^T W X``; with ``log_prior_mean`` and ``prior_var`` the MAP estimate.
    Returns the float64 log dispersions; with ``return_info`` also a dict: ``objective``, ``beta`` (genes x p, the coefficients at
    the maximiser), ``steps`` (the Newton steps of all 384 inner fits of a gene), ``flags`` (``_lib.NB_NOT_CONVERGED``) and
    ``n_not_converged``.  A gene of zeros gives NaN.  The same bits from a repeated call, from float32 and float64 storage, from
    host and device matrices and for a gene alone or in any batch.  More samples than :func:`nb_design_limits` allows for p:
    NotImplementedError; a negative or non-finite count: ValueError naming its row and column; every other argument is checked
    before any device work (ValueError)."""
    Y = _dense_arg(counts, "counts", mode="strict")
    sf = _nb_blind_args(Y.rows, Y.cols, size_factors)
    X = _nb_design_arg(design, Y.rows)
    if (log_prior_mean is None) != (prior_var is None):
        raise ValueError("log_prior_mean and prior_var come together")
    if log_prior_mean is not None:
        log_prior_mean = np.ascontiguousarray(log_prior_mean, dtype=np.float64)
        if log_prior_mean.shape != (Y.cols,):
            raise ValueError("log_prior_mean has shape %s for %d genes" % (log_prior_mean.shape, Y.cols))
        prior_var = float(prior_var)
        if not (np.isfinite(prior_var) and prior_var > 0):
            raise ValueError("prior_var=%r must be positive and finite" % (prior_var,))
    p = X.shape[1]
    limit = nb_design_limits()["max_samples"][p]
    if Y.rows > limit:
        raise NotImplementedError("nb_design_dispersions: %d samples; a gene is staged in LDS, at most %d with %d design columns"
                                  % (Y.rows, limit, p))
    x, objective, beta = np.empty(Y.cols), np.empty(Y.cols), np.empty((Y.cols, p))
    steps, flags = np.empty(Y.cols, dtype=np.int32), np.empty(Y.cols, dtype=np.int32)
    bad = ctypes.c_int(0)
    _nb_call(_lib.load().pilot_ot_nb_design_dispersions,
             Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, Y.cols, Y.ld, _lib.dptr(X), p, _lib.dptr(sf),
             None if log_prior_mean is None else _lib.dptr(log_prior_mean), 0.0 if prior_var is None else prior_var, _lib.dptr(x),
             _lib.dptr(objective), _lib.dptr(beta), _lib.iptr(steps), _lib.iptr(flags), ctypes.byref(bad))
    info = {"objective": objective, "beta": beta, "steps": steps, "flags": flags, "n_not_converged": bad.value}
    return (x, info) if return_info else x


def nb_design_fits(counts, design, size_factors, dispersion, return_info=False):
    """K26: per gene the coefficients of the negative-binomial GLM ``mu_j = s_j exp(x_j^T beta)`` at the gene's ``dispersion`` (one
    per gene in [1e-8, max(10, m)]; NaN, or a gene of zeros, leaves the gene out: NaN results) -- the maximiser of the likelihood with
    the ridge 1e-6 on every coefficient, natural-log scale (include/pilot_ot.h).  ``counts``, ``design`` and ``size_factors`` are
    :func:`nb_design_dispersions`'s.  Returns ``(beta, cov, loglik)``: genes x p; genes x p x p, ``(X^T W X + 1e-6 I)^-1`` with
    ``W = diag(mu~ / (1 + alpha mu~))``, ``mu~ = max(mu, 0.5)`` (the plain inverse, not DESeq2's sandwich); and the unpenalised
    log likelihood at the unfloored means.  With ``return_info`` also a dict: ``steps``, ``flags`` (``_lib.NB_NOT_CONVERGED``)
    and ``n_not_converged``.  Errors as :func:`nb_design_dispersions` (no limit on the samples)."""
    Y = _dense_arg(counts, "counts", mode="strict")
    sf = _nb_blind_args(Y.rows, Y.cols, size_factors)
    X = _nb_design_arg(design, Y.rows)
    alpha = _nb_dispersion_arg(dispersion, Y.cols, Y.rows)
    p = X.shape[1]
    beta, packed, loglik = np.empty((Y.cols, p)), np.empty((Y.cols, p * (p + 1) // 2)), np.empty(Y.cols)
    steps, flags = np.empty(Y.cols, dtype=np.int32), np.empty(Y.cols, dtype=np.int32)
    bad = ctypes.c_int(0)
    _nb_call(_lib.load().pilot_ot_nb_design_fits,
             Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, Y.cols, Y.ld, _lib.dptr(X), p, _lib.dptr(sf), _lib.dptr(alpha),
             _lib.dptr(beta), _lib.dptr(packed), _lib.dptr(loglik), _lib.iptr(steps), _lib.iptr(flags), ctypes.byref(bad))
    iu = np.triu_indices(p)
    cov = np.empty((Y.cols, p, p))
    cov[:, iu[0], iu[1]] = packed
    cov[:, iu[1], iu[0]] = packed
    info = {"steps": steps, "flags": flags, "n_not_converged": bad.value}
    return (beta, cov, loglik, info) if return_info else (beta, cov, loglik)


# ---- shrunken fold changes (K23; apeglm's posterior mode for the two groups of pilotpy's compute_pseudobulk_DE) ----------------
NB_INTERCEPT_SCALE = 15.0
NB_FAR_END_FLOORED = 30.0


def nb_far_end(lfc, floored):
    """``sg * E`` of :func:`nb_shrink`'s search from the maximum-likelihood fold change ``lfc`` (natural log): sg its sign (+ for
    0), ``E = |lfc| + 1``, or 30 where ``floored`` (a group's fit carries ``_lib.NB_FLOORED``: the likelihood is monotone there
    and only the prior bounds the mode).  A NaN ``lfc`` (a gene left out) gives 1."""
    lfc, floored = np.asarray(lfc, dtype=np.float64), np.asarray(floored, dtype=bool)
    with np.errstate(invalid="ignore"):
        E = np.where(floored, NB_FAR_END_FLOORED, np.abs(lfc) + 1.0)
        return np.where(np.isnan(lfc), 1.0, np.where(lfc >= 0, E, -E))


def nb_shrink(counts, codes, size_factors, dispersion, far_end, prior_scale, intercept_scale=NB_INTERCEPT_SCALE, return_info=False):
    """K23: per gene (column) of ``counts`` the posterior mode ``(beta0, beta1)``, on the natural-log scale, of the two-group
    negative-binomial model ``log mu_j = beta0 + beta1 [codes[j] = 1] + log s_j`` at the gene's ``dispersion`` under apeglm's
    priors: a normal of scale ``intercept_scale`` on beta0 and a Cauchy of scale ``prior_scale`` on beta1 (include/pilot_ot.h,
    pilot_ot_nb_shrink; the rule is this library's statement, unpinned).  The profile over beta0 can have two
    local maxima in beta1, so the mode is found by six rounds of a 64-point grid over ``t in [0, asinh(E / S)]``,
    ``beta1 = sg S sinh(t)``, with ``far_end = sg E`` per gene (:func:`nb_far_end`).  ``counts``, ``codes`` (0 / 1, both used)
    and ``size_factors`` as :func:`nb_dispersions`; ``dispersion``: one per gene in [1e-8, max(10, m)], NaN leaves the gene out
    (NaN results, no flags).  Returns ``(beta0, beta1)``; with ``return_info`` also a dict: ``objective`` (the log posterior up
    to constants there), ``w0`` / ``w1`` (the groups' observed information, for :func:`nb_posterior_sd`), ``flags``
    (``_lib.NB_NOT_CONVERGED``, ``_lib.NB_AT_BOUND``), ``steps`` (the gene's inner Newton steps over all grid points and rounds),
    ``n_at_bound``, ``n_not_converged``.  The same bits from a repeated call, from float32 and float64 storage and from host and
    device matrices.  Errors as :func:`nb_dispersions`."""
    Y = _dense_arg(counts, "counts", mode="strict")
    codes, _, sf = _nb_args(Y.rows, Y.cols, codes, 2, size_factors)
    alpha, far = np.ascontiguousarray(dispersion, dtype=np.float64), np.ascontiguousarray(far_end, dtype=np.float64)
    if alpha.shape != (Y.cols,) or far.shape != (Y.cols,):
        raise ValueError("dispersion %s and far_end %s: one of each for %d genes" % (alpha.shape, far.shape, Y.cols))
    alpha = _nb_dispersion_arg(alpha, Y.cols, Y.rows, shape_checked=True)
    if not np.isfinite(far).all():
        raise ValueError("far_end must be finite")
    prior_scale, intercept_scale = float(prior_scale), float(intercept_scale)
    if not (np.isfinite(prior_scale) and prior_scale > 0):
        raise ValueError("prior_scale=%r must be positive and finite" % (prior_scale,))
    if not (np.isfinite(intercept_scale) and intercept_scale > 0):
        raise ValueError("intercept_scale=%r must be positive and finite" % (intercept_scale,))
    _nb_sample_limit("nb_shrink", Y.rows)
    b0, b1, objective, w = np.empty(Y.cols), np.empty(Y.cols), np.empty(Y.cols), np.empty((Y.cols, 2))
    raw = np.empty(Y.cols, dtype=np.int32)
    at_bound = ctypes.c_int(0)
    _nb_call(_lib.load().pilot_ot_nb_shrink,
             Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, Y.cols, Y.ld, _lib.iptr(codes), _lib.dptr(sf), _lib.dptr(alpha),
             _lib.dptr(far), prior_scale, intercept_scale, _lib.dptr(b0), _lib.dptr(b1), _lib.dptr(objective), _lib.dptr(w),
             _lib.iptr(raw), ctypes.byref(at_bound))
    if not return_info:
        return b0, b1
    flags = raw & ((1 << _lib.NB_SHRINK_STEPS_SHIFT) - 1)
    return b0, b1, {"objective": objective, "w0": w[:, 0].copy(), "w1": w[:, 1].copy(), "flags": flags,
                    "steps": raw >> _lib.NB_SHRINK_STEPS_SHIFT, "n_at_bound": at_bound.value,
                    "n_not_converged": int(np.count_nonzero(flags & _lib.NB_NOT_CONVERGED))}


def nb_prior_scale(lfc, se, use=None):
    """The scale of :func:`nb_shrink`'s Cauchy prior from the maximum-likelihood fold changes ``lfc`` and their standard errors
    ``se`` (natural log), as apeglm's ``priorVar``; numpy and scipy.  Over the genes where both are finite (and ``use``, a mask:
    the genes without a floored group fit), with ``D = lfc`` and ``V = se^2``: ``A`` is the root on [1e-6, 400] of the score of the
    marginal likelihood ``D ~ N(0, V + A)``, ``f(A) = sum (D^2 - V - A) / (V + A)^2`` (``scipy.optimize.brentq``); 1e-6 if
    ``f(1e-6) <= 0`` and 400 if ``f(400) >= 0``.  Returns ``(S, A)`` with ``S = min(sqrt(A), 1)``.  Fewer than two usable genes:
    ValueError."""
    from scipy import optimize
    D, se = np.asarray(lfc, dtype=np.float64), np.asarray(se, dtype=np.float64)
    if D.ndim != 1 or D.shape != se.shape:
        raise ValueError("lfc %s and se %s: one of each per gene" % (D.shape, se.shape))
    ok = np.isfinite(D) & np.isfinite(se)
    if use is not None:
        use = np.asarray(use, dtype=bool)
        if use.shape != D.shape:
            raise ValueError("use has shape %s for %d genes" % (use.shape, D.size))
        ok &= use
    if np.count_nonzero(ok) < 2:
        raise ValueError("nb_prior_scale: %d usable genes (finite, no floored group fit), at least 2" % np.count_nonzero(ok))
    D, V = D[ok], se[ok] ** 2

    def f(A):
        return float(((D * D - V - A) / (V + A) ** 2).sum())

    lo, hi = 1e-6, 400.0
    if f(lo) <= 0:
        A = lo
    elif f(hi) >= 0:
        A = hi
    else:
        A = float(optimize.brentq(f, lo, hi, xtol=1e-14, rtol=1e-14, maxiter=500))
    return min(float(np.sqrt(A)), 1.0), A


def nb_posterior_sd(beta1, w0, w1, prior_scale, intercept_scale=NB_INTERCEPT_SCALE):
    """The Laplace approximation of the posterior standard deviation of beta1 at :func:`nb_shrink`'s mode: with the Hessian of
    minus the log posterior, ``H00 = w0 + w1 + 1 / sigma0^2``, ``H01 = w1``, ``H11 = w1 + 2 (S^2 - b1^2) / (S^2 + b1^2)^2``,
    ``sd = sqrt(H00 / (H00 H11 - H01^2))``; NaN where the determinant is not positive (the Cauchy prior is not log-concave
    beyond ``|b1| = S``) and where an input is NaN."""
    b1, w0, w1 = (np.asarray(a, dtype=np.float64) for a in (beta1, w0, w1))
    S2 = float(prior_scale) ** 2
    h00 = w0 + w1 + 1.0 / float(intercept_scale) ** 2
    h11 = w1 + 2.0 * (S2 - b1 * b1) / (S2 + b1 * b1) ** 2
    det = h00 * h11 - w1 * w1
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(det > 0, np.sqrt(h00 / det), np.nan)


# ---- shrunken coefficient under a general design (K27; lfcShrink(type = "apeglm") after `~ covariates + stage`) -------------------
def nb_design_far_end(beta_k):
    """``sg * E`` of :func:`nb_design_shrink`'s search from :func:`nb_design_fits`' coefficient ``beta_k`` (natural log): sg its
    sign (+ for 0), ``E = |beta_k| + 1`` (that fit's ridge keeps the coefficient finite, so there is no floored case as in
    :func:`nb_far_end`).  A NaN (a gene left out) gives 1."""
    return nb_far_end(beta_k, np.zeros(np.shape(beta_k), dtype=bool))


def _nb_coef_arg(coef, p):
    """the shrunk design column as an index in [1, p - 1]; a negative ``coef`` counts from the end"""
    if isinstance(coef, (bool, np.bool_)) or not isinstance(coef, (int, np.integer)):
        raise ValueError("coef=%r must be an integer" % (coef,))
    k = int(coef) + p if coef < 0 else int(coef)
    if not 1 <= k <= p - 1:
        raise ValueError("coef=%r must name one of the design columns 1 .. %d (the intercept is not shrunk)" % (coef, p - 1))
    return k


def nb_design_shrink(counts, design, size_factors, dispersion, beta_mle, far_end, prior_scale, coef=-1, other_scale=NB_INTERCEPT_SCALE,
                     return_info=False):
    """K27: :func:`nb_shrink` for a general ``design`` (:func:`nb_design_fits`' m x p matrix): per gene (column) of ``counts`` the
    posterior mode ``beta`` (genes x p, natural log) of ``log mu_j = x_j^T beta + log s_j`` at the gene's ``dispersion`` under a
    Cauchy prior of scale ``prior_scale`` on the coefficient of column ``coef`` (default: the last, the group) and a normal of
    scale ``other_scale`` on EVERY other coefficient, the intercept included (include/pilot_ot.h, pilot_ot_nb_design_shrink;
    DESIGN.md K27; the rule is this library's statement, unpinned).  The profile over the other coefficients can have two local
    maxima, so the mode is found by six rounds of a 64-point grid over ``t in [0, asinh(E / S)]``, ``beta_coef = sg S sinh(t)``,
    with ``far_end = sg E`` per gene (:func:`nb_design_far_end`); at every grid point the p - 1 other coefficients are fitted by
    Newton steps, round 0 from ``beta_mle`` (genes x p, :func:`nb_design_fits`' coefficients).  For ``design = [1, codes]`` the
    rule is :func:`nb_shrink`'s.  A NaN dispersion, a gene of zeros or a non-finite ``beta_mle`` leaves the gene out (NaN results,
    no flags).  Returns ``beta``; with ``return_info`` also a dict: ``objective`` (the log posterior up to constants there),
    ``information`` (genes x p x p, ``X^T W X`` with ``w = mu (1 + alpha c) / (1 + alpha mu)^2``, for
    :func:`nb_design_posterior_sd`), ``flags`` (``_lib.NB_NOT_CONVERGED``, ``_lib.NB_AT_BOUND``), ``steps`` (the gene's inner
    Newton steps over all grid points and rounds), ``n_at_bound``, ``n_not_converged``.  The same bits from a repeated call, from
    float32 and float64 storage, from host and device matrices, from column windows and for a gene alone or in any batch.  Errors
    as :func:`nb_design_dispersions`."""
    Y = _dense_arg(counts, "counts", mode="strict")
    sf = _nb_blind_args(Y.rows, Y.cols, size_factors)
    X = _nb_design_arg(design, Y.rows)
    p = X.shape[1]
    k = _nb_coef_arg(coef, p)
    alpha = _nb_dispersion_arg(dispersion, Y.cols, Y.rows)
    mle, far = np.ascontiguousarray(beta_mle, dtype=np.float64), np.ascontiguousarray(far_end, dtype=np.float64)
    if mle.shape != (Y.cols, p):
        raise ValueError("beta_mle has shape %s for %d genes and %d design columns" % (mle.shape, Y.cols, p))
    if far.shape != (Y.cols,):
        raise ValueError("far_end has shape %s for %d genes" % (far.shape, Y.cols))
    if not np.isfinite(far).all():
        raise ValueError("far_end must be finite")
    prior_scale, other_scale = _positive_finite_arg("prior_scale", prior_scale), _positive_finite_arg("other_scale", other_scale)
    limit = nb_design_limits()["max_samples"][p]
    if Y.rows > limit:
        raise NotImplementedError("nb_design_shrink: %d samples; a gene is staged in LDS, at most %d with %d design columns"
                                  % (Y.rows, limit, p))
    beta, objective, packed = np.empty((Y.cols, p)), np.empty(Y.cols), np.empty((Y.cols, p * (p + 1) // 2))
    raw = np.empty(Y.cols, dtype=np.int32)
    at_bound = ctypes.c_int(0)
    _nb_call(_lib.load().pilot_ot_nb_design_shrink,
             Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, Y.cols, Y.ld, _lib.dptr(X), p, k, _lib.dptr(sf), _lib.dptr(alpha),
             _lib.dptr(mle), _lib.dptr(far), prior_scale, other_scale, _lib.dptr(beta), _lib.dptr(objective), _lib.dptr(packed),
             _lib.iptr(raw), ctypes.byref(at_bound))
    if not return_info:
        return beta
    iu = np.triu_indices(p)
    information = np.empty((Y.cols, p, p))
    information[:, iu[0], iu[1]] = packed
    information[:, iu[1], iu[0]] = packed
    flags = raw & ((1 << _lib.NB_SHRINK_STEPS_SHIFT) - 1)
    return beta, {"objective": objective, "information": information, "flags": flags, "steps": raw >> _lib.NB_SHRINK_STEPS_SHIFT,
                  "n_at_bound": at_bound.value, "n_not_converged": int(np.count_nonzero(flags & _lib.NB_NOT_CONVERGED))}


def nb_design_posterior_sd(beta, information, prior_scale, coef=-1, other_scale=NB_INTERCEPT_SCALE):
    """The Laplace approximation of the posterior standard deviation of the shrunk coefficient at :func:`nb_design_shrink`'s mode;
    numpy.  With the Hessian of minus the log posterior, ``H = information + diag(1 / other_scale^2 for every other column;
    2 (S^2 - b^2) / (S^2 + b^2)^2 for column coef)``, ``b = beta[:, coef]``: ``sd = sqrt((H^-1)[coef, coef])``; NaN where H is not
    positive definite (the Cauchy prior is not log-concave beyond ``|b| = S``) and where an input is NaN.  With two columns this is
    :func:`nb_posterior_sd`'s formula."""
    beta, info = np.asarray(beta, dtype=np.float64), np.asarray(information, dtype=np.float64)
    if beta.ndim != 2 or info.shape != beta.shape + beta.shape[1:]:
        raise ValueError("beta %s and information %s: genes x p and genes x p x p" % (beta.shape, info.shape))
    p = beta.shape[1]
    k = _nb_coef_arg(coef, p)
    S2 = _positive_finite_arg("prior_scale", prior_scale) ** 2
    b = beta[:, k]
    with np.errstate(invalid="ignore", divide="ignore"):
        prior = np.full(beta.shape, 1.0 / _positive_finite_arg("other_scale", other_scale) ** 2)
        prior[:, k] = 2.0 * (S2 - b * b) / (S2 + b * b) ** 2
    H = info.copy()
    H[:, np.arange(p), np.arange(p)] += prior
    sd = np.full(beta.shape[0], np.nan)
    for g in np.flatnonzero(np.isfinite(H).all(axis=(1, 2))):
        try:
            np.linalg.cholesky(H[g])
        except np.linalg.LinAlgError:
            continue
        e = np.zeros(p)
        e[k] = 1.0
        v = np.linalg.solve(H[g], e)[k]
        if v > 0:
            sd[g] = np.sqrt(v)
    return sd


# ---- regularised log transform (K24; DESeq2's rlog(blind = TRUE) of pilotpy's compute_pseudobulk_PCA) ---------------------------
def nb_dispersions_blind(counts, size_factors, return_info=False):
    """K24: :func:`nb_dispersions` for the design ``~ 1`` (DESeq2's ``blind = TRUE``): ONE group of all the samples, which that call
    refuses, and no prior -- ``mu_j = max(s_j * mean_i(c_i / s_i), 0.5)`` and the same six rounds of the 64-point grid on the
    Cox-Reid adjusted profile likelihood.  ``counts`` and ``size_factors`` as there, at least 2 samples.  Returns the float64 log
    dispersions (NaN for a gene of zeros); with ``return_info`` also a dict: ``objective`` and ``base_mean`` (the mean of
    ``c / s`` over the samples, as the device summed it).  Errors as :func:`nb_dispersions`."""
    Y = _dense_arg(counts, "counts", mode="strict")
    sf = _nb_blind_args(Y.rows, Y.cols, size_factors)
    _nb_sample_limit("nb_dispersions_blind", Y.rows)
    x, objective, base_mean = np.empty(Y.cols), np.empty(Y.cols), np.empty(Y.cols)
    _nb_call(_lib.load().pilot_ot_nb_dispersions_blind,
             Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, Y.cols, Y.ld, _lib.dptr(sf), _lib.dptr(x), _lib.dptr(objective),
             _lib.dptr(base_mean))
    return (x, {"objective": objective, "base_mean": base_mean}) if return_info else x


NB_RLOG_UPPER_QUANTILE = 0.05


def nb_rlog_prior_var(counts, size_factors, base_mean, disp_fit):
    """The prior variance of :func:`nb_rlog`'s sample coefficients on the log2 scale (step 2 of DESIGN.md K24: DESeq2's
    ``matchWeightedUpperQuantileForVariance`` restated); numpy and scipy, one sort of samples x genes values on the host.
    ``counts``: a host samples x genes array (c = rint); ``base_mean`` and ``disp_fit`` one per gene.  Over the genes with
    ``base_mean > 0`` and all samples: ``x = |log2(c / s + 0.5) - log2(base_mean + 0.5)|`` with weight
    ``1 / (1 / base_mean + disp_fit)``; the weights of equal x are summed, ``cum`` is their running sum in ascending x and W its
    total; ``o = 1 + (W - 1) 0.95``, ``low = max(floor(o), 1)``, ``high = min(low + 1, W)``, ``f = o mod 1``; q(t) is the x at the
    first position with ``cum >= t`` (the last x beyond the end); ``Q = (1 - f) q(low) + f q(high)`` (Hmisc's ``wtd.quantile`` with
    ``normwt = FALSE``); returns ``(Q / norm.ppf(0.975))^2``.  No gene with a positive mean and a finite trend: ValueError."""
    from scipy import special
    c = np.rint(np.asarray(counts, dtype=np.float64))
    if c.ndim != 2:
        raise ValueError("counts: a samples x genes host array, got shape %s" % (c.shape,))
    sf = _nb_blind_args(c.shape[0], c.shape[1], size_factors)
    mean, fit = np.asarray(base_mean, dtype=np.float64), np.asarray(disp_fit, dtype=np.float64)
    if mean.shape != (c.shape[1],) or fit.shape != mean.shape:
        raise ValueError("base_mean %s and disp_fit %s: one of each for %d genes" % (mean.shape, fit.shape, c.shape[1]))
    with np.errstate(invalid="ignore"):
        use = (mean > 0) & np.isfinite(fit)
    if not use.any():
        raise ValueError("nb_rlog_prior_var: no gene has a positive mean and a finite dispersion trend")
    x = np.abs(np.log2(c[:, use] / sf[:, None] + 0.5) - np.log2(mean[use] + 0.5)[None])
    weight = np.broadcast_to((1.0 / (1.0 / mean[use] + fit[use]))[None], x.shape)
    values, inverse = np.unique(x.ravel(), return_inverse=True)
    cum = np.cumsum(np.bincount(np.ravel(inverse), weights=weight.ravel(), minlength=values.size))
    W = cum[-1]
    o = 1.0 + (W - 1.0) * (1.0 - NB_RLOG_UPPER_QUANTILE)
    low = max(np.floor(o), 1.0)
    high = min(low + 1.0, W)
    f = o % 1.0
    q = lambda t: values[min(int(np.searchsorted(cum, t, side="left")), values.size - 1)]
    Q = (1.0 - f) * q(low) + f * q(high)
    return float((Q / special.ndtri(1.0 - NB_RLOG_UPPER_QUANTILE / 2.0)) ** 2)


def nb_rlog(counts, size_factors, dispersion, prior_var, on_device=False, return_info=False):
    """K24: the regularised log transform of ``counts`` (samples x genes, as :func:`nb_dispersions` takes them) on the log2 scale
    (include/pilot_ot.h, pilot_ot_nb_rlog; the rule is this library's statement, unpinned).  Per gene the
    negative-binomial GLM ``log mu_j = beta0 + beta_j + log s_j`` with one coefficient a sample at the gene's ``dispersion`` (the
    trend value, in [1e-8, max(10, m)]; NaN leaves the gene out), a normal prior of variance ``prior_var`` (log2 scale,
    :func:`nb_rlog_prior_var`) on the sample coefficients and an all but flat one on the intercept; the posterior mode is the one
    maximiser of a strictly concave function, found by damped Newton steps (one wave per gene, the samples along the lanes) to
    1e-10.  Returns ``(beta0 + beta_j) / ln 2`` as a samples x genes float64 array, or with ``on_device`` as a
    :class:`DeviceMatrix` that :func:`pca` takes without a trip through the host.  A gene of zeros gives 0 in every sample.  With
    ``return_info`` also a dict: ``intercept`` (``beta0 / ln 2``; NaN for a gene of zeros), ``steps`` (Newton iterations),
    ``flags`` (``_lib.NB_NOT_CONVERGED`` after 100) and ``n_not_converged``.  The same bits from a repeated call, from float32 and
    float64 storage, from host and device matrices, and for a gene alone or in any batch.  Errors as :func:`nb_dispersions`."""
    Y = _dense_arg(counts, "counts", mode="strict")
    sf = _nb_blind_args(Y.rows, Y.cols, size_factors)
    alpha = _nb_dispersion_arg(dispersion, Y.cols, Y.rows)
    prior_var = _positive_finite_arg("prior_var", prior_var)
    _nb_sample_limit("nb_rlog", Y.rows)
    out, out_ptr = _result_matrix(Y.rows, Y.cols, on_device)
    intercept = np.empty(Y.cols)
    steps, flags = np.empty(Y.cols, dtype=np.int32), np.empty(Y.cols, dtype=np.int32)
    bad = ctypes.c_int(0)
    _nb_call(_lib.load().pilot_ot_nb_rlog,
             Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, Y.cols, Y.ld, _lib.dptr(sf), _lib.dptr(alpha), prior_var, out_ptr,
             int(bool(on_device)), Y.cols, _lib.dptr(intercept), _lib.iptr(steps), _lib.iptr(flags), ctypes.byref(bad))
    return (out, {"intercept": intercept, "steps": steps, "flags": flags, "n_not_converged": bad.value}) if return_info else out


# ---- Cook's distances, outlier replacement and independent filtering (K25; DESeq(dds) and results(dds) of compute_pseudobulk_DE) -
NB_COOKS_MIN_REPLACE = 7
NB_COOKS_MIN_GROUP = 3
NB_COOKS_QUANTILE = 0.99


def nb_cooks_cutoff(m, p):
    """DESeq2's default ``cooksCutoff``: ``qf(0.99, p, m - p)`` of m samples and p coefficients."""
    from scipy import stats
    if isinstance(m, bool) or isinstance(p, bool) or int(m) != m or int(p) != p or p < 1 or m - p < 1:
        raise ValueError("nb_cooks_cutoff: m=%r samples and p=%r coefficients must be integers with p >= 1 and m - p >= 1" % (m, p))
    return float(stats.f.ppf(NB_COOKS_QUANTILE, int(p), int(m) - int(p)))


def _nb_cutoff_arg(cutoff):
    return _positive_finite_arg("cutoff", cutoff)


def _nb_min_replace_arg(min_replace):
    if isinstance(min_replace, bool) or int(min_replace) != min_replace or min_replace < NB_COOKS_MIN_GROUP:
        raise ValueError("min_replace=%r must be an integer >= %d" % (min_replace, NB_COOKS_MIN_GROUP))
    return int(min_replace)


def nb_cooks(counts, codes, n_groups, size_factors, dispersion, q, cutoff, min_replace=NB_COOKS_MIN_REPLACE, return_distances=False):
    """K25: per gene (column) of ``counts`` the Cook's distances of the negative-binomial group fits, as DESeq2's outlier handling
    reads them (include/pilot_ot.h, pilot_ot_nb_cooks; the rule is this library's statement, unpinned).
    ``counts``, ``codes``, ``n_groups`` and ``size_factors`` as :func:`nb_group_fits`; ``dispersion``: the gene's final dispersion
    (NaN leaves the gene out); ``q``: genes x groups, :func:`nb_group_fits`' fits at it (positive where the gene has a
    dispersion).  The variance in the distance comes from a ROBUST dispersion -- the largest trimmed variance of ``c / s`` over
    the groups of at least 3 samples -- so that the outlier does not hide itself; the hat diagonal is
    ``w_j / sum_{group} w`` at the final dispersion.  ``cutoff`` (:func:`nb_cooks_cutoff`) and ``min_replace`` only count.
    Returns a dict of per-gene arrays: ``alpha_robust``, ``max_cooks`` (over the samples of groups with at least 3),
    ``arg_max`` (the lowest sample that attains it, -1 without one), ``n_above`` (samples with a larger count than that one),
    ``n_replace`` (samples above ``cutoff`` in groups of at least ``min_replace``), ``trimmed_base`` (the 0.2-trimmed mean of
    ``c / s`` over all samples); with ``return_distances`` also ``D``, samples x genes (``"device"``: a :class:`DeviceMatrix`).
    One wave per gene, a bitonic sort in LDS.  The same bits from a repeated call, from float32 and float64 storage, from host and
    device matrices, and for a gene alone or in any batch.  Errors as :func:`nb_dispersions`."""
    Y = _dense_arg(counts, "counts", mode="strict")
    codes, n_groups, sf = _nb_args(Y.rows, Y.cols, codes, n_groups, size_factors)
    alpha = _nb_dispersion_arg(dispersion, Y.cols, Y.rows)
    q = np.ascontiguousarray(q, dtype=np.float64)
    if q.shape != (Y.cols, n_groups):
        raise ValueError("q has shape %s for %d genes in %d groups" % (q.shape, Y.cols, n_groups))
    fitted = q[~np.isnan(alpha)]
    if not (np.isfinite(fitted).all() and (fitted > 0).all()):
        raise ValueError("q must be positive and finite where the gene has a dispersion")
    cutoff, min_replace = _nb_cutoff_arg(cutoff), _nb_min_replace_arg(min_replace)
    if return_distances not in (False, True, "device"):
        raise ValueError("return_distances=%r must be False, True or 'device'" % (return_distances,))
    _nb_sample_limit("nb_cooks", Y.rows)
    out = {name: np.empty(Y.cols) for name in ("alpha_robust", "max_cooks", "trimmed_base")}
    out.update({name: np.empty(Y.cols, dtype=np.int32) for name in ("arg_max", "n_above", "n_replace")})
    on_device = return_distances == "device"
    D, D_ptr = _result_matrix(Y.rows, Y.cols, on_device) if return_distances else (None, None)
    _nb_call(_lib.load().pilot_ot_nb_cooks,
             Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, Y.cols, Y.ld, _lib.iptr(codes), n_groups, _lib.dptr(sf), _lib.dptr(alpha),
             _lib.dptr(q), cutoff, min_replace, _lib.dptr(out["alpha_robust"]), _lib.dptr(out["max_cooks"]), _lib.iptr(out["arg_max"]),
             _lib.iptr(out["n_above"]), _lib.iptr(out["n_replace"]), _lib.dptr(out["trimmed_base"]), D_ptr, int(on_device), Y.cols)
    if D is not None:
        out["D"] = D
    return out


def nb_replacements(counts, codes, size_factors, D, cutoff, trimmed_base, min_replace=NB_COOKS_MIN_REPLACE):
    """DESeq2's ``replaceOutliers`` as tidy rows; pure numpy.  ``counts`` (samples x genes, host; c = rint), ``D`` (samples x
    genes, :func:`nb_cooks`' distances) and ``trimmed_base`` (one per gene) describe the same genes.  A count is replaced where
    ``D > cutoff`` in a group of at least ``min_replace`` samples, by ``trunc(trimmed_base * s_j)`` (R's ``as.integer``).  Returns
    a structured array with the fields ``gene`` and ``sample`` (positions), ``count`` and ``replacement`` (float64), ordered by
    gene, then sample."""
    c = np.rint(np.asarray(counts, dtype=np.float64))
    D, base = np.asarray(D, dtype=np.float64), np.asarray(trimmed_base, dtype=np.float64)
    if c.ndim != 2 or D.shape != c.shape or base.shape != (c.shape[1],):
        raise ValueError("counts %s, D %s and trimmed_base %s: samples x genes, the same, and one per gene" % (c.shape, D.shape, base.shape))
    codes = np.asarray(codes)
    if codes.shape != (c.shape[0],) or codes.dtype.kind not in "iu" or (codes.size and codes.min() < 0):
        raise ValueError("codes: one non-negative integer per sample")
    sf = np.asarray(size_factors, dtype=np.float64)
    if sf.shape != (c.shape[0],) or not (np.isfinite(sf).all() and (sf > 0).all()):
        raise ValueError("size_factors: one positive finite value per sample")
    cutoff, min_replace = _nb_cutoff_arg(cutoff), _nb_min_replace_arg(min_replace)
    big = np.bincount(codes)[codes] >= min_replace
    with np.errstate(invalid="ignore"):
        sample, gene = np.nonzero((D > cutoff) & big[:, None])
    at = np.lexsort((sample, gene))
    sample, gene = sample[at], gene[at]
    rows = np.empty(gene.size, dtype=[("gene", np.int64), ("sample", np.int64), ("count", np.float64), ("replacement", np.float64)])
    rows["gene"], rows["sample"], rows["count"] = gene, sample, c[sample, gene]
    rows["replacement"] = np.trunc(base[gene] * sf[sample])
    return rows


# ---- Cook's distances under a general design (K28; the outlier handling of K25 for the model with covariates of K26) -----------------
def nb_design_cells(design):
    """DESeq2's ``nOrMoreInCell`` grouping of a design matrix; pure numpy.  A cell is a maximal set of samples whose rows of
    ``design`` (m x p) are bit-identical; cells are numbered by first appearance.  Returns ``(codes int32, n_cells)``.  For
    ``[1, indicator]`` the cells are the two groups; with a numeric covariate every cell is usually one sample."""
    X = np.asarray(design)
    if X.ndim != 2 or X.shape[0] < 1 or X.dtype.kind not in "biuf":
        raise ValueError("design must be a numeric samples x columns matrix, got shape %s of %s" % (X.shape, X.dtype))
    X = np.ascontiguousarray(X, dtype=np.float64)
    seen, codes = {}, np.empty(X.shape[0], dtype=np.int32)
    for j in range(X.shape[0]):
        codes[j] = seen.setdefault(X[j].tobytes(), len(seen))
    return codes, len(seen)


def nb_design_cooks(counts, design, size_factors, dispersion, beta, cutoff, min_replace=NB_COOKS_MIN_REPLACE, return_distances=False):
    """K28: :func:`nb_cooks` for a general ``design`` (as :func:`nb_design_fits` takes it): per gene (column) of ``counts`` the Cook's
    distances of the negative-binomial GLM with covariates (include/pilot_ot.h, pilot_ot_nb_design_cooks; the rule is
    this library's statement, unpinned).  ``dispersion``: the gene's final dispersion (NaN leaves the gene out); ``beta``: genes x p,
    :func:`nb_design_fits`' coefficients at it (finite where the gene has a dispersion).  K25's groups become CELLS
    (:func:`nb_design_cells`: samples with identical design rows).  The robust dispersion comes from the largest trimmed variance of
    ``c / s`` over the cells of at least 3 samples, or, without one, from the 1/8-trimmed variance over all samples; the hat diagonal is
    ``h_j = w_j x_j^T (X^T W X + 1e-6 I)^-1 x_j`` at the fitted means and the final dispersion, and the distance divides by p.
    Returns the dict of :func:`nb_cooks` (``max_cooks`` and ``arg_max`` over the samples of cells with at least 3, ``n_replace`` over
    those of at least ``min_replace``); with ``return_distances`` also ``D`` and ``H`` (the hat diagonal), samples x genes
    (``"device"``: :class:`DeviceMatrix`).  Under a design whose cells are all below 3 (a numeric covariate) the distances are
    computed but nothing can be replaced or flagged: ``max_cooks`` is NaN and ``n_replace`` 0, as in DESeq2.  One wave per gene.  The
    same bits from a repeated call, from float32 and float64 storage, from host and device matrices, and for a gene alone or in any
    batch.  More samples than :func:`nb_design_limits` allows for p: NotImplementedError; errors otherwise as
    :func:`nb_design_fits`."""
    Y = _dense_arg(counts, "counts", mode="strict")
    sf = _nb_blind_args(Y.rows, Y.cols, size_factors)
    X = _nb_design_arg(design, Y.rows)
    alpha = _nb_dispersion_arg(dispersion, Y.cols, Y.rows)
    p = X.shape[1]
    beta = np.ascontiguousarray(beta, dtype=np.float64)
    if beta.shape != (Y.cols, p):
        raise ValueError("beta has shape %s for %d genes and %d design columns" % (beta.shape, Y.cols, p))
    if not np.isfinite(beta[~np.isnan(alpha)]).all():
        raise ValueError("beta must be finite where the gene has a dispersion")
    cutoff, min_replace = _nb_cutoff_arg(cutoff), _nb_min_replace_arg(min_replace)
    if return_distances not in (False, True, "device"):
        raise ValueError("return_distances=%r must be False, True or 'device'" % (return_distances,))
    cells, n_cells = nb_design_cells(X)
    limit = nb_design_limits()["max_samples"][p]
    if Y.rows > limit:
        raise NotImplementedError("nb_design_cooks: %d samples; a gene is staged in LDS, at most %d with %d design columns" % (Y.rows, limit, p))
    out = {name: np.empty(Y.cols) for name in ("alpha_robust", "max_cooks", "trimmed_base")}
    out.update({name: np.empty(Y.cols, dtype=np.int32) for name in ("arg_max", "n_above", "n_replace")})
    on_device = return_distances == "device"
    D, D_ptr = _result_matrix(Y.rows, Y.cols, on_device) if return_distances else (None, None)
    H, H_ptr = _result_matrix(Y.rows, Y.cols, on_device) if return_distances else (None, None)
    _nb_call(_lib.load().pilot_ot_nb_design_cooks,
             Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, Y.cols, Y.ld, _lib.dptr(X), p, _lib.iptr(cells), n_cells, _lib.dptr(sf),
             _lib.dptr(alpha), _lib.dptr(beta), cutoff, min_replace, _lib.dptr(out["alpha_robust"]), _lib.dptr(out["max_cooks"]),
             _lib.iptr(out["arg_max"]), _lib.iptr(out["n_above"]), _lib.iptr(out["n_replace"]), _lib.dptr(out["trimmed_base"]),
             D_ptr, int(on_device), Y.cols, H_ptr, int(on_device), Y.cols)
    if D is not None:
        out["D"], out["H"] = D, H
    return out


def bh_adjust(p):
    """Benjamini-Hochberg adjusted p-values (statsmodels' multipletests(method='fdr_bh')[1])."""
    p = np.asarray(p, dtype=np.float64)
    m = p.size
    if m == 0:
        return p.copy()
    order = np.argsort(p, kind="stable")
    scaled = p[order] * m / np.arange(1, m + 1)
    adj = np.minimum(np.minimum.accumulate(scaled[::-1])[::-1], 1.0)
    out = np.empty(m)
    out[order] = adj
    return out


def lowess(x, y, f=2.0 / 3.0, iters=3):
    """R's ``lowess(x, y, f, iter = iters, delta = 0)`` restated (Cleveland 1979, as in R's clowess.c, from memory; statsmodels is
    not available where this library is tested, so the rule is UNPINNED): every point is fitted, there is no ``delta``
    skipping.  ``x`` ascending.  Per point the window of ``ns = max(min(n, floor(f n + 1e-7)), 2)`` nearest points, tricube
    weights over its half-width h (1 within 0.001 h, 0 beyond 0.999 h; points beyond the window that tie its edge are kept), a
    weighted line (a weighted mean where the weighted spread of x is below 0.001 of its range); after each of ``iters`` passes
    the bisquare robustness weights ``(1 - (r / 6 MAD)^2)^2`` of the residuals r (1 within 0.001, 0 beyond 0.999 of 6 MAD),
    stopping early once 6 MAD is below 1e-7 of the mean absolute residual.  Returns the fitted values."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.ndim != 1 or x.shape != y.shape or x.size < 2:
        raise ValueError("lowess: x %s and y %s must be two vectors of one length >= 2" % (x.shape, y.shape))
    if not (np.isfinite(x).all() and np.isfinite(y).all() and (np.diff(x) >= 0).all()):
        raise ValueError("lowess: x and y must be finite and x ascending")
    if isinstance(f, bool) or not np.isscalar(f) or not 0 < f <= 1:
        raise ValueError("lowess: f=%r must be in (0, 1]" % (f,))
    if isinstance(iters, bool) or int(iters) != iters or iters < 0:
        raise ValueError("lowess: iters=%r must be a non-negative integer" % (iters,))
    n = x.size
    ns = max(min(n, int(f * n + 1e-7)), 2)
    span = x[-1] - x[0]
    rw = np.ones(n)
    fit = np.empty(n)
    for it in range(int(iters) + 1):
        nleft, nright = 0, ns - 1
        for i in range(n):
            while nright < n - 1 and x[nright + 1] - x[i] < x[i] - x[nleft]:
                nleft, nright = nleft + 1, nright + 1
            h = max(x[i] - x[nleft], x[nright] - x[i])
            stop = nright + 1
            while stop < n and x[stop] - x[i] <= 0.999 * h:          # ties with the edge of the window
                stop += 1
            xs, r = x[nleft:stop], np.abs(x[nleft:stop] - x[i])
            w = np.where(r <= 0.999 * h, np.where(r <= 0.001 * h, 1.0, (1.0 - (r / h) ** 3) ** 3 if h > 0 else 1.0), 0.0) * rw[nleft:stop]
            a = w.sum()
            if not a > 0:
                fit[i] = y[i]
                continue
            w = w / a
            if h > 0:
                centre = (w * xs).sum()
                c = (w * (xs - centre) ** 2).sum()
                if np.sqrt(c) > 0.001 * span:
                    w = w * ((x[i] - centre) / c * (xs - centre) + 1.0)
            fit[i] = (w * y[nleft:stop]).sum()
        if it == iters:
            break
        res = np.abs(y - fit)
        part = np.sort(res)
        cmad = 3.0 * (part[n // 2] + part[n - n // 2 - 1])
        if cmad < 1e-7 * res.mean():
            break
        with np.errstate(invalid="ignore"):                          # (cmad = 0: every residual is 0 and keeps weight 1)
            u = res / cmad
        rw = np.where(res <= 0.001 * cmad, 1.0, np.where(res <= 0.999 * cmad, (1.0 - u * u) ** 2, 0.0))
    return fit


NB_FILTER_THETAS = 50
NB_FILTER_UPPER = 0.95
NB_FILTER_LOWESS_F = 0.2


def independent_filtering(pvalue, base_mean, alpha=0.05):
    """DESeq2's ``pvalueAdjustment`` with independent filtering on the mean (Bourgon, Gentleman, Huber 2010; genefilter's
    ``filtered_p``), restated; numpy on the host, UNPINNED.  The filter statistic is ``base_mean`` (NaN reads as 0);
    ``lo = mean(filter == 0)``; ``theta`` = 50 points from lo to 0.95 (``[0]`` if lo >= 0.95); for each theta Benjamini-Hochberg runs
    over the genes with ``filter >= quantile(filter, theta)`` (linear interpolation, R's type 7) that have a p-value, and
    ``num_rej`` counts ``padj < alpha``.  If ``max(num_rej) <= 10`` the first column is taken; otherwise
    ``fit = lowess(theta, num_rej, f = 1/5)``, ``thresh = max(fit) - sqrt(mean(residual^2))`` over the columns with rejections,
    and the first column with ``num_rej > thresh`` (the first column if there is none).  Returns ``(padj, info)``: ``padj`` is NaN
    below the cutoff and without a p-value; ``info`` holds ``theta``, ``num_rej``, ``lowess`` (None if not fitted), ``chosen``
    and ``filter_threshold``."""
    p, mean = np.asarray(pvalue, dtype=np.float64), np.asarray(base_mean, dtype=np.float64)
    if p.ndim != 1 or p.shape != mean.shape or p.size < 1:
        raise ValueError("independent_filtering: pvalue %s and base_mean %s: one of each per gene" % (p.shape, mean.shape))
    if isinstance(alpha, (str, bytes, bool)) or not np.isscalar(alpha) or not 0 < alpha < 1:
        raise ValueError("independent_filtering: alpha=%r must be in (0, 1)" % (alpha,))
    filt = np.where(np.isnan(mean), 0.0, mean)
    lo = float(np.mean(filt == 0))
    theta = np.linspace(lo, NB_FILTER_UPPER, NB_FILTER_THETAS) if lo < NB_FILTER_UPPER else np.zeros(1)
    cutoffs = np.quantile(filt, theta)
    has_p = ~np.isnan(p)
    columns = np.full((theta.size, p.size), np.nan)
    for i, cut in enumerate(cutoffs):
        use = has_p & (filt >= cut)
        columns[i, use] = bh_adjust(p[use])
    with np.errstate(invalid="ignore"):
        num_rej = (columns < alpha).sum(axis=1)
    fit, chosen = None, 0
    if num_rej.max() > 10:
        fit = lowess(theta, num_rej.astype(np.float64), f=NB_FILTER_LOWESS_F)
        residual = (num_rej - fit)[num_rej > 0]
        thresh = fit.max() - np.sqrt(np.mean(residual ** 2))
        above = np.flatnonzero(num_rej > thresh)
        chosen = int(above[0]) if above.size else 0
    return columns[chosen].copy(), {"theta": theta, "num_rej": num_rej.astype(np.int64), "lowess": fit, "chosen": chosen,
                                    "filter_threshold": float(cutoffs[chosen])}


# ---- principal components (K15; scanpy's scale + tl.pca(svd_solver='arpack') of pilotpy's extract_annot_expression) ----------
PCA_MAX_COMPS = 64


def _pca_args(n, n_total, n_comps, scale, max_value, cols):
    """pca's arguments checked on the host: (n_comps, scale 0 / 1, max_value with None -> inf, cols int32 or None, columns)"""
    if cols is not None:
        cols = np.asarray(cols)
        if cols.ndim != 1 or (cols.size and cols.dtype.kind not in "iu"):
            raise ValueError("cols: a 1-D array of column indices, got %s %s" % (cols.shape, cols.dtype))
        if cols.size and (int(cols.min()) < 0 or int(cols.max()) >= n_total):
            raise ValueError("cols outside [0, %d)" % n_total)
        if np.unique(cols).size != cols.size:
            raise ValueError("cols names a column twice")
        cols = np.ascontiguousarray(cols, dtype=np.int32)
    n_sel = n_total if cols is None else cols.size
    if n < 2:
        raise ValueError("principal components need at least 2 rows, got %d" % n)
    cap = min(n - 1, n_sel - 1, PCA_MAX_COMPS)
    if isinstance(n_comps, bool) or int(n_comps) != n_comps or not 1 <= n_comps <= cap:
        raise ValueError("n_comps=%r outside [1, min(rows - 1, columns - 1, %d)] = [1, %d]" % (n_comps, PCA_MAX_COMPS, cap))
    if max_value is None:
        max_value = np.inf
    if isinstance(max_value, (str, bytes, bool)) or not np.isscalar(max_value) or not float(max_value) > 0.0:
        raise ValueError("max_value=%r must be positive (None: no clip)" % (max_value,))
    return int(n_comps), int(bool(scale)), float(max_value), cols, n_sel


def _pca_outputs(n, n_sel, k):
    return np.empty((n, k)), np.empty((n_sel, k)), np.empty(k), np.empty(k), np.zeros(2, dtype=np.int32)


def _pca_result(out, return_info):
    scores, pcs, variance, ratio, info = out
    steps, flags = int(info[0]), int(info[1])
    if return_info:
        return scores, pcs, variance, ratio, dict(steps=steps, flags=flags, converged=not flags & _lib.PCA_NOT_CONVERGED,
                                                  rank_deficient=bool(flags & _lib.PCA_RANK_DEFICIENT))
    if flags & _lib.PCA_RANK_DEFICIENT:
        raise ValueError("pca: the matrix has fewer than n_comps=%d principal directions (rank-deficient)" % scores.shape[1])
    if flags & _lib.PCA_NOT_CONVERGED:
        raise ValueError("pca: Lanczos did not converge in %d steps" % steps)
    return scores, pcs, variance, ratio


def pca(Y, n_comps=50, scale=True, max_value=10.0, cols=None, return_info=False):
    """K15: the principal components of the rows x columns matrix ``Y`` (include/pilot_ot.h, "principal components") -- scanpy's
    ``pp.scale(max_value)`` followed by ``tl.pca`` restated, without ever forming the standardised matrix.  ``Y``: a
    :class:`DeviceCSR` (forwarded to its own method), a C-contiguous float32 / float64 numpy array, a :class:`DeviceMatrix` or
    :func:`device_columns` of one.  ``scale``: every selected column is centred, divided by its ddof-1 standard deviation (0 -> 1)
    and clipped from above at ``max_value`` (None: no clip) first; False: the values as they are.  ``cols``: the selected columns,
    distinct, in any order (default: all).  Returns ``(scores, pcs, variance, variance_ratio)``, all float64: rows x n_comps,
    columns x n_comps, and two vectors of n_comps, largest variance first; in every component the score of largest magnitude is
    positive.  All arithmetic is float64 in a fixed order: a repeated call, and float32 / float64 uploads of the same values,
    return the same bits.  Every argument is checked before any device work (ValueError: fewer than 2 rows, ``n_comps`` outside
    ``[1, min(rows - 1, columns - 1, 64)]``, a column out of range or repeated, ``max_value`` not positive, a non-finite value
    of a host array).  A matrix with fewer than ``n_comps`` directions, or no verified convergence within the basis of
    min(columns, 1024) vectors (a repeated eigenvalue is found or the call says so), raises ValueError; with
    ``return_info`` nothing is raised and a fifth item, ``dict(steps, flags, converged, rank_deficient)``, tells."""
    if isinstance(Y, DeviceCSR):
        return Y.pca(n_comps=n_comps, scale=scale, max_value=max_value, cols=cols, return_info=return_info)
    Y = _dense_arg(Y, "Y", mode="strict")
    k, scale, max_value, cols, n_sel = _pca_args(Y.rows, Y.cols, n_comps, scale, max_value, cols)
    if not Y.on_dev and not np.isfinite(Y.keep if cols is None else Y.keep[:, cols]).all():
        raise ValueError("Y holds a non-finite value")
    out = _pca_outputs(Y.rows, n_sel, k)
    _lib.check(_lib.load().pilot_ot_pca(Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, Y.cols, Y.ld,
                                        None if cols is None else _lib.iptr(cols), n_sel, scale, max_value, k,
                                        *(_lib.dptr(a) for a in out[:4]), _lib.iptr(out[4])))
    return _pca_result(out, return_info)


# ---- cell neighbours (K16; scanpy's pp.neighbors of pilotpy's extract_annot_expression / reclustering_data) -------------------
KNN_MAX_K = _lib.KNN_ROWS_MAX_K


def _knn_k(k, what="k"):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= KNN_MAX_K:
        raise ValueError("%s=%r outside [1, %d]" % (what, k, KNN_MAX_K))
    return int(k)


def knn(X, k, metric="euclidean", rows=None):
    """K16: the exact ``k`` nearest neighbours of rows of the n x D matrix ``X`` among all its rows (include/pilot_ot.h, "cell
    neighbours"), by brute force on the device: the n x n distance matrix is never formed.  ``X``: a numpy array (a view with a
    unit column stride goes up as it is) or a :class:`DeviceMatrix`, float32 or float64; other dtypes convert to float64.
    ``metric``: ``"euclidean"`` or ``"cosine"`` (1 - cos, from unit rows).  ``rows=(begin, end)``: the query rows (default: all);
    the corpus is always all n rows.  Returns ``(indices int32 (m, k), distances float64 (m, k))``; a row is never its own
    neighbour (left out by index, so duplicates of it are neighbours at distance 0), and its neighbours are ordered by (distance,
    index) ascending.  Distances are direct sums of squared differences in X's dtype: every one is within (D + 6) u relative of the
    exact distance between the stored values (u = 2^-24 / 2^-53), far from the origin too, and a repeated call returns the same
    bits.  ValueError before any device work: ``k`` outside [1, 64], n < k + 1, an unknown metric, a bad row range; from the
    device's first pass: a non-finite value, or under cosine an all-zero row (the message names the row)."""
    Y = _dense_arg(X, "X", mode="strided", axes=" (rows x dims)")
    k = _knn_k(k)
    if metric not in _lib.ROW_METRICS:
        raise ValueError("metric=%r: %s" % (metric, " or ".join(_lib.ROW_METRICS)))
    n, D = Y.rows, Y.cols
    if D < 1:
        raise ValueError("X has no columns")
    if n < k + 1:
        raise ValueError("k=%d neighbours need at least k + 1 rows, got %d" % (k, n))
    if n > np.iinfo(np.int32).max:
        raise NotImplementedError("%d rows need more than 32-bit row indices" % n)
    begin, end = (0, n) if rows is None else rows
    if isinstance(begin, bool) or isinstance(end, bool) or int(begin) != begin or int(end) != end or not 0 <= begin < end <= n:
        raise ValueError("rows=%r: (begin, end) with 0 <= begin < end <= %d" % (rows, n))
    m = int(end) - int(begin)
    indices, distances = np.empty((m, k), dtype=np.int32), np.empty((m, k))
    _lib.check(_lib.load().pilot_ot_knn_rows(Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), n, D, Y.ld, _lib.ROW_METRICS[metric], k,
                                             int(begin), int(end), _lib.iptr(indices), _lib.dptr(distances)))
    return indices, distances


def _knn_graph_args(indices, distances, n_neighbors):
    distances = np.ascontiguousarray(distances, dtype=np.float64)
    if distances.ndim != 2 or isinstance(n_neighbors, bool) or not isinstance(n_neighbors, (int, np.integer)) \
            or distances.shape[1] != n_neighbors - 1:
        raise ValueError("distances %s: n x (n_neighbors - 1) with n_neighbors=%r" % (distances.shape, n_neighbors))
    _knn_k(distances.shape[1], "n_neighbors - 1")
    if distances.shape[0] < 1:
        raise ValueError("distances has no rows")
    if not (np.isfinite(distances).all() and (distances >= 0).all()):
        raise ValueError("distances must be finite and not negative")
    if indices is not None:
        indices = np.asarray(indices)
        if indices.shape != distances.shape or indices.dtype.kind not in "iu":
            raise ValueError("indices: integers of shape %s, got %s %s" % (distances.shape, indices.shape, indices.dtype))
        if indices.size and (indices.min() < 0 or indices.max() >= distances.shape[0]):
            raise ValueError("indices outside [0, %d): the graph needs every row's neighbours" % distances.shape[0])
    return indices, distances


def knn_smooth(distances, n_neighbors):
    """The per-row part of UMAP's fuzzy simplicial set on the device, in float64: ``distances`` n x (n_neighbors - 1) as
    :func:`knn` returns them (``n_neighbors`` counts the cell itself, as scanpy's does).  Returns ``(weights (n, n_neighbors - 1),
    sigma (n,), rho (n,))``: rho the smallest non-zero distance of the row (0: none), sigma from at most 64 bisection steps of
    ``sum_j exp(-max(0, d_j - rho) / sigma) = log2(n_neighbors)`` to 1e-5, floored at 1e-3 x the row's mean distance (rho = 0: x the
    mean of all distances), weights 1 where ``d_j <= rho`` or sigma = 0 and ``exp(-(d_j - rho) / sigma)`` otherwise."""
    _, distances = _knn_graph_args(None, distances, n_neighbors)
    n, k = distances.shape
    weights, sigma, rho = np.empty((n, k)), np.empty(n), np.empty(n)
    _lib.check(_lib.load().pilot_ot_knn_smooth(_lib.dptr(distances), n, k, _lib.dptr(weights), _lib.dptr(sigma), _lib.dptr(rho)))
    return weights, sigma, rho


def knn_connectivities(indices, distances, n_neighbors):
    """UMAP's symmetric connectivities of the whole graph ``(indices, distances)`` of :func:`knn`: the weights W of
    :func:`knn_smooth` placed at (i, indices[i, c]) give A, and the result is the fuzzy union A + A^T - A o A^T, an n x n scipy CSR
    matrix in float64, exactly symmetric (the union is formed on the host: it is O(n k))."""
    import scipy.sparse as sp
    indices, distances = _knn_graph_args(indices, distances, n_neighbors)
    weights = knn_smooth(distances, n_neighbors)[0]
    n, k = distances.shape
    A = sp.csr_matrix((weights.ravel(), indices.ravel().astype(np.int32), np.arange(0, n * k + 1, k)), shape=(n, n))
    At = A.T.tocsr()
    C = (A + At - A.multiply(At)).tocsr()
    C.eliminate_zeros()
    return C


# ---- Louvain communities (K17; sknetwork's Louvain of pilotpy's extract_annot_expression / reclustering_data, by a synchronous rule) --
def check_resolution(resolution):
    """ValueError unless ``resolution`` is what :func:`louvain` takes: a finite number, not negative"""
    if isinstance(resolution, bool) or not isinstance(resolution, (int, float, np.integer, np.floating)) \
            or not np.isfinite(resolution) or resolution < 0:
        raise ValueError("resolution=%r: a finite number, not negative" % (resolution,))


def _louvain_args(graph, resolution, tol, max_levels):
    """(indptr int64, indices int32, data float64, n) of the square graph, every argument judged: nothing touches the library"""
    import scipy.sparse as sp
    check_resolution(resolution)
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not tol >= 0:
        raise ValueError("tol=%r: a number, not negative" % (tol,))
    if isinstance(max_levels, bool) or not isinstance(max_levels, (int, np.integer)) or max_levels < 1:
        raise ValueError("max_levels=%r: an integer of at least 1" % (max_levels,))
    if sp.issparse(graph):
        A = graph.tocsr()
    else:
        A = np.asarray(graph) if graph is not None else np.empty(0)
        if A.ndim != 2 or A.dtype.kind not in "fiub":
            raise ValueError("graph: a scipy sparse matrix or a square 2-D array of numbers, got %s %s" % (A.shape, A.dtype))
        A = sp.csr_matrix(A)
    if A.shape[0] != A.shape[1]:
        raise ValueError("graph must be square, got %s" % (A.shape,))
    if A.dtype.kind not in "fiub":
        raise ValueError("graph: weights of dtype %s" % A.dtype)
    n = A.shape[0]
    if n > np.iinfo(np.int32).max:
        raise NotImplementedError("%d nodes need more than 32-bit node indices" % n)
    data = np.ascontiguousarray(A.data, dtype=np.float64)
    if data.size and not (np.isfinite(data).all() and data.min() >= 0):
        raise ValueError("graph: every weight must be finite and not negative")
    return np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int32), data, n


def _communities(symbol, keys, graph, resolution, tol, max_levels, return_info):
    """the call behind :func:`louvain` and :func:`leiden`: the library's ``symbol``, whose info counters are named by ``keys``"""
    indptr, indices, data, n = _louvain_args(graph, resolution, tol, max_levels)
    labels, q, info = np.empty(n, dtype=np.int32), ctypes.c_double(0.0), np.zeros(len(keys), dtype=np.int32)
    _lib.check(getattr(_lib.load(), symbol)(n, _lib.lptr(indptr), _lib.iptr(indices), _lib.dptr(data), float(resolution), float(tol),
                                            int(max_levels), _lib.iptr(labels), ctypes.byref(q), _lib.iptr(info)))
    return (labels, dict(zip(("modularity",) + keys, [q.value] + info.tolist()))) if return_info else labels


def louvain(graph, resolution=1.0, tol=1e-3, max_levels=32, return_info=False):
    """K17: the Louvain communities of a weighted graph on the device (include/pilot_ot.h, "Louvain communities"), by a
    SYNCHRONOUS rule: every node of a sweep chooses its move against the same snapshot, and a sweep is kept only if the modularity
    rose by more than ``tol``; deterministic, no seed, the same bits from every call.  It is not sknetwork's sequential sweep, so
    where the node order decides, the labels differ from sknetwork's; on clustered data the partitions agree.
    ``graph``: a scipy sparse matrix of any format or a square ndarray, weights finite and >= 0; it may be unsymmetric (the
    modularity is then Dugue and Perez's directed one at ``resolution``, as sknetwork's is; Newman's for a symmetric graph).
    Returns ``labels`` (int32, 0 .. k-1 by decreasing community size, ties to the smallest member); with ``return_info``
    ``(labels, dict(modularity, levels, sweeps, communities))``.  ValueError before any device work: a graph that is not square, a
    weight negative or not finite, ``resolution`` negative or not finite, ``tol < 0``, ``max_levels < 1``."""
    return _communities("pilot_ot_louvain", ("levels", "sweeps", "communities"), graph, resolution, tol, max_levels, return_info)


# ---- Leiden communities (K20; sc.tl.leiden of pilotpy's Clustering, clustering_emd and select_best_sil, by K17's synchronous rule) ---
def leiden(graph, resolution=1.0, tol=1e-3, max_levels=32, return_info=False):
    """K20: Leiden communities of a weighted graph on the device (include/pilot_ot.h, "Leiden communities"): every level is a
    level of :func:`louvain` followed by Leiden's refinement of its partition under the same synchronous rule, and the refined
    sub-communities become the next level's nodes.  EVERY RETURNED COMMUNITY IS CONNECTED in A + A^T, which :func:`louvain` does
    not promise; the modularity is about the same.  Deterministic, no seed, the same bits from every call.  It is
    not leidenalg: greedy where leidenalg draws at random, synchronous, and every level restarts from singletons, so the labels
    are not leidenalg's.  ``graph``, ``resolution``, ``tol``, ``max_levels``, the labels and the ValueErrors before any device
    work are :func:`louvain`'s; with ``return_info`` ``(labels, dict(modularity, levels, move_sweeps, refine_sweeps,
    communities))``."""
    return _communities("pilot_ot_leiden", ("levels", "move_sweeps", "refine_sweeps", "communities"), graph, resolution, tol, max_levels,
                        return_info)


def check_clustering_method(method):
    """the engine call ``method`` names (``"louvain"`` or ``"leiden"``); ValueError for anything else"""
    if method == "louvain":
        return louvain
    if method == "leiden":
        return leiden
    raise ValueError("method=%r: 'louvain' or 'leiden'" % (method,))


# ---- silhouette of labelled points (K18; the score pilotpy's select_best_sil takes per resolution, at the cell level) -------------
def silhouette_geometry(D, dtype=np.float32):
    """``(queries per block, corpus rows per staged tile)`` of :func:`silhouette_samples` for ``D`` columns of ``dtype``."""
    if np.dtype(dtype) not in (np.float32, np.float64):
        raise ValueError("dtype=%s: float32 or float64" % np.dtype(dtype).name)
    block, tile = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().pilot_ot_silhouette_points_geometry(int(D), _lib.dtype_code(np.dtype(dtype)), ctypes.byref(block),
                                                               ctypes.byref(tile)))
    return block.value, tile.value


def silhouette_samples(X, labels, metric="euclidean", return_score=False):
    """K18: ``sklearn.metrics.silhouette_samples(X, labels, metric=metric)`` of the C rows of the C x D matrix ``X`` on the device
    (include/pilot_ot.h, "silhouette of labelled rows"), without the C x C distance matrix and without a C x k table, so it works
    at the cell level where :func:`silhouette_of_rows` cannot.  ``X`` and ``metric`` are :func:`knn`'s, and so are the distances:
    direct sums of squared differences in X's dtype, never |x|^2 + |y|^2 - 2 x.y.  ``labels``: one per row, of any hashable type.
    With a_i the mean distance from i to the other members of its cluster (i is left out by index, so copies of it count at
    distance 0) and b_i the smallest mean distance to the members of another cluster, s_i = (b_i - a_i) / max(a_i, b_i), and
    0 where i's cluster has one member or max(a_i, b_i) = 0.  Returns the float64 array s, or ``(s, mean of s)`` with
    ``return_score``.  Every s_i is within 4 ((D + 6) u + C 2^-53) of the value the exact distances give (u = 2^-24 / 2^-53);
    sums are float64 in a fixed order, so a repeated call and the host and device routes return the same bits.  ValueError
    before any device work: a wrong label length, an unknown metric, no columns, a number of labels outside 2 .. C - 1; from the
    device's first pass: a non-finite value, or under cosine an all-zero row (the message names the row)."""
    Y = _dense_arg(X, "X", mode="strided", axes=" (rows x dims)")
    if metric not in _lib.ROW_METRICS:
        raise ValueError("metric=%r: %s" % (metric, " or ".join(_lib.ROW_METRICS)))
    n, D = Y.rows, Y.cols
    if D < 1:
        raise ValueError("X has no columns")
    codes, n_clusters = _label_codes(labels, n)
    if not 2 <= n_clusters <= n - 1:
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % n_clusters)
    if n > np.iinfo(np.int32).max:
        raise NotImplementedError("%d rows need more than 32-bit row indices" % n)
    samples, score = np.empty(n, dtype=np.float64), ctypes.c_double(0.0)
    _lib.check(_lib.load().pilot_ot_silhouette_points(Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), n, D, Y.ld, _lib.ROW_METRICS[metric],
                                                      _lib.iptr(codes), n_clusters, _lib.dptr(samples), ctypes.byref(score)))
    return (samples, score.value) if return_score else samples


def fitted_curves(params, model, times, noise=None, device=False):
    """One standardised curve per gene over ``times``: ``design(model[g], t) @ params[g]`` (``params``: G x 3 = Intercept, Treat,
    Treat2; ``model``: indices into :data:`TRAJFIT_MODELS`, or their names), plus, with ``noise`` (T x G per-time-point spreads,
    :func:`segment_std`'s output, numpy or :class:`DeviceMatrix`), ``noise[t, g] / 10 * (Treat + Treat2 - Intercept)`` with NaN
    sums set to 0; then scikit-learn's StandardScaler per gene (make_curves and the scaling of get_noised_curves,
    gene_selection_analysis.py:52-165).  Returns G x T float64 (a :class:`DeviceMatrix` with ``device=True``)."""
    params = _as_f64(params, "params")
    if params.ndim != 2 or params.shape[1] != 3:
        raise ValueError("params must be G x 3 (Intercept, Treat, Treat2), got %s" % (params.shape,))
    G = params.shape[0]
    model = np.ravel(np.asarray(model))
    if model.dtype.kind in "OUS":
        model = np.array([TRAJFIT_MODELS.index(str(m)) for m in model], dtype=np.int32)
    model = np.ascontiguousarray(model, dtype=np.int32)
    if model.size != G:
        raise ValueError("model has %d entries for %d genes" % (model.size, G))
    times = _as_f64(np.ravel(times), "times")
    T = times.size
    if noise is None:
        sp, s_dev = None, 0
    else:
        noise = _dense_arg(noise, "noise", (np.float64,))
        if (noise.rows, noise.cols) != (T, G):
            raise ValueError("noise must be T x G = %d x %d, got %d x %d" % (T, G, noise.rows, noise.cols))
        sp, s_dev = noise.ptr, noise.on_dev
    out, out_ptr = _result_matrix(G, T, device)
    _lib.check(_lib.load().pilot_ot_fitted_curves(_lib.dptr(params), _lib.iptr(model), G, _lib.dptr(times), T, sp, s_dev, out_ptr, int(device)))
    return out


def linkage_of_rows(Y, method="complete", return_info=False):
    """K11b: ``scipy.cluster.hierarchy.linkage(pdist(Y), method)`` of the rows of ``Y`` (G x T float64, numpy array or
    :class:`DeviceMatrix`) on the device, and ``pdist(Y).max()``: Euclidean distances in the direct form, the nearest-neighbour
    chain over the G x G matrix in HBM, scipy's ordering and labelling of Z.  Returns ``(Z, dmax)``; the distances never reach
    the host.  ``method``: single, complete, average or weighted; G at most ``_lib.LINKAGE_MAX_G`` (the matrix is G^2 x 8 bytes
    of HBM)."""
    if method in _LINKAGE_UNSUPPORTED:
        raise NotImplementedError("linkage method %r needs centroids: only %s run on the device" % (method, ", ".join(LINKAGE_METHODS)))
    if method not in _lib.LINKAGE_METHODS:
        raise ValueError("Invalid method: %r" % (method,))
    Y = _dense_arg(Y, "Y", (np.float64,))
    G, T = Y.rows, Y.cols
    if G < 2:
        raise ValueError("The number of observations cannot be determined on an empty distance matrix.")
    if G > _lib.LINKAGE_MAX_G:
        raise ValueError("G=%d rows: the G x G float64 distance matrix would take %.1f GiB of HBM; at most %d rows"
                         % (G, G * G * 8 / 2.0 ** 30, _lib.LINKAGE_MAX_G))
    if not Y.on_dev and not np.all(np.isfinite(Y.keep)):
        raise ValueError("Y contains NaN or inf")
    Z = np.empty((G - 1, 4), dtype=np.float64)
    dmax, steps = ctypes.c_double(0.0), ctypes.c_int(0)
    _lib.check(_lib.load().pilot_ot_linkage_of_rows(Y.ptr, Y.on_dev, G, T, _lib.LINKAGE_METHODS[method], _lib.dptr(Z), ctypes.byref(dmax),
                                                    ctypes.byref(steps)))
    if return_info:
        return Z, dmax.value, dict(chain_steps=steps.value)
    return Z, dmax.value


def flat_clusters(Z, t):
    """``scipy.cluster.hierarchy.fcluster(Z, t, 'distance')`` restated on the host (Z is small): a node whose height and whose
    descendants' heights are all <= t is one cluster; numbers are handed out depth-first from the root, left child first.
    The loop is scipy's cluster_monocrit (cluster/_hierarchy.pyx) step by step, so the numbering is scipy's."""
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim != 2 or Z.shape[1] != 4:
        raise ValueError("Z must be a (G - 1) x 4 linkage matrix, got %s" % (Z.shape,))
    n = Z.shape[0] + 1
    left, right = Z[:, 0].astype(np.int64), Z[:, 1].astype(np.int64)
    md = Z[:, 2].copy()                                   # the largest height in each node's subtree (children come first in Z)
    for i in range(n - 1):
        for c in (left[i], right[i]):
            if c >= n and md[c - n] > md[i]:
                md[i] = md[c - n]
    T = np.zeros(n, dtype=np.int32)
    if n == 1:
        T[0] = 1
        return T
    # scipy's cluster_monocrit: inner children first (left, then right), then the node's own leaves; a leaf outside every
    # cluster is a cluster of its own, numbered when its parent is finished
    nc, leader = 0, -1
    visited = np.zeros(n - 1, dtype=bool)
    stack = [n - 2]
    while stack:
        i = stack[-1]
        lc, rc = left[i], right[i]
        if leader == -1 and md[i] <= t:
            leader = i
            nc += 1
        if lc >= n and not visited[lc - n]:
            visited[lc - n] = True
            stack.append(lc - n)
            continue
        if rc >= n and not visited[rc - n]:
            visited[rc - n] = True
            stack.append(rc - n)
            continue
        for c in (lc, rc):
            if c < n:
                if leader == -1:
                    nc += 1
                T[c] = nc
        if leader == i:
            leader = -1
        stack.pop()
    return T


def curve_activities(curves, times):
    """G x 4 unrounded float64: terminal logFC, transient logFC, switching time and area of every row of ``curves`` (G x T
    float64, numpy array or :class:`DeviceMatrix`) over ``times`` (plot/curve_activity.py: median-of-three clamp, trapezoid
    rule).  ``times`` must be strictly increasing with at least two values (ValueError otherwise, as the reference)."""
    times = np.ascontiguousarray(np.ravel(times), dtype=np.float64)
    if times.size < 2 or not (times[1:] > times[:-1]).all():
        raise ValueError("times must be increasing and have at least 2 values.")
    curves = _dense_arg(curves, "curves", (np.float64,))
    G, T = curves.rows, curves.cols
    if T != times.size:
        raise ValueError("curves has %d columns for %d times" % (T, times.size))
    out = np.empty((G, 4), dtype=np.float64)
    _lib.check(_lib.load().pilot_ot_curve_activities(curves.ptr, curves.on_dev, G, T, _lib.dptr(times), _lib.dptr(out)))
    return out


# ---- elastic principal tree and pseudotime (K19; the two ElPiGraph calls of pilotpy's fit_pricipla_graph) ------------------------
TREE_MAX_NODES = _lib.ELASTIC_MAX_NODES - 1       # a tree of M nodes peaks at M + 1 while it grows
TREE_BAND = 1e-10                                 # candidates within this relative distance of the lowest energy are tied


def _points_arg(X):
    Y = _dense_arg(X, "X", mode="strided", axes=" (points x dims)")
    if not 1 <= Y.cols <= _lib.ELASTIC_MAX_D:
        raise ValueError("X has %d columns: the principal tree takes 1 to %d" % (Y.cols, _lib.ELASTIC_MAX_D))
    if Y.rows < 1:
        raise ValueError("X has no rows")
    if Y.rows > np.iinfo(np.int32).max:
        raise NotImplementedError("%d rows need more than 32-bit row indices" % Y.rows)
    return Y


def _points_call(fn, Y, *args):
    _lib.check(fn(Y.ptr, Y.on_dev, _lib.dtype_code(Y.dtype), Y.rows, Y.cols, Y.ld, *args))


def _fit_controls(max_iter, eps):
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError("max_iter=%r must be an integer >= 1" % (max_iter,))
    if not eps >= 0:
        raise ValueError("eps=%r must be >= 0" % (eps,))
    return int(max_iter), float(eps)


def point_moments(X):
    """``(mean (D,), cross (D, D))`` of the rows of ``X``: the column means and ``sum_i (x_i - mean)(x_i - mean)^T``, float64 sums
    in a fixed order on the device (include/pilot_ot.h, "elastic principal tree").  ``X`` as in :func:`principal_tree`."""
    Y = _points_arg(X)
    mean, cross = np.empty(Y.cols), np.empty((Y.cols, Y.cols))
    _points_call(_lib.load().pilot_ot_point_moments, Y, _lib.dptr(mean), _lib.dptr(cross))
    return mean, cross


def tree_springs(n_nodes, edges, lam=0.01, mu=0.1):
    """The m x m spring matrix of a tree: ``lam * v v^T`` per edge (a, b), v = e_a - e_b, plus ``mu * s s^T`` per node c of degree
    k >= 2, s = e_c - (1 / k) sum of e_l over c's neighbours l (in edge-list order)."""
    S = np.zeros((n_nodes, n_nodes))
    nb = [[] for _ in range(n_nodes)]
    for a, b in edges:
        v = np.zeros(n_nodes)
        v[a], v[b] = 1.0, -1.0
        S += lam * np.outer(v, v)
        nb[a].append(b)
        nb[b].append(a)
    for c, ls in enumerate(nb):
        if len(ls) >= 2:
            s = np.zeros(n_nodes)
            s[c] = 1.0
            s[ls] = -1.0 / len(ls)
            S += mu * np.outer(s, s)
    return S


ElasticFit = collections.namedtuple("ElasticFit", "nodes energy iters flags counts sums")


def _elastic_fit(Y, nodes, springs, centre, max_iter, eps):
    """:func:`elastic_fit` of a batch (B, m, D) / (B, m, m) with the singular flag left to the caller"""
    nodes, springs, centre = _as_f64(nodes, "nodes"), _as_f64(springs, "springs"), _as_f64(centre, "centre")
    if nodes.ndim != 3 or nodes.shape[0] < 1 or nodes.shape[2] != Y.cols:
        raise ValueError("nodes: (candidates, m, %d) expected, got %s" % (Y.cols, nodes.shape))
    B, m, D = nodes.shape
    if not 2 <= m <= _lib.ELASTIC_MAX_NODES:
        raise ValueError("m=%d nodes outside [2, %d]" % (m, _lib.ELASTIC_MAX_NODES))
    if springs.shape != (B, m, m):
        raise ValueError("springs: %s expected, got %s" % ((B, m, m), springs.shape))
    if centre.shape != (D,):
        raise ValueError("centre: %d values expected, got %s" % (D, centre.shape))
    max_iter, eps = _fit_controls(max_iter, eps)
    out = ElasticFit(np.empty((B, m, D)), np.empty((B, 2)), np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32),
                     np.empty((B, m), dtype=np.int32), np.empty((B, m, D)))
    _points_call(_lib.load().pilot_ot_elastic_fit_batch, Y, B, m, _lib.dptr(nodes), _lib.dptr(springs), _lib.dptr(centre), max_iter, eps,
                 _lib.dptr(out.nodes), _lib.dptr(out.energy), _lib.iptr(out.iters), _lib.iptr(out.flags), _lib.iptr(out.counts),
                 _lib.dptr(out.sums))
    return out


def elastic_fit(X, nodes, springs, centre, max_iter=10, eps=0.01):
    """K19: fit elastic graphs to the rows of ``X`` on the device (include/pilot_ot.h, "elastic principal tree").  ``nodes``
    (m, D) start positions and ``springs`` (m, m) the spring matrix (:func:`tree_springs`), or batches (B, m, D) / (B, m, m) fitted
    in one call; ``centre`` (D,): the point the change of a node is measured against (the data mean).  At most ``max_iter`` times:
    partition the points by nearest node (:func:`knn`'s distances in X's dtype, ties to the lowest node), solve
    ``(diag(cnt) / n + S) Y' = sum / n``, stop once ``max_j |Y'_j - Y_j| / |Y'_j - centre| < eps``.  Returns ``ElasticFit(nodes,
    energy, iters, flags, counts, sums)``: the fitted positions, ``energy[..., 0]`` the mean squared distance of the points to
    their nodes and ``energy[..., 1] = trace(Y^T S Y)``, the solves done, ``flags & 1`` converged, and the counts and sums of the
    final partition.  A candidate gives the same bits alone and in any batch.  ValueError: a bad shape, m outside [2, 65], D
    outside [1, 64], non-finite arguments, ``max_iter < 1``, ``eps < 0`` (all before any device work); a candidate whose system
    is singular (a pivot of the Cholesky factor was not positive; the message names the candidate)."""
    Y = _points_arg(X)
    nodes, springs = np.asarray(nodes, dtype=np.float64), np.asarray(springs, dtype=np.float64)
    single = nodes.ndim == 2
    fit = _elastic_fit(Y, nodes[None] if single else nodes, springs[None] if single and springs.ndim == 2 else springs, centre,
                       max_iter, eps)
    bad = np.flatnonzero(fit.flags & _lib.ELASTIC_SINGULAR)
    if bad.size:
        raise ValueError("elastic fit: the system of candidate %d is singular (a node without points and without springs?)" % bad[0])
    return ElasticFit(*(a[0] for a in fit)) if single else fit


def _tree_neighbours(m, edges):
    nb = [[] for _ in range(m)]
    for a, b in edges:
        nb[a].append(b)
        nb[b].append(a)
    return nb


def _drop_index(edges, gone, into=None):
    """the edge list with node ``gone`` replaced by ``into`` and every index above it shifted down"""
    def f(v):
        v = into if v == gone and into is not None else v
        return v - 1 if v > gone else v
    return [(f(a), f(b)) for a, b in edges]


def _grow_candidates(nodes, edges, counts, sums):
    """every tree one node larger, in the listed order: an edge bisected, then a node attached to every node"""
    m = len(nodes)
    nb = _tree_neighbours(m, edges)
    out = []
    for i, (a, b) in enumerate(edges):
        e = list(edges)
        e[i] = (a, m)
        e.append((m, b))
        out.append((np.vstack([nodes, 0.5 * (nodes[a] + nodes[b])]), e, "bisect edge %d" % i))
    for v in range(m):
        if len(nb[v]) == 1:
            y = 2.0 * nodes[v] - nodes[nb[v][0]]
        elif counts[v] > 0:
            y = sums[v] / counts[v]
        else:
            y = nodes[nb[v]].mean(axis=0)
        out.append((np.vstack([nodes, y]), list(edges) + [(v, m)], "attach to node %d" % v))
    return out


def _shrink_candidates(nodes, edges):
    """every tree one node smaller, in the listed order: an edge contracted, then a leaf deleted"""
    m = len(nodes)
    nb = _tree_neighbours(m, edges)
    out = []
    for i, (a, b) in enumerate(edges):
        keep, gone = min(a, b), max(a, b)
        y = nodes.copy()
        y[keep] = 0.5 * (nodes[a] + nodes[b])
        out.append((np.delete(y, gone, axis=0), _drop_index(edges[:i] + edges[i + 1:], gone, keep), "contract edge %d" % i))
    for v in range(m):
        if len(nb[v]) == 1:
            rest = [e for e in edges if v not in e]
            out.append((np.delete(nodes, v, axis=0), _drop_index(rest, v), "delete leaf %d" % v))
    return out


def principal_tree(X, n_nodes=20, lam=0.01, mu=0.1, max_iter=10, eps=0.01, return_info=False):
    """K19: the elastic principal tree of the rows of ``X`` (Albergante et al., Entropy 2020; what ElPiGraph's
    ``computeElasticPrincipalTree(X, n_nodes)`` fits), grown on the host and fitted on the device.  ``X``: n x D, D <= 64, a numpy
    array or a :class:`DeviceMatrix`, float32 or float64 (other dtypes convert to float64); it goes up once.  The tree starts as
    two nodes at ``mean -/+ sqrt(w) v`` for the leading eigenpair (w, v) of the covariance (v's largest entry positive) and grows
    by the grammar *grow, grow, shrink* until it has ``n_nodes`` nodes (3 to 64).  A grow step tries every edge bisected and a node
    attached to every node; a shrink step every edge contracted and every leaf deleted; all candidates of a step are fitted in one
    :func:`elastic_fit` batch and the lowest-listed one whose energy (mean squared distance + ``trace(Y^T S Y)``) is within
    1e-10 relative of the lowest wins -- candidates of the same topology reach the same optimum and tie to rounding.  Returns
    ``(nodes float64 (n_nodes, D), edges int32 (n_nodes - 1, 2))``; with ``return_info`` also a dict: ``steps``, ``candidates``
    (fitted per step), ``winners`` (index per step), ``energy`` (of the winner per step, the last one the tree's) and ``labels``.
    The same call returns the same bits.  ValueError: bad arguments (before any device work), all points coincide, a non-finite
    value in X (names the row), a candidate with a singular system (names the step and the candidate)."""
    Y = _points_arg(X)
    if isinstance(n_nodes, bool) or not isinstance(n_nodes, (int, np.integer)) or not 3 <= n_nodes <= TREE_MAX_NODES:
        raise ValueError("n_nodes=%r outside [3, %d]" % (n_nodes, TREE_MAX_NODES))
    if not (np.isfinite(lam) and np.isfinite(mu) and lam >= 0 and mu >= 0):
        raise ValueError("lam=%r, mu=%r must be finite and >= 0" % (lam, mu))
    max_iter, eps = _fit_controls(max_iter, eps)
    n = Y.rows
    if n < 2:
        raise ValueError("a principal tree needs at least 2 points, got %d" % n)
    if not Y.on_dev:
        Y = _dense_arg(DeviceMatrix.upload(Y.keep), "X")
    centre, cross = point_moments(Y.keep)
    w, V = np.linalg.eigh(cross / (n - 1))
    w, v = w[-1], V[:, -1]
    if not w > 0:
        raise ValueError("all points coincide: there is no direction to start the tree along")
    v = v if v[np.argmax(np.abs(v))] > 0 else -v
    half = np.sqrt(w) * v

    def fit(cands, step):
        B = len(cands)
        springs = np.stack([tree_springs(len(c[0]), c[1], lam, mu) for c in cands])
        res = _elastic_fit(Y, np.stack([c[0] for c in cands]), springs, centre, max_iter, eps)
        bad = np.flatnonzero(res.flags & _lib.ELASTIC_SINGULAR)
        if bad.size:
            raise ValueError("principal tree: step %d, candidate %d (%s): its system is singular" % (step, bad[0], cands[bad[0]][2]))
        E = res.energy.sum(axis=1)
        win = int(np.flatnonzero(E <= E.min() * (1.0 + TREE_BAND))[0])
        info["candidates"].append(B)
        info["winners"].append(win)
        info["energy"].append(float(E[win]))
        info["labels"].append(cands[win][2])
        return res.nodes[win], cands[win][1], res.counts[win], res.sums[win]

    info = {"candidates": [], "winners": [], "energy": [], "labels": []}
    nodes, edges, counts, sums = fit([(np.stack([centre - half, centre + half]), [(0, 1)], "start")], 0)
    step = 0
    while len(nodes) < n_nodes:
        for grow in (True, True, False):
            step += 1
            cands = _grow_candidates(nodes, edges, counts, sums) if grow else _shrink_candidates(nodes, edges)
            nodes, edges, counts, sums = fit(cands, step)
    edges = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    info["steps"] = step
    return (nodes, edges, info) if return_info else (nodes, edges)


def tree_orientation(nodes, edges, source=0):
    """``(oriented edges int32 (E, 2), base float64 (m,))`` of a tree: every edge as (a, b) with a the end nearer ``source``, in
    the order given, and the tree distance from ``source`` to every node (a host walk).  ValueError unless the edges form a tree
    on the m nodes and ``source`` is one of them."""
    nodes = _as_f64(nodes, "nodes")
    if nodes.ndim != 2 or not 2 <= nodes.shape[0] <= _lib.ELASTIC_MAX_NODES:
        raise ValueError("nodes: (m, D) with 2 <= m <= %d expected, got %s" % (_lib.ELASTIC_MAX_NODES, nodes.shape))
    m = nodes.shape[0]
    edges = np.asarray(edges)
    if edges.shape != (m - 1, 2) or not np.issubdtype(edges.dtype, np.integer) or edges.min() < 0 or edges.max() >= m:
        raise ValueError("edges: %d pairs of node indices in [0, %d) expected" % (m - 1, m))
    if isinstance(source, bool) or not isinstance(source, (int, np.integer)) or not 0 <= source < m:
        raise ValueError("source=%r is not a node index in [0, %d)" % (source, m))
    nb = [[] for _ in range(m)]
    for e, (a, b) in enumerate(edges):
        nb[a].append((int(b), e))
        nb[b].append((int(a), e))
    base = np.full(m, np.nan)
    base[source] = 0.0
    oriented = np.array(edges, dtype=np.int32)
    stack = [int(source)]
    while stack:
        a = stack.pop()
        for b, e in nb[a]:
            if np.isnan(base[b]):
                base[b] = base[a] + np.sqrt(((nodes[b] - nodes[a]) ** 2).sum())
                oriented[e] = (a, b)
                stack.append(b)
    if np.isnan(base).any():
        raise ValueError("edges: not a tree (node %d is not connected to the source)" % int(np.flatnonzero(np.isnan(base))[0]))
    return oriented, base


def tree_pseudotime(X, nodes, edges, source=0):
    """K19: every row of ``X`` onto its nearest edge of the tree ``(nodes, edges)`` and its pseudotime from node ``source`` (what
    ElPiGraph's ``getPseudotime`` gives), on the device in float64.  Returns ``(pseudotime, d2, edge, t)``, one entry per row: with
    (a, b) = ``tree_orientation(nodes, edges, source)[0][edge]`` the projection is ``y_a + t (y_b - y_a)``, t clipped to [0, 1],
    ``d2`` its squared distance from the row (the smallest over the edges, ties to the lowest edge) and
    ``pseudotime = dist(source, a) + t |y_b - y_a|``.  ValueError before any device work: bad shapes, edges that are no tree, a bad
    ``source``; from the device's first pass: a non-finite value in X (names the row)."""
    Y = _points_arg(X)
    oriented, base = tree_orientation(nodes, edges, source)
    nodes = _as_f64(nodes, "nodes")
    if nodes.shape[1] != Y.cols:
        raise ValueError("nodes have %d columns, X has %d" % (nodes.shape[1], Y.cols))
    n = Y.rows
    oriented = np.ascontiguousarray(oriented, dtype=np.int32)
    pt, d2, edge, t = np.empty(n), np.empty(n), np.empty(n, dtype=np.int32), np.empty(n)
    _points_call(_lib.load().pilot_ot_tree_projection, Y, nodes.shape[0], _lib.dptr(nodes), len(oriented), _lib.iptr(oriented),
                 _lib.dptr(base), _lib.dptr(pt), _lib.dptr(d2), _lib.iptr(edge), _lib.dptr(t))
    return pt, d2, edge, t
