"""The grid call's bookkeeping between calls: a plan holds two control blocks, an ordinary call works on one while its prep
kernel zeroes the other for the call after it, and no call starts with a memset.  Whatever a plan ran before -- a call that
left its hand-over and NaN counters non-zero, a row selection, a rejected call, an empty row range, a call sent to the
POT-literal kernel, graph capture and replay -- every call must return, array for array and bit for bit, what the same call
returns as the FIRST call of a fresh plan, and must write every output of the rows it was asked for.

Shapes: N = 48, K = 50 (four row-tiles, the one-wave path for the diagonal) and N = 40, K = 14 (one row-tile); K = 130 for the
wide kernel's call, which keeps its memset and its one block.  The references are computed once, each on a plan of its own."""
import functools

import numpy as np
import pytest

from pilot_amd import _lib, engine
from pilot_amd.synthetic import make_problem

pytestmark = pytest.mark.gpu

SHAPES = {"n48_k50": dict(n_patients=48, n_types=50, n_dims=30, seed=11, cells_per_patient=3000),
          "n40_k14": dict(n_patients=40, n_types=14, n_dims=30, seed=12, cells_per_patient=3000),
          "n40_k130": dict(n_patients=40, n_types=130, n_dims=30, seed=13, cells_per_patient=3000)}
SENT = -7

# a call: (reg, run() keywords); None stands for the call that is rejected for a bad argument
FULL_01 = (0.1, ())
FULL_001 = (0.01, ())                  # max(M)/reg = 100: pairs are handed to the tracking pass and on, the counters end non-zero
ROWS_1_3 = (0.1, (("row_begin", 1), ("row_step", 3)))
EMPTY = (0.1, (("row_begin", 5), ("row_end", 5)))
SEQUENCE = (FULL_01, FULL_001, FULL_01, ROWS_1_3, None, FULL_01)


@functools.lru_cache(maxsize=None)
def problem(shape):
    P, M = make_problem(**SHAPES[shape])
    assert np.array_equal(M, M.T)
    return P, M


def n_rows_of(plan, kw):
    kw = dict(kw)
    return engine.n_rows_of(plan.N, kw.get("row_begin", 0), kw.get("row_end", plan.N), kw.get("row_step", 1))


def fill_sentinels(plan):
    n = plan.N * plan.N
    for ptr, dtype in ((plan.dE, np.float64), (plan.dErr, np.float64), (plan.dIt, np.int32), (plan.dFl, np.int32)):
        a = np.full(n, SENT, dtype=dtype)
        _lib.check(plan.L.pilot_ot_memcpy_h2d(ptr, a.ctypes.data, a.nbytes))


def call(plan, spec, precision):
    """One call behind fresh sentinels: (emd, iters, err, flags) of the rows it was asked for."""
    reg, kw = spec
    fill_sentinels(plan)
    plan.run(reg, precision=precision, **dict(kw))
    plan.sync()
    E, info = plan.fetch(n_rows_of(plan, kw))
    return E, info["iters"], info["err"], info["flags"]


@functools.lru_cache(maxsize=None)
def fresh(shape, spec, precision):
    """The call as the first call of a plan of its own."""
    plan = engine.DevicePlan(*problem(shape))
    out = call(plan, spec, precision)
    plan.close()
    for a in out:
        a.setflags(write=False)
    return out


def check(out, shape, spec, precision, what):
    ref = fresh(shape, spec, precision)
    for name, a, r in zip(("emd", "iters", "err", "flags"), out, ref):
        assert a.shape == r.shape
        if name in ("iters", "flags"):
            assert not np.any(a == SENT), "%s: %s keeps a sentinel" % (what, name)
        else:
            assert not np.any(a == float(SENT)), "%s: %s keeps a sentinel" % (what, name)
        assert np.array_equal(a, r), "%s: %s differs from the fresh plan's" % (what, name)


def rejected(plan, precision):
    with pytest.raises(ValueError, match="reg"):
        plan.run(-1.0, precision=precision)


@pytest.mark.parametrize("precision", ["f16x2", "auto"])
@pytest.mark.parametrize("shape", ["n48_k50", "n40_k14"])
def test_reused_plan_returns_what_a_fresh_plan_returns(shape, precision):
    plan = engine.DevicePlan(*problem(shape))
    for i, spec in enumerate(SEQUENCE):
        if spec is None:
            rejected(plan, precision)
        else:
            check(call(plan, spec, precision), shape, spec, precision, "call %d" % i)
    plan.close()


def test_the_small_reg_call_leaves_its_counters_behind():
    """The sequence is only a test while its second call hands pairs over: at reg 0.01 pairs must have left the fast path
    (tau-absorptions tracked, pairs solved again in f64), which their flags show; at reg 0.1 none does."""
    for shape in ("n48_k50", "n40_k14"):
        handed = _lib.FLAG_ABSORBED | _lib.FLAG_F64 | _lib.FLAG_NAN
        assert np.any(fresh(shape, FULL_001, "auto")[3] & handed)
        assert not np.any(fresh(shape, FULL_01, "auto")[3] & handed)


@pytest.mark.parametrize("precision", ["f16x2", "auto"])
@pytest.mark.parametrize("shape", ["n48_k50", "n40_k14"])
def test_graph_mode_returns_what_a_fresh_plan_returns(shape, precision):
    """pilot_ot_plan_enable_graph: of three identical calls the first runs as usual, the second is captured, the third replayed."""
    plan = engine.DevicePlan(*problem(shape))
    plan.enable_graph(True)
    for i, spec in enumerate(SEQUENCE):
        for rep in range(3):
            if spec is None:
                rejected(plan, precision)
            else:
                check(call(plan, spec, precision), shape, spec, precision, "call %d, repeat %d" % (i, rep))
    plan.enable_graph(False)
    check(call(plan, FULL_01, precision), shape, FULL_01, precision, "after graph mode")
    check(call(plan, FULL_001, precision), shape, FULL_001, precision, "after graph mode, small reg")
    plan.close()


@pytest.mark.parametrize("shape", ["n48_k50", "n40_k14"])
def test_empty_row_range_and_generic_call_between_ordinary_calls(shape):
    plan = engine.DevicePlan(*problem(shape))
    check(call(plan, FULL_001, "auto"), shape, FULL_001, "auto", "first")
    E = call(plan, EMPTY, "auto")[0]
    assert E.shape == (0, plan.N)
    check(call(plan, FULL_01, "auto"), shape, FULL_01, "auto", "after the empty call")
    check(call(plan, FULL_01, "generic"), shape, FULL_01, "generic", "the POT-literal call")
    check(call(plan, FULL_01, "auto"), shape, FULL_01, "auto", "after the POT-literal call")
    check(call(plan, ROWS_1_3, "generic"), shape, ROWS_1_3, "generic", "the POT-literal call on a row selection")
    check(call(plan, FULL_001, "auto"), shape, FULL_001, "auto", "last")
    plan.close()


def test_wide_call_before_and_after_an_ordinary_call():
    """128 < K <= 256 with a symmetric cost runs the wide kernel's call, which keeps its own memset and control block."""
    wide, plan = engine.DevicePlan(*problem("n40_k130")), engine.DevicePlan(*problem("n48_k50"))
    check(call(wide, FULL_01, "auto"), "n40_k130", FULL_01, "auto", "wide, first")
    check(call(plan, FULL_01, "auto"), "n48_k50", FULL_01, "auto", "ordinary")
    check(call(wide, FULL_01, "auto"), "n40_k130", FULL_01, "auto", "wide, second")
    check(call(wide, ROWS_1_3, "auto"), "n40_k130", ROWS_1_3, "auto", "wide, row selection")
    check(call(plan, FULL_01, "auto"), "n48_k50", FULL_01, "auto", "ordinary, second")
    wide.close()
    plan.close()
