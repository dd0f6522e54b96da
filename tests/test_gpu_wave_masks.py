"""The fp16-split pair-grid kernel's two per-column flags -- `active` (the column iterates a pair) and `want` (it asks for one) -- as
64-bit wave masks (profiles/r11/wave_masks.md).  A mask is updated at wave-uniform level from ballots; a per-lane view of it that
outlives such an update is stale, and the kernel that reads it counts a column in a batch's ranks without giving it its item: pairs
are never written.  Outputs that were written by an earlier call hide that, so every call here runs behind fresh sentinels in all four
outputs (the method of tests/test_gpu_loop_waits.py::run) and none may survive.

`precision="f16x2"` is forced throughout: with "auto" the cases of test_gpu_loop_waits.py never take the hand-over paths of the
fp16-split kernel, which are where the flags change outside the retire block.

(a) 48 x 50 at reg 0.05, 48 x 17 at reg 0.06, 64 x 2 at reg 0.1 (make_problem(N, K, 30, seed=7), the inputs of
    tests/test_gpu_loop_control.py: 693 / 934 / 1 297 pairs absorbed on the fp64 oracle, 50 / 53 capped in the first two): hand-over,
    capped and converged columns in one wave.  Every pair written; |E - E_oracle| <= 1e-5 away from the pairs whose absorb-on-last
    flag differs from the oracle's (at most 5 %); update counts 1 mod 20 below the cap.
(b) the same three with one and with two resident workgroups per CU and as the row shards 0::2 and 1::2: bit-identical to the full grid.
(c) 300 x 50 at reg 0.05 at one workgroup per CU: waves hold several batches, the hand-over buffer flushes inside the launch, refills,
    hand-overs and retirements fall into the same iteration.  No oracle (it would take seconds): no sentinel, iters >= 1, emd finite
    where the flags carry no NaN, the bits of a second call and of the two row shards.
(d) 5 x 50 and 17 x 50 with one repeated row at reg 0.1: fewer pairs than one batch per wave, columns go dark at the first draw while
    their neighbours run.  No sentinel, the bits of the two row shards.

The hand_all_over path (histograms of unequal mass: every column that takes a pair asks for the next one in the refill block itself) is
driven with "f16x2" by tests/test_gpu_loop_stalls.py::test_oracle_parity_and_the_same_bits_as_two_shards[n48_k50_unequal], full grid and
both shards; nothing is added for it here."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from pilot_amd import _lib, engine
from pilot_amd.synthetic import make_problem

pytestmark = pytest.mark.gpu

TOL32 = 1e-5
SENT = -7
DBG_WGS_SHIFT = 4          # PILOT_OT_DEBUG bits 4..6: resident workgroups per CU of the fast launch
NAMES = ("emd", "iters", "err", "flags")

#          name: (N, K, reg, absorbed on the oracle, capped on the oracle; None: not stated)
COHORTS = {"n48_k50_reg0.05": (48, 50, 0.05, 693, 50),
           "n48_k17_reg0.06": (48, 17, 0.06, 934, 53),
           "n64_k2_reg0.1": (64, 2, 0.1, 1297, None)}
#        name: (N, K, seed, repeated row or None)      (the inputs of test_gpu_loop_waits.py's n5_k50 and n17_k50_repeat)
SMALL = {"n5_k50": (5, 50, 17, None),
         "n17_k50_repeat": (17, 50, 18, (2, 9))}


@functools.lru_cache(maxsize=None)
def cohort(name):
    N, K, reg, _, _ = COHORTS[name]
    P, M = make_problem(N, K, 30, seed=7)
    Eo, io = O.sinkhorn_grid(P, M, reg, n_threads=16, return_info=True)
    for a in (P, M, Eo, io["iters"], io["flags"]):
        a.setflags(write=False)
    return P, M, reg, Eo, io


def run(plan, reg, **rows):
    """One "f16x2" call behind fresh sentinels: (emd, iters, err, flags) of the rows asked for, none of them a sentinel."""
    n = plan.N * plan.N
    for ptr, dtype in ((plan.dE, np.float64), (plan.dErr, np.float64), (plan.dIt, np.int32), (plan.dFl, np.int32)):
        a = np.full(n, SENT, dtype=dtype)
        _lib.check(plan.L.pilot_ot_memcpy_h2d(ptr, a.ctypes.data, a.nbytes))
    plan.run(reg, precision="f16x2", **rows)
    plan.sync()
    n_rows = engine.n_rows_of(plan.N, rows.get("row_begin", 0), rows.get("row_end", plan.N), rows.get("row_step", 1))
    E, info = plan.fetch(n_rows)
    out = (E, info["iters"], info["err"], info["flags"])
    for name, a in zip(NAMES, out):
        assert a.shape == (n_rows, plan.N)
        assert not np.any(a == SENT), "%s keeps a sentinel: %d pairs were never written" % (name, int(np.sum(a == SENT)))
    return out


def same_bits(got, ref, what):
    for name, a, r in zip(NAMES, got, ref):
        assert np.array_equal(a, r, equal_nan=name in ("emd", "err")), "%s: %s differs" % (what, name)


def shards_same_bits(plan, reg, full, what):
    for r in (0, 1):
        same_bits(run(plan, reg, row_begin=r, row_step=2), tuple(a[r::2] for a in full), "row shard %d::2, %s" % (r, what))


@pytest.mark.parametrize("name", list(COHORTS))
def test_every_pair_written_and_oracle_parity(name):
    P, M, reg, Eo, io = cohort(name)
    plan = engine.DevicePlan(P, M)
    E, it, _, fl = run(plan, reg)
    plan.close()
    absorbed_o, capped_o = (io["flags"] & O.FLAG_ABSORBED) > 0, io["iters"] >= engine.NUM_ITER_MAX
    print("%s: oracle absorbed %d, capped %d of %d" % (name, int(absorbed_o.sum()), int(capped_o.sum()), it.size))
    assert int(absorbed_o.sum()) == COHORTS[name][3]              # (the input is the one this file's docstring describes)
    if COHORTS[name][4] is not None:
        assert int(capped_o.sum()) == COHORTS[name][4]
    edge = ((io["flags"] & O.FLAG_ABSORB_ON_LAST) > 0) != ((fl & _lib.FLAG_ABSORB_LAST) > 0)
    fin = np.isfinite(Eo)
    capped = it == engine.NUM_ITER_MAX
    print("%s: max|gpu - oracle| %.3e, edge share %.4f, gpu absorbed %d, at the cap %d, not 1 mod 20 below it: %d"
          % (name, np.abs(E - Eo)[fin & ~edge].max(), edge.mean(), int(((fl & _lib.FLAG_ABSORBED) > 0).sum()), int(capped.sum()),
             int((it[~capped] % 20 != 1).sum())))
    assert np.isfinite(E[fin]).all() and edge.mean() < 0.05
    assert np.abs(E - Eo)[fin & ~edge].max() <= TOL32
    assert np.all(it[~capped] % 20 == 1)


@pytest.mark.parametrize("name", list(COHORTS))
def test_same_bits_at_one_and_two_workgroups_per_cu_and_as_shards(name, switches):
    N, K, reg, _, _ = COHORTS[name]
    P, M = make_problem(N, K, 30, seed=7)
    plan = engine.DevicePlan(P, M)
    full = run(plan, reg)
    shards_same_bits(plan, reg, full, "default launch")
    for wgs in (1, 2):
        switches.setenv("PILOT_OT_DEBUG", str(wgs << DBG_WGS_SHIFT))
        what = "%d resident workgroup(s) per CU" % wgs
        same_bits(run(plan, reg), full, what)
        shards_same_bits(plan, reg, full, what)
    switches.delenv("PILOT_OT_DEBUG")
    plan.close()


def test_several_batches_per_wave_at_one_workgroup_per_cu(switches):
    P, M = make_problem(300, 50, 30, seed=7)
    plan = engine.DevicePlan(P, M)
    switches.setenv("PILOT_OT_DEBUG", str(1 << DBG_WGS_SHIFT))
    full = run(plan, 0.05)
    E, it, _, fl = full
    print("n300_k50_reg0.05: updates %.1f per pair, absorbed %d, NaN-flagged %d, at the cap %d of %d"
          % (it.mean(), int(((fl & _lib.FLAG_ABSORBED) > 0).sum()), int(((fl & _lib.FLAG_NAN) > 0).sum()),
             int((it == engine.NUM_ITER_MAX).sum()), it.size))
    assert np.all(it >= 1)
    assert np.isfinite(E[(fl & _lib.FLAG_NAN) == 0]).all()
    same_bits(run(plan, 0.05), full, "second call")
    shards_same_bits(plan, 0.05, full, "one workgroup per CU")
    switches.delenv("PILOT_OT_DEBUG")
    plan.close()


@pytest.mark.parametrize("name", list(SMALL))
def test_columns_that_go_dark_at_the_first_draw(name):
    N, K, seed, repeat = SMALL[name]
    P, M = make_problem(N, K, 30, seed=seed, cells_per_patient=3000)
    if repeat:
        P[repeat[1]] = P[repeat[0]]
    plan = engine.DevicePlan(P, M)
    full = run(plan, 0.1)
    shards_same_bits(plan, 0.1, full, "default launch")
    plan.close()
