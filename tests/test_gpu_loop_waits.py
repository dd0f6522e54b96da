"""The pair-grid kernel's loop around the update block: a refill whose loads are waited for where they are first used (a last
row-tile with one live slot loaded as that slot alone, the reload behind the parked cost flush in one block), and a refill that
outruns the wave's batch of 16 work items and draws the next batch in the same iteration.  None of it may change a bit, lose a
pair or write one that was not asked for.

Every case runs behind sentinels in all four outputs, must leave none (every pair written), stays within the f32-class tolerance
of the fp64 oracle, and returns the same bits with one and with two resident workgroups per CU (other waves, other batches,
other slot mates) and as the two row shards 0::2 and 1::2 (other queues altogether).  What this cannot see: a pair handed to
two columns is written twice with the same bits, and no output counts writes; an item handed out twice shows only through
the item it displaced, which keeps its sentinel.

Shapes: the smallest at which the touched paths run.  The launch has min(CUs x workgroups per CU, tiles / 4) workgroups of four
waves, and a wave's first batch is dealt statically, so a wave draws a second batch -- and a refill can take items of two batches
in one iteration, the new hand-out -- only where the batches of 16 outnumber the waves severalfold: N = 300 (5 607 batches behind
the diagonal, against at most 1 024 waves at one workgroup per CU and 2 048 at two on 256 CUs), at K = 50 with the symmetric cost
(the headline's kernel) and at K = 33 with a non-symmetric one (three row-tiles, LDS image).  Both cases assert that count, replay
the queue on the update counts the GPU returned (tools/queue_replay.py) and require refills that span two batches there; their
shards run at one workgroup per CU as well, where 2 804 batches still outnumber the waves.  In the N <= 40 cases below the waves outnumber the batches: every wave takes its static batch and finds the
queue empty at its one draw, which is the exhaustion path, the partial last batch (N = 33: 1 089 pairs = 68 batches and one item)
and, at fewer than three row-tiles, the unchanged feed.  K = 50 is the headline's kernel (four row-tiles, one live slot in the last,
operand image in registers), K = 64 four full row-tiles, K = 33 three row-tiles with the 16-wide tail k-block in update and
flush, K = 14 the sharded queue at four workgroups per CU; a non-symmetric cost takes the LDS image; reg 0.01 hands pairs to the
tracking pass (two exponent bands); N = 5 has fewer pairs than one batch per wave; a repeated row puts off-diagonal duplicates at
the head of the queue.  In every reg-0.1 case some pair ends at its first error test (21 updates) and some run past 41, so refills
and flushes fall on different iterations of a wave (checked below on the update counts the GPU returns; with the oracle at the
GPU's stopping floor of 8 f32 ulps the counts are 252 / 64 of 1 089 at K = 50, 571 / 37 at K = 64, 199 / 94 at K = 33, 113 / 743
of 1 600 at K = 14, 4 / 7 of 25 at N = 5, 81 / 20 of 289 with the repeated row).  At reg 0.01 no pair ends at 21: there the fast
pass refills when it hands a pair over."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import account_for_absorb_on_last
from oracle import oracle as O
from pilot_amd import _lib, engine
from pilot_amd.synthetic import make_problem

pytestmark = pytest.mark.gpu

TOL32 = 1e-5
SENT = -7
DBG_WGS_SHIFT = 4          # PILOT_OT_DEBUG bits 4..6: resident workgroups per CU of the fast launch


def _problem(N, K, seed, asym=False, repeat=None):
    P, M = make_problem(N, K, 30, seed=seed, cells_per_patient=3000)
    if asym:                # (the cohort's own cost, bent: a uniform random cost converges at the first or second test everywhere)
        M = M * (1.0 + 0.2 * np.random.default_rng(seed).random((K, K)))
        M /= M.max()
        assert not np.array_equal(M, M.T)
    if repeat:
        P[repeat[1]] = P[repeat[0]]
    return P, M


#        name: (N, K, seed, reg, keywords of _problem)
CASES = {"n33_k50": (33, 50, 11, 0.1, {}),
         "n33_k64": (33, 64, 12, 0.1, {}),
         "n33_k33": (33, 33, 13, 0.1, {}),
         "n40_k14": (40, 14, 14, 0.1, {}),
         "n33_k50_asym": (33, 50, 15, 0.1, dict(asym=True)),
         "n33_k50_reg001": (33, 50, 11, 0.01, {}),
         "n5_k50": (5, 50, 17, 0.1, {}),
         "n17_k50_repeat": (17, 50, 18, 0.1, dict(repeat=(2, 9))),
         "n300_k50": (300, 50, 19, 0.1, {}),
         "n300_k33_asym": (300, 33, 20, 0.1, dict(asym=True))}
MAX_CUS = 256              # MI355X; fewer CUs mean fewer waves, which only helps the batches outnumber them


def spanning_refills(P, iters, n_waves, rows=slice(None)):
    """Refills that take items of two batches in one iteration, by the CPU replay of the queue on these update counts."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "queue_replay.py")
    spec = importlib.util.spec_from_file_location("queue_replay", path)
    qr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(qr)
    off = ~np.eye(P.shape[0], dtype=bool)            # (the diagonal runs on waves of its own at this size)
    key = qr.l1_bucket_key(P)[rows][off[rows]]
    r = qr.replay(iters[rows][off[rows]], qr.order_of(key), n_waves=n_waves)
    return r["spans"], r["later_draws"]


@functools.lru_cache(maxsize=None)
def case(name):
    N, K, seed, reg, kw = CASES[name]
    P, M = _problem(N, K, seed, **kw)
    Eo, io = O.sinkhorn_grid(P, M, reg, n_threads=16, return_info=True)
    for a in (P, M, Eo, io["iters"], io["flags"]):
        a.setflags(write=False)
    return P, M, reg, Eo, io


def run(plan, reg, **rows):
    """One call behind fresh sentinels: (emd, iters, err, flags) of the rows asked for, none of them a sentinel."""
    n = plan.N * plan.N
    for ptr, dtype in ((plan.dE, np.float64), (plan.dErr, np.float64), (plan.dIt, np.int32), (plan.dFl, np.int32)):
        a = np.full(n, SENT, dtype=dtype)
        _lib.check(plan.L.pilot_ot_memcpy_h2d(ptr, a.ctypes.data, a.nbytes))
    plan.run(reg, precision="auto", **rows)
    plan.sync()
    n_rows = engine.n_rows_of(plan.N, rows.get("row_begin", 0), rows.get("row_end", plan.N), rows.get("row_step", 1))
    E, info = plan.fetch(n_rows)
    out = (E, info["iters"], info["err"], info["flags"])
    for name, a in zip(("emd", "iters", "err", "flags"), out):
        assert a.shape == (n_rows, plan.N)
        assert not np.any(a == SENT), "%s keeps a sentinel: %d pairs were never written" % (name, int(np.sum(a == SENT)))
    return out


def same_bits(got, ref, what):
    for name, a, r in zip(("emd", "iters", "err", "flags"), got, ref):
        assert np.array_equal(a, r), "%s: %s differs" % (what, name)


@pytest.mark.parametrize("name", list(CASES))
def test_every_pair_once_and_the_same_bits_under_other_schedules(name, switches):
    P, M, reg, Eo, io = case(name)
    N, K = P.shape
    plan = engine.DevicePlan(P, M)
    full = run(plan, reg)
    E, it, _, fl = full
    last_o, last_g = (io["flags"] & O.FLAG_ABSORB_ON_LAST) > 0, (fl & _lib.FLAG_ABSORB_LAST) > 0
    print("%s: max|gpu - oracle| %.3e, updates gpu %.1f / oracle %.1f per pair, at 21: %d, past 41: %d of %d"
          % (name, np.abs(E - Eo)[~(last_o | last_g)].max(), it.mean(), io["iters"].mean(), int((it == 21).sum()), int((it > 41).sum()), it.size))
    account_for_absorb_on_last(E, Eo, last_g, last_o, K, TOL32, max_one_sided_frac=1e-4)
    assert np.all(it <= io["iters"])                      # POT's check or an earlier one (the f32 stopping floor)
    if reg == 0.1:
        assert np.any(it == 21) and np.any(it > 41)       # refills and flushes at different phases of a wave
    else:
        assert np.any(fl & (_lib.FLAG_ABSORBED | _lib.FLAG_F64))      # pairs left the fast pass
    big = N >= 300
    if big:
        for wgs, rows in ((1, slice(None)), (2, slice(None)), (1, slice(0, None, 2)), (1, slice(1, None, 2))):
            n = it[rows].size - it[rows].shape[0]
            batches, waves = (n + 15) // 16, MAX_CUS * wgs * 4
            assert batches > waves, "%d batches do not outnumber %d waves" % (batches, waves)
            spans, later = spanning_refills(P, it, waves, rows)
            print("%s, rows %s: %d workgroup(s) per CU: %d batches, %d waves; replay: %d refills span two batches, %d later draws"
                  % (name, rows, wgs, batches, waves, spans, later))
            assert spans > 0 and later > 0
    for wgs in (1, 2):
        switches.setenv("PILOT_OT_DEBUG", str(wgs << DBG_WGS_SHIFT))
        same_bits(run(plan, reg), full, "%d resident workgroup(s) per CU" % wgs)
        if big and wgs == 1:
            for r in (0, 1):
                same_bits(run(plan, reg, row_begin=r, row_step=2), tuple(a[r::2] for a in full), "row shard %d::2 at one workgroup per CU" % r)
    switches.delenv("PILOT_OT_DEBUG")
    for r in (0, 1):
        part = run(plan, reg, row_begin=r, row_step=2)
        same_bits(part, tuple(a[r::2] for a in full), "row shard %d::2" % r)
    plan.close()
