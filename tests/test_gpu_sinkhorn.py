"""Parity of the HIP Sinkhorn pair grid (through the C ABI) against the CPU oracle.  GPU only.

Tolerances (BASELINE.json north star): |EMD_gpu - EMD_oracle|_inf <= 1e-5 in f32, <= 1e-12 in f64."""
import numpy as np
import pytest

from conftest import GOLDEN_CASES, account_for_absorb_on_last, load_golden
from oracle import oracle as O
from pilot_amd import _lib, engine
from pilot_amd.synthetic import CONFIGS, make_problem

pytestmark = pytest.mark.gpu
TOL32, TOL64 = 1e-5, 1e-12


def test_device_is_gfx950():
    assert _lib.device_count() >= 1
    assert "gfx950" in _lib.device_name()


def test_pot_docstring_known_answers_through_the_c_abi():
    """ot.sinkhorn2([.5, .5], [.5, .5], [[0, 1], [1, 0]], 1) = 0.26894142 and ot.emd2(...) = 0.0 (POT docstrings)."""
    P = np.array([[0.5, 0.5], [0.5, 0.5], [1.0, 0.0], [0.0, 1.0]])
    M = np.array([[0.0, 1.0], [1.0, 0.0]])
    for prec, tol in (("fp32", 1e-6), ("bf16x3", 1e-6), ("f16x2", 1e-6), ("fp64", 5e-9)):
        E = engine.sinkhorn_grid(P, M, 1.0, precision=prec)
        assert abs(E[0, 1] - 0.26894142) < tol and abs(E[0, 0] - 0.26894142) < tol
    X = engine.emd_grid(P, M)
    assert X[0, 1] == 0.0 and X[2, 3] == 1.0 and X[3, 2] == 1.0 and X[2, 2] == 0.0


@pytest.mark.parametrize("cfg,step", [("c1", 1), ("c2", 5), ("c3", 40)])
@pytest.mark.parametrize("reg", [1.0, 0.1])
def test_parity_f32_and_f64(cfg, step, reg):
    P, M = make_problem(**CONFIGS[cfg])
    Eo, io = O.sinkhorn_grid(P, M, reg, row_step=step, n_threads=16, return_info=True)
    E32, i32 = engine.sinkhorn_grid(P, M, reg, precision="fp32", row_step=step, return_info=True)
    E64, i64 = engine.sinkhorn_grid(P, M, reg, precision="fp64", row_step=step, return_info=True)
    # precision "auto" at these regs (max(M)/reg <= 16) = f32 values iterated with fp16-split products (PILOT_OT_PREC_F16X2)
    Es, isp = engine.sinkhorn_grid(P, M, reg, precision="auto", row_step=step, return_info=True)
    np.testing.assert_array_equal(Es, engine.sinkhorn_grid(P, M, reg, precision="f16x2", row_step=step))
    assert np.abs(Es - Eo).max() <= TOL32
    # the bf16-split configuration (AUTO for 16 < max(M)/reg <= 60) on the same problem
    Eb, ib = engine.sinkhorn_grid(P, M, reg, precision="bf16x3", row_step=step, return_info=True)
    assert np.abs(Eb - Eo).max() <= TOL32 and (ib["iters"] == i32["iters"]).mean() > 0.98
    assert np.all(isp["iters"] <= io["iters"]) and np.all(isp["iters"] % 20 == 1) and np.all((isp["flags"] & _lib.FLAG_F64) == 0)
    # same stopping decisions as the f32 MFMA path, up to rounding at knife-edge checks
    assert (isp["iters"] == i32["iters"]).mean() >= 0.97
    assert np.abs(E32 - Eo).max() <= TOL32
    assert np.abs(E64 - Eo).max() <= TOL64
    # f64 follows POT's control flow update for update
    np.testing.assert_array_equal(i64["iters"], io["iters"])
    assert np.all((i64["flags"] & _lib.FLAG_CONVERGED) == (io["flags"] & O.FLAG_CONVERGED))
    assert np.all((i64["flags"] & _lib.FLAG_F64) > 0) and np.all((i32["flags"] & _lib.FLAG_F64) == 0)
    # f32 stops at an earlier check when the true error is below its stop-threshold floor, never later
    assert np.all(i32["iters"] <= io["iters"]) and np.all(i32["iters"] % 20 == 1)
    np.testing.assert_allclose(i64["err"], io["err"], rtol=1e-3, atol=1e-13)


def test_small_reg_goes_through_absorption_tracking_f64():
    """reg = 0.01: every pair tau-absorbs, ~half hit the 1000-update cap; the f64 kernel must follow the
    oracle's iteration semantics exactly, including POT's absorb-on-the-final-update scaling."""
    P, M = make_problem(**CONFIGS["c3"])
    rows = dict(row_begin=275, row_end=276, row_step=1)             # contains two known absorb-on-last pairs
    Eo, io = O.sinkhorn_grid(P, M, 0.01, n_threads=16, return_info=True, **rows)
    Eg, ig = engine.sinkhorn_grid(P, M, 0.01, precision="fp64", return_info=True, **rows)
    assert np.all((ig["flags"] & _lib.FLAG_F64) > 0)
    assert np.abs(Eg - Eo).max() <= 1e-9
    np.testing.assert_array_equal(ig["iters"], io["iters"])
    hit_o = (io["flags"] & O.FLAG_ABSORB_ON_LAST) > 0
    hit_g = (ig["flags"] & _lib.FLAG_ABSORB_LAST) > 0
    assert hit_o.sum() >= 2
    np.testing.assert_array_equal(hit_g, hit_o)
    assert ((ig["flags"] & _lib.FLAG_ABSORBED) > 0).mean() > 0.9
    capped = io["iters"] == 1000
    assert 0.2 < capped.mean() < 0.9


def test_small_reg_f32_stays_within_tolerance_on_this_distribution(switches):
    """The raw f32-input MFMA kernel at max(M)/reg = 100 (outside its range; normal calls run AUTO_MIXED there)."""
    switches.setenv("PILOT_OT_RAW_PRECISION", "1")
    P, M = make_problem(**CONFIGS["c3"])
    rows = dict(row_begin=100, row_end=102, row_step=1)
    Eo, io = O.sinkhorn_grid(P, M, 0.01, n_threads=16, return_info=True, **rows)
    Eg, ig = engine.sinkhorn_grid(P, M, 0.01, precision="fp32", return_info=True, **rows)
    ok = (io["flags"] & O.FLAG_ABSORB_ON_LAST) == 0
    same = ig["iters"] == io["iters"]
    # capped pairs ran the same 1000 updates; converged pairs may stop a check early
    assert np.abs(Eg - Eo)[ok & same].max() <= TOL32
    assert np.abs(Eg - Eo)[ok].max() <= 1e-4
    assert not np.isnan(Eg).any()


@pytest.mark.parametrize("K", [1, 2, 7, 31, 32, 33, 48, 64, 65, 96, 100, 128])
@pytest.mark.parametrize("prec,tol", [("fp32", TOL32), ("bf16x3", TOL32), ("f16x2", TOL32), ("fp64", TOL64)])
def test_every_tile_shape(K, prec, tol):
    """K sweeps the row-tile counts (f32: 32 rows per tile, f64: 16) incl. padding edges; N=37 is not a
    multiple of the 32 / 16 pairs a wave handles."""
    P, M = make_problem(37, K, 8, seed=100 + K, cells_per_patient=400)
    if K == 1:
        M = np.zeros((1, 1))
    Eo = O.sinkhorn_grid(P, M, 0.2, n_threads=16)
    Eg = engine.sinkhorn_grid(P, M, 0.2, precision=prec)
    assert Eg.shape == (37, 37)
    assert np.abs(Eg - Eo).max() <= tol


@pytest.mark.parametrize("K", [130, 200])
def test_k_above_128_runs_the_reference_semantics_kernel(K):
    """The reference has no limit on the number of cell types (Trajectory.py:479-523).  Asked for fp64 (or POT-literal)
    arithmetic, or outside the fp16-split range, a grid beyond the single-wave MFMA kernels' 128 runs POT's loop literally in
    fp64 (generic_kernels.hpp) and must follow the oracle update for update."""
    P, M = make_problem(9, K, 4, seed=K, cells_per_patient=2000)
    Eo, io = O.sinkhorn_grid(P, M, 0.1, n_threads=16, return_info=True)
    Eg, ig = engine.sinkhorn_grid(P, M, 0.1, return_info=True, precision="fp64")
    assert np.abs(Eg - Eo).max() <= 1e-12
    np.testing.assert_array_equal(ig["iters"], io["iters"])
    assert np.all((ig["flags"] & _lib.FLAG_F64) > 0)
    part = engine.sinkhorn_grid(P, M, 0.1, row_begin=2, row_end=7, row_step=3, precision="fp64")
    np.testing.assert_array_equal(part, Eg[2:7:3])
    Eo2 = O.sinkhorn_grid(P, M, 0.04, n_threads=16)                      # max(M)/reg = 25: outside the fp16-split range
    assert np.abs(engine.sinkhorn_grid(P, M, 0.04) - Eo2).max() <= 1e-12
    # exact mode up to 256 cell types (cost matrix read from L2 instead of LDS)
    assert np.abs(engine.emd_grid(P, M) - O.emd_grid(P, M, n_threads=16)).max() <= 1e-12


@pytest.mark.parametrize("K", [113, 120, 128])
def test_k_113_to_128_runs_four_waves_per_tile(K, switches):
    """112 < K <= 128 (8 row-tiles), symmetric cost, fp16-split range: sinkhorn_quad_kernel (quad_kernels.hpp) -- a tile's cell types spread over
    four waves, the operand image in registers, the costs formed inside the kernel -- takes the place of the one-wave-per-tile
    stream kernel's fast pass (PILOT_OT_NO_QUAD: that kernel).  f32-class tolerance against the fp64 oracle, the f32 stopping rule
    (the oracle's check or an earlier one), the two kernels agree (same update counts but for pairs at the stop floor), shard / full
    identity bit for bit, duplicate patients, a partially filled last ring, and hand-overs: a small tau sends pairs to the tracking
    kernel, which must return the oracle's values for them."""
    N = 75
    P, M = make_problem(N, K, 6, seed=K, cells_per_patient=3000)
    P[7] = P[3]                                                          # duplicate patients: the slowest pairs
    Eo, io = O.sinkhorn_grid(P, M, 0.1, n_threads=16, return_info=True)
    Eq, iq = engine.sinkhorn_grid(P, M, 0.1, return_info=True)
    assert np.isfinite(Eq).all() and np.abs(Eq - Eo).max() <= TOL32
    assert np.all(iq["iters"] <= io["iters"]) and np.all(iq["iters"] % 20 == 1)
    assert int(((iq["flags"] & _lib.FLAG_F64) > 0).sum()) == 0
    switches.setenv("PILOT_OT_NO_QUAD", "1")
    Es, is_ = engine.sinkhorn_grid(P, M, 0.1, return_info=True)          # one wave per tile
    switches.delenv("PILOT_OT_NO_QUAD")
    assert np.abs(Eq - Es).max() <= 2e-6 and (iq["iters"] == is_["iters"]).mean() > 0.98
    for rb, re_, rs in ((0, N, 7), (5, 6, 1), (3, N, 11)):
        part = engine.sinkhorn_grid(P, M, 0.1, row_begin=rb, row_end=re_, row_step=rs)
        np.testing.assert_array_equal(part, Eq[rb:re_:rs])
    np.testing.assert_array_equal(engine.sinkhorn_grid(P, M, 0.1), Eq)   # deterministic
    assert np.abs(engine.sinkhorn_grid(P, M, 1.0) - O.sinkhorn_grid(P, M, 1.0, n_threads=16)).max() <= TOL32
    if K not in (113, 128):
        return
    for tau in (40.0, 6.0):
        Et, it_ = engine.sinkhorn_grid(P, M, 0.1, tau=tau, return_info=True)
        Eot, iot = O.sinkhorn_grid(P, M, 0.1, tau=tau, n_threads=16, return_info=True)
        last_o, last_g = (iot["flags"] & O.FLAG_ABSORB_ON_LAST) > 0, (it_["flags"] & _lib.FLAG_ABSORB_LAST) > 0
        account_for_absorb_on_last(Et, Eot, last_g, last_o, K, TOL32, max_one_sided_frac=2e-3)
        absorbed_o = (iot["flags"] & O.FLAG_ABSORBED) > 0
        assert (((it_["flags"] & _lib.FLAG_ABSORBED) > 0) != absorbed_o).mean() < 0.01
    assert absorbed_o.sum() > 0                                          # (at tau = 6 some pair does absorb)


@pytest.mark.parametrize("K", [129, 130, 160, 192, 250, 256])
def test_k_129_to_256_runs_eight_waves_per_tile(K, switches):
    """128 < K <= 256, symmetric cost, max(M)/reg <= 16: sinkhorn_wide_kernel (wide_kernels.hpp) -- the fp16-split products with
    a tile's cell types spread over the eight waves of a workgroup -- instead of one workgroup per pair (round 3: 600x slower
    than K = 128).  f32-class tolerance against the fp64 oracle, the f32 stopping rule (same or an earlier check), shard /
    full identity bit for bit, the diagonal included; pairs it hands over (tau) come back from the POT-literal kernel."""
    N = 40
    P, M = make_problem(N, K, 6, seed=K, cells_per_patient=3000)
    P[7] = P[3]                                                          # duplicate patients: the slowest pairs
    Eo, io = O.sinkhorn_grid(P, M, 0.1, n_threads=16, return_info=True)
    Eg, ig = engine.sinkhorn_grid(P, M, 0.1, return_info=True)
    assert np.isfinite(Eg).all() and np.abs(Eg - Eo).max() <= TOL32
    f64 = (ig["flags"] & _lib.FLAG_F64) > 0
    assert f64.mean() < 0.2                                              # (hand-overs only)
    assert np.all(ig["iters"][~f64] <= io["iters"][~f64]) and np.all(ig["iters"][~f64] % 20 == 1)
    for rb, re_, rs in ((0, N, 7), (5, 6, 1), (3, N, 11)):
        part = engine.sinkhorn_grid(P, M, 0.1, row_begin=rb, row_end=re_, row_step=rs)
        np.testing.assert_array_equal(part, Eg[rb:re_:rs])
    np.testing.assert_array_equal(engine.sinkhorn_grid(P, M, 0.1), Eg)   # deterministic
    # reg 1.0 (few updates) and a tau that makes many pairs hand over
    assert np.abs(engine.sinkhorn_grid(P, M, 1.0) - O.sinkhorn_grid(P, M, 1.0, n_threads=16)).max() <= TOL32
    if K not in (130, 256):
        return
    switches.setenv("PILOT_OT_WIDE_CHUNK", "300")                     # row chunks of 7 rows (the 1 GB cap of the records, forced)
    np.testing.assert_array_equal(engine.sinkhorn_grid(P, M, 0.1), Eg)
    switches.delenv("PILOT_OT_WIDE_CHUNK")
    for tau in (2.0, 1.2):
        Et, it_ = engine.sinkhorn_grid(P, M, 0.1, tau=tau, return_info=True)
        Eot, iot = O.sinkhorn_grid(P, M, 0.1, tau=tau, n_threads=16, return_info=True)
        edge = ((iot["flags"] & O.FLAG_ABSORB_ON_LAST) > 0) | ((it_["flags"] & _lib.FLAG_ABSORB_LAST) > 0)
        assert np.abs(Et - Eot)[~edge].max() <= TOL32
        absorbed = (it_["flags"] & _lib.FLAG_ABSORBED) > 0
        assert np.all((it_["flags"][absorbed] & _lib.FLAG_F64) > 0)      # absorbing pairs were handed to the POT-literal kernel
    assert absorbed.sum() > 0                                            # (at tau = 1.2 some pair does absorb)


@pytest.mark.parametrize("K,N", [(113, 101), (129, 81), (113, 1), (128, 3), (129, 4), (256, 8)])
def test_four_and_eight_wave_kernels_draw_batches_from_the_queue(K, N):
    """The pair feed of sinkhorn_quad_kernel and sinkhorn_wide_kernel (split_tile.hpp): a workgroup's first batch of 16 pairs is
    the one of its own number, the later ones come from the device-wide counter through LDS.  Premise: 256 CUs, so quad launches
    at most 512 workgroups and wide at most 256, one tile each per draw.  (113, 101): 10 201 pairs, 638 tiles, a last batch of 9
    (drawn up to 318 CUs); (129, 81): 6 561 pairs, 411 tiles, a last batch of 1 (drawn up to 410 CUs).  Their row subsets are
    served by static batches only, so subset / full identity ties the two feed paths together.  The small grids are the other
    end: fewer pairs than one tile (1, 9) and exact multiples of 16 (16, 64).  In the oracle every pair of these grids converges
    (at most 61 updates) and none absorbs, so no pair is excluded from the tolerance."""
    P, M = make_problem(N, K, 6, seed=K, cells_per_patient=3000)
    if N > 7:
        P[7] = P[3]                                                      # duplicate patients: the slowest pairs
    Eo, io = O.sinkhorn_grid(P, M, 0.1, n_threads=16, return_info=True)
    Eg, ig = engine.sinkhorn_grid(P, M, 0.1, return_info=True)
    f64 = (ig["flags"] & _lib.FLAG_F64) > 0
    print("K %d N %d: max|E - Eo| %.3e, iters max %d (oracle %d), f64 share %.4f"
          % (K, N, np.abs(Eg - Eo).max(), ig["iters"].max(), io["iters"].max(), f64.mean()))
    assert Eg.shape == (N, N) and np.abs(Eg - Eo).max() <= TOL32
    assert np.all(ig["iters"] % 20 == 1) and np.all(ig["iters"] <= io["iters"])
    assert f64.sum() == 0 if K <= 128 else f64.mean() < 0.2
    Er, ir = engine.sinkhorn_grid(P, M, 0.1, return_info=True)
    np.testing.assert_array_equal(Er, Eg)                                # deterministic
    np.testing.assert_array_equal(ir["iters"], ig["iters"])
    for rb, rs in ((0, 7), (3, 11)):
        if rb < N:
            np.testing.assert_array_equal(engine.sinkhorn_grid(P, M, 0.1, row_begin=rb, row_end=N, row_step=rs), Eg[rb:N:rs])


def test_generic_kernel_is_pot_literal_including_absorption_and_tiny_reg():
    """precision='generic' forces the reference-semantics kernel on any shape: same update counts, absorption flags and
    errors as the oracle at reg 0.01 (every pair absorbs, some on their last update); and a reg whose exp(-M/reg) leaves the
    f64 range (max(M)/reg = 1000) is solved through the rebuilt absorbed kernel instead of returning NaN."""
    P, M = make_problem(**CONFIGS["c1"])
    for reg, kw in ((0.1, {}), (0.01, {}), (0.05, dict(tau=30.0)), (1e-3, {})):
        Eo, io = O.sinkhorn_grid(P, M, reg, n_threads=16, return_info=True, **kw)
        Eg, ig = engine.sinkhorn_grid(P, M, reg, precision="generic" if reg > 2e-3 else "auto", return_info=True, **kw)
        assert np.isfinite(Eg).all()
        np.testing.assert_array_equal(ig["iters"], io["iters"])
        for bit in (1, 2, 4, 8):
            np.testing.assert_array_equal(ig["flags"] & bit, io["flags"] & bit)
        assert np.abs(Eg - Eo).max() <= 1e-10, (reg, np.abs(Eg - Eo).max())
        np.testing.assert_allclose(ig["err"], io["err"], rtol=1e-6, atol=1e-13)
    assert ((io["flags"] & 8) > 0).mean() > 0.9          # at reg 1e-3 nearly every pair absorbs


@pytest.mark.parametrize("K,sym", [(40, False), (64, True), (21, True), (100, True)])
def test_small_reg_two_exponent_bands_other_shapes(K, sym):
    """precision='auto' beyond the f32 range (max(M)/reg = 90): f32 values with the Gibbs kernel in two exponent bands --
    non-symmetric costs (both operand forms get a second band), K mod 16 in 1..4 (dead registers skipped), a K whose two
    bands do not fit LDS (100: falls back to the f64 kernel).  Every pair within the f32 tolerance of the fp64 oracle."""
    rng = np.random.default_rng(K)
    P, M = make_problem(24, K, 8, seed=K, cells_per_patient=500)
    if not sym:
        M = rng.random((K, K)); M /= M.max()
    reg = 1.0 / 90.0
    Eo, io = O.sinkhorn_grid(P, M, reg, n_threads=16, return_info=True)
    Eg, ig = engine.sinkhorn_grid(P, M, reg, precision="auto", return_info=True)
    last = ((io["flags"] & O.FLAG_ABSORB_ON_LAST) > 0) | ((ig["flags"] & _lib.FLAG_ABSORB_LAST) > 0)
    assert np.isfinite(Eg).all()
    assert np.abs(Eg - Eo)[~last].max() <= TOL32
    assert np.all(ig["iters"] <= io["iters"])
    f64 = (ig["flags"] & _lib.FLAG_F64) > 0
    assert f64.all() if K == 100 else f64.mean() < 0.2


def test_pairs_that_go_nan_are_resolved_like_pot(switches):
    """POT breaks out of a pair whose scalings become NaN and returns the cost of the last good iterate.  The
    fast kernels hand such pairs to the POT-literal kernel instead of writing NaN: forcing the f32 kernel far outside its
    range (max(M)/reg = 400: exp(-M/reg) underflows in f32) must leave no NaN behind, and every pair that was handed over
    (flag F64) must carry the oracle's value, update count and flags."""
    P, M = make_problem(**CONFIGS["c1"])
    Eo, io = O.sinkhorn_grid(P, M, 0.0025, n_threads=16, return_info=True)
    # (an explicit f32-class precision beyond max(M)/reg = 60 normally runs AUTO_MIXED: the raw kernels are forced here)
    switches.setenv("PILOT_OT_RAW_PRECISION", "1")
    for prec in ("fp32", "bf16x3", "f16x2"):
        Eg, ig = engine.sinkhorn_grid(P, M, 0.0025, precision=prec, return_info=True)
        assert not np.isnan(Eg).any()
        redone = (ig["flags"] & _lib.FLAG_F64) > 0
        assert redone.any()
        assert np.abs(Eg - Eo)[redone].max() <= 1e-10
        np.testing.assert_array_equal(ig["iters"][redone], io["iters"][redone])
        np.testing.assert_array_equal((ig["flags"] & 15)[redone], (io["flags"] & 15)[redone])


@pytest.mark.parametrize("prec,tol", [("fp32", TOL32), ("bf16x3", TOL32), ("f16x2", TOL32), ("fp64", TOL64)])
def test_nonsymmetric_cost(prec, tol):
    rng = np.random.default_rng(4)
    P, _ = make_problem(20, 40, 6, seed=9, cells_per_patient=300)
    M = rng.random((40, 40))
    M /= M.max()
    assert not np.array_equal(M, M.T)
    Eo = O.sinkhorn_grid(P, M, 0.3, n_threads=16)
    Eg = engine.sinkhorn_grid(P, M, 0.3, precision=prec)
    assert np.abs(Eg - Eo).max() <= tol


@pytest.mark.parametrize("K,cap", [(48, 40), (64, 40), (50, 1000)])
def test_unequal_masses_do_not_run_in_the_scaled_fp16_domain(K, cap):
    """Histograms of unequal mass (never PILOT's proportions, but the ABI takes any P): u grows and v shrinks by the mass
    ratio at every update and the shrinking panel leaves the range in which two fp16 pieces hold 22 bits long before tau is
    reached (fuzz: 1.1e-5 / 2.4e-5 off at 40 capped updates, reg 1).  The prep kernel flags such a P and the fp16 pass only
    forwards its pairs to the tracking kernel: f32 tolerance again, and the equal-mass rows of the same call too."""
    rng = np.random.default_rng(K + cap)
    P = rng.dirichlet(np.ones(K), size=40)
    P[:30] *= rng.uniform(0.5, 2.0, size=(30, 1))
    _, M = make_problem(40, K, 6, seed=K, cells_per_patient=300)
    for reg in (1.0, 0.3):
        Eo, io = O.sinkhorn_grid(P, M, reg, n_threads=16, return_info=True, numItermax=cap)
        Eg, ig = engine.sinkhorn_grid(P, M, reg, return_info=True, num_iter_max=cap)
        fin = np.isfinite(Eo)
        edge = ((io["flags"] & O.FLAG_ABSORB_ON_LAST) > 0) != ((ig["flags"] & _lib.FLAG_ABSORB_LAST) > 0)
        assert np.isfinite(Eg[fin]).all() and edge.mean() < 0.05
        assert np.abs(Eg - Eo)[fin & ~edge].max() <= TOL32 * max(1.0, np.abs(Eo[fin]).max())


@pytest.mark.parametrize("K", [10, 30, 50, 64])
def test_register_image_and_lds_image_give_the_same_bits(K):
    """fp16-split configuration: with a symmetric cost and K <= 64 the operand image lives in registers and the four
    accumulator chains are interleaved; declared non-symmetric, the same matrix goes through the LDS image (two forms, tile
    after tile).  Every tile's MFMA sequence is the same, so off the diagonal (duplicates take the one-wave path only in
    the symmetric launch) the two must agree bit for bit, update counts included."""
    P, M = make_problem(60, K, 8, seed=7 * K, cells_per_patient=300)
    N = P.shape[0]
    L = _lib.load()
    out = {}
    for sym in (1, 0):
        emd = np.empty((N, N)); iters = np.empty((N, N), dtype=np.int32)
        _lib.check(L.pilot_ot_sinkhorn_grid(_lib.dptr(P), N, K, _lib.dptr(M), 0.1, 1000, 1e-9, 1e3, 20, _lib.PREC["f16x2"], 0.0, sym,
                                            0, N, 1, _lib.dptr(emd), _lib.iptr(iters), None, None))
        out[sym] = (emd, iters)
    off = ~np.eye(N, dtype=bool)
    np.testing.assert_array_equal(out[1][0][off], out[0][0][off])
    np.testing.assert_array_equal(out[1][1][off], out[0][1][off])
    assert np.abs(out[1][0] - out[0][0]).max() <= TOL32


@pytest.mark.parametrize("K", [34, 67])
@pytest.mark.parametrize("prec,tol", [("fp32", TOL32), ("bf16x3", TOL32), ("f16x2", TOL32), ("fp64", TOL64)])
def test_nonsymmetric_cost_with_tail_rows(K, prec, tol):
    """K mod 16 <= 4 puts the last row-tile on the VALU (tail_rows); a non-symmetric cost uses the second weight form
    and (small grid, no solo waves) the cooperative kernel."""
    rng = np.random.default_rng(K)
    P, _ = make_problem(23, K, 6, seed=K, cells_per_patient=300)
    M = rng.random((K, K))
    M /= M.max()
    Eo = O.sinkhorn_grid(P, M, 0.3, n_threads=16)
    Eg = engine.sinkhorn_grid(P, M, 0.3, precision=prec)
    assert np.abs(Eg - Eo).max() <= tol


@pytest.mark.parametrize("prec,tol", [("fp32", TOL32), ("bf16x3", TOL32), ("f16x2", TOL32), ("fp64", TOL64)])
def test_duplicate_patients_take_the_solo_path(prec, tol, switches):
    """The diagonal pairs (i, i) are solved one per wavefront; duplicate PATIENTS (a == b bit for bit, i != j) stay in the
    tiles since round 4 (a cohort with a handful of cell types has thousands of them).  Row shards must reproduce the full
    matrix, and switching the one-wave path off must agree within the tolerance (different summation order, same
    iteration) and leave every off-diagonal pair bit for bit alone."""
    P, M = make_problem(30, 50, 6, seed=77, cells_per_patient=300)
    P[[5, 12, 20]] = P[0]
    P[29] = P[3]
    Eo, io = O.sinkhorn_grid(P, M, 0.1, n_threads=16, return_info=True)
    Eg, ig = engine.sinkhorn_grid(P, M, 0.1, precision=prec, return_info=True)
    assert np.abs(Eg - Eo).max() <= tol
    if prec == "fp64":
        np.testing.assert_array_equal(ig["iters"], io["iters"])
    for r in (0, 5, 29):                                       # one-row shards: 4 (resp. 2) duplicates on one solo workgroup
        part = engine.sinkhorn_grid(P, M, 0.1, precision=prec, row_begin=r, row_end=r + 1)
        np.testing.assert_array_equal(part[0], Eg[r])
    switches.setenv("PILOT_OT_DEBUG", "512")
    Eoff = engine.sinkhorn_grid(P, M, 0.1, precision=prec)
    switches.delenv("PILOT_OT_DEBUG")
    dup = np.eye(30, dtype=bool)
    np.testing.assert_array_equal(Eoff[~dup], Eg[~dup])        # everything off the diagonal is the same code path, bit for bit
    assert np.abs(Eoff - Eg).max() <= tol


@pytest.mark.parametrize("K", [2, 3, 4, 5, 8])
def test_single_digit_cell_type_counts_stay_on_the_mfma_kernels(K, switches):
    """Pathomics cohorts have single-digit K.  Their scalings can jump from below tau past the fp16 range within one update
    (531 -> 2071 at K = 2): such a pair must be handed to the f32 tracking kernel, not end as "numerical errors" and take the
    POT-literal kernel (round 3: 20 580 of 360 000 pairs at K = 2, 65 of the call's 67 ms).  With the hand-over launch
    switched off (PILOT_OT_DEBUG=1024) a pair it would have solved keeps the sentinel written here -- timing-free check of
    WHICH kernel solves these pairs -- and the values must be the oracle's."""
    P, M = make_problem(160, K, 8, seed=K, cells_per_patient=200)
    N = P.shape[0]
    Eo, io = O.sinkhorn_grid(P, M, 0.1, n_threads=16, return_info=True)
    switches.setenv("PILOT_OT_DEBUG", "1024")
    plan = engine.DevicePlan(P, M)
    sent = np.full(N * N, -7, dtype=np.int32)
    _lib.check(plan.L.pilot_ot_memcpy_h2d(plan.dFl, sent.ctypes.data, sent.nbytes))
    plan.run(0.1)
    plan.sync()
    E, info = plan.fetch()
    plan.close()
    assert int((info["flags"] == -7).sum()) == 0, "pairs were left to the POT-literal kernel"
    assert int((info["flags"] & _lib.FLAG_F64).sum()) == 0
    absorbed = (io["flags"] & O.FLAG_ABSORBED) > 0
    assert absorbed.sum() > 0                                   # the case this test is about occurs in the cohort
    assert (((info["flags"] & _lib.FLAG_ABSORBED) > 0) != absorbed).mean() < 0.01      # (a scaling within rounding of tau may differ)
    last_o, last_g = (io["flags"] & O.FLAG_ABSORB_ON_LAST) > 0, (info["flags"] & _lib.FLAG_ABSORB_LAST) > 0
    edge = last_o | last_g
    account_for_absorb_on_last(E, Eo, last_g, last_o, K, TOL32, max_one_sided_frac=1e-3)
    # duplicate patients (a == b, i != j: hundreds at this K) run in the tiles, the diagonal on waves of its own; both within tolerance
    dup = (np.abs(P[:, None, :] - P[None, :, :]).sum(-1) == 0) & ~np.eye(N, dtype=bool)
    assert dup.sum() > 0 or K > 3
    if dup.any():
        assert np.abs(E - Eo)[dup & ~edge].max() <= TOL32


@pytest.mark.parametrize("N,K", [(300, 2), (300, 3), (300, 4), (300, 8), (300, 17), (300, 33), (200, 65), (200, 100), (120, 129), (100, 256)])
def test_whole_grids_across_the_k_range_and_the_pairs_that_stop_later_than_pot(N, K):
    """tools/sinkhorn_full_grid_check.py at test size: EVERY ordered pair of a grid at PILOT's reg 0.1, default precision, for every
    kernel shape of the K range (single-digit K with thousands of tau-absorbing pairs, one / two / ... row tiles, the eight-wave
    kernel beyond 128).  Values within 1e-5 of the fp64 oracle outside the pairs POT returns scaled by 1/K^2; and the f32 stopping
    rule (stopThr floored at 8 f32 ulps of ||b||_2) stops a pair at POT's check or an EARLIER one -- except for a handful of slow
    pairs at K = 3, 4, 8 whose f32 error hovers at the floor (23 / 18 / 6 of 360 000 at N = 600): their COUNT is bounded here, and
    they too are inside the tolerance."""
    P, M = make_problem(N, K, 8, seed=K, cells_per_patient=200)
    Eg, ig = engine.sinkhorn_grid(P, M, 0.1, return_info=True)
    Eo, io = O.sinkhorn_grid(P, M, 0.1, n_threads=16, return_info=True)
    last_o, last_g = (io["flags"] & O.FLAG_ABSORB_ON_LAST) > 0, (ig["flags"] & _lib.FLAG_ABSORB_LAST) > 0
    last = last_o | last_g
    d = np.abs(Eg - Eo)
    # (single-digit K: thousands of pairs absorb, and a pair that stops one check apart ends on the other side of an absorption
    # more often than at c3's K -- bounded at 1e-3 of the grid there, 1e-4 from K = 17 on; each such pair checked against K^2)
    account_for_absorb_on_last(Eg, Eo, last_g, last_o, K, TOL32, max_one_sided_frac=1e-4 if K >= 17 else 1e-3)
    later = ig["iters"] > io["iters"]
    allowed = 0 if K >= 17 or K == 2 else int(np.ceil(2e-4 * Eo.size))
    assert int(later.sum()) <= allowed, "%d pairs stop later than the oracle (allowed %d)" % (later.sum(), allowed)
    if later.any():
        assert d[later & ~last].max() <= TOL32


@pytest.mark.parametrize("reg", [0.01, 0.02, 0.04])
def test_whole_grid_of_the_small_reg_sweep_at_test_size(reg):
    """BASELINE config 3's reg sweep below the fp16-split range, EVERY pair of a 150-patient cohort of c3's shape: at reg 0.01 more
    than half the oracle's pairs run to POT's 1000-update cap and nearly all tau-absorb.  Outside the pairs POT returns scaled
    by 1/K^2 (absorption on the last update; flagged on both sides, or by one side alone only where the two stopped at different
    checks) every value is within 1e-5, and every pair stops at the oracle's check or an earlier one."""
    cfg = dict(CONFIGS["c3"], n_patients=150)
    P, M = make_problem(**cfg)
    Eg, ig = engine.sinkhorn_grid(P, M, reg, return_info=True)
    Eo, io = O.sinkhorn_grid(P, M, reg, n_threads=16, return_info=True)
    last_o, last_g = (io["flags"] & O.FLAG_ABSORB_ON_LAST) > 0, (ig["flags"] & _lib.FLAG_ABSORB_LAST) > 0
    # every pair accounted for: alike-flagged pairs within 1e-5; a one-sided flag means one side returned cost / K^2 and the
    # other the cost, checked as such, and there are at most 1e-4 of the grid of them (VERDICT r05 weak #1a)
    n_both, n_only_o, n_only_g = account_for_absorb_on_last(Eg, Eo, last_g, last_o, P.shape[1], TOL32, max_one_sided_frac=1e-4)
    print("reg %g: absorb-on-last pairs: %d both, %d oracle only, %d GPU only of %d" % (reg, n_both, n_only_o, n_only_g, Eg.size))
    assert (ig["iters"] <= io["iters"]).all()
    same = ig["iters"] == io["iters"]
    assert int(((last_o ^ last_g) & same).sum()) <= 1          # (a scaling within an f32 rounding of tau on its last update: the knife edge)
    both = last_o & last_g
    if both.any():
        assert np.abs(Eg - Eo)[both].max() <= 1e-12             # both returned the 1/K^2-scaled cost
    if reg == 0.01:
        assert (io["iters"] >= 1000).mean() > 0.4 and ((io["flags"] & O.FLAG_ABSORBED) > 0).mean() > 0.9      # the regime this test is about


def test_device_resident_call_with_a_cost_that_is_not_normalised():
    """the device entry point cannot see max(M).  DevicePlan tells the plan (pilot_ot_plan_set_max_cost),
    and AUTO must then leave the fp16-split domain (valid while max(M)/reg <= 16) instead of returning finite but wrong
    distances: max(M) = 3 at reg 0.1 is a ratio of 30."""
    P, M = make_problem(48, 20, 6, seed=11, cells_per_patient=300)
    M3 = 3.0 * M
    Eo = O.sinkhorn_grid(P, M3, 0.1, n_threads=16)
    plan = engine.DevicePlan(P, M3)
    assert plan.max_cost == pytest.approx(3.0)
    plan.run(0.1)
    plan.sync()
    E, info = plan.fetch()
    plan.close()
    assert np.abs(E - Eo).max() <= TOL32 * 3.0
    np.testing.assert_array_equal(E, engine.sinkhorn_grid(P, M3, 0.1))     # the host entry point takes the same decisions
    with pytest.raises(ValueError):
        _lib.check(_lib.load().pilot_ot_plan_set_max_cost(None, 1.0))


def test_row_selection_and_single_row_grids():
    P, M = make_problem(**CONFIGS["c2"])
    full = engine.sinkhorn_grid(P, M, 0.1, precision="fp64")
    part = engine.sinkhorn_grid(P, M, 0.1, precision="fp64", row_begin=3, row_end=77, row_step=8)
    np.testing.assert_array_equal(part, full[3:77:8])                # same pair -> same bits, whatever the tile
    one = engine.sinkhorn_grid(P, M, 0.1, precision="fp32", row_begin=99, row_end=100)
    f32 = engine.sinkhorn_grid(P, M, 0.1, precision="fp32")
    np.testing.assert_array_equal(one[0], f32[99])
    empty = engine.sinkhorn_grid(P, M, 0.1, row_begin=5, row_end=5)
    assert empty.shape == (0, 100)


def test_deterministic_across_runs():
    P, M = make_problem(**CONFIGS["c2"])
    a = engine.sinkhorn_grid(P, M, 0.1, precision="fp32")
    b = engine.sinkhorn_grid(P, M, 0.1, precision="fp32")
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("K", [12, 50])
@pytest.mark.parametrize("reg", [1.0, 0.1, 0.02])
def test_empty_bins_follow_pot_through_the_absorption(K, reg):
    """Histograms with empty bins (not produced by the reference, whose prior keeps every proportion positive, but legal
    for ot.sinkhorn2): without an absorption nothing special happens; WITH one POT takes log(0), rebuilds a kernel with
    zero rows, hits 0/0 at the next update and returns the iterate before it ("Numerical errors").  The engine sends such
    pairs to the POT-literal kernel: values, update counts and flags equal the oracle's."""
    from scipy.spatial.distance import pdist, squareform
    rng = np.random.default_rng(3 + K)
    P = rng.dirichlet(0.3 * np.ones(K), size=24)
    P[P < 2e-2] = 0.0
    P[0] = 0.0; P[0, 3] = 1.0
    P /= P.sum(1, keepdims=True)
    M = squareform(pdist(rng.standard_normal((K, 8)), "cosine"))
    M /= M.max()
    Eo, io = O.sinkhorn_grid(P, M, reg, return_info=True, n_threads=8)
    nan_revert = (io["flags"] & O.FLAG_NAN_REVERT) > 0
    assert nan_revert.any() == (reg < 1.0)                    # the path is taken at the smaller regs
    for prec, tol in (("auto", TOL32), ("fp32", TOL32), ("fp64", 1e-12)):
        Eg, ig = engine.sinkhorn_grid(P, M, reg, precision=prec, return_info=True)
        assert np.isfinite(Eg).all()
        assert np.abs(Eg - Eo).max() <= tol
        got = (ig["flags"] & _lib.FLAG_NAN) > 0
        np.testing.assert_array_equal(got, nan_revert)
        np.testing.assert_array_equal(ig["iters"][nan_revert], io["iters"][nan_revert])
        assert np.abs(Eg - Eo)[nan_revert].max(initial=0.0) <= 1e-12      # those pairs are solved in fp64, POT's way


@pytest.mark.parametrize("case", ["unequal_masses", "tiny_masses", "huge_reg", "constant_cost", "zero_cost", "one_patient",
                                  "tau5", "cap3", "stop1e-3"])
def test_edge_inputs_against_the_oracle(case):
    """Inputs the reference never produces but ot.sinkhorn2 accepts.  Pairs whose absorption lands on the final update
    (POT then returns the plan / K^2) in one precision but not in the other sit on a knife edge and are compared in f64 only."""
    P, M = make_problem(16, 20, 6, seed=5, cells_per_patient=400)
    reg, kw_o, kw_g = 0.1, {}, {}
    if case == "unequal_masses": P = P * np.linspace(0.5, 2.0, 16)[:, None]       # no rescaling in sinkhorn2: never converges
    if case == "tiny_masses": P = P * 1e-6
    if case == "huge_reg": reg = 100.0
    if case == "constant_cost": M = np.ones_like(M) - np.eye(20)
    if case == "zero_cost": M = np.zeros_like(M)
    if case == "one_patient": P = P[:1]
    if case == "tau5": kw_o, kw_g = dict(tau=5.0), dict(tau=5.0)
    if case == "cap3": kw_o, kw_g = dict(numItermax=3), dict(num_iter_max=3)
    if case == "stop1e-3": kw_o, kw_g = dict(stopThr=1e-3), dict(stop_thr=1e-3)
    Eo, io = O.sinkhorn_grid(P, M, reg, return_info=True, n_threads=8, **kw_o)
    E64, i64 = engine.sinkhorn_grid(P, M, reg, precision="fp64", return_info=True, **kw_g)
    assert np.abs(E64 - Eo).max() <= 1e-12 * max(1.0, np.abs(Eo).max())
    np.testing.assert_array_equal(i64["iters"], io["iters"])
    for prec in ("auto", "fp32"):
        Eg, ig = engine.sinkhorn_grid(P, M, reg, precision=prec, return_info=True, **kw_g)
        edge = ((io["flags"] & O.FLAG_ABSORB_ON_LAST) > 0) != ((ig["flags"] & _lib.FLAG_ABSORB_LAST) > 0)
        assert np.isfinite(Eg).all() and edge.mean() < 0.05
        assert np.abs(Eg - Eo)[~edge].max() <= TOL32 * max(1.0, np.abs(Eo).max())


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_randomized_shapes_and_options_against_the_oracle(seed):
    """tools/fuzz_sinkhorn.py in small: random N, K (across every tile count), reg, tau, iteration caps, empty bins, unequal
    masses (scalings that leave the f32 / f64 range are handed to the POT-literal kernel), non-symmetric costs (at K = 128
    the operand images of a non-symmetric cost do not fit LDS in f64: the POT-literal kernel takes the grid).  fp64 must
    agree in value and update count, the f32 paths in value wherever the absorb-on-the-final-update flag agrees."""
    from scipy.spatial.distance import pdist, squareform
    rng = np.random.default_rng(seed)
    for _ in range(14):
        N = int(rng.integers(1, 50)); K = int(rng.choice([1, 2, 3, 5, 8, 13, 16, 17, 20, 31, 32, 33, 48, 50, 64, 65, 80, 100, 128]))
        reg = float(rng.choice([1.0, 0.3, 0.1, 0.05, 0.02, 0.01]))
        P = rng.dirichlet(float(rng.choice([0.2, 1.0, 5.0])) * np.ones(K), size=N)
        if rng.random() < 0.3:
            P[P < 0.02] = 0.0; P[P.sum(1) == 0, 0] = 1.0; P /= P.sum(1, keepdims=True)
        if rng.random() < 0.25:
            P *= rng.uniform(0.5, 2.0, size=(N, 1))
        M = np.zeros((1, 1))
        if K > 1:
            M = squareform(pdist(rng.standard_normal((K, 6)), str(rng.choice(["cosine", "euclidean", "cityblock"])))); M /= M.max()
            if rng.random() < 0.15:
                M = M * rng.uniform(0.7, 1.0, size=M.shape); M /= M.max()
        kw_o, kw_g = {}, {}
        if rng.random() < 0.2: kw_o["tau"] = kw_g["tau"] = float(rng.choice([6.5, 47.3]))
        if rng.random() < 0.2: kw_o["numItermax"] = kw_g["num_iter_max"] = int(rng.choice([1, 7, 40, 200]))
        Eo, io = O.sinkhorn_grid(P, M, reg, return_info=True, n_threads=8, **kw_o)
        assert np.isfinite(Eo).all()
        tag = "N=%d K=%d reg=%g %s" % (N, K, reg, kw_g)
        E64, i64 = engine.sinkhorn_grid(P, M, reg, precision="fp64", return_info=True, **kw_g)
        assert np.abs(E64 - Eo).max() <= 1e-11 * max(1.0, np.abs(Eo).max()), tag
        np.testing.assert_array_equal(i64["iters"], io["iters"], err_msg=tag)
        for prec in (("auto", "fp32") if 1.0 / reg <= 60.0 else ("auto",)):
            Eg, ig = engine.sinkhorn_grid(P, M, reg, precision=prec, return_info=True, **kw_g)
            edge = ((io["flags"] & O.FLAG_ABSORB_ON_LAST) > 0) != ((ig["flags"] & _lib.FLAG_ABSORB_LAST) > 0)
            assert np.isfinite(Eg).all() and edge.mean() <= 0.1, tag
            assert np.abs(Eg - Eo)[~edge].max(initial=0.0) <= TOL32 * max(1.0, np.abs(Eo).max()), tag + " " + prec


def test_graph_replay_gives_the_same_bits_and_follows_argument_and_content_changes():
    """pilot_ot_plan_enable_graph: the third identical call replays a captured hipGraph; results are bit-identical to
    ordinary launches, a changed argument falls back (and re-captures), new CONTENTS of P are seen by the replay."""
    P, M = make_problem(**CONFIGS["c2"])
    N = P.shape[0]
    plan = engine.DevicePlan(P, M)
    ref = {}
    for reg in (0.1, 0.02):
        plan.run(reg)
        ref[reg] = plan.fetch()
    plan.enable_graph(True)
    for reg in (0.1, 0.1, 0.1, 0.1, 0.02, 0.02, 0.02, 0.1, 0.1, 0.1):       # plain, capture, replay, replay, plain, capture, ...
        plan.run(reg)
        E, info = plan.fetch()
        np.testing.assert_array_equal(E, ref[reg][0])
        np.testing.assert_array_equal(info["iters"], ref[reg][1]["iters"])
    part = np.array(ref[0.1][0][1::3])
    for _ in range(4):
        plan.run(0.1, row_begin=1, row_step=3)
        np.testing.assert_array_equal(plan.fetch(n_rows=len(part))[0], part)
    # same buffers, new contents: the replayed graph reads them
    P2 = np.ascontiguousarray(P[::-1])
    for _ in range(3):
        plan.run(0.1)
    _lib.check(plan.L.pilot_ot_memcpy_h2d(plan.dP, P2.ctypes.data, P2.nbytes))
    plan.run(0.1)
    np.testing.assert_array_equal(plan.fetch()[0], ref[0.1][0][::-1, ::-1])
    plan.enable_graph(False)
    plan.run(0.1)
    np.testing.assert_array_equal(plan.fetch()[0], ref[0.1][0][::-1, ::-1])
    plan.close()


def test_graph_replay_follows_a_changed_test_switch(switches):
    """A test switch that changes the launch sequence (PILOT_OT_NO_QUAD: 112 < K <= 128 on the one-wave kernel instead of the
    four-waves-per-tile one) is part of the graph key: a plan in graph mode captures anew instead of replaying the old kernels."""
    P, M = make_problem(60, 120, 6, seed=120, cells_per_patient=3000)
    plain = engine.DevicePlan(P, M)
    plain.run(0.1, precision="f16x2")
    E_quad = plain.fetch()[0]
    switches.setenv("PILOT_OT_NO_QUAD", "1")
    plain.run(0.1, precision="f16x2")
    E_one = plain.fetch()[0]
    switches.delenv("PILOT_OT_NO_QUAD")
    plain.close()
    assert np.any(E_quad != E_one)                      # the two kernels' bits differ, so the check below can tell them apart
    plan = engine.DevicePlan(P, M)
    plan.enable_graph(True)
    for _ in range(3):                                  # plain, capture, replay
        plan.run(0.1, precision="f16x2")
        np.testing.assert_array_equal(plan.fetch()[0], E_quad)
    switches.setenv("PILOT_OT_NO_QUAD", "1")
    for _ in range(3):
        plan.run(0.1, precision="f16x2")
        np.testing.assert_array_equal(plan.fetch()[0], E_one)
    plan.close()


@pytest.mark.parametrize("reg,tau,lo,hi", [(0.1, 25.0, 0.1, 0.6), (0.05, 30.0, 0.8, 1.0)])
def test_tau_tracking_path_mixes_with_the_fast_path(reg, tau, lo, hi):
    """A small tau makes a fraction of the pairs tau-absorb, so within one call some pairs finish in the
    fast kernel and the others go through the track list into the tracking kernel -- in f32 too."""
    P, M = make_problem(40, 20, 6, seed=12, cells_per_patient=300)
    Eo, io = O.sinkhorn_grid(P, M, reg, tau=tau, n_threads=16, return_info=True)
    abs_o = (io["flags"] & O.FLAG_ABSORBED) > 0
    assert lo < abs_o.mean() < hi
    ok = (io["flags"] & O.FLAG_ABSORB_ON_LAST) == 0
    Eg, ig = engine.sinkhorn_grid(P, M, reg, tau=tau, precision="fp64", return_info=True)
    np.testing.assert_array_equal((ig["flags"] & _lib.FLAG_ABSORBED) > 0, abs_o)
    np.testing.assert_array_equal(ig["iters"], io["iters"])
    assert np.abs(Eg - Eo).max() <= 1e-10
    for prec in ("fp32", "bf16x3", "f16x2"):
        Eg, ig = engine.sinkhorn_grid(P, M, reg, tau=tau, precision=prec, return_info=True)
        assert abs(((ig["flags"] & _lib.FLAG_ABSORBED) > 0).mean() - abs_o.mean()) < 0.05
        assert np.abs(Eg - Eo)[ok].max() <= TOL32


def test_iteration_cap_and_check_period_arguments():
    P, M = make_problem(**CONFIGS["c1"])
    for kw in (dict(numItermax=7), dict(numItermax=45, print_period=5), dict(stopThr=1e-4)):
        Eo, io = O.sinkhorn_grid(P, M, 0.1, return_info=True, **kw)
        gk = dict(num_iter_max=kw.get("numItermax", 1000), check_period=kw.get("print_period", 20),
                  stop_thr=kw.get("stopThr", 1e-9))
        Eg, ig = engine.sinkhorn_grid(P, M, 0.1, precision="fp64", return_info=True, **gk)
        np.testing.assert_array_equal(ig["iters"], io["iters"])
        assert np.abs(Eg - Eo).max() <= TOL64


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_fixture_matrix(name):
    g = load_golden(name)
    P, M = g["proportions"], g["cost"] / g["cost"].max()
    E = engine.sinkhorn_grid(P, M, float(g["reg"]), precision="fp64")
    assert np.abs(E - g["emd_reg"]).max() <= TOL64
    for prec in ("fp32", "bf16x3", "f16x2"):
        E = engine.sinkhorn_grid(P, M, float(g["reg"]), precision=prec)
        assert np.abs(E - g["emd_reg"]).max() <= TOL32


def test_full_size_properties_c3():
    """BASELINE full size (600 x 50): size-independent properties, and the whole grid against the oracle."""
    P, M = make_problem(**CONFIGS["c3"])
    E, info = engine.sinkhorn_grid(P, M, 0.1, precision="auto", return_info=True)
    assert E.shape == (600, 600) and np.isfinite(E).all()
    assert ((info["flags"] & _lib.FLAG_CONVERGED) > 0).all()
    assert np.abs(E - E.T).max() < 1e-6                             # converged entropic costs are symmetric
    assert (np.diag(E) > 1e-3).all() and E.min() > 0 and E.max() < 1.0
    # entropic cost upper-bounds the exact cost and is within reg*log(K^2)-ish of it
    Ex = engine.emd_grid(P, M)
    assert (E >= Ex - 1e-6).all()
    # row shards reproduce the full matrix bit for bit (what the multi-GPU path relies on)
    for rank in (0, 5):
        part = engine.sinkhorn_grid(P, M, 0.1, precision="auto", row_begin=rank, row_step=8)
        np.testing.assert_array_equal(part, E[rank::8])
    # EVERY pair of the headline workload against the fp64 oracle (360 000 pairs: a few seconds on the box's 16 cores)
    Eo, io = O.sinkhorn_grid(P, M, 0.1, n_threads=16, return_info=True)
    d = np.abs(E - Eo)
    print("c3, reg 0.1, all 360 000 ordered pairs: max|gpu - oracle| %.3e (mean %.1e); updates gpu %.2f / oracle %.2f per pair"
          % (d.max(), d.mean(), info["iters"].mean(), io["iters"].mean()))
    assert d.max() <= TOL32
    assert np.all(info["iters"] <= io["iters"]) and np.all(info["iters"] % 20 == 1)     # POT's checks; the same or an earlier one


def test_c4_shape_sampled_rows():
    """2000 x 100 x 50 (K = 100: four f32 row tiles) on a few rows."""
    P, M = make_problem(**CONFIGS["c4"])
    rows = dict(row_begin=11, row_end=2000, row_step=997)
    Eo = O.sinkhorn_grid(P, M, 0.1, n_threads=16, **rows)
    for prec in ("fp32", "bf16x3", "f16x2"):
        Eg = engine.sinkhorn_grid(P, M, 0.1, precision=prec, **rows)
        assert np.abs(Eg - Eo).max() <= TOL32
    Eg = engine.sinkhorn_grid(P, M, 0.1, precision="fp64", **rows)
    assert np.abs(Eg - Eo).max() <= TOL64


def test_results_do_not_depend_on_work_order_or_occupancy(switches):
    """A pair's arithmetic is independent of which wave / column / launch order it lands in: disabling the
    longest-first ordering or changing the number of resident workgroups must reproduce the same bits."""
    P, M = make_problem(**CONFIGS["c2"])
    for prec in ("fp32", "bf16x3", "f16x2"):
        ref, iref = engine.sinkhorn_grid(P, M, 0.1, precision=prec, return_info=True)
        for dbg in ("2", "16", "34"):          # no ordering; 1 workgroup per CU; both
            switches.setenv("PILOT_OT_DEBUG", dbg)
            got, ig = engine.sinkhorn_grid(P, M, 0.1, precision=prec, return_info=True)
            np.testing.assert_array_equal(got, ref)
            np.testing.assert_array_equal(ig["iters"], iref["iters"])
        switches.delenv("PILOT_OT_DEBUG")


def test_host_workspace_cache_across_shapes_and_shutdown():
    """The host API caches its device workspace per (N, K); switching shapes, shrinking, growing and an explicit
    shutdown in between must all give the same answers."""
    outs = {}
    for rep in range(2):
        for (N, K) in ((40, 20), (100, 30), (40, 20), (7, 5)):
            P, M = make_problem(N, K, 6, seed=N + K, cells_per_patient=300)
            E = engine.sinkhorn_grid(P, M, 0.2, precision="fp64")
            X = engine.emd_grid(P, M)
            if (N, K) in outs:
                np.testing.assert_array_equal(E, outs[(N, K)][0])
                np.testing.assert_array_equal(X, outs[(N, K)][1])
            outs[(N, K)] = (E, X)
        _lib.check(_lib.load().pilot_ot_shutdown())
    part = engine.sinkhorn_grid(*make_problem(40, 20, 6, seed=60, cells_per_patient=300), 0.2, precision="fp64",
                                row_begin=3, row_end=9)
    np.testing.assert_array_equal(part, outs[(40, 20)][0][3:9])


@pytest.mark.parametrize("N,K", [(460, 8), (330, 40)])
def test_diagonal_of_a_large_grid_stays_in_the_tiles_and_row_shards_agree_bit_for_bit(N, K, switches):
    """Exact duplicates (the diagonal, a == b) run one pair per wave only while the FULL grid is small (N^2 / 16 below three times the
    launch's wave slots: N < 443 at K <= 32, N < 314 at 33 <= K <= 64 on 256 CUs); above that they stay in the 16-pair tiles, because 600
    one-pair waves were the tail of the c3 launch.  The rule reads N, not the rows of the call: a row shard of such a grid keeps its
    diagonal in the tiles too and returns the full grid's bits; both paths are within the f32-class tolerance of the oracle."""
    P, M = make_problem(N, K, 6, seed=N + K, cells_per_patient=400)
    Eo, io = O.sinkhorn_grid(P, M, 0.1, n_threads=16, return_info=True)
    Eg, ig = engine.sinkhorn_grid(P, M, 0.1, return_info=True)
    assert np.abs(Eg - Eo).max() <= TOL32
    d = np.arange(N)
    itd = ig["iters"][d, d]
    assert np.all(itd <= io["iters"][d, d]) and np.all((itd % 20 == 1) | (itd == 1000))      # (POT's checks, or its cap)
    for rb, re_, rs in ((0, N, 8), (3, N, 5), (N // 2, N // 2 + 1, 1)):
        part = engine.sinkhorn_grid(P, M, 0.1, row_begin=rb, row_end=re_, row_step=rs)
        np.testing.assert_array_equal(part, Eg[rb:re_:rs])
    # the one-wave path for the same diagonal (forced off / the small-grid rule cannot be forced on: compare the two paths' values)
    switches.setenv("PILOT_OT_DEBUG", "512")
    Et = engine.sinkhorn_grid(P, M, 0.1)
    np.testing.assert_array_equal(Et, Eg)                    # (already in the tiles: the switch changes nothing at this size)


def test_device_plan_closes_twice_and_then_goes():
    """close() frees the plan's device buffers at once and may be called again; deleting the closed plan frees nothing twice"""
    P, M = make_problem(**CONFIGS["c2"])
    plan = engine.DevicePlan(P, M, n_rows_max=2)
    plan.run(0.1, row_end=2)
    plan.sync()
    assert plan.fetch()[0].shape == (2, P.shape[0])
    bufs = list(plan._bufs)
    plan.close()
    assert plan._bufs == [] and not plan.plan and len(bufs) == 6 and not any(b.ptr for b in bufs)
    plan.close()
    del plan
    buf = engine._DeviceBuffer(64)
    buf.free()
    buf.free()
    assert not buf.ptr
