"""Cell-level W2: every compiled kernel variant, the shape edges and the control arguments against the fp64 oracle.

``cell_w2_enqueue`` picks one of eight ``cell_w2_kernel<KB, AUG, HALF>``: KB = 1 / 2 (D <= 32 / 64), AUG (two spare
k-slots, D <= 32 KB - 2, off under PILOT_OT_CELL_NO_AUG) and HALF (two fp16 operand pieces; three bf16 pieces under
PILOT_OT_CELL_BF16 -- the scaled coordinates that would select them without it lie beyond the far-out-cell limit, which is
refused).  Every case asserts the pieces the call used, so a changed dispatch cannot quietly turn two cases into one.

Reference: oracle.cell_w2_c (fp64, POT sinkhorn_log control flow, the same as oracle.cell_w2) on the same float32 input.
Tolerance: 1e-5 * max(1, |W_oracle|) per pair."""
import os
from functools import lru_cache

import numpy as np
import pandas as pd
import pytest

from oracle import oracle as O
from pilot_amd import engine, tl
from pilot_amd.synthetic import Cohort

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _host_cores():
    """Cores this process may run on (affinity, capped by a cgroup v2 quota): OpenMP beyond them only spins."""
    n = len(os.sched_getaffinity(0))
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, int(float(q) / float(per) + 0.5))
    except (OSError, ValueError):
        pass
    return max(1, min(16, n))


THREADS = _host_cores()
BF16, NO_AUG = "PILOT_OT_CELL_BF16", "PILOT_OT_CELL_NO_AUG"
LOG2E = 1.4426950408889634


def clouds(sizes, D, seed, offset=0.0):
    """Patients of the given sizes: unit-variance cells around centres of spread 0.5; scale from the data (tl's default)."""
    rng = np.random.default_rng(seed)
    centres = 0.5 * rng.standard_normal((len(sizes), D))
    X = np.concatenate([centres[p] + rng.standard_normal((n, D)) for p, n in enumerate(sizes)]) + offset
    X = X.astype(np.float32)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    Xd = X.astype(np.float64)
    scale = 2.0 * float(((Xd - Xd.mean(0)) ** 2).sum(1).mean())
    return X, offs, scale


def oracle_pair(X, offs, i, j, scale, reg, **kw):
    return O.cell_w2_c(X[offs[i]:offs[i + 1]], X[offs[j]:offs[j + 1]], scale, reg, n_threads=THREADS, return_info=True, **kw)


def oracle_grid(X, offs, scale, reg, **kw):
    N = len(offs) - 1
    W, it, err = np.zeros((N, N)), np.zeros((N, N), dtype=np.int64), np.zeros((N, N))
    for i in range(N):
        for j in range(N):
            W[i, j], info = oracle_pair(X, offs, i, j, scale, reg, **kw)
            it[i, j], err[i, j] = info["iters"], info["err"]
    return W, it, err


def assert_parity(Wg, Wo, tol=TOL, what=""):
    Wg, Wo = np.asarray(Wg), np.asarray(Wo)
    assert np.isfinite(Wg).all(), what
    bad = np.abs(Wg - Wo) > tol * np.maximum(1.0, np.abs(Wo))
    assert not bad.any(), "%s: %d pairs beyond %.1e relative, worst |dW| = %.3e at %s" % (
        what, bad.sum(), tol, np.abs(Wg - Wo).max(), np.argwhere(bad)[:4].tolist())


def gpu_grid(X, offs, scale, reg, **kw):
    co = engine.CellCohort(X, offs)
    try:
        W, info = co.w2_grid(scale, reg, return_info=True, **kw)
        return W, info, co.last_pieces
    finally:
        co.close()


# ---- 1. the variant matrix --------------------------------------------------------------------------------------------
DIMS = (1, 30, 31, 32, 33, 62, 63, 64)
REGS = (0.5, 0.1, 0.02)


@lru_cache(maxsize=None)
def _matrix_case(D, reg):
    rng = np.random.default_rng(1000 + D)
    sizes = rng.integers(8, 48, int(rng.integers(3, 6)))
    X, offs, scale = clouds(sizes, D, seed=D)
    return X, offs, scale, oracle_grid(X, offs, scale, reg)[0]


def _variant(D, switch):
    """(KB, AUG, pieces) that the dispatch must pick"""
    KB = 1 if D <= 32 else 2
    aug = D <= 32 * KB - 2 and switch != NO_AUG
    return KB, aug, 3 if switch == BF16 else 2


@pytest.mark.parametrize("reg", REGS)
@pytest.mark.parametrize("switch", [None, BF16, NO_AUG])
@pytest.mark.parametrize("D", DIMS)
def test_every_kernel_variant_matches_the_oracle(D, switch, reg, switches):
    X, offs, scale, Wo = _matrix_case(D, reg)
    if switch:
        switches.setenv(switch, "1")
    Wg, info, pieces = gpu_grid(X, offs, scale, reg)
    assert pieces == _variant(D, switch)[2]
    assert_parity(Wg, Wo, what="D=%d %s reg=%g" % (D, switch, reg))


def test_the_matrix_reaches_all_eight_instantiations():
    seen = {_variant(D, s) for D in DIMS for s in (None, BF16, NO_AUG)}
    assert seen == {(kb, aug, np_) for kb in (1, 2) for aug in (False, True) for np_ in (2, 3)}


# ---- 2. cohort state across calls ---------------------------------------------------------------------------------------
def test_cohort_switches_pieces_and_slots_between_calls(switches):
    """One cohort, calls alternating between the fp16 and bf16 operand pieces and with / without the spare-slot variant: every
    call gives the bits (values and update counts) of a freshly created cohort with the same settings."""
    for D in (30, 62):
        X, offs, scale = clouds([40, 23, 57, 17], D, seed=70 + D)
        co = engine.CellCohort(X, offs)
        try:
            for reg, sw in ((0.1, None), (0.1, BF16), (0.5, None), (0.5, NO_AUG), (0.1, BF16), (0.1, NO_AUG),
                            (0.5, BF16), (0.1, None), (0.5, None)):
                switches.delenv(BF16)
                switches.delenv(NO_AUG)
                if sw:
                    switches.setenv(sw, "1")
                got, ig = co.w2_grid(scale, reg, return_info=True)
                assert co.last_pieces == (3 if sw == BF16 else 2)
                ref, ir, pieces = gpu_grid(X, offs, scale, reg)
                assert pieces == co.last_pieces
                np.testing.assert_array_equal(got, ref, err_msg="D=%d reg=%g %s" % (D, reg, sw))
                np.testing.assert_array_equal(ig["iters"], ir["iters"])
        finally:
            co.close()


def test_bf16_multi_device_shards_match_one_device(switches):
    switches.setenv(BF16, "1")
    X, offs, scale = clouds([33, 20, 45, 16, 9], 40, seed=5)
    ref, ir, pieces = gpu_grid(X, offs, scale, 0.1)
    assert pieces == 3
    multi, im = engine.cell_w2_grid(X, offs, scale, 0.1, devices=[0, 0], return_info=True)
    np.testing.assert_array_equal(multi, ref)
    np.testing.assert_array_equal(im["iters"], ir["iters"])


# ---- 3. cell-count edges -------------------------------------------------------------------------------------------------
EDGE_SIZES = (257, 65, 64, 63, 33, 32, 31, 16, 15, 2, 17, 1)


@pytest.mark.parametrize("D", [30, 62])
def test_patient_size_edges_and_the_operand_pad(D):
    """Patients of 1 .. 257 cells around the 16-cell tiles.  The fp16 column sweep reads up to 31 cells past a patient; a
    1-cell patient and a partial-tile patient each go LAST in one of the two orders, so that read lands in the pad."""
    X, offs, scale = clouds(EDGE_SIZES, D, seed=D)
    Wo = oracle_grid(X, offs, scale, 0.1)[0]
    N = len(EDGE_SIZES)
    for order in (list(range(N)), [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 10]):      # ... 17, 1  and  ... 1, 17
        Xp = np.concatenate([X[offs[p]:offs[p + 1]] for p in order])
        op = np.concatenate([[0], np.cumsum([EDGE_SIZES[p] for p in order])]).astype(np.int64)
        Wg, info, pieces = gpu_grid(Xp, op, scale, 0.1)
        assert pieces == 2
        assert_parity(Wg, Wo[np.ix_(order, order)], what="order %s" % order[-2:])


def test_degenerate_clouds():
    """A patient whose cells are one point, two patients with identical clouds, and every coordinate offset by 1e3 (the
    cohort is centred in fp64 before the f32 work); the oracle sees the same float32 input."""
    D = 30
    rng = np.random.default_rng(9)
    base = rng.standard_normal((40, D))
    point = np.repeat(rng.standard_normal((1, D)), 25, axis=0)
    X = np.concatenate([base, point, base, rng.standard_normal((31, D)) + 0.7]) + 1e3
    X = X.astype(np.float32)
    offs = np.array([0, 40, 65, 105, 136], dtype=np.int64)
    Xd = X.astype(np.float64)
    scale = 2.0 * float(((Xd - Xd.mean(0)) ** 2).sum(1).mean())
    for reg in (0.1, 0.02):
        Wo = oracle_grid(X, offs, scale, reg)[0]
        Wg, info, pieces = gpu_grid(X, offs, scale, reg)
        assert pieces == 2
        assert_parity(Wg, Wo, what="reg %g" % reg)
        assert np.abs(Wg[0] - Wg[2]).max() <= TOL and np.abs(Wg[:, 0] - Wg[:, 2]).max() <= TOL
        assert abs(Wg[1, 1]) <= TOL


@pytest.mark.parametrize("D,switch", [(50, None), (64, BF16)])
def test_kb2_patients_beyond_one_pass_of_the_waves(D, switch, switches):
    """KB = 2 keeps 2 row blocks (32 rows) per wave and 16 waves per pair: 512 rows per pass, so 1 500 cells loop three times."""
    if switch:
        switches.setenv(switch, "1")
    X, offs, scale = clouds([1500, 1433], D, seed=D)
    kw = dict(numItermax=40)
    Wo = oracle_grid(X, offs, scale, 0.2, **kw)[0]
    Wg, info, pieces = gpu_grid(X, offs, scale, 0.2, num_iter_max=40)
    assert pieces == _variant(D, switch)[2]
    assert_parity(Wg, Wo)


@pytest.mark.parametrize("D", [30, 50])
def test_the_largest_patient_the_lds_holds(D):
    """3 max_n + 48 floats of LDS per workgroup: 13 637 cells is the largest patient (test_cell_w2_args pins the refusal of
    one more).  Row and column order; the cross pairs against the oracle, the big self-pair finite and the row's minimum."""
    big, small = 13637, 17
    rng = np.random.default_rng(D)
    Xb = rng.standard_normal((big, D))
    Xs = rng.standard_normal((small, D)) + 1.5
    n_it = 21
    for first_big in (True, False):
        X = np.concatenate([Xb, Xs] if first_big else [Xs, Xb]).astype(np.float32)
        offs = np.array([0, big, big + small] if first_big else [0, small, big + small], dtype=np.int64)
        Xd = X.astype(np.float64)
        scale = 2.0 * float(((Xd - Xd.mean(0)) ** 2).sum(1).mean())
        Wg, info, pieces = gpu_grid(X, offs, scale, 0.1, num_iter_max=n_it)
        assert pieces == 2
        b, s = (0, 1) if first_big else (1, 0)
        for i, j in ((b, s), (s, b), (s, s)):
            wo, io = oracle_pair(X, offs, i, j, scale, 0.1, numItermax=n_it)
            assert_parity(Wg[i, j], wo, what="pair %d %d" % (i, j))
        assert np.isfinite(Wg[b, b]) and Wg[b, b] < Wg[b, s]


# ---- 4. control arguments -----------------------------------------------------------------------------------------------
def assert_same_updates(it_g, X, offs, scale, reg, thr_of, **kw):
    """Update counts equal the oracle's.  A count may differ only for a pair whose oracle marginal error at the deciding
    check lies within 1e-3 relative of its threshold (the f32 / fp64 difference can decide the strict <)."""
    N = len(offs) - 1
    for i in range(N):
        for j in range(N):
            wo, io = oracle_pair(X, offs, i, j, scale, reg, **kw)
            if it_g[i, j] == io["iters"]:
                continue
            kw2 = dict(kw, numItermax=int(min(it_g[i, j], io["iters"])))
            _, at = oracle_pair(X, offs, i, j, scale, reg, **kw2)
            thr = thr_of(offs[j + 1] - offs[j])
            assert abs(at["err"] - thr) <= 1e-3 * thr, "pair (%d, %d): %d updates, oracle %d" % (i, j, it_g[i, j], io["iters"])


@pytest.mark.parametrize("n_it", [1, 2])
def test_one_and_two_updates(n_it):
    """The first update of a pair runs the online-maximum form; the second is the first with the reference shift."""
    for D in (30, 64):
        X, offs, scale = clouds([37, 12, 50], D, seed=n_it + D)
        Wo, io, _ = oracle_grid(X, offs, scale, 0.1, numItermax=n_it)
        Wg, info, _ = gpu_grid(X, offs, scale, 0.1, num_iter_max=n_it)
        assert (info["iters"] == n_it).all() and (io == n_it).all()
        assert_parity(Wg, Wo, what="D=%d" % D)


@pytest.mark.parametrize("period", [1, 7, 10])
def test_stop_threshold_above_the_floor_and_check_period(period):
    """stop_thr = 1e-5 lies above the f32 floor: the kernel stops at the oracle's update."""
    X, offs, scale = clouds([41, 26, 60, 33], 30, seed=period)
    kw = dict(stopThr=1e-5, check_period=period)
    Wo, io, _ = oracle_grid(X, offs, scale, 0.1, **kw)
    Wg, info, _ = gpu_grid(X, offs, scale, 0.1, stop_thr=1e-5, check_period=period)
    assert ((info["iters"] - 1) % period == 0).all()
    assert_same_updates(info["iters"], X, offs, scale, 0.1, lambda n: 1e-5, **kw)
    assert_parity(Wg, Wo)


def test_f32_floor_ulps_sets_the_stop_threshold():
    """The kernel stops at max(stop_thr, floor_ulps 2^-23 / sqrt(n_col)): with a large floor the oracle run at that threshold
    takes the same number of updates."""
    X, offs, scale = clouds([44, 19, 64], 30, seed=3)
    ulps = 2000.0
    floor = lambda n: ulps * 2.0 ** -23 / np.sqrt(n)
    Wg, info, _ = gpu_grid(X, offs, scale, 0.1, f32_floor_ulps=ulps)
    N = len(offs) - 1
    Wo = np.zeros((N, N))
    for i in range(N):
        for j in range(N):
            thr = floor(offs[j + 1] - offs[j])
            Wo[i, j], io = oracle_pair(X, offs, i, j, scale, 0.1, stopThr=thr)
            if info["iters"][i, j] != io["iters"]:
                _, at = oracle_pair(X, offs, i, j, scale, 0.1, stopThr=thr, numItermax=int(min(info["iters"][i, j], io["iters"])))
                assert abs(at["err"] - thr) <= 1e-3 * thr, (i, j, info["iters"][i, j], io["iters"])
    assert_parity(Wg, Wo)


# ---- 5. far-out cells: the accuracy envelope -------------------------------------------------------------------------------
S_LIMIT = 50.0               # pilot::CELL_MAX_SCALED_NORM (cellw2_kernels.hpp): the measurement behind it is cited there
FAR_SIZES = (160, 120, 90)


def far_cohort(n_far, s_max, reg, direction="axis", scale=60.0, D=30):
    """The first n_far cells of patient 0 moved out -- along an axis each, or along a diagonal (+-1 in every coordinate) -- so
    that the largest scaled norm of the centred cohort, max_i |x_i - mean| * sqrt(2 log2(e) / (scale * reg)), is s_max."""
    op = np.sqrt(2 * LOG2E / (scale * reg))
    rng = np.random.default_rng(n_far + D)
    X = np.concatenate([rng.standard_normal((n, D)) + 0.5 * rng.standard_normal(D) for n in FAR_SIZES])
    C = len(X)
    if direction == "axis":
        U = np.eye(D)[:n_far]
    else:
        U = np.where(rng.random((n_far, D)) < 0.5, -1.0, 1.0) / np.sqrt(D)
    for _ in range(20):                                  # every far cell at scaled norm s_max (the mean moves with them)
        mu = X.mean(0)
        for f in range(n_far):
            X[f] += U[f] * (s_max / op - np.linalg.norm(X[f] - mu)) / (1.0 - 1.0 / C)
    X = X.astype(np.float32)
    c = X.astype(np.float64) - X.astype(np.float64).mean(0)
    got = float(np.sqrt((c ** 2).sum(1)).max() * op)
    assert abs(got - s_max) <= 1e-4 * s_max
    return X, np.concatenate([[0], np.cumsum(FAR_SIZES)]).astype(np.int64), scale, float(np.abs(c).max() * op)


@pytest.mark.parametrize("reg", [0.1, 0.02])
@pytest.mark.parametrize("D,direction,n_far", [(30, "axis", 1), (30, "axis", 3), (30, "diagonal", 1), (30, "diagonal", 3),
                                               (64, "diagonal", 1)])
def test_far_out_cells_within_the_accepted_envelope(D, direction, n_far, reg, switches):
    """One and three far-out cells, along axes or diagonals, up to just below the limit: both operand formats hold the 1e-5
    contract on the pairs that carry the far cells."""
    pairs = ((0, 0), (0, 1), (1, 0), (2, 0))
    for s_max in (25.0, 38.0, 0.98 * S_LIMIT):
        X, offs, scale, _ = far_cohort(n_far, s_max, reg, direction, D=D)
        Wo = [oracle_pair(X, offs, i, j, scale, reg)[0] for i, j in pairs]
        for sw in (None, BF16):
            switches.delenv(BF16)
            if sw:
                switches.setenv(sw, "1")
            Wg, info, pieces = gpu_grid(X, offs, scale, reg)
            assert pieces == (3 if sw else 2)
            assert_parity([Wg[i, j] for i, j in pairs], Wo, what="s_max %.1f %s" % (s_max, sw))


@pytest.mark.parametrize("direction", ["axis", "diagonal"])
@pytest.mark.parametrize("s_max", [1.02 * S_LIMIT, 150.0, 250.0, 2.0e3, 3.5e4])
def test_far_out_cells_beyond_the_envelope_are_refused(s_max, direction, switches):
    """Beyond the limit the measured error leaves the contract (1e-5 relative is broken from a scaled norm of ~150 on): the
    call is refused with ENOTSUP, in both formats.  A diagonal cell counts by its norm, not by its largest coordinate: up to
    250 every scaled coordinate of the diagonal cohorts stays below the limit.  3.5e4 is where the fp16 pieces used to give way
    to bf16 without a switch."""
    for reg in (0.1, 0.02):
        X, offs, scale, s_coord = far_cohort(1, s_max, reg, direction)
        if direction == "diagonal" and s_max <= 250.0:
            assert s_coord < S_LIMIT
        for sw in (None, BF16):
            switches.delenv(BF16)
            if sw:
                switches.setenv(sw, "1")
            with pytest.raises(NotImplementedError, match="too far out"):
                engine.cell_w2_grid(X, offs, scale, reg)
    with pytest.raises(NotImplementedError, match="too far out"):
        engine.cell_w2_grid(X, offs, scale, reg, devices=[0, 0])


def test_refused_call_leaves_the_cohort_intact():
    """The limit depends on scale * reg, so one cohort can be accepted at one reg and refused at a smaller one; a refused call
    changes nothing: the next accepted call gives the bits of a fresh cohort."""
    X, offs, scale, _ = far_cohort(1, 45.0, 0.1, "diagonal")     # s_max 45 at reg 0.1, 45 * sqrt(5) = 101 at reg 0.02
    ref, iref, _ = gpu_grid(X, offs, scale, 0.1)
    co = engine.CellCohort(X, offs)
    try:
        for reg in (0.1, 0.02, 0.1, 0.02, 0.1):
            if reg == 0.02:
                with pytest.raises(NotImplementedError, match="too far out"):
                    co.w2_grid(scale, reg)
                continue
            got, ig = co.w2_grid(scale, reg, return_info=True)
            np.testing.assert_array_equal(got, ref)
            np.testing.assert_array_equal(ig["iters"], iref["iters"])
    finally:
        co.close()


# ---- 7. the tl surface ----------------------------------------------------------------------------------------------------
def _adata(X, sample_of_row, status_of_row):
    obs = pd.DataFrame({"sampleID": sample_of_row, "status": status_of_row})
    return Cohort(X, obs, emb_key="X_pca")


def test_tl_explicit_scale_and_interleaved_samples(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    X, offs, scale = clouds([30, 45, 22, 38], 12, seed=21)
    names = np.array(["p%d" % p for p in range(4)], dtype=object)
    grouped = np.repeat(names, np.diff(offs))
    status = np.array(["s%d" % (p % 2) for p in range(4)], dtype=object)[np.repeat(np.arange(4), np.diff(offs))]
    # an explicit scale reaches the kernel and the record
    ad = _adata(X, grouped, status)
    tl.cell_level_wasserstein(ad, emb_matrix="X_pca", reg=0.2, scale=3.0 * scale)
    assert ad.uns["EMD_cell_scale"] == 3.0 * scale
    np.testing.assert_array_equal(ad.uns["EMD_cell"], engine.cell_w2_grid(X, offs, 3.0 * scale, 0.2))
    ad_default = _adata(X, grouped, status)
    tl.cell_level_wasserstein(ad_default, emb_matrix="X_pca", reg=0.2)
    assert ad_default.uns["EMD_cell_scale"] == pytest.approx(scale, rel=1e-12)
    assert np.abs(ad_default.uns["EMD_cell"] - ad.uns["EMD_cell"]).max() > 1e-3
    # rows of the samples interleaved: the matrix of the grouped input, samples in order of first appearance
    perm = np.random.default_rng(4).permutation(len(X))
    ad_mixed = _adata(X[perm], grouped[perm], status[perm])
    tl.cell_level_wasserstein(ad_mixed, emb_matrix="X_pca", reg=0.2)
    first = list(dict.fromkeys(grouped[perm]))
    assert list(ad_mixed.uns["EMD_cell_df"].index) == first
    idx = [int(s[1:]) for s in first]
    assert np.abs(ad_mixed.uns["EMD_cell"] - ad_default.uns["EMD_cell"][np.ix_(idx, idx)]).max() <= 1e-6
