"""The apeglm-style shrunken coefficient under a general design on the device (K27: engine.nb_design_shrink,
engine.nb_design_posterior_sd, tl.lfc_shrink_design) against the numpy / scipy restatement (tests/nb_design_shrink_restatement.py,
itself pinned to scipy in test_nb_design_shrink_args.py).

Cases (m, p, G, S): (4, 2, 1, 1) the smallest; (9, 8, 63, 0.3) with m - p = 1 at the widest design; (12, 4, 65, 0.02);
(12, 4, 63, 1); (65, 3, 63, 0.3); (130, 5, 65, 1) -- m = 65 and 130 cross the 64-lane staging stride, G = 63 / 65 sit around a wave
of genes in K26's fit kernel, which supplies beta_mle here.  S = 0.02 rides with m <= 12 only (test_gpu_nb_shrink.py's docstring).
The designs are nb_design_restatement.make_design's, the group column last.  Gene classes, dealt round-robin: NB with planted
coefficients, alpha = minDisp, alpha = 10, means of 2e6, the group column's samples all zero, a single non-zero count, all zero with
a NaN dispersion.  The dispersions are inputs; the far ends come from the device's own maximum-likelihood coefficients.

Parity has K23's two parts, because p is flat to rounding near its top.  (1) For EVERY live gene the restatement's p at the device's
b may fall short of its own best by at most B = 64 * 2^-53 * (sum_j [|c log(a mu)| + |(c + 1/a) log1p(a mu)|] + sum_{l != k}
beta_l^2 / (2 sigma0^2) + log1p(b^2 / S^2) + 4 m + 2), and the device's objective is within B of p at its own point.  (2) On the
genes the restatement resolves (t -+ 1e-4 inside the first bracket, p drops by more than 2 B there) t agrees to 2e-4, the
restatement's profile Newton step at the device's (beta_{-k}, b) is at most 1e-9 (K26's measure) and every entry of the information
is within 1e-9 sqrt(M_aa M_bb) of the restatement's at the device's point; at least 90 % of the NB-class genes must be resolved.
The flags equal the restatement's, and nothing is unconverged or at its bound."""
import functools

import numpy as np
import pandas as pd
import pytest

import nb_design_restatement as DR
import nb_design_shrink_restatement as K
import nb_shrink_restatement as SR
from pilot_amd import engine, tl
from test_nb_design_shrink_args import ARGS, hold_shrunk_frame, pseudobulk_with_a_group_of_zeros, shrunk_design_by_hand

pytestmark = pytest.mark.gpu

CASES = K.CASES


def _ids(case):
    return "m%d-p%d-G%d-S%g" % case


def _freeze(*arrays):
    for a in arrays:
        a.flags.writeable = False


@functools.lru_cache(maxsize=None)
def _case(m, p, G, S):
    """the case's inputs, the device's maximum-likelihood coefficients, and the restatement's search from the same far ends"""
    C = K.case_inputs(m, p, G, S)
    mle = engine.nb_design_fits(C["c"], C["X"], C["s"], C["alpha"])[0]
    far = engine.nb_design_far_end(mle[:, -1])
    want = K.search(C["c"], C["X"], C["s"], C["alpha"], far, S, p - 1, start=mle)
    _freeze(C["c"], C["X"], C["s"], C["alpha"], mle, far, *want.values())
    return dict(C, k=p - 1, mle=mle, far=far, want=want)


def _hold(c, X, s, alpha, far, S, k, want, beta, info, kind=None):
    """parts (1) and (2) and the flags; returns the resolved genes"""
    dead = ~K.live_genes(c, alpha)
    for a in (beta, info["information"].reshape(alpha.size, -1)):
        np.testing.assert_array_equal(np.isnan(a), np.repeat(dead[:, None], a.shape[1], axis=1))
    np.testing.assert_array_equal(np.isnan(info["objective"]), dead)
    assert not info["flags"][dead].any() and not info["steps"][dead].any()
    live = np.flatnonzero(~dead)
    res = np.zeros(alpha.size, dtype=bool)
    if not live.size:
        return res
    cl, al, b = c[:, live], alpha[live], beta[live, k]
    np.testing.assert_array_equal(info["flags"], want["flags"])        # the restatement's, which holds NOT_CONVERGED only if its own fit fails
    assert not info["flags"].any() and info["n_at_bound"] == 0 and info["n_not_converged"] == 0
    assert (np.abs(b) <= np.abs(far[live]) * (1 + 1e-12)).all() and (b * far[live] >= 0).all()
    # (1) the objective, every live gene
    B = K.bound(cl, X, s, al, want["beta"][live], S, k)
    at_got, _, _ = K.profile(cl, X, s, al, b, S, k, start=beta[live])
    short = want["p"][live] - at_got
    off = np.abs(info["objective"][live] - at_got)
    worst = int(np.argmax(short / B))
    print("\nobjective shortfall / B: max %.3g%s; device objective off by at most %.3g B; mean inner steps a lane and round %.2f"
          % ((short / B).max(), "" if kind is None else " (gene class %s)" % K.CLASSES[kind[live][worst]], (off / B).max(),
             info["steps"][live].mean() / (K.GRID * K.ROUNDS)))
    assert (short <= B).all(), (short / B).max()
    assert (off <= B).all(), (off / B).max()
    # (2) the resolved genes
    res = K.resolved(c, X, s, alpha, far, S, k, want)
    r = res[live]
    dt = np.abs(K.t_of(b, S) - want["t"][live])[r]
    step = np.abs(K.profile_step(cl, X, s, al, beta[live], k)).max(axis=1)[r]
    M = K.information(cl, X, s, al, beta[live])
    scale = np.sqrt(np.einsum("gaa,gbb->gab", M, M))
    dM = (np.abs(info["information"][live] - M) / scale).max(axis=(1, 2))[r]
    print("resolved %d of %d genes; t off by at most %.3g; profile Newton step at most %.3g; information off by at most %.3g relative"
          % (r.sum(), live.size, dt.max(initial=0), step.max(initial=0), dM.max(initial=0)))
    assert (dt <= 2e-4).all()
    assert (step <= 1e-9).all()
    assert (dM <= 1e-9).all()
    return res


def _shrink(C, Y=None, cols=slice(None), **kw):
    return engine.nb_design_shrink(C["c"] if Y is None else Y, C["X"], C["s"], C["alpha"][cols], C["mle"][cols], C["far"][cols], C["S"],
                                   return_info=True, **kw)


# ---- (1) parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_shrink_against_the_restatement(case):
    C = _case(*case)
    beta, info = _shrink(C)
    res = _hold(C["c"], C["X"], C["s"], C["alpha"], C["far"], C["S"], C["k"], C["want"], beta, info, C["kind"])
    nb = C["kind"] == 0
    print("NB class: %d of %d resolved" % (res[nb].sum(), nb.sum()))
    assert res[nb].sum() >= 0.9 * nb.sum()                              # a condition on the generator, not a measurement
    assert np.isnan(beta[C["kind"] == K.CLASSES.index("all zero")]).all()
    np.testing.assert_array_equal(engine.nb_design_shrink(C["c"], C["X"], C["s"], C["alpha"], C["mle"], C["far"], C["S"]), beta)
    np.testing.assert_array_equal(info["information"], np.swapaxes(info["information"], 1, 2))


# ---- (2) the reduction to K23 ---------------------------------------------------------------------------------------------------------
def test_two_columns_are_k23():
    """X = [1, codes] on K23's case (12, (7, 5), 63, 0.02) with its two constructed bimodal genes, against engine.nb_shrink"""
    import test_gpu_nb_shrink as T23
    C = T23._case(*T23.BIMODAL)
    assert C["bimodal"]
    c, codes, s, alpha, far, S = C["c"], C["codes"], C["s"], C["alpha"], C["far"], C["S"]
    X = np.stack([np.ones(C["m"]), codes.astype(np.float64)], axis=1)
    b0, b1, old = engine.nb_shrink(c, codes, s, alpha, far, S, return_info=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        mle = np.stack([np.log(C["q"][:, 0]), np.log(C["q"][:, 1]) - np.log(C["q"][:, 0])], axis=1)
    beta, new = engine.nb_design_shrink(c, X, s, alpha, mle, far, S, return_info=True)
    live = np.flatnonzero(~np.isnan(alpha))
    assert np.isnan(beta[np.isnan(alpha)]).all() and np.isfinite(beta[live]).all() and not new["flags"].any()
    cl, al = c[:, live], alpha[live]
    B = SR.bound(cl, codes, s, al, C["want"]["b0"][live], C["want"]["b1"][live], S)
    p_old, _ = SR.profile(cl, codes, s, al, b1[live], S)
    p_new, _ = SR.profile(cl, codes, s, al, beta[live, 1], S)
    print("\np(K23's point) - p(K27's point): within %.3g B" % (np.abs(p_old - p_new) / B).max())
    assert (np.abs(p_old - p_new) <= B).all()
    res = SR.resolved(c, codes, s, alpha, far, S, C["want"])
    assert (np.abs(SR.t_of(beta[:, 1], S) - SR.t_of(b1, S))[res] <= 2e-4).all() and res.sum() >= 20
    near, away = C["kind"] == T23.CLASSES.index("bimodal near"), C["kind"] == T23.CLASSES.index("bimodal far")
    ml = mle[:, 1]
    assert near.any() and away.any()
    assert (np.abs(beta[near, 1]) < S).all() and (np.abs(beta[away, 1]) > 0.5 * np.abs(ml[away])).all()
    w0, w1 = SR.weights(cl, codes, s, al, beta[live, 0], beta[live, 1])
    want_info = np.stack([np.stack([w0 + w1, w1], axis=1), np.stack([w1, w1], axis=1)], axis=1)
    np.testing.assert_allclose(new["information"][live], want_info, rtol=1e-9, atol=0)
    sd = engine.nb_design_posterior_sd(beta, new["information"], S)[live]
    ref = engine.nb_posterior_sd(beta[live, 1], w0, w1, S)
    np.testing.assert_array_equal(np.isnan(sd), np.isnan(ref))
    np.testing.assert_allclose(sd[np.isfinite(ref)], ref[np.isfinite(ref)], rtol=1e-9, atol=0)
    assert np.isfinite(ref).sum() >= 0.5 * live.size


# ---- (3) the column position ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,coef", [(CASES[2], 1), (CASES[5], 2), (CASES[1], 4)], ids=["p4-coef1", "p5-coef2", "p8-coef4"])
def test_the_shrunk_column_may_stand_anywhere(case, coef):
    C = _case(*case)
    p = C["p"]
    beta, info = _shrink(C)
    order = [l for l in range(p - 1)]
    order.insert(coef, p - 1)                                           # the caller's column l is the case's order[l]
    X = np.ascontiguousarray(C["X"][:, order])
    moved, minfo = engine.nb_design_shrink(C["c"], X, C["s"], C["alpha"], np.ascontiguousarray(C["mle"][:, order]), C["far"], C["S"],
                                           coef=coef, return_info=True)
    np.testing.assert_array_equal(moved, beta[:, order])
    np.testing.assert_array_equal(minfo["information"], info["information"][:, order][:, :, order])
    for name in ("objective", "flags", "steps"):
        np.testing.assert_array_equal(minfo[name], info[name])
    negative = engine.nb_design_shrink(C["c"], X, C["s"], C["alpha"], np.ascontiguousarray(C["mle"][:, order]), C["far"], C["S"], coef=coef - p)
    np.testing.assert_array_equal(negative, moved)
    sd = engine.nb_design_posterior_sd(beta, info["information"], C["S"])
    np.testing.assert_allclose(engine.nb_design_posterior_sd(moved, minfo["information"], C["S"], coef=coef), sd, rtol=1e-9, atol=0)


# ---- (4) same bits --------------------------------------------------------------------------------------------------------------------
def _all(C, Y, cols=slice(None)):
    beta, info = _shrink(C, Y, cols)
    return [beta, info["objective"], info["information"], info["flags"], info["steps"]]


@pytest.mark.parametrize("case", [CASES[2], CASES[4]], ids=_ids)
def test_same_bits_by_every_route(case):
    C = _case(*case)
    c, G = C["c"], C["G"]
    assert c.max() < 2 ** 24                                           # float32 holds every count
    first = _all(C, np.ascontiguousarray(c))
    wide = np.full((C["m"], G + 7), 3.0)
    wide[:, 3:3 + G] = c
    D = engine.DeviceMatrix.upload(wide)
    routes = {"again": np.ascontiguousarray(c), "float32": c.astype(np.float32), "device": engine.DeviceMatrix.upload(c),
              "device float32": engine.DeviceMatrix.upload(c.astype(np.float32)), "window": engine.device_columns(D, 3, 3 + G)}
    for name, Y in routes.items():
        for a, b in zip(first, _all(C, Y)):
            np.testing.assert_array_equal(a, b, err_msg=name)
    for j in (0, 8, G - 1):                                            # a gene alone, as in its batch
        for a, b in zip(first, _all(C, engine.device_columns(D, 3 + j, 4 + j), slice(j, j + 1))):
            np.testing.assert_array_equal(a[j:j + 1], b, err_msg="gene %d alone" % j)


# ---- (5) limits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [2, 8])
def test_the_largest_sample_count(p):
    """m = the limit for p: the whole LDS layout, three genes (NB, the group column's samples zero, all zero), part (1)"""
    m = engine.nb_design_limits()["max_samples"][p]
    rng = np.random.default_rng(2700 + p)
    s = DR.size_factors(rng, m)
    X, kinds = DR.make_design(rng, m, p)
    c = DR.nb_class(rng, s, X, kinds, 3)
    alpha = np.clip(0.05 + 2.0 / np.maximum((c / s[:, None]).mean(axis=0), 1.0), DR.MIN_DISP, 10.0)
    c[X[:, -1] == 1, 1] = 0.0
    c[:, 2], alpha[2] = 0.0, np.nan
    mle = engine.nb_design_fits(c, X, s, alpha)[0]
    far = engine.nb_design_far_end(mle[:, -1])
    want = K.search(c, X, s, alpha, far, 0.3, p - 1, start=mle)
    beta, info = engine.nb_design_shrink(c, X, s, alpha, mle, far, 0.3, return_info=True)
    _hold(c, X, s, alpha, far, 0.3, p - 1, want, beta, info)
    more, X1, s1 = np.concatenate([c, c[:1]]), np.concatenate([X, X[:1]]), np.concatenate([s, s[:1]])     # one sample more
    with pytest.raises(NotImplementedError, match="staged in LDS"):
        engine.nb_design_shrink(more, X1, s1, alpha, mle, far, 0.3)


# ---- (6) bad inputs -------------------------------------------------------------------------------------------------------------------
def test_bad_counts_and_left_out_genes():
    C = _case(*CASES[2])
    for value, row, col in ((-1.0, 2, 5), (np.nan, 0, 62), (np.inf, 1, 0), (-0.6, 11, 64)):
        Y = np.array(C["c"])
        Y[row, col] = value
        with pytest.raises(ValueError, match=r"Y\[%d, %d\]" % (row, col)) as err:
            _shrink(C, Y)
        assert (err.value.row, err.value.col) == (row, col)
    alpha = np.array(C["alpha"])
    alpha[[0, 4]] = np.nan                                              # a NaN dispersion leaves its gene out, whatever its counts
    beta, info = engine.nb_design_shrink(C["c"], C["X"], C["s"], alpha, C["mle"], C["far"], C["S"], return_info=True)
    gone = ~K.live_genes(C["c"], alpha)
    assert gone[[0, 4]].all()
    np.testing.assert_array_equal(np.isnan(beta).all(axis=1), gone)
    np.testing.assert_array_equal(np.isnan(beta).any(axis=1), gone)
    np.testing.assert_array_equal(np.isnan(info["objective"]), gone)
    np.testing.assert_array_equal(np.isnan(info["information"]).all(axis=(1, 2)), gone)
    assert not info["flags"][gone].any() and not info["steps"][gone].any()
    np.testing.assert_array_equal(beta[~gone], _shrink(C)[0][~gone])
    # a non-finite maximum-likelihood coefficient in an unshrunk column leaves its gene out as well; in the shrunk column it is not read
    mle = np.array(C["mle"])
    mle[1, 0], mle[7, 2], mle[8, 3] = np.nan, np.inf, np.nan
    beta, info = engine.nb_design_shrink(C["c"], C["X"], C["s"], C["alpha"], mle, C["far"], C["S"], return_info=True)
    gone = ~K.live_genes(C["c"], C["alpha"])
    assert not gone[[1, 7, 8]].any()
    gone[[1, 7]] = True
    np.testing.assert_array_equal(np.isnan(beta).all(axis=1), gone)
    np.testing.assert_array_equal(np.isnan(info["objective"]), gone)
    np.testing.assert_array_equal(np.isnan(info["information"]).all(axis=(1, 2)), gone)
    assert not info["flags"][gone].any() and not info["steps"][gone].any()
    np.testing.assert_array_equal(beta[~gone], _shrink(C)[0][~gone])


# ---- (7) tl ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("test", ["wald", "lrt"])
def test_lfc_shrink_design_is_the_host_tail_of_the_engine_calls(test):
    counts, meta = pseudobulk_with_a_group_of_zeros()
    plain = tl.compute_pseudobulk_DE(counts, meta, covariates=["batch", "age"], test=test, **ARGS)
    sub = counts.loc[plain.attrs["design"].index]
    out = tl.lfc_shrink_design(sub, plain)
    hold_shrunk_frame(out, plain, sub)
    assert out.attrs["test"] == test
    fixed = tl.lfc_shrink_design(sub, plain, prior_scale=0.5)
    pd.testing.assert_frame_equal(fixed, shrunk_design_by_hand(sub, plain, 0.5)[0], check_exact=True)
    assert fixed.attrs["prior_scale"] == 0.5 and fixed.attrs["prior_var"] == 0.25
    with pytest.raises(ValueError, match="already shrunken"):
        tl.lfc_shrink_design(sub, out)


# ---- the workspace guard ----------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_scratch():
    """test_gpu_ws_guard.py's rule for the new call: under the guard (every slot filled with a pattern before it is handed out,
    canaries past the request) the results keep their bits, left-out genes included, and nothing is written past a request"""
    C = _case(*CASES[2])
    plain = _all(C, np.ascontiguousarray(C["c"]))
    with engine.ws_guard() as guard:
        guarded = _all(C, np.ascontiguousarray(C["c"]))
    seen, damage = guard.result
    for a, b in zip(plain, guarded):
        np.testing.assert_array_equal(a, b)
    assert damage is None, damage
    assert {"WS_NB_Y", "WS_NB_SF", "WS_NB_BAD", "WS_NB_PRIOR", "WS_NB_OUT", "WS_NB_FIT_INT"} <= seen
