"""K27 without a device: the restatement (tests/nb_design_shrink_restatement.py) pinned to scipy on its own, the condition on the
generator that keeps the device test's parity honest, the refusals of pilot_ot_nb_design_shrink, engine.nb_design_shrink and
tl.lfc_shrink_design before any device work, and tl.lfc_shrink_design's host tail with the device call replaced by the restatement.

Tolerances.  scipy's local optimiser stops at its own gradient tolerance, so the restatement's posterior may exceed scipy's best by
any amount (another basin) and fall short of it by at most 1e-6 (the last grid spacing of the search is t_end (2 / 63)^5 / 63 < 1e-8
and p is smooth).  P against scipy's logpmf / logpdf: 1e-9 of the magnitudes added (the pins run at max(alpha, 1e-3), as
test_nb_design_args.py's, because scipy's logpmf loses digits at r = 1e8)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pandas as pd
import pytest
from scipy import optimize, stats

import nb_design_restatement as DR
import nb_design_shrink_restatement as K
import nb_glm_restatement as RR
import nb_shrink_restatement as SR
from conftest import ROOT
from pilot_amd import _lib, engine, tl
from test_nb_design_args import _fakes, pseudobulk_with_batch


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())


@functools.lru_cache(maxsize=None)
def solved(m, p, G, S):
    """a case of the device test solved by the restatement alone, the maximum-likelihood coefficients from K26's restatement"""
    C = K.case_inputs(m, p, G, S)
    k = p - 1
    mle = DR.final_fit(C["c"], C["X"], C["s"], C["alpha"])[0]
    far = K.far_end(mle[:, k])
    found = K.search(C["c"], C["X"], C["s"], C["alpha"], far, S, k, start=mle)
    return dict(C, k=k, mle=mle, far=far, found=found)


# ---- pins for the restatement -------------------------------------------------------------------------------------------------------
def _log_posterior(c, X, s, alpha, beta, S, k, sigma0=K.SIGMA0):
    """the full log posterior of one gene from scipy's densities"""
    mu = s * np.exp(X @ beta)
    r = 1.0 / alpha
    others = np.delete(beta, k)
    return float(stats.nbinom.logpmf(c, r, r / (r + mu)).sum() + stats.norm.logpdf(others, scale=sigma0).sum()
                 + stats.cauchy.logpdf(beta[k], scale=S))


@functools.lru_cache(maxsize=None)
def _pin_case():
    C = K.case_inputs(12, 4, 14, 0.3)
    alpha = np.where(np.isnan(C["alpha"]), np.nan, np.maximum(C["alpha"], 1e-3))
    mle = DR.final_fit(C["c"], C["X"], C["s"], alpha)[0]
    far = K.far_end(mle[:, 3])
    return dict(C, alpha=alpha, mle=mle, far=far, found=K.search(C["c"], C["X"], C["s"], alpha, far, 0.3, 3, start=mle))


def test_the_mode_is_scipys_best_over_five_starts():
    C = _pin_case()
    c, X, s, alpha, S, found = C["c"], C["X"], C["s"], C["alpha"], C["S"], C["found"]
    live = np.flatnonzero(K.live_genes(c, alpha))
    assert live.size == 12 and np.isnan(found["beta"][~K.live_genes(c, alpha)]).all()
    agree = excused = 0
    for j in live:
        f = lambda beta: -_log_posterior(c[:, j], X, s, alpha[j], beta, S, 3)
        ours = -f(found["beta"][j])
        zero = np.array(C["mle"][j])
        zero[3] = 0.0
        best, where = -np.inf, None
        for frac in (0.0, 0.25, 0.5, 0.75, 1.0):
            start = zero + frac * (C["mle"][j] - zero)
            start[:3] = K.solve_others(c[:, j:j + 1], X, s, alpha[j:j + 1], start[3:4], 3, start=start[None])[0][0, :3]
            got = optimize.minimize(f, start, method="BFGS", options={"gtol": 1e-9})
            if -got.fun > best:
                best, where = -got.fun, got.x
        if where[3] * C["far"][j] >= 0 and abs(where[3]) <= abs(C["far"][j]):
            assert ours >= best - 1e-6, (j, ours, best)
        else:
            # the rule searches [0, sg E] only, as K23's: a mode that scipy finds on the other side of 0 (the normal prior on the
            # other coefficients can move the profile's top across 0 when the maximum-likelihood coefficient is small against it)
            # is outside the definition, and the search ends on 0
            assert found["t"][j] == 0.0 and abs(where[3]) < 0.01, (j, where, found["beta"][j])
            excused += 1
            continue
        # P is the posterior up to a constant of the gene: the same difference between two points by either formula
        pair = np.stack([found["beta"][j], C["mle"][j]])
        mine = K.P(c[:, [j, j]], X, s, alpha[[j, j]], pair, S, 3)
        theirs = np.array([-f(pair[0]), -f(pair[1])])
        scale = K.bound(c[:, [j, j]], X, s, alpha[[j, j]], pair, S, 3).max() / (64 * 2.0 ** -53)
        assert abs((mine[0] - mine[1]) - (theirs[0] - theirs[1])) <= 1e-9 * scale, j
        if abs(ours - best) <= 1e-6 and np.abs(where - found["beta"][j]).max() <= 1e-3:
            agree += 1
    assert agree >= 8                                                    # scipy finds the same mode in most genes
    assert excused <= 2                                                  # and the one-sided search excuses few of the 12


def test_the_profile_step_vanishes_at_the_mode_and_the_information_is_the_explicit_gram():
    C = _pin_case()
    c, X, s, alpha, found = C["c"], C["X"], C["s"], C["alpha"], C["found"]
    live = np.flatnonzero(K.live_genes(c, alpha))
    beta = found["beta"][live]
    assert np.abs(K.profile_step(c[:, live], X, s, alpha[live], beta, 3)).max() <= 1e-9
    assert np.abs(K.profile_step(c[:, live], X, s, alpha[live], beta + 0.01, 3)).max() > 1e-4
    for n, j in enumerate(live):
        mu = s * np.exp(X @ beta[n])
        w = mu * (1.0 + alpha[j] * c[:, j]) / (1.0 + alpha[j] * mu) ** 2
        M = X.T @ np.diag(w) @ X
        assert (np.abs(found["info"][j] - M) <= 1e-12 * np.sqrt(np.outer(np.diag(M), np.diag(M)))).all()


def test_sd_is_numpys_inverse_and_the_engines():
    C = _pin_case()
    found, S = C["found"], C["S"]
    sd = K.posterior_sd(found["beta"], found["info"], S, 3)
    live = K.live_genes(C["c"], C["alpha"])
    assert np.isnan(sd[~live]).all() and np.isfinite(sd[live]).sum() >= 8
    for j in np.flatnonzero(np.isfinite(sd)):
        b = found["beta"][j, 3]
        H = found["info"][j] + np.diag([1 / 225.0, 1 / 225.0, 1 / 225.0, 2 * (S * S - b * b) / (S * S + b * b) ** 2])
        assert np.linalg.eigvalsh(H).min() > 0
        assert abs(sd[j] - np.sqrt(np.linalg.inv(H)[3, 3])) <= 1e-12 * sd[j]
    got = engine.nb_design_posterior_sd(found["beta"], found["info"], S)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(sd))
    np.testing.assert_allclose(got[np.isfinite(sd)], sd[np.isfinite(sd)], rtol=1e-9)
    # the shrunk column in the middle: the same number once the columns are permuted
    order = [0, 3, 1, 2]
    moved = engine.nb_design_posterior_sd(found["beta"][:, order], found["info"][:, order][:, :, order], S, coef=1)
    np.testing.assert_allclose(moved[np.isfinite(sd)], sd[np.isfinite(sd)], rtol=1e-9)
    np.testing.assert_array_equal(engine.nb_design_far_end(C["mle"][:, 3]), C["far"])
    np.testing.assert_array_equal(engine.nb_design_far_end([0.0, -0.0, 2.5, -3.0, np.nan]), [1.0, 1.0, 3.5, -4.0, 1.0])


def test_two_columns_are_k23():
    """X = [1, codes]: the objective is nb_shrink_restatement's to rounding, and so are the weights and the standard deviation"""
    rng = np.random.default_rng(23)
    s = RR.size_factors(rng, 12)
    codes = rng.permutation(np.repeat(np.arange(2), (7, 5))).astype(np.int32)
    c = RR.nb_class(rng, s, codes, 2, 20)
    alpha = np.clip(0.05 + 2.0 / np.maximum((c / s[:, None]).mean(axis=0), 1.0), RR.MIN_DISP, 12.0)
    X = np.stack([np.ones(12), codes.astype(np.float64)], axis=1)
    b0, b1 = rng.normal(3.0, 1.0, (20, 5)), rng.normal(0.0, 1.0, (20, 5))
    mine = K.P(c, X, s, alpha, np.stack([b0, b1], axis=2), 0.3, 1)
    theirs = SR.P(c, codes, s, alpha, b0, b1, 0.3)
    B = np.stack([SR.bound(c, codes, s, alpha, b0[:, i], b1[:, i], 0.3) for i in range(5)], axis=1)
    assert (np.abs(mine - theirs) <= B).all()
    q, _, flags = RR.group_fits(c, codes, 2, s, alpha)
    far = SR.far_end(q, flags)
    old = SR.search(c, codes, s, alpha, far, 0.3)
    new = K.search(c, X, s, alpha, far, 0.3, 1)
    res = SR.resolved(c, codes, s, alpha, far, 0.3, old)
    assert res.sum() >= 15
    assert (np.abs(K.t_of(new["beta"][:, 1], 0.3) - old["t"])[res] <= 2e-4).all()
    w0, w1 = SR.weights(c, codes, s, alpha, new["beta"][:, 0], new["beta"][:, 1])
    np.testing.assert_allclose(new["info"], np.stack([np.stack([w0 + w1, w1], axis=1), np.stack([w1, w1], axis=1)], axis=1), rtol=1e-12)
    np.testing.assert_allclose(K.posterior_sd(new["beta"], new["info"], 0.3, 1), SR.posterior_sd(new["beta"][:, 1], w0, w1, 0.3), rtol=1e-9)
    np.testing.assert_allclose(engine.nb_design_posterior_sd(new["beta"], new["info"], 0.3),
                               engine.nb_posterior_sd(new["beta"][:, 1], w0, w1, 0.3), rtol=1e-9)


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: "m%d-p%d-G%d-S%g" % c)
def test_the_restatement_alone_resolves_the_nb_class(case):
    """the cap that keeps the device test's rule (2) honest: a condition on the generator, checked without the device"""
    m, p, G, S = case
    assert S > 0.02 or m <= 12                                          # (test_gpu_nb_shrink.py's docstring: B grows with the counts)
    C = solved(*case)
    res = K.resolved(C["c"], C["X"], C["s"], C["alpha"], C["far"], S, C["k"], C["found"])
    nb = C["kind"] == 0
    assert nb.sum() >= 1 and res[nb].sum() >= 0.9 * nb.sum(), (res[nb].sum(), nb.sum())
    assert not C["found"]["flags"].any()
    assert sorted(set(C["kind"])) == list(range(min(G, len(K.CLASSES))))


# ---- the C entry point ---------------------------------------------------------------------------------------------------------------
X6 = [[1.0, 0.0, -1.0], [1.0, 1.0, 0.5], [1.0, 0.0, 0.2], [1.0, 1.0, 1.3], [1.0, 1.0, -0.7], [1.0, 0.0, 0.1]]
GOOD = dict(y=True, dtype=1, m=6, genes=5, ld=5, X=X6, p=3, coef=2, sf=[1.0, 0.5, 2.0, 1.0, 1.5, 0.7], disp=[0.1] * 5, mle=np.zeros((5, 3)),
            far=[1.0, -2.0, 1.5, 1.0, 3.0], S=0.3, other=15.0, out=True, objective=True, info=True, flags=True)


def _call(**kw):
    a = dict(GOOD)
    a.update(kw)
    L = _lib.load()
    Y = np.ones((6, 8), dtype=np.float64)
    arr = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    X, sf, disp, mle, far = arr(a["X"]), arr(a["sf"]), arr(a["disp"]), arr(a["mle"]), arr(a["far"])
    ptr = lambda v: None if v is None else _lib.dptr(v)
    d = [np.zeros(512) for _ in range(3)]
    flags = np.zeros(64, dtype=np.int32)
    bad_row, bad_col, n_bound = ctypes.c_longlong(5), ctypes.c_int(5), ctypes.c_int(5)
    y = ctypes.c_void_p(Y.ctypes.data) if a["y"] else None
    rc = L.pilot_ot_nb_design_shrink(y, 0, a["dtype"], a["m"], a["genes"], a["ld"], ptr(X), a["p"], a["coef"], ptr(sf), ptr(disp), ptr(mle),
                                     ptr(far), a["S"], a["other"], _lib.dptr(d[0]) if a["out"] else None,
                                     _lib.dptr(d[1]) if a["objective"] else None, _lib.dptr(d[2]) if a["info"] else None,
                                     _lib.iptr(flags) if a["flags"] else None, ctypes.byref(n_bound), ctypes.byref(bad_row),
                                     ctypes.byref(bad_col))
    assert bad_row.value == -1 and bad_col.value == -1 and n_bound.value == 0
    return rc, L.pilot_ot_last_error()


def _wide(p):
    return [[1.0] + [float((j >> k) & 1) for k in range(p - 1)] for j in range(6)]


BAD = [
    (dict(y=False), b"NULL"), (dict(X=None), b"NULL"), (dict(sf=None), b"NULL"), (dict(out=False), b"NULL"), (dict(disp=None), b"NULL"),
    (dict(mle=None), b"NULL"), (dict(far=None), b"NULL"), (dict(objective=False), b"NULL"), (dict(info=False), b"NULL"),
    (dict(flags=False), b"NULL"),
    (dict(genes=0, ld=0), b"n_genes=0"), (dict(ld=4), b"ld=4"), (dict(dtype=2), b"dtype"), (dict(m=1), b"m=1"),
    (dict(sf=[1.0, 0.0, 2.0, 1.0, 1.5, 0.7]), b"size_factors[1]"), (dict(sf=[1.0, 0.5, 2.0, np.nan, 1.5, 0.7]), b"size_factors[3]"),
    (dict(disp=[0.1, 0.1, 9e-9, 0.1, 0.1]), b"dispersion[2]"), (dict(disp=[10.5] + [0.1] * 4), b"dispersion[0]"),
    (dict(p=1), b"p=1"), (dict(p=9), b"p=9"), (dict(p=0), b"p=0"), (dict(p=6, X=_wide(6), coef=1), b"no residual degree of freedom"),
    (dict(X=[[1.0, 0.0, -1.0]] * 3 + [[0.5, 1.0, 1.3]] + [[1.0, 1.0, 0.1]] * 2), b"X[3, 0]=0.5"),
    (dict(X=[[1.0, 0.0, -1.0]] * 4 + [[1.0, np.nan, 1.3]] + [[1.0, 1.0, 0.1]]), b"X[4, 1]"),
    (dict(coef=0), b"coef=0"), (dict(coef=3), b"coef=3"), (dict(coef=-1), b"coef=-1"), (dict(p=2, X=_wide(2), coef=2), b"coef=2"),
    (dict(far=[1.0, np.nan, 1.5, 1.0, 3.0]), b"far_end[1]"), (dict(far=[1.0, 2.0, 1.5, 1.0, np.inf]), b"far_end[4]"),
    (dict(S=0.0), b"prior_scale"), (dict(S=-1.0), b"prior_scale"), (dict(S=np.nan), b"prior_scale"), (dict(S=np.inf), b"prior_scale"),
    (dict(other=0.0), b"other_scale"), (dict(other=np.inf), b"other_scale"),
]


@pytest.mark.parametrize("bad,fragment", BAD)
def test_entry_point_refuses_before_any_hip_call(bad, fragment):
    rc, msg = _call(**bad)
    assert rc == _lib.EINVAL and fragment in msg, (bad, msg)


def test_too_many_samples_and_good_arguments():
    limits = engine.nb_design_limits()["max_samples"]
    m = limits[3] + 1
    X = np.stack([np.ones(m), np.arange(m) % 2, np.sin(np.arange(m))], axis=1)
    rc, msg = _call(m=m, X=X, sf=[1.0] * m, genes=1, ld=1, disp=[0.1], mle=np.zeros((1, 3)), far=[1.0])
    assert rc == _lib.ENOTSUP and b"staged in LDS" in msg
    with pytest.raises(NotImplementedError, match="staged in LDS"):
        engine.nb_design_shrink(np.ones((m, 1)), X, np.ones(m), [0.1], np.zeros((1, 3)), [1.0], 0.3)
    want = _lib.OK if _lib.device_count() > 0 else _lib.EHIP
    for kw in (dict(), dict(ld=8), dict(dtype=0), dict(coef=1), dict(p=2, X=_wide(2), coef=1, mle=np.zeros((5, 2))),
               dict(disp=[1e-8, 10.0, np.nan, 0.1, 0.1]), dict(mle=np.full((5, 3), np.nan))):
        rc, msg = _call(**kw)
        assert rc == want, (kw, msg)


def test_symbol_and_header(tmp_path):
    assert "pilot_ot_nb_design_shrink" in _lib.SYMBOLS and hasattr(_lib.load(), "pilot_ot_nb_design_shrink")
    assert engine.NB_INTERCEPT_SCALE == K.SIGMA0 == 15.0
    src = tmp_path / "t.c"
    src.write_text('#include "pilot_ot.h"\nint main(void){return pilot_ot_nb_design_shrink(0, 0, 1, 6, 1, 1, 0, 3, 2, 0, 0, 0, 0, 0.3, 15.0, 0, 0, 0, '
                   '0, 0, 0, 0) == PILOT_OT_OK;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


# ---- engine and tl refuse on the host --------------------------------------------------------------------------------------------------
Y6, S6, XA = np.ones((6, 5)), np.array([1.0, 0.5, 2.0, 1.0, 1.5, 0.7]), np.array(X6)
ENGINE_GOOD = dict(counts=Y6, design=XA, size_factors=S6, dispersion=np.full(5, 0.1), beta_mle=np.zeros((5, 3)), far_end=np.ones(5),
                   prior_scale=0.3)


@pytest.mark.parametrize("kw", [
    dict(counts=np.ones(6)), dict(counts=np.ones((6, 5), dtype=np.int64)), dict(design=XA[:5]), dict(design=XA[:, :1]),
    dict(design=np.hstack([XA] * 3)), dict(design=XA[:, ::-1]), dict(design=np.stack([XA[:, 0], XA[:, 1], 1.0 - XA[:, 1]], axis=1)),
    dict(size_factors=S6[:5]), dict(size_factors=-S6), dict(dispersion=np.full(4, 0.1)), dict(dispersion=[0.1, 0.1, 9e-9, 0.1, 0.1]),
    dict(dispersion=[10.5, 0.1, 0.1, 0.1, 0.1]), dict(beta_mle=np.zeros((5, 2))), dict(beta_mle=np.zeros(5)), dict(beta_mle=np.zeros((4, 3))),
    dict(far_end=np.ones(4)), dict(far_end=[1.0, np.nan, 1.0, 1.0, 1.0]), dict(far_end=[1.0, np.inf, 1.0, 1.0, 1.0]),
    dict(prior_scale=0.0), dict(prior_scale=-0.3), dict(prior_scale=np.nan), dict(prior_scale="0.3"), dict(prior_scale=True),
    dict(other_scale=0.0), dict(other_scale=np.inf), dict(coef=0), dict(coef=3), dict(coef=-3), dict(coef=1.0), dict(coef=True),
])
def test_engine_refuses_before_the_library(no_library, kw):
    a = dict(ENGINE_GOOD)
    a.update(kw)
    with pytest.raises(ValueError):
        engine.nb_design_shrink(**a)


def test_good_engine_arguments_reach_the_library(no_library):
    for kw in (dict(), dict(coef=1), dict(coef=-2), dict(dispersion=[0.1, np.nan, 1e-8, 6.0, 0.1]), dict(other_scale=3.0, return_info=True)):
        with pytest.raises(AssertionError, match="the library was touched"):
            engine.nb_design_shrink(**dict(ENGINE_GOOD, **kw))


def test_posterior_sd_refuses_bad_shapes():
    for args in ((np.zeros(5), np.zeros((5, 3, 3)), 0.3), (np.zeros((5, 3)), np.zeros((5, 3, 2)), 0.3), (np.zeros((5, 3)), np.zeros((5, 3, 3)), 0.0)):
        with pytest.raises(ValueError):
            engine.nb_design_posterior_sd(*args)
    with pytest.raises(ValueError):
        engine.nb_design_posterior_sd(np.zeros((5, 3)), np.zeros((5, 3, 3)), 0.3, coef=0)


ARGS = dict(group1="T1", group2="T2", cluster_col="Predicted_Labels")


@functools.lru_cache(maxsize=None)
def pseudobulk_with_a_group_of_zeros():
    """test_nb_design_args.py's frame (12 samples, batch and age; gene 5 zero everywhere) with gene 7 zero in every T2 sample"""
    counts, meta = pseudobulk_with_batch()
    counts = counts.copy()
    counts.loc[(meta["stage"] == "T2").to_numpy(), "g007"] = 0.0
    return counts, meta


def shrunk_design_by_hand(sub, plain, prior_scale=None):
    """tl.lfc_shrink_design from the engine calls and the host tail written out; sub: the selected samples' counts, plain: the
    unshrunken frame.  Returns (frame, S, A, beta)."""
    c = np.ascontiguousarray(sub.to_numpy(dtype=np.float64))
    sf = tl.deseq2_size_factors(sub).to_numpy()
    X = plain.attrs["design"].to_numpy()
    mle = plain.attrs["coefficients"].loc[sub.columns].to_numpy()
    at = pd.Index(plain["gene"]).get_indexer(sub.columns)               # the frame's row of every gene of the table
    ln2 = np.log(2.0)
    disp, se = plain["dispersion"].to_numpy()[at], plain["lfcSE"].to_numpy()[at] * ln2
    bk = mle[:, -1]
    with np.errstate(invalid="ignore"):
        S, A = engine.nb_prior_scale(bk, se, use=np.isfinite(bk) & (np.abs(bk) < 10)) if prior_scale is None else (prior_scale, prior_scale ** 2)
        far = np.where(np.isnan(bk), 1.0, np.where(bk >= 0, np.abs(bk) + 1.0, -np.abs(bk) - 1.0))
    beta, info = engine.nb_design_shrink(c, X, sf, disp, mle, far, S, return_info=True)
    sd = engine.nb_design_posterior_sd(beta, info["information"], S)
    row = pd.Index(sub.columns).get_indexer(plain["gene"])              # the table's column of every row of the frame
    out = plain.copy()
    out["lfcMLE"], out["lfcMLESE"] = plain["log2FoldChange"], plain["lfcSE"]
    out["log2FoldChange"], out["lfcSE"] = (beta[:, -1] / ln2)[row], (sd / ln2)[row]
    return out, S, A, beta


def hold_shrunk_frame(out, plain, sub, prior_scale=None):
    """what every tl.lfc_shrink_design frame must satisfy, against the host tail recomputed from the same engine calls"""
    want, S, A, beta = shrunk_design_by_hand(sub, plain, prior_scale)
    assert list(out.columns) == list(plain.columns) + ["lfcMLE", "lfcMLESE"]
    pd.testing.assert_frame_equal(out, want, check_exact=True)
    assert out.attrs["shrink"] == "apeglm" and out.attrs["prior_scale"] == S and out.attrs["prior_var"] == A and out.attrs["n_at_bound"] == 0
    assert 0 < S <= 1.0
    np.testing.assert_array_equal(out.attrs["coefficients_shrunk"].to_numpy(), beta)
    assert list(out.attrs["coefficients_shrunk"].columns) == list(plain.attrs["design"].columns)
    assert list(out.attrs["coefficients_shrunk"].index) == list(sub.columns)
    for col in ("gene", "baseMean", "stat", "pvalue", "padj", "dispersion"):      # lfcShrink keeps the test and arrange(padj)
        pd.testing.assert_series_equal(out[col], plain[col], check_exact=True)
    pd.testing.assert_series_equal(out["lfcMLE"], plain["log2FoldChange"], check_names=False, check_exact=True)
    pd.testing.assert_series_equal(out["lfcMLESE"], plain["lfcSE"], check_names=False, check_exact=True)
    assert "lfcMLE" not in plain.columns and "shrink" not in plain.attrs     # the input is left as it was
    live = out["padj"].notna().to_numpy()
    nb = live & ~out["gene"].isin(["g007"]).to_numpy()                  # (g007 has a group of zeros)
    lfc, mle = out["log2FoldChange"].to_numpy(), out["lfcMLE"].to_numpy()
    assert (np.abs(lfc[nb]) <= np.abs(mle[nb]) + 1e-9).all()
    assert out.loc[~live, ["log2FoldChange", "lfcSE"]].isna().all().all() and np.isfinite(lfc[live]).all()
    assert (np.abs(lfc) < np.abs(mle) - 1e-3).sum() >= 10               # the prior does move the estimates
    # the group of zeros: the score of the likelihood decays like e^b, the maximum-likelihood fit stops where it meets K26's ridge,
    # 1e-6 |b|, the mode where it meets the Cauchy's 2 |b| / (S^2 + b^2) ~ 2 / |b|; for |b| < 100 the two differ by a factor of more
    # than 2e-2 / 1e-4 = 200 > e^5, so the mode lies more than 5 natural-log units inside
    zero = (out["gene"] == "g007").to_numpy()
    assert zero.sum() == 1 and np.isfinite(lfc[zero]).all() and np.isfinite(out["lfcSE"].to_numpy()[zero]).all()
    assert (np.abs(lfc[zero]) < np.abs(mle[zero]) - 5.0 / np.log(2.0)).all() and (np.abs(mle[zero]) * np.log(2.0) > 10).all()
    return want


def _fake_shrink(monkeypatch):
    """the device call of tl.lfc_shrink_design replaced by the restatement"""
    def shrink(counts, design, size_factors, dispersion, beta_mle, far_end, prior_scale, coef=-1, other_scale=K.SIGMA0, return_info=False):
        k = coef % design.shape[1]
        found = K.search(np.asarray(counts), design, size_factors, dispersion, far_end, prior_scale, k, other_scale, start=beta_mle)
        info = {"objective": found["p"], "information": found["info"], "flags": found["flags"], "steps": np.zeros(found["p"].size, dtype=np.int32),
                "n_at_bound": int(np.count_nonzero(found["flags"] & K.AT_BOUND)), "n_not_converged": 0}
        return (found["beta"], info) if return_info else found["beta"]

    monkeypatch.setattr(engine, "nb_design_shrink", shrink)


@pytest.mark.parametrize("test", ["wald", "lrt"])
def test_tl_lfc_shrink_design_on_the_restatement(monkeypatch, test):
    _fakes(monkeypatch)
    _fake_shrink(monkeypatch)
    counts, meta = pseudobulk_with_a_group_of_zeros()
    plain = tl.compute_pseudobulk_DE(counts, meta, covariates=["batch", "age"], test=test, **ARGS)
    sub = counts.loc[plain.attrs["design"].index]
    out = tl.lfc_shrink_design(sub, plain)
    hold_shrunk_frame(out, plain, sub)
    fixed = tl.lfc_shrink_design(sub, plain, prior_scale=0.5)
    pd.testing.assert_frame_equal(fixed, shrunk_design_by_hand(sub, plain, 0.5)[0], check_exact=True)
    assert fixed.attrs["prior_scale"] == 0.5 and fixed.attrs["prior_var"] == 0.25
    # the order of the table's columns does not matter
    shuffled = sub[sub.columns[::-1]]
    pd.testing.assert_frame_equal(tl.lfc_shrink_design(shuffled, plain, prior_scale=0.5)[list(fixed.columns)], fixed, check_exact=True)


def test_tl_refuses_before_the_library(monkeypatch):
    _fakes(monkeypatch)
    counts, meta = pseudobulk_with_a_group_of_zeros()
    plain = tl.compute_pseudobulk_DE(counts, meta, covariates=["batch"], **ARGS)
    sub = counts.loc[plain.attrs["design"].index]
    _fake_shrink(monkeypatch)
    shrunk = tl.lfc_shrink_design(sub, plain, prior_scale=0.5)
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())
    monkeypatch.setattr(engine, "nb_design_shrink", lambda *a, **k: _Untouchable().nb_design_shrink)
    k22 = plain.copy()
    del k22.attrs["design"]
    with pytest.raises(ValueError, match="lfc_shrink"):
        tl.lfc_shrink_design(sub, k22)
    with pytest.raises(ValueError, match="already shrunken"):
        tl.lfc_shrink_design(sub, shrunk)
    with pytest.raises(ValueError, match="genes"):
        tl.lfc_shrink_design(sub.iloc[:, :-1], plain)
    with pytest.raises(ValueError, match="genes"):
        tl.lfc_shrink_design(sub.rename(columns={"g003": "other"}), plain)
    with pytest.raises(ValueError, match="samples"):
        tl.lfc_shrink_design(sub.iloc[:-1], plain)
    with pytest.raises(ValueError, match="samples"):
        tl.lfc_shrink_design(sub.iloc[::-1], plain)
    with pytest.raises(ValueError, match="samples"):
        tl.lfc_shrink_design(counts, plain)
    for bad in (0.0, -1.0, np.nan, "0.3", True):
        with pytest.raises(ValueError, match="prior_scale"):
            tl.lfc_shrink_design(sub, plain, prior_scale=bad)
    with pytest.raises(ValueError, match="frame of compute_pseudobulk_DE"):
        tl.lfc_shrink_design(sub, plain.drop(columns=["lfcSE"]))
    with pytest.raises(ValueError, match="frame of compute_pseudobulk_DE"):
        tl.lfc_shrink_design(sub, None)


def test_the_refusals_of_the_de_calls_are_unchanged(no_library):
    counts, meta = pseudobulk_with_batch()
    for kw in (dict(shrink="apeglm"), dict(shrink="apeglm", test="lrt")):
        with pytest.raises(NotImplementedError, match="K23.*K25"):
            tl.compute_pseudobulk_DE(counts, meta, covariates=["batch"], **ARGS, **kw)
        with pytest.raises(NotImplementedError, match="lfc_shrink_design"):
            tl.get_pseudobulk_DE(None, None, "alpha", covariates=["batch"], **kw)
    with pytest.raises(NotImplementedError, match="K25"):
        tl.compute_pseudobulk_DE(counts, meta, covariates=["batch"], outliers="deseq2", **ARGS)
