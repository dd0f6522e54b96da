"""Cook's outlier handling under covariates (K28), the parts that need no device.

The restatement (tests/nb_design_cooks_restatement.py) is pinned where something independent exists here: its trimmed mean (K25's)
to scipy.stats.trim_mean at the fallback's ratio too, its cutoff to scipy.stats.f.ppf with p coefficients, its refined long-double
solve to the identity sum_j h_j = p - lambda tr(M^-1) and to numpy's float64 inverse, and the whole rule to K25's restatement
(nb_cooks_restatement.cooks) for X = [1, indicator] within the ridge's pull.  The case generator's cap -- every design keeps at least
90 % of its generated genes and one gene of every class -- is tested here.  pilot_ot_nb_design_cooks refuses every bad argument before
any HIP call; engine and tl raise before the library is touched; tl.outliers_design runs with the device calls replaced by the
restatements, against the host tail written out here (outliers_design_by_hand, which tests/test_gpu_nb_design_cooks.py runs on the
device calls)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pandas as pd
import pytest
from scipy import stats

import nb_cooks_restatement as CR
import nb_design_cooks_restatement as KR
import nb_design_restatement as DR
import nb_glm_restatement as RR
from conftest import ROOT
from pilot_amd import _lib, engine, tl
from test_nb_cooks_args import planted_table
from test_nb_design_args import _fakes


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())


# ---- pins for the restatement -------------------------------------------------------------------------------------------------------
def test_the_fallback_variance_is_scipys_trimmed_mean():
    rng = np.random.default_rng(0)
    for n in (8, 9, 24, 65):
        q = rng.gamma(2.0, 10.0, n)
        drop = n // 8
        prop = (drop + 0.5) / n                                          # (a proportion inside the step: no float product on its edge)
        t = stats.trim_mean(q, prop)
        want = 1.51 * stats.trim_mean((q - t) ** 2, prop)
        got = KR.robust_variance(q, np.arange(n), np.ones(n, dtype=np.int64))
        assert abs(got - want) <= 1e-13 * want
    # with a cell of three or more it is K25's per-group expression, the largest over those cells
    codes, size = np.repeat(np.arange(3), (2, 3, 7)), np.array([2, 3, 7])
    q = rng.gamma(2.0, 10.0, 12)
    per = [CR.trim_rule(n)[1] * CR.tm((q[codes == g] - CR.tm(q[codes == g], CR.trim_rule(n)[0])) ** 2, CR.trim_rule(n)[0]) for g, n in ((1, 3), (2, 7))]
    assert KR.robust_variance(q, codes, size) == max(per)


def test_cutoff_is_the_f_quantile_with_p_coefficients():
    for m, p in ((10, 2), (14, 3), (24, 4), (9, 8), (65, 8)):
        assert engine.nb_cooks_cutoff(m, p) == KR.cutoff(m, p) == float(stats.f.ppf(0.99, p, m - p))


def test_the_hat_diagonal_sums_to_p_less_the_ridge_and_is_numpys_inverse():
    rng = np.random.default_rng(1)
    for p, m in ((2, 10), (4, 24), (8, 9), (8, 65)):
        X = KR.numeric_design(rng, p, m) if p > 2 else KR.cell_design(rng, (3, 7))
        w = rng.gamma(2.0, 3.0, m)
        h, trace, kappa = KR.hat(w, X)
        assert abs(h.sum() - (p - trace)) <= 1e-13 * p and 0 < trace < 1e-3 and (h > 0).all() and (h < 1).all()
        M = (X * w[:, None]).T @ X + KR.RIDGE * np.eye(p)
        want = w * np.einsum("jk,kl,jl->j", X, np.linalg.inv(M), X)
        assert np.abs(h - want).max() <= 100 * p * kappa * 2.0 ** -53
        assert abs(KR.jacobi_cond(M) - kappa) <= 1e-9 * kappa


def ridge_pull(X, s, alpha, beta):
    """per gene, how far the ridge can move a coefficient of K26 from the unpenalised optimum: lambda |beta| / lambda_min(X^T W X)
    plus 1e-9, as tests/test_gpu_nb_design.py bounds it for the group roots"""
    mu = np.maximum(s[:, None] * np.exp(X @ beta.T), DR.MIN_MU)
    W = mu / (1.0 + alpha[None] * mu)
    lam_min = np.array([np.linalg.eigvalsh((X * W[:, g][:, None]).T @ X)[0] for g in range(beta.shape[0])])
    return DR.RIDGE * np.linalg.norm(beta, axis=1) / lam_min + 1e-9


def hold_to_k25(got, want, pull):
    """K28's answer `got` on X = [1, indicator] against K25's `want` (both with D, H or not, D_scale from `want`): the integers are
    the same; trimmed_base and alpha_robust do not see the coefficients and agree to 1e-12; with eps the ridge's pull on a
    coefficient, mu and w move by at most 2 eps relative (both coefficients add up in group 1) and M^-1 by lambda / lambda_min <= eps,
    so h moves by 3 eps relative and D, whose logarithmic derivatives in mu and h are at most 4 (in the c + mu form) and
    1 + 2 h / (1 - h), by 3 eps (5 + 2 h / (1 - h)); held with a margin of 4 for the second order"""
    for name in ("arg_max", "n_above", "n_replace"):
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    live = ~np.isnan(want["trimmed_base"])
    np.testing.assert_array_equal(np.isnan(got["trimmed_base"]), ~live)
    for name in ("trimmed_base", "alpha_robust"):
        ok = ~np.isnan(want[name])
        np.testing.assert_allclose(got[name][ok], want[name][ok], rtol=1e-12, atol=0)
    h = got["H"]
    with np.errstate(invalid="ignore"):
        allowed = 12.0 * pull[None] * (5.0 + 2.0 * h / (1.0 - h))
        err = np.abs(got["D"] - want["D"]) / want["D_scale"]
    ok = ~np.isnan(want["D"])
    assert np.isnan(got["D"][:, ~live]).all() and (err[ok] <= allowed[ok]).all(), np.nanmax(err / allowed)
    top = ~np.isnan(want["max_cooks"])
    assert (np.abs(got["max_cooks"][top] - want["max_cooks"][top]) <= (allowed * want["D_scale"]).max(axis=0)[top]).all()
    return float(np.nanmax(err[ok] / allowed[ok]))


@pytest.mark.parametrize("sizes", [(3, 7), (2, 5), (23, 24)], ids=lambda s: "%dx%d" % s)
def test_one_factor_design_is_k25(sizes):
    C = KR.design_case(("cells", sizes))
    X, s, alpha, c = C["X"], C["s"], C["alpha"], C["c"]
    codes = X[:, 1].astype(np.int32)
    q = RR.group_fits(c, codes, 2, s, alpha)[0]
    want = CR.cooks(c, codes, 2, s, alpha, q, C["cutoff"])
    live = ~np.isnan(C["want"]["trimmed_base"])
    pull = np.full(C["G"], np.nan)
    pull[live] = ridge_pull(X, s, alpha[live], C["beta"][live])
    print("worst share of the ridge bound: %.3g" % hold_to_k25(C["want"], want, pull))
    # the hat diagonal is the weight over its group's sum, up to the same pull
    j = int(np.flatnonzero(live)[0])
    mu = np.maximum(s * np.exp(X @ C["beta"][j]), DR.MIN_MU)
    w = mu / (1.0 + alpha[j] * mu)
    np.testing.assert_allclose(C["want"]["H"][:, j], w / np.bincount(codes, weights=w)[codes], rtol=1e-6)


# ---- the cells --------------------------------------------------------------------------------------------------------------------------
def test_cells_by_first_appearance():
    rows = np.array([[1.0, 0.0, 0.5], [1.0, 1.0, 0.5], [1.0, 0.0, 0.5], [1.0, 1.0, -0.5], [1.0, 1.0, 0.5], [1.0, 0.0, 0.5]])
    codes, n = engine.nb_design_cells(rows)
    assert codes.dtype == np.int32 and codes.tolist() == [0, 1, 0, 2, 1, 0] and n == 3
    rng = np.random.default_rng(3)
    for X in (rows, np.repeat(rows, 3, axis=0), KR.numeric_design(rng, 4, 24), KR.cell_design(rng, (1, 3, 7, 2))):
        for _ in range(3):
            Xp = X[rng.permutation(X.shape[0])]
            codes, n = engine.nb_design_cells(Xp)
            want, wn = KR.cells(Xp)
            np.testing.assert_array_equal(codes, want)
            assert n == wn == len(np.unique(Xp, axis=0))
            first = [int(np.flatnonzero(codes == g)[0]) for g in range(n)]
            assert first == sorted(first)                                # numbered by first appearance
            for g in range(n):
                assert (Xp[codes == g] == Xp[first[g]]).all()
    assert engine.nb_design_cells(KR.numeric_design(rng, 4, 24))[1] == 24   # all distinct: every cell a singleton
    assert engine.nb_design_cells(np.array([[1.0, 0.0], [1.0, -0.0]]))[1] == 2   # bit-identical, not numerically equal
    for bad in (np.ones(5), np.ones((0, 3)), np.array([["a", "b"]])):
        with pytest.raises(ValueError):
            engine.nb_design_cells(bad)


# ---- the generator's cap ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KR.DESIGN_KEYS, ids=str)
def test_every_case_keeps_nine_genes_in_ten_and_every_class(key):
    C = KR.design_case(key)
    assert C["generated"] == KR.GENERATED and C["G"] >= 0.9 * C["generated"] and C["G"] >= 65
    assert sorted(set(C["kind"])) == list(range(len(KR.CLASSES)))
    W = C["want"]
    assert KR.conditions_hold(W, C["s"], C["cutoff"]).all() and np.nanmax(W["kappa"]) <= KR.MAX_COND
    name = lambda n: C["kind"] == KR.CLASSES.index(n)
    assert np.isnan(W["max_cooks"][name("zeros") | name("nan dispersion")]).all()
    if key[0] == "numeric":                                              # every cell a singleton: distances, but nothing to replace or flag
        assert C["n_cells"] == C["m"] and np.isnan(W["max_cooks"]).all() and not W["n_replace"].any() and (W["arg_max"] == -1).all()
        assert np.isfinite(W["D"][:, name("clean")]).all() and np.isfinite(W["alpha_robust"][name("clean")]).all()
    else:
        if C["sizes"].max() >= KR.MIN_REPLACE:
            assert (W["n_replace"][name("outlier in a replaceable cell")] >= 1).all()
        if ((C["sizes"] >= KR.MIN_GROUP) & (C["sizes"] < KR.MIN_REPLACE)).any():
            flag = name("outlier in a flaggable cell")
            assert (W["n_replace"][flag] == 0).all() and (W["max_cooks"][flag] > C["cutoff"]).all()


# ---- the C entry point ------------------------------------------------------------------------------------------------------------------
X6 = [[1.0, 0.0, -1.0], [1.0, 1.0, 0.5], [1.0, 0.0, -1.0], [1.0, 1.0, 1.3], [1.0, 1.0, 0.5], [1.0, 0.0, 0.1]]
GOOD = dict(y=True, dtype=1, m=6, genes=5, ld=5, X=X6, p=3, cells=[0, 1, 0, 2, 1, 3], nc=4, sf=[1.0, 0.5, 2.0, 1.0, 1.5, 0.7], disp=[0.1] * 5,
            beta=np.zeros((5, 3)), cutoff=3.0, min_replace=7, out=True, D=False, ld_D=5, H=False, ld_H=5)


def _call(**kw):
    a = dict(GOOD)
    a.update(kw)
    L = _lib.load()
    Y = np.ones((6, 8), dtype=np.float64)
    arr = lambda v, t=np.float64: None if v is None else np.ascontiguousarray(v, dtype=t)
    X, cells, sf, disp, beta = arr(a["X"]), arr(a["cells"], np.int32), arr(a["sf"]), arr(a["disp"]), arr(a["beta"])
    ptr = lambda v, f=_lib.dptr: None if v is None else f(v)
    d = [np.zeros(64) for _ in range(3)]
    i = [np.zeros(64, dtype=np.int32) for _ in range(3)]
    Dbuf, Hbuf = np.zeros(64), np.zeros(64)
    bad_row, bad_col = ctypes.c_longlong(5), ctypes.c_int(5)
    rc = L.pilot_ot_nb_design_cooks(ctypes.c_void_p(Y.ctypes.data) if a["y"] else None, 0, a["dtype"], a["m"], a["genes"], a["ld"], ptr(X), a["p"],
                                    ptr(cells, _lib.iptr), a["nc"], ptr(sf), ptr(disp), ptr(beta), a["cutoff"], a["min_replace"],
                                    _lib.dptr(d[0]) if a["out"] else None, _lib.dptr(d[1]), _lib.iptr(i[0]), _lib.iptr(i[1]), _lib.iptr(i[2]),
                                    _lib.dptr(d[2]), ctypes.c_void_p(Dbuf.ctypes.data) if a["D"] else None, 0, a["ld_D"],
                                    ctypes.c_void_p(Hbuf.ctypes.data) if a["H"] else None, 0, a["ld_H"], ctypes.byref(bad_row),
                                    ctypes.byref(bad_col))
    assert bad_row.value == -1 and bad_col.value == -1
    return rc, L.pilot_ot_last_error()


def _wide(p):
    return [[1.0] + [float((j >> k) & 1) for k in range(p - 1)] for j in range(6)]


def _beta_with(j, t, v):
    beta = np.zeros((5, 3))
    beta[j, t] = v
    return beta


@pytest.mark.parametrize("bad,fragment", [
    (dict(y=False), b"NULL"), (dict(X=None), b"NULL"), (dict(cells=None), b"NULL"), (dict(sf=None), b"NULL"), (dict(out=False), b"NULL"),
    (dict(disp=None), b"NULL"), (dict(beta=None), b"NULL"),
    (dict(genes=0, ld=0), b"n_genes=0"), (dict(ld=4), b"ld=4"), (dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"),
    (dict(m=1), b"m=1"), (dict(m=0), b"m=0"),
    (dict(sf=[1.0, 0.0, 2.0, 1.0, 1.5, 0.7]), b"size_factors[1]"), (dict(sf=[1.0, 0.5, 2.0, np.nan, 1.5, 0.7]), b"size_factors[3]"),
    (dict(sf=[1.0, 0.5, 2.0, 1.0, np.inf, 0.7]), b"size_factors[4]"),
    (dict(disp=[0.1, 0.1, 9e-9, 0.1, 0.1]), b"dispersion[2]"), (dict(disp=[10.5] + [0.1] * 4), b"dispersion[0]"),
    (dict(disp=[0.1, np.inf, 0.1, 0.1, 0.1]), b"dispersion[1]"),
    (dict(cutoff=0.0), b"cutoff"), (dict(cutoff=-1.0), b"cutoff"), (dict(cutoff=np.nan), b"cutoff"), (dict(cutoff=np.inf), b"cutoff"),
    (dict(min_replace=2), b"min_replace=2"), (dict(min_replace=0), b"min_replace=0"), (dict(min_replace=-7), b"min_replace=-7"),
    (dict(D=True, ld_D=4), b"ld_D=4"), (dict(H=True, ld_H=4), b"ld_H=4"),
    (dict(p=1), b"p=1"), (dict(p=9), b"p=9"), (dict(p=0), b"p=0"),
    (dict(p=6, X=_wide(6), cells=[0, 1, 2, 3, 4, 5], nc=6), b"no residual degree of freedom"),
    (dict(X=[[1.0, 0.0, -1.0]] * 3 + [[0.5, 1.0, 1.3]] + [[1.0, 1.0, 0.1]] * 2), b"X[3, 0]=0.5"),
    (dict(X=[[1.0, 0.0, -1.0]] * 4 + [[1.0, np.nan, 1.3]] + [[1.0, 1.0, 0.1]]), b"X[4, 1]"),
    (dict(nc=0), b"n_cells=0"), (dict(nc=7), b"n_cells=7"), (dict(nc=-1), b"n_cells=-1"),
    (dict(cells=[0, 1, 0, 4, 1, 3]), b"cells[3]=4"), (dict(cells=[0, -1, 0, 2, 1, 3]), b"cells[1]=-1"),
    (dict(cells=[0, 1, 0, 2, 1, 0]), b"cells[5]=0: row 5 of X differs from row 0"), (dict(cells=[0, 1, 1, 2, 1, 3]), b"cells[2]=1: row 2 of X differs"),
    (dict(nc=5), b"cell 4 has no sample"), (dict(cells=[0, 1, 0, 3, 1, 4], nc=5), b"cell 2 has no sample"),
    (dict(beta=_beta_with(3, 1, np.nan)), b"beta[3, 1]"), (dict(beta=_beta_with(0, 0, np.inf)), b"beta[0, 0]"),
    (dict(beta=_beta_with(4, 2, -np.inf)), b"beta[4, 2]"),
])
def test_entry_point_refuses_before_any_hip_call(bad, fragment):
    rc, msg = _call(**bad)
    assert rc == _lib.EINVAL and fragment in msg, (bad, msg)


def test_too_many_samples_and_good_arguments():
    limits = engine.nb_design_limits()["max_samples"]
    assert all(8 * (2 * n + (1 << (n - 1).bit_length())) <= 96 * 1024 for n in limits.values())   # c, q and the sort buffer fit at every limit
    m = limits[3] + 1
    X = np.stack([np.ones(m), np.arange(m) % 2, np.sin(np.arange(m))], axis=1)
    rc, msg = _call(m=m, X=X, cells=np.arange(m), nc=m, sf=[1.0] * m, genes=1, ld=1, disp=[0.1], beta=np.zeros((1, 3)))
    assert rc == _lib.ENOTSUP and b"counts, normalised counts and sort buffer are staged in LDS" in msg    # (X is not: K28 reads it from HBM)
    with pytest.raises(NotImplementedError, match="staged in LDS"):
        engine.nb_design_cooks(np.ones((m, 1)), X, np.ones(m), [0.1], np.zeros((1, 3)), 3.0)
    want = _lib.OK if _lib.device_count() > 0 else _lib.EHIP
    for kw in (dict(), dict(ld=8), dict(dtype=0), dict(D=True), dict(H=True, ld_H=7), dict(D=True, H=True), dict(min_replace=3), dict(ld_D=0, ld_H=0),
               dict(p=2, X=_wide(2), cells=[0, 1, 0, 1, 0, 1], nc=2, beta=np.zeros((5, 2))),
               dict(disp=[1e-8, 10.0, np.nan, 0.1, 0.1], beta=_beta_with(2, 1, np.nan)),
               dict(cells=[3, 1, 3, 2, 1, 0])):                           # (any numbering of the cells is taken: first appearance is the engine's)
        rc, msg = _call(**kw)
        assert rc == want, (kw, msg)


def test_symbol_and_header(tmp_path):
    assert "pilot_ot_nb_design_cooks" in _lib.SYMBOLS and hasattr(_lib.load(), "pilot_ot_nb_design_cooks")
    assert not [n for n in engine.ws_slot_names() if n.startswith("WS_NB_")
                and n not in ("WS_NB_Y", "WS_NB_INT", "WS_NB_SF", "WS_NB_BAD", "WS_NB_PRIOR", "WS_NB_OUT", "WS_NB_FIT_INT")]
    src = tmp_path / "t.c"
    src.write_text('#include "pilot_ot.h"\nint main(void){return pilot_ot_nb_design_cooks(0, 0, 1, 6, 1, 1, 0, 3, 0, 4, 0, 0, 0, 3.0, 7, 0, 0, 0, 0, '
                   '0, 0, 0, 0, 1, 0, 0, 1, 0, 0) == PILOT_OT_OK;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


# ---- engine refuses on the host -----------------------------------------------------------------------------------------------------------
Y6, S6, XA = np.ones((6, 5)), np.array([1.0, 0.5, 2.0, 1.0, 1.5, 0.7]), np.array(X6)
ENGINE_GOOD = dict(counts=Y6, design=XA, size_factors=S6, dispersion=np.full(5, 0.1), beta=np.zeros((5, 3)), cutoff=3.0)


@pytest.mark.parametrize("kw", [
    dict(counts=np.ones(6)), dict(counts=np.ones((6, 5), dtype=np.int64)), dict(design=XA[:5]), dict(design=XA[:, :1]),
    dict(design=np.hstack([XA] * 3)), dict(design=XA[:, ::-1]), dict(design=np.stack([XA[:, 0], XA[:, 1], 1.0 - XA[:, 1]], axis=1)),
    dict(size_factors=S6[:5]), dict(size_factors=-S6), dict(dispersion=np.full(4, 0.1)), dict(dispersion=[0.1, 0.1, 9e-9, 0.1, 0.1]),
    dict(dispersion=[10.5, 0.1, 0.1, 0.1, 0.1]), dict(beta=np.zeros((5, 2))), dict(beta=np.zeros(5)), dict(beta=np.zeros((4, 3))),
    dict(beta=np.full((5, 3), np.nan)), dict(beta=np.full((5, 3), np.inf)),
    dict(cutoff=0.0), dict(cutoff=-2.0), dict(cutoff=np.nan), dict(cutoff=np.inf), dict(cutoff="3"), dict(cutoff=None), dict(cutoff=True),
    dict(min_replace=2), dict(min_replace=0), dict(min_replace=7.5), dict(min_replace=True),
    dict(return_distances="host"), dict(return_distances=2),
])
def test_engine_refuses_before_the_library(no_library, kw):
    with pytest.raises(ValueError):
        engine.nb_design_cooks(**dict(ENGINE_GOOD, **kw))


def test_good_engine_arguments_reach_the_library(no_library):
    nan_row = np.zeros((5, 3))
    nan_row[1] = np.nan
    for kw in (dict(), dict(min_replace=3), dict(return_distances=True), dict(dispersion=[0.1, np.nan, 1e-8, 6.0, 0.1], beta=nan_row)):
        with pytest.raises(AssertionError, match="the library was touched"):
            engine.nb_design_cooks(**dict(ENGINE_GOOD, **kw))


# ---- tl on the restatement -------------------------------------------------------------------------------------------------------------------
ARGS = dict(group1="T1", group2="T2", cluster_col="Predicted_Labels")


@functools.lru_cache(maxsize=None)
def planted_table_with_batch(n0, n1, G=90):
    """test_nb_cooks_args.planted_table with a batch column that halves each group in turn (the samples of a group alternate between
    A and B), so that the design ~ batch + stage has four cells of about n0 / 2 and n1 / 2 samples"""
    counts, meta, planted = planted_table(n0, n1, G=G)
    meta = meta.copy()
    batch = np.empty(len(meta), dtype=object)
    for label in ("T1", "T2"):
        at = np.flatnonzero((meta["Predicted_Labels"] == label).to_numpy())
        batch[at] = np.array(["A", "B"])[np.arange(at.size) % 2]
    meta["batch"] = batch
    return counts, meta, planted


def _fake_cooks(monkeypatch):
    """the device call of tl.outliers_design replaced by the restatement"""
    def cooks(counts, design, size_factors, dispersion, beta, cutoff, min_replace=7, return_distances=False):
        out = KR.cooks(np.asarray(counts), design, size_factors, dispersion, beta, cutoff, min_replace)
        for name in ("D_scale", "kappa", "ridge_trace") + (() if return_distances else ("D", "H")):
            out.pop(name)
        return out

    monkeypatch.setattr(engine, "nb_design_cooks", cooks)


def outliers_design_by_hand(counts, plain, independent_filtering=False, alpha=0.05, min_replace=7):
    """tl.outliers_design from the engine calls and the host tail written out (DESIGN.md K28 over K25's steps 1-6); counts: the
    selected samples' table; plain: the frame compute_pseudobulk_DE(covariates=...) returned.  Returns (frame, replaced rows)"""
    c = np.ascontiguousarray(counts.to_numpy(dtype=np.float64))
    m, G = c.shape
    sf = plain.attrs["size_factors"].to_numpy()
    X = plain.attrs["design"].to_numpy()
    p = X.shape[1]
    table = plain.attrs["dispersions"]
    beta = plain.attrs["coefficients"].loc[counts.columns].to_numpy().copy()
    at = pd.Index(plain["gene"]).get_indexer(counts.columns)
    col = {name: plain[name].to_numpy()[at].copy() for name in ("baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "dispersion")}
    disp = table["dispersion"].to_numpy().copy()
    cut = float(stats.f.ppf(0.99, p, m - p))
    cells = KR.cells(X)[0]
    first = engine.nb_design_cooks(c, X, sf, disp, beta, cut, min_replace)
    max_cooks, n_above = first["max_cooks"].copy(), first["n_above"].copy()
    rep = np.flatnonzero(first["n_replace"] > 0)
    rows = []
    if rep.size:
        sub = np.ascontiguousarray(c[:, rep])
        second = engine.nb_design_cooks(sub, X, sf, disp[rep], beta[rep], cut, min_replace, return_distances=True)
        rows = KR.replacements(sub, cells, sf, second["D"], cut, second["trimmed_base"], min_replace)
        new = sub.copy()
        for j, i, _, value in rows:
            new[i, j] = value
        x = engine.nb_design_dispersions(new, X, sf)
        nbase = np.where(np.isnan(x), np.nan, (new / sf[:, None]).mean(axis=0))
        a0, a1 = table.attrs["trend"]["coefficients"]
        with np.errstate(divide="ignore", invalid="ignore"):
            log_fit = np.log(a0 + a1 / nbase)
        x_map = engine.nb_design_dispersions(new, X, sf, log_prior_mean=log_fit, prior_var=table.attrs["prior_var"])
        clip = lambda d: np.clip(d, RR.MIN_DISP, RR.max_disp(m))
        ndisp = np.where(RR.outliers(x, log_fit, table.attrs["var_log_disp"]), clip(np.exp(x)), clip(np.exp(x_map)))
        nbeta, cov, loglik = engine.nb_design_fits(new, X, sf, ndisp)
        a = np.zeros(p)
        a[-1] = 1.0
        lfc, se, stat, pv = DR.wald(nbeta, cov, a)
        if plain.attrs["test"] == "lrt":
            stat, pv = DR.lrt(loglik, engine.nb_design_fits(new, np.ascontiguousarray(X[:, :-1]), sf, ndisp)[2])
        beta[rep] = nbeta
        for name, v in (("baseMean", nbase), ("log2FoldChange", lfc), ("lfcSE", se), ("stat", stat), ("pvalue", pv), ("dispersion", ndisp)):
            col[name][rep] = v
        live = ~np.isnan(ndisp)
        max_cooks[rep], n_above[rep] = np.nan, 0
        if live.any():
            third = engine.nb_design_cooks(np.ascontiguousarray(new[:, live]), X, sf, ndisp[live], nbeta[live], cut, min_replace,
                                           return_distances=True)
            max_cooks[rep[live]], n_above[rep[live]] = KR.refit_max_cooks(new[:, live], cells, third["D"], min_replace)
        rows = [(counts.columns[rep[j]], counts.index[i], was, value) for j, i, was, value in rows]
    with np.errstate(invalid="ignore"):
        flagged = (max_cooks > cut) & (n_above < 3)
    pv = col["pvalue"]
    pv[flagged] = np.nan
    if independent_filtering:
        padj = CR.independent_filtering(pv, col["baseMean"], alpha, fit_lowess=engine.lowess)[0]
    else:
        padj = np.full(G, np.nan)
        padj[~np.isnan(pv)] = CR.bh(pv[~np.isnan(pv)])
    replace = np.zeros(G, dtype=bool)
    replace[rep] = True
    frame = pd.DataFrame({"gene": np.asarray(counts.columns), "baseMean": col["baseMean"], "log2FoldChange": col["log2FoldChange"],
                          "lfcSE": col["lfcSE"], "stat": col["stat"], "pvalue": pv, "padj": padj, "dispersion": col["dispersion"],
                          "maxCooks": max_cooks, "cooksOutlier": flagged, "replace": replace})
    return frame.iloc[np.argsort(padj, kind="stable")].reset_index(drop=True), rows, beta


def hold_outliers_frame(out, plain, sub, planted, replaceable, **kw):
    """what every tl.outliers_design frame must satisfy, against the host tail recomputed from the same engine calls"""
    want, rows, beta = outliers_design_by_hand(sub, plain, **kw)
    assert list(out.columns) == list(plain.columns) + ["maxCooks", "cooksOutlier", "replace"]
    pd.testing.assert_frame_equal(out, want, check_exact=True)
    m, p = plain.attrs["design"].shape
    assert out.attrs["cooks_cutoff"] == KR.cutoff(m, p) and out.attrs["test"] == plain.attrs["test"]
    replaced = out.attrs["replaced"]
    assert list(replaced.columns) == ["gene", "sample", "count", "replacement"]
    assert [tuple(r) for r in replaced.itertuples(index=False)] == rows
    np.testing.assert_array_equal(out.attrs["coefficients"].to_numpy(), beta)
    at, was = out.set_index("gene"), plain.set_index("gene")
    np.testing.assert_array_equal(out.attrs["dispersions"].loc[at.index, "dispersion"].to_numpy(), at["dispersion"].to_numpy())
    assert "maxCooks" not in plain.columns and "replaced" not in plain.attrs      # the input is left as it was
    same = ~(at["replace"] | at["cooksOutlier"]).to_numpy()
    for name in ("baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "dispersion"):
        np.testing.assert_array_equal(at[name].to_numpy()[same], was.loc[at.index, name].to_numpy()[same])
    if replaceable:
        for g, samples in planted.items():
            assert at.loc[g, "replace"] and not at.loc[g, "cooksOutlier"]
            assert replaced.loc[replaced["gene"] == g, "sample"].tolist() == samples
        for g in ("g003", "g017"):
            assert abs(at.loc[g, "log2FoldChange"]) < abs(was.loc[g, "log2FoldChange"]) or abs(at.loc[g, "stat"]) < abs(was.loc[g, "stat"])
        assert at.loc["g025", ["baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "padj", "dispersion"]].isna().all()
        assert (replaced["replacement"] == np.trunc(replaced["replacement"])).all()
    else:
        for g in planted:
            assert at.loc[g, "cooksOutlier"] and np.isnan(at.loc[g, "pvalue"]) and np.isnan(at.loc[g, "padj"]) and not at.loc[g, "replace"]
        assert len(replaced) == 0 and not at["replace"].any()
    return want


@pytest.mark.parametrize("test,n", [("wald", 7), ("lrt", 14)], ids=["wald-flaggable", "lrt-replaceable"])
def test_tl_outliers_design_on_the_restatement(monkeypatch, test, n):
    _fakes(monkeypatch)
    _fake_cooks(monkeypatch)
    counts, meta, planted = planted_table_with_batch(n, n, G=32)
    planted = {g: v for g, v in planted.items() if g in counts.columns}
    plain = tl.compute_pseudobulk_DE(counts, meta, covariates=["batch"], test=test, **ARGS)
    sub = counts.loc[plain.attrs["design"].index]
    out = tl.outliers_design(sub, plain)
    hold_outliers_frame(out, plain, sub, planted, replaceable=n >= 14)
    assert "independent_filtering" not in out.attrs
    both = tl.outliers_design(sub, plain, independent_filtering=True, alpha=0.1)
    pd.testing.assert_frame_equal(both, outliers_design_by_hand(sub, plain, True, 0.1)[0], check_exact=True)
    assert "independent_filtering" in both.attrs
    table = tl.deseq2_cooks_design(sub, out)
    assert list(table.columns) == ["alpha_robust", "max_cooks", "arg_max", "n_above", "n_replace", "trimmed_base"]
    assert list(table.index) == list(sub.columns) and table.attrs["cooks_cutoff"] == out.attrs["cooks_cutoff"]
    np.testing.assert_array_equal(table.attrs["cells"].to_numpy(), KR.cells(plain.attrs["design"].to_numpy())[0])
    if n < 14:
        np.testing.assert_array_equal(table["max_cooks"].to_numpy(), out.set_index("gene").loc[sub.columns, "maxCooks"].to_numpy())


def test_a_clean_table_keeps_every_old_column(monkeypatch):
    _fakes(monkeypatch)
    _fake_cooks(monkeypatch)
    counts, meta, _ = planted_table_with_batch(7, 7, G=32)
    clean = counts.drop(columns=["g003", "g017", "g020", "g025", "g030"])
    plain = tl.compute_pseudobulk_DE(clean, meta, covariates=["batch"], **ARGS)
    out = tl.outliers_design(clean, plain)
    assert not out["replace"].any() and not out["cooksOutlier"].any() and len(out.attrs["replaced"]) == 0
    pd.testing.assert_frame_equal(out[list(plain.columns)], plain, check_exact=True)
    pd.testing.assert_frame_equal(out.attrs["dispersions"], plain.attrs["dispersions"], check_exact=True)
    pd.testing.assert_frame_equal(out.attrs["coefficients"], plain.attrs["coefficients"], check_exact=True)
    assert out.attrs["n_not_converged"] == plain.attrs["n_not_converged"]


def test_a_numeric_covariate_computes_but_neither_replaces_nor_flags(monkeypatch):
    _fakes(monkeypatch)
    _fake_cooks(monkeypatch)
    counts, meta, _ = planted_table_with_batch(7, 7, G=32)
    meta = meta.assign(age=np.random.default_rng(2).normal(50.0, 10.0, len(meta)))
    plain = tl.compute_pseudobulk_DE(counts, meta, covariates=["age"], **ARGS)
    out = tl.outliers_design(counts, plain)
    assert out["maxCooks"].isna().all() and not out["replace"].any() and not out["cooksOutlier"].any()
    pd.testing.assert_frame_equal(out[list(plain.columns)], plain, check_exact=True)


def test_tl_refuses_before_the_library(monkeypatch):
    _fakes(monkeypatch)
    _fake_cooks(monkeypatch)
    counts, meta, _ = planted_table_with_batch(7, 7, G=32)
    plain = tl.compute_pseudobulk_DE(counts, meta, covariates=["batch"], **ARGS)
    handled = tl.outliers_design(counts, plain)
    shrunk = plain.copy()
    shrunk["lfcMLE"], shrunk["lfcMLESE"] = plain["log2FoldChange"], plain["lfcSE"]
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())
    monkeypatch.setattr(engine, "nb_design_cooks", lambda *a, **k: _Untouchable().nb_design_cooks)
    k22 = plain.copy()
    del k22.attrs["design"]
    for fn in (tl.outliers_design, tl.deseq2_cooks_design):
        who = fn.__name__
        with pytest.raises(ValueError, match=r"compute_pseudobulk_DE\(outliers=" if fn is tl.outliers_design else "deseq2_cooks") as err:
            fn(counts, k22)
        assert str(err.value).startswith(who + ": ")
        with pytest.raises(ValueError, match="genes"):
            fn(counts.iloc[:, :-1], plain)
        with pytest.raises(ValueError, match="genes"):
            fn(counts.rename(columns={"g003": "other"}), plain)
        with pytest.raises(ValueError, match="samples"):
            fn(counts.iloc[:-1], plain)
        with pytest.raises(ValueError, match="samples"):
            fn(counts.iloc[::-1], plain)
        with pytest.raises(ValueError, match="frame of compute_pseudobulk_DE"):
            fn(counts, plain.drop(columns=["dispersion"]))
        with pytest.raises(ValueError, match="frame of compute_pseudobulk_DE"):
            fn(counts, None)
        for bad in (2, 0, 7.5, True):
            with pytest.raises(ValueError, match="min_replace"):
                fn(counts, plain, min_replace=bad)
    with pytest.raises(ValueError, match="maxCooks"):
        tl.outliers_design(counts, handled)
    with pytest.raises(ValueError, match="shrink afterwards"):
        tl.outliers_design(counts, shrunk)
    for kw in (dict(alpha=0.0), dict(alpha=1.0), dict(alpha="0.05"), dict(independent_filtering="yes"), dict(independent_filtering=1)):
        with pytest.raises(ValueError):
            tl.outliers_design(counts, plain, **kw)
    bare = plain.copy()
    del bare.attrs["dispersions"]
    with pytest.raises(ValueError, match="dispersions"):
        tl.outliers_design(counts, bare)


def test_the_refusals_of_the_de_calls_stand_and_point_here(no_library):
    counts, meta, _ = planted_table_with_batch(7, 7, G=32)
    with pytest.raises(NotImplementedError, match="K25.*outliers_design"):
        tl.compute_pseudobulk_DE(counts, meta, covariates=["batch"], outliers="deseq2", **ARGS)
    with pytest.raises(NotImplementedError, match="K25.*outliers_design"):
        tl.get_pseudobulk_DE(None, None, "alpha", covariates=["batch"], outliers="deseq2")


def test_lfc_shrink_design_fits_the_replaced_counts(monkeypatch):
    """the engine stubbed: what reaches nb_design_shrink is the table with attrs['replaced'] written in, and a record that does not
    match the table is refused"""
    _fakes(monkeypatch)
    counts, meta, _ = planted_table_with_batch(7, 7, G=32)
    plain = tl.compute_pseudobulk_DE(counts, meta, covariates=["batch"], **ARGS)
    seen = {}

    def shrink(c, design, size_factors, dispersion, beta_mle, far_end, prior_scale, coef=-1, other_scale=15.0, return_info=False):
        seen["c"] = np.array(c)
        p = design.shape[1]
        info = {"information": np.tile(np.eye(p), (c.shape[1], 1, 1)), "n_at_bound": 0}
        return np.zeros((c.shape[1], p)), info

    monkeypatch.setattr(engine, "nb_design_shrink", shrink)
    tl.lfc_shrink_design(counts, plain, prior_scale=0.5)
    np.testing.assert_array_equal(seen["c"], counts.to_numpy())
    sample, gene = counts.index[4], "g007"
    record = pd.DataFrame({"gene": [gene], "sample": [sample], "count": [counts.loc[sample, gene]], "replacement": [3.0]})
    marked = plain.copy()
    marked.attrs["replaced"] = record
    tl.lfc_shrink_design(counts, marked, prior_scale=0.5)
    want = np.rint(counts.to_numpy(dtype=np.float64))
    want[4, list(counts.columns).index(gene)] = 3.0
    np.testing.assert_array_equal(seen["c"], want)
    marked.attrs["replaced"] = record.assign(count=record["count"] + 1.0)
    with pytest.raises(ValueError, match="lfc_shrink_design: .*records other counts"):
        tl.lfc_shrink_design(counts, marked, prior_scale=0.5)
    marked.attrs["replaced"] = record.assign(sample="nobody")
    with pytest.raises(ValueError, match="names a gene or a sample"):
        tl.lfc_shrink_design(counts, marked, prior_scale=0.5)
