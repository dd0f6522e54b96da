"""K29 without a device: the restatement (tests/permanova_restatement.py) pinned to published and classical answers, the host side
of engine.permanova_* (every refusal comes before device work), and the reference's four clinical-variable tests held to a
fixture made by the reference's own code (tests/golden/gen_clinical_golden.py)."""
import json
import os
import types

import numpy as np
import pandas as pd
import pytest
from scipy import stats

import permanova_restatement as R
from conftest import GOLDEN
from pilot_amd import _lib, engine, tl


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = R.philox4x32_10(counter, key)
    assert " ".join("%08x" % int(w) for w in got) == want


def test_key_is_the_first_two_words():
    k = R.row_keys(3, 2 ** 32 + 7, 2 ** 63 + 5)
    w = R.philox4x32_10((2, 7, 1, 0), (5, 2 ** 31))
    assert int(k[2]) == (int(w[0]) << 32) + int(w[1])


def _line_cohort(seed, n=31):
    rs = np.random.RandomState(seed)
    y = rs.randn(n) + np.repeat([0.0, 0.7, -0.4], [11, 9, 11])[:n]
    group = np.repeat(["a", "b", "c"], [11, 9, 11])[:n].astype(object)
    x = 0.5 * y + rs.randn(n)
    return y, group, x, np.abs(y[:, None] - y[None, :])


def _observed(D, X):
    Q, terms = engine.permanova_basis(X)
    A = R.a_matrix(D)
    total = R.ss_total(A)[0]
    ss = R.ss_terms(A, Q, terms, [np.arange(len(Q))])[0]
    return total, ss, terms, R.f_stat(total, ss, terms, len(Q))


def test_residual_is_the_classical_within_group_sum():
    y, group, x, D = _line_cohort(1)
    rs = np.random.RandomState(2)
    D = D + 0.05 * rs.rand(*D.shape)                      # not symmetric, a non-zero diagonal: the rule symmetrises
    total, ss, _, _ = _observed(D, {"group": group})
    S = (D + D.T) / 2
    within = sum((S[np.ix_(m, m)][np.triu_indices(m.sum(), 1)] ** 2).sum() / m.sum() for m in (group == g for g in "abc"))
    assert abs(float(total - ss[0, 0]) - within) <= 1e-12 * within
    n = len(y)
    assert abs(float(total) - (S[np.triu_indices(n, 1)] ** 2).sum() / n) <= 1e-12 * float(total)


def test_pseudo_f_is_anova_f_on_a_line():
    y, group, x, D = _line_cohort(3)
    F = _observed(D, {"group": group})[3]
    want = stats.f_oneway(*[y[group == g] for g in "abc"]).statistic
    assert abs(float(F[0, 0]) - want) <= 1e-10 * want


def test_pseudo_f_is_the_regression_f_on_a_line():
    y, group, x, D = _line_cohort(4)
    F = _observed(D, {"x": x})[3]
    r = stats.pearsonr(x, y)[0]
    want = r * r * (len(y) - 2) / (1 - r * r)
    assert abs(float(F[0, 0]) - want) <= 1e-10 * want


@pytest.mark.parametrize("n", [1, 2, 5, 64, 65])
def test_rows_are_permutations_within_strata(n):
    rs = np.random.RandomState(n)
    for strata in (None, np.zeros(n, int), np.arange(n), rs.randint(0, 3, n), np.array(["x", "y"], dtype=object)[rs.randint(0, 2, n)]):
        P = R.permutations(n, 12, 2 ** 63 + 5, strata)
        assert P.shape == (13, n) and P[0].tolist() == list(range(n))
        assert all(sorted(p.tolist()) == list(range(n)) for p in P)
        if strata is not None:
            assert all((np.asarray(strata)[p] == np.asarray(strata)).all() for p in P)
        assert R.permutations(n, 12, 2 ** 63 + 5, strata, start=9).tolist() == P[9:].tolist()
    if n >= 5:
        assert len({tuple(p) for p in R.permutations(n, 12, 0).tolist()}) > 6
        assert R.permutations(n, 3, 0).tolist() != R.permutations(n, 3, 1).tolist()


def test_p_value_rule():
    F = np.array([[2.0, 1.0], [2.0 - 1e-9, 0.5], [3.0, 0.999], [1.0, 1.0 + 1e-12]])
    assert R.p_values(F).tolist() == [0.75, 0.5]
    assert engine.permanova_p(F).tolist() == [0.75, 0.5]
    assert engine.PERMANOVA_EPS == R.EPS == 2.0 ** -26


# ---- the host side of the engine ----------------------------------------------------------------------------------------------------
def test_abi_and_limits():
    for name in ("pilot_ot_permanova", "pilot_ot_permanova_permutations", "pilot_ot_permanova_limits"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)
    max_n, chunk, tile_cols, row_block = engine.permanova_limits()
    assert max_n == 8192 and chunk >= 1 and tile_cols % 16 == 0 and row_block % 16 == 0
    _lib.test_switch("PILOT_OT_PERMANOVA_CHUNK", 3)
    try:
        assert engine.permanova_limits()[1] == 3
    finally:
        _lib.test_switch("PILOT_OT_PERMANOVA_CHUNK", None)
    assert engine.permanova_limits()[1] == chunk


def test_basis():
    rs = np.random.RandomState(0)
    n = 20
    g = np.array(["b", "a", "c", "a"], dtype=object)[rs.randint(0, 4, n)]
    x = rs.randn(n)
    Q, terms = engine.permanova_basis({"g": g, "x": x, "flag": x > 0})
    assert terms.tolist() == [0, 2, 3, 4] and terms.dtype == np.int32 and Q.shape == (n, 4) and Q.dtype == np.float64
    assert np.abs(Q.sum(axis=0)).max() < 1e-12
    assert np.abs(Q[:, :2].T @ Q[:, :2] - np.eye(2)).max() < 1e-12
    # the span: the indicators of all levels but the first in string order ("a"), centred
    M = np.stack([(g == "b") * 1.0, (g == "c") * 1.0], axis=1)
    M -= M.mean(axis=0)
    assert np.abs(Q[:, :2] @ (Q[:, :2].T @ M) - M).max() < 1e-12
    assert np.abs(np.abs(Q[:, 2]) - np.abs(x - x.mean()) / np.linalg.norm(x - x.mean())).max() < 1e-12
    # a frame and a list are taken too
    assert engine.permanova_basis(pd.DataFrame({"g": g, "x": x}))[1].tolist() == [0, 2, 3]
    assert engine.permanova_basis([x])[1].tolist() == [0, 1]
    for bad, word in (({"one": np.array(["a"] * n, dtype=object)}, "'one'"), ({"const": np.full(n, 3.7)}, "'const'"),
                      ({"ok": x, "same": np.full(n, 1e9) + 0.0}, "'same'")):
        with pytest.raises(ValueError, match="rank 0") as err:
            engine.permanova_basis(bad)
        assert word in str(err.value)
    with pytest.raises(ValueError, match="missing"):
        engine.permanova_basis({"x": np.where(np.arange(n) == 3, np.nan, x)})
    with pytest.raises(ValueError, match="missing"):
        engine.permanova_basis({"g": np.where(np.arange(n) == 3, None, g)})
    with pytest.raises(ValueError, match="one value per sample"):
        engine.permanova_basis({"x": x, "y": x[:-1]})


def _valid(n=12, N=None):
    rs = np.random.RandomState(n)
    N = n if N is None else N
    D = rs.rand(N, N)
    Q, terms = engine.permanova_basis({"x": rs.randn(n), "g": np.array(["a", "b", "c"], dtype=object)[np.arange(n) % 3]})
    return D, Q, terms


def test_refusals_come_before_device_work():
    """every one a ValueError: a call that reached the device would fail otherwise where there is none"""
    D, Q, terms = _valid()
    bad_calls = [
        (lambda: engine.permanova_ss(D[:, :5], Q, terms, 9), "samples x samples"),
        (lambda: engine.permanova_ss(D[0], Q, terms, 9), "2-D"),
        (lambda: engine.permanova_ss(D, Q[:5], terms, 9), "n x c float64"),
        (lambda: engine.permanova_ss(D, Q.astype(np.float32), terms, 9), "n x c float64"),
        (lambda: engine.permanova_ss(D, Q[:, 0], terms, 9), "n x c float64"),
        (lambda: engine.permanova_ss(D, Q, [0, 1], 9), "terms"),
        (lambda: engine.permanova_ss(D, Q, [0, 2, 2, 3], 9), "terms"),
        (lambda: engine.permanova_ss(D, Q, [1, 3], 9), "terms"),
        (lambda: engine.permanova_ss(D, Q + 0.25, terms, 9), "not centred"),
        (lambda: engine.permanova_ss(D, np.where(Q == Q[0, 0], np.nan, Q), terms, 9), "NaN"),
        (lambda: engine.permanova_ss(D, Q, terms, 9, seed=-1), "seed"),
        (lambda: engine.permanova_ss(D, Q, terms, 9, seed=2 ** 64), "seed"),
        (lambda: engine.permanova_ss(D, Q, terms, 9, start=10), "start"),
        (lambda: engine.permanova_ss(D, Q, terms, 9, start=-1), "start"),
        (lambda: engine.permanova_ss(D, Q, terms, -1), "n_perm"),
        (lambda: engine.permanova_ss(D, Q, terms, 9, strata=np.zeros(5)), "one label per sample"),
        (lambda: engine.permanova_ss(D, Q, terms, 9, rows=np.arange(12)[::-1]), "ascending"),
        (lambda: engine.permanova_ss(D, Q, terms, 9, rows=np.arange(1, 13)), "ascending"),
        (lambda: engine.permanova_ss(D, Q, terms, 9, rows=np.arange(12) * 1.0), "integer"),
        (lambda: engine.permanova_ss(D, Q, terms, 9, rows=np.arange(5)), "n x c float64"),
        (lambda: engine.permanova_permutations(0, 9), "n=0"),
        (lambda: engine.permanova_permutations(8193, 9), "at most 8192"),
        (lambda: engine.permanova_permutations(5, 9, seed=-3), "seed"),
        (lambda: engine.permanova_permutations(5, 9, start=10), "start"),
        (lambda: engine.permanova_permutations(5, 9, strata=[0, 1]), "one label per sample"),
    ]
    for call, word in bad_calls:
        with pytest.raises(ValueError, match=word):
            call()
    big = np.broadcast_to(np.zeros(1), (8193, 8193))            # no memory behind it: refused by its shape alone
    with pytest.raises(ValueError, match="at most 8192"):
        engine.permanova_ss(big, np.zeros((8193, 1)), [0, 1], 9)


def test_c_abi_refuses_before_any_hip_call():
    L = _lib.load()
    D, Q, terms = _valid()
    out, tot = np.zeros((10, 2)), np.zeros(1)
    ip, dp = _lib.iptr, _lib.dptr

    def call(D=D, dtype=1, N=12, ld=12, rows=None, n=12, Q=Q, c=3, terms=terms, n_terms=2, strata=None, start=0, count=10):
        return L.pilot_ot_permanova(D.ctypes.data, 0, dtype, N, ld, None if rows is None else ip(rows), n, dp(Q), c, ip(terms), n_terms,
                                    None if strata is None else ip(strata), 0, start, count, dp(tot), dp(out), None, None, None)
    i32 = lambda *v: np.array(v, dtype=np.int32)
    assert call(dtype=2) == _lib.EINVAL and call(ld=11) == _lib.EINVAL and call(N=0) == _lib.EINVAL and call(n=11) == _lib.EINVAL
    assert call(rows=i32(*range(11), 12)) == _lib.EINVAL and call(rows=i32(1, 0, *range(2, 12))) == _lib.EINVAL
    assert call(c=0) == _lib.EINVAL and call(n_terms=4) == _lib.EINVAL and call(terms=i32(0, 0, 3)) == _lib.EINVAL
    assert call(terms=i32(0, 1, 2)) == _lib.EINVAL and call(start=-1) == _lib.EINVAL and call(count=-1) == _lib.EINVAL
    assert call(strata=i32(*([0] * 11), -1)) == _lib.EINVAL
    assert call(Q=np.ascontiguousarray(Q + 1.0)) == _lib.EINVAL and b"not centred" in L.pilot_ot_last_error()
    perm = np.zeros((2, 9000), dtype=np.int32)
    assert L.pilot_ot_permanova_permutations(9000, None, 0, 0, 2, ip(perm)) == _lib.ENOTSUP
    assert L.pilot_ot_permanova_permutations(0, None, 0, 0, 2, ip(perm)) == _lib.EINVAL
    assert L.pilot_ot_permanova_permutations(5, None, 0, 0, 2, None) == _lib.EINVAL


# ---- tl: the reference's four tests, held to the reference's own frames -------------------------------------------------------------
def _frame(columns):
    return pd.DataFrame({k: [np.nan if v is None else v for v in col] for k, col in columns.items()})


@pytest.fixture(scope="module")
def clinical():
    with open(os.path.join(GOLDEN, "clinical_tests.json")) as f:
        g = json.load(f)
    obs = _frame(g["obs"])
    assert obs["grade"].dtype == object and obs["age"].dtype == np.float64
    adata = types.SimpleNamespace(obs=obs, uns={"orders": _frame(g["orders"])})
    return g, adata, _frame(g["proportion_df"])


@pytest.mark.parametrize("name", ["correlation_categorical_with_trajectory", "correlation_numeric_with_trajectory",
                                  "correlation_categorical_with_clustering", "correlation_numeric_with_clustering"])
def test_reference_frames(clinical, name):
    g, adata, proportion_df = clinical
    want = g["results"][name]
    args = (adata,) if name.endswith("trajectory") else (adata, proportion_df)
    got = getattr(tl, name)(*args, sample_col="sampleID", features=list(want["features"]))
    frame = want["frame"]
    assert list(got.columns) == frame["columns"] and [int(i) for i in got.index] == frame["index"]
    assert 0 < len(got) < len(want["features"])              # the fixture holds a feature that fails the 0.05 filter
    for c in frame["columns"]:
        assert got[c].tolist() == frame["data"][c], c         # the same scipy calls on the same numbers: exactly


def test_fixture_covers_the_cleaning(clinical):
    g, adata, _ = clinical
    grade = adata.obs.drop_duplicates("sampleID")["grade"]
    assert grade.isna().sum() == 1 and {"1", "2", "3", "low", "high"} <= set(grade.dropna())
    assert adata.obs.drop_duplicates("sampleID")["egfr"].isna().sum() == 1
    sex = adata.obs.groupby("sampleID")["sex"].nunique()
    assert (sex == 2).all()                                    # only a sample's first row may count
    kinds = {name: tl._permanova_variable(list(adata.obs.drop_duplicates("sampleID")[name]))[0] for name in ("grade", "egfr", "sex", "age")}
    assert kinds == {"grade": "categorical", "egfr": "numeric", "sex": "categorical", "age": "numeric"}


def test_permanova_variable():
    kind, used, x = tl._permanova_variable([1, "2.5", None, np.nan, 4.0])
    assert kind == "numeric" and used.tolist() == [True, True, False, False, True] and x.tolist() == [1.0, 2.5, 4.0]
    kind, used, x = tl._permanova_variable(["low", "3", 3.0, np.nan, "high", None])
    assert kind == "categorical" and used.tolist() == [True, True, False, False, True, False] and x.tolist() == ["low", "3", "high"]


def test_permanova_refusals():
    obs = pd.DataFrame({"sampleID": ["a", "b", "c", "d"], "x": [1.0, 2.0, 3.0, 5.0], "one": ["u"] * 4, "s": ["p", "p", "q", None]})
    uns = {"EMD": np.zeros((4, 4)), "proportions": {k: None for k in "abcd"}}
    adata = types.SimpleNamespace(obs=obs, uns=uns)
    for kwargs, word in ((dict(features=["nope"]), "no column"), (dict(features=[]), "no feature"), (dict(features=["one"]), "rank 0"),
                         (dict(features=["x"], strata="nope"), "no column"), (dict(features=["x"], strata="s"), "missing"),
                         (dict(features=["x"], D=np.zeros((3, 3))), "4 samples"), (dict(features=["x"], permutations=0), "permutations")):
        with pytest.raises(ValueError, match=word):
            tl.permanova(adata, **kwargs)
    with pytest.raises(ValueError, match="EMD"):
        tl.permanova(types.SimpleNamespace(obs=obs, uns={"proportions": uns["proportions"]}), ["x"])
    three = types.SimpleNamespace(obs=obs.iloc[:3], uns={"EMD": np.zeros((3, 3)), "proportions": {k: None for k in "abc"}})
    obs3 = three.obs.assign(g=["u", "v", "w"])
    with pytest.raises(ValueError, match="too few"):
        tl.permanova(types.SimpleNamespace(obs=obs3, uns=three.uns), ["g"])
