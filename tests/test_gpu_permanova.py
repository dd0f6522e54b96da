"""K29 on the device against tests/permanova_restatement.py: the permutations bit for bit, the sums of squares within the
dot-product bound applied twice, permutation b's bits whatever the batch, tl.permanova's p-values exactly, the workspace guard.

Measured on an MI355X (2026-10-21; the tests print the figures): a sum of squares uses at most 0.143 of the bound
4 n 2^-53 sum |z_i||A_ij||z_j| (at n = 3; at most 0.015 from n = 15 on, 7.4e-5 at n = 257) and SS_total at most 0.101 of the same form
of bound -- DESIGN.md K29, "asked / measured"."""
import types

import numpy as np
import pandas as pd
import pytest

import permanova_restatement as R
from pilot_amd import _lib, engine, tl

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


class chunk_of:
    """the permutations per pass lowered by the test switch"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        _lib.test_switch("PILOT_OT_PERMANOVA_CHUNK", self.value)

    def __exit__(self, *exc):
        _lib.test_switch("PILOT_OT_PERMANOVA_CHUNK", None)
        return False


# ---- permutations -------------------------------------------------------------------------------------------------------------------
# 1, 2, 5, 64, 65, 257 and every power of two the LDS sort pads to with the size one past it, up to 1025
PERM_SIZES = sorted({1, 2, 5, 64, 65, 257} | {2 ** k for k in range(11)} | {2 ** k + 1 for k in range(11)})


def _strata_variants(n):
    rs = np.random.RandomState(n)
    uneven = np.sort(rs.randint(0, 4, n)) if n > 1 else np.zeros(n, int)
    rs.shuffle(uneven)
    return [None, np.zeros(n, dtype=int), np.arange(n)[::-1].copy(), uneven]


@pytest.mark.parametrize("n", PERM_SIZES)
def test_permutations_equal_the_restatement(n):
    for seed in (0, 1, 2 ** 63 + 5):
        for strata in _strata_variants(n):
            want = R.permutations(n, 7, seed, strata)
            with chunk_of(3):                                       # 8 permutations: chunks of 3, 3, 2
                got = engine.permanova_permutations(n, 7, seed=seed, strata=strata)
                tail = engine.permanova_permutations(n, 7, seed=seed, strata=strata, start=4)     # 4 permutations: 3, 1
            assert got.dtype == np.int32 and got.tolist() == want.tolist()
            assert tail.tolist() == want[4:].tolist()
            assert engine.permanova_permutations(n, 7, seed=seed, strata=strata, start=2).tolist() == want[2:].tolist()


def test_permutation_index_beyond_32_bits():
    b = 2 ** 32 + 3
    got = engine.permanova_permutations(65, b + 1, seed=9, start=b)
    assert got.tolist() == R.permutations(65, b + 1, 9, start=b).tolist()


# ---- sums of squares ----------------------------------------------------------------------------------------------------------------
def _matrix(N, seed, dtype):
    """Sinkhorn-like: not symmetric, a non-zero diagonal"""
    rs = np.random.RandomState(seed)
    X = rs.randn(N, 3)
    D = np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1)) + 0.05 * rs.rand(N, N) + 0.01
    assert np.abs(D - D.T).max() > 1e-3 and D.diagonal().min() > 0
    return np.ascontiguousarray(D.astype(dtype))


def _design(n, widths, seed):
    """centred columns (nothing else is asked of Q by the sums)"""
    rs = np.random.RandomState(seed)
    Q = rs.randn(n, sum(widths))
    Q -= Q.mean(axis=0, keepdims=True)
    return np.ascontiguousarray(Q), np.concatenate([[0], np.cumsum(widths)]).astype(np.int32)


SHARE = {"ss": 0.0, "total": 0.0}
DESIGNS = [(1,), (1, 2), (5, 1, 10), (4, 6, 2, 5)]                  # 1, 3, 16, 17 columns over 1 to 4 terms


def _hold(D, rows, Q, terms, n_perm, seed, strata=None, device=False):
    n = Q.shape[0]
    A = R.a_matrix(D, rows)
    want_total, total_mag = R.ss_total(A)
    want, mag = R.ss_terms(A, Q, terms, R.permutations(n, n_perm, seed, strata))
    arg = engine.DeviceMatrix.upload(D) if device else D
    total, ss = engine.permanova_ss(arg, Q, terms, n_perm, seed=seed, rows=rows, strata=strata)
    assert ss.shape == want.shape and ss.dtype == np.float64
    err, bound = np.abs(ss.astype(np.longdouble) - want), 4 * n * U * mag
    share = float((err / bound).max())
    total_share = float(abs(np.longdouble(total) - want_total) / (4 * n * U * total_mag)) if total_mag > 0 else 0.0
    SHARE["ss"], SHARE["total"] = max(SHARE["ss"], share), max(SHARE["total"], total_share)
    print("n=%d c=%d: share of the bound %.3g (SS), %.3g (SS_total); largest so far %.3g, %.3g"
          % (n, Q.shape[1], share, total_share, SHARE["ss"], SHARE["total"]))
    assert (err <= bound).all(), (share, np.argwhere(err > bound)[:5])
    assert abs(np.longdouble(total) - want_total) <= 4 * n * U * total_mag
    return total, ss


@pytest.mark.parametrize("n", [3, 15, 16, 17, 67, 257])
def test_sums_hold_to_the_restatement(n):
    n_perm = 30 if n == 257 else 200
    for k, widths in enumerate(DESIGNS):
        dtype, device = (np.float64, np.float32)[k % 2], k >= 2      # f64 host, f32 host, f64 device, f32 device
        Q, terms = _design(n, widths, 10 * n + k)
        _hold(_matrix(n, n + k, dtype), None, Q, terms, n_perm, seed=k, device=device)


def test_sums_of_a_rows_subset_and_strata():
    rs = np.random.RandomState(40)
    rows = np.sort(rs.choice(40, 23, replace=False)).astype(np.int32)
    Q, terms = _design(23, (2, 1), 41)
    strata = rs.randint(0, 3, 23)
    for dtype in (np.float64, np.float32):
        for device in (False, True):
            _hold(_matrix(40, 42, dtype), rows, Q, terms, 200, seed=3, strata=strata, device=device)


def test_a_strided_host_view_and_a_bad_entry():
    big = _matrix(50, 7, np.float64)
    view = big[:40, :40]                                             # leading dimension 50
    Q, terms = _design(40, (3,), 8)
    a = engine.permanova_ss(view, Q, terms, 5)
    b = engine.permanova_ss(np.ascontiguousarray(view), Q, terms, 5)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()
    bad = np.array(view)
    bad[7, 31] = np.nan
    with pytest.raises(ValueError, match=r"D\[(7, 31|31, 7)\]"):
        engine.permanova_ss(bad, Q, terms, 5)
    rows = np.array([r for r in range(40) if r != 31], dtype=np.int32)
    Q39, _ = _design(39, (3,), 8)
    engine.permanova_ss(bad, Q39, terms, 5, rows=rows)              # an unused sample's entries are never judged


# ---- permutation b's bits -----------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_batch():
    n, b = 67, 7
    D = _matrix(n, 1, np.float64)
    Q, terms = _design(n, (1, 2), 2)
    total, full = engine.permanova_ss(D, Q, terms, 10, seed=5)
    alone = engine.permanova_ss(D, Q, terms, b, seed=5, start=b)
    assert alone[1].shape == (1, 2) and alone[0] == total and alone[1][0].tobytes() == full[b].tobytes()
    assert engine.permanova_ss(D, Q, terms, b, seed=5)[1].tobytes() == full[:b + 1].tobytes()
    with chunk_of(3):
        assert engine.permanova_ss(D, Q, terms, 10, seed=5)[1].tobytes() == full.tobytes()
        assert engine.permanova_ss(D, Q, terms, 10, seed=5, start=2)[1].tobytes() == full[2:].tobytes()
    first = engine.permanova_ss(D, np.ascontiguousarray(Q[:, :1]), [0, 1], 10, seed=5)[1]
    assert first[:, 0].tobytes() == full[:, 0].tobytes()            # with or without the other term beside it
    second = engine.permanova_ss(D, np.ascontiguousarray(Q[:, 1:]), [0, 2], 10, seed=5)[1]
    assert second[:, 0].tobytes() == full[:, 1].tobytes()
    wide_Q, wide_terms = _design(n, (4, 6, 2, 5), 3)                  # a term's columns on both sides of a 16-column tile edge
    wide = engine.permanova_ss(D, wide_Q, wide_terms, 10, seed=5)[1]
    third = engine.permanova_ss(D, np.ascontiguousarray(wide_Q[:, 10:12]), [0, 2], 10, seed=5)[1]
    assert third[:, 0].tobytes() == wide[:, 2].tobytes()


# ---- tl.permanova -------------------------------------------------------------------------------------------------------------------
PERMUTATIONS, SEED = 999, 11


def _cohort():
    """40 samples x 4 features: a planted 3-level effect, a null one, a numeric one, one with missing values"""
    rs = np.random.RandomState(2026)
    n = 40
    group = np.array(["a", "b", "c"], dtype=object)[np.arange(n) % 3]
    X = rs.randn(n, 3) + 2.5 * np.stack([group == "b", group == "c", np.zeros(n, bool)], axis=1)
    D = np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1)) + 0.02 * rs.rand(n, n) + 0.01
    samples = ["S%02d" % i for i in range(n)]
    null = np.array(["u", "v"], dtype=object)[rs.randint(0, 2, n)]
    score = X[:, 2] + 0.8 * rs.randn(n)
    lab = np.round(X[:, 0] + rs.randn(n), 3).astype(object)
    lab[[4, 17, 33]] = np.nan
    obs = pd.DataFrame({"sampleID": np.repeat(samples, 2), "planted": np.repeat(group, 2), "null": np.repeat(null, 2),
                        "score": np.repeat(score, 2), "lab": np.repeat(lab, 2)})
    obs.loc[1::2, "null"] = "w"                                       # only a sample's first row counts
    adata = types.SimpleNamespace(obs=obs, uns={"EMD": D, "proportions": {s: None for s in samples}})
    return adata, D, {"planted": group, "null": null, "score": score, "lab": lab}


def test_p_values_equal_the_restatement():
    adata, D, values = _cohort()
    features = ["planted", "null", "score", "lab"]
    want = {}
    complete = np.arange(40)
    kept = np.array([i for i in range(40) if i not in (4, 17, 33)])
    for rows, names in ((complete, features[:3]), (kept, features[3:])):
        X = {name: (values[name][rows] if name in ("planted", "null") else values[name][rows].astype(np.float64)) for name in names}
        Q, terms = engine.permanova_basis(X)
        A = R.a_matrix(D, rows)
        total = R.ss_total(A)[0]
        ss = R.ss_terms(A, Q, terms, R.permutations(len(rows), PERMUTATIONS, SEED))[0]
        F = R.f_stat(total, ss, terms, len(rows))
        assert (np.abs(F[1:] - (F[0] - np.longdouble(R.EPS))) > 1e-9).all()       # no permuted F near the threshold: p is decided
        p = R.p_values(F)
        for t, name in enumerate(names):
            want[name] = (len(rows), int(terms[t + 1] - terms[t]), float(ss[0, t]), float(total), float(F[0, t]), float(p[t]))
    got = tl.permanova(adata, features, permutations=PERMUTATIONS, seed=SEED)
    assert list(got.columns) == ["Feature", "kind", "n", "df", "SS_model", "SS_total", "R2", "pseudo_F", "p_value", "p_adj"]
    assert got["Feature"].tolist() == features and got["kind"].tolist() == ["categorical", "categorical", "numeric", "numeric"]
    assert got.attrs == {"permutations": PERMUTATIONS, "seed": SEED, "strata": None}
    for _, row in got.iterrows():
        n, df, ss, total, F, p = want[row["Feature"]]
        assert (row["n"], row["df"]) == (n, df)
        assert row["p_value"] == p, row["Feature"]
        assert abs(row["SS_model"] - ss) <= 1e-12 * total and abs(row["SS_total"] - total) <= 1e-12 * total
        assert abs(row["pseudo_F"] - F) <= 1e-10 * F and abs(row["R2"] - ss / total) <= 1e-12
    assert got["p_value"][0] == 1.0 / 1000 and got["p_value"][1] > 0.05
    assert got["p_adj"].tolist() == engine.bh_adjust(got["p_value"].to_numpy()).tolist()
    on_device = tl.permanova(adata, features, permutations=PERMUTATIONS, seed=SEED, D=engine.DeviceMatrix.upload(D))
    assert on_device.drop(columns="Feature").to_numpy().tolist() == got.drop(columns="Feature").to_numpy().tolist()


# ---- the workspace -------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_scratch():
    """the workspace guard (tests/test_gpu_ws_guard.py) over the new calls: they take the consumers' slots and no new one"""
    D = _matrix(40, 5, np.float32)
    rows = np.arange(3, 36, dtype=np.int32)
    Q, terms = _design(33, (1, 2), 6)
    strata = np.arange(33) % 2

    def run():
        total, ss = engine.permanova_ss(D, Q, terms, 20, seed=1, rows=rows, strata=strata)
        return [np.float64(total), ss, engine.permanova_permutations(33, 20, seed=1, strata=strata)]
    plain = run()
    with chunk_of(3):
        with engine.ws_guard() as guard:
            guarded = run()
    assert guard.damage is None, guard.damage
    assert {"WS_CONS_E", "WS_CONS_D", "WS_CONS_MAX", "WS_CONS_LABELS", "WS_CONS_SIZES", "WS_CONS_SCORES", "WS_CONS_K"} <= guard.seen
    for a, b in zip(plain, guarded):
        assert a.tobytes() == b.tobytes()
    assert engine.ws_guard_report() == (set(), None)
