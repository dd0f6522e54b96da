"""Group sums and the pseudobulk tables (K14), the parts that need no device.  pilot_ot_group_sums and pilot_ot_csr_group_sums refuse
every bad argument before any HIP call (a box without a device returns PILOT_OT_EHIP from the first HIP call, so PILOT_OT_EINVAL
shows the check came first); engine.group_sums and DeviceCSR.group_sums raise ValueError before the library is touched (the
library handle is replaced by an object that fails the test on any use); tl.deseq2_size_factors and the frame logic of
tl.pseudobulk_inputs run on the host.  A sparse handle cannot be made without a device, so the two checks of
pilot_ot_csr_group_sums that read the handle -- a column outside the matrix (and n_cols != the matrix's without cols), a code
reaching n_groups -- are in tests/test_gpu_group_sums.py; every other one is here."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import pseudobulk_restatement as PR
from pilot_amd import _lib, engine, tl

LLP = ctypes.POINTER(ctypes.c_longlong)


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _Untouchable())


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
GOOD = dict(y=True, dtype=0, n=6, total=5, ld=5, codes=[0, 1, 0, 1, -1, 0], ng=2, cols=None, n_cols=5, count=True, sums=True)


def _dense_call(**kw):
    a = dict(GOOD)
    a.update(kw)
    L = _lib.load()
    Y = np.zeros((6, 8), dtype=np.float32)
    codes = None if a["codes"] is None else np.ascontiguousarray(a["codes"], dtype=np.int32)
    cols = None if a["cols"] is None else np.ascontiguousarray(a["cols"], dtype=np.int32)
    groups = max(8, min(a["ng"], 2 ** 20))                         # (room for every group a valid call may write)
    count, sums = np.zeros(groups, dtype=np.int64), np.zeros((groups, 8))
    rc = L.pilot_ot_group_sums(ctypes.c_void_p(Y.ctypes.data) if a["y"] else None, 0, a["dtype"], a["n"], a["total"], a["ld"],
                               None if codes is None else _lib.iptr(codes), a["ng"], None if cols is None else _lib.iptr(cols),
                               a["n_cols"], count.ctypes.data_as(LLP) if a["count"] else None, _lib.dptr(sums) if a["sums"] else None)
    return rc, L.pilot_ot_last_error()


@pytest.mark.parametrize("bad,fragment", [
    (dict(y=False), b"NULL"), (dict(codes=None), b"NULL"), (dict(count=False), b"NULL"), (dict(sums=False), b"NULL"),
    (dict(n=-1), b"n=-1"),
    (dict(total=0, n_cols=0, ld=0), b"n_cols_total=0"),
    (dict(ld=4), b"ld=4"),
    (dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"),
    (dict(ng=0), b"n_groups"), (dict(ng=-3), b"n_groups"), (dict(ng=2 ** 20 + 1), b"n_groups"),
    (dict(n_cols=-1, cols=[0]), b"n_sel=-1"),
    (dict(n_cols=4), b"n_sel=4"),                                  # fewer than all of them without cols
    (dict(cols=[0, 5], n_cols=2), b"outside [0, 5)"),
    (dict(cols=[-1], n_cols=1), b"outside [0, 5)"),
    (dict(codes=[0, 1, 2, 1, -1, 0]), b"codes[2]=2"),
])
def test_dense_entry_point_refuses_before_any_hip_call(bad, fragment):
    rc, msg = _dense_call(**bad)
    assert rc == _lib.EINVAL and fragment in msg, (bad, msg)


def test_good_arguments_get_as_far_as_the_device():
    for kw in (dict(), dict(ng=2 ** 20), dict(cols=[4, 0, 4], n_cols=3), dict(ld=8)):
        rc, msg = _dense_call(**kw)
        assert rc == (_lib.OK if _lib.device_count() > 0 else _lib.EHIP), (kw, msg)


def test_what_needs_no_device_needs_none():
    """no selected column, or no used row: the counts (and zeros) come back without a device"""
    rc, msg = _dense_call(cols=[0], n_cols=0)
    assert rc == _lib.OK, msg
    rc, msg = _dense_call(codes=[-1] * 6)
    assert rc == _lib.OK, msg


def test_sparse_entry_point_refuses_what_it_can_judge_without_a_matrix():
    L = _lib.load()
    count, sums = np.zeros(8, dtype=np.int64), np.zeros(8)
    codes = np.zeros(4, dtype=np.int32)

    def call(ng=2, n_cols=1):
        return L.pilot_ot_csr_group_sums(None, _lib.iptr(codes), ng, None, n_cols, count.ctypes.data_as(LLP), _lib.dptr(sums))
    for ng in (0, -1, 2 ** 20 + 1):
        assert call(ng=ng) == _lib.EINVAL and b"n_groups" in L.pilot_ot_last_error()
    assert call(n_cols=-1) == _lib.EINVAL and b"n_cols=-1" in L.pilot_ot_last_error()
    assert call() == _lib.EINVAL and b"NULL" in L.pilot_ot_last_error()
    assert call(ng=2 ** 20) == _lib.EINVAL and b"NULL" in L.pilot_ot_last_error()


def test_constants_and_symbols():
    L = _lib.load()
    assert L.pilot_ot_group_sums_slice_rows() == engine.group_sums_slice_rows() >= 64
    B = L.pilot_ot_group_sums_col_block()
    assert B == engine.group_sums_col_block() and B % 64 == 0 and 8 * B <= 160 * 1024          # f64 accumulators within the LDS
    for name in ("pilot_ot_group_sums", "pilot_ot_csr_group_sums", "pilot_ot_group_sums_slice_rows", "pilot_ot_group_sums_col_block"):
        assert name in _lib.SYMBOLS


# ---- engine ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def shell(no_library):
    """a DeviceCSR of 6 x 5 around a handle that must never be used"""
    S = engine.DeviceCSR(ctypes.c_void_p(0x1000), (6, 5), np.float32, 7)
    yield S
    S.h = None                                                     # (nothing to destroy)


CODES = np.array([0, 1, 0, 1, -1, 0])
BAD_ARGS = [
    dict(codes=CODES[:5]),                                        # length different from n
    dict(codes=CODES.reshape(2, 3)),
    dict(codes=CODES.astype(np.float64)),
    dict(codes=np.array([0, 1, 2, 1, -1, 0])),                    # a code >= n_groups
    dict(n_groups=0), dict(n_groups=2 ** 20 + 1), dict(n_groups=2.5), dict(n_groups=True),
    dict(cols=[0, 5]), dict(cols=[-1]), dict(cols=[[0, 1]]), dict(cols=[0.0]),
]


@pytest.mark.parametrize("kwargs", BAD_ARGS)
def test_group_sums_argument_errors(shell, kwargs):
    args = dict(codes=CODES, n_groups=2)
    args.update(kwargs)
    with pytest.raises(ValueError):
        engine.group_sums(np.zeros((6, 5), dtype=np.float32), **args)
    with pytest.raises(ValueError):
        shell.group_sums(**args)
    with pytest.raises(ValueError):                                # the module-level function forwards a DeviceCSR
        engine.group_sums(shell, **args)


def test_group_sums_matrix_arguments(shell):
    for Y in (np.zeros((6, 5), dtype=np.int32), np.zeros(6, dtype=np.float32), np.zeros((5, 6), dtype=np.float32).T, [[0.0] * 5] * 6):
        with pytest.raises(ValueError):
            engine.group_sums(Y, CODES, 2)
    D = engine.DeviceMatrix(0x1000, 6, shape=(6, 5), dtype=np.float32)
    with pytest.raises(ValueError):
        engine.group_sums(D, CODES[:4], 2)
    with pytest.raises(ValueError):
        engine.group_sums(engine.device_columns(D, 1, 4), CODES, 2, cols=[3])
    for route in (D, engine.device_columns(D, 1, 4), np.zeros((6, 5))):    # every check passed: the call is the first use of the library
        with pytest.raises(AssertionError, match="touched"):
            engine.group_sums(route, CODES, 2 ** 20)
    with pytest.raises(AssertionError, match="touched"):
        shell.group_sums(CODES, 600, cols=[4, 0, 4])


# ---- tl.deseq2_size_factors -------------------------------------------------------------------------------------------------------
def test_size_factors_by_hand():
    """genes 0 and 1 are positive in both samples: geometric means 4 and 4, ratios {0.5, 2} and {2, 0.5}, medians of logs 0"""
    counts = pd.DataFrame([[2, 8, 0], [8, 2, 5]], index=["a", "b"], columns=["g0", "g1", "g2"])
    sf = tl.deseq2_size_factors(counts)
    assert isinstance(sf, pd.Series) and list(sf.index) == ["a", "b"]
    assert np.allclose(sf.values, [1.0, 1.0], rtol=1e-15, atol=0)
    assert np.allclose(PR.size_factors(counts), [1.0, 1.0], rtol=1e-15, atol=0)


def test_size_factors_even_number_of_usable_genes():
    counts = np.array([[10.0, 3.0, 0.0, 40.0, 7.0],
                       [20.0, 9.0, 5.0, 10.0, 1.0],
                       [5.0, 27.0, 8.0, 80.0, 2.0]])               # gene 2 has a zero: four usable genes, the median is a mean of two
    sf = tl.deseq2_size_factors(pd.DataFrame(counts, index=list("xyz")))
    want = PR.size_factors(counts)
    assert np.all(np.abs(sf.values - want) <= 1e-15 * want)
    # by hand for sample x: log ratios against the geometric means (10, 9, 40^(1/3) * 800^(1/3) = 31.748..., 14^(1/3))
    gm = np.array([1000.0, 729.0, 32000.0, 14.0]) ** (1.0 / 3.0)
    r = np.sort(np.array([10.0, 3.0, 40.0, 7.0]) / gm)
    assert abs(sf["x"] - np.sqrt(r[1] * r[2])) <= 1e-14 * sf["x"]


def test_size_factors_round_half_to_even():
    """DESeq2 takes round(counts), R's round: 2.5 -> 2 and 3.5 -> 4; a count of 0.5 rounds to 0 and takes its gene out"""
    counts = np.array([[2.5, 6.0, 0.5, 3.0], [3.5, 6.0, 9.0, 12.0]])
    sf = tl.deseq2_size_factors(pd.DataFrame(counts))
    rounded = np.array([[2.0, 6.0, 0.0, 3.0], [4.0, 6.0, 9.0, 12.0]])
    want = PR.size_factors(rounded)
    assert np.all(np.abs(sf.values - want) <= 1e-15 * want)
    assert np.all(np.abs(PR.size_factors(counts) - want) <= 1e-15 * want)
    other = PR.size_factors(np.array([[3.0, 6.0, 1.0, 3.0], [4.0, 6.0, 9.0, 12.0]]))          # half away from zero would give this
    assert np.abs(other - want).max() > 1e-3


def test_size_factors_need_one_gene_without_a_zero():
    with pytest.raises(ValueError, match="zero"):
        tl.deseq2_size_factors(pd.DataFrame([[0, 3, 4], [5, 0, 4], [5, 3, 0]]))
    with pytest.raises(ValueError):
        PR.size_factors([[0, 3, 4], [5, 0, 4], [5, 3, 0]])


# ---- tl.pseudobulk_inputs: the frame logic, the device call stubbed ------------------------------------------------------------------
class _Adata:
    def __init__(self, X, obs, var_names):
        self.X, self.obs, self.var_names = X, obs, var_names


def _tiny():
    """7 cells x 4 genes, types T / U, samples s3 s1 s2 (s2 only in U); gene g2 is zero in T, g1 only counts in T's s3"""
    X = np.array([[1, 2, 0, 0], [3, 0, 0, 1], [0, 4, 0, 2], [5, 0, 0, 0], [0, 0, 7, 1], [2, 0, 1, 0], [1, 0, 0, 3]], dtype=np.float32)
    obs = pd.DataFrame({"cell_types": np.array(["T", "T", "T", "T", "U", "U", "T"], dtype=object),
                        "sampleID": np.array(["s3", "s1", "s3", "s1", "s2", "s1", "s9"], dtype=object)})
    props = pd.DataFrame({"Predicted_Labels": ["A", "B", "A", "B"], "other": [1, 2, 3, 4]}, index=["s1", "s2", "s3", "s9"])
    return _Adata(X, obs, ["g0", "g1", "g2", "g3"]), props


@pytest.fixture
def host_sums(monkeypatch):
    """engine.group_sums answered by the restatement: only tl's host side is under test here"""
    monkeypatch.setattr(engine, "group_sums", lambda Y, codes, n_groups, cols=None: PR.group_sums(Y, codes, n_groups, cols))


def test_pseudobulk_inputs_frame_logic(host_sums):
    adata, props = _tiny()
    aggr = PR.aggr_counts(adata).astype(np.float64)
    counts, meta = tl.pseudobulk_inputs(adata, props, "T")
    want_counts, want_meta = PR.pseudobulk_inputs(aggr, props, "T")
    pd.testing.assert_frame_equal(counts, want_counts, check_exact=True)
    pd.testing.assert_frame_equal(meta, want_meta, check_exact=True)
    assert list(counts.index) == ["s1", "s3", "s9"] and counts.index.name == "sampleID"        # sorted, observed samples of T only
    assert list(counts.columns) == ["g0", "g1", "g3"]                                        # g2 is zero in every sample of T
    assert list(meta.columns) == ["Predicted_Labels", "other", "stage"] and list(meta["stage"]) == ["A", "A", "B"]
    assert counts.attrs["n_cells"] == {"s1": 2, "s3": 2, "s9": 1}
    assert "stage" not in props.columns                                                      # the caller's frame is not written to

    counts, meta = tl.pseudobulk_inputs(adata, props, "T", remove_samples=["s3", "s2", "nowhere"])
    want_counts, want_meta = PR.pseudobulk_inputs(aggr, props, "T", remove_samples=["s3", "s2", "nowhere"])
    pd.testing.assert_frame_equal(counts, want_counts, check_exact=True)
    pd.testing.assert_frame_equal(meta, want_meta, check_exact=True)
    assert list(counts.index) == ["s1", "s9"] and list(meta.index) == ["s1", "s9"]
    assert list(counts.columns) == ["g0", "g3"]                                              # g1 counted only in the removed s3
    assert counts.attrs["n_cells"] == {"s1": 2, "s9": 1}
    counts, _ = tl.pseudobulk_inputs(adata, props, "T", remove_samples=None)                   # the reference allows None
    assert list(counts.index) == ["s1", "s3", "s9"]


def test_pseudobulk_counts_index_and_errors(host_sums, no_library):
    adata, props = _tiny()
    full = tl.pseudobulk_counts(adata)
    pd.testing.assert_frame_equal(full, PR.aggr_counts(adata).astype(np.float64), check_exact=True)
    assert full.index.names == ["cell_types", "sampleID"]
    assert list(full.index) == [("T", "s1"), ("T", "s3"), ("T", "s9"), ("U", "s1"), ("U", "s2")]          # observed combinations only
    assert full.attrs["n_cells"] == {("T", "s1"): 2, ("T", "s3"): 2, ("T", "s9"): 1, ("U", "s1"): 1, ("U", "s2"): 1}
    pd.testing.assert_frame_equal(tl.pseudobulk_counts(adata, "U"), full.loc["U"], check_exact=True)
    with pytest.raises(ValueError, match="no cell"):
        tl.pseudobulk_counts(adata, "V")
    with pytest.raises(KeyError):                                  # a sample of the cell type missing from proportion_df
        tl.pseudobulk_inputs(adata, props.drop(index="s9"), "T")
