"""The pseudobulk tables on the device (K14: tl.pseudobulk_counts, tl.pseudobulk_inputs, tl.deseq2_size_factors) against the
reference's pandas expressions on the dense frame and the explicit size-factor loop (tests/pseudobulk_restatement.py).

Cohort: 900 cells x 40 genes of Poisson counts, 3 cell types x 7 samples with one (type, sample) combination absent, one gene that
counts only in a sample the test removes and one that is zero everywhere.  Every sum of these counts is an integer far below 2^24,
which the reference's float32 frame and the device's float64 sums both hold exactly: the frames must be EQUAL (values, index, names,
column order) once the pandas result is cast to float64."""
import functools

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import pseudobulk_restatement as PR
from pilot_amd import engine, tl

pytestmark = pytest.mark.gpu

TYPES, SAMPLES = ["beta", "alpha", "gamma"], ["p%d" % i for i in (5, 1, 7, 3, 2, 6, 4)]
ABSENT = ("alpha", "p3")
REMOVED = "p6"


class _Adata:
    def __init__(self, X, obs, var_names):
        self.X, self.obs, self.var_names, self.uns = X, obs, var_names, {}


@functools.lru_cache(maxsize=None)
def _cohort():
    rng = np.random.default_rng(14)
    n, G = 900, 40
    cell = rng.choice(TYPES, n)
    sample = rng.choice(SAMPLES, n)
    clash = (cell == ABSENT[0]) & (sample == ABSENT[1])
    sample[clash] = "p1"
    K = rng.poisson(rng.gamma(2.0, 1.5, G), (n, G))
    K[:, 17] = 0                                                   # zero in every cell
    K[:, 23] = np.where((cell == "alpha") & (sample == REMOVED), K[:, 23] + 1, 0)              # counts only in the removed sample
    obs = pd.DataFrame({"cell_types": cell.astype(object), "sampleID": sample.astype(object)})
    props = pd.DataFrame({"Predicted_Labels": ["Tumor %d" % (1 + i % 3) for i in range(7)], "frac": np.linspace(0.1, 0.7, 7)},
                         index=sorted(SAMPLES))
    return K, obs, props, ["g%02d" % j for j in range(G)]


def _adata(kind, labels):
    K, obs, props, genes = _cohort()
    if kind == "csr":
        X = sp.csr_matrix(K.astype(np.float32))
        for r in range(X.shape[0]):                                # reverse every row: the indices come unsorted
            a, b = X.indptr[r], X.indptr[r + 1]
            X.indices[a:b], X.data[a:b] = X.indices[a:b][::-1].copy(), X.data[a:b][::-1].copy()
        X.has_sorted_indices = False
    else:
        X = K.astype(kind)
    if labels == "categorical":
        obs = obs.astype("category")
    return _Adata(X, obs, genes), props


@functools.lru_cache(maxsize=None)
def _want():
    K, obs, props, genes = _cohort()
    aggr = PR.aggr_counts(_Adata(K.astype(np.float32), obs, genes))
    assert aggr.to_numpy().dtype == np.float32                     # the reference's frame
    return aggr.astype(np.float64)


KINDS = [np.float32, np.float64, "csr"]


@pytest.fixture
def no_toarray(monkeypatch):
    def refuse(self, *a, **k):
        raise AssertionError("the sparse matrix was made dense on the host")
    for cls in (sp.csr_matrix, getattr(sp, "csr_array", sp.csr_matrix)):
        monkeypatch.setattr(cls, "toarray", refuse)
        monkeypatch.setattr(cls, "todense", refuse)


@pytest.mark.parametrize("labels", ["object", "categorical"])
@pytest.mark.parametrize("kind", KINDS, ids=["f32", "f64", "csr"])
def test_counts_equal_the_reference_frame(kind, labels, no_toarray):
    want = _want()
    assert len(want) == 20 and ABSENT not in want.index and want.index.names == ["cell_types", "sampleID"]
    adata, _ = _adata(kind, labels)
    got = tl.pseudobulk_counts(adata)
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    sizes = adata.obs.astype(object).groupby(["cell_types", "sampleID"]).size()
    assert got.attrs["n_cells"] == dict(zip(sizes.index.tolist(), sizes.tolist()))
    for cell in TYPES:
        one = tl.pseudobulk_counts(adata, cell)
        pd.testing.assert_frame_equal(one, want.loc[cell], check_exact=True)
        assert one.index.name == "sampleID" and sum(one.attrs["n_cells"].values()) == int((adata.obs["cell_types"] == cell).sum())
    assert len(tl.pseudobulk_counts(adata, "alpha")) == 6          # the absent combination is no row
    with pytest.raises(ValueError, match="no cell"):
        tl.pseudobulk_counts(adata, "delta")


@pytest.mark.parametrize("kind", KINDS, ids=["f32", "f64", "csr"])
def test_inputs_and_size_factors(kind, no_toarray):
    adata, props = _adata(kind, "object")
    want_counts, want_meta = PR.pseudobulk_inputs(_want(), props, "alpha", remove_samples=[REMOVED, "p3"])
    assert "g17" not in want_counts.columns and "g23" not in want_counts.columns and REMOVED not in want_counts.index
    counts, meta = tl.pseudobulk_inputs(adata, props, "alpha", remove_samples=[REMOVED, "p3"])
    pd.testing.assert_frame_equal(counts, want_counts, check_exact=True)
    pd.testing.assert_frame_equal(meta, want_meta, check_exact=True)
    assert list(meta["stage"]) == list(meta["Predicted_Labels"]) and list(meta.index) == list(counts.index)
    kept, _ = tl.pseudobulk_inputs(adata, props, "alpha")
    assert "g23" in kept.columns and "g17" not in kept.columns and REMOVED in kept.index
    sf = tl.deseq2_size_factors(counts)
    ref = PR.size_factors(want_counts)
    assert list(sf.index) == list(counts.index) and np.all(np.abs(sf.values - ref) <= 1e-15 * ref)
    assert 0.3 < sf.min() <= 1.0 <= sf.max() < 3.0                 # (samples of a few dozen cells each: factors around 1)
