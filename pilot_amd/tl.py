"""``pilot_amd.tl`` -- host-side mirror of the ``pilotpy.tl`` functions on the Wasserstein path.

Same names, arguments, defaults, ``adata.uns`` keys and Python types as the reference
(``pilotpy/tools/Trajectory.py``), so code written against ``pilotpy.tl.wasserstein_distance``
runs unchanged; the pair loop and the centroid distance matrix execute on the MI355X through
``libpilot_ot.so`` (``pilot_amd.engine``).  Nothing here falls back to a CPU solver.

=============================================  ==========================================
this module                                    reference (``/root/reference/pilotpy/tools/``)
=============================================  ==========================================
wasserstein_distance                           Trajectory.py:36-115
extract_data_anno_scRNA_from_h5ad              Trajectory.py:234-266
extract_data_anno_pathomics_from_h5ad          Trajectory.py:270-299
set_path_for_results                           Trajectory.py:146-164
Cluster_Representations                        Trajectory.py:377-436
cost_matrix                                    Trajectory.py:441-475
wasserstein_d                                  Trajectory.py:479-523
return_real_labels                             Trajectory.py:617-642
Sil_computing                                  Trajectory.py:592-612
Precomputed_distance                           Trajectory.py:1687-1727
diffusion_kernel                               plot/ploting.py:95-110 (the dense part of pl.trajectory)
diffusion_map                                  plot/ploting.py:95-110 (pl.trajectory's embedding, without the plot)
cell_importance                                Trajectory.py:646-800 (the table and uns keys, without plots or files)
genes_importance                               Trajectory.py:860-995 (the table, without plots or files)
get_noised_curves, cluster_genes_curves,       plot/gene_selection_analysis.py:86-203, 360-415, 850-955 and
compute_curves_activities,                     plot/curve_activity.py (the frames, without plots, files or
genes_selection_analysis                       enrichment)
compute_diff_expressions,                      patients_sub_clustering.py:15-240 (limma's lmFit / eBayes / topTable
extract_cells_from_gene_expression_for_...,    restated from device moments, without R, plots or files) and
highly_variable_genes,                         scanpy's pp.highly_variable_genes(flavor='seurat') restated;
cell_type_diff_two_sub_patient_groups          plot/ploting.py:460-556 (the table, without the plot or the file)
pseudobulk_counts, pseudobulk_inputs,          plot/pseudobulk_DE_analysis.py:590-610 (get_pseudobulk_DE's aggregation and the
deseq2_size_factors                            inputs of its R calls) and DESeq2's median-of-ratios size factors restated
deseq2_dispersions, compute_pseudobulk_DE,     plot/pseudobulk_DE_analysis.py:96-159, 628-646 (DESeq2's NB GLM for `~ stage` restated:
get_pseudobulk_DE                              dispersions, Wald test, BH; no apeglm shrinkage, rlog, plots, files or R)
pca, extract_annot_expression                  Trajectory.py:171-228 (scanpy's normalize_total / log1p / scale / tl.pca restated;
                                               no reclustering)
neighbors                                      Trajectory.py:217-220, 1045-1060 (scanpy's pp.neighbors: the exact kNN graph of the
                                               cells and UMAP's connectivities restated)
louvain, reclustering_data                     Trajectory.py:217-220, 1000-1062 (sknetwork's Louvain(resolution) of the neighbour
                                               graph by a synchronous, deterministic rule)
leiden, leiden_clustering, sil_ari                  Trajectory.py:527-588, 107-113 (sc.tl.leiden by the synchronous rule of DESIGN.md
                                               K20: connected communities, labels unpinned; the resolution loop and the Rand index
                                               of Clustering; the tail of return_sil_ari=True, which itself stays as it was)
select_best_sil, clustering_emd                plot/ploting.py:384-458, 287-354 (the silhouette sweep over resolutions and the
                                               samples' Predicted_Labels, without plots or files; Louvain by default,
                                               method="leiden" for the reference's choice)
select_best_resolution, silhouette             the same sweep over cells, on the matrix-free silhouette (not in the reference)
=============================================  ==========================================
"""
from __future__ import annotations

import ctypes
import os
import threading

import numpy as np
import pandas as pd

from . import engine

path_to_results = None  # module global, as in the reference (Trajectory.py:254)

# engine options that have no counterpart in the reference signature; set via `engine_options`
_DEFAULT_ENGINE_OPTIONS = dict(precision="auto")


def set_path_for_results():
    """Create ``Results_PILOT/plots`` under the cwd and return it (Trajectory.py:146-164).

    The reference does this as a side effect of every ``wasserstein_distance`` call; set
    ``PILOT_AMD_NO_RESULTS_DIR=1`` to skip the mkdir (the path is still returned).
    """
    if os.environ.get("PILOT_AMD_NO_RESULTS_DIR", "") not in ("", "0"):
        return "Results_PILOT/plots"
    if not os.path.exists("Results_PILOT/plots"):
        os.makedirs("Results_PILOT/plots")
    return "Results_PILOT/plots"


def extract_data_anno_scRNA_from_h5ad(adata, emb_matrix="PCA", clusters_col="cell_type",
                                      sample_col="sampleID", status="status"):
    """(data, annot) for scRNA input: ``adata.obsm[emb_matrix]`` as a frame with columns
    ``PCA_1..D``; ``adata.obs`` columns renamed ``cell_type, sampleID, status`` (Trajectory.py:234-266)."""
    global path_to_results
    data = adata.obsm[emb_matrix]
    col_add = ["PCA_" + str(i) for i in range(1, data.shape[1] + 1)]
    # The reference's frame is an independent copy of the embedding (DataFrame(...).reset_index(drop=True), :249-252).  The
    # frame built here VIEWS adata.obsm[emb_matrix]; wasserstein_distance replaces its array by a private copy (made on a
    # helper thread beside the device work) before it stores the frame in adata.uns['data'].  Direct callers of this helper
    # get the view.
    data = pd.DataFrame(data, columns=col_add)
    annot = _annot_frame(adata.obs, clusters_col, sample_col, status)
    path_to_results = set_path_for_results()
    return data, annot


def extract_data_anno_pathomics_from_h5ad(adata, var_names=[], clusters_col="Cell_type",
                                          sample_col="sampleID", status="status"):
    """(data, annot) for pathomics input: ``adata[:, var_names].X`` (Trajectory.py:270-299)."""
    global path_to_results
    data = adata[:, var_names].X
    data = pd.DataFrame(data, columns=var_names)
    annot = _annot_frame(adata.obs, clusters_col, sample_col, status)
    path_to_results = set_path_for_results()
    return data, annot


def _annot_frame(obs, clusters_col, sample_col, status):
    """``obs[[clusters_col, sample_col, status]]`` renamed to ``cell_type, sampleID, status`` with a fresh RangeIndex
    (Trajectory.py:257-262): one column selection (new arrays, dtypes kept); the shallow copy on top only drops pandas'
    "this is a slice of another frame" marker, so that later column assignments on ``adata.uns['annot']`` neither warn
    (SettingWithCopyWarning under the reference's pandas 2.0) nor touch ``adata.obs``."""
    annot = obs[[clusters_col, sample_col, status]].copy(deep=False)
    annot.columns = ["cell_type", "sampleID", "status"]
    annot.index = pd.RangeIndex(len(annot))
    return annot


def _first_appearance_codes(series):
    """(codes, uniques) with uniques in first-appearance order, as ``Series.unique()`` gives; missing values get -1.

    ``pd.factorize`` on an object column hashes millions of Python objects (~25 ms per 1.8 M cells and column) and holds the
    interpreter lock.  Two shortcuts, both one native pass of ``libpilot_ot.so`` (``engine.label_codes``, int32 codes out,
    no lock held -- ``wasserstein_distance`` runs its two columns side by side):

    * categorical columns (what AnnData gives for ``obs`` labels): the integer codes are there already, only their
      numbering is changed to first appearance;
    * object columns: the labels of 1.8 M cells are a few hundred distinct Python objects repeated (AnnData / pandas /
      numpy fancy indexing copy POINTERS), so the column is numbered by object identity and only the distinct objects
      are then factorised by value (equal strings at different addresses merge there).
    """
    if isinstance(series.dtype, pd.CategoricalDtype):
        values = series.array
        raw = values.codes                                            # int8 / int16 / int32 (int64 beyond 2^31 categories)
        if raw.dtype.itemsize <= 4:
            codes, first = engine.label_codes(raw, max_uniques=len(values.categories) + 1)
            return codes, np.asarray(values.categories[raw[first]])
        seen = pd.unique(raw[raw >= 0]) if (raw < 0).any() else pd.unique(raw)       # category numbers, first appearance
        remap = np.full(len(values.categories) + 1, -1, dtype=np.int64)              # (slot -1 serves the missing code)
        remap[seen] = np.arange(len(seen))
        return remap[raw], np.asarray(values.categories[seen])
    arr = series.to_numpy()
    if arr.dtype == object and arr.ndim == 1 and arr.strides == (arr.itemsize,) and arr.size:
        ptrs = np.ctypeslib.as_array((ctypes.c_size_t * arr.size).from_address(arr.ctypes.data))      # (arr stays alive here)
        #  the shortcut only pays while the labels are few shared objects: a column built row by row holds one
        # str object per cell (as many pointers as cells) -- such a column goes the plain way
        got = engine.label_codes(ptrs.view(np.uint64), max_uniques=max(4096, arr.size // 8))
        if got is None:
            codes, uniques = pd.factorize(series, sort=False, use_na_sentinel=True)
            return codes, np.asarray(uniques)
        pcodes, first = got
        objs = arr[first]                                              # the distinct objects, in order of first appearance
        vcodes, uniques = pd.factorize(objs, sort=False, use_na_sentinel=True)
        if len(uniques) == len(objs) and np.array_equal(vcodes, np.arange(len(objs))):
            return pcodes, np.asarray(uniques)                         # every object its own value: the identity codes stand
        lut = np.append(vcodes, -1).astype(np.int32)                   # (slot -1 serves the missing code)
        return lut[pcodes], np.asarray(uniques)
    codes, uniques = pd.factorize(series, sort=False, use_na_sentinel=True)
    return codes, np.asarray(uniques)


def Cluster_Representations(df, cell_col=0, sample_col=1, regulizer=0.2, normalization=True):
    """Proportions of clusters per sample (Trajectory.py:377-436).

    Returns an insertion-ordered dict ``{sampleID: float64[K]}``: samples and cell types in
    first-appearance order (``.unique()``, :402/:412); prior_k = regulizer * n_k / (C - 1)
    (:405-409, note C - 1); with ``normalization`` p = (counts + prior) / (sum counts + sum prior)
    (:428-430).  The host only factorises the two label columns into integer codes; the histogram and
    the smoothing run on the device (``engine.proportions``) and are bit-identical to the reference.
    """
    cell_col = df.columns[cell_col]
    sample_col = df.columns[sample_col]
    ccodes, cells = _first_appearance_codes(df[cell_col])
    scodes, samples = _first_appearance_codes(df[sample_col])
    K, N = len(cells), len(samples)
    if str(cell_col) != "cell_type":
        # the reference counts n_k in the column literally named 'cell_type' (:403-407); with a different
        # cell_col the two must at least label the same partition
        other, _ = _first_appearance_codes(df["cell_type"])
        if not np.array_equal(other, ccodes):
            raise NotImplementedError("Cluster_Representations: cell_col differs from the 'cell_type' column")
    return _proportions_from_codes(ccodes, scodes, samples, K, len(df), regulizer, normalization)


def _proportions_from_codes(ccodes, scodes, samples, K, n_total, regulizer, normalization):
    N = len(samples)
    P = engine.proportions(ccodes, scodes, N, K, regulizer=regulizer, normalization=normalization, n_total=n_total)
    return dict(zip(samples, np.array(P, dtype=np.float64, order="C", copy=True)))


def cost_matrix(annot, data, metric="cosine"):
    """Ground-cost matrix between cell types (Trajectory.py:441-475): per-type column-wise MEDIAN
    centroids, pairwise ``metric`` distance (device kernel; scipy ``pdist`` names), returned as
    ``(ndarray K x K, DataFrame indexed 'cell_types')``.  NOT normalised (the caller divides by max)."""
    codes, cells = _first_appearance_codes(annot[annot.columns[0]])
    X = data.to_numpy() if isinstance(data, pd.DataFrame) else np.asarray(data)
    return _cost_from_codes(X, codes, cells, metric)


def _cost_from_codes(X, codes, cells, metric):
    centroids = engine.centroid_medians(X, codes, len(cells))
    return _cost_frame(engine.pdist_square(centroids, metric=metric), cells)


def _labelled_square_frame(A, names, index_name):
    """The frame the reference builds as ``from_dict(A).T`` + ``columns = names`` + a names column + ``set_index`` (Trajectory.py:470-473,
    :518-521), in ONE constructor call: the transposed values in a block of their own (the frame must not alias the array it was made
    from), ``names`` as columns and as the named index.  Same object for every consumer -- values, dtypes, both axes and the index
    name are asserted equal to the reference's construction in tests/test_host_logic.py; a third of the time at 634 samples."""
    # (the reference's columns pass through a frame that also holds the str-labelled names column: their Index is of object dtype
    # whatever the labels are, while the index takes the dtype pandas infers for the labels)
    return pd.DataFrame(np.ascontiguousarray(np.asarray(A).T), index=pd.Index(names, name=index_name),
                        columns=pd.Index(names, dtype=object), copy=False)


def _cost_frame(dis, cells):
    return dis, _labelled_square_frame(dis, cells, "cell_types")


def wasserstein_d(Clu_rep, cost, regularized="unreg", reg=0.1, engine_options=None):
    """Wasserstein distances among all ordered sample pairs (Trajectory.py:479-523).

    ``regularized == "unreg"`` -> exact OT (``ot.emd2``); anything else -> entropic OT with POT's
    ``sinkhorn_stabilized`` semantics (``ot.sinkhorn2``).  Returns ``(EMD float64 N x N, DataFrame)``;
    the frame is ``DataFrame.from_dict(EMD).T`` indexed by sample id, exactly as the reference builds it.
    """
    samples_id = list(Clu_rep.keys())
    if len(samples_id) == 0:
        EMD = np.zeros((0, 0))
    else:
        P = np.stack([np.asarray(Clu_rep[s], dtype=np.float64) for s in samples_id])
        EMD = _pair_grid(P, cost, regularized, reg, engine_options)
    return EMD, _emd_frame(EMD, samples_id)


def _pair_grid(P, cost, regularized, reg, engine_options):
    """The N x N matrix of all ordered pairs on the device(s): the loop of Trajectory.py:505-515."""
    opts = dict(_DEFAULT_ENGINE_OPTIONS)
    opts.update(engine_options or {})
    cost = np.asarray(cost, dtype=np.float64)
    if regularized == "unreg":
        # ot.emd2 (POT 0.9: check_marginals=True) refuses histograms of different mass before it rescales them:
        # np.testing.assert_almost_equal(a.sum(0), b.sum(0), decimal=6).  With normalization=False the reference's
        # proportions are raw counts and this is what stops it (Trajectory.py:428-436, :511).
        sums = P.sum(1)
        if sums.size and float(sums.max() - sums.min()) >= 1.5e-6:
            raise AssertionError("a and b vector must have the same sum (sample masses range from %g to %g)"
                                 % (sums.min(), sums.max()))
    multi = {k: opts.pop(k) for k in ("devices", "n_devices", "gather") if k in opts}
    if multi.get("devices") is not None or (multi.get("n_devices") or 1) > 1:
        # the pair grid row-sharded over several GPUs of this node, one RCCL all-gather (pilot_amd.multi)
        from . import multi as _multi
        if regularized == "unreg":
            return _multi.emd_grid_multi(P, cost, **multi)
        return _multi.sinkhorn_grid_multi(P, cost, reg, **multi, **opts)
    if regularized == "unreg":
        return engine.emd_grid(P, cost)
    return engine.sinkhorn_grid(P, cost, reg, **opts)


def _emd_frame(EMD, samples_id):
    return _labelled_square_frame(EMD, samples_id, "sampleID")


def return_real_labels(df, category="status", sample_col=1):
    """First status value of every sample, samples in first-appearance order (Trajectory.py:617-642)."""
    scodes, samples = _first_appearance_codes(df[df.columns[sample_col]])
    return _labels_from_codes(scodes, len(samples), df[category].to_numpy())


def _labels_from_codes(scodes, n_samples, cond):
    first_row = np.full(n_samples, -1, dtype=np.int64)
    idx = np.flatnonzero(scodes >= 0)
    # first occurrence of each sample code: assign the row numbers back to front, the earliest row is written last
    first_row[scodes[idx][::-1]] = idx[::-1]
    return [cond[r] for r in first_row]


def _values_at(series, rows):
    """``[series.iloc[r] for r in rows]`` as ``Series.unique()[0]`` hands the values out, without materialising a
    categorical column (1.8 M Python references for a few hundred lookups)."""
    if isinstance(series.dtype, pd.CategoricalDtype):
        values = series.array
        codes = values.codes[np.asarray(rows, dtype=np.int64)]
        cats = values.categories.to_numpy()             # (one array lookup: `categories[c]` per element is 0.4 us of pandas each)
        out = list(cats[np.where(codes >= 0, codes, 0)]) if len(cats) else [np.nan] * len(codes)
        for i in np.flatnonzero(codes < 0):
            out[i] = np.nan
        return out
    values = series.to_numpy()
    return [values[int(r)] for r in rows]


_libc = None


def _empty_like_huge(X):
    """``np.empty_like(X)`` whose pages the kernel may back with 2 MB huge pages (``madvise(MADV_HUGEPAGE)`` where transparent
    huge pages are in ``madvise`` mode): the private copy of a 216 MB embedding is 52 000 first-touch page faults otherwise,
    which is most of what the copy costs."""
    global _libc
    huge = 2 << 20
    if X.nbytes < 8 * huge or not X.flags.c_contiguous:
        return np.empty_like(X)
    try:
        if _libc is None:
            _libc = ctypes.CDLL(None, use_errno=True)
        raw = np.empty(X.nbytes + huge, dtype=np.uint8)
        off = (-raw.ctypes.data) % huge
        _libc.madvise(ctypes.c_void_p(raw.ctypes.data + off), ctypes.c_size_t((X.nbytes // huge) * huge), 14)       # MADV_HUGEPAGE; advisory
        return raw[off:off + X.nbytes].view(X.dtype).reshape(X.shape)
    except Exception:
        return np.empty_like(X)


class _DeviceWorker:
    """ONE long-lived helper thread that runs the device chain of ``wasserstein_distance`` (the library caches its
    workspace per calling thread: a fresh thread per call would rebuild it every time)."""

    class _Job:
        def __init__(self):
            self.done = threading.Event()
            self.error = None

        def wait(self):
            self.done.wait()

    def __init__(self):
        import queue
        self.q = queue.SimpleQueue()
        self.thread = threading.Thread(target=self._loop, name="pilot_amd_device_chain", daemon=True)
        self.thread.start()

    def _loop(self):
        from . import _lib
        while True:
            job, device, fn, args = self.q.get()
            try:
                _lib.check(_lib.load().pilot_ot_set_device(device))      # (the caller's current device)
                fn(*args)
            except BaseException as e:                                     # handed to the submitting thread
                job.error = e
            finally:
                job.done.set()

    def submit(self, device, fn, *args):
        job = self._Job()
        self.q.put((job, device, fn, args))
        return job


_worker = None
_worker_lock = threading.Lock()


def _device_worker():
    global _worker
    with _worker_lock:
        if _worker is None or not _worker.thread.is_alive():
            _worker = _DeviceWorker()
        return _worker


_SIL_ARI_MESSAGE = ("return_sil_ari=True: the ARI is the Rand index of a Leiden clustering of the finished matrix "
                    "(pilotpy.tl.Clustering, Trajectory.py:525-588: scanpy neighbors + leiden) -- a consumer of adata.uns['EMD'] "
                    "outside this engine's scope (SURVEY.md section 2 #6), so it is run by the reference's OWN function and "
                    "pilotpy (with scanpy / leidenalg) is not importable here: %s.  Run wasserstein_distance without it; the "
                    "silhouette alone is tl.Sil_computing(EMD / EMD.max(), adata.uns['real_labels']) (INTEGRATION.md, 'Sil / ARI')")


def _reference_clustering():
    """``pilotpy.tools.Trajectory.Clustering`` (Trajectory.py:525-588) when the reference package and its scanpy / leidenalg
    stack are installed next to this engine -- imported lazily, only for ``return_sil_ari=True``; nothing of it is restated
    here.  Raises NotImplementedError (before any device work) when it is not importable."""
    try:
        from pilotpy.tools.Trajectory import Clustering
    except Exception as e:            # ImportError, or whatever the eager import chain of pilotpy raises
        raise NotImplementedError(_SIL_ARI_MESSAGE % (repr(e),)) from e
    return Clustering


def Sil_computing(EMD, real_labels, metric="cosine"):
    """Silhouette score of a labelling of the samples, the rows of ``EMD`` being the points (Trajectory.py:592-612:
    ``sklearn.metrics.silhouette_score(EMD, real_labels, metric=metric)``; callers pass ``EMD / EMD.max()``,
    plot/ploting.py:324).  Row-to-row distances and the score are chained on the device (the matrix goes up once, N per-sample
    scores come back); metric "cosine" or "euclidean".  ``EMD`` may also be an ``engine.DeviceMatrix`` (a result still in HBM)."""
    return engine.silhouette_of_rows(EMD, real_labels, metric=metric)


def diffusion_kernel(adata, epsilon=1, knn=64):
    """The dense part of ``pl.trajectory`` (plot/ploting.py:95-110): ``EMD / EMD.max()``, Euclidean distances between its
    rows, and pydiffmap's k-nearest-neighbour Gaussian kernel ``exp(-d^2 / (4 epsilon))``, all on the device.  Returns
    ``(EMD_normalised_row_distances, kernel_matrix)``; the eigen-decomposition stays with pydiffmap / scipy."""
    return engine.diffusion_kernel_of_rows(adata.uns["EMD"], k=knn, epsilon=epsilon)


def diffusion_map(adata, n_evecs=2, epsilon=1, alpha=0.5, knn=64):
    """What ``pl.trajectory`` (plot/ploting.py:95-110) stores before it plots: pydiffmap's
    ``DiffusionMap.from_sklearn(n_evecs, epsilon, alpha, k=knn).fit_transform(EMD / EMD.max())`` in ``adata.uns['embedding']``
    (float64, N x n_evecs, sample order), computed on the device from ``adata.uns['EMD']`` (a numpy array or an
    ``engine.DeviceMatrix``).  Returns the embedding.  A disconnected neighbour graph (eigenvalue 1 repeated: the coordinates
    sqrt(-1 / lambda) are meaningless) or an eigensolver that did not converge raises ValueError and leaves ``adata.uns``
    alone.  The plot itself is not part of this; the pseudotime along the embedding is :func:`fit_principal_graph`'s."""
    E = adata.uns["EMD"]
    dmap, _, _, info = engine.diffusion_map_of_rows(E, n_evecs=n_evecs, epsilon=epsilon, alpha=alpha, k=knn, return_info=True)
    if info["degenerate"]:
        raise ValueError("diffusion map: the %d-nearest-neighbour graph of the samples is (nearly) disconnected -- eigenvalue 1 "
                         "of the Markov matrix is repeated; raise knn" % knn)
    if not info["converged"]:
        raise ValueError("diffusion map: the eigensolver did not converge in %d Lanczos steps" % info["steps"])
    adata.uns["embedding"] = dmap
    return dmap


def fit_principal_graph(adata, NumNodes=20, source_node=0, Lambda=0.01, Mu=0.1, X=None):
    """fit_pricipla_graph (plot/ploting.py:229-282) without ElPiGraph, plots or files: the elastic principal tree of the
    embedding (``engine.principal_tree``, ``NumNodes`` nodes, elasticity ``Lambda`` / ``Mu``) and every sample's pseudotime along
    it from node ``source_node`` (``engine.tree_pseudotime``), both on the device.  The points are ``X`` when given, else
    ``adata.uns['embedding']`` (:func:`diffusion_map`).  Writes ``adata.uns['pseudotime']`` (n float64, row order) and
    ``adata.uns['principal_graph']``: ``nodes``, ``edges`` (each as (a, b) with a the end nearer the source), ``energy`` of the
    tree, per point the ``edge`` it projects onto and the parameter ``t`` along it, and ``params``.  Returns the pseudotime.
    Nothing is written when a step raises.  The rule is this library's statement of the published algorithm (README, "Principal
    tree"), not a pin to an elpigraph release."""
    if X is None:
        if "embedding" not in adata.uns:
            raise KeyError("fit_principal_graph needs points: run tl.diffusion_map (adata.uns['embedding']) or pass X=")
        X = adata.uns["embedding"]
    nodes, edges, info = engine.principal_tree(X, n_nodes=NumNodes, lam=Lambda, mu=Mu, return_info=True)
    pseudotime, _, edge, t = engine.tree_pseudotime(X, nodes, edges, source=source_node)
    oriented, _ = engine.tree_orientation(nodes, edges, source_node)
    adata.uns["pseudotime"] = pseudotime
    adata.uns["principal_graph"] = {"nodes": nodes, "edges": oriented, "energy": info["energy"][-1], "edge": edge, "t": t,
                                    "params": {"NumNodes": int(NumNodes), "source_node": int(source_node), "Lambda": float(Lambda),
                                               "Mu": float(Mu), "steps": info["steps"]}}
    return pseudotime


fit_pricipla_graph = fit_principal_graph      # the reference's spelling


def wasserstein_distance(adata, emb_matrix="X_PCA", clusters_col="cell_types", sample_col="sampleID",
                         status="status", metric="cosine", regulizer=0.2, normalization=True,
                         regularized="unreg", reg=0.1, res=0.01, steper=0.01, data_type="scRNA",
                         return_sil_ari=False, engine_options=None):
    """Wasserstein distance among samples (Trajectory.py:36-115); results go to ``adata.uns``:
    ``data, annot, proportions, cost, EMD_df, EMD, real_labels``.

    ``engine_options`` (not in the reference): dict forwarded to the device engine, e.g.
    ``{"precision": "fp64"}``; ``{"n_devices": G}`` (or ``{"devices": [0, 1, ...]}``) row-shards the pair grid over G GPUs
    of this node with one RCCL all-gather -- same bits as the single-GPU matrix.
    """
    # (Trajectory.py:108-113) the Leiden / ARI tail is the reference's own function: found, or refused, BEFORE any device work
    reference_clustering = _reference_clustering() if return_sil_ari else None
    if metric not in engine._lib.METRICS:
        raise NotImplementedError("metric %r: the device kernel implements scipy's pdist names %s" % (metric, sorted(engine._lib.METRICS)))
    global path_to_results
    # the embedding frame first (extract_data_anno_*_from_h5ad, :234-299): its bytes start moving at once
    if data_type == "scRNA":
        X = adata.obsm[emb_matrix]
        data = pd.DataFrame(X, columns=["PCA_" + str(i) for i in range(1, X.shape[1] + 1)])
    else:
        var_names = list(adata.var_names)
        data = pd.DataFrame(adata[:, var_names].X, columns=var_names)
    # While the label columns are numbered (native passes, side by side), helper threads move bytes: the embedding to the device
    # (H2D) and into the private copy that adata.uns['data'] holds, like the reference's.
    X = data.to_numpy()
    upload = engine.EmbeddingUpload(X)
    own = _empty_like_huge(X)
    n_copy = min(8, max(1, (os.cpu_count() or 2) - 2)) if X.size >= (1 << 22) else (1 if X.nbytes >= (4 << 20) else 0)
    bounds = np.linspace(0, X.shape[0], max(n_copy, 1) + 1).astype(np.int64)
    copiers = [threading.Thread(target=np.copyto, args=(own[a:b], X[a:b]), name="pilot_amd_data_copy")
               for a, b in zip(bounds[:-1], bounds[1:])] if n_copy else []
    if not n_copy:
        np.copyto(own, X)          # (a small embedding: a thread costs more than the copy)
    for t in copiers:
        t.start()
    dev = {}

    def device_chain(ccodes, scodes, n_samples, n_types):
        # runs with the GIL released almost throughout (ctypes calls): proportions + first rows + medians, pdist, pair grid
        try:
            dev["P"], dev["first"], centroids = upload.prepass(ccodes, scodes, n_samples, n_types, regulizer=regulizer,
                                                               normalization=normalization, n_total=len(ccodes))
            cost = engine.pdist_square(centroids, metric=metric)
            dev["cost"] = cost
            dev["EMD"] = _pair_grid(dev["P"], cost / cost.max(), regularized, reg, engine_options) if n_samples else np.zeros((0, 0))
        except BaseException as e:          # re-raised on the calling thread
            dev["error"] = e
    chain = None
    try:
        # the two label columns are numbered ONCE (first-appearance order, Trajectory.py:402,412), straight from adata.obs,
        # and shared by the three steps that the reference runs as separate pandas scans; the cell-type column on a helper
        # thread beside the sample column on this one when the columns are long enough to pay for the thread ...
        side = {}
        if len(adata.obs) >= (1 << 17):
            def number_types():
                try:
                    side["cells"] = _first_appearance_codes(adata.obs[clusters_col])
                except BaseException as e:
                    side["error"] = e
            helper = threading.Thread(target=number_types, name="pilot_amd_label_codes")
            helper.start()
            try:
                scodes, samples = _first_appearance_codes(adata.obs[sample_col])
            finally:
                helper.join()
            if "error" in side:
                raise side["error"]
            ccodes, cells = side["cells"]
        else:
            ccodes, cells = _first_appearance_codes(adata.obs[clusters_col])
            scodes, samples = _first_appearance_codes(adata.obs[sample_col])
        chain = _device_worker().submit(upload.device, device_chain, ccodes, scodes, len(samples), len(cells))
        # ... and while the device works, this thread does the GIL-bound part: the annotation frame (a copy of three object
        # columns of adata.obs, Trajectory.py:257-262)
        annot = _annot_frame(adata.obs, clusters_col, sample_col, status)
        path_to_results = set_path_for_results()
    finally:
        if chain is not None:
            chain.wait()
        upload.close()
        for t in copiers:
            t.join()
    if "error" in dev or chain.error is not None:
        raise dev.get("error") or chain.error
    # One private N x K block, a row view per sample (634 separate copies were a third of a millisecond).  Same values, keys and
    # order as the reference's dict (Trajectory.py:432-436); unlike its independent arrays the rows share a base array: `arr.base`
    # is the block and `arr.flags.owndata` is False, so a consumer that keeps one row keeps the block alive.
    proportions = dict(zip(samples, np.array(dev["P"], dtype=np.float64, order="C", copy=True)))
    first_rows = dev["first"]
    adata.uns["data"] = pd.DataFrame(own, columns=data.columns, copy=False)
    adata.uns["annot"] = annot
    adata.uns["proportions"] = proportions
    cost, cost_df = _cost_frame(dev["cost"], cells)
    adata.uns["cost"] = cost_df
    EMD = dev["EMD"]
    adata.uns["EMD_df"] = _emd_frame(EMD, list(proportions.keys()))
    adata.uns["EMD"] = EMD
    # first status value of every sample (return_real_labels, :617-642): the first row of a sample came out of the
    # device pass over the codes
    # (the values as ``Series.unique()[0]`` hands them out; ``.iloc`` per sample on a categorical column was 3 - 6 ms at 634 samples)
    real_labels = _values_at(annot["status"], first_rows)
    if reference_clustering is not None:      # Trajectory.py:108-113: the reference's Clustering on the finished matrix, the silhouette on the device
        _predicted, ARI, real_labels = reference_clustering(EMD / EMD.max(), annot, metric=metric, res=res, steper=steper)
        adata.uns["real_labels"] = real_labels
        adata.uns["Sil"] = Sil_computing(EMD / EMD.max(), real_labels, metric=metric)
        adata.uns["ARI"] = ARI
        return
    adata.uns["real_labels"] = real_labels


def _plan_inputs(adata):
    """P (samples in uns['proportions'] order), the cost handed to the pair loop (uns['cost'] / its max, Trajectory.py:101)
    and the cell-type labels, from what wasserstein_distance left in adata.uns."""
    uns = adata.uns
    if "proportions" not in uns or "cost" not in uns:
        raise ValueError("adata.uns has no 'proportions' / 'cost': run wasserstein_distance first")
    samples = list(uns["proportions"].keys())
    P = np.stack([np.asarray(uns["proportions"][s], dtype=np.float64) for s in samples])
    cost_df = uns["cost"]
    cost = np.asarray(cost_df, dtype=np.float64)
    return samples, P, cost / cost.max(), list(cost_df.index), list(cost_df.columns)


def transport_plans(adata, pairs, regularized="unreg", reg=0.1):
    """Optimal couplings of sample pairs: how much of each cell type of the source sample moves to each cell type of the
    target.  EXTENSION, not in pilotpy (its pair loop keeps only the value of ``ot.emd`` / ``ot.sinkhorn``).

    Uses what ``wasserstein_distance`` left in ``adata.uns`` and writes nothing to it.  ``pairs``: list of
    (source sampleID, target sampleID).  The cost is ``uns['cost'] / uns['cost'].max()``, the one the pair loop gets
    (Trajectory.py:101).  ``regularized == "unreg"``: an exact optimal plan (the optimum's value is unique, its plan need not
    be); otherwise POT's ``sinkhorn_stabilized`` plan in f64 with ``reg``.  Returns a list of K x K DataFrames, index = the
    source's cell types, columns = the target's, in ``uns['cost']`` order; <cost / max, plan> is ``uns['EMD']`` at the pair.
    """
    samples, P, M, rows, cols = _plan_inputs(adata)
    where = {s: k for k, s in enumerate(samples)}
    try:
        idx = np.array([(where[a], where[b]) for a, b in pairs], dtype=np.int64).reshape(-1, 2)
    except KeyError as e:
        raise ValueError("unknown sampleID %r" % (e.args[0],)) from None
    plans = engine.transport_plans(P, M, idx, regularized=regularized, reg=reg)
    return [pd.DataFrame(G, index=list(rows), columns=list(cols)) for G in plans]


def group_transport(adata, source, target, regularized="unreg", reg=0.1):
    """Mean optimal coupling from the samples of status ``source`` to those of status ``target``: the mean of the plans of
    every ordered pair (i, j), i of status ``source``, j of status ``target`` (statuses from ``uns['real_labels']``).
    EXTENSION, not in pilotpy.

    Writes nothing to ``adata.uns``.  Plans as in ``transport_plans``; the sum runs on the device in a fixed order (the
    result is the same bits on every run).  Rows sum to the mean source proportions; columns to the mean target proportions
    (exactly so for exact plans of equal-mass samples).  Returns a K x K DataFrame labelled like ``transport_plans``'.
    A status without samples raises ValueError.
    """
    samples, P, M, rows, cols = _plan_inputs(adata)
    labels = np.asarray(adata.uns["real_labels"], dtype=object)
    if len(labels) != len(samples):
        raise ValueError("uns['real_labels'] has %d entries for %d samples" % (len(labels), len(samples)))
    src = np.flatnonzero(labels == source)
    dst = np.flatnonzero(labels == target)
    for name, sel in ((source, src), (target, dst)):
        if sel.size == 0:
            raise ValueError("no sample has status %r (statuses: %s)" % (name, sorted(set(map(str, labels)))))
    idx = np.stack(np.meshgrid(src, dst, indexing="ij"), axis=-1).reshape(-1, 2)
    total = engine.transport_plans(P, M, idx, regularized=regularized, reg=reg, groups=np.zeros(len(idx), dtype=np.int32))[0]
    return pd.DataFrame(total / len(idx), index=list(rows), columns=list(cols))


def Precomputed_distance(adata, distances, cost_df, features_matrix, emb_matrix="X_PCA",
                         clusters_col="cell_types", sample_col="sampleID", status="status", data_type="scRNA"):
    """Store externally computed distances in ``adata.uns`` (Trajectory.py:1687-1727; the reference
    reads an undefined ``data_type`` at :1716 -- here it is an explicit argument)."""
    if data_type == "scRNA":
        data, annot = extract_data_anno_scRNA_from_h5ad(adata, emb_matrix=emb_matrix, clusters_col=clusters_col,
                                                        sample_col=sample_col, status=status)
    else:
        data, annot = extract_data_anno_pathomics_from_h5ad(adata, var_names=list(adata.var_names),
                                                            clusters_col=clusters_col, sample_col=sample_col,
                                                            status=status)
    adata.uns["data"] = data
    adata.uns["annot"] = annot
    adata.uns["proportions"] = features_matrix
    adata.uns["cost"] = cost_df
    adata.uns["EMD"] = distances
    adata.uns["real_labels"] = return_real_labels(annot)


def cell_level_wasserstein(adata, emb_matrix="X_PCA", sample_col="sampleID", status="status", reg=0.1, scale=None,
                           num_iter_max=1000, stop_thr=1e-9):
    """EXTENSION -- not part of pilotpy (BASELINE config 5): Wasserstein-2 distance between
    samples computed on their raw cell clouds instead of on cell-type proportions.

    Every sample is the uniform measure on its cells in ``adata.obsm[emb_matrix]``; the ground cost is the squared
    Euclidean distance divided by ``scale`` (default: twice the mean squared distance of the cells to the global
    centroid, i.e. the expected squared distance between two random cells); entropic OT with regularisation ``reg`` is
    solved in the log domain on the device for all ordered sample pairs.  Writes ``adata.uns['EMD_cell']`` (ndarray
    N x N of transport costs), ``adata.uns['EMD_cell_df']`` and ``adata.uns['real_labels']``; returns nothing, like
    ``wasserstein_distance``.

    Raises ``NotImplementedError`` when the cell farthest from the global centroid lies beyond the kernel's accuracy
    envelope, ``max_i |x_i - mean| * sqrt(2 log2(e) / (scale * reg)) > 50`` (include/pilot_ot.h): one stray cell is enough,
    and so is a reg too small for the spread of the cohort.  Drop the outlier cells, or raise ``scale`` or ``reg``.
    """
    X = np.asarray(adata.obsm[emb_matrix], dtype=np.float32)
    obs = adata.obs[[sample_col, status]].copy()
    obs.columns = ["sampleID", "status"]
    obs = obs.reset_index(drop=True)
    scodes, samples = _first_appearance_codes(obs["sampleID"])
    if (scodes < 0).any():
        raise ValueError("cells without a sample id")
    order = np.argsort(scodes, kind="stable")                 # group the cells of a sample, keep their order
    counts = np.bincount(scodes, minlength=len(samples))
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    Xg = np.ascontiguousarray(X[order])
    if scale is None:
        mu = Xg.mean(axis=0, dtype=np.float64)
        scale = 2.0 * float(((Xg.astype(np.float64) - mu) ** 2).sum(axis=1).mean())
    W = engine.cell_w2_grid(Xg, offsets, scale, reg, num_iter_max=num_iter_max, stop_thr=stop_thr)
    df = pd.DataFrame(W.T, columns=list(samples))
    df["sampleID"] = list(samples)
    df = df.set_index("sampleID")
    adata.uns["EMD_cell"] = W
    adata.uns["EMD_cell_df"] = df
    adata.uns["EMD_cell_scale"] = scale
    adata.uns["real_labels"] = return_real_labels(pd.DataFrame({"cell_type": 0, "sampleID": obs["sampleID"], "status": obs["status"]}))


# ---- trajectory model fits: cell_importance / genes_importance (Trajectory.py:646-995) -------------------------------------
_PATTERNS = {0: ("linear up", "linear down"),
             1: ("linear up quadratic up", "linear down quadratic up", "linear up quadratic down", "linear down quadratic down"),
             2: ("quadratic up", "quadratic down")}


def _bh_adjust(p):
    """Benjamini-Hochberg adjusted p-values (statsmodels' multipletests(method='fdr_bh')[1])."""
    return engine.bh_adjust(p)


def _fits_table(fits, names, id_col, p_val, modify_r2):
    """fit_best_model's sorted dict -> save_data's table (Cell_gene_selection.py:680-760) with numeric columns: targets with a
    chosen model, sorted by the deciding adjusted R^2 (descending, ties in target order), BH-adjusted Pearson p-values, rows
    with adjusted p <= p_val.  Returns (table, names of every selected target in sorted order)."""
    chosen = fits["chosen"]
    sel = np.flatnonzero(chosen >= 0)
    key = (fits["mod_rsquared_adj"] if modify_r2 else fits["rsquared_adj"])[sel, chosen[sel]]
    sel = sel[np.argsort(-key, kind="stable")]
    m = chosen[sel]
    params = fits["params"][sel, m]
    names = np.asarray(names, dtype=object)
    table = pd.DataFrame({
        id_col: names[sel],
        "Expression pattern": [_PATTERNS[int(a)][int(b)] for a, b in zip(m, fits["pattern"][sel])],
        "Slope": fits["slope"][sel],
        "Fitted function": [engine.TRAJFIT_MODELS[int(a)] for a in m],
        "Intercept": params[:, 0],
        "Treat": params[:, 1],
        "Treat2": params[:, 2],
        "adjusted P-value": _bh_adjust(fits["pearson_p"][sel]),
        "R-squared": fits["rsquared_adj"][sel, m],
        "mod_rsquared_adj": fits["mod_rsquared_adj"][sel, m],
    })
    if not (m == 1).any():                       # the reference drops Treat2 when no selected fit has three coefficients
        table = table.drop(columns="Treat2")
    return table[table["adjusted P-value"] <= p_val], list(names[sel])


def cell_importance(adata, pseudotime=None, p_val=1):
    """cell_importance (Trajectory.py:646-800) without plots or files: the cell-type proportions of ``adata.uns['proportions']``
    against the samples' rank in pseudotime, OLS fits of the three trajectory models per cell type on the device
    (``engine.trajectory_fits``, every p-value <= ``p_val`` to be eligible), and the report table (numeric columns).  Writes
    ``adata.uns['cellnames']`` (the selected cell types, best R^2 first) and ``adata.uns['orders']`` (sampleID, Time_score
    1..N in pseudotime order).  ``pseudotime``: one value per sample in ``uns['proportions']`` order; default
    ``adata.uns['pseudotime']`` (pilotpy's fit_pricipla_graph; here :func:`fit_principal_graph` writes it)."""
    if pseudotime is None:
        if "pseudotime" not in adata.uns:
            raise KeyError("cell_importance needs a pseudotime: pass pseudotime= (one value per sample, e.g. a diffusion "
                           "coordinate) or set adata.uns['pseudotime'] (pilotpy's fit_pricipla_graph)")
        pseudotime = adata.uns["pseudotime"]
    bins = adata.uns["proportions"]
    samples = list(bins.keys())
    P = np.stack([np.asarray(bins[k], dtype=np.float64) for k in samples])
    cell_types = adata.uns["annot"]["cell_type"].unique()
    pseudotime = np.asarray(pseudotime, dtype=np.float64).ravel()
    if pseudotime.size != len(samples):
        raise ValueError("pseudotime has %d values for %d samples" % (pseudotime.size, len(samples)))
    order = np.argsort(pseudotime, kind="stable")
    N = len(samples)
    fits = engine.trajectory_fits(P[order], np.arange(1, N + 1, dtype=np.float64), model="ols", pval_thr=p_val)
    table, cellnames = _fits_table(fits, cell_types, "Cell name", p_val, False)
    adata.uns["cellnames"] = cellnames
    adata.uns["orders"] = pd.DataFrame({"sampleID": np.asarray(samples, dtype=object)[order],
                                        "Time_score": np.arange(1, N + 1, dtype=np.int64)})
    return table


def _cell_rows(adata, name_cell, sample_col, col_cell, orders, col):
    """The reference's ``orders.merge(cells, on='sampleID')``: the cells of ``name_cell`` ordered by their sample's row in
    ``orders`` (cells of one sample in obs order; cells of samples missing from ``orders`` dropped).  (rows, time)"""
    obs = adata.obs
    cells = np.flatnonzero(np.asarray(obs[col_cell].isin([name_cell])))
    pos = {s: i for i, s in enumerate(orders["sampleID"])}
    rank = np.array([pos.get(s, -1) for s in np.asarray(obs[sample_col])[cells]], dtype=np.int64)
    keep = rank >= 0
    cells, rank = cells[keep], rank[keep]
    o = np.argsort(rank, kind="stable")
    return cells[o], np.asarray(orders[col], dtype=np.float64)[rank[o]]


def genes_importance(adata, name_cell, col="Time_score", p_value=0.05, model_type="HuberRegressor", epsilon_huber=1.35,
                     modify_r2=False, sample_col="sampleID", col_cell="cell_types", normalize=True):
    """genes_importance (Trajectory.py:860-995) without plots or files: the cells of ``name_cell`` in the order of
    ``adata.uns['orders']`` (what cell_importance wrote), optionally normalize_total(1e4) + log1p on the device (a restatement of
    scanpy's, unpinned), genes with a zero fraction > 0.95 dropped, then fits of the three trajectory models per gene
    against the cells' ``col``, the report table with numeric columns and each gene's ``proportion`` (zero fraction) and
    ``mean``.  A dense ``adata.X`` is normalised through the host-in, host-out ``pilot_ot_normalize_log1p``; a scipy sparse one
    goes up once as an ``engine.DeviceCSR`` (the chosen rows, taken with scipy), is counted and normalised there, and only the kept
    genes are made dense, in HBM, for the fits -- no dense copy exists on the host.  ``model_type``: 'HuberRegressor' (the OPTIMUM of its objective with
    ``epsilon_huber``; scikit-learn's own fit stops early on some fits with an x^2 feature) or 'LinearRegression'.  A
    (gene, model) whose Huber solve did not converge is ineligible, as the engine flags it."""
    if model_type not in ("HuberRegressor", "LinearRegression"):
        raise ValueError("model_type=%r must be 'HuberRegressor' or 'LinearRegression'" % (model_type,))
    rows, x = _cell_rows(adata, name_cell, sample_col, col_cell, adata.uns["orders"], col)
    genes = np.asarray(list(adata.var_names), dtype=object)
    if _is_sparse(adata.X):
        S = _sparse_rows(adata.X, rows)
        n = S.shape[0]
        zero = (n - S.column_nnz()) / n if n else np.zeros(S.shape[1])
        cols = np.flatnonzero(~(zero > 0.95)).astype(np.int32)
        if normalize:
            S.normalize_log1p(1e4)
        Y = S.densify(cols)
        del S
    else:
        X = _dense_rows(adata.X, rows)
        zero = (X == 0).mean(axis=0) if X.shape[0] else np.zeros(X.shape[1])
        cols = np.flatnonzero(~(zero > 0.95)).astype(np.int32)
        if normalize:
            Y = np.empty((X.shape[0], cols.size), dtype=X.dtype)
            _lib_check_normalize(X, cols, Y)
        else:
            Y = X[:, cols]
    fits = engine.trajectory_fits(Y, x, model="huber" if model_type == "HuberRegressor" else "ols", epsilon=epsilon_huber,
                                  pval_thr=p_value, modify_r2=modify_r2)
    table, _ = _fits_table(fits, genes[cols], "Gene ID", p_value, modify_r2)
    pro = pd.DataFrame({"Gene ID": genes[cols], "proportion": fits["zero_fraction"], "mean": fits["mean"]})
    return pd.merge(table, pro, on="Gene ID")


def _is_sparse(X):
    import scipy.sparse as sp
    return sp.issparse(X)


def _sparse_rows(X, rows):
    """The rows ``rows`` of the scipy sparse matrix X as an ``engine.DeviceCSR`` (any other sparse format is converted to CSR on
    the host first; nothing dense is formed)"""
    return engine.DeviceCSR.upload(X if X.format == "csr" else X.tocsr(), rows)


def _dense_rows(X, rows):
    """The rows ``rows`` of the dense matrix X as a C-contiguous float32 / float64 array"""
    X = np.asarray(X[rows])
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float32)
    return np.ascontiguousarray(X)


def _lib_check_normalize(X, cols, out):
    from . import _lib
    _lib.check(_lib.load().pilot_ot_normalize_log1p(X.ctypes.data, 0 if X.dtype == np.float32 else 1, X.shape[0], X.shape[1],
                                                    1e4, _lib.iptr(cols), int(cols.size), out.ctypes.data))


# ---- principal components (Trajectory.py:199-208: normalize_total -> log1p -> scale(max_value) -> sc.tl.pca) ------------------
def _gene_columns(adata, genes, n_vars):
    """``genes`` (names of ``adata.var_names`` or a boolean mask over them) as column indices; None: every column"""
    if genes is None:
        return None
    genes = np.asarray(genes)
    if genes.ndim != 1:
        raise ValueError("genes: a 1-D list of names or a boolean mask, got shape %s" % (genes.shape,))
    if genes.dtype == bool:
        if genes.size != n_vars:
            raise ValueError("genes: a mask of %d entries for %d genes" % (genes.size, n_vars))
        return np.flatnonzero(genes).astype(np.int32)
    where = pd.Index(adata.var_names).get_indexer(genes)
    if (where < 0).any():
        raise ValueError("genes not in adata.var_names: %s" % list(genes[where < 0][:5]))
    return where.astype(np.int32)


def pca(adata, n_comps=50, normalize=False, target_sum=1e4, scale=True, max_value=10, genes=None, key_added="X_pca"):
    """The embedding the other entry points read from ``adata.obsm['X_pca']``, made on the device from ``adata.X``: optionally
    scanpy's ``normalize_total(target_sum)`` + ``log1p`` (``normalize``; on the device copy only, ``adata.X`` is untouched), then
    ``pp.scale(max_value)`` and ``tl.pca`` restated (``engine.pca``; scanpy is not installed where this library is built and
    tested, so the rule is UNPINNED here: scanpy 1.9's ddof-1 scale with the clip on the upper side only, scikit-learn 1.3's
    u-based sign).  ``genes``: the genes to use, names or a boolean mask (default: all).  A scipy sparse ``adata.X`` goes up once as
    an ``engine.DeviceCSR`` and is never made dense; the standardised matrix is not formed either way.  Like scanpy, ``n_comps``
    is lowered to ``min(cells, genes) - 1`` when it is not below ``min(cells, genes)``.  Writes ``adata.obsm[key_added]`` (cells x
    n_comps, float32 as scanpy gives for float32 data), ``adata.varm['PCs']`` (all genes x n_comps, zero rows for genes not used)
    and ``adata.uns['pca'] = {'variance', 'variance_ratio'}``; returns the scores.  Differences from scanpy: all arithmetic is
    float64 (scanpy scales in float32), the Lanczos start vector is fixed (ARPACK's is random), and Z is never dense."""
    X = adata.X
    n, n_vars = X.shape
    cols = _gene_columns(adata, genes, n_vars)
    n_sel = n_vars if cols is None else cols.size
    if not 0 < float(target_sum) < np.inf:
        raise ValueError("target_sum=%r must be positive" % (target_sum,))
    if min(n, n_sel) >= 2 and n_comps is not None and n_comps >= min(n, n_sel):
        n_comps = min(n, n_sel) - 1
    engine._pca_args(n, n_vars, n_comps, scale, max_value, cols)       # every argument judged before anything goes up
    if _is_sparse(X):
        if not np.isfinite(X.data).all():
            raise ValueError("adata.X holds a non-finite value")
        Y = _sparse_rows(X, None)
        if normalize and Y.nnz:
            Y.normalize_log1p(target_sum)
    else:
        Y = _dense_rows(X, slice(None))
        if not np.isfinite(Y).all():
            raise ValueError("adata.X holds a non-finite value")
        if normalize and Y.size:
            from . import _lib
            out = np.empty_like(Y)
            every = np.arange(n_vars, dtype=np.int32)
            _lib.check(_lib.load().pilot_ot_normalize_log1p(Y.ctypes.data, _lib.dtype_code(Y.dtype), n, n_vars, float(target_sum),
                                                            _lib.iptr(every), n_vars, out.ctypes.data))
            Y = out
    scores, pcs, variance, ratio = engine.pca(Y, n_comps=n_comps, scale=scale, max_value=max_value, cols=cols)
    del Y
    PCs = np.zeros((n_vars, pcs.shape[1]))
    PCs[slice(None) if cols is None else cols] = pcs
    scores = scores.astype(np.float32)
    adata.obsm[key_added] = scores
    adata.varm["PCs"] = PCs
    adata.uns["pca"] = {"variance": variance, "variance_ratio": ratio}
    return scores


def extract_annot_expression(adata, columns=["cell_type_original", "patient_region", "region", "X_pca"], reclustering=False,
                             reduction=False, resu=0.1, max_value=10, target_sum=1e4):
    """(data, annot) of a scRNA data set (Trajectory.py:171-228).  ``data``: the embedding as a frame with columns ``PCA_1..``
    -- ``adata.obsm[columns[3]]``, or with ``reduction`` the one :func:`pca` makes from ``adata.X`` (normalize_total(target_sum),
    log1p, scale(max_value), 50 components) and writes to ``adata.obsm['X_pca']``; unlike the reference, ``adata.X`` itself is
    left as it is.  ``annot``: ``adata.obs[columns[:3]]`` renamed ``cell_types, sampleID, status``.  ``reclustering`` (Louvain
    communities of scanpy's neighbour graph) is not implemented here and raises before any device work: :func:`neighbors` makes
    the graph, the Louvain step is the missing part of THIS function -- :func:`louvain` and :func:`reclustering_data` take it."""
    if reclustering:
        raise NotImplementedError("extract_annot_expression: reclustering is not implemented: tl.neighbors builds the neighbour graph "
                                  "(obsp['distances'] / ['connectivities']), the Louvain communities of it are the missing part here; "
                                  "tl.louvain writes them to obs, tl.reclustering_data returns them")
    if reduction:
        data = pca(adata, normalize=True, target_sum=target_sum, scale=True, max_value=max_value)
    else:
        data = adata.obsm[columns[3]]
    data = pd.DataFrame(data, columns=["PCA_" + str(i) for i in range(1, data.shape[1] + 1)])
    annot = adata.obs[list(columns[0:3])].copy(deep=False)
    annot.columns = ["cell_types", "sampleID", "status"]
    return data, annot


def _metric_checked(metric):
    if metric not in ("euclidean", "cosine"):
        raise ValueError("metric=%r: euclidean or cosine" % (metric,))
    return metric


def _representation(adata, use_rep, n_pcs):
    """``adata.obsm[use_rep]``, or the strided view of its first ``n_pcs`` columns"""
    if use_rep not in adata.obsm:
        raise ValueError("adata.obsm has no %r (tl.pca makes 'X_pca')" % (use_rep,))
    X = adata.obsm[use_rep]
    if len(X.shape) != 2:
        raise ValueError("adata.obsm[%r] must be 2-D, got %s" % (use_rep, X.shape))
    if n_pcs is not None:
        if isinstance(n_pcs, bool) or not isinstance(n_pcs, (int, np.integer)) or not 1 <= n_pcs <= X.shape[1]:
            raise ValueError("n_pcs=%r outside [1, %d], the columns of adata.obsm[%r]" % (n_pcs, X.shape[1], use_rep))
        X = np.asarray(X)[:, :int(n_pcs)]
    return X


def neighbors(adata, n_neighbors=15, n_pcs=None, use_rep="X_pca", metric="euclidean", key_added=None):
    """The cell neighbour graph scanpy's ``pp.neighbors`` gives (Trajectory.py:217-220, 1045-1060), made on the device from
    ``adata.obsm[use_rep]`` (its first ``n_pcs`` columns, read as a strided view without a copy): the exact ``n_neighbors - 1``
    nearest other cells of every cell (``engine.knn``; ``n_neighbors`` counts the cell itself, as scanpy's does) under
    ``metric`` ``"euclidean"`` or ``"cosine"``, and UMAP's fuzzy-simplicial-set connectivities of them
    (``engine.knn_connectivities``).  Writes ``adata.obsp['distances']`` (cells x cells CSR, float64, ``n_neighbors - 1`` stored
    entries per row before ``eliminate_zeros()``, which scanpy also applies), ``adata.obsp['connectivities']`` (symmetric CSR,
    float64) and ``adata.uns['neighbors'] = {'connectivities_key', 'distances_key', 'params': {n_neighbors, method: 'umap', metric,
    use_rep, n_pcs}}``; with ``key_added`` the names are ``uns[key_added]``, ``obsp[key_added + '_distances']`` and
    ``obsp[key_added + '_connectivities']``, as scanpy names them.  An ``adata`` without ``obsp`` gets a dict.  Returns None.
    ValueError before any device work: a missing representation, ``n_neighbors < 2`` or ``n_neighbors - 1 > 64``, ``n_pcs``
    outside the representation.  Differences from scanpy: the graph is exact at every size (scanpy switches to approximate
    NN-descent above 4 096 cells); ties are ordered by index; sigma, rho and the weights are float64 (umap-learn: float32);
    ``method='gauss'``, ``knn=False`` and custom metrics are not offered.  scanpy and umap-learn are not installed where this
    library is built and tested, so the rule is UNPINNED here: it is held to tests/neighbors_restatement.py."""
    import scipy.sparse as sp
    if isinstance(n_neighbors, bool) or not isinstance(n_neighbors, (int, np.integer)) or n_neighbors < 2:
        raise ValueError("n_neighbors=%r: an integer of at least 2 (it counts the cell itself)" % (n_neighbors,))
    if n_neighbors - 1 > engine.KNN_MAX_K:
        raise ValueError("n_neighbors=%d: at most %d" % (n_neighbors, engine.KNN_MAX_K + 1))
    _metric_checked(metric)
    X = _representation(adata, use_rep, n_pcs)
    n = X.shape[0]
    if n < n_neighbors:
        raise ValueError("n_neighbors=%d needs at least as many cells, got %d" % (n_neighbors, n))
    k = int(n_neighbors) - 1
    indices, distances = engine.knn(X, k, metric=metric)
    connectivities = engine.knn_connectivities(indices, distances, int(n_neighbors))
    graph = sp.csr_matrix((distances.ravel(), indices.ravel(), np.arange(0, n * k + 1, k)), shape=(n, n))
    graph.eliminate_zeros()
    prefix = "" if key_added is None else key_added + "_"
    if getattr(adata, "obsp", None) is None:
        adata.obsp = {}
    adata.obsp[prefix + "distances"] = graph
    adata.obsp[prefix + "connectivities"] = connectivities
    adata.uns["neighbors" if key_added is None else key_added] = {
        "connectivities_key": prefix + "connectivities", "distances_key": prefix + "distances",
        "params": {"n_neighbors": int(n_neighbors), "method": "umap", "metric": metric, "use_rep": use_rep, "n_pcs": n_pcs}}


# ---- Louvain communities of the neighbour graph (Trajectory.py:217-220, 1000-1062: sknetwork's Louvain(resolution)) -------------
def _check_mode(mode):
    if mode not in ("connectivities", "distances"):
        raise ValueError("mode=%r: connectivities or distances" % (mode,))


def _neighbor_graph(adata, mode, neighbors_key):
    _check_mode(mode)
    key = "neighbors" if neighbors_key is None else neighbors_key
    entry = adata.uns.get(key) if hasattr(adata.uns, "get") else None
    name = entry.get(mode + "_key") if isinstance(entry, dict) else None
    obsp = getattr(adata, "obsp", None)
    if name is None or obsp is None or name not in obsp:
        raise ValueError("adata has no neighbour graph under uns[%r] / obsp: run tl.neighbors first" % (key,))
    return obsp[name]


def _write_communities(adata, cluster, resolution, mode, neighbors_key, key_added):
    labels, info = cluster(_neighbor_graph(adata, mode, neighbors_key), resolution=resolution, return_info=True)
    adata.obs[key_added] = pd.Categorical.from_codes(labels, categories=[str(c) for c in range(info["communities"])])
    adata.uns[key_added] = {"params": {"resolution": resolution, "mode": mode}, "modularity": info["modularity"]}


def louvain(adata, resolution=1.0, mode="connectivities", neighbors_key=None, key_added="louvain"):
    """The Louvain communities of the cells' neighbour graph, on the device (``engine.louvain``): reads the ``obsp`` matrix that
    ``adata.uns[neighbors_key or 'neighbors']`` names for ``mode`` (``"connectivities"`` or ``"distances"``, what :func:`neighbors`
    wrote), writes ``adata.obs[key_added]`` as a pandas Categorical of the strings ``"0" .. "k-1"`` (scanpy's convention; 0 is the
    largest community) and ``adata.uns[key_added] = {'params': {'resolution', 'mode'}, 'modularity': Q}``.  Returns None.  A
    missing graph raises ValueError naming ``tl.neighbors``.  The rule is synchronous and deterministic, not
    sknetwork's or scanpy's sequential, seeded sweep: where the node order decides, the labels differ from theirs.  Leiden is
    :func:`leiden`."""
    _write_communities(adata, engine.louvain, resolution, mode, neighbors_key, key_added)


def leiden(adata, resolution=1.0, mode="connectivities", neighbors_key=None, key_added="leiden"):
    """:func:`louvain` with ``engine.leiden`` in place of ``engine.louvain``: the same graph, the same
    ``adata.obs[key_added]`` Categorical and ``adata.uns[key_added] = {'params': {'resolution', 'mode'}, 'modularity': Q}``, but
    every community is connected in the graph.  Synchronous and deterministic, not leidenalg's seeded random refinement: the labels
    are not scanpy's ``tl.leiden`` labels.  Returns None."""
    _write_communities(adata, engine.leiden, resolution, mode, neighbors_key, key_added)


class _Cells:
    """what reclustering_data's array branch hands to :func:`neighbors`: the reference wraps the array in an AnnData"""

    def __init__(self, rep):
        self.obsm, self.uns, self.obsp = {"X": rep}, {}, {}


def reclustering_data(adata, resu=0.01, normalization=False, target_sum=1e6, n_neighbor=15, method_="umap", metric_t="cosine",
                      mode="distances", origine_scr_rna=False, dimension_rect=False, n_component=25):
    """The reference's re-clustering (Trajectory.py:1000-1062): the integer Louvain labels of the cells' neighbour graph.
    ``origine_scr_rna=True``: ``adata`` is an AnnData; :func:`pca` (50 components; ``normalize_total(target_sum)``, ``log1p`` and
    ``scale(max_value=10)`` iff ``normalization``) then :func:`neighbors` (``n_neighbors=n_neighbor``, ``metric=metric_t``,
    ``n_pcs=n_component`` iff ``dimension_rect``); a matrix of at most 50 genes without ``dimension_rect`` gives its neighbours from
    X itself, as scanpy does (with ``normalization`` that case raises NotImplementedError: the scaled matrix is never formed).  ``origine_scr_rna=False``: ``adata`` is a cells x features array and the neighbours are scanpy's
    defaults (15, euclidean), found on the array itself when it has at most 50 columns, else on its 50-component ``engine.pca``
    (no scaling).  Then ``engine.louvain`` of the ``mode`` matrix (``"distances"`` or ``"connectivities"``) at resolution ``resu``;
    returns the int32 label array.  ``method_`` other than ``"umap"`` raises ValueError.  Deviations from pilotpy: the Louvain rule
    is the synchronous one of DESIGN.md K17, not sknetwork's sequential sweep, so labels differ from pilotpy's where sknetwork's
    node order matters; ``adata.X`` and ``adata.raw`` are left alone (the reference normalises and scales ``adata`` in place); with
    ``origine_scr_rna`` the graph is left in ``adata.obsp`` / ``adata.uns['neighbors']`` and the scores in ``adata.obsm['X_pca']``,
    as scanpy leaves them."""
    if method_ != "umap":
        raise ValueError("method_=%r: only 'umap' (scanpy's default connectivities) is offered" % (method_,))
    _check_mode(mode)
    engine.check_resolution(resu)
    if origine_scr_rna:
        n_vars = adata.X.shape[1]
        if dimension_rect or n_vars > 50:
            pca(adata, n_comps=50, normalize=bool(normalization), target_sum=target_sum, scale=bool(normalization), max_value=10)
            neighbors(adata, n_neighbors=n_neighbor, metric=metric_t, n_pcs=n_component if dimension_rect else None)
        else:
            if normalization:
                raise NotImplementedError("reclustering_data: normalization=True with at most 50 genes and dimension_rect=False would take the "
                                          "neighbours from the normalised and scaled matrix itself, which is not formed here")
            cells = _Cells(_dense_rows(adata.X.toarray() if _is_sparse(adata.X) else adata.X, slice(None)))
            neighbors(cells, n_neighbors=n_neighbor, metric=metric_t, use_rep="X")
            if getattr(adata, "obsp", None) is None:
                adata.obsp = {}
            adata.obsp.update(cells.obsp)
            adata.uns["neighbors"] = cells.uns["neighbors"]
        graph = adata.obsp[mode]
    else:
        X = np.asarray(adata)
        if X.ndim != 2:
            raise ValueError("adata: a cells x features array, got shape %s" % (X.shape,))
        rep = _dense_rows(X, slice(None))
        if rep.shape[1] > 50:
            rep = engine.pca(rep, n_comps=50, scale=False)[0]
        cells = _Cells(rep)
        neighbors(cells, use_rep="X")
        graph = cells.obsp[mode]
    return engine.louvain(graph, resolution=resu)


# ---- choosing the resolution: silhouette sweeps (plot/ploting.py:287-458: select_best_sil, clustering_emd) ----------------------
_SWEEP_COLUMNS = ["resolution", "silhouette", "n_clusters", "modularity"]


def _resolution_list(resolutions, start, step, end):
    """a non-empty ``resolutions`` as floats, else the reference's list (ploting.py:408): 0.2, 0.3 .. 2.0 by default"""
    out = list(resolutions) if resolutions is not None and len(resolutions) else \
        [start + step * i for i in range(int((end - start) / step) + 1)]
    for res in out:
        engine.check_resolution(res)
    return [float(res) for res in out]


def _best_resolution(resolutions, scores, start):
    """the reference's rule (ploting.py:410-434): ``start`` unless a silhouette is > 0, then the first resolution, in list order,
    whose silhouette is strictly greater than every earlier one's; NaN never wins"""
    best_res, best_sil = start, 0
    for res, sil in zip(resolutions, scores):
        if float(sil) > best_sil:
            best_sil, best_res = sil, res
    return best_res


def _sweep(adata, resolutions, start, graph, score, cluster):
    """one ``cluster`` run (engine.louvain or engine.leiden) and one ``score(labels)`` per resolution; a labelling with one
    cluster, or one cluster per point, scores NaN"""
    n, rows = graph.shape[0], []
    for res in resolutions:
        labels, info = cluster(graph, resolution=res, return_info=True)
        k = info["communities"]
        rows.append((res, score(labels) if 2 <= k <= n - 1 else np.nan, k, info["modularity"]))
    frame = pd.DataFrame(rows, columns=_SWEEP_COLUMNS)
    adata.uns["best_res"] = _best_resolution(frame["resolution"], frame["silhouette"], start)
    return frame


def silhouette(adata, labels_key="louvain", use_rep="X_pca", n_pcs=None, metric="euclidean", key_added=None):
    """The silhouette of every cell under the labels ``adata.obs[labels_key]`` (what :func:`louvain` wrote), from the cells' rows of
    ``adata.obsm[use_rep]`` (its first ``n_pcs`` columns) on the device: ``engine.silhouette_samples`` (K18), which forms neither
    the cells x cells distance matrix nor a cells x clusters table.  Writes ``adata.obs[key_added or labels_key + '_silhouette']``
    (float64) and returns the mean, ``sklearn.metrics.silhouette_score``'s value.  ValueError before any device work: a missing
    representation or label column, an unknown metric, ``n_pcs`` outside the representation, fewer than 2 labels or one per cell."""
    _metric_checked(metric)
    X = _representation(adata, use_rep, n_pcs)
    if labels_key not in adata.obs:
        raise ValueError("adata.obs has no %r (tl.louvain writes 'louvain')" % (labels_key,))
    samples, score = engine.silhouette_samples(X, np.asarray(adata.obs[labels_key]), metric=metric, return_score=True)
    adata.obs[labels_key + "_silhouette" if key_added is None else key_added] = samples
    return score


def select_best_resolution(adata, resolutions=None, start=0.2, step=0.1, end=2, mode="connectivities", neighbors_key=None,
                           use_rep="X_pca", n_pcs=None, metric="euclidean", method="louvain"):
    """:func:`select_best_sil` at the cell level: for every resolution, ``engine.louvain`` of the graph :func:`neighbors` left in
    ``adata.obsp`` (``mode``, ``neighbors_key`` as in :func:`louvain`) and the mean of ``engine.silhouette_samples`` (K18) of
    the cells' rows of ``adata.obsm[use_rep]`` (its first ``n_pcs`` columns) under those labels.  The resolution list and the
    best-resolution rule are :func:`select_best_sil`'s.  Returns a frame with the columns ``resolution, silhouette, n_clusters,
    modularity`` and writes ``adata.uns['best_res']``; it writes no labels: call ``tl.louvain(adata, resolution=best_res)`` next.
    Every resolution costs one Louvain run plus one all-pairs pass over the cells (19 of each by default): the distances are
    recomputed, not kept, since cells x cells of them do not fit.  A labelling with one cluster, or one cluster per cell, gets NaN
    and is never best.  ``method="leiden"`` clusters with ``engine.leiden`` (K20) instead.  ValueError before any device work: a
    missing graph or representation, an unknown metric or method."""
    _metric_checked(metric)
    cluster = engine.check_clustering_method(method)
    resolutions = _resolution_list(resolutions, start, step, end)
    graph = _neighbor_graph(adata, mode, neighbors_key)
    X = _representation(adata, use_rep, n_pcs)
    if X.shape[0] != graph.shape[0]:
        raise ValueError("the graph has %d cells, adata.obsm[%r] %d" % (graph.shape[0], use_rep, X.shape[0]))
    return _sweep(adata, resolutions, start, graph,
                  lambda labels: engine.silhouette_samples(X, labels, metric=metric, return_score=True)[1], cluster)


_EMD_NEIGHBORS = 15          # scanpy's pp.neighbors default, which the reference takes for the samples


def _emd_square(EMD, name):
    E = np.ascontiguousarray(EMD, dtype=np.float64)
    if E.ndim != 2 or E.shape[0] != E.shape[1]:
        raise ValueError("%s must be samples x samples, got %s" % (name, E.shape))
    return E


def _emd_enough(E):
    if E.shape[0] < _EMD_NEIGHBORS:
        raise ValueError("%d samples: the neighbour graph of scanpy's defaults needs n_neighbors = %d of them" % (E.shape[0], _EMD_NEIGHBORS))


def _emd_points(adata, metric):
    """``uns['EMD']`` as the reference's ``sc.AnnData(EMD)`` has it: the samples are the points, the rows their coordinates"""
    _metric_checked(metric)
    if "EMD" not in adata.uns:
        raise ValueError("adata.uns has no 'EMD': run tl.wasserstein_distance first")
    E = _emd_square(adata.uns["EMD"], "uns['EMD']")
    _emd_enough(E)
    return E


def _emd_graph(E, metric):
    indices, distances = engine.knn(E, _EMD_NEIGHBORS - 1, metric=metric)
    return engine.knn_connectivities(indices, distances, _EMD_NEIGHBORS)


def select_best_sil(adata, resolutions=None, metric="cosine", start=0.2, step=0.1, end=2, method="louvain"):
    """The numerical core of the reference's ``pl.select_best_sil`` (plot/ploting.py:384-458; no plots, no files): the silhouette
    of the samples' clustering at every resolution, and the best resolution in ``adata.uns['best_res']``.  Returns a frame with
    the columns ``resolution, silhouette, n_clusters, modularity``.

    The rule, shared with :func:`clustering_emd`.  Points: the rows of ``uns['EMD']``, unnormalised, as ``sc.AnnData(EMD)`` has
    them.  Graph: ``engine.knn(E, 14, metric)`` then ``engine.knn_connectivities(.., 15)``, scanpy's defaults ``n_neighbors=15``,
    ``method='umap'``; fewer than 15 samples raise ValueError.  Clustering: ``engine.louvain(graph, resolution)``.  Silhouette:
    ``engine.silhouette_of_rows(E, labels, metric)`` -- on ``EMD`` here, on ``EMD / EMD.max()`` in :func:`clustering_emd`, as
    the reference does; the samples x samples matrix path is the right one at this size.  Resolution list: the reference's
    ``[start + step * i for i in range(int((end - start) / step) + 1)]``, 19 values 0.2 .. 2.0 by default.  Best resolution: the
    reference's rule, ``best_sil = 0``, ``best_res = start``, replaced only by a strictly greater silhouette, in list order.

    Deviations from pilotpy: Louvain by the synchronous rule of DESIGN.md K17 where the reference runs Leiden (the labels are
    unpinned, as everywhere in K17); the rows themselves are used (scanpy silently reduces them to 50 principal components when
    there are more than 50 samples); a non-empty ``resolutions`` is honoured (the reference overwrites its argument); a labelling
    with one cluster, or one cluster per sample, gets silhouette NaN and can never be best (the reference crashes inside
    scikit-learn).  ``method="leiden"`` clusters with ``engine.leiden`` (K20: Leiden by the synchronous rule, every group connected
    in the graph; still not leidenalg's labels).  ValueError before any device work: no ``uns['EMD']``, an unknown metric or
    method, fewer than 15 samples."""
    cluster = engine.check_clustering_method(method)
    E = _emd_points(adata, metric)
    resolutions = _resolution_list(resolutions, start, step, end)
    return _sweep(adata, resolutions, start, _emd_graph(E, metric),
                  lambda labels: engine.silhouette_of_rows(E, labels, metric=metric), cluster)


def clustering_emd(adata, res=0.3, metric="cosine", method="louvain"):
    """The numerical core of the reference's ``pl.clustering_emd`` (plot/ploting.py:287-354; no heat map): the sub-groups of the
    samples at resolution ``res``.  Returns the reference's ``proportion_df``: one row per sample (``uns['proportions']`` order),
    the columns ``uns['annot'].cell_type.unique()``, then ``Predicted_Labels`` (the strings "0" .. "k-1", 0 the largest group, as
    :func:`louvain` names them) and ``sampleID`` -- what :func:`compute_diff_expressions`,
    :func:`cell_type_diff_two_sub_patient_groups` and :func:`pseudobulk_inputs` take.  Writes ``adata.uns['clustering_emd'] =
    {'params': {res, metric}, 'silhouette', 'modularity'}``, the silhouette being the one the reference computes here and drops.

    The rule, shared with :func:`select_best_sil`.  Points: the rows of ``uns['EMD']``, unnormalised, as ``sc.AnnData(EMD)`` has
    them.  Graph: ``engine.knn(E, 14, metric)`` then ``engine.knn_connectivities(.., 15)``, scanpy's defaults ``n_neighbors=15``,
    ``method='umap'``; fewer than 15 samples raise ValueError.  Clustering: ``engine.louvain(graph, res)``.  Silhouette:
    ``engine.silhouette_of_rows`` with ``metric`` on ``EMD / EMD.max()`` here (on ``EMD`` in :func:`select_best_sil`), as the
    reference does.  Resolution list and best resolution: see :func:`select_best_sil`; pass ``res=adata.uns['best_res']``.

    Deviations from pilotpy: those of :func:`select_best_sil` (Louvain by K17's synchronous rule instead of Leiden, labels
    unpinned; the rows themselves instead of 50 principal components; NaN for a labelling of one cluster or of one per sample).
    ``method="leiden"`` clusters with ``engine.leiden`` (K20) and is recorded as ``params['method']``; the default leaves ``params``
    as it was.  ValueError before any device work: no ``uns['EMD']`` / ``['proportions']`` / ``['annot']``, an unknown metric or
    method, fewer than 15 samples, proportions that do not match EMD or the cell types."""
    cluster = engine.check_clustering_method(method)
    E = _emd_points(adata, metric)
    for key in ("proportions", "annot"):
        if key not in adata.uns:
            raise ValueError("adata.uns has no %r: run tl.wasserstein_distance first" % key)
    engine.check_resolution(res)
    proportions = adata.uns["proportions"]
    cell_types = adata.uns["annot"]["cell_type"].unique()
    proportion_df = pd.DataFrame(proportions).T
    if proportion_df.shape != (E.shape[0], len(cell_types)):
        raise ValueError("uns['proportions'] is %d samples x %d cell types, uns['EMD'] has %d samples and uns['annot'] %d cell types"
                         % (proportion_df.shape + (E.shape[0], len(cell_types))))
    labels, info = cluster(_emd_graph(E, metric), resolution=res, return_info=True)
    k = info["communities"]
    sil = engine.silhouette_of_rows(E, labels, metric=metric, normalize_by_max=True) if 2 <= k <= E.shape[0] - 1 else np.nan
    adata.uns["clustering_emd"] = {"params": {"res": res, "metric": metric}, "silhouette": sil, "modularity": info["modularity"]}
    if method != "louvain":
        adata.uns["clustering_emd"]["params"]["method"] = method
    proportion_df.columns = cell_types
    proportion_df["Predicted_Labels"] = np.array([str(c) for c in labels], dtype=object)
    proportion_df["sampleID"] = list(proportions.keys())
    return proportion_df


# ---- the samples' Leiden clusters against their statuses (Trajectory.py:527-588: Clustering; :107-113: return_sil_ari's tail) ---
def rand_index(labels_true, labels_pred):
    """``sklearn.metrics.rand_score``: the share of the pairs of points on which two labellings agree (together in both or apart in
    both), from the contingency table; 1.0 for fewer than two points.  It is the plain Rand index, not the adjusted one."""
    a, b = np.asarray(labels_true).ravel(), np.asarray(labels_pred).ravel()
    if a.shape != b.shape:
        raise ValueError("labels_true has %d entries, labels_pred %d" % (a.size, b.size))
    n = a.size
    if n < 2:
        return 1.0
    ia, ib = np.unique(a, return_inverse=True)[1], np.unique(b, return_inverse=True)[1]
    table = np.zeros((int(ia.max()) + 1, int(ib.max()) + 1), dtype=np.int64)
    np.add.at(table, (ia, ib), 1)

    def together(counts):                          # the pairs inside the cells / rows / columns of the table
        return int((counts * (counts - 1) // 2).sum())
    pairs = n * (n - 1) // 2
    return float(pairs + 2 * together(table) - together(table.sum(axis=1)) - together(table.sum(axis=0))) / float(pairs)


def leiden_clustering(EMD, df, category="status", sample_col=1, res=0.01, metric="cosine", steper=0.01, max_steps=1000):
    """The reference's ``Clustering`` (Trajectory.py:527-588) under a name of its own -- ``wasserstein_distance(return_sil_ari=True)``
    is pinned to the REFERENCE's function of that name, and ``tl`` keeps the name free for it: Leiden clusters of the samples, as many as there are statuses, and
    their Rand index against the statuses.  Points: the rows of ``EMD`` (callers pass ``EMD / EMD.max()``).  Graph: the one of
    :func:`select_best_sil` (``engine.knn(EMD, 14, metric)``, ``engine.knn_connectivities(.., 15)``; fewer than 15 samples raise
    ValueError), formed once.  The reference's loop on it with ``engine.leiden`` (K20): ``res += steper`` while there are fewer
    clusters than ``df[category].unique()``, ``res -= 0.001`` while there are more, stop at equality.  Returns ``(labels,
    rand_index, true_labels)``: the integer labels, :func:`rand_index` of them against ``true_labels`` (what the reference calls
    ARI is ``rand_score``, the plain Rand index), and the first ``category`` value of every sample in first-appearance order
    (:func:`return_real_labels`).  Deviations from pilotpy: Leiden by the synchronous rule (labels unpinned); ``category`` where
    the reference reads ``df.status``; the reference's loop can oscillate for ever, here ``max_steps`` steps without equality
    raise ValueError naming the last two resolutions and cluster counts, and so does a resolution that falls below 0.
    ValueError before any device work: ``EMD`` not square or not matching the samples, a missing column, an unknown metric,
    ``res`` negative or not finite, ``steper`` not positive, ``max_steps < 1``, fewer than 15 samples."""
    _metric_checked(metric)
    E = _emd_square(EMD, "EMD")
    if category not in df.columns:
        raise ValueError("df has no column %r" % (category,))
    if isinstance(sample_col, bool) or not isinstance(sample_col, (int, np.integer)) or not -len(df.columns) <= sample_col < len(df.columns):
        raise ValueError("sample_col=%r: the position of the sample column among %d" % (sample_col, len(df.columns)))
    engine.check_resolution(res)
    if isinstance(steper, bool) or not isinstance(steper, (int, float, np.integer, np.floating)) or not np.isfinite(steper) or steper <= 0:
        raise ValueError("steper=%r: a positive number" % (steper,))
    if isinstance(max_steps, bool) or not isinstance(max_steps, (int, np.integer)) or max_steps < 1:
        raise ValueError("max_steps=%r: an integer of at least 1" % (max_steps,))
    first_rows = ~df[df.columns[sample_col]].duplicated().to_numpy()           # (what return_real_labels returns, without the library)
    true_labels = list(df[category].to_numpy()[first_rows])
    if len(true_labels) != E.shape[0]:
        raise ValueError("EMD has %d samples, df[%r] %d" % (E.shape[0], df.columns[sample_col], len(true_labels)))
    _emd_enough(E)
    n_clust = len(df[category].unique())
    graph = _emd_graph(E, metric)
    res, seen = float(res), []
    for _ in range(int(max_steps)):
        if res < 0:
            raise ValueError("the resolution fell to %g with %d clusters for %d statuses (before it: resolution %g)"
                             % (res, seen[-1][1], n_clust, seen[-1][0]))
        labels, info = engine.leiden(graph, resolution=res, return_info=True)
        k = info["communities"]
        seen = seen[-1:] + [(res, k)]
        if k < n_clust:
            res = res + steper
        elif k > n_clust:
            res = res - 0.001
        else:
            return labels.astype(int), rand_index(true_labels, labels), true_labels
    raise ValueError("no resolution gave %d clusters in %d steps: the last two were resolution %g with %d clusters and %g with %d"
                     % ((n_clust, max_steps) + seen[0] + seen[-1]))


def sil_ari(adata, res=0.01, steper=0.01, metric="cosine"):
    """What the reference's ``wasserstein_distance(return_sil_ari=True)`` does after the distances (Trajectory.py:107-113), from
    ``uns['EMD']`` and ``uns['annot']``: :func:`leiden_clustering` of ``EMD / EMD.max()`` against the statuses, then ``uns['real_labels']``
    (the statuses), ``uns['Sil']`` (:func:`Sil_computing` of the statuses on ``EMD / EMD.max()``) and ``uns['ARI']`` (the Rand
    index).  Returns None.  ``wasserstein_distance(return_sil_ari=True)`` itself is unchanged."""
    E = _emd_points(adata, metric)
    if "annot" not in adata.uns:
        raise ValueError("adata.uns has no 'annot': run tl.wasserstein_distance first")
    E = E / E.max()
    _predicted, ari, real_labels = leiden_clustering(E, adata.uns["annot"], metric=metric, res=res, steper=steper)
    adata.uns["real_labels"] = real_labels
    adata.uns["Sil"] = Sil_computing(E, real_labels, metric=metric)
    adata.uns["ARI"] = ari


# ---- gene-cluster differentiation (Gene_cluster_specific.py:8-201, Trajectory.py:1129-1172) --------------------------------
_GCD_COLUMNS = ["gene", "cluster", "waldStat", "df", "pvalue", "FC", "Expression pattern", "fit-pvalue", "fit-rsquared",
                "fit-mod-rsquared"]
_GCD_TABLE_COLUMNS = ("Gene ID", "Fitted function", "Intercept", "Treat", "Expression pattern", "adjusted P-value", "R-squared",
                      "mod_rsquared_adj")


def _gcd_features(model, x, fill):
    """[1, f(x)] (generate_feature) or, with ``fill``, [1, x or 0, x^2 or 0] (generate_feature_by_fill_empty), as the reference
    builds them (np.append of a ones column)."""
    x = np.asarray(x, dtype=np.float64)
    if fill:
        f = {"linear": np.column_stack((x, np.zeros(x.shape[0]))), "linear_quadratic": np.column_stack((x, np.power(x, 2))),
             "quadratic": np.column_stack((np.zeros(x.shape[0]), np.power(x, 2)))}[model]
    else:
        f = {"linear": x.reshape(-1, 1), "linear_quadratic": np.column_stack((x, np.power(x, 2))),
             "quadratic": np.power(x, 2).reshape(-1, 1)}[model]
    return np.append(np.ones((len(f), 1)), f, axis=1)


def _gcd_params(row):
    """a table row's coefficients on [1, f(x)]: Intercept, Treat and, for linear_quadratic, Treat2 (the table may lack Treat2)"""
    names = ["Intercept", "Treat", "Treat2"] if row["Fitted function"] == "linear_quadratic" else ["Intercept", "Treat"]
    return np.asarray([float(row[k]) for k in names], dtype=np.float64)


def _gcd_fill_betas(model, params):
    """get_betas_by_table / get_betas_by_model: (Intercept, Feature, Feature2) with the model's missing slot 0"""
    if model == "linear":
        return [float(params[0]), float(params[1]), 0.0]
    if model == "quadratic":
        return [float(params[0]), 0.0, float(params[1])]
    return [float(params[0]), float(params[1]), float(params[2])]


def _gcd_draws(rs, sizes, n_bootstraps):
    """make_bootstraps' resamples in call order: for each size n, ``n_bootstraps`` times np.random.choice(range(n), n,
    replace=True) -- the same legacy stream as rs.randint(0, n, n) -- as an n x n_bootstraps int32 array (observation-major)."""
    out = []
    for n in sizes:
        a = np.empty((n, n_bootstraps), dtype=np.int32)
        for b in range(n_bootstraps):
            a[:, b] = rs.randint(0, n, n)
        out.append(a)
    return out


def _gcd_wald(polyline1, polyline2, betas, boot, log_fc_cutoff, eigen_thresh):
    """The reference's Wald step for one row, with its numpy / scipy calls: betas (6), boot (B x 6 bootstrap betas).
    Returns (waldStat, df, pvalue)."""
    from scipy import stats
    gene_covs = np.cov(np.ascontiguousarray(np.asarray(boot, dtype=np.float64).T), ddof=1)    # pandas' .cov() on the same layout
    CC = np.concatenate((polyline1, polyline2 * -1), axis=1)
    estFC = np.matmul(CC, np.array(betas, dtype=np.float64).reshape(6, 1))
    est = np.sign(estFC) * np.maximum(0, np.abs(estFC) - log_fc_cutoff)
    sigma = np.matmul(np.matmul(CC, gene_covs), CC.transpose())
    ev, V = np.linalg.eig(sigma)
    keep = ev / np.max(ev) > eigen_thresh
    r = int(np.sum(keep))
    half = np.matmul(V[keep].transpose(), np.diag(1 / np.sqrt(ev[keep])))      # rows of V: the reference's indexing
    hs = np.matmul(est.transpose(), half)
    stat = float(np.matmul(hs, hs.transpose()).ravel()[0].real)
    return stat, r, float(stats.chi2.sf(stat, r))


def _gcd_check_tables(tables, cluster_names):
    for c in cluster_names:
        if c not in tables:
            raise KeyError("cluster %r has no table in `tables` (%s)" % (c, sorted(map(str, tables))))
        missing = [k for k in _GCD_TABLE_COLUMNS if k not in tables[c].columns]
        if missing:
            raise ValueError("table of %r lacks the genes_importance columns %s" % (c, missing))
        bad = set(tables[c]["Fitted function"]) - set(engine.TRAJFIT_MODELS)
        if bad:
            raise ValueError("table of %r: unknown fitted functions %s" % (c, sorted(map(str, bad))))


def infer_gene_cluster_differentiation(adata, tables, gene_list=None, cluster_names=None, col="Time_score", fc_thr=1.5,
                                       eigenThresh=1e-8, n_points=20, start=1, end=20, n_bootstraps=50, random_state=None,
                                       sample_col="sampleID", col_cell="cell_types", normalize=True, return_info=False):
    """infer_gene_cluster_differentiation (Gene_cluster_specific.py:8-201) without plots or files: for every gene of
    ``gene_list`` and every cell type whose ``tables`` entry (cell type -> ``genes_importance`` table) lists it, a Wald test of
    its trend there against the mean trend of the other cell types listing it, with a bootstrap covariance.  Returns the
    ``extend_stats`` frame (columns ``gene, cluster, waldStat, df, pvalue, FC, Expression pattern, fit-pvalue, fit-rsquared,
    fit-mod-rsquared``; numeric columns numeric).  A gene in one cell type gives the row (1, 1, 0.0, 0.0).

    Cells come as in ``genes_importance`` (the cells of the type in ``adata.uns['orders']`` order, normalize_total(1e4) + log1p
    on the device with ``normalize``), then sorted by ``col`` with numpy's quicksort as the reference's sort_values does.  The
    mean curve's fit (``_fit_best_model_``, pval_thr 1) is ``engine.trajectory_fits(model="huber", pval_thr=1)``; each side's
    ``n_bootstraps`` Huber fits regress the expression, in its own order, on resampled times (only x is resampled, as in the
    reference) and run on the device (``engine.bootstrap_huber_fits``).  Every fit is the optimum of HuberRegressor's objective,
    which scikit-learn can stop short of.  Resamples are drawn on the host in the reference's order: ``random_state=None`` uses
    numpy's global legacy stream (``np.random.seed(s)`` then this call draws what the reference draws), an int seeds a private
    ``np.random.RandomState``.  The Wald step runs on the host with the reference's numpy / scipy calls.  A row whose bootstrap
    fits did not all converge, or whose mean curve has no eligible model (the reference crashes there), gets NaN ``waldStat`` and
    ``pvalue`` and ``df`` 0 (the latter also a NaN ``FC``); ``return_info`` adds a dict with their counts and timings, each Wald
    row's mean-curve model (``table2``, its params ``table2_params``), the bootstrap betas (``boot``, rows x B x 6) and which of
    its three mean-curve fits were flagged not converged (ineligible).  The mean
    curve is a polynomial of degree <= 2, so linear_quadratic (and often another model) fits it exactly: the choice among exact
    fits follows K9's rule, the first of linear, linear_quadratic, quadratic on a tie, a fit flagged not converged excluded."""
    import time
    from . import _lib
    t_all = time.perf_counter()
    n_points = int(n_points)
    n_bootstraps = int(n_bootstraps)
    if n_points < 3:
        raise ValueError("n_points=%d: the mean-curve fit needs at least 3 distinct points" % n_points)
    if n_bootstraps < 2:
        raise ValueError("n_bootstraps=%d: the covariance needs at least 2 bootstraps" % n_bootstraps)
    if not (np.isfinite(start) and np.isfinite(end)) or not end > start:
        raise ValueError("start=%r, end=%r: need finite start < end" % (start, end))
    if not (fc_thr > 0 and np.isfinite(fc_thr)):
        raise ValueError("fc_thr=%r must be positive" % (fc_thr,))
    cluster_names = list(tables) if cluster_names is None else list(cluster_names)
    _gcd_check_tables(tables, cluster_names)
    if gene_list is None:
        gene_list = np.unique(np.concatenate([np.asarray(tables[c]["Gene ID"], dtype=object) for c in cluster_names])
                              if cluster_names else np.array([], dtype=object))
    gene_list = list(gene_list)
    rows_of = {c: {g: i for i, g in reversed(list(enumerate(tables[c]["Gene ID"])))} for c in cluster_names}   # first row per gene
    gene_dict = {g: [c for c in cluster_names if g in rows_of[c]] for g in gene_list}
    if random_state is None:
        rs = np.random.mtrand._rand
    elif isinstance(random_state, np.random.RandomState):
        rs = random_state
    else:
        rs = np.random.RandomState(random_state)
    l2fc = np.log2(fc_thr)
    log_fc_cutoff = np.log(np.power(2, l2fc))
    pline = np.linspace(start, end, n_points)
    orders = adata.uns["orders"]

    # the rows, in the reference's order; the cells of every cell type that has a row
    def trow(c, g):
        return tables[c].iloc[rows_of[c][g]]
    rows = []
    for g in gene_list:
        cl = gene_dict[g]
        if len(cl) == 1:
            rows.append((g, cl[0], None))
        elif len(cl) > 1:
            rows.extend((g, c, [o for o in cl if o != c]) for c in cl)
    multi = [k for k, r in enumerate(rows) if r[2] is not None]
    cells = {}
    for k in multi:
        c = rows[k][1]
        if c not in cells:
            rws, x = _cell_rows(adata, c, sample_col, col_cell, orders, col)
            key = x.astype(orders[col].dtype) if np.asarray(orders[col]).dtype.kind in "iu" else x
            o = np.argsort(key, kind="quicksort")           # data.sort_values(col): numpy's quicksort on the column
            cells[c] = dict(rows=rws[o], x=x[o], genes=[])
        if rows[k][0] not in cells[c]["genes"]:
            cells[c]["genes"].append(rows[k][0])
    for c, d in cells.items():
        if d["x"].size < 1:
            raise ValueError("cell type %r has no cells in adata.uns['orders']" % (c,))

    # curves on pline: curve1 (the row's own fit) and the mean of the others' (table2's target)
    curve1, ybar, model1 = [], [], []
    for k in multi:
        g, c, others = rows[k]
        r1 = trow(c, g)
        model1.append(r1["Fitted function"])
        curve1.append(np.matmul(_gcd_features(model1[-1], pline, False), _gcd_params(r1)))
        cs = []
        for o in others:
            ro = trow(o, g)
            cs.append(np.matmul(_gcd_features(ro["Fitted function"], pline, False), _gcd_params(ro)))
        ybar.append(np.mean(np.stack(cs), axis=0))

    # host draws, in the reference's order (per row: the cell type's n, then n_points)
    t0 = time.perf_counter()
    sizes = []
    for k in multi:
        sizes += [cells[rows[k][1]]["x"].size, n_points]
    draws = _gcd_draws(rs, sizes, n_bootstraps)
    t_draw = time.perf_counter() - t0

    # device: the mean curves' fits, then the bootstrap fits (per cell type, then all mean curves at once)
    t0 = time.perf_counter()
    R = len(multi)
    ok = np.ones(R, dtype=bool)
    no_t2 = np.zeros(R, dtype=bool)
    boot = np.full((R, n_bootstraps, 6), np.nan)
    model2 = [None] * R
    params2 = np.full((R, 3), np.nan)
    n_nc = 0
    if R:
        Ybar = np.ascontiguousarray(np.stack(ybar, axis=1))
        t2, t2_info = engine.trajectory_fits(Ybar, pline, model="huber", pval_thr=1, return_info=True)
        for j in range(R):
            ch = int(t2["chosen"][j])
            if ch < 0:
                no_t2[j] = True
                continue
            model2[j] = engine.TRAJFIT_MODELS[ch]
            params2[j] = t2["params"][j, ch]
        for c, d in cells.items():
            js = [j for j, k in enumerate(multi) if rows[k][1] == c]
            gcol = np.asarray([list(adata.var_names).index(g) for g in d["genes"]], dtype=np.int32)
            if _is_sparse(adata.X):                    # sparse: up once, normalised in HBM, the cell type's genes made dense there
                S = _sparse_rows(adata.X, d["rows"])
                if normalize:
                    S.normalize_log1p(1e4)
                Y = S.densify(gcol)
                del S
            else:
                X = _dense_rows(adata.X, d["rows"])
                if normalize:
                    Y = np.empty((X.shape[0], gcol.size), dtype=X.dtype)
                    _lib_check_normalize(X, gcol, Y)
                else:
                    Y = np.ascontiguousarray(X[:, gcol])
            pos = {g: i for i, g in enumerate(d["genes"])}
            idx = np.stack([draws[2 * j] for j in js])
            prm, inf = engine.bootstrap_huber_fits(
                Y, d["x"], [pos[rows[multi[j]][0]] for j in js], [engine.TRAJFIT_MODELS.index(model1[j]) for j in js], idx,
                return_info=True)
            for q, j in enumerate(js):
                boot[j, :, :3] = [_gcd_fill_betas(model1[j], p) for p in prm[q]]
                ok[j] &= not (inf["flags"][q] & _lib.TRAJFIT_NOT_CONVERGED).any()
            n_nc += inf["not_converged"]
        js = [j for j in range(R) if not no_t2[j]]
        if js:
            prm, inf = engine.bootstrap_huber_fits(Ybar, pline, js, [engine.TRAJFIT_MODELS.index(model2[j]) for j in js],
                                                   np.stack([draws[2 * j + 1] for j in js]), return_info=True)
            for q, j in enumerate(js):
                boot[j, :, 3:] = [_gcd_fill_betas(model2[j], p) for p in prm[q]]
                ok[j] &= not (inf["flags"][q] & _lib.TRAJFIT_NOT_CONVERGED).any()
            n_nc += inf["not_converged"]
    t_dev = time.perf_counter() - t0

    # host: the Wald step per row, then extend_stats
    t0 = time.perf_counter()
    out = []
    j_of = {k: j for j, k in enumerate(multi)}
    for k, (g, c, others) in enumerate(rows):
        if others is None:
            stat = [1.0, 1, 0.0, 0.0]
        else:
            j = j_of[k]
            if no_t2[j]:
                stat = [np.nan, 0, np.nan, np.nan]
            else:
                c2 = np.matmul(_gcd_features(model2[j], pline, False), params2[j][:3 if model2[j] == "linear_quadratic" else 2])
                with np.errstate(divide="ignore", invalid="ignore"):
                    fc = float(np.log2(curve1[j].mean()) - np.log2(c2.mean()))
                if not ok[j]:
                    stat = [np.nan, 0, np.nan, fc]
                else:
                    betas = _gcd_fill_betas(model1[j], _gcd_params(trow(c, g))) + _gcd_fill_betas(model2[j], params2[j])
                    w, r, pv = _gcd_wald(_gcd_features(model1[j], pline, True), _gcd_features(model2[j], pline, True), betas,
                                         boot[j], log_fc_cutoff, eigenThresh)
                    stat = [w, r, pv, fc]
        tr = trow(c, g)
        out.append([str(g), str(c)] + stat + [tr["Expression pattern"], float(tr["adjusted P-value"]), float(tr["R-squared"]),
                                              float(tr["mod_rsquared_adj"])])
    frame = pd.DataFrame(out, columns=_GCD_COLUMNS)
    frame = frame.astype({"waldStat": np.float64, "df": np.int64, "pvalue": np.float64, "FC": np.float64,
                          "fit-pvalue": np.float64, "fit-rsquared": np.float64, "fit-mod-rsquared": np.float64})
    t_host = time.perf_counter() - t0
    if not return_info:
        return frame
    info = dict(rows=len(rows), wald_rows=R, not_converged_rows=int((~ok & ~no_t2).sum()), no_table2_rows=int(no_t2.sum()),
                not_converged_fits=int(n_nc), draw_s=t_draw, device_s=t_dev, wald_s=t_host,
                total_s=time.perf_counter() - t_all, table2=list(model2), table2_params=params2, boot=boot,
                table2_not_converged=(t2_info["flags"] & _lib.TRAJFIT_NOT_CONVERGED).astype(bool) if R else np.zeros((0, 3), bool))
    return frame, info


def _gcd_select_genes(tables, cellnames, sort, number_genes):
    """gene_cluster_differentiation's gene list: per cell type, its table sorted by ``sort`` (ascending True, True, False) and
    the first ``number_genes`` rows of every expression pattern; np.unique of them all."""
    genes = []
    for c in cellnames:
        sel = tables[c].sort_values(sort, ascending=[True, True, False]).groupby("Expression pattern").head(number_genes)
        genes.extend(sel["Gene ID"].tolist())
    return np.unique(genes)


def gene_cluster_differentiation(adata, tables, cellnames=(), sort=("Expression pattern", "adjusted P-value", "R-squared"),
                                 number_genes=10, gene_list=(), **kw):
    """gene_cluster_differentiation (Trajectory.py:1129-1172) without plots or files: the gene list from the ``tables`` of
    ``cellnames`` (each sorted by ``sort``, the first ``number_genes`` genes of every expression pattern), or np.unique of
    ``gene_list`` when given; start / end from min / max of ``adata.uns['orders']['Time_score']``; then
    :func:`infer_gene_cluster_differentiation` (``**kw``: its other arguments).  Returns its frame."""
    sort = list(sort)
    if len(sort) != 3:
        raise ValueError("sort=%r: three columns, sorted ascending, ascending, descending" % (sort,))
    for c in cellnames:
        if c not in tables:
            raise KeyError("cell type %r has no table in `tables`" % (c,))
    if len(gene_list) == 0:
        genes = _gcd_select_genes(tables, list(cellnames), sort, number_genes)
    else:
        genes = np.unique(list(gene_list))
    ts = adata.uns["orders"]["Time_score"]
    return infer_gene_cluster_differentiation(adata, tables, gene_list=genes, start=min(ts), end=max(ts), **kw)


# ---- gene curve clustering (plot/gene_selection_analysis.py:86-203, 360-415, 850-955; plot/curve_activity.py) ----------------
_ACTIVITY_COLUMNS = ["Terminal_logFC", "Terminal_pvalue", "Terminal_adjPvalue", "Transient_logFC", "Switching_time", "area", "cluster"]


class _Curves:
    """Standardised curves that live on the device (genes x time points) with their frame labels."""

    def __init__(self, matrix, index, columns, columns_name=None):
        self.matrix, self.index, self.columns, self.columns_name = matrix, list(index), columns, columns_name

    def frame(self):
        df = pd.DataFrame(engine.download(self.matrix), index=pd.Index(self.index, name="Gene ID"), columns=self.columns)
        df.columns.name = self.columns_name
        return df


def _noised_curves(adata, cell_type, table, filter_table_feature, filter_table_feature_pval, table_filter_thr,
                   table_filter_pval_thr, col, sample_col, col_cell, normalize):
    """get_noised_curves with its two curve matrices left on the device: (curves, noised curves, pseudotime_sample_names)"""
    rows, x = _cell_rows(adata, cell_type, sample_col, col_cell, adata.uns["orders"], col)
    if rows.size == 0:
        raise ValueError("no cells of %r in adata.uns['orders']" % (cell_type,))
    o = np.argsort(x, kind="stable")                 # cells of one time point contiguous (already so after cell_importance)
    rows, x = rows[o], x[o]
    times, first = np.unique(x, return_index=True)
    kind = np.asarray(adata.uns["orders"][col]).dtype        # the frames carry the time points in the dtype of orders[col]
    labels = times.astype(kind) if kind.kind in "iu" else times
    names = pd.DataFrame({sample_col: np.asarray(adata.obs[sample_col])[rows[first]]}, index=pd.Index(labels, name=col))
    offsets = np.r_[first, x.size].astype(np.int64)

    table = table.fillna(0)
    if "Treat2" not in table.columns:                # genes_importance drops it when no fit has three coefficients
        table = table.assign(Treat2=0.0)
    sel = table[(np.abs(table[filter_table_feature]) >= table_filter_thr) & (table[filter_table_feature_pval] <= table_filter_pval_thr)]
    genes = list(sel["Gene ID"])
    pos = {g: i for i, g in enumerate(adata.var_names)}
    missing = [g for g in genes if g not in pos]
    if missing:
        raise KeyError("genes of the table that adata.var_names lacks: %s" % missing[:5])
    cols = np.array([pos[g] for g in genes], dtype=np.int32)
    params = sel[["Intercept", "Treat", "Treat2"]].to_numpy(dtype=np.float64).reshape(-1, 3)
    model = np.array([engine.TRAJFIT_MODELS.index(f) for f in sel["Fitted function"]], dtype=np.int32)

    if not cols.size:
        sd = None
    elif _is_sparse(adata.X):                          # sparse: up once, normalised in HBM, the table's genes made dense there
        S = _sparse_rows(adata.X, rows)
        if normalize:
            S.normalize_log1p(1e4)
        sd = engine.segment_std(S.densify(cols), offsets, device=True)
        del S
    else:
        X = _dense_rows(adata.X, rows)
        if normalize:
            Y = np.empty((X.shape[0], cols.size), dtype=X.dtype)
            _lib_check_normalize(X, cols, Y)
            sd = engine.segment_std(Y, offsets, device=True)
        else:
            sd = engine.segment_std(X, offsets, cols=cols, device=True)
    plain = engine.fitted_curves(params, model, times, device=True)
    noised = engine.fitted_curves(params, model, times, noise=sd, device=True)
    return (_Curves(plain, genes, labels), _Curves(noised, genes, list(names[sample_col]), sample_col), names)


def get_noised_curves(adata, cell_type, table, filter_table_feature="R-squared", filter_table_feature_pval="adjusted P-value",
                      table_filter_thr=0.1, table_filter_pval_thr=0.05, col="Time_score", sample_col="sampleID",
                      col_cell="cell_types", normalize=True):
    """get_noised_curves (plot/gene_selection_analysis.py:86-165) without files: ``table`` is the frame ``genes_importance``
    returned (the reference reads Markers/<cell>/Whole_expressions.csv), the cells are those of ``genes_importance``
    (``adata.uns['orders']``, normalised the same way on the device).  Rows of ``table.fillna(0)`` with
    ``|table[feature]| >= thr`` and ``table[pval] <= pthr`` are kept; each gene's fitted curve over the sorted time points of the
    cell type's cells, the same curve plus ``std(cells of the time point, ddof 1) / 10 * (Treat + Treat2 - Intercept)`` (a time
    point with one cell: the whole entry 0), both standardised per gene like StandardScaler -- all on the device
    (``engine.segment_std``, ``engine.fitted_curves``).  Returns ``(scaled_curves, scaled_noised_curves,
    pseudotime_sample_names)`` as the reference's frames.  One deviation: a table without a ``Treat2`` column (genes_importance
    drops it when no fit has three coefficients) is read as Treat2 = 0; the reference raises KeyError there."""
    curves, noised, names = _noised_curves(adata, cell_type, table, filter_table_feature, filter_table_feature_pval, table_filter_thr,
                                           table_filter_pval_thr, col, sample_col, col_cell, normalize)
    return curves.frame(), noised.frame(), names


def _curve_matrix(curves):
    """(matrix for the engine, gene ids) of a curves frame or of curves left on the device"""
    if isinstance(curves, _Curves):
        return curves.matrix, curves.index
    return np.ascontiguousarray(curves.to_numpy(dtype=np.float64)), list(curves.index)


def cluster_genes_curves(curves, cluster_method="complete", cluster_metric="correlation", scaler_value=0.65):
    """cluster_genes_curves (plot/gene_selection_analysis.py:167-203): Euclidean distances between the curves, agglomerative
    linkage and ``fcluster(Z, scaler_value * d.max(), 'distance')``; distances and linkage on the device
    (``engine.linkage_of_rows``), the flat clusters on the host (``engine.flat_clusters``).  ``cluster_metric`` is accepted and
    ignored: the reference hands scipy's ``linkage`` a condensed Euclidean ``pdist``, for which scipy ignores ``metric``.
    ``cluster_method``: complete, average, weighted or single; centroid, median and ward raise NotImplementedError.  Fewer than two
    genes: every gene gets cluster 1 (the reference's ``except ValueError`` path).  Returns a frame ``Gene ID``, ``cluster``."""
    if cluster_method in engine._LINKAGE_UNSUPPORTED:
        raise NotImplementedError("cluster_method=%r: the device linkage implements %s" % (cluster_method, ", ".join(engine.LINKAGE_METHODS)))
    if cluster_method not in engine.LINKAGE_METHODS:
        raise ValueError("Invalid method: %r" % (cluster_method,))
    M, genes = _curve_matrix(curves)
    if len(genes) < 2:
        clusters = [1] * len(genes)
    else:
        Z, dmax = engine.linkage_of_rows(M, cluster_method)
        clusters = engine.flat_clusters(Z, scaler_value * dmax)
    return pd.DataFrame({"Gene ID": genes, "cluster": clusters})


def compute_curves_activities(curves, genes_clusters, pseudotime_sample_names):
    """compute_curves_activities (plot/gene_selection_analysis.py:360-415) without files: terminal and transient logFC, switching
    time and area of every curve on the device (``engine.curve_activities``, unrounded), then on the host, in the reference's
    order: ``np.round(., 2)``, the z-score of the rounded terminal logFC, ``2 * norm.sf(|z|)`` and the reference's
    ``adjust_p_values``.  Times that are not strictly increasing, or fewer than two, raise ValueError."""
    from scipy.stats import norm, zscore
    M, genes = _curve_matrix(curves)
    raw = engine.curve_activities(M, np.asarray(pseudotime_sample_names.index, dtype=np.float64))
    out = pd.DataFrame(index=pd.Index(genes, name="Gene ID"), columns=_ACTIVITY_COLUMNS[:-1])
    out["Terminal_logFC"] = np.round(raw[:, 0], 2)
    p = norm.sf(abs(zscore(out["Terminal_logFC"]))) * 2
    out["Terminal_pvalue"] = p
    p = np.asarray(p, dtype=np.float64)              # adjust_p_values (gene_selection_analysis.py:352-358)
    by_descend = p.argsort()[::-1]
    by_orig = by_descend.argsort()
    steps = float(len(p)) / np.arange(len(p), 0, -1)
    out["Terminal_adjPvalue"] = np.minimum(1, np.minimum.accumulate(steps * p[by_descend]))[by_orig]
    out["Transient_logFC"] = np.round(raw[:, 1], 2)
    out["Switching_time"] = np.round(raw[:, 2], 2)
    out["area"] = np.round(raw[:, 3], 2)
    gc = genes_clusters.set_index(genes_clusters["Gene ID"].values)
    out["cluster"] = gc.loc[out.index, "cluster"].to_numpy()
    return out


def genes_selection_analysis(adata, cell_type, table, filter_table_feature="R-squared", filter_table_feature_pval="adjusted P-value",
                             table_filter_thr=0.05, table_filter_pval_thr=0.05, cluster_method="complete",
                             cluster_metric="correlation", scaler_value=0.4, col="Time_score", sample_col="sampleID",
                             col_cell="cell_types", normalize=True):
    """genes_selection_analysis (plot/gene_selection_analysis.py:850-955) without plots, files or enrichment:
    :func:`get_noised_curves`, then :func:`cluster_genes_curves` and :func:`compute_curves_activities` on the noised curves, which
    stay on the device between the three steps.  Returns a dict: ``curves``, ``noised_curves``, ``pseudotime_sample_names``,
    ``genes_clusters``, ``curves_activities`` (rows in the order of the filtered table)."""
    if cluster_method in engine._LINKAGE_UNSUPPORTED:
        raise NotImplementedError("cluster_method=%r: the device linkage implements %s" % (cluster_method, ", ".join(engine.LINKAGE_METHODS)))
    curves, noised, names = _noised_curves(adata, cell_type, table, filter_table_feature, filter_table_feature_pval, table_filter_thr,
                                           table_filter_pval_thr, col, sample_col, col_cell, normalize)
    genes_clusters = cluster_genes_curves(noised, cluster_method, cluster_metric, scaler_value)
    activities = compute_curves_activities(noised, genes_clusters, names)
    return dict(curves=curves.frame(), noised_curves=noised.frame(), pseudotime_sample_names=names, genes_clusters=genes_clusters,
                curves_activities=activities)


# ---- patient sub-group detection: HVG, moderated t, Welch t (tools/patients_sub_clustering.py:15-240, plot/ploting.py:460-556) --
_DE_DESIGNS = ("reference", "two_group")


def highly_variable_genes(X, n_top_genes=2000):
    """scanpy's ``pp.highly_variable_genes(flavor='seurat')`` for one batch, restated (scanpy is not installed where this
    library is built and tested, so the rule is UNPINNED here, like ``normalize_total``).  ``X``: the cells x genes log1p values, a
    C-contiguous float32 / float64 array, an ``engine.DeviceMatrix`` or an ``engine.DeviceCSR``.  Mean and ddof-1 variance of ``expm1(X)`` per gene come
    from one device pass (``engine.group_moments``); the tail is scanpy's, on the host with pandas: a mean of 0 becomes 1e-12,
    dispersion = var / mean with 0 -> NaN, then its log; log1p of the mean; ``pd.cut`` of the means into 20 bins; per bin the mean
    and ddof-1 std of the dispersions, a one-gene bin getting std = its mean and mean = 0; the normalised dispersion; the cut-off
    is the ``n_top_genes``-th largest non-NaN value (all of them when there are fewer) and a gene is selected when
    ``nan_to_num(value) >= cutoff``.  Returns a frame (one row per gene, in gene order) with ``means``, ``dispersions``,
    ``dispersions_norm``, ``highly_variable``."""
    n_top_genes = int(n_top_genes)
    if n_top_genes < 1:
        raise ValueError("n_top_genes=%d must be positive" % n_top_genes)
    n = X.shape[0]
    count, mean, m2 = engine.group_moments(X, np.zeros(n, dtype=np.int32), 1, transform="expm1")
    with np.errstate(divide="ignore", invalid="ignore"):
        mean, var = mean[0].copy(), m2[0] / (n - 1.0)
        mean[mean == 0] = 1e-12
        dispersion = var / mean
        dispersion[dispersion == 0] = np.nan
        dispersion = np.log(dispersion)
        mean = np.log1p(mean)
    df = pd.DataFrame({"means": mean, "dispersions": dispersion})
    df["mean_bin"] = pd.cut(df["means"], bins=20)
    grouped = df.groupby("mean_bin", observed=False)["dispersions"]
    bin_mean, bin_std = grouped.mean(), grouped.std(ddof=1)
    single = bin_std.isnull()
    bin_std[single] = bin_mean[single].values
    bin_mean[single] = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = (df["dispersions"].values - bin_mean[df["mean_bin"]].values) / bin_std[df["mean_bin"]].values
    ranked = np.sort(norm[~np.isnan(norm)])[::-1]
    if ranked.size == 0:
        raise ValueError("highly_variable_genes: no gene has a finite normalised dispersion")
    cutoff = ranked[min(n_top_genes, ranked.size) - 1]
    return pd.DataFrame({"means": mean, "dispersions": dispersion, "dispersions_norm": norm,
                         "highly_variable": np.nan_to_num(norm) >= cutoff})


def _cell_type_rows(adata, col_cell, cell):
    return np.flatnonzero(np.asarray(adata.obs[col_cell].isin([cell])))


def _cell_type_matrix(adata, rows, normalization):
    """The rows ``rows`` of adata.X on the device, optionally normalize_total(1e4) + log1p: a sparse adata.X as an
    ``engine.DeviceCSR`` (normalised in place there), a dense one as an ``engine.DeviceMatrix`` of :func:`_cell_type_values`"""
    if _is_sparse(adata.X):
        S = _sparse_rows(adata.X, rows)
        if normalization and S.nnz:
            S.normalize_log1p(1e4)
        return S
    return engine.DeviceMatrix.upload(_cell_type_values(adata, rows, normalization))


def _cell_type_values(adata, rows, normalization):
    """The rows ``rows`` of the dense adata.X as a float32 / float64 array, optionally normalize_total(1e4) + log1p on the device"""
    X = _dense_rows(adata.X, rows)
    if normalization and X.size:
        out = np.empty_like(X)
        _lib_check_normalize(X, np.arange(X.shape[1], dtype=np.int32), out)
        X = out
    return X


def extract_cells_from_gene_expression_for_clustering(adata, sample_col, col_cell, cell_list, normalization=True, n_top_genes=2000,
                                                      highly_variable_genes_=False):
    """extract_cells_from_gene_expression_for_clustering (tools/patients_sub_clustering.py:15-76) without the CSV file: the
    expression frame of the FIRST cell type of ``cell_list`` (the reference returns inside its loop) -- one row per cell, one
    column per gene (every gene, or the highly variable ones of :func:`highly_variable_genes` in gene order) plus ``sampleID``.
    ``normalization``: normalize_total(1e4) + log1p on the device (``pilot_ot_normalize_log1p``).  A scipy sparse ``adata.X`` goes
    up as an ``engine.DeviceCSR``: normalisation and the HVG moments run on the sparse form in HBM, and only the columns of the
    frame are made dense and downloaded."""
    if len(cell_list) < 1:
        raise ValueError("cell_list is empty")
    rows = _cell_type_rows(adata, col_cell, cell_list[0])
    genes = np.asarray(list(adata.var_names), dtype=object)
    if _is_sparse(adata.X):
        S = _cell_type_matrix(adata, rows, normalization)
        keep = None
        if highly_variable_genes_:
            keep = np.flatnonzero(highly_variable_genes(S, n_top_genes)["highly_variable"].values)
            genes = genes[keep]
        X = engine.download(S.densify(keep))           # the one dense copy: the frame this returns
        del S
    else:
        X = _cell_type_values(adata, rows, normalization)
        if highly_variable_genes_:
            keep = np.flatnonzero(highly_variable_genes(X, n_top_genes)["highly_variable"].values)
            X, genes = X[:, keep], genes[keep]
    df = pd.DataFrame(X, columns=list(genes))
    df["sampleID"] = list(np.asarray(adata.obs[sample_col])[rows])
    return df


def _sample_labels(proportions, label_name):
    """sample id -> sub-group label of a proportions frame: ids from its 'sampIeD' column (sic, the reference's name), else
    'sampleID', else the index"""
    ids = proportions["sampIeD"] if "sampIeD" in proportions.columns else \
        proportions["sampleID"] if "sampleID" in proportions.columns else proportions.index
    return dict(zip(list(ids), list(proportions[label_name])))


def _trigamma_inverse(x):
    """limma's trigammaInverse for one positive value: Newton on 1 / trigamma from 0.5 + 1 / x, at most 50 steps"""
    from scipy.special import polygamma
    if x > 1e7:
        return 1.0 / np.sqrt(x)
    if x < 1e-6:
        return 1.0 / x
    y = 0.5 + 1.0 / x
    for _ in range(50):
        tri = float(polygamma(1, y))
        dif = tri * (1.0 - tri / x) / float(polygamma(2, y))
        y += dif
        if -dif / y < 1e-8:
            break
    return y


def _ebayes_prior(s2, df):
    """limma's fitFDist for one residual df: (s0^2, df0) from the per-gene variances"""
    from scipy.special import digamma, polygamma
    med = np.median(s2)
    if not med > 0:
        raise ValueError("compute_diff_expressions: the median residual variance is %g; the prior cannot be estimated" % med)
    e = np.log(np.maximum(s2, 1e-5 * med)) - digamma(df / 2.0) + np.log(df / 2.0)
    emean = e.mean()
    evar = e.var(ddof=1) - float(polygamma(1, df / 2.0)) if e.size > 1 else np.nan
    if evar > 0:
        df0 = 2.0 * _trigamma_inverse(evar)
        return float(np.exp(emean + digamma(df0 / 2.0) - np.log(df0 / 2.0))), df0
    return float(np.exp(emean)), np.inf


def _two_group_fit(count, mean, m2, design, first):
    """lmFit's results for two groups from their moments (count: 2; mean, m2: 2 x genes; group 0 is group1):
    (logFC, AveExpr, RSS, residual df, unscaled stdev).  ``design='reference'``: ONE column x = 1 for group ``first`` and 2 for the
    other, beta = (S_a + 2 S_b) / (n_a + 4 n_b), RSS = m2_a + m2_b + n_a (m_a - beta)^2 + n_b (m_b - 2 beta)^2, df = n - 1;
    ``'two_group'``: intercept + indicator of group1, logFC = m_1 - m_2, RSS = m2_1 + m2_2, df = n - 2."""
    n1, n2 = float(count[0]), float(count[1])
    n = n1 + n2
    ave = (n1 * mean[0] + n2 * mean[1]) / n
    if design == "reference":
        a, b = first, 1 - first
        na, nb = float(count[a]), float(count[b])
        xtx = na + 4.0 * nb
        logfc = (na * mean[a] + 2.0 * nb * mean[b]) / xtx
        rss = m2[a] + m2[b] + na * (mean[a] - logfc) ** 2 + nb * (mean[b] - 2.0 * logfc) ** 2
        return logfc, ave, rss, n - 1.0, xtx ** -0.5
    return mean[0] - mean[1], ave, m2[0] + m2[1], n - 2.0, np.sqrt(1.0 / n1 + 1.0 / n2)


def _subgroup_selection(who, adata, cell_type, proportions, selected_genes, groups, label_name, sample_col, col_cell, normalization,
                        n_top_genes, highly_variable_genes_):
    """The cell, label and gene selection of the sub-group comparisons (``who`` names the caller in the errors): the cells of
    ``cell_type`` take the ``label_name`` of their sample in ``proportions`` and the code of that label's position in ``groups``
    (-1: another label, left out; ``groups=None``: every label that occurs, sorted); the matrix goes up once
    (:func:`_cell_type_matrix`), the highly variable genes are taken over ALL the cell type's cells and ``selected_genes``
    restricts and orders them.  Every check that needs no device comes before the upload.  Returns
    ``(matrix, codes int32, cols, gene names, group names)``."""
    genes = np.asarray(list(adata.var_names), dtype=object)
    if selected_genes is not None:
        pos = {g: i for i, g in enumerate(genes)}
        unknown = [g for g in selected_genes if g not in pos]
        if unknown:
            raise KeyError("%s: selected_genes not in adata.var_names: %s" % (who, unknown))
    label_of = _sample_labels(proportions, label_name)
    rows = _cell_type_rows(adata, col_cell, cell_type)
    samples = np.asarray(adata.obs[sample_col])[rows]
    missing = [s for s in pd.unique(samples) if s not in label_of]
    if missing:
        raise KeyError("%s: samples of %r missing from proportions: %s" % (who, cell_type, missing))
    labels = np.asarray([label_of[s] for s in samples], dtype=object)
    if groups is None:
        groups = sorted(pd.unique(labels), key=str)
        if len(groups) < 2:
            raise ValueError("%s: the cells of %r carry one label, %s" % (who, cell_type, groups))
    codes = np.full(labels.size, -1, dtype=np.int32)
    for g, name in enumerate(groups):                      # (the callers refuse a name given twice)
        codes[labels == name] = g
        if not (codes == g).any():
            raise ValueError("%s: group %r has no cells of %r" % (who, name, cell_type))

    D = _cell_type_matrix(adata, rows, normalization)
    cols = np.arange(genes.size)
    if highly_variable_genes_:
        cols = np.flatnonzero(highly_variable_genes(D, n_top_genes)["highly_variable"].values)
    if selected_genes is not None:
        among = set(cols.tolist())
        outside = [g for g in selected_genes if pos[g] not in among]
        if outside:
            raise KeyError("%s: selected_genes outside the highly variable genes: %s" % (who, outside))
        cols = np.asarray([pos[g] for g in selected_genes], dtype=np.int64)
    return D, codes, cols, genes, list(groups)


def compute_diff_expressions(adata, cell_type, proportions, selected_genes=None, group1="Tumor 1", group2="Tumor 2",
                             label_name="Predicted_Labels", sample_col="sampleID", col_cell="cell_types", normalization=False,
                             n_top_genes=2000, highly_variable_genes_=True, design="reference"):
    """compute_diff_expressions (tools/patients_sub_clustering.py:77-240) without R, plots or files: limma's ``lmFit`` ->
    ``eBayes`` -> ``topTable`` for the cells of ``cell_type`` in two patient sub-groups, from per-gene, per-group count, mean and
    centred sum of squares taken in one device pass (``engine.group_moments``); the O(genes) tail runs on the host.  limma is not
    installed where this library is built and tested, so its arithmetic is restated and UNPINNED here.

    The cells of ``cell_type`` are optionally normalised, uploaded once (a dense ``adata.X`` as an ``engine.DeviceMatrix``; a
    scipy sparse one as an ``engine.DeviceCSR``, normalised in HBM, whose column form serves both moment calls: nothing dense is
    ever formed), reduced to the highly variable genes over ALL the cell type's cells (:func:`highly_variable_genes`) as the reference does, and each cell takes the
    ``label_name`` of its sample in ``proportions`` (sample ids from its ``sampIeD`` column -- sic -- else ``sampleID``, else the
    index); cells of other labels are left out.  ``selected_genes`` restricts (and orders) the genes.

    ``design='reference'`` is what the reference's call computes: ``design = unclass(as.factor(labels))`` is ONE column x in
    {1, 2}, 1 for the name that sorts first (Python's string ordering here; R's locale collation can order mixed-case names
    differently).  That is a regression through the origin, not a group contrast: logFC = beta = (S1 + 2 S2) / (n1 + 4 n2),
    RSS = m2_1 + m2_2 + n1 (m1 - beta)^2 + n2 (m2 - 2 beta)^2, df = n - 1, unscaled stdev (n1 + 4 n2)^-1/2.
    ``design='two_group'`` (not in PILOT) is an intercept plus an indicator: logFC = mean(group1) - mean(group2), positive =
    higher in group1 as in :func:`cell_type_diff_two_sub_patient_groups`; RSS = m2_1 + m2_2, df = n - 2, unscaled stdev
    sqrt(1 / n1 + 1 / n2).

    eBayes: s^2 = RSS / df; e = log s^2 - digamma(df / 2) + log(df / 2) with zero variances floored at 1e-5 median(s^2) for the
    prior only (median 0: ValueError); evar = var(e, ddof 1) - trigamma(df / 2); evar > 0: df0 = 2 trigammaInverse(evar) (limma's
    Newton iteration), s0^2 = exp(mean(e) + digamma(df0 / 2) - log(df0 / 2)), else df0 = inf, s0^2 = exp(mean(e)); posterior
    variance (df0 s0^2 + df s^2) / (df0 + df); t = logFC / (unscaled stdev * posterior sd); total df = min(df + df0, G df);
    two-sided p; Benjamini-Hochberg.

    Returns a frame indexed by gene, in gene order: ``logFC``, ``AveExpr`` (mean over the selected cells), ``t``, ``P.Value``,
    ``adj.P.Val``; ``attrs['df_prior']``, ``attrs['s2_prior']``.  Deviations from the reference: no ``B`` column; every gene is
    returned (the reference's ``topTable(n=2000)`` leaves genes beyond 2 000 as NaN); the reference's ``cells.iloc[:, 1:-1]``
    silently drops the first gene, this does not.  Raised before any device work: ValueError for an unknown ``design`` or a group
    without cells (named), KeyError for a sample of the cell type that ``proportions`` lacks."""
    from scipy import stats
    if design not in _DE_DESIGNS:
        raise ValueError("design=%r must be one of %s" % (design, ", ".join(map(repr, _DE_DESIGNS))))
    if group1 == group2:
        raise ValueError("group1 and group2 are both %r" % (group1,))
    D, codes, cols, genes, _ = _subgroup_selection("compute_diff_expressions", adata, cell_type, proportions, selected_genes, (group1, group2),
                                                   label_name, sample_col, col_cell, normalization, n_top_genes, highly_variable_genes_)
    count, mean, m2 = engine.group_moments(D, codes, 2, cols=_selected_or_every(cols, genes.size))
    del D

    G = cols.size
    logfc, ave, rss, df, unscaled = _two_group_fit(count, mean, m2, design, 0 if str(group1) < str(group2) else 1)
    if df < 1:
        raise ValueError("compute_diff_expressions: %d cells leave no residual degrees of freedom" % int(count.sum()))
    s2 = rss / df
    s2_prior, df_prior = _ebayes_prior(s2, df)
    s2_post = np.full(G, s2_prior) if np.isinf(df_prior) else (df_prior * s2_prior + df * s2) / (df_prior + df)
    t = logfc / (unscaled * np.sqrt(s2_post))
    df_total = min(df + df_prior, G * df)
    p = 2.0 * (stats.norm.sf(np.abs(t)) if np.isinf(df_total) else stats.t.sf(np.abs(t), df_total))
    res = pd.DataFrame({"logFC": logfc, "AveExpr": ave, "t": t, "P.Value": p, "adj.P.Val": _bh_adjust(p)},
                       index=pd.Index(genes[cols], name="gene"))
    res.attrs["df_prior"], res.attrs["s2_prior"] = float(df_prior), float(s2_prior)
    return res


def _selected_or_every(cols, n_vars):
    """None when ``cols`` is every column in order (the calls then take their contiguous reads), else ``cols`` as int32"""
    every = cols.size == n_vars and np.array_equal(cols, np.arange(n_vars))
    return None if every else cols.astype(np.int32)


def wilcoxon_diff_expressions(adata, cell_type, proportions, selected_genes=None, group1="Tumor 1", group2="Tumor 2",
                              label_name="Predicted_Labels", sample_col="sampleID", col_cell="cell_types", normalization=False,
                              n_top_genes=2000, highly_variable_genes_=True, tie_correct=True):
    """The non-parametric companion of :func:`compute_diff_expressions`: per gene, the Wilcoxon rank-sum (Mann-Whitney) test of
    the cells of ``cell_type`` in sub-group ``group1`` against those in ``group2``, with the same cell, label and gene selection.
    The ranks are taken on the device among the cells of the two groups (``engine.rank_sums``), the means come from
    ``engine.group_sums``, and the tail is ``engine.rank_sum_z``: with ``tie_correct`` (the default here) U, z and the p-value
    are those of ``scipy.stats.mannwhitneyu(x1, x2, use_continuity=False, method="asymptotic")``.  A gene whose values are all
    equal has z = 0, p = 1.  Returns a frame indexed by gene, in gene order: ``logFC`` (mean of group1 - mean of group2),
    ``AveExpr``, ``U`` (of group1), ``z`` (positive: higher in group1), ``P.Value``, ``adj.P.Val`` (Benjamini-Hochberg).  Raised
    before any device work: ValueError for equal group names or a group without cells, KeyError as
    :func:`compute_diff_expressions`."""
    from scipy import stats
    if group1 == group2:
        raise ValueError("group1 and group2 are both %r" % (group1,))
    D, codes, cols, genes, _ = _subgroup_selection("wilcoxon_diff_expressions", adata, cell_type, proportions, selected_genes, (group1, group2),
                                                   label_name, sample_col, col_cell, normalization, n_top_genes, highly_variable_genes_)
    sel = _selected_or_every(cols, genes.size)
    count, R, ties = engine.rank_sums(D, codes, 2, cols=sel)
    sums = engine.group_sums(D, codes, 2, cols=sel)[1]
    del D
    n = count.astype(np.float64)[:, None]
    mean = sums / n
    z, U = engine.rank_sum_z(count, R, ties, tie_correct=tie_correct)
    p = 2.0 * stats.norm.sf(np.abs(z[0]))
    return pd.DataFrame({"logFC": mean[0] - mean[1], "AveExpr": (n[0] * mean[0] + n[1] * mean[1]) / n.sum(), "U": U[0], "z": z[0],
                         "P.Value": p, "adj.P.Val": _bh_adjust(p)}, index=pd.Index(genes[cols], name="gene"))


def kruskal_diff_expressions(adata, cell_type, proportions, groups=None, selected_genes=None, label_name="Predicted_Labels",
                             sample_col="sampleID", col_cell="cell_types", normalization=False, n_top_genes=2000,
                             highly_variable_genes_=True):
    """The Kruskal-Wallis test, per gene, of the cells of ``cell_type`` over the patient sub-groups ``groups`` (default: every
    label of ``label_name`` that a sample of the cell type carries, sorted) -- what :func:`clustering_emd` returns is often three
    or more sub-groups, which the two-group tests cannot take at once.  Selection as :func:`compute_diff_expressions`; the ranks
    among the cells of those groups come from ``engine.rank_sums``, H and its chi-square p-value from ``engine.kruskal_h``: the
    values of ``scipy.stats.kruskal``.  A gene whose values are all equal has H = p = NaN, as in scipy, and is left out of the
    Benjamini-Hochberg adjustment.  Returns a frame indexed by gene, in gene order: ``H``, ``df``, ``P.Value``, ``adj.P.Val`` and
    one column ``mean(<group>)`` per group.  Raised before any device work: ValueError for fewer than two groups, a group named
    twice or a group without cells, KeyError as :func:`compute_diff_expressions`."""
    if groups is not None:
        groups = list(groups)
        if len(set(groups)) != len(groups):
            raise ValueError("kruskal_diff_expressions: a group is named twice in %s" % (groups,))
        if len(groups) < 2:
            raise ValueError("kruskal_diff_expressions: %d group(s); the test compares at least two" % len(groups))
    D, codes, cols, genes, groups = _subgroup_selection("kruskal_diff_expressions", adata, cell_type, proportions, selected_genes, groups,
                                                        label_name, sample_col, col_cell, normalization, n_top_genes, highly_variable_genes_)
    sel =_selected_or_every(cols, genes.size)
    count, R, ties = engine.rank_sums(D, codes, len(groups), cols=sel)
    sums = engine.group_sums(D, codes, len(groups), cols=sel)[1]
    del D
    H, p, df = engine.kruskal_h(count, R, ties)
    adj = np.full(p.size, np.nan)
    adj[np.isfinite(p)] = _bh_adjust(p[np.isfinite(p)])
    out = {"H": H, "df": np.full(p.size, df, dtype=np.int64), "P.Value": p, "adj.P.Val": adj}
    for g, name in enumerate(groups):
        out["mean(%s)" % (name,)] = sums[g] / float(count[g])
    return pd.DataFrame(out, index=pd.Index(genes[cols], name="gene"))


_RGG_CORRECTIONS = ("benjamini-hochberg", "bonferroni")


def rank_genes_groups(adata, groupby, groups="all", reference="rest", n_genes=None, method="wilcoxon", tie_correct=False,
                      corr_method="benjamini-hochberg", genes=None, key_added=None):
    """scanpy's ``tl.rank_genes_groups(method="wilcoxon")`` on the device: the marker genes of every group of
    ``adata.obs[groupby]`` -- what names the clusters ``"0" .. "k-1"`` of :func:`louvain`, :func:`leiden` and
    :func:`reclustering_data`.  Reads ``adata.X`` (dense, or scipy sparse: uploaded once as an ``engine.DeviceCSR`` and never made
    dense); ``.raw`` is left alone.  scanpy is not installed where this library is built and tested, so the layout of the result
    is UNPINNED; the statistic is pinned to scipy.

    ``reference="rest"``: one ``engine.rank_sums`` call over all cells gives the rank-sum z of every group against all other
    cells.  ``reference=<group>``: one call per tested group, the ranks taken among the cells of the two groups only.  The score
    is z (``engine.rank_sum_z``; ``tie_correct`` as scanpy's, off by default), ``pvals = 2 norm.sf(|z|)``, ``pvals_adj`` is
    Benjamini-Hochberg over the genes tested or ``min(p * genes tested, 1)`` for ``corr_method="bonferroni"``, and
    ``logfoldchanges = log2((expm1(mean_group) + 1e-9) / (expm1(mean_other) + 1e-9))`` with the means from
    ``engine.group_sums`` (log1p data, as scanpy assumes).  ``groups``: ``"all"`` (every group that has cells) or a list of
    names; ``genes``: names or a boolean mask (default: all); per group the genes come in descending score, equal scores in
    gene order, and the first ``n_genes`` are kept (default: all).

    Writes ``adata.uns[key_added or "rank_genes_groups"]``: ``params`` and the record arrays ``names`` (object), ``scores``
    (float32), ``pvals``, ``pvals_adj`` (float64), ``logfoldchanges`` (float32), one field per tested group.  Returns the tidy
    frame ``group, names, scores, pvals, pvals_adj, logfoldchanges``.  ValueError before any device work: another ``method`` or
    ``corr_method``, a missing ``groupby``, an unknown group or reference, a group without cells, nothing left to test."""
    from scipy import stats
    if method != "wilcoxon":
        raise ValueError("rank_genes_groups: method=%r is not implemented, only 'wilcoxon'" % (method,))
    if corr_method not in _RGG_CORRECTIONS:
        raise ValueError("rank_genes_groups: corr_method=%r must be one of %s" % (corr_method, ", ".join(map(repr, _RGG_CORRECTIONS))))
    if groupby not in adata.obs:
        raise ValueError("rank_genes_groups: adata.obs has no column %r" % (groupby,))
    if n_genes is not None and int(n_genes) < 1:
        raise ValueError("rank_genes_groups: n_genes=%r must be positive" % (n_genes,))
    labels = pd.Series(np.asarray(adata.obs[groupby])).astype("category") if not isinstance(adata.obs[groupby].dtype, pd.CategoricalDtype) \
        else adata.obs[groupby]
    names = [str(c) for c in labels.cat.categories]
    cat = np.asarray(labels.cat.codes, dtype=np.int32)
    sizes = np.bincount(cat[cat >= 0], minlength=len(names))
    if len(names) > engine.RANK_SUMS_MAX_GROUPS:
        raise ValueError("rank_genes_groups: %d groups in %r, at most %d" % (len(names), groupby, engine.RANK_SUMS_MAX_GROUPS))
    index = {name: g for g, name in enumerate(names)}
    if isinstance(groups, str) and groups == "all":
        tested = [g for g in range(len(names)) if sizes[g] > 0]
    else:
        if isinstance(groups, (str, int)):
            raise ValueError("rank_genes_groups: groups=%r must be 'all' or a list of group names" % (groups,))
        unknown = [str(g) for g in groups if str(g) not in index]
        if unknown:
            raise ValueError("rank_genes_groups: groups not in adata.obs[%r]: %s" % (groupby, unknown))
        tested = list(dict.fromkeys(index[str(g)] for g in groups))
    ref = None
    if reference != "rest":
        if str(reference) not in index:
            raise ValueError("rank_genes_groups: reference=%r is not a group of adata.obs[%r]" % (reference, groupby))
        ref = index[str(reference)]
        tested = [g for g in tested if g != ref]
    empty = [names[g] for g in tested + ([] if ref is None else [ref]) if sizes[g] == 0]
    if empty:
        raise ValueError("rank_genes_groups: groups without cells: %s" % empty)
    if not tested:
        raise ValueError("rank_genes_groups: nothing to test (groups=%r, reference=%r)" % (groups, reference))
    if ref is None and any(sizes[g] == sizes.sum() for g in tested):
        raise ValueError("rank_genes_groups: one group holds every cell, there is no rest to test it against")
    X = adata.X
    n_vars = X.shape[1]
    cols = _gene_columns(adata, genes, n_vars)
    var_names = np.asarray(list(adata.var_names), dtype=object)
    tested_genes = var_names if cols is None else var_names[cols]
    G = tested_genes.size
    keep = G if n_genes is None else min(int(n_genes), G)

    Y = _sparse_rows(X, None) if _is_sparse(X) else engine.DeviceMatrix.upload(_dense_rows(X, slice(None)))
    K = len(names)
    sums = engine.group_sums(Y, cat, K, cols=cols)[1]
    n = sizes.astype(np.float64)
    if ref is None:
        count, R, ties = engine.rank_sums(Y, cat, K, cols=cols)
        z_all = engine.rank_sum_z(count, R, ties, tie_correct=tie_correct)[0]
        total = sums.sum(axis=0)
    out = {k: [] for k in ("names", "scores", "pvals", "pvals_adj", "logfoldchanges")}
    for g in tested:
        if ref is None:
            z = z_all[g]
            mean_other = (total - sums[g]) / (n.sum() - n[g])
        else:
            two = np.where(cat == g, 0, np.where(cat == ref, 1, -1)).astype(np.int32)
            z = engine.rank_sum_z(*engine.rank_sums(Y, two, 2, cols=cols), tie_correct=tie_correct)[0][0]
            mean_other = sums[ref] / n[ref]
        p = 2.0 * stats.norm.sf(np.abs(z))
        adj = _bh_adjust(p) if corr_method == "benjamini-hochberg" else np.minimum(p * G, 1.0)
        lfc = np.log2((np.expm1(sums[g] / n[g]) + 1e-9) / (np.expm1(mean_other) + 1e-9))
        order = np.argsort(-z, kind="stable")[:keep]
        out["names"].append(tested_genes[order])
        out["scores"].append(z[order].astype(np.float32))
        out["pvals"].append(p[order])
        out["pvals_adj"].append(adj[order])
        out["logfoldchanges"].append(lfc[order].astype(np.float32))
    del Y
    fields = [names[g] for g in tested]
    kinds = {"names": "O", "scores": "float32", "pvals": "float64", "pvals_adj": "float64", "logfoldchanges": "float32"}
    result = {"params": {"groupby": groupby, "reference": reference, "method": method, "use_raw": False, "layer": None,
                         "corr_method": corr_method, "tie_correct": bool(tie_correct)}}
    for k, arrays in out.items():
        result[k] = np.rec.fromarrays(arrays, dtype=[(f, kinds[k]) for f in fields])
    adata.uns[key_added or "rank_genes_groups"] = result
    frame = {"group": np.repeat(np.asarray(fields, dtype=object), keep)}
    for k, arrays in out.items():
        frame[k] = np.concatenate(arrays)
    return pd.DataFrame(frame)


def cell_type_diff_two_sub_patient_groups(proportions, cell_types, labels="Predicted_Labels", group1="Tumor 1", group2="Tumor 2"):
    """cell_type_diff_two_sub_patient_groups (plot/ploting.py:460-556) without the plot, the CSV file or the p-value filter:
    Welch's t-test per cell type on the proportions of the samples labelled ``group1`` against ``group2`` (``labels``: the
    column of sub-group labels; the reference reads 'Predicted_Labels' whatever its own argument says).  Group means and centred
    sums of squares of the samples x cell-types columns come from ``engine.group_moments``; the statistic, the Satterthwaite
    degrees of freedom and the two-sided p-value are formed on the host, the p-values Benjamini-Hochberg adjusted.  Returns the
    reference's unfiltered table ``cell_type``, ``adjPval``, ``-logPval``, ``score`` (positive: higher in ``group1``), sorted by
    ``score`` then ``-logPval``, both descending."""
    from scipy import stats
    cell_types = list(cell_types)
    lab = np.asarray(proportions[labels], dtype=object)
    codes = np.where(lab == group1, 0, np.where(lab == group2, 1, -1)).astype(np.int32)
    for g, name in enumerate((group1, group2)):
        if not (codes == g).any():
            raise ValueError("cell_type_diff_two_sub_patient_groups: group %r has no samples" % (name,))
    P = np.ascontiguousarray(proportions[cell_types].to_numpy(dtype=np.float64))
    count, mean, m2 = engine.group_moments(P, codes, 2)
    n1, n2 = float(count[0]), float(count[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        v1, v2 = m2[0] / (n1 - 1.0) / n1, m2[1] / (n2 - 1.0) / n2
        score = (mean[0] - mean[1]) / np.sqrt(v1 + v2)
        dof = (v1 + v2) ** 2 / (v1 ** 2 / (n1 - 1.0) + v2 ** 2 / (n2 - 1.0))
        adj = _bh_adjust(2.0 * stats.t.sf(np.abs(score), dof))
        out = pd.DataFrame({"cell_type": cell_types, "adjPval": adj, "-logPval": -np.log(adj), "score": score})
    return out.sort_values(by=["score", "-logPval"], ascending=[False, False])


# ---- pseudobulk counts: per-sample gene sums, size factors (plot/pseudobulk_DE_analysis.py:590-610) -----------------------------
def _pseudobulk_matrix(adata, rows):
    """adata.X (its rows ``rows``, or all of them) for ``engine.group_sums``: a sparse one as an ``engine.DeviceCSR``, a dense one
    as a C-contiguous float32 / float64 array (other dtypes become float64, which holds every integer count below 2^53)"""
    if _is_sparse(adata.X):
        return _sparse_rows(adata.X, rows)
    X = np.asarray(adata.X if rows is None else adata.X[rows])
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    return np.ascontiguousarray(X)


def pseudobulk_counts(adata, cell_type=None, celltype_col="cell_types", sample_col="sampleID"):
    """The aggregation that opens ``get_pseudobulk_DE`` (plot/pseudobulk_DE_analysis.py:590-597) without the dense frame:
    ``adata.to_df()`` with the two label columns, ``groupby([celltype_col, sample_col]).sum()`` -- and, with ``cell_type``, its
    ``.loc[cell_type]``.  The labels are grouped on the host as the reference groups them (the object values of the two ``obs``
    columns; observed combinations only, sorted; a cell with a missing label belongs to no group); the sums over the cells x
    genes matrix come from one device pass (``engine.group_sums``), a scipy sparse ``adata.X`` as an ``engine.DeviceCSR`` that is
    never made dense.  With ``cell_type`` only that type's cells are uploaded.

    Returns a frame of float64 sums with ``adata.var_names`` as columns, indexed by the MultiIndex ``(celltype_col, sample_col)``,
    or by the samples of ``cell_type``.  ``attrs['n_cells']``: a dict, row label -> number of cells, in row order (what
    ``plot_cell_numbers`` draws).  Deviation: the sums are float64, where the reference's float32 frames stop being exact above
    2^24.  An unknown ``cell_type`` raises ValueError before any device work."""
    labels = pd.DataFrame(adata.obs[[celltype_col, sample_col]].values, columns=[celltype_col, sample_col])
    rows = None
    if cell_type is not None:
        rows = np.flatnonzero((labels[celltype_col] == cell_type).to_numpy())
        if rows.size == 0:
            raise ValueError("pseudobulk_counts: no cell of %r in obs[%r]" % (cell_type, celltype_col))
        grouped = labels[sample_col].iloc[rows].groupby(labels[sample_col].iloc[rows], sort=True)
    else:
        grouped = labels.groupby([celltype_col, sample_col], sort=True)
    index = grouped.size().index
    if len(index) == 0:
        raise ValueError("pseudobulk_counts: no cell carries both labels")
    codes = grouped.ngroup().to_numpy().astype(np.int32)           # the rank of every cell's group in `index`, -1: a missing label
    count, sums = engine.group_sums(_pseudobulk_matrix(adata, rows), codes, len(index))
    out = pd.DataFrame(sums, index=index, columns=pd.Index(list(adata.var_names)))
    out.attrs["n_cells"] = dict(zip(index.tolist(), count.tolist()))
    return out


def _sample_constant_obs(adata, sample_col, columns, samples):
    """the ``adata.obs`` columns ``columns`` as a frame indexed by ``samples``: the one value every cell of a sample carries"""
    missing = [col for col in columns if col not in adata.obs.columns]
    if missing:
        raise ValueError("pseudobulk_inputs: obs_columns %r are not columns of adata.obs" % (missing,))
    out = {}
    for col in columns:
        per_sample = adata.obs.groupby(sample_col, observed=True)[col]
        spread = per_sample.nunique(dropna=False).reindex(samples)
        if (spread > 1).any():
            raise ValueError("pseudobulk_inputs: obs[%r] is not constant within sample %r" % (col, spread.index[(spread > 1).to_numpy()][0]))
        out[col] = per_sample.first().reindex(samples).to_numpy()
    return pd.DataFrame(out, index=samples)


def pseudobulk_inputs(adata, proportion_df, cell_type, celltype_col="cell_types", sample_col="sampleID", cluster_col="Predicted_Labels",
                      remove_samples=(), obs_columns=()):
    """``(cluster_counts, cluster_metadata)`` as ``get_pseudobulk_DE`` hands them to DESeq2 (plot/pseudobulk_DE_analysis.py:
    597-610): the samples x genes sums of ``cell_type`` (:func:`pseudobulk_counts`), the rows of ``proportion_df`` for those
    samples with the ``stage`` column (a copy of ``cluster_col``), ``remove_samples`` dropped from both, the metadata in the
    counts' order, and the genes that are zero in every remaining sample dropped.  No plots, CSV files or R: this pair is what the
    reference's ``compute_pseudobulk_DE`` takes, unchanged, and :func:`compute_pseudobulk_DE` here takes it too.  A sample of the
    cell type that ``proportion_df`` lacks raises KeyError, as in the reference.  ``obs_columns``: columns of ``adata.obs`` that are
    constant within every sample (batch, sex, age, centre: the covariates of :func:`compute_pseudobulk_DE`), copied into the metadata
    by sample; one that varies within a sample raises ValueError naming the sample.  The default returns the pair as it always was."""
    cluster_counts = pseudobulk_counts(adata, cell_type, celltype_col, sample_col)
    n_cells = cluster_counts.attrs["n_cells"]
    cluster_metadata = proportion_df.loc[cluster_counts.index.values].copy()
    cluster_metadata["stage"] = cluster_metadata[cluster_col].values
    if obs_columns is not None and len(obs_columns):
        extra = _sample_constant_obs(adata, sample_col, list(obs_columns), cluster_metadata.index)
        for col in extra.columns:
            cluster_metadata[col] = extra[col].to_numpy()
    for sample in (remove_samples if remove_samples is not None else ()):
        if sample in cluster_metadata.index:
            cluster_metadata = cluster_metadata.drop(index=sample)
        if sample in cluster_counts.index:
            cluster_counts = cluster_counts.drop(index=sample)
    cluster_metadata = cluster_metadata.loc[cluster_counts.index]
    cluster_counts = cluster_counts.loc[:, (cluster_counts != 0).any(axis=0)]
    cluster_counts.attrs["n_cells"] = {s: n_cells[s] for s in cluster_counts.index}
    return cluster_counts, cluster_metadata


def deseq2_size_factors(cluster_counts):
    """DESeq2's median-of-ratios size factors of a samples x genes count frame: ``estimateSizeFactorsForMatrix`` with its
    defaults on ``round(t(cluster_counts))``, as ``compute_pseudobulk_PCA`` / ``compute_pseudobulk_DE`` reach it through
    ``DESeqDataSetFromMatrix`` (DESeq2 is not installed where this library is built and tested, so the rule is restated and
    UNPINNED here, like limma's).  With c = rint(counts): the log geometric mean of a gene is the mean over the samples of log c,
    finite only where every sample's count is positive; a sample's factor is exp(median over those genes of log c - that mean).
    No gene with all counts positive: ValueError (DESeq2 stops there too).  The O(samples x genes) tail of the pseudobulk step, on
    the host.  Returns a Series indexed by sample."""
    c = np.rint(np.asarray(cluster_counts, dtype=np.float64))
    if c.ndim != 2:
        raise ValueError("deseq2_size_factors: a samples x genes frame, got shape %s" % (c.shape,))
    with np.errstate(divide="ignore", invalid="ignore"):
        logc = np.log(c)
        lg = logc.mean(axis=0) if c.shape[0] else np.full(c.shape[1], np.nan)
    use = np.isfinite(lg)
    if not use.any():
        raise ValueError("deseq2_size_factors: every gene contains at least one zero, cannot compute log geometric means")
    sf = np.exp(np.median(logc[:, use] - lg[use], axis=1))
    return pd.Series(sf, index=getattr(cluster_counts, "index", None))


# ---- pseudobulk differential expression: DESeq2's NB GLM for `~ stage` (plot/pseudobulk_DE_analysis.py:96-159, 628-646) ----------
def _nb_counts(cluster_counts, who):
    """the samples x genes table as a C-contiguous float32 / float64 array (the device rounds it) and its gene names"""
    c = np.asarray(cluster_counts)
    if c.ndim != 2:
        raise ValueError("%s: a samples x genes frame, got shape %s" % (who, c.shape))
    if c.dtype not in (np.float32, np.float64):
        c = c.astype(np.float64)
    names = getattr(cluster_counts, "columns", None)
    return np.ascontiguousarray(c), pd.Index(names if names is not None else np.arange(c.shape[1]))


def _estimated_or_positive(who, name, v):
    """``v`` is None (the caller estimates it) or a positive finite number that is no bool"""
    if v is not None and not (isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and np.isfinite(v) and v > 0):
        raise ValueError("%s: %s=%r must be positive and finite (None: estimated)" % (who, name, v))


def _nb_dispersion_table(c, genes, codes, k, sf, fit_type, frozen=None, design=None):
    """steps 1-5 of DESIGN.md K22 for the samples x genes array c: the frame of :func:`deseq2_dispersions`.  ``frozen``: the attrs
    of an earlier table, whose trend (``engine.nb_trend_at``) and two prior widths are used as they are instead of estimated
    (``fit_type`` is not read): the refit of DESIGN.md K25.  On the counts of that table it returns the table again, bit for bit.
    ``design``: an m x p design matrix instead of ``codes`` and ``k`` (neither is read): the same steps with the searches of
    DESIGN.md K26 (``engine.nb_design_dispersions``) and p coefficients in the prior width."""
    if design is not None:
        return _nb_table_from(c, genes, lambda **prior: engine.nb_design_dispersions(c, design, sf, **prior), design.shape[1], sf, fit_type, frozen)
    return _nb_table_from(c, genes, lambda **prior: engine.nb_dispersions(c, codes, k, sf, **prior), k, sf, fit_type, frozen)


def _nb_table_from(c, genes, search, k, sf, fit_type, frozen):
    """:func:`_nb_dispersion_table` around ``search(**prior)``, the log dispersions of the model with k coefficients"""
    m = c.shape[0]
    x_gene = search()
    q = np.rint(c.astype(np.float64)) / sf[:, None]
    base_mean, base_var = q.mean(axis=0), q.var(axis=0, ddof=1)
    base_mean[np.isnan(x_gene)] = np.nan
    base_var[np.isnan(x_gene)] = np.nan
    disp_gene = engine.nb_clip(np.exp(x_gene), m)               # (the grid's end points are the bounds up to an ulp)
    if frozen is None:
        fit, trend = engine.nb_trend(base_mean, disp_gene, fit_type)
        log_fit = np.log(fit)
        prior_var, var_log_disp = engine.nb_prior_var(x_gene, log_fit, m, k)
    else:
        trend, prior_var, var_log_disp = frozen["trend"], frozen["prior_var"], frozen["var_log_disp"]
        fit = engine.nb_trend_at(trend, base_mean)
        log_fit = np.log(fit)
    x_map = search(log_prior_mean=log_fit, prior_var=prior_var)
    with np.errstate(invalid="ignore"):
        outlier = x_gene > log_fit + 2.0 * np.sqrt(var_log_disp)
    disp_map = engine.nb_clip(np.exp(x_map), m)
    out = pd.DataFrame({"baseMean": base_mean, "baseVar": base_var, "dispGeneEst": disp_gene, "dispFit": fit, "dispMAP": disp_map,
                        "dispersion": np.where(outlier, disp_gene, disp_map), "dispOutlier": outlier}, index=genes)
    out.attrs.update(trend=trend, prior_var=prior_var, var_log_disp=var_log_disp)
    return out


def _nb_size_factors(cluster_counts, size_factors, m):
    sf = deseq2_size_factors(cluster_counts) if size_factors is None else size_factors
    sf = np.ascontiguousarray(sf, dtype=np.float64)
    if sf.shape != (m,):
        raise ValueError("size_factors has shape %s for %d samples" % (sf.shape, m))
    return sf


def deseq2_dispersions(cluster_counts, groups=None, size_factors=None, fit_type="parametric", design=None):
    """DESeq2's dispersion estimates (``estimateDispersions``; Love, Huber, Anders 2014) of a samples x genes count frame under
    the one-factor design ``~ groups`` (one label per sample; at least two groups and one residual degree of freedom), on the
    device (``engine.nb_dispersions``).  DESeq2 is not installed where this library is built and tested: the rule
    is this library's statement, UNPINNED, like limma's.  With c = rint(counts), ``size_factors`` (default
    :func:`deseq2_size_factors` of the table) and ``q = c / s``: ``baseMean`` / ``baseVar`` the mean and ddof-1 variance of q;
    ``dispGeneEst`` the maximiser of the Cox-Reid adjusted profile likelihood at the group-mean fitted values, clipped to
    [1e-8, max(10, m)]; ``dispFit`` the trend (``engine.nb_trend``: ``"parametric"`` a0 + a1 / baseMean by Gamma-GLM passes, which
    raises ValueError where DESeq2 would fall back to a local regression, or ``"mean"``); ``dispMAP`` the maximiser with the
    log-normal prior around the trend (``engine.nb_prior_var``); ``dispOutlier``: dispGeneEst more than two residual standard
    deviations above the trend, where ``dispersion`` keeps dispGeneEst, else dispMAP.  A gene of zeros has NaN everywhere (and
    dispOutlier False).  ``attrs``: ``trend`` (fit_type, coefficients, the genes of the last fit, passes), ``prior_var``,
    ``var_log_disp``.

    Deviations from DESeq2: the dispersion search is global (six rounds of a 64-point grid) where DESeq2 runs a line search from a
    moments start, so on a multimodal gene the two can differ; the Cook's-distance handling is
    :func:`compute_pseudobulk_DE`'s ``outliers="deseq2"`` (K25), which refits the genes it replaces counts in; for ``m - k <= 3`` the same
    prior-variance formula is used, where DESeq2 simulates.

    ``design``: an m x p design matrix (:func:`deseq2_design`; ``groups`` must then be None) for a model with covariates: the same
    frame by the route of DESIGN.md K26 (``engine.nb_design_dispersions``), where ``dispGeneEst`` and ``dispMAP`` maximise the
    adjusted profile likelihood with the coefficients fitted again at every dispersion, and the prior width counts p coefficients."""
    c, genes = _nb_counts(cluster_counts, "deseq2_dispersions")
    if design is not None:
        if groups is not None:
            raise ValueError("deseq2_dispersions: groups and design are given, pass one (the design has its group column)")
        X = engine._nb_design_arg(getattr(design, "values", design), c.shape[0])
        sf = _nb_size_factors(cluster_counts, size_factors, c.shape[0])
        return _nb_dispersion_table(c, genes, None, None, sf, fit_type, design=X)
    uniq, codes = np.unique(np.asarray(groups), return_inverse=True)
    codes = np.ravel(codes)
    if codes.shape != (c.shape[0],):
        raise ValueError("deseq2_dispersions: %d group labels for %d samples" % (codes.size, c.shape[0]))
    sf = _nb_size_factors(cluster_counts, size_factors, c.shape[0])
    return _nb_dispersion_table(c, genes, codes.astype(np.int32), len(uniq), sf, fit_type)


class _NBFit:
    """One fit of the two-group model: the frame of :func:`deseq2_dispersions` and, genes x groups at its final dispersions, the
    normalised means ``q``, their information ``w`` and the ``flags`` of ``engine.nb_group_fits``."""

    def __init__(self, table, q, w, flags):
        self.table, self.q, self.w, self.flags = table, q, w, flags

    def with_rows(self, rep, sub):
        """a copy with the rows of ``sub``, a fit of the genes at the positions ``rep``, written over its own"""
        table, q, w, flags = self.table.copy(), self.q.copy(), self.w.copy(), self.flags.copy()
        for j, name in enumerate(table.columns):
            table.iloc[rep, j] = sub.table[name].to_numpy()
        q[rep], w[rep], flags[rep] = sub.q, sub.w, sub.flags
        return _NBFit(table, q, w, flags)


def _nb_fit(c, genes, codes, sf, fit_type, frozen=None):
    """the :class:`_NBFit` of two groups: :func:`_nb_dispersion_table` (which reads ``frozen``) and the group fits at its dispersions"""
    table = _nb_dispersion_table(c, genes, codes, 2, sf, fit_type, frozen)
    q, w, info = engine.nb_group_fits(c, codes, 2, sf, table["dispersion"].to_numpy(), return_info=True)
    return _NBFit(table, q, w, info["flags"])


def _nb_padj(p, base_mean, filtering_alpha):
    """``padj`` of the p-values in gene order: plain BH over the genes with one, or with ``filtering_alpha``
    ``engine.independent_filtering``; ``(padj, info or None)``"""
    if filtering_alpha is not None:
        return engine.independent_filtering(p, base_mean, filtering_alpha)
    padj = np.full(p.shape, np.nan)
    ok = ~np.isnan(p)
    padj[ok] = _bh_adjust(p[ok])
    return padj, None


def _nb_wald_table(genes, fit, cooks=None, filtering_alpha=None):
    """the host tail of the Wald test: group 1 over group 0 of the :class:`_NBFit` ``fit``, rows ordered by padj (NaN last, stable).
    ``cooks``: the columns maxCooks, cooksOutlier and replace in gene order (a flagged gene loses its p-value before the
    adjustment); ``filtering_alpha``: independent filtering instead of plain BH (its info dict goes to attrs)"""
    from scipy import stats
    table, q, w = fit.table, fit.q, fit.w
    with np.errstate(divide="ignore", invalid="ignore"):
        lfc = np.log2(q[:, 1]) - np.log2(q[:, 0])                   # (as a difference: swapping the groups negates it exactly)
        se = np.log2(np.e) * np.sqrt(1.0 / w[:, 0] + 1.0 / w[:, 1])
        stat = lfc / se
    p = 2.0 * stats.norm.sf(np.abs(stat))
    if cooks is not None:
        p[cooks["cooksOutlier"]] = np.nan
    padj, filtering = _nb_padj(p, table["baseMean"].to_numpy(), filtering_alpha)
    out = pd.DataFrame({"gene": np.asarray(genes), "baseMean": table["baseMean"].to_numpy(), "log2FoldChange": lfc, "lfcSE": se,
                        "stat": stat, "pvalue": p, "padj": padj, "dispersion": table["dispersion"].to_numpy()})
    if cooks is not None:
        for name in ("maxCooks", "cooksOutlier", "replace"):
            out[name] = cooks[name]
    out = out.iloc[np.argsort(padj, kind="stable")].reset_index(drop=True)
    if filtering is not None:
        out.attrs["independent_filtering"] = filtering
    return out


_DE_OUTLIERS = (None, "deseq2")
_REPLACED_COLUMNS = ["gene", "sample", "count", "replacement"]


def _alpha_arg(who, alpha):
    if isinstance(alpha, (str, bytes, bool)) or not np.isscalar(alpha) or not 0 < alpha < 1:
        raise ValueError("%s: alpha=%r must be in (0, 1)" % (who, alpha))
    return float(alpha)


def _check_de_options(outliers, independent_filtering, alpha, who):
    if not (outliers is None or (isinstance(outliers, str) and outliers in _DE_OUTLIERS)):
        raise ValueError("%s: outliers=%r must be None or 'deseq2'" % (who, outliers))
    if not isinstance(independent_filtering, (bool, np.bool_)):
        raise ValueError("%s: independent_filtering=%r must be True or False" % (who, independent_filtering))
    _alpha_arg(who, alpha)


def _apply_replaced(c, genes, samples, replaced, who):
    """a float64 copy of rint(c) (samples x genes) with the rows of a ``replaced`` frame (gene, sample, count, replacement) written"""
    new = np.rint(np.asarray(c, dtype=np.float64))
    if replaced is None or len(replaced) == 0:
        return new
    col, row = pd.Index(genes).get_indexer(replaced["gene"]), pd.Index(samples).get_indexer(replaced["sample"])
    if (col < 0).any() or (row < 0).any():
        raise ValueError("%s: de.attrs['replaced'] names a gene or a sample that cluster_counts lacks" % who)
    if not np.array_equal(new[row, col], replaced["count"].to_numpy(dtype=np.float64)):
        raise ValueError("%s: de.attrs['replaced'] records other counts than cluster_counts holds" % who)
    new[row, col] = replaced["replacement"].to_numpy(dtype=np.float64)
    return new


def _nb_refit_max_cooks(new, codes, D, min_replace):
    """step 5 of DESIGN.md K25 for the refitted genes: the largest distance over the samples of groups with 3 <= n_g <
    min_replace (NaN without one) and how many samples have a larger count than the lowest sample that attains it"""
    size = np.bincount(codes)[codes]
    small = np.flatnonzero((size >= engine.NB_COOKS_MIN_GROUP) & (size < min_replace))
    max_cooks, n_above = np.full(new.shape[1], np.nan), np.zeros(new.shape[1], dtype=np.int32)
    if small.size:
        for j in range(new.shape[1]):
            d = D[small, j]
            if np.isnan(d).all():
                continue
            at = small[int(np.nanargmax(d))]                     # (the first largest: the lowest sample)
            max_cooks[j], n_above[j] = D[at, j], np.count_nonzero(new[:, j] > new[at, j])
    return max_cooks, n_above


def _nb_outliers(c, genes, samples, codes, sf, fit, min_replace=engine.NB_COOKS_MIN_REPLACE):
    """steps 1-6 of DESIGN.md K25 after the fit of :func:`compute_pseudobulk_DE` (``fit``, an :class:`_NBFit`): the distances,
    the replacements and the refit of the genes that had one.  Returns ``(fit, cooks, extra)``: the fit with the refitted genes'
    rows replaced (a copy), ``cooks`` the gene-order columns maxCooks / cooksOutlier / replace, ``extra`` the new attrs."""
    cutoff = engine.nb_cooks_cutoff(c.shape[0], 2)
    disp = fit.table["dispersion"].to_numpy()
    ck = engine.nb_cooks(c, codes, 2, sf, disp, fit.q, cutoff, min_replace)
    max_cooks, n_above = ck["max_cooks"].copy(), ck["n_above"].copy()
    rep = np.flatnonzero(ck["n_replace"] > 0)
    replaced = pd.DataFrame({name: [] for name in _REPLACED_COLUMNS})
    if rep.size:
        sub = np.ascontiguousarray(c[:, rep])
        ck2 = engine.nb_cooks(sub, codes, 2, sf, disp[rep], fit.q[rep], cutoff, min_replace, return_distances=True)
        rows = engine.nb_replacements(sub, codes, sf, ck2["D"], cutoff, ck2["trimmed_base"], min_replace)
        new = np.rint(sub.astype(np.float64))
        new[rows["sample"], rows["gene"]] = rows["replacement"]
        replaced = pd.DataFrame({"gene": np.asarray(genes)[rep[rows["gene"]]], "sample": np.asarray(samples)[rows["sample"]],
                                 "count": rows["count"], "replacement": rows["replacement"]})
        # the refit: the same fit of the replaced counts, the trend and both prior widths as they were
        refit = _nb_fit(new, genes[rep], codes, sf, None, frozen=fit.table.attrs)
        fit = fit.with_rows(rep, refit)
        disp = refit.table["dispersion"].to_numpy()
        live = ~np.isnan(disp)
        if live.any():
            ck3 = engine.nb_cooks(np.ascontiguousarray(new[:, live]), codes, 2, sf, disp[live], refit.q[live], cutoff, min_replace,
                                  return_distances=True)
            mc, na = _nb_refit_max_cooks(new[:, live], codes, ck3["D"], min_replace)
            max_cooks[rep[live]], n_above[rep[live]] = mc, na
        max_cooks[rep[~live]], n_above[rep[~live]] = np.nan, 0
    with np.errstate(invalid="ignore"):
        flagged = (max_cooks > cutoff) & (n_above < 3)
    replace = np.zeros(len(genes), dtype=bool)
    replace[rep] = True
    return fit, {"maxCooks": max_cooks, "cooksOutlier": flagged, "replace": replace}, {"cooks_cutoff": cutoff, "replaced": replaced}


def _check_shrink(shrink, who):
    if shrink not in (None, "apeglm"):
        raise ValueError("%s: shrink=%r must be None or 'apeglm'" % (who, shrink))


def _nb_de_intake(who, cluster_counts, groups, de, columns, attrs=(), groups_are="", both_groups=False, first=None, unless=None):
    """``(cluster_counts, groups, de)`` as :func:`lfc_shrink` and :func:`deseq2_cooks` take them apart, every refusal in ``who``'s
    name and in the order the two have always made them (which one comes first is behaviour).  ``groups_are`` ends the refusal of
    the groups in ``who``'s words; ``first()``, ``both_groups`` and ``unless()`` are the checks only one of them makes, each in its
    old place.  Returns ``(c, genes, samples, codes, sf, at, dispersion)``: the counts with ``attrs['replaced']`` applied, the
    table's labels, int32 codes, float64 size factors, the frame's row of every gene of the table, its dispersions in that order."""
    c, genes = _nb_counts(cluster_counts, who)
    if first:
        first()
    codes = np.asarray(groups)
    if codes.shape != (c.shape[0],):
        raise ValueError("%s: groups has shape %s for %d samples" % (who, codes.shape, c.shape[0]))
    if codes.dtype.kind not in "biu" or not np.isin(codes, (0, 1)).all():
        raise ValueError("%s: groups must be 0 / 1 or boolean%s" % (who, groups_are))
    codes = codes.astype(np.int32)
    if both_groups and codes.min() == codes.max():
        raise ValueError("%s: every sample is in group %d" % (who, codes[0]))
    if not hasattr(de, "columns") or any(col not in de.columns for col in columns) or any(name not in de.attrs for name in attrs):
        needed = "; ".join(kind + " " + ", ".join(names) for kind, names in (("columns", columns), ("attrs", attrs)) if names)
        raise ValueError("%s: de must be a frame of compute_pseudobulk_DE (%s)" % (who, needed))
    if unless:
        unless()
    named = pd.Index(de["gene"])
    at = named.get_indexer(genes) if named.is_unique and genes.is_unique else np.full(1, -1)
    if len(de) != len(genes) or (at < 0).any():
        raise ValueError("%s: the genes of de are not the columns of cluster_counts" % who)
    sf = _nb_size_factors(cluster_counts, de.attrs["size_factors"], c.shape[0])
    samples = getattr(cluster_counts, "index", pd.RangeIndex(c.shape[0]))
    if "replaced" in de.attrs:                                   # (outliers="deseq2": the fit is of the replaced counts)
        c = _apply_replaced(c, genes, samples, de.attrs["replaced"], who)
    return c, genes, samples, codes, sf, at, de["dispersion"].to_numpy(dtype=np.float64)[at]


def lfc_shrink(cluster_counts, groups, de, prior_scale=None):
    """The reference's ``lfcShrink(dds, coef, res, type = "apeglm")`` step (plot/pseudobulk_DE_analysis.py:146-151; Zhu, Ibrahim,
    Love 2019) without R, on the device (``engine.nb_shrink``; apeglm is not installed where this library is built
    and tested, so the rule is this library's statement, UNPINNED).  ``cluster_counts``: the samples x genes counts of the
    selected samples; ``groups``: 0 / 1 or a boolean per sample, 1 for the numerator group; ``de``: the frame
    :func:`compute_pseudobulk_DE` returned for those samples, which supplies the dispersions, the size factors
    (``attrs['size_factors']``), the maximum-likelihood columns and which genes have a floored group fit (``attrs['floored']``).
    Per gene the posterior mode of the fold change under a Cauchy prior of scale ``prior_scale`` (default: estimated from the
    maximum-likelihood fold changes and their standard errors, ``engine.nb_prior_scale``, at most 1) and a wide normal on the
    intercept, and its Laplace standard deviation (``engine.nb_posterior_sd``).  Returns a copy of ``de`` with
    ``log2FoldChange = beta1 / ln 2`` and ``lfcSE = sd / ln 2`` (NaN where the posterior is not log-concave at its mode); the
    new columns ``lfcMLE`` and ``lfcMLESE`` keep the old values; ``stat``, ``pvalue``, ``padj`` and the row order are unchanged,
    as ``lfcShrink`` keeps the unshrunken Wald test.  ``attrs`` gains ``shrink='apeglm'``, ``prior_scale``, ``prior_var``,
    ``n_at_bound`` (genes whose mode sits at the end of the searched interval; none is expected).  A frame made with
    ``outliers="deseq2"`` carries ``attrs['replaced']``: those counts are replaced in ``cluster_counts`` before the fit, and the
    dispersions are the refitted ones.

    Not covered: s-values, other coefficients or more than two groups, apeglm's other likelihoods.  The intercept prior sits
    on group 0, as in apeglm, so swapping the groups moves the estimate slightly instead of negating it."""
    def shrunken_or_bare():
        if "lfcMLE" in de.columns:
            raise ValueError("lfc_shrink: de is already shrunken (it has a column lfcMLE)")
        if "size_factors" not in de.attrs or "floored" not in de.attrs:
            raise ValueError("lfc_shrink: de.attrs lacks 'size_factors' / 'floored': pass the frame compute_pseudobulk_DE returned")
        _estimated_or_positive("lfc_shrink", "prior_scale", prior_scale)

    c, genes, _, codes, sf, at, disp = _nb_de_intake("lfc_shrink", cluster_counts, groups, de, ["gene", "log2FoldChange", "lfcSE", "dispersion"],
                                                     groups_are=", 1 for the numerator group", both_groups=True, unless=shrunken_or_bare)
    ln2 = np.log(2.0)
    lfc, se = de["log2FoldChange"].to_numpy(dtype=np.float64)[at] * ln2, de["lfcSE"].to_numpy(dtype=np.float64)[at] * ln2
    floored = np.asarray(de.attrs["floored"].reindex(genes), dtype=bool)
    if prior_scale is None:
        S, A = engine.nb_prior_scale(lfc, se, use=~floored)
    else:
        S, A = float(prior_scale), float(prior_scale) ** 2
    b0, b1, info = engine.nb_shrink(c, codes, sf, disp, engine.nb_far_end(lfc, floored), S, return_info=True)
    sd = engine.nb_posterior_sd(b1, info["w0"], info["w1"], S)
    row = genes.get_indexer(de["gene"])                          # the table's column of every row of the frame
    out = de.copy()
    out["lfcMLE"], out["lfcMLESE"] = de["log2FoldChange"], de["lfcSE"]
    out["log2FoldChange"], out["lfcSE"] = (b1 / ln2)[row], (sd / ln2)[row]
    out.attrs.update(shrink="apeglm", prior_scale=S, prior_var=A, n_at_bound=info["n_at_bound"])
    return out


_DE_TESTS = ("wald", "lrt")


def _check_design_options(who, covariates, test, shrink, outliers):
    """the K26 arguments of :func:`compute_pseudobulk_DE`, refused before any device work; the covariates as a list (empty: none)"""
    if not (isinstance(test, str) and test in _DE_TESTS):
        raise ValueError("%s: test=%r must be 'wald' or 'lrt'" % (who, test))
    if covariates is None:
        covariates = []
    if isinstance(covariates, (str, bytes)) or not all(isinstance(name, str) for name in covariates):
        raise ValueError("%s: covariates=%r must be a list of column names" % (who, covariates))
    covariates = list(covariates)
    if len(set(covariates)) != len(covariates):
        raise ValueError("%s: covariates=%r names a column twice" % (who, covariates))
    if covariates and (shrink or outliers):
        raise NotImplementedError("%s: covariates with %s: the shrinkage (K23) and the outlier handling (K25) are rules for the design "
                                  "`~ group`%s" % (who, "shrink=%r" % (shrink,) if shrink else "outliers=%r" % (outliers,),
                                                   "; shrink the frame afterwards with tl.lfc_shrink_design" if shrink
                                                   else "; pass the frame to tl.outliers_design afterwards (K28)"))
    if test == "lrt" and not covariates:
        raise ValueError("%s: test='lrt' is the test of the design with covariates, pass covariates" % who)
    return covariates


def deseq2_design(cluster_metadata, cluster_col, group1, group2, covariates):
    """The design matrix of ``~ covariates + group`` for the samples of ``group1`` and ``group2`` (by
    ``cluster_metadata[cluster_col]``), as :func:`compute_pseudobulk_DE` builds it.  Returns ``(X, column_names,
    selected_index)``: X is float64, one row per selected sample in the metadata's order.  The intercept comes first; then, in the
    order of ``covariates``, for a categorical one (object, category or bool dtype) an indicator per level except the first in
    Python string order (``<covariate>_<level>``), and a numeric one centred and scaled to unit ddof-1 standard deviation over the
    selected samples (DESeq2 does not scale; the scaling changes only that nuisance coefficient); the indicator of ``group2``
    (``<cluster_col>_<group2>_vs_<group1>``) comes last.  ValueError: an unknown column, a missing value, a covariate that is
    constant over the selected samples, or one that is confounded with the columns before it (the message names it; a group
    indicator that the covariates already determine names the group column)."""
    who = "deseq2_design"
    if cluster_col is None or cluster_col not in cluster_metadata.columns:
        raise ValueError("%s: cluster_col=%r is not a column of cluster_metadata" % (who, cluster_col))
    if group1 == group2:
        raise ValueError("%s: group1 and group2 are both %r" % (who, group1))
    stage = cluster_metadata[cluster_col]
    meta = cluster_metadata[(stage == group1) | (stage == group2)]
    if len(meta) == 0:
        raise ValueError("%s: no sample of %r or %r" % (who, group1, group2))
    columns, names = [np.ones(len(meta))], ["Intercept"]

    def full_rank():
        return np.linalg.matrix_rank(np.stack(columns, axis=1)) == len(columns)

    for cov in covariates:
        if cov not in meta.columns or cov == cluster_col:
            raise ValueError("%s: covariate %r is not a column of cluster_metadata beside %r" % (who, cov, cluster_col))
        values, before = meta[cov], len(names)
        if values.isna().any():
            raise ValueError("%s: covariate %r has a missing value in sample %r" % (who, cov, values.index[values.isna().to_numpy()][0]))
        if values.dtype == object or values.dtype == bool or isinstance(values.dtype, pd.CategoricalDtype):
            labels = np.array([str(v) for v in values])
            levels = sorted(set(labels))
            if len(levels) < 2:
                raise ValueError("%s: covariate %r is constant (%r) over the selected samples" % (who, cov, levels[0]))
            for level in levels[1:]:
                columns.append((labels == level).astype(np.float64))
                names.append("%s_%s" % (cov, level))
        else:
            v = values.to_numpy(dtype=np.float64)
            sd = v.std(ddof=1) if v.size > 1 else 0.0
            if not (np.isfinite(sd) and sd > 0):
                raise ValueError("%s: covariate %r is constant over the selected samples" % (who, cov))
            columns.append((v - v.mean()) / sd)
            names.append(cov)
        if not full_rank():
            raise ValueError("%s: covariate %r is confounded with the columns before it (%s)" % (who, cov, ", ".join(names[:before])))
    columns.append((meta[cluster_col] == group2).to_numpy().astype(np.float64))
    names.append("%s_%s_vs_%s" % (cluster_col, group2, group1))
    if not full_rank():
        raise ValueError("%s: the group column %r is confounded with the covariates %r" % (who, cluster_col, list(covariates)))
    return np.stack(columns, axis=1), names, meta.index


def _nb_design_tests(c, X, sf, disp, test):
    """the final fit of DESIGN.md K26 at the dispersions ``disp`` and the test of the last design column: ``(beta, log2FoldChange,
    lfcSE, stat, pvalue, fits that did not converge)``; ``test="lrt"`` runs the reduced fit too"""
    from scipy import stats
    beta, cov, loglik, info = engine.nb_design_fits(c, X, sf, disp, return_info=True)
    n_bad = info["n_not_converged"]
    log2e = np.log2(np.e)
    with np.errstate(divide="ignore", invalid="ignore"):
        lfc, se = log2e * beta[:, -1], log2e * np.sqrt(cov[:, -1, -1])
        stat = lfc / se
    p = 2.0 * stats.norm.sf(np.abs(stat))
    if test == "lrt":
        _, _, reduced, info0 = engine.nb_design_fits(c, np.ascontiguousarray(X[:, :-1]), sf, disp, return_info=True)
        n_bad += info0["n_not_converged"]
        stat = 2.0 * (loglik - reduced)
        p = stats.chi2.sf(stat, 1)
    return beta, lfc, se, stat, p, int(n_bad)


def _nb_design_de(counts, X, names, fit_type, test, filtering_alpha):
    """:func:`compute_pseudobulk_DE` by the route of DESIGN.md K26: the dispersion table, the final fit and the host tail for the
    last design column"""
    c, genes = _nb_counts(counts, "compute_pseudobulk_DE")
    sf = _nb_size_factors(counts, None, c.shape[0])
    table = _nb_dispersion_table(c, genes, None, None, sf, fit_type, design=X)
    disp = table["dispersion"].to_numpy()
    beta, lfc, se, stat, p, n_bad = _nb_design_tests(c, X, sf, disp, test)
    base_mean = table["baseMean"].to_numpy()
    padj, filtering = _nb_padj(p, base_mean, filtering_alpha)
    out = pd.DataFrame({"gene": np.asarray(genes), "baseMean": base_mean, "log2FoldChange": lfc, "lfcSE": se, "stat": stat, "pvalue": p,
                        "padj": padj, "dispersion": disp})
    out = out.iloc[np.argsort(padj, kind="stable")].reset_index(drop=True)
    if filtering is not None:
        out.attrs["independent_filtering"] = filtering
    out.attrs.update(dispersions=table, size_factors=pd.Series(sf, index=counts.index), n_not_converged=int(n_bad),
                     design=pd.DataFrame(X, index=counts.index, columns=names), coefficients=pd.DataFrame(beta, index=genes, columns=names),
                     test=test)
    return out


def _shrunken_or_bad_scale(who, de, prior_scale):
    if "lfcMLE" in de.columns:
        raise ValueError("%s: de is already shrunken (it has a column lfcMLE)" % who)
    _estimated_or_positive(who, "prior_scale", prior_scale)


def _nb_design_intake(who, cluster_counts, de, columns, no_design, unless=None):
    """``(cluster_counts, de)`` as the readers of a frame that :func:`compute_pseudobulk_DE` made WITH covariates take them apart
    (:func:`lfc_shrink_design`, :func:`outliers_design`, :func:`deseq2_cooks_design`), every refusal in ``who``'s name and in one
    order: the frame's columns, its design (``no_design`` ends that refusal in ``who``'s words), ``unless()`` (what only ``who``
    checks), the genes, the samples, the coefficients.  Returns ``(c, genes, samples, sf, X, beta, at, dispersion)``: the counts
    with ``attrs['replaced']`` applied, the table's labels, float64 size factors, the design matrix, the coefficients in the table's
    gene order, the frame's row of every gene of the table and its dispersions in that order."""
    c, genes = _nb_counts(cluster_counts, who)
    if not hasattr(de, "columns") or any(col not in de.columns for col in columns) or "size_factors" not in de.attrs:
        raise ValueError("%s: de must be a frame of compute_pseudobulk_DE (columns %s; attrs size_factors, design, coefficients)"
                         % (who, ", ".join(columns)))
    if "design" not in de.attrs or "coefficients" not in de.attrs:
        raise ValueError("%s: de.attrs has no 'design': %s" % (who, no_design))
    if unless:
        unless()
    named = pd.Index(de["gene"])
    at = named.get_indexer(genes) if named.is_unique and genes.is_unique else np.full(1, -1)
    if len(de) != len(genes) or (at < 0).any():
        raise ValueError("%s: the genes of de are not the columns of cluster_counts" % who)
    design, coefficients = de.attrs["design"], de.attrs["coefficients"]
    samples = getattr(cluster_counts, "index", pd.RangeIndex(c.shape[0]))
    if len(design) != c.shape[0] or not pd.Index(design.index).equals(pd.Index(samples)):
        raise ValueError("%s: the samples of de.attrs['design'] are not the rows of cluster_counts" % who)
    if list(coefficients.columns) != list(design.columns) or (pd.Index(coefficients.index).get_indexer(genes) < 0).any():
        raise ValueError("%s: de.attrs['coefficients'] is not genes x design columns of this table" % who)
    sf = _nb_size_factors(cluster_counts, de.attrs["size_factors"], c.shape[0])
    X = engine._nb_design_arg(design.to_numpy(dtype=np.float64), c.shape[0])
    if "replaced" in de.attrs:                                   # (outliers_design: the fit is of the replaced counts)
        c = _apply_replaced(c, genes, samples, de.attrs["replaced"], who)
    beta = np.ascontiguousarray(coefficients.reindex(genes).to_numpy(dtype=np.float64))
    return c, genes, samples, sf, X, beta, at, de["dispersion"].to_numpy(dtype=np.float64)[at]


def lfc_shrink_design(cluster_counts, de, prior_scale=None):
    """:func:`lfc_shrink` for a frame that :func:`compute_pseudobulk_DE` made WITH ``covariates``: the reference's
    ``lfcShrink(dds, coef, res, type = "apeglm")`` step under the design ``~ covariates + stage``, on the device
    (``engine.nb_design_shrink``; apeglm is not installed where this library is built and tested, so the rule is
    this library's statement, UNPINNED).  ``cluster_counts``: the samples x genes counts of the selected samples; ``de``: the
    frame, whose ``attrs`` supply the design matrix (``design``), the maximum-likelihood coefficients (``coefficients``), the size
    factors and the dispersions.  The group column, the last of the design, is shrunk: per gene the posterior mode under a Cauchy
    prior of scale ``prior_scale`` on it (default: ``engine.nb_prior_scale`` of the maximum-likelihood coefficients and their
    standard errors over the genes with ``|beta| < 10``, at most 1) and a normal of scale 15 on every other coefficient, and its
    Laplace standard deviation (``engine.nb_design_posterior_sd``).  Returns a copy of ``de`` with ``log2FoldChange = beta_group /
    ln 2`` and ``lfcSE = sd / ln 2`` (NaN where the posterior is not log-concave at its mode); ``lfcMLE`` and ``lfcMLESE`` keep the
    old values; ``stat``, ``pvalue``, ``padj`` and the row order are unchanged, for ``test="lrt"`` frames too.  ``attrs`` gain
    ``shrink='apeglm'``, ``prior_scale``, ``prior_var``, ``n_at_bound`` (none is expected) and ``coefficients_shrunk`` (genes x p
    at the mode, natural log).  ValueError before any device work: a frame without ``attrs['design']`` (the design ``~ stage``:
    use :func:`lfc_shrink`), a frame already shrunken, genes or samples that are not the table's.  A frame that went through
    :func:`outliers_design` carries ``attrs['replaced']``: those counts are replaced in ``cluster_counts`` before the fit, and the
    dispersions and coefficients are the refitted ones.

    Deviations, unpinned: the global grid search instead of apeglm's local optimiser; the normal prior sits on every unshrunk
    coefficient; ``|beta| < 10`` stands in for K23's "no floored group fit" when the prior scale is estimated; numeric covariates
    are scaled (:func:`deseq2_design`); no s-values."""
    c, genes, _, sf, X, mle, at, disp = _nb_design_intake(
        "lfc_shrink_design", cluster_counts, de, ["gene", "log2FoldChange", "lfcSE", "dispersion"],
        "the frame is of the design `~ group` (no covariates); use lfc_shrink", lambda: _shrunken_or_bad_scale("lfc_shrink_design", de, prior_scale))
    design = de.attrs["design"]
    ln2 = np.log(2.0)
    bk, se = mle[:, -1], de["lfcSE"].to_numpy(dtype=np.float64)[at] * ln2
    if prior_scale is None:
        with np.errstate(invalid="ignore"):
            S, A = engine.nb_prior_scale(bk, se, use=np.isfinite(bk) & (np.abs(bk) < 10.0))
    else:
        S, A = float(prior_scale), float(prior_scale) ** 2
    beta, info = engine.nb_design_shrink(c, X, sf, disp, mle, engine.nb_design_far_end(bk), S, return_info=True)
    sd = engine.nb_design_posterior_sd(beta, info["information"], S)
    row = genes.get_indexer(de["gene"])                          # the table's column of every row of the frame
    out = de.copy()
    out["lfcMLE"], out["lfcMLESE"] = de["log2FoldChange"], de["lfcSE"]
    out["log2FoldChange"], out["lfcSE"] = (beta[:, -1] / ln2)[row], (sd / ln2)[row]
    out.attrs.update(shrink="apeglm", prior_scale=S, prior_var=A, n_at_bound=info["n_at_bound"],
                     coefficients_shrunk=pd.DataFrame(beta, index=genes, columns=list(design.columns)))
    return out


_DE_COLUMNS = ["gene", "baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "padj", "dispersion"]


def outliers_design(cluster_counts, de, min_replace=engine.NB_COOKS_MIN_REPLACE, independent_filtering=None, alpha=0.05):
    """The outlier handling of ``DESeq(dds)`` and ``results(dds)`` (:func:`compute_pseudobulk_DE`'s ``outliers="deseq2"``, DESIGN.md
    K25) for a frame that :func:`compute_pseudobulk_DE` made WITH ``covariates``, Wald or LRT, on the device
    (``engine.nb_design_cooks``; the rule is this library's statement, UNPINNED).  ``cluster_counts``: the samples x
    genes counts of the selected samples; ``de``: the frame, whose ``attrs`` supply the design, the coefficients, the size factors
    and the dispersion table with its trend and prior widths.  K25's groups become CELLS, the sets of samples with identical design
    rows (``engine.nb_design_cells``; DESeq2's ``nOrMoreInCell``); the hat diagonal comes from the whole design and the cutoff is
    ``qf(0.99, p, m - p)``.  The steps are K25's: every sample's Cook's distance; in a cell of at least ``min_replace`` samples a
    count whose distance passes the cutoff is replaced by ``trunc(trimmed mean of c / s  *  s_j)``; the genes with a replacement are
    fitted again on the replaced counts (size factors, trend and prior widths stay; for ``test="lrt"`` the reduced fit too); a gene
    whose largest distance over the samples of cells of 3 to ``min_replace - 1`` passes the cutoff loses ``pvalue`` unless three or
    more samples have a larger count.  ``padj`` is recomputed by plain BH, or by ``engine.independent_filtering`` at ``alpha``;
    ``independent_filtering=None`` means as the frame was made (on iff ``attrs['independent_filtering']`` exists; pass the ``alpha``
    it was made with).  Returns a new frame ordered by ``padj`` with the columns ``maxCooks``, ``cooksOutlier``, ``replace`` and the
    attrs ``cooks_cutoff`` and ``replaced`` (``gene, sample, count, replacement``); ``attrs['dispersions']`` and
    ``attrs['coefficients']`` hold the refitted rows and ``n_not_converged`` grows by the refit's.  A gene that the replacement
    empties becomes all NaN.  A frame in which nothing is replaced or flagged keeps every old column bit for bit.

    Under a design whose cells are all below 3 samples (a numeric covariate) the distances are computed but nothing is replaced or
    flagged, as in DESeq2: ``maxCooks`` is NaN throughout.  ValueError before any device work: a frame without ``attrs['design']``
    (use ``compute_pseudobulk_DE(outliers="deseq2")`` for the design ``~ group``), a frame already handled (it has ``maxCooks``), a
    shrunken frame (it has ``lfcMLE``: shrink afterwards, :func:`lfc_shrink_design` reads ``attrs['replaced']``), genes or samples
    that are not the table's.  Deviations beyond K25's: DESIGN.md K28."""
    who = "outliers_design"

    def handled_or_shrunken():
        if "maxCooks" in de.columns:
            raise ValueError("%s: de has been through the outlier handling already (it has a column maxCooks)" % who)
        if "lfcMLE" in de.columns:
            raise ValueError("%s: de is shrunken (it has a column lfcMLE): handle the outliers first and shrink afterwards with "
                             "lfc_shrink_design, which reads attrs['replaced']" % who)
        if "dispersions" not in de.attrs or de.attrs.get("test") not in _DE_TESTS:
            raise ValueError("%s: de.attrs lacks 'dispersions' / 'test': pass the frame compute_pseudobulk_DE returned" % who)
        engine._nb_min_replace_arg(min_replace)
        if not (independent_filtering is None or isinstance(independent_filtering, (bool, np.bool_))):
            raise ValueError("%s: independent_filtering=%r must be None, True or False" % (who, independent_filtering))
        _alpha_arg(who, alpha)

    c, genes, samples, sf, X, beta, at, disp = _nb_design_intake(
        who, cluster_counts, de, _DE_COLUMNS, "the frame is of the design `~ group` (no covariates); use compute_pseudobulk_DE(outliers=\"deseq2\")",
        handled_or_shrunken)
    table, test = de.attrs["dispersions"], de.attrs["test"]
    if not pd.Index(table.index).equals(genes):
        raise ValueError("%s: de.attrs['dispersions'] is not the table of these genes" % who)
    if independent_filtering is None:
        independent_filtering = "independent_filtering" in de.attrs
    m, p = X.shape
    cells, _ = engine.nb_design_cells(X)
    cutoff = engine.nb_cooks_cutoff(m, p)
    ck = engine.nb_design_cooks(c, X, sf, disp, beta, cutoff, min_replace)
    max_cooks, n_above = ck["max_cooks"].copy(), ck["n_above"].copy()
    cols = {name: de[name].to_numpy()[at].copy() for name in _DE_COLUMNS[1:]}       # the frame's columns in the table's gene order
    beta, table, n_bad = beta.copy(), table.copy(), int(de.attrs.get("n_not_converged", 0))
    rep = np.flatnonzero(ck["n_replace"] > 0)
    replaced = pd.DataFrame({name: [] for name in _REPLACED_COLUMNS})
    if rep.size:
        sub = np.ascontiguousarray(c[:, rep])
        ck2 = engine.nb_design_cooks(sub, X, sf, disp[rep], beta[rep], cutoff, min_replace, return_distances=True)
        rows = engine.nb_replacements(sub, cells, sf, ck2["D"], cutoff, ck2["trimmed_base"], min_replace)
        new = np.rint(sub.astype(np.float64))
        new[rows["sample"], rows["gene"]] = rows["replacement"]
        replaced = pd.DataFrame({"gene": np.asarray(genes)[rep[rows["gene"]]], "sample": np.asarray(samples)[rows["sample"]],
                                 "count": rows["count"], "replacement": rows["replacement"]})
        # the refit: the same fit of the replaced counts, the trend and both prior widths as they were
        refit = _nb_dispersion_table(new, genes[rep], None, None, sf, None, frozen=table.attrs, design=X)
        ndisp = refit["dispersion"].to_numpy()
        beta[rep], lfc, se, stat, pv, bad = _nb_design_tests(new, X, sf, ndisp, test)
        n_bad += bad
        for j, name in enumerate(table.columns):
            table.iloc[rep, j] = refit[name].to_numpy()
        for name, v in (("baseMean", refit["baseMean"].to_numpy()), ("log2FoldChange", lfc), ("lfcSE", se), ("stat", stat), ("pvalue", pv),
                        ("dispersion", ndisp)):
            cols[name][rep] = v
        live = ~np.isnan(ndisp)
        max_cooks[rep], n_above[rep] = np.nan, 0
        if live.any():
            ck3 = engine.nb_design_cooks(np.ascontiguousarray(new[:, live]), X, sf, ndisp[live], beta[rep[live]], cutoff, min_replace,
                                         return_distances=True)
            max_cooks[rep[live]], n_above[rep[live]] = _nb_refit_max_cooks(new[:, live], cells, ck3["D"], min_replace)
    with np.errstate(invalid="ignore"):
        flagged = (max_cooks > cutoff) & (n_above < 3)
    cols["pvalue"][flagged] = np.nan
    padj, filtering = _nb_padj(cols["pvalue"], cols["baseMean"], float(alpha) if independent_filtering else None)
    cols["padj"] = padj
    replace = np.zeros(len(genes), dtype=bool)
    replace[rep] = True
    out = pd.DataFrame({"gene": np.asarray(genes), **{name: cols[name] for name in _DE_COLUMNS[1:]}, "maxCooks": max_cooks,
                        "cooksOutlier": flagged, "replace": replace})
    out = out.iloc[np.argsort(padj, kind="stable")].reset_index(drop=True)
    out.attrs.update({k: v for k, v in de.attrs.items() if k != "independent_filtering"})
    if filtering is not None:
        out.attrs["independent_filtering"] = filtering
    names = list(de.attrs["design"].columns)
    out.attrs.update(dispersions=table, coefficients=pd.DataFrame(beta, index=genes, columns=names), n_not_converged=n_bad, cooks_cutoff=cutoff,
                     replaced=replaced)
    return out


def deseq2_cooks_design(cluster_counts, de, min_replace=engine.NB_COOKS_MIN_REPLACE):
    """The per-gene Cook's-distance table behind :func:`outliers_design` (``engine.nb_design_cooks``), for looking at
    what the rule saw: :func:`deseq2_cooks` for a frame made WITH covariates.  ``de`` supplies the design, the size factors, the
    dispersions and the coefficients; a frame that went through :func:`outliers_design` has its replacements applied first, so
    the table describes the refitted state.  Returns a frame indexed by gene, in the table's column order: ``alpha_robust``,
    ``max_cooks``, ``arg_max`` (the sample's label; None without one), ``n_above``, ``n_replace``, ``trimmed_base``;
    ``attrs['cooks_cutoff']`` and ``attrs['cells']`` (per sample its cell, ``engine.nb_design_cells``)."""
    who = "deseq2_cooks_design"
    c, genes, samples, sf, X, beta, _, disp = _nb_design_intake(
        who, cluster_counts, de, ["gene", "dispersion"], "the frame is of the design `~ group` (no covariates); use deseq2_cooks",
        lambda: engine._nb_min_replace_arg(min_replace))
    cutoff = engine.nb_cooks_cutoff(*X.shape)
    ck = engine.nb_design_cooks(c, X, sf, disp, beta, cutoff, min_replace)
    labels = np.asarray(samples, dtype=object)
    out = pd.DataFrame({"alpha_robust": ck["alpha_robust"], "max_cooks": ck["max_cooks"],
                        "arg_max": [labels[i] if i >= 0 else None for i in ck["arg_max"]], "n_above": ck["n_above"],
                        "n_replace": ck["n_replace"], "trimmed_base": ck["trimmed_base"]}, index=genes)
    out.attrs.update(cooks_cutoff=cutoff, cells=pd.Series(engine.nb_design_cells(X)[0], index=samples))
    return out


def compute_pseudobulk_DE(cluster_counts=None, cluster_metadata=None, group1=None, group2=None, cluster_col=None, fit_type="parametric",
                          shrink=None, prior_scale=None, outliers=None, independent_filtering=False, alpha=0.05, covariates=None,
                          test="wald"):
    """The reference's ``compute_pseudobulk_DE`` (plot/pseudobulk_DE_analysis.py:96-159) without R: the negative-binomial Wald
    test of DESeq2 for the design ``~ stage`` between two patient sub-groups, on the device.  Takes :func:`pseudobulk_inputs`'
    pair unchanged; the samples of ``group1`` and ``group2`` (by ``cluster_metadata[cluster_col]``) are selected first, as the
    reference does, so the size factors (:func:`deseq2_size_factors`) and the dispersions (:func:`deseq2_dispersions`) come from
    those samples only.  Then per gene and group the maximum-likelihood normalised mean at the final dispersion
    (``engine.nb_group_fits``) and, on the host, ``log2FoldChange = log2(mean_group2) - log2(mean_group1)``,
    ``lfcSE = log2(e) sqrt(1 / W_1 + 1 / W_2)``, ``stat``, ``pvalue = 2 norm.sf(|stat|)`` and the Benjamini-Hochberg ``padj`` over
    the genes with a p-value.  Returns ONE frame -- ``gene, baseMean, log2FoldChange, lfcSE, stat, pvalue, padj, dispersion`` --
    ordered by ``padj`` (NaN last, ties in gene order: the reference's ``arrange(padj)``); a gene that is zero in every selected
    sample has NaN in every numeric column.  ``attrs``: ``dispersions`` (the frame of :func:`deseq2_dispersions`),
    ``size_factors``, ``n_not_converged``, ``floored`` (per gene whether a group's fit was raised to its floor, a group of zeros).

    ``shrink``: ``None`` (the default) returns the maximum-likelihood ``log2FoldChange`` and its Wald ``lfcSE``; ``"apeglm"``
    applies :func:`lfc_shrink` (with ``prior_scale``), which is what the reference's call returns: the posterior mode and
    standard deviation under apeglm's prior, beside the unchanged Wald columns, with ``lfcMLE`` / ``lfcMLESE`` keeping the
    maximum-likelihood values.  Anything else: ValueError before any device work.

    ``outliers``: ``None`` (the default) or ``"deseq2"``, the outlier handling of ``DESeq(dds)`` and ``results(dds)`` (DESIGN.md
    K25; ``engine.nb_cooks``): after the fit, every sample's Cook's distance with a robust dispersion in its variance; in a group
    of at least 7 samples a count whose distance passes ``cooks_cutoff = qf(0.99, 2, m - 2)`` is replaced by
    ``trunc(trimmed mean of c / s  *  s_j)`` and the genes with a replacement are fitted again on the replaced counts (the size
    factors, the trend and the prior widths stay; a gene the replacement empties becomes all NaN); a gene whose largest distance
    over the samples that could NOT be replaced (groups of 3 to 6) passes the cutoff loses ``pvalue`` and ``padj`` unless three or
    more samples have a larger count than the one at the maximum.  New columns: ``maxCooks``, ``cooksOutlier``, ``replace``;
    new ``attrs``: ``cooks_cutoff``, ``replaced`` (a frame ``gene, sample, count, replacement``); ``attrs['dispersions']`` holds
    the refitted rows.  ``independent_filtering=True`` (with or without ``outliers``) adjusts the p-values as ``results(dds,
    alpha = alpha)`` does (``engine.independent_filtering``): BH over the genes whose ``baseMean`` passes the quantile that
    maximises the rejections at ``alpha``; ``padj`` is NaN below it, and ``attrs['independent_filtering']`` records the choice.
    With the defaults the frame is what it was without these arguments, bit for bit.  Any other ``outliers``, or an ``alpha``
    outside (0, 1): ValueError before any device work.

    Deviations from the reference's call, which is unpinned here (no DESeq2 or apeglm where this library is tested): the
    shrinkage, the outlier handling and the independent filtering are opt-in (``shrink="apeglm"``, ``outliers="deseq2"``,
    ``independent_filtering=True``; the reference's call has all three on) and the shrunken mode comes from a global grid
    search, not apeglm's local optimiser; no s-values; ``rlog`` is :func:`compute_pseudobulk_PCA`'s; the deviations of the outlier
    rule are DESIGN.md K25's; no beta ridge; the dispersion search is global; for ``m - 2 <= 3`` the prior variance uses the
    formula where DESeq2 simulates; the reference returns R's list (the frame at index 1), this returns the frame.  Fewer than
    three selected samples, or a group without samples: ValueError before any device work.

    ``covariates``: ``None`` (the default; an empty list is the same) is the design ``~ stage`` described above, untouched.  A list
    of columns of ``cluster_metadata`` (batch, sex, age, centre; :func:`pseudobulk_inputs` copies them from ``adata.obs`` with
    ``obs_columns``) makes the design ``~ covariates + stage`` (:func:`deseq2_design`) and takes the route of DESIGN.md K26: the
    dispersions from the adjusted profile likelihood with the coefficients fitted again at every dispersion
    (``engine.nb_design_dispersions``), the trend, prior and outlier rule as above with p coefficients, then the coefficients, their
    covariance ``(X^T W X + 1e-6 I)^-1`` and the log likelihood at the final dispersion (``engine.nb_design_fits``).
    ``log2FoldChange = log2(e) beta_group``, ``lfcSE = log2(e) sqrt(Sigma_group,group)`` and, with ``test="wald"``, ``stat`` their
    ratio and ``pvalue = 2 norm.sf(|stat|)``; with ``test="lrt"`` a second fit without the group column at the same dispersions,
    ``stat = 2 (loglik_full - loglik_reduced)`` and ``pvalue = chi2.sf(stat, 1)`` (the fold change and its error stay the Wald
    ones).  The frame has the same columns; ``attrs`` gain ``design`` (the frame of X), ``coefficients`` (genes x p, natural log)
    and ``test``, and have no ``floored``.  ``independent_filtering`` works as above.  ``shrink="apeglm"`` or ``outliers="deseq2"``
    with covariates: NotImplementedError before any device work -- K23 and K25 are rules for the group design (for the shrinkage,
    pass the returned frame to :func:`lfc_shrink_design`).  Any other
    ``test``, ``test="lrt"`` without covariates, an unknown, constant or confounded covariate, more than
    ``engine.NB_DESIGN_MAX_COLS`` design columns or no residual degree of freedom: ValueError before any device work.  Deviations
    from DESeq2 under a design: the profile re-solves the coefficients where DESeq2 holds the means of one rough
    fit; the global search; the plain inverse instead of the sandwich covariance; numeric covariates are scaled; no betaPrior."""
    _check_shrink(shrink, "compute_pseudobulk_DE")
    _check_de_options(outliers, independent_filtering, alpha, "compute_pseudobulk_DE")
    covariates = _check_design_options("compute_pseudobulk_DE", covariates, test, shrink, outliers)
    if cluster_col is None or cluster_col not in cluster_metadata.columns:
        raise ValueError("compute_pseudobulk_DE: cluster_col=%r is not a column of cluster_metadata" % (cluster_col,))
    stage = cluster_metadata[cluster_col]
    if group1 == group2:
        raise ValueError("compute_pseudobulk_DE: group1 and group2 are both %r" % (group1,))
    meta = cluster_metadata[(stage == group1) | (stage == group2)]
    counts = cluster_counts.loc[meta.index]
    codes = (meta[cluster_col] == group2).to_numpy().astype(np.int32)
    n2 = int(codes.sum())
    if n2 == 0 or n2 == codes.size:
        raise ValueError("compute_pseudobulk_DE: no sample of %r" % ((group2 if n2 == 0 else group1),))
    if codes.size < 3:
        raise ValueError("compute_pseudobulk_DE: %d samples in two groups leave no residual degree of freedom" % codes.size)
    if covariates:
        X, names, _ = deseq2_design(cluster_metadata, cluster_col, group1, group2, covariates)
        X = engine._nb_design_arg(X, codes.size)
        return _nb_design_de(counts, X, names, fit_type, test, float(alpha) if independent_filtering else None)
    c, genes = _nb_counts(counts, "compute_pseudobulk_DE")
    sf = _nb_size_factors(counts, None, c.shape[0])
    fit, cooks, extra = _nb_fit(c, genes, codes, sf, fit_type), None, {}
    if outliers:
        fit, cooks, extra = _nb_outliers(c, genes, counts.index, codes, sf, fit)
    out = _nb_wald_table(genes, fit, cooks, float(alpha) if independent_filtering else None)
    floored = pd.Series(((fit.flags & engine._lib.NB_FLOORED) != 0).any(axis=1), index=genes)
    out.attrs.update(dispersions=fit.table, size_factors=pd.Series(sf, index=counts.index),
                     n_not_converged=int(np.count_nonzero(fit.flags & engine._lib.NB_NOT_CONVERGED)), floored=floored, **extra)
    return lfc_shrink(counts, codes, out, prior_scale) if shrink else out


def deseq2_cooks(cluster_counts, groups, de, min_replace=engine.NB_COOKS_MIN_REPLACE):
    """The per-gene Cook's-distance table behind ``outliers="deseq2"`` (``engine.nb_cooks``), for looking at what
    the rule saw.  ``cluster_counts`` and ``groups`` (0 / 1 or boolean per sample) as :func:`lfc_shrink` takes them; ``de``: the
    frame :func:`compute_pseudobulk_DE` returned for those samples, which supplies the dispersions and the size factors.  A frame
    made with ``outliers="deseq2"`` has its replacements applied first, so the table describes the refitted state.  The group
    means are fitted again at the frame's dispersions (``engine.nb_group_fits``).  Returns a frame indexed by gene, in the
    table's column order: ``alpha_robust``, ``max_cooks``, ``arg_max`` (the sample's label; None without one), ``n_above``,
    ``n_replace``, ``trimmed_base``; ``attrs['cooks_cutoff']``."""
    c, genes, samples, codes, sf, _, disp = _nb_de_intake("deseq2_cooks", cluster_counts, groups, de, ["gene", "dispersion"], ["size_factors"],
                                                          first=lambda: engine._nb_min_replace_arg(min_replace))
    cutoff = engine.nb_cooks_cutoff(c.shape[0], 2)
    q, _ = engine.nb_group_fits(c, codes, 2, sf, disp)
    ck = engine.nb_cooks(c, codes, 2, sf, disp, q, cutoff, min_replace)
    labels = np.asarray(samples, dtype=object)
    out = pd.DataFrame({"alpha_robust": ck["alpha_robust"], "max_cooks": ck["max_cooks"],
                        "arg_max": [labels[i] if i >= 0 else None for i in ck["arg_max"]], "n_above": ck["n_above"],
                        "n_replace": ck["n_replace"], "trimmed_base": ck["trimmed_base"]}, index=genes)
    out.attrs["cooks_cutoff"] = cutoff
    return out


def independent_filtering(de, alpha=0.05):
    """``engine.independent_filtering`` on a frame :func:`compute_pseudobulk_DE` already made: a copy whose ``padj`` comes from
    its ``pvalue`` and ``baseMean`` columns, ordered by the new ``padj`` (NaN last, ties in gene order where
    ``attrs['dispersions']`` tells it, else in the frame's), with ``attrs['independent_filtering']`` the info dict."""
    if not hasattr(de, "columns") or any(col not in de.columns for col in ("gene", "baseMean", "pvalue", "padj")):
        raise ValueError("independent_filtering: de must be a frame of compute_pseudobulk_DE (columns gene, baseMean, pvalue, padj)")
    alpha = _alpha_arg("independent_filtering", alpha)
    out = de.copy()
    table = de.attrs.get("dispersions")
    if table is not None and len(table) == len(de) and table.index.is_unique:
        at = pd.Index(de["gene"]).get_indexer(table.index)
        if (at >= 0).all():
            out = out.iloc[at].reset_index(drop=True)
    padj, info = engine.independent_filtering(out["pvalue"].to_numpy(dtype=np.float64), out["baseMean"].to_numpy(dtype=np.float64), alpha)
    out["padj"] = padj
    out = out.iloc[np.argsort(padj, kind="stable")].reset_index(drop=True)
    out.attrs.update(de.attrs)
    out.attrs["independent_filtering"] = info
    return out


# ---- regularised log transform and its PCA: rlog(dds, blind = TRUE), plotPCA_subgroups (plot/pseudobulk_DE_analysis.py:161-233) ---
def rlog(cluster_counts, size_factors=None, fit_type="parametric", prior_var=None):
    """DESeq2's ``rlog(dds, blind = TRUE)`` of a samples x genes count frame without R, on the device (DESeq2 is not
    installed where this library is built and tested, so the rule is this library's statement, UNPINNED).  With c = rint(counts)
    and ``size_factors`` (default :func:`deseq2_size_factors`): the gene-wise dispersions of the design ``~ 1``
    (``engine.nb_dispersions_blind``), their trend over ``baseMean = mean_j(c_j / s_j)`` (``engine.nb_trend`` with ``fit_type``),
    clipped to [1e-8, max(10, m)] -- rlog reads the TREND value for every gene, there is no MAP step --, the prior variance of the
    sample coefficients (``engine.nb_rlog_prior_var``; ``prior_var`` skips it) and per gene the ridge-penalised negative-binomial
    GLM with one coefficient a sample (``engine.nb_rlog``).  Returns a float64 frame shaped and labelled like ``cluster_counts``:
    ``log2`` of the fitted normalised count of every sample; a gene of zeros is 0 everywhere.  ``attrs``: ``size_factors``,
    ``dispFit`` (what the fit used), ``prior_var``, ``intercept`` (log2; NaN for a gene of zeros), ``n_not_converged``.

    Deviations from DESeq2: the fit is the optimum of the penalised likelihood (to 1e-10 in the coefficients), where DESeq2's IRLS
    stops at a deviance change of 1e-4 and clamps mu at 0.5 inside its loop; the dispersions come from the global grid search of
    :func:`deseq2_dispersions`; a parametric trend that does not fit raises ValueError where DESeq2 falls back to a local
    regression (``fit_type="mean"``); the weighted-quantile rule of the prior variance is restated from memory of Hmisc."""
    c, genes = _nb_counts(cluster_counts, "rlog")
    m = c.shape[0]
    if m < 2:
        raise ValueError("rlog: %d samples, at least 2" % m)
    if c.shape[1] < 1:
        raise ValueError("rlog: the table has no genes")
    if fit_type not in ("parametric", "mean"):
        raise ValueError("rlog: fit_type=%r must be 'parametric' or 'mean'" % (fit_type,))
    _estimated_or_positive("rlog", "prior_var", prior_var)
    sf = _nb_size_factors(cluster_counts, size_factors, m)
    if not (np.isfinite(sf).all() and (sf > 0).all()):
        raise ValueError("rlog: size_factors must be positive and finite")
    x = engine.nb_dispersions_blind(c, sf)
    base_mean = (np.rint(c.astype(np.float64)) / sf[:, None]).mean(axis=0)
    fit, _ = engine.nb_trend(base_mean, engine.nb_clip(np.exp(x), m), fit_type)
    fit = engine.nb_clip(fit, m)
    pv = engine.nb_rlog_prior_var(c, sf, base_mean, fit) if prior_var is None else float(prior_var)
    values, info = engine.nb_rlog(c, sf, fit, pv, return_info=True)
    out = pd.DataFrame(values, index=getattr(cluster_counts, "index", None), columns=genes)
    out.attrs.update(size_factors=pd.Series(sf, index=out.index), dispFit=pd.Series(fit, index=genes), prior_var=pv,
                     intercept=pd.Series(info["intercept"], index=genes), n_not_converged=info["n_not_converged"])
    return out


def compute_pseudobulk_PCA(cluster_counts=None, cluster_metadata=None):
    """The reference's ``compute_pseudobulk_PCA`` (plot/pseudobulk_DE_analysis.py:161-207) without R: ``as.data.frame(assay(rlog(dds,
    blind = TRUE)))`` of :func:`pseudobulk_inputs`' pair, a genes x samples frame (:func:`rlog`, transposed; its ``attrs`` are
    kept).  ``cluster_metadata`` is only aligned -- its index must be the samples of ``cluster_counts``, as
    ``DESeqDataSetFromMatrix`` demands -- because ``blind`` ignores the design.  The deviations of :func:`rlog` apply."""
    if cluster_metadata is not None and not pd.Index(cluster_metadata.index).equals(pd.Index(cluster_counts.index)):
        raise ValueError("compute_pseudobulk_PCA: the rows of cluster_metadata are not the samples of cluster_counts, in their order")
    rld = rlog(cluster_counts)
    out = rld.T
    out.attrs.update(rld.attrs)
    return out


def pseudobulk_pca(rld, variance_threshold=0.2, n_components=2):
    """The numbers of the reference's ``plotPCA_subgroups`` (plot/pseudobulk_DE_analysis.py:209-218): of a samples x genes table
    ``rld`` (:func:`rlog`'s frame, or ``compute_pseudobulk_PCA(...).T`` as the reference passes it; any other samples x genes table
    is taken as it is, nothing is transformed) keep the genes whose variance over the samples (ddof 0, scikit-learn's
    ``VarianceThreshold``) exceeds ``variance_threshold``, then the first ``n_components`` principal components of the centred
    samples x kept-genes matrix on the device (``engine.pca(scale=False)``), with scikit-learn 1.7's signs: in every component
    the loading of largest magnitude is positive.  Returns ``(scores, variance_ratio)``: a frame samples x ``PC1 ..`` and the
    explained variance ratios.  Fewer than ``n_components + 1`` genes pass, or a bad argument: ValueError before any device work.
    No plot."""
    X = np.asarray(rld, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("pseudobulk_pca: a samples x genes table, got shape %s" % (X.shape,))
    if isinstance(n_components, bool) or int(n_components) != n_components or n_components < 1:
        raise ValueError("pseudobulk_pca: n_components=%r must be a positive integer" % (n_components,))
    if not isinstance(variance_threshold, (int, float, np.integer, np.floating)) or isinstance(variance_threshold, bool) \
            or not variance_threshold >= 0:
        raise ValueError("pseudobulk_pca: variance_threshold=%r must be a number >= 0" % (variance_threshold,))
    if not np.isfinite(X).all():
        raise ValueError("pseudobulk_pca: the table holds a non-finite value")
    kept = np.flatnonzero(X.var(axis=0) > variance_threshold)
    if kept.size < n_components + 1:
        raise ValueError("pseudobulk_pca: %d genes have a variance above %g, at least n_components + 1 = %d are needed"
                         % (kept.size, variance_threshold, n_components + 1))
    scores, pcs, _, ratio = engine.pca(np.ascontiguousarray(X), n_comps=int(n_components), scale=False, cols=kept.astype(np.int32))
    sign = np.sign(pcs[np.abs(pcs).argmax(axis=0), np.arange(pcs.shape[1])])
    sign[sign == 0] = 1.0
    names = ["PC%d" % (i + 1) for i in range(scores.shape[1])]
    return pd.DataFrame(scores * sign[None], index=getattr(rld, "index", None), columns=names), ratio


def get_pseudobulk_DE(adata, proportion_df, cell_type, celltype_col="cell_types", sample_col="sampleID", cluster_col="Predicted_Labels",
                      remove_samples=(), shrink=None, outliers=None, independent_filtering=False, alpha=0.05, covariates=None, test="wald"):
    """The numbers of the reference's ``get_pseudobulk_DE`` (plot/pseudobulk_DE_analysis.py:506-666) in one process with no R:
    :func:`pseudobulk_inputs` of ``cell_type``, then :func:`compute_pseudobulk_DE` for every pair of
    ``itertools.combinations(np.unique(proportion_df[cluster_col]), 2)``.  Returns ``{"<g2>vs<g1>": frame}`` (the names of the
    reference's ``_DE.csv`` files; the fold change is g2 over g1).  ``shrink`` is :func:`compute_pseudobulk_DE`'s (``"apeglm"``:
    the shrunken fold changes the reference writes), and so are ``outliers``, ``independent_filtering`` and ``alpha``.  No plots,
    no files, no enrichment; the rlog PCA the reference draws first is :func:`compute_pseudobulk_PCA` / :func:`pseudobulk_pca` on
    :func:`pseudobulk_inputs`' pair; the deviations of :func:`compute_pseudobulk_DE` apply.  ``covariates`` and ``test`` are
    :func:`compute_pseudobulk_DE`'s too; a covariate that ``proportion_df`` lacks is taken from ``adata.obs``, where
    it must be constant within every sample (:func:`pseudobulk_inputs`' ``obs_columns``)."""
    import itertools
    _check_shrink(shrink, "get_pseudobulk_DE")
    _check_de_options(outliers, independent_filtering, alpha, "get_pseudobulk_DE")
    covariates = _check_design_options("get_pseudobulk_DE", covariates, test, shrink, outliers)
    cluster_counts, cluster_metadata = pseudobulk_inputs(adata, proportion_df, cell_type, celltype_col, sample_col, cluster_col, remove_samples,
                                                         obs_columns=[name for name in covariates if name not in proportion_df.columns])
    out = {}
    for g1, g2 in itertools.combinations(np.unique(proportion_df[cluster_col]), 2):
        out["%svs%s" % (g2, g1)] = compute_pseudobulk_DE(cluster_counts, cluster_metadata, group1=g1, group2=g2, cluster_col=cluster_col,
                                                         shrink=shrink, outliers=outliers, independent_filtering=independent_filtering,
                                                         alpha=alpha, covariates=covariates or None, test=test)
    return out


# ---- clinical variables (Trajectory.py:1361-1609: the four correlation_* tests; PERMANOVA of uns['EMD']: DESIGN.md K29) ---------
def _converts_to_float(value):
    try:
        float(value)
    except ValueError:
        return False
    return True


def _clinical_values(adata, left, sample_col, feature):
    """``left`` (a frame with a ``sampleID`` column) with the feature's value of every sample beside it: the value of the sample's
    first row of ``adata.obs``, NaN for a sample obs does not have"""
    values = adata.obs[[sample_col, feature]].rename(columns={sample_col: "sampleID"})
    return left.merge(values, on="sampleID", how="left").drop_duplicates(subset="sampleID")


def _drop_numbers(frame, feature):
    """a categorical test's cleaning: the rows whose value is among the floats the column's values convert to are dropped -- real
    numbers and NaN go, a numeric STRING stays (it is not equal to its float) and is a level"""
    numbers = [float(v) for v in frame[feature] if _converts_to_float(v)]
    return frame[~frame[feature].isin(numbers)]


def _drop_labels(frame, feature):
    """a numeric test's cleaning: the rows whose value does not convert to a float are dropped; NaN converts, and stays"""
    labels = np.unique([v for v in frame[feature] if not _converts_to_float(v)])
    return frame[~frame[feature].isin(list(labels))]


def _significant(rows, p_column, sort_column):
    """the reference's last three lines: the features with p < 0.05, sorted"""
    table = pd.DataFrame(rows)
    table = table[table[p_column].astype(float) < 0.05]
    return table.sort_values(by=sort_column)


def correlation_categorical_with_trajectory(adata, sample_col="sampleID", features=[], sort_column="ANOVA_PValue"):
    """The reference's test of categorical clinical variables against the pseudotime (Trajectory.py:1377-1427), host only:
    per feature, ``scipy.stats.f_oneway`` of ``uns['orders'].Time_score`` over the feature's levels, one value per sample (its
    first row of ``adata.obs``), after dropping real numbers and missing values.  Returns the reference's frame ``Feature,
    ANOVA_FStatistic, ANOVA_PValue``: only the features with p < 0.05, sorted by ``sort_column``.  The Kruskal-Wallis statistic
    the reference computes and discards is not computed.  :func:`permanova` tests the same question on the distances themselves."""
    from scipy import stats
    rows = []
    for feature in features:
        frame = _drop_numbers(_clinical_values(adata, adata.uns["orders"], sample_col, feature), feature)
        frame = frame.dropna(subset=["Time_score", feature])
        stat, p = stats.f_oneway(*[group["Time_score"] for _, group in frame.groupby(feature)])
        rows.append({"Feature": feature, "ANOVA_FStatistic": stat, "ANOVA_PValue": float(p)})
    return _significant(rows, "ANOVA_PValue", sort_column)


def correlation_numeric_with_trajectory(adata, sample_col="sampleID", features=[], sort_column="Spearman_PValue"):
    """The reference's test of numeric clinical variables against the pseudotime (Trajectory.py:1444-1492), host only: per
    feature, ``scipy.stats.spearmanr`` of ``uns['orders'].Time_score`` and the feature, one value per sample, after dropping the
    values that are no numbers.  A missing value is NOT dropped, as in the reference: the correlation is NaN and the feature
    fails the filter.  Returns ``Feature, Spearman_Correlation, Spearman_PValue`` for p < 0.05, sorted by ``sort_column``
    (Kendall's tau, computed and discarded by the reference, is not computed)."""
    from scipy import stats
    rows = []
    for feature in features:
        frame = _drop_labels(_clinical_values(adata, adata.uns["orders"], sample_col, feature), feature)
        corr, p = stats.spearmanr(frame["Time_score"], frame[feature])
        rows.append({"Feature": feature, "Spearman_Correlation": corr, "Spearman_PValue": float(p)})
    return _significant(rows, "Spearman_PValue", sort_column)


def correlation_categorical_with_clustering(adata, proportion_df, sample_col="sampleID", features=[], sort_column="ChiSquared_PValue"):
    """The reference's test of categorical clinical variables against the samples' sub-groups (Trajectory.py:1497-1549), host
    only: per feature, ``scipy.stats.chi2_contingency`` of the table ``Predicted_Labels`` x levels.  ``proportion_df`` is what
    :func:`clustering_emd` returns.  Returns ``Feature, ChiSquared_Statistic, ChiSquared_PValue`` for p < 0.05, sorted."""
    from scipy import stats
    groups = proportion_df[["sampleID", "Predicted_Labels"]]
    rows = []
    for feature in features:
        frame = _drop_numbers(_clinical_values(adata, groups, sample_col, feature), feature)
        table = pd.crosstab(frame["Predicted_Labels"].astype(str), frame[feature])
        stat, p = stats.chi2_contingency(table)[:2]
        rows.append({"Feature": feature, "ChiSquared_Statistic": stat, "ChiSquared_PValue": float(p)})
    return _significant(rows, "ChiSquared_PValue", sort_column)


def correlation_numeric_with_clustering(adata, proportion_df, sample_col="sampleID", features=[], sort_column="ANOVA_P_Value"):
    """The reference's test of numeric clinical variables against the samples' sub-groups (Trajectory.py:1551-1609), host only:
    per feature, ``scipy.stats.f_oneway`` of the feature over the ``Predicted_Labels``, in their order of first appearance.
    Returns ``Feature, ANOVA_F_Statistic, ANOVA_P_Value`` for p < 0.05, sorted (no Kruskal-Wallis statistic)."""
    from scipy import stats
    groups = proportion_df[["sampleID", "Predicted_Labels"]]
    rows = []
    for feature in features:
        frame = _drop_labels(_clinical_values(adata, groups, sample_col, feature), feature)
        labels = frame["Predicted_Labels"].astype(str)
        result = stats.f_oneway(*[frame[labels == g][feature].values for g in labels.unique()])
        rows.append({"Feature": feature, "ANOVA_F_Statistic": result.statistic, "ANOVA_P_Value": float(result.pvalue)})
    return _significant(rows, "ANOVA_P_Value", sort_column)


_PERMANOVA_COLUMNS = ["Feature", "kind", "n", "df", "SS_model", "SS_total", "R2", "pseudo_F", "p_value", "p_adj"]


def _permanova_variable(values):
    """One value per sample -> ``(kind, used, x)``: the reference's cleaning.  A missing value (None, NaN) drops its sample.  If
    every other value converts with ``float()`` the variable is numeric (``detect_values_to_remove`` would remove nothing) and
    ``x`` the floats; else it is categorical, the real numbers among its values are dropped as ``detect_numeric_values`` drops
    them (a numeric string stays, and is a level), and ``x`` the values as strings."""
    present = np.array([not (v is None or (isinstance(v, (float, np.floating)) and v != v)) for v in values], dtype=bool)
    if all(_converts_to_float(v) for v, ok in zip(values, present) if ok):
        return "numeric", present, np.array([float(v) for v, ok in zip(values, present) if ok], dtype=np.float64)
    numbers = [float(v) for v, ok in zip(values, present) if ok and _converts_to_float(v)]
    used = present & ~pd.Series(list(values), dtype=object).isin(numbers).to_numpy()
    return "categorical", used, np.array([str(v) for v, ok in zip(values, used) if ok], dtype=object)


def permanova(adata, features, sample_col="sampleID", permutations=9999, seed=0, strata=None, D=None):
    """PERMANOVA of the samples' distance matrix against clinical variables (Anderson 2001; the rule is this library's, DESIGN.md
    K29): does the variable explain the distances between the samples?  Where the reference tests a variable against the
    one-dimensional pseudotime or the sub-group labels, this is the permutation test on ``uns['EMD']`` itself.

    ``D`` (default ``adata.uns['EMD']``): a samples x samples array or ``engine.DeviceMatrix``, in the order of
    ``uns['proportions']``.  Per feature: one value per sample (its first row of ``adata.obs``); numeric if every value present
    converts with ``float()``, else categorical (real numbers among the values are dropped, numeric strings are levels), as the
    reference's ``detect_values_to_remove`` / ``detect_numeric_values`` decide; a sample with a missing value is dropped.  The
    features with the same used samples share one ``engine.permanova_ss`` call: every feature is a marginal term, tested
    against the same ``permutations`` permutations of ``seed`` (within the levels of the obs column ``strata``, if given).
    Returns a frame, one row per feature in the order given: ``Feature, kind, n, df, SS_model, SS_total, R2, pseudo_F, p_value,
    p_adj``; ``p_value = (1 + #{F_b >= F_0 - sqrt(2^-52)}) / (1 + permutations)`` and ``p_adj`` its Benjamini-Hochberg
    adjustment over the features.  ``attrs``: ``permutations``, ``seed``, ``strata``.  No 0.05 filter, no plots, no files.

    Not covered / deviations: sequential or adjusted terms (every term is tested alone), PERMDISP, pairwise post-hoc tests.
    ValueError before any device work: no ``uns['EMD']`` / ``['proportions']``, a matrix of another size, an unknown feature or
    strata column, a missing stratum, a feature with one level or no variation, fewer than ``df + 2`` samples left."""
    if D is None:
        if "EMD" not in adata.uns:
            raise ValueError("adata.uns has no 'EMD': run tl.wasserstein_distance first, or pass D")
        D = adata.uns["EMD"]
    if "proportions" not in adata.uns:
        raise ValueError("adata.uns has no 'proportions': run tl.wasserstein_distance first")
    samples = list(adata.uns["proportions"].keys())
    N = len(samples)
    if tuple(getattr(D, "shape", np.shape(D))) != (N, N):
        raise ValueError("D is %s, uns['proportions'] has %d samples" % (tuple(getattr(D, "shape", np.shape(D))), N))
    features = list(features)
    if not features:
        raise ValueError("permanova: no feature")
    for name in features + ([strata] if strata is not None else []):
        if name not in adata.obs.columns:
            raise ValueError("adata.obs has no column %r" % (name,))
    permutations = int(permutations)
    if permutations < 1:
        raise ValueError("permutations=%d" % permutations)
    first = adata.obs.drop_duplicates(subset=sample_col).set_index(sample_col)

    def per_sample(name):
        return [first.at[s, name] if s in first.index else None for s in samples]

    strata_values = None
    if strata is not None:
        strata_values = np.array([str(v) for v in per_sample(strata)], dtype=object)
        if any(v is None or (isinstance(v, float) and v != v) for v in per_sample(strata)):
            raise ValueError("strata column %r has a missing value" % (strata,))
    calls = {}
    for position, name in enumerate(features):
        kind, used, x = _permanova_variable(per_sample(name))
        calls.setdefault(used.tobytes(), (used, []))[1].append((position, name, kind, x))
    bases = []
    for used, members in calls.values():
        Q, terms = engine.permanova_basis({name: x for _, name, _, x in members})
        n = int(used.sum())
        if n - int(np.diff(terms).max()) - 1 < 1:
            raise ValueError("permanova: %d samples are too few for a term of %d columns" % (n, int(np.diff(terms).max())))
        bases.append((Q, terms, n))
    records = [None] * len(features)
    for (used, members), (Q, terms, n) in zip(calls.values(), bases):
        rows = None if used.all() else np.flatnonzero(used).astype(np.int32)
        ss_total, ss = engine.permanova_ss(D, Q, terms, permutations, seed=seed, rows=rows,
                                           strata=None if strata_values is None else strata_values[used])
        F = engine.permanova_f(ss_total, ss, terms, n)
        p = engine.permanova_p(F)
        for t, (position, name, kind, _) in enumerate(members):
            records[position] = {"Feature": name, "kind": kind, "n": n, "df": int(terms[t + 1] - terms[t]), "SS_model": ss[0, t],
                                 "SS_total": ss_total, "R2": ss[0, t] / ss_total, "pseudo_F": F[0, t], "p_value": p[t]}
    table = pd.DataFrame(records)
    table["p_adj"] = _bh_adjust(table["p_value"].to_numpy())
    table = table[_PERMANOVA_COLUMNS]
    table.attrs.update(permutations=permutations, seed=int(seed), strata=strata)
    return table
