"""Inputs shared by tests/test_silhouette_args.py and tests/test_gpu_silhouette.py: the sample cohorts of the resolution sweeps, the
duck-typed AnnData they ride in, and the sweep composed on the CPU from the restatements (neighbors_restatement,
louvain_restatement, scikit-learn's silhouette_score) -- what tl.select_best_sil is held to where the device is not looked at."""
import functools

import numpy as np
import pandas as pd
from scipy.spatial.distance import cdist
from sklearn.metrics import silhouette_score

import louvain_restatement as LR
import neighbors_restatement as NR

CELL_TYPES = ["T", "B", "NK", "Mono"]
REFERENCE_RESOLUTIONS = [0.2 + 0.1 * i for i in range(int((2 - 0.2) / 0.1) + 1)]


class Adata:
    def __init__(self, obsm=None, uns=None, obs=None, obsp=None):
        self.obsm, self.uns, self.obs, self.obsp = obsm or {}, uns or {}, pd.DataFrame() if obs is None else obs, obsp


@functools.lru_cache(maxsize=None)
def cohort(name):
    """(points, group of every sample, E): ``three_groups`` -- 20 samples around each of (0, 0), (6, 0), (0, 6), normals x 0.5, rows
    permuted; ``one_blob`` -- 60 samples of one tight blob.  E: the Euclidean distance matrix of the points, read-only."""
    rng = np.random.default_rng(1)
    if name == "three_groups":
        centres = np.repeat(np.array([[0.0, 0.0], [6.0, 0.0], [0.0, 6.0]]), 20, axis=0)
        group = np.repeat(np.arange(3), 20)
        points = centres + 0.5 * rng.normal(size=(60, 2))
        perm = rng.permutation(60)
        points, group = points[perm], group[perm]
    else:
        points, group = 0.05 * rng.normal(size=(60, 2)), np.zeros(60, dtype=int)
    E = cdist(points, points)
    for a in (points, group, E):
        a.setflags(write=False)
    return points, group, E


def emd_adata(name, n=None):
    """what tl.wasserstein_distance leaves in uns, for the first n samples of the cohort"""
    _, _, E = cohort(name)
    n = E.shape[0] if n is None else n
    rng = np.random.default_rng(7)
    P = rng.dirichlet(np.ones(len(CELL_TYPES)), size=n)
    proportions = {"s%02d" % i: P[i] for i in range(n)}
    # the cell types in first-appearance order, which is not the sorted one
    annot = pd.DataFrame({"cell_type": [CELL_TYPES[i % len(CELL_TYPES)] for i in range(3 * len(CELL_TYPES))]})
    return Adata(uns={"EMD": np.array(E[:n, :n]), "proportions": proportions, "annot": annot})


def cpu_graph(E, metric):
    idx, dist, _ = NR.knn(E, 14, metric)
    return NR.connectivities(idx, dist, 15)


def cpu_sweep(E, metric, resolutions, normalize=False):
    """[(labels, silhouette or NaN, k, Q)] per resolution, on the CPU"""
    graph = cpu_graph(E, metric)
    out = []
    for res in resolutions:
        labels, q, (_, _, k) = LR.louvain(graph, resolution=res)
        sil = silhouette_score(E / E.max() if normalize else E, labels, metric=metric) if 2 <= k <= E.shape[0] - 1 else np.nan
        out.append((labels, sil, k, q))
    return out


def same_partition(a, b):
    """two labellings name the same groups"""
    pairs = set(zip(np.asarray(a).tolist(), np.asarray(b).tolist()))
    return len(pairs) == len(set(np.asarray(a).tolist())) == len(set(np.asarray(b).tolist()))


def best_by_rule(resolutions, scores, start):
    """the reference's rule, restated: start unless a silhouette is > 0; the strictly greatest, the first of equals"""
    best_res, best_sil = start, 0
    for res, sil in zip(resolutions, scores):
        if sil > best_sil:
            best_res, best_sil = res, sil
    return best_res
