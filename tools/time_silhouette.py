#!/usr/bin/env python3
"""Time of the matrix-free silhouette (K18, engine.silhouette_samples) on synthetic embeddings, beside the exact neighbour search
(K16, engine.knn) of the same rows in the same run, scikit-learn's silhouette_samples on the host, and a whole resolution sweep.

Cases: --cells x --dims float32 (default 50 000 x 50), both metrics.  The cloud is a mixture of 32 Gaussian blobs, uploaded once as a
``DeviceMatrix``; the labels are the blobs (32 clusters).  Device: each call timed with a host clock around it (it ends in the
device-to-host copy of its results, which is part of what a caller waits for) after one warm-up call per case; the best and the
median of --repeats calls are quoted, K18 and K16 alternating.  K18 forms the same n^2 D terms (x_d - y_d)^2 as K16 and adds one
float64 add per pair, and under ``euclidean`` one square root per pair (K16 takes roots only of its k results): the ratio says what
those cost.  --sweep: ``tl.neighbors`` once, then ``tl.select_best_resolution`` with its 19 default resolutions -- 19 Louvain runs
plus 19 all-pairs passes.  Host (--cpu N): ``sklearn.metrics.silhouette_samples`` of the first N rows (it chunks an N x N matrix
on the host, so N is what it can hold; default 20 000), and the largest difference from the device's values of the same rows.
Writes OUT/silhouette_rate.txt (--out, default profiles/silhouette/)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 14
BLOBS = 32


def cloud(n, D, seed):
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.normal(size=(BLOBS, D))
    blob = rng.integers(0, BLOBS, n)
    return (centres[blob] + rng.normal(size=(n, D))).astype(np.float32), blob


class _Cells:
    def __init__(self, X):
        import pandas as pd
        self.obsm, self.uns, self.obsp, self.obs = {"X_pca": X}, {}, {}, pd.DataFrame(index=np.arange(X.shape[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "silhouette"))
    ap.add_argument("--cells", type=int, nargs="+", default=[50000])
    ap.add_argument("--dims", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="also time a 19-resolution tl.select_best_resolution (smallest case)")
    ap.add_argument("--cpu", type=int, nargs="?", const=20000, default=0, metavar="N",
                    help="also time scikit-learn's silhouette_samples on the first N rows on the host (default 20000)")
    a = ap.parse_args()
    from pilot_amd import _lib, engine, tl

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("silhouette of labelled rows (K18) beside the exact kNN (K16, k = %d), float32, D = %d, %d clusters, on %s"
        % (K, a.dims, BLOBS, _lib.device_name()))
    for n in a.cells:
        X, blob = cloud(n, a.dims, n)
        Xd = engine.DeviceMatrix.upload(X)
        for metric in ("euclidean", "cosine"):
            engine.silhouette_samples(Xd, blob, metric=metric)
            engine.knn(Xd, K, metric=metric)
            t_sil, t_knn = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                s, score = engine.silhouette_samples(Xd, blob, metric=metric, return_score=True)
                t_sil.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                engine.knn(Xd, K, metric=metric)
                t_knn.append(time.perf_counter() - t0)
            say("%7d x %d %-9s: K18 best %8.1f ms, median %8.1f ms; K16 best %8.1f ms, median %8.1f ms of %d calls each; K18 / K16 = %.2f; "
                "%.2f T terms/s; mean silhouette %.4f" % (n, a.dims, metric, 1e3 * min(t_sil), 1e3 * float(np.median(t_sil)), 1e3 * min(t_knn),
                                                         1e3 * float(np.median(t_knn)), a.repeats, min(t_sil) / min(t_knn),
                                                         n * n * a.dims / min(t_sil) / 1e12, score))
    if a.sweep:
        n = min(a.cells)
        X, _ = cloud(n, a.dims, n)
        cells = _Cells(X)
        t0 = time.perf_counter()
        tl.neighbors(cells)
        t_graph = time.perf_counter() - t0
        t0 = time.perf_counter()
        frame = tl.select_best_resolution(cells)
        t_sweep = time.perf_counter() - t0
        say("sweep %d x %d euclidean: tl.neighbors %.2f s, then tl.select_best_resolution over %d resolutions %.2f s (%d Louvain runs + %d "
            "all-pairs passes); best_res %.1f, clusters %d .. %d" % (n, a.dims, t_graph, len(frame), t_sweep, len(frame), len(frame),
                                                                      cells.uns["best_res"], frame["n_clusters"].min(), frame["n_clusters"].max()))
    if a.cpu:
        from sklearn.metrics import silhouette_samples
        n = min(a.cpu, min(a.cells))
        X, blob = cloud(min(a.cells), a.dims, min(a.cells))
        X, blob = X[:n], blob[:n]
        for metric in ("euclidean", "cosine"):
            t0 = time.perf_counter()
            ref = silhouette_samples(X, blob, metric=metric)
            t = time.perf_counter() - t0
            t0 = time.perf_counter()
            s = engine.silhouette_samples(X, blob, metric=metric)
            td = time.perf_counter() - t0
            say("host: scikit-learn silhouette_samples %7d x %d %-9s: %.1f s (%s threads); the device, from a host array: %.1f ms; "
                "max |device - scikit-learn| = %.1e (scikit-learn expands |x|^2 + |y|^2 - 2 x.y in float32)"
                % (n, a.dims, metric, t, os.environ.get("OMP_NUM_THREADS", os.cpu_count()), 1e3 * td, float(np.abs(s - ref).max())))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "silhouette_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
