#!/usr/bin/env python3
"""Time of the exact cell neighbour search (K16, engine.knn) on synthetic embeddings, beside its lane-operation floor and
scikit-learn's brute-force search on the host.

Cases: --cells x --dims float32 (default 50 000 x 50 and 200 000 x 50), k = 14 (scanpy's n_neighbors = 15), both metrics.  The cloud
is a mixture of 32 Gaussian blobs, uploaded once as a ``DeviceMatrix``.  Device: ``engine.knn`` timed with a host clock around the
call (it ends in the device-to-host copies of the two result arrays, which are part of what a caller waits for) after one warm-up
call per case; the best and the median of --repeats calls are quoted.  Floor: the kernel forms n^2 D terms (x_d - y_d)^2, one
subtraction and one fused multiply-add each, 3 flop per term, over the packed-float32 vector rate measured on a GEMM-shaped loop
(52 TFLOP/s; the 157 TFLOP/s peak is not reached by any vector loop).  Host (--cpu, the smaller case only):
``sklearn.neighbors.NearestNeighbors(algorithm='brute')`` of the same rows, and how many of its neighbours the device returned.
Writes OUT/knn_rate.txt (--out, default profiles/neighbors/)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_F32_RATE = 52e12
K = 14


def cloud(n, D, seed):
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.normal(size=(32, D))
    return (centres[rng.integers(0, 32, n)] + rng.normal(size=(n, D))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbors"))
    ap.add_argument("--cells", type=int, nargs="+", default=[50000, 200000])
    ap.add_argument("--dims", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu", action="store_true", help="also time scikit-learn's brute-force search on the host (smallest case)")
    a = ap.parse_args()
    from pilot_amd import _lib, engine

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("exact kNN of the rows, float32, D = %d, k = %d, on %s" % (a.dims, K, _lib.device_name()))
    kept = {}
    for n in a.cells:
        X = cloud(n, a.dims, n)
        Xd = engine.DeviceMatrix.upload(X)
        floor = 3.0 * n * n * a.dims / VALU_F32_RATE
        for metric in ("euclidean", "cosine"):
            engine.knn(Xd, K, metric=metric)
            times = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                out = engine.knn(Xd, K, metric=metric)
                times.append(time.perf_counter() - t0)
            best, med = min(times), float(np.median(times))
            say("%7d x %d %-9s: best %8.1f ms, median %8.1f ms of %d calls; floor %7.1f ms (n^2 D terms x 3 flop at %.0f TFLOP/s): "
                "%.1f x the floor, %.2f T terms/s" % (n, a.dims, metric, 1e3 * best, 1e3 * med, a.repeats, 1e3 * floor, VALU_F32_RATE / 1e12,
                                                      best / floor, n * n * a.dims / best / 1e12))
            kept[(n, metric)] = (X, out)
    if a.cpu:
        from sklearn.neighbors import NearestNeighbors
        n = min(a.cells)
        for metric in ("euclidean", "cosine"):
            X, (idx, _) = kept[(n, metric)]
            t0 = time.perf_counter()
            nn = NearestNeighbors(n_neighbors=K + 1, algorithm="brute", metric=metric).fit(X)
            ref = nn.kneighbors(X, return_distance=False)
            t = time.perf_counter() - t0
            # its first column is the row itself wherever no other row coincides with it
            share = np.mean([len((set(ref[i]) - {i}) & set(idx[i])) / K for i in range(0, n, max(1, n // 2000))])
            say("host: scikit-learn brute force %7d x %d %-9s: %.1f s (%s threads); %.4f of its neighbours are the device's"
                % (n, a.dims, metric, t, os.environ.get("OMP_NUM_THREADS", os.cpu_count()), share))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "knn_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
