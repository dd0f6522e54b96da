#!/usr/bin/env python3
"""Time of the device PCA (K15, engine.DeviceCSR.pca) on one synthetic data set, beside the reference-style route on the host.

Case cells x genes, about --fill stored: float32 Poisson counts from a gamma model of --rank latent factors (strengths 1 .. 0.45:
the leading --comps eigenvalues are separated, as in real data; a matrix of independent counts has no gaps and no Lanczos run ends
on it), built in process in row chunks.  Device: upload, normalize_log1p, then ``pca(n_comps, scale=True, max_value=10)`` timed
with a host clock around the call (it ends in device-to-host copies) after one warm-up call; ``info['steps']`` gives the Lanczos
steps, and a second timed call with ``PILOT_OT_PCA_BASIS`` = half of them gives the cost of the late steps: ms per step is quoted
as total / steps.  Beside it the streaming floor of the two products: per step 12 bytes per stored entry for the row form and 12
for the column form at 6.3 TB/s.  Host (--cpu): the same normalised matrix made dense in float32, scaled as scanpy does
(mean / ddof-1 std / upper clip, numpy), then ``sklearn.decomposition.PCA(n_comps, svd_solver='arpack')``; the leading variances
of the two routes are compared.  Writes OUT/time_pca.txt (--out, default profiles/pca/)."""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.3e12


def synthetic(n, G, rank, fill, seed, chunk=20000):
    rng = np.random.default_rng(seed)
    W = rng.gamma(0.4, 1.0, (rank, G))
    strengths = np.linspace(1.0, 0.45, rank)
    depth = -np.log1p(-fill) / (W.sum(axis=0).mean() * strengths.mean())      # E[lambda] ~ -log(1 - fill): about `fill` non-zero
    parts = []
    for r0 in range(0, n, chunk):
        L = rng.gamma(1.0, 1.0, (min(chunk, n - r0), rank)) * strengths
        parts.append(sp.csr_matrix(rng.poisson(depth * (L @ W)).astype(np.float32)))
    return sp.vstack(parts, format="csr")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca"))
    ap.add_argument("--cells", type=int, default=200000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--fill", type=float, default=0.10)
    ap.add_argument("--rank", type=int, default=50)
    ap.add_argument("--comps", type=int, default=50)
    ap.add_argument("--cpu", action="store_true", help="also time the dense scale + scikit-learn arpack route on the host")
    a = ap.parse_args()
    from pilot_amd import _lib, engine

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    t0 = time.perf_counter()
    X = synthetic(a.cells, a.genes, a.rank, a.fill, 0)
    say("case %d x %d, %d stored (fill %.3f), %d factors, %d components; built in %.1f s on %s"
        % (X.shape[0], X.shape[1], X.nnz, X.nnz / np.prod(X.shape), a.rank, a.comps, time.perf_counter() - t0, _lib.device_name()))
    t0 = time.perf_counter()
    S = engine.DeviceCSR.upload(X).normalize_log1p(1e4)
    S.build_columns()
    say("upload + normalize_log1p + column form: %.1f ms" % (1e3 * (time.perf_counter() - t0)))

    def run():
        t = time.perf_counter()
        out = S.pca(n_comps=a.comps, return_info=True)
        return time.perf_counter() - t, out

    run()
    total, out = run()
    info = out[4]
    floor = 24.0 * X.nnz / COPY_RATE
    say("device pca: %.1f ms, %d Lanczos steps (converged %s, rank_deficient %s): %.3f ms per step; streaming floor of the two "
        "products %.3f ms per step" % (1e3 * total, info["steps"], info["converged"], info["rank_deficient"], 1e3 * total / info["steps"],
                                       1e3 * floor))
    half = max(a.comps, info["steps"] // 2)
    _lib.test_switch("PILOT_OT_PCA_BASIS", half)
    t_half, out_half = run()
    _lib.test_switch("PILOT_OT_PCA_BASIS", None)
    say("the first %d steps alone: %.1f ms (%.3f ms per step; the re-orthogonalisation grows with the basis)"
        % (out_half[4]["steps"], 1e3 * t_half, 1e3 * t_half / out_half[4]["steps"]))
    say("leading variances: %s; ratio sum %.4f" % (np.array2string(out[2][:4], precision=5), out[3].sum()))

    if a.cpu:
        from sklearn.decomposition import PCA
        Y = engine.download(S.densify())                          # the normalised values, float32
        t0 = time.perf_counter()
        mean = Y.mean(axis=0, dtype=np.float64)
        std = Y.std(axis=0, ddof=1, dtype=np.float64)
        std[std == 0] = 1.0
        Y -= mean.astype(np.float32)
        Y /= std.astype(np.float32)
        np.minimum(Y, np.float32(10.0), out=Y)
        t_scale = time.perf_counter() - t0
        t0 = time.perf_counter()
        p = PCA(n_components=a.comps, svd_solver="arpack").fit(Y)
        Xp = p.transform(Y)
        t_pca = time.perf_counter() - t0
        rel = np.abs(p.explained_variance_ - out[2]).max() / out[2][0]
        say("host: dense float32 scale %.1f s, scikit-learn arpack PCA %.1f s (%d threads); its variances differ from the device's by "
            "%.1e of the leading one (float32 data)" % (t_scale, t_pca, os.cpu_count() if "OMP_NUM_THREADS" not in os.environ
                                                         else int(os.environ["OMP_NUM_THREADS"]), rel))
        del Xp
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time_pca.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
