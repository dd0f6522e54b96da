#!/usr/bin/env python3
"""Time of the Louvain communities (K17, engine.louvain) on the neighbour graphs of synthetic cells, beside a sequential Louvain on
the host.

Cases: --cells x --dims float32 (default 50 000 x 50 and 200 000 x 50), a mixture of 32 Gaussian blobs; ``tl.neighbors`` (15
neighbours, euclidean) makes both graphs once, ``obsp['connectivities']`` (symmetric) and ``obsp['distances']`` (directed), and both
stay resident on the host as scipy CSR while ``engine.louvain`` is timed on each: a host clock around the call, which forms A + A^T
on the host, uploads it once and ends in the copy of the labels, after one warm-up call; the best and the median of --repeats calls,
with the levels, the sweeps and the time per sweep (the whole call over its sweeps: aggregation and the host steps included).
Host (--cpu, the smallest case, connectivities): ``networkx.community.louvain_communities`` (sequential, seed 0) if networkx is
importable, else the sequential reference of tests/louvain_restatement.py, with the modularity either reaches at the same
resolution.  --leiden: ``engine.leiden`` (K20) is timed beside ``engine.louvain`` on the same graphs in the same way, with its
levels, move and refinement sweeps, its ratio to the Louvain time, and the number of communities of either that are not connected
in A + A^T (tests/leiden_restatement.py's ``disconnected``).  No threshold is set.  Writes OUT/louvain_rate.txt, with --leiden
OUT/leiden_rate.txt (--out, default profiles/louvain/)."""
import argparse
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class Cells:
    def __init__(self, X):
        self.obsm, self.uns, self.obsp, self.obs = {"X_pca": X}, {}, {}, pd.DataFrame(index=np.arange(X.shape[0]))


def cloud(n, D, seed):
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.normal(size=(32, D))
    return (centres[rng.integers(0, 32, n)] + rng.normal(size=(n, D))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "louvain"))
    ap.add_argument("--cells", type=int, nargs="+", default=[50000, 200000])
    ap.add_argument("--dims", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--resolution", type=float, default=1.0)
    ap.add_argument("--cpu", action="store_true", help="also run a sequential Louvain on the host (smallest case, connectivities)")
    ap.add_argument("--leiden", action="store_true", help="also time engine.leiden on the same graphs")
    a = ap.parse_args()
    import leiden_restatement as LD
    import louvain_restatement as LR
    from pilot_amd import _lib, engine, tl

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("synchronous Louvain of tl.neighbors graphs (15 neighbours, euclidean), D = %d, resolution %g, tol 1e-3, on %s"
        % (a.dims, a.resolution, _lib.device_name()))
    kept = {}
    for n in a.cells:
        ad = Cells(cloud(n, a.dims, n))
        t0 = time.perf_counter()
        tl.neighbors(ad)
        say("%7d cells: tl.neighbors %.2f s; connectivities %d stored entries, distances %d"
            % (n, time.perf_counter() - t0, ad.obsp["connectivities"].nnz, ad.obsp["distances"].nnz))
        for mode in ("connectivities", "distances"):
            A = ad.obsp[mode]
            engine.louvain(A, resolution=a.resolution)
            times = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                labels, info = engine.louvain(A, resolution=a.resolution, return_info=True)
                times.append(time.perf_counter() - t0)
            best, med = min(times), float(np.median(times))
            say("%7d %-14s: best %8.1f ms, median %8.1f ms of %d calls; %d levels, %d sweeps, %.2f ms per sweep; %d communities, Q = %.4f"
                % (n, mode, 1e3 * best, 1e3 * med, a.repeats, info["levels"], info["sweeps"], 1e3 * best / max(info["sweeps"], 1),
                   info["communities"], info["modularity"]))
            kept[(n, mode)] = (A, labels, info)
            if a.leiden:
                engine.leiden(A, resolution=a.resolution)
                times = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    refined, rinfo = engine.leiden(A, resolution=a.resolution, return_info=True)
                    times.append(time.perf_counter() - t0)
                rbest, rmed = min(times), float(np.median(times))
                say("%7d %-14s: leiden best %8.1f ms, median %8.1f ms of %d calls (%.2f x louvain); %d levels, %d move + %d refinement sweeps; "
                    "%d communities, Q = %.4f; communities not connected: louvain %d, leiden %d"
                    % (n, mode, 1e3 * rbest, 1e3 * rmed, a.repeats, rbest / best, rinfo["levels"], rinfo["move_sweeps"], rinfo["refine_sweeps"],
                       rinfo["communities"], rinfo["modularity"], LD.disconnected(A, labels), LD.disconnected(A, refined)))
    if a.cpu:
        n = min(a.cells)
        A, labels, info = kept[(n, "connectivities")]
        try:
            import networkx as nx
        except ImportError:
            nx = None
        t0 = time.perf_counter()
        if nx is not None:
            parts = nx.community.louvain_communities(nx.from_scipy_sparse_array(A), weight="weight", resolution=a.resolution, seed=0)
            host = np.empty(n, dtype=np.int64)
            for c, members in enumerate(parts):
                host[list(members)] = c
            name = "networkx %s louvain_communities (seed 0)" % nx.__version__
        else:
            host = LR.sequential_louvain(A, a.resolution)[0]
            name = "the sequential reference of tests/louvain_restatement.py"
        t = time.perf_counter() - t0
        say("host: %s, %d connectivities: %.1f s, %d communities, Q = %.4f (device: %d communities, Q = %.4f)"
            % (name, n, t, int(host.max()) + 1, LR.modularity(A, host, a.resolution), info["communities"], info["modularity"]))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "leiden_rate.txt" if a.leiden else "louvain_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
