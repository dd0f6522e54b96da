#!/usr/bin/env python3
"""Time of the elastic principal tree (K19, engine.principal_tree) and of its fit kernels.

Cases: a sample-level one (--samples x 2 float64 from a host array, M = 20 nodes: what tl.fit_principal_graph sees after
tl.diffusion_map) and a cell-level one (--cells x 50 float32 from a ``DeviceMatrix``, M = 30; --cells 0 leaves it out).  Both
clouds are three noisy branches from the origin.  Per case: the total time of ``engine.principal_tree`` with a host clock around
it (best of --repeats after a warm-up), the time per growth step, the candidates fitted, and the kernel launches per step: a
step is one library call and one read-back, and launches its row check once and a partition and a finish kernel max_iter + 1
times (candidates that have converged leave those at once).  The fit kernels: ``engine.elastic_fit`` of a batch of the final
tree's grow candidates with eps = 0 (no candidate stops early) at max_iter = 2 and 12; the difference / 10 / candidates is one
partition + finish per candidate, quoted beside the partition's lane-operation floor: n m D subtract + FMA terms (3 flop) at the
52 TFLOP/s packed-f32 vector rate measured for K16.  --cpu: the numpy restatement (tests/principal_tree_restatement.py) on the
same host, whole for the sample-level case, one partition + solve of one candidate for the cell-level one.
Writes OUT/time_principal_tree.txt (--out, default profiles/principal_tree/)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VECTOR_FLOPS = 52e12


def branches(n, D, seed, dtype):
    rng = np.random.default_rng(seed)
    dirs = rng.normal(size=(3, D)) / np.sqrt(D)
    t, br = rng.uniform(0, 1, n), rng.integers(0, 3, n)
    return np.ascontiguousarray((t[:, None] * dirs[br] + 0.05 / np.sqrt(D) * rng.normal(size=(n, D))).astype(dtype))


def best(fn, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return min(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "principal_tree"))
    ap.add_argument("--samples", type=int, default=600)
    ap.add_argument("--cells", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu", action="store_true", help="also time the numpy restatement on this host")
    a = ap.parse_args()
    from pilot_amd import _lib, engine

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("elastic principal tree (K19) on %s" % _lib.device_name())
    cases = [("sample-level", a.samples, 2, np.float64, 20, False)]
    if a.cells:
        cases.append(("cell-level", a.cells, 50, np.float32, 30, True))
    for label, n, D, dtype, M, on_device in cases:
        X = branches(n, D, n, dtype)
        arg = engine.DeviceMatrix.upload(X) if on_device else X
        engine.principal_tree(arg, n_nodes=min(M, 4))
        t, (nodes, edges, info) = best(lambda: engine.principal_tree(arg, n_nodes=M, return_info=True), a.repeats)
        steps, cands = info["steps"], info["candidates"]
        say("%-12s %7d x %-2d %s, M = %d, %s: total %9.1f ms, %d steps, %7.2f ms per step, %d candidates (at most %d a step), "
            "%d kernel launches per step; energy %.6g"
            % (label, n, D, np.dtype(dtype).name, M, "DeviceMatrix" if on_device else "host array", 1e3 * t, steps, 1e3 * t / steps,
               sum(cands), max(cands), 2 * 11 + 1, info["energy"][-1]))
        counts = np.zeros(M, dtype=np.int64)
        grown = engine._grow_candidates(nodes, [tuple(e) for e in edges], counts + 1, nodes.copy())
        Y0 = np.stack([c[0] for c in grown])
        S = np.stack([engine.tree_springs(M + 1, c[1]) for c in grown])
        centre = engine.point_moments(arg)[0]
        engine.elastic_fit(arg, Y0, S, centre, max_iter=2, eps=0.0)
        t2, _ = best(lambda: engine.elastic_fit(arg, Y0, S, centre, max_iter=2, eps=0.0), a.repeats)
        t12, _ = best(lambda: engine.elastic_fit(arg, Y0, S, centre, max_iter=12, eps=0.0), a.repeats)
        per = (t12 - t2) / 10 / len(grown)
        floor = 3.0 * n * (M + 1) * D / VECTOR_FLOPS
        say("%-12s fit of %d candidates of %d nodes: %8.2f ms at max_iter 2, %8.2f ms at 12; partition + finish per candidate "
            "%8.1f us; partition floor %7.2f us (n m D x 3 flop at 52 TFLOP/s); ratio %.1f"
            % (label, len(grown), M + 1, 1e3 * t2, 1e3 * t12, 1e6 * per, 1e6 * floor, per / floor))
        tp, _ = best(lambda: engine.tree_pseudotime(arg, nodes, edges), a.repeats)
        say("%-12s tree_pseudotime: %8.2f ms" % (label, 1e3 * tp))
        if a.cpu:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import principal_tree_restatement as R
            if not on_device:
                t0 = time.perf_counter()
                Yr, er, _ = R.tree(X, M)
                tr = time.perf_counter() - t0
                say("%-12s host: the numpy restatement of the whole tree %.2f s (%.0f x the device call); max |nodes - restatement| "
                    "%.1e" % (label, tr, tr / t if t else 0.0, float(np.abs(Yr - nodes).max()) if np.array_equal(er, edges) else np.nan))
            else:
                t0 = time.perf_counter()
                _, cnt, s, _ = R.partition(X, Y0[0])
                np.linalg.solve(np.diag(cnt / n) + S[0], s / n)
                tr = time.perf_counter() - t0
                say("%-12s host: one numpy partition + solve of one candidate %.2f s (%.0f x the device's)" % (label, tr, tr / per))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time_principal_tree.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
