#!/usr/bin/env python3
"""Wall time of pl.trajectory's embedding (pydiffmap's DiffusionMap.from_sklearn(n_evecs=2, epsilon=1, alpha=0.5, k=64)
.fit_transform(E / E.max()), pilotpy/plot/ploting.py:95-110) at c3 (N = 600) and c4 (N = 2000) synthetic grids:

  * device chain from a DeviceMatrix (the pair grid's result still in HBM; only the N x 2 result comes back);
  * the same chain from a host array (one N x N upload);
  * the numpy / scipy restatement (tests/diffmap_restatement.py: kNN kernel, then sparse eigs(L, which='LR')) on this host's CPUs.

Writes profiles/diffmap/diffmap_rate.txt.  `--chain-only c4` runs just the device chain a few times (for a rocprofv3 kernel trace
of its own).  GPU only."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import diffmap_restatement as R  # noqa: E402
from pilot_amd import _lib, engine  # noqa: E402
from pilot_amd.synthetic import CONFIGS, make_problem  # noqa: E402

KW = dict(n_evecs=2, epsilon=1.0, alpha=0.5, k=64)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t)
    return out, 1e3 * float(np.median(ts)), 1e3 * float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chain-only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffmap", "diffmap_rate.txt"))
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("diffmap_rate.py needs a HIP device")
    cfgs = [a.chain_only] if a.chain_only else ["c3", "c4"]
    lines = ["# diffusion map (n_evecs=2, epsilon=1, alpha=0.5, knn=64) on %s; median / min of the timed calls, ms" % _lib.device_name()]
    for cfg in cfgs:
        P, M = make_problem(**CONFIGS[cfg])
        N = P.shape[0]
        plan = engine.DevicePlan(P, M)
        plan.run(0.1)
        plan.sync()
        E = plan.fetch()[0]
        dm = plan.device_matrix()
        (dmap, _, evals, info), med, mn = timed(lambda: engine.diffusion_map_of_rows(dm, return_info=True, **KW), 3 if a.chain_only else 10)
        lines.append("%s N=%4d  device chain from DeviceMatrix      %9.2f  %9.2f   Lanczos steps %d, flags %d" % (cfg, N, med, mn, info["steps"], info["flags"]))
        if not a.chain_only:
            (hmap, _, _, _), med, mn = timed(lambda: engine.diffusion_map_of_rows(E, return_info=True, **KW), 10)
            assert np.array_equal(hmap, dmap)
            lines.append("%s N=%4d  device chain from a host array      %9.2f  %9.2f" % (cfg, N, med, mn))
            X = E / E.max()
            K, med_k, mn_k = timed(lambda: R.knn_kernel(X, KW["k"], KW["epsilon"]), 3)
            (rd, _, rl), med_e, mn_e = timed(lambda: R.diffusion_map_from_kernel(K, KW["epsilon"], KW["alpha"], KW["n_evecs"]), 3)
            lines.append("%s N=%4d  host restatement: kNN kernel        %9.2f  %9.2f" % (cfg, N, med_k, mn_k))
            lines.append("%s N=%4d  host restatement: normalise + eigs  %9.2f  %9.2f   max|d lambda| vs device %.1e" %
                         (cfg, N, med_e, mn_e, np.abs(rl - evals).max()))
        plan.close()
        print("\n".join(lines[-4:] if not a.chain_only else lines[-1:]), flush=True)
    if not a.chain_only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
