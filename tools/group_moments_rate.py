#!/usr/bin/env python3
"""Times of the patient sub-group step (K12) on the device and of its restatement with numpy / pandas / scipy
(tests/limma_restatement.py) on the same box's CPUs.

Cases cells x genes: that many float32 log1p-scale values (uniform in [0, 3): the arithmetic does not depend on them), one cell
type, 12 samples in two sub-groups.  Device parts, each a host clock around a call that ends in a device-to-host copy, after a
warm-up call of the same shape, the median of --reps: engine.group_moments with two groups from a DeviceMatrix (GB/s of Y beside
it), with transform='expm1' and one group (the HVG pass), and from a host array; tl.compute_diff_expressions end to end (upload,
HVG pass, moments of the selected genes, host tail).  Restatement: highly_variable_genes + diff_expressions (two-pass moments,
lstsq on the explicit design), once.  Also prints the largest relative |device - restatement| of logFC and t.  Writes
OUT/group_moments_rate.txt (--out, default profiles/group_moments/)."""
import argparse
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_moments"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="200000x2000")
    ap.add_argument("--no-restatement", action="store_true")
    a = ap.parse_args()
    import limma_restatement as LR
    from subgroup_helpers import Cohort
    from pilot_amd import _lib, engine, tl
    if _lib.device_count() < 1:
        raise SystemExit("group_moments_rate.py needs a HIP device: there is no CPU path to time")
    os.makedirs(a.out, exist_ok=True)
    lines = ["device: %s" % _lib.device_name()]
    for case in a.cases.split(","):
        n, G = (int(v) for v in case.split("x"))
        rng = np.random.default_rng(n + G)
        X = rng.random((n, G), dtype=np.float32) * np.float32(3.0)
        samples = np.array(["s%02d" % i for i in range(12)], dtype=object)
        sample = samples[rng.integers(0, 12, n)]
        labels = dict(zip(samples, ["Tumor 1"] * 6 + ["Tumor 2"] * 6))
        codes = np.array([0 if labels[s] == "Tumor 1" else 1 for s in sample], dtype=np.int32)
        gb = X.nbytes / 1e9
        D = engine.DeviceMatrix.upload(X)
        s_dev, _ = timed(lambda: engine.group_moments(D, codes, 2), a.reps)
        s_hvg, _ = timed(lambda: engine.group_moments(D, np.zeros(n, dtype=np.int32), 1, transform="expm1"), a.reps)
        s_host, _ = timed(lambda: engine.group_moments(X, codes, 2), max(1, a.reps // 2))
        del D
        adata = Cohort(X, pd.DataFrame({"cell_types": np.full(n, "alpha", dtype=object), "sampleID": sample}), ["g%d" % j for j in range(G)])
        props = pd.DataFrame({"sampIeD": samples, "Predicted_Labels": [labels[s] for s in samples]})
        top = min(2000, G)
        s_de, res = timed(lambda: tl.compute_diff_expressions(adata, "alpha", props, n_top_genes=top), max(1, a.reps // 2))
        lines.append("cells=%d genes=%d (%.2f GB f32) DEVICE: group_moments, 2 groups, %.2f ms from HBM (%.0f GB/s of Y); expm1, 1 group, "
                     "%.2f ms (%.0f GB/s); 2 groups from a host array %.1f ms; compute_diff_expressions (n_top_genes=%d, %d genes kept) %.2f s"
                     % (n, G, gb, s_dev * 1e3, gb / s_dev, s_hvg * 1e3, gb / s_hvg, s_host * 1e3, top, len(res), s_de))
        print(lines[-1], flush=True)
        if not a.no_restatement:
            t0 = time.perf_counter()
            keep = np.flatnonzero(LR.highly_variable_genes(X, top)["highly_variable"].values)
            c_hvg = time.perf_counter() - t0
            lab = np.array([labels[s] for s in sample], dtype=object)
            t0 = time.perf_counter()
            want = LR.diff_expressions(X[:, keep], lab, "Tumor 1", "Tumor 2", "reference")
            c_de = time.perf_counter() - t0
            same = len(keep) == len(res) and list(res.index) == [adata.var_names[j] for j in keep]
            err = (float(np.max(np.abs(res["logFC"].values - want["logFC"]) / np.abs(want["logFC"]))),
                   float(np.max(np.abs(res["t"].values - want["t"]) / np.abs(want["t"])))) if same else (np.nan, np.nan)
            lines.append("cells=%d genes=%d RESTATEMENT: highly_variable_genes %.1f s; lmFit (lstsq) + eBayes %.1f s; sum %.1f s.  same genes: "
                         "%s; max rel |device - restatement|: logFC %.2e, t %.2e" % (n, G, c_hvg, c_de, c_hvg + c_de, same, err[0], err[1]))
            print(lines[-1], flush=True)
    with open(os.path.join(a.out, "group_moments_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
