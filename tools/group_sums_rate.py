#!/usr/bin/env python3
"""Times of the pseudobulk grouped sum (K14) on the device and of pandas' groupby().sum() on the dense matrix on the same box's CPUs.

Dense case cells x genes (default 200000x2000): float32 counts resident in HBM as a DeviceMatrix, --groups (600) groups of unequal
size.  Sparse case (default 100000x20000 at --fill 0.05): a DeviceCSR with exactly fill * genes stored counts per row.  Each device
time is a host clock around engine.group_sums -- the row lists made on the host, their upload, the kernels and the download of the
groups x genes float64 result -- after a warm-up call of the same shape, the median of --reps.  Beside it the read-once floor: the
bytes the kernels must read (the dense matrix; indices and values of the sparse one) at 6.3 TB/s.  Kernel times come from a
separate run of this tool under a kernel trace (--no-pandas --reps 1).  pandas: DataFrame(X).groupby(codes).sum() on the dense
float32 matrix (the sparse case's dense copy included, 8 GB at the default shape; --no-pandas skips both), once.  Also checks that
the device sums of the integer counts equal pandas' wherever both ran.  Writes OUT/group_sums_rate.txt (--out, default
profiles/pseudobulk/)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def group_codes(rng, n, n_groups):
    """unequal groups: sizes follow a gamma law, every group has at least one row"""
    p = rng.gamma(2.0, 1.0, n_groups)
    codes = rng.choice(n_groups, n, p=p / p.sum()).astype(np.int32)
    codes[:n_groups] = np.arange(n_groups)
    return codes


def pandas_sums(X, codes, n_groups):
    import pandas as pd
    t0 = time.perf_counter()
    out = pd.DataFrame(X).groupby(codes, sort=True).sum()
    s = time.perf_counter() - t0
    assert len(out) == n_groups
    return s, out.to_numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pseudobulk"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense", default="200000x2000")
    ap.add_argument("--sparse", default="100000x20000")
    ap.add_argument("--fill", type=float, default=0.05)
    ap.add_argument("--groups", type=int, default=600)
    ap.add_argument("--no-pandas", action="store_true")
    a = ap.parse_args()
    import scipy.sparse as sp
    from pilot_amd import _lib, engine
    if _lib.device_count() < 1:
        raise SystemExit("group_sums_rate.py needs a HIP device: there is no CPU path to time")
    os.makedirs(a.out, exist_ok=True)
    lines = ["device: %s; slice rows %d, column block %d" % (_lib.device_name(), engine.group_sums_slice_rows(), engine.group_sums_col_block())]

    n, G = (int(v) for v in a.dense.split("x"))
    rng = np.random.default_rng(n + G)
    X = rng.poisson(2.0, (n, G)).astype(np.float32)
    codes = group_codes(rng, n, a.groups)
    D = engine.DeviceMatrix.upload(X)
    s_dev, got = timed(lambda: engine.group_sums(D, codes, a.groups), a.reps)
    del D
    floor = X.nbytes / HBM_BYTES_PER_S
    lines.append("DENSE cells=%d genes=%d (%.2f GB f32), %d groups: group_sums from HBM %.2f ms by the host clock (%.0f GB/s of Y; read-once "
                 "floor %.3f ms)" % (n, G, X.nbytes / 1e9, a.groups, s_dev * 1e3, X.nbytes / 1e9 / s_dev, floor * 1e3))
    print(lines[-1], flush=True)
    if not a.no_pandas:
        s_pd, want = pandas_sums(X, codes, a.groups)
        lines.append("DENSE pandas groupby().sum() on the same matrix: %.2f s (%.0f x the device call); sums equal: %s"
                     % (s_pd, s_pd / s_dev, bool(np.array_equal(got[1], want.astype(np.float64)))))
        print(lines[-1], flush=True)
    del X

    n, G = (int(v) for v in a.sparse.split("x"))
    per_row = max(1, int(round(a.fill * G)))
    rng = np.random.default_rng(n + G)
    base = rng.choice(G, per_row, replace=False)
    indices = ((base[None, :] + rng.integers(0, G, (n, 1))) % G).astype(np.int32).ravel()      # distinct within a row, unsorted
    data = (rng.poisson(1.0, indices.size) + 1).astype(np.float32)
    S = sp.csr_matrix((data, indices, np.arange(n + 1, dtype=np.int64) * per_row), shape=(n, G))
    codes = group_codes(rng, n, a.groups)
    C = engine.DeviceCSR.upload(S)
    s_dev, got = timed(lambda: C.group_sums(codes, a.groups), a.reps)
    cols = np.sort(rng.choice(G, min(2000, G), replace=False)).astype(np.int32)
    s_sel, _ = timed(lambda: C.group_sums(codes, a.groups, cols=cols), a.reps)
    del C
    read = indices.nbytes + data.nbytes
    lines.append("SPARSE cells=%d genes=%d, %d stored per row (%.2f GB of indices and values), %d groups: group_sums %.2f ms by the host "
                 "clock, of which the %d x %d float64 result's download is %.0f MB (%.0f GB/s of the entries; read-once floor %.3f ms); "
                 "%d selected genes: %.2f ms" % (n, G, per_row, read / 1e9, a.groups, s_dev * 1e3, a.groups, G, a.groups * G * 8 / 1e6,
                                                read / 1e9 / s_dev, read / HBM_BYTES_PER_S * 1e3, cols.size, s_sel * 1e3))
    print(lines[-1], flush=True)
    if not a.no_pandas:
        t0 = time.perf_counter()
        Y = S.toarray()
        s_dense = time.perf_counter() - t0
        s_pd, want = pandas_sums(Y, codes, a.groups)
        lines.append("SPARSE pandas on the dense copy (%.1f GB f32; toarray() %.1f s, not counted): groupby().sum() %.2f s (%.0f x the device "
                     "call); sums equal: %s" % (Y.nbytes / 1e9, s_dense, s_pd, s_pd / s_dev, bool(np.array_equal(got[1], want.astype(np.float64)))))
        print(lines[-1], flush=True)
    with open(os.path.join(a.out, "group_sums_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
