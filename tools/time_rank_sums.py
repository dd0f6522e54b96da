#!/usr/bin/env python3
"""Time of the device rank sums (K21, engine.DeviceCSR.rank_sums) beside DeviceCSR.group_sums on the same handle, and beside
scipy.stats.rankdata on the host.

Matrix: tools/time_pca.py's synthetic float32 CSR (cells x 2 000 genes at 10 % fill, 50-factor gamma model), normalize_log1p'd
on the device, 32 random groups; --cells takes several sizes (default 50 000 and 200 000).  Device: after one warm-up call of
each, ``rank_sums`` and ``group_sums`` alternate in one process, the host clock around each call (both end in device-to-host
copies), best of --reps.  ``group_sums`` is a streaming pass over the same stored entries, so it is the yardstick.  Floor: the
column form read once (12 B per stored entry: value, row, and the row's code at 4 B) plus the sort records written and read once
(2 x 8 B per non-zero entry for float32) at 6.3 TB/s; the ratio to it is stated, and the bins the columns fall into.  Host (--host,
at the last size): ``scipy.stats.rankdata(axis=0)`` on the dense copy of 200 of the columns, one thread, scaled by genes / 200 and
reported as such.  Writes OUT/rank_sums_rate.txt (--out, default profiles/rank_sums/)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

COPY_RATE = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_sums"))
    ap.add_argument("--cells", type=int, nargs="+", default=[50000, 200000])
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--fill", type=float, default=0.10)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", action="store_true", help="also time scipy.stats.rankdata on 200 dense columns of the last size")
    a = ap.parse_args()
    from scipy.stats import rankdata
    from time_pca import synthetic
    from pilot_amd import _lib, engine

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    w, W, T = engine.rank_sums_limits()
    say("%s; bins: wave <= %d, workgroup <= %d, sort tile %d; %s" % (_lib.device_name(), w, W, T, time.strftime("%Y-%m-%d")))
    for n in a.cells:
        t0 = time.perf_counter()
        X = synthetic(n, a.genes, 50, a.fill, 0)
        codes = np.random.default_rng(1).integers(0, a.groups, n).astype(np.int32)
        S = engine.DeviceCSR.upload(X).normalize_log1p(1e4)
        S.build_columns()
        nz = S.column_nnz()
        say("case %d x %d float32 CSR, %d stored (fill %.3f), %d groups; built and uploaded in %.1f s"
            % (n, a.genes, X.nnz, X.nnz / np.prod(X.shape), a.groups, time.perf_counter() - t0))
        say("  columns by non-zero entries: %d wave, %d workgroup, %d long (median %d, max %d)"
            % ((nz <= w).sum(), ((nz > w) & (nz <= W)).sum(), (nz > W).sum(), np.median(nz), nz.max()))

        def timed(fn):
            t = time.perf_counter()
            out = fn(codes, a.groups)
            return time.perf_counter() - t, out

        timed(S.rank_sums)
        timed(S.group_sums)
        best = {"rank": np.inf, "sums": np.inf}
        for _ in range(a.reps):                                    # the compared calls alternate
            t, ranks = timed(S.rank_sums)
            best["rank"] = min(best["rank"], t)
            t, _ = timed(S.group_sums)
            best["sums"] = min(best["sums"], t)
        N = n
        assert (ranks[1].sum(axis=0) == N * (N + 1) / 2).all() and ranks[0].sum() == N
        floor = (12.0 * X.nnz + 16.0 * nz.sum()) / COPY_RATE
        say("  rank_sums %.2f ms, group_sums %.2f ms (best of %d, alternating): %.1f x the streaming pass; floor (column form read "
            "once + records written and read once) %.3f ms: rank_sums is %.0f x its floor"
            % (1e3 * best["rank"], 1e3 * best["sums"], a.reps, best["rank"] / best["sums"], 1e3 * floor, best["rank"] / floor))
        if a.host and n == a.cells[-1]:
            k = min(200, a.genes)
            Y = engine.download(S.densify(np.arange(k, dtype=np.int32)))
            t0 = time.perf_counter()
            rankdata(Y, axis=0)
            t_host = time.perf_counter() - t0
            say("  host: scipy.stats.rankdata(axis=0) on the dense copy of %d columns %.2f s; scaled by %d / %d: %.1f s for the "
                "ranking alone (one thread)" % (k, t_host, a.genes, k, t_host * a.genes / k))
        del S
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "rank_sums_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
