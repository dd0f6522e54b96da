#!/usr/bin/env python3
"""CPU replay of the pair-grid kernel's work queue: how many tile-updates a launch executes for a given order of the pairs.

The kernel (sinkhorn_stream_kernel) runs W waves of 16 columns.  A wave's update costs the same MFMAs whether 16
or one of its columns hold a pair, so what a launch executes is the number of (wave, update) steps in which the wave holds
any pair -- "tile-updates" -- against the ideal sum(iters) / 16.  The replay needs nothing but the update count of every pair
(`iters.npy` of `bench.py --dump-outputs DIR`, or of the oracle at the GPU's stopping floor) and an order:

  key       the kernel's own key recomputed on the host: L1-distance buckets, b = int(4 (1 - log2 |a - b|_1)) clamped to 0 .. 46,
            duplicates 47, higher buckets first, natural order inside a bucket (the device's order inside a bucket varies from
            run to run)
  natural   row-major
  dupfirst  exact duplicates first, then row-major: what is left of the key without the order pass
  perfect   longest pair first (not available before the pairs have run: the bound, not a proposal)
  a function key(P, M) -> (N, N) array, larger first (--key-func FILE.py:NAME, or replay(..., order=order_of(values)))

Queue model, as in the kernel: wave w takes batch w as its first (static) batch, later batches of 16 items come from one
counter in the order the waves ask (waves step in lockstep here, lower wave first within a step); a column that wants a pair
takes the next item of the wave's batch; when the batch has fewer items left than columns that want one, the next batch is
drawn in the same step (--late-draw: in the next step, the kernel before profiles/r08) and never earlier.

--merge-within N models a consolidated drain (not built: profiles/r09/loop_stalls.md): after the refills of a step, a wave that has
seen the queue's end hands ALL its live columns to another such wave among the N consecutive waves of its workgroup (N = 4) whenever
they fit into that wave's empty columns, the wave with the fewest live columns giving first, to the fullest wave that can take them.

Prints: tile-updates executed, the ideal, the excess, the makespan (steps until the last wave is done), the mean finish
step of a wave, and how many refills took items of two batches in one step (`spans`; 0 with --late-draw) out of how many
non-empty batches waves drew after their first (`later draws`).

  python tools/queue_replay.py ITERS.npy --config c3 --order key natural perfect
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

TILE = 16
ORDER_NB = 48


def l1_bucket_key(P, M=None):
    """The prep kernel's order key (order_tile_body): bucket number per ordered pair, f32 arithmetic."""
    P = np.asarray(P, dtype=np.float32)
    N = P.shape[0]
    key = np.empty((N, N), dtype=np.int32)
    for i in range(N):
        l1 = np.abs(P[i][None, :] - P).sum(1, dtype=np.float32)
        with np.errstate(divide="ignore"):
            v = 4.0 * (1.0 - np.log2(l1))
        b = np.where(l1 > 0, np.clip(np.nan_to_num(v, posinf=ORDER_NB - 2), 0, ORDER_NB - 2).astype(np.int32), ORDER_NB - 2)
        b[i] = ORDER_NB - 1 if l1[i] == 0 else b[i]
        key[i] = b
    return key


def order_of(values):
    """Pair numbers, larger value first, ties in natural order."""
    v = np.asarray(values).reshape(-1)
    return np.argsort(-v.astype(np.float64), kind="stable")


def replay(iters, order, n_waves=2048, late_draw=False, merge_within=0):
    """-> dict(executed, ideal, excess, makespan, mean_finish).  iters: update count per pair; order: pair numbers in queue order."""
    it = np.asarray(iters).reshape(-1).astype(np.int64)[np.asarray(order)]
    n = it.size
    n_batches = (n + TILE - 1) // TILE
    left = np.zeros((n_waves, TILE), dtype=np.int64)        # updates the column's pair still needs; 0: the column wants a pair
    nxt = np.zeros(n_waves, dtype=np.int64)                 # the wave's batch: next item, end
    end = np.zeros(n_waves, dtype=np.int64)
    first = np.ones(n_waves, dtype=bool)
    dry = np.zeros(n_waves, dtype=bool)                     # the wave has seen the queue's end
    head = min(n_waves, n_batches)                          # next batch of the counter (behind the statically dealt ones)
    finish = np.zeros(n_waves, dtype=np.int64)
    executed, step, spans, later_draws, merges = 0, 0, 0, 0, 0

    def draw(w):
        nonlocal head, later_draws
        if first[w]:
            first[w] = False
            b = w
        else:
            b = head
            head += 1
            later_draws += int(b < n_batches)
        if b >= n_batches:
            dry[w] = True
            nxt[w] = end[w] = n
        else:
            nxt[w], end[w] = b * TILE, min((b + 1) * TILE, n)

    while True:
        for w in np.nonzero((left == 0).any(1) & ~dry)[0]:
            cols = np.nonzero(left[w] == 0)[0]
            drawn = fed = False
            while cols.size and not dry[w]:
                avail = end[w] - nxt[w]
                if avail == 0:
                    if drawn:
                        break
                    draw(w)
                    drawn = True
                    continue
                k = min(avail, cols.size)
                spans += int(drawn and fed)       # this refill took items of the old batch and now takes items of the new one
                fed = True
                left[w, cols[:k]] = it[nxt[w]:nxt[w] + k]
                nxt[w] += k
                cols = cols[k:]
                if late_draw and not drawn:       # the old kernel: the batch ran out under this refill, the draw waits a step
                    break
        if merge_within > 1 and dry.any():
            live = (left > 0).sum(1)
            for g in np.unique(np.nonzero(dry & (live > 0) & (live < TILE))[0] // merge_within):
                ws = [w for w in range(g * merge_within, min((g + 1) * merge_within, n_waves)) if dry[w] and 0 < live[w] < TILE]
                for d in sorted(ws, key=lambda w: live[w]):                     # the giver: fewest live columns first
                    takers = [w for w in ws if w != d and live[w] > 0 and live[w] + live[d] <= TILE]
                    if not live[d] or not takers:
                        continue
                    t = max(takers, key=lambda w: live[w])
                    free = np.nonzero(left[t] == 0)[0][:live[d]]
                    left[t, free] = left[d][left[d] > 0]
                    left[d] = 0
                    live[t] += live[d]
                    live[d] = 0
                    merges += 1
        busy = (left > 0).any(1)
        if not busy.any():
            break
        step += 1
        executed += int(busy.sum())
        finish[busy] = step
        np.subtract(left, 1, out=left, where=left > 0)
    ideal = it.sum() / TILE
    return dict(executed=executed, ideal=float(ideal), excess=executed / ideal - 1.0, makespan=step, mean_finish=float(finish.mean()),
                spans=spans, later_draws=later_draws, merges=merges)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("iters", help="iters.npy of bench.py --dump-outputs (any shape, row-major pair numbers)")
    ap.add_argument("--config", default="c3", help="synthetic config the dump came from (for the key order)")
    ap.add_argument("--order", nargs="+", default=["key", "natural", "perfect"], choices=["key", "natural", "dupfirst", "perfect"])
    ap.add_argument("--key-func", default=None, metavar="FILE.py:NAME", help="a further order: key(P, M) -> (N, N), larger first")
    ap.add_argument("--waves", type=int, default=2048, help="waves of the launch (256 CUs x 4 SIMDs x 2)")
    ap.add_argument("--late-draw", action="store_true", help="draw a batch in the step after the one that ran out")
    ap.add_argument("--merge-within", type=int, default=0, metavar="N",
                    help="dry waves hand their live columns to another dry wave among the N waves of their workgroup (0: off)")
    args = ap.parse_args()
    iters = np.load(args.iters)
    orders = {}
    P = M = None
    if "key" in args.order or "dupfirst" in args.order or args.key_func:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
        from pilot_amd.synthetic import CONFIGS, make_problem
        P, M = make_problem(**CONFIGS[args.config])
        if P.shape[0] ** 2 != iters.size:
            sys.exit("iters holds %d pairs, config %s has %d" % (iters.size, args.config, P.shape[0] ** 2))
    for o in args.order:
        orders[o] = (order_of(l1_bucket_key(P)) if o == "key" else order_of(l1_bucket_key(P) == ORDER_NB - 1) if o == "dupfirst"
                     else np.arange(iters.size) if o == "natural" else order_of(iters))
    if args.key_func:
        path, name = args.key_func.rsplit(":", 1)
        spec = importlib.util.spec_from_file_location("queue_replay_key", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        orders[name] = order_of(getattr(mod, name)(P, M))
    it = iters.reshape(-1)
    print("%d pairs, mean %.2f updates, max %d; %d waves, draw in the %s step" % (it.size, it.mean(), it.max(), args.waves, "next" if args.late_draw else "same"))
    if args.merge_within > 1:
        print("dry waves merge within groups of %d" % args.merge_within)
    print("%-10s %12s %12s %8s %9s %12s %8s %12s %8s" % ("order", "executed", "ideal", "excess", "makespan", "mean finish", "spans", "later draws", "merges"))
    for name, order in orders.items():
        r = replay(it, order, args.waves, args.late_draw, args.merge_within)
        print("%-10s %12d %12.1f %7.2f%% %9d %12.1f %8d %12d %8d"
              % (name, r["executed"], r["ideal"], 100 * r["excess"], r["makespan"], r["mean_finish"], r["spans"], r["later_draws"], r["merges"]))


if __name__ == "__main__":
    main()
