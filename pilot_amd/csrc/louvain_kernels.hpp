// K17: synchronous Louvain on the symmetric graph S = A + A^T of one level (CSR, the columns of a row ascending and distinct, the
// diagonal allowed) with the directed node weights out / in; host side: pilot_ot_louvain.hip; the rule: DESIGN.md K17, restated in
// tests/louvain_restatement.py.
//
// A sweep reads one snapshot (comm, Out, In, size) and writes next[]: node i in X takes, for every community C != X that holds a
// stored neighbour j != i, k_C = the sum of S_ij over those neighbours IN THE ROW'S STORED ORDER (k_X alike, 0 without one) and
//     g(C) = w (k_C - k_X) - gamma (out_i (In_C - (In_X - in_i)) + in_i (Out_C - (Out_X - out_i)))
// with every product and sum rounded on its own (__dmul_rn / __dadd_rn: the build contracts a * b + c otherwise).  Largest g, ties
// to the lowest C; the node moves iff g > 0, and a singleton never moves to a singleton of higher id.
//
// Three move kernels by degree d of the node (limits: LV_WAVE_MAX, LV_WG_MAX, lowered by the test switch PILOT_OT_LOUVAIN_BINS):
//   d <= 64    a wave per node: the (community, weight) pairs sit in LDS, and every lane walks all d of them in stored order adding
//              the weights of its own pair's community -- the sum a stable sort by community followed by an in-order walk of the
//              run gives, without the sort;
//   d <= 8192  a workgroup per node: the pairs are staged in LDS as 64-bit keys (community << 32 | position) plus the weights,
//              16 B a neighbour padded to a power of two, so 8192 neighbours = 128 KiB of the CU's 160 KiB; a bitonic sort of the
//              keys (distinct, so the order is the stable one), then the lane that finds a run's head walks the run in order;
//   longer     a workgroup per node straight from HBM, quadratic in d: correct, not fast (coarse levels can reach d = m - 1).
// Nothing here depends on the launch geometry: a node's result is a function of the snapshot alone.  The only atomics are integer
// counters.  Every other sum also has one fixed order: community totals over the members ascending (lv_runs_kernel), the two sums
// of Qs in chunks of LV_CHUNK consecutive entries and then over the chunks (lv_chunk_sums_kernel, lv_qs_kernel), a coarse weight
// over its fine edges in (row, column) order (lv_coarse_edges_kernel).
//
// K20 (Leiden's refinement under the same synchronous rule; DESIGN.md K20, restated in tests/leiden_restatement.py) runs the three
// move kernels in their CONSTRAINED form, `template <bool CON>` with an LvRefine beside the snapshot: the snapshot is then the
// refinement R of the move phase's partition `parent`; a node decides only while it is a singleton of R with node_ok, any other
// writes next[i] = X; a neighbour in another parent community is staged as no neighbour; a candidate without sub_ok is skipped;
// moves are counted by ld_settle_kernel, not here.  CON = false is K17 as it was: every constrained branch is `if constexpr`.
// The small kernels of the refinement are at the end of this file.
#pragma once
#include <hip/hip_runtime.h>

#include "reduce.hpp"

namespace pilot {

constexpr int LV_WAVE_MAX = 64;        // neighbours a wave stages, one per lane
constexpr int LV_WG_MAX = 8192;        // neighbours a workgroup sorts in LDS: 16 B each, 128 KiB
constexpr int LV_THREADS = 256;
constexpr int LV_CHUNK = 256;          // the chunk of the two-stage ordered sums
constexpr int LV_MAX_SWEEPS = 128;
constexpr int LV_SORT_TILE = 2048;     // elements a workgroup of the global sort keeps in LDS (32 KiB of edge records)
constexpr int LV_SCAN_ITEMS = 8;       // entries per thread and round of the single-workgroup scan

typedef unsigned long long lv_u64;
constexpr lv_u64 LV_PAD = ~0ull;       // sorts behind every real key (communities and positions are below 2^31)

struct LvCounters {                    // what a level brings back to the host
    double qs;                         // Qs of the assignment lv_qs_kernel last judged
    int moved;                         // nodes the last sweep moved
    int n_wg, n_long, max_wg_degree;   // the level's nodes in the workgroup and the long bin
    int coarse_m, coarse_nnz;          // sizes of the aggregated graph
    int pad;
};

struct LvGraph {
    const int *indptr, *col;
    const double *val, *out, *in;
    int m;
};
struct LvState {                       // the snapshot of a sweep
    const int *comm;
    const double *Out, *In;
    const int *size;
};
struct LvRefine {                      // K20: what constrains a sweep of the refinement (unread when CON = false)
    const int *parent;                 // the move phase's community of every node
    const int *node_ok, *sub_ok;       // per node, fixed for the level; per sub-community id, of this snapshot
};
struct LvEdge {                        // an edge of the aggregation's sort: (coarse row << 32 | coarse column, fine edge index)
    lv_u64 key, e;
};

__device__ inline void *lv_dyn_lds() {
    extern __shared__ lv_u64 lv_lds_raw[];
    return lv_lds_raw;
}

__device__ inline double lv_gain(double w, double gamma, double kC, double kX, double out_i, double in_i, double OutC, double InC,
                                 double OutX, double InX) {
    const double a = __dmul_rn(out_i, __dadd_rn(InC, -__dadd_rn(InX, -in_i)));
    const double b = __dmul_rn(in_i, __dadd_rn(OutC, -__dadd_rn(OutX, -out_i)));
    return __dadd_rn(__dmul_rn(w, __dadd_rn(kC, -kX)), -__dmul_rn(gamma, __dadd_rn(a, b)));
}
// is candidate (g1, c1) ahead of (g2, c2)?  c < 0: no candidate
__device__ inline bool lv_better(double g1, int c1, double g2, int c2) { return c1 >= 0 && (c2 < 0 || g1 > g2 || (g1 == g2 && c1 < c2)); }
struct LvTake {       // the (value, index) order of reduce.hpp's pair reductions
    __device__ void operator()(double g2, int c2, double &g, int &C) const {
        if (lv_better(g2, c2, g, C)) { g = g2; C = c2; }
    }
};

template <bool CON> __device__ inline void lv_decide(int i, int X, double g, int C, const int *size, int *next, LvCounters *cnt) {
    const bool move = C >= 0 && g > 0.0 && !(size[X] == 1 && size[C] == 1 && C > X);
    next[i] = move ? C : X;
    if constexpr (!CON)
        if (move) atomicAdd(&cnt->moved, 1);
}
// K20: may node i of sub-community X decide in this sweep?
__device__ inline bool lv_decides(const LvRefine &R, int i, int X, const int *size) { return size[X] == 1 && R.node_ok[i] != 0; }

__global__ void lv_iota_kernel(int *x, int n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = (int)i;
}

// the level's nodes beyond the wave bin, listed by bin (the order of a list is not fixed and nothing depends on it)
__global__ void lv_bin_kernel(const int *indptr, int m, int wave_max, int wg_max, int *wg_list, int *long_list, LvCounters *cnt) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int d = indptr[i + 1] - indptr[i];
    if (d > wg_max) long_list[atomicAdd(&cnt->n_long, 1)] = (int)i;
    else if (d > wave_max) {
        wg_list[atomicAdd(&cnt->n_wg, 1)] = (int)i;
        atomicMax(&cnt->max_wg_degree, d);
    }
}

// ---- the move kernels ---------------------------------------------------------------------------------------------------------
// four nodes per workgroup, a wave each; a node of another bin is left to that bin's kernel
template <bool CON>
__global__ __launch_bounds__(LV_THREADS) void lv_move_wave_kernel(LvGraph G, LvState S, LvRefine R, double w, double gamma, int wave_max,
                                                                  int *next, LvCounters *cnt) {
    __shared__ int s_c[LV_THREADS / 64][64];
    __shared__ double s_v[LV_THREADS / 64][64];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long node = (long)blockIdx.x * (LV_THREADS / 64) + wv;
    int d = -1, e0 = 0;
    if (node < G.m) {
        e0 = G.indptr[node];
        d = G.indptr[node + 1] - e0;
    }
    const bool mine = d >= 0 && d <= wave_max;
    int c = -1;
    double v = 0.0;
    if (mine && lane < d) {
        const int j = G.col[e0 + lane];
        v = G.val[e0 + lane];
        c = j == node ? -1 : S.comm[j];
        if constexpr (CON)
            if (R.parent[j] != R.parent[node]) c = -1;
    }
    s_c[wv][lane] = c;
    s_v[wv][lane] = v;
    __syncthreads();
    if (!mine) return;
    const int i = (int)node, X = S.comm[i];
    if constexpr (CON)
        if (!lv_decides(R, i, X, S.size)) {                                    // (the whole wave leaves: one node per wave)
            if (lane == 0) next[i] = X;
            return;
        }
    double kC = 0.0, kX = 0.0;
    for (int q = 0; q < d; ++q) {
        const int cq = s_c[wv][q];
        const double vq = s_v[wv][q];
        if (cq == c) kC = __dadd_rn(kC, vq);
        if (cq == X) kX = __dadd_rn(kX, vq);
    }
    int C = (c >= 0 && c != X) ? c : -1;
    if constexpr (CON)
        if (C >= 0 && !R.sub_ok[C]) C = -1;
    double g = C >= 0 ? lv_gain(w, gamma, kC, kX, G.out[i], G.in[i], S.Out[C], S.In[C], S.Out[X], S.In[X]) : 0.0;
    lanes_best(g, C, LvTake{});
    if (lane == 0) lv_decide<CON>(i, X, g, C, S.size, next, cnt);
}

// the workgroup's best candidate, then the decision
template <bool CON> __device__ inline void lv_reduce_decide(int i, int X, double g, int C, const int *size, int *next, LvCounters *cnt) {
    __shared__ double r_g[LV_THREADS];
    __shared__ int r_c[LV_THREADS];
    const int tid = threadIdx.x;
    r_g[tid] = g;
    r_c[tid] = C;
    __syncthreads();
    tree_best<LV_THREADS>(r_g, r_c, LvTake{});
    if (tid == 0) lv_decide<CON>(i, X, r_g[0], r_c[0], size, next, cnt);
}

// a workgroup per listed node; dynamic LDS: 16 B x (the list's largest degree padded to a power of two)
template <bool CON>
__global__ __launch_bounds__(LV_THREADS) void lv_move_wg_kernel(LvGraph G, LvState S, LvRefine R, double w, double gamma, const int *list,
                                                                int *next, LvCounters *cnt) {
    __shared__ double s_kX;
    const int tid = threadIdx.x;
    const int i = list[blockIdx.x], e0 = G.indptr[i], d = G.indptr[i + 1] - e0, X = S.comm[i];
    if constexpr (CON)
        if (!lv_decides(R, i, X, S.size)) {                                    // (the whole workgroup leaves, before any barrier)
            if (tid == 0) next[i] = X;
            return;
        }
    int P = 2;
    while (P < d) P <<= 1;
    lv_u64 *keys = static_cast<lv_u64 *>(lv_dyn_lds());
    double *vals = reinterpret_cast<double *>(keys + P);
    for (int p = tid; p < P; p += LV_THREADS) {
        lv_u64 key = LV_PAD;
        if (p < d) {
            const int j = G.col[e0 + p];
            vals[p] = G.val[e0 + p];
            bool neighbour = j != i;
            if constexpr (CON) neighbour = neighbour && R.parent[j] == R.parent[i];
            if (neighbour) key = ((lv_u64)S.comm[j] << 32) | (lv_u64)p;
        }
        keys[p] = key;
    }
    if (tid == 0) s_kX = 0.0;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += LV_THREADS) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const lv_u64 a = keys[lo], b = keys[hi];
                if ((a > b) == ((lo & k) == 0)) { keys[lo] = b; keys[hi] = a; }
            }
            __syncthreads();
        }
    // a run's head walks the run: first the run of X, then, with k_X known, every other
    double g = 0.0;
    int C = -1;
    for (int phase = 0; phase < 2; ++phase) {
        for (int p = tid; p < d; p += LV_THREADS) {
            const lv_u64 key = keys[p];
            if (key == LV_PAD) continue;
            const lv_u64 ck = key >> 32;
            if (((int)ck == X) != (phase == 0)) continue;
            if (p > 0 && (keys[p - 1] >> 32) == ck) continue;
            if constexpr (CON)
                if (!R.sub_ok[(int)ck]) continue;
            double k = 0.0;
            for (int q = p; q < d && (keys[q] >> 32) == ck; ++q) k = __dadd_rn(k, vals[(int)(keys[q] & 0xffffffffu)]);
            if (phase == 0) s_kX = k;
            else {
                const int c = (int)ck;
                const double gc = lv_gain(w, gamma, k, s_kX, G.out[i], G.in[i], S.Out[c], S.In[c], S.Out[X], S.In[X]);
                if (lv_better(gc, c, g, C)) { g = gc; C = c; }
            }
        }
        __syncthreads();
    }
    lv_reduce_decide<CON>(i, X, g, C, S.size, next, cnt);
}

// a workgroup per listed node, the neighbours' communities staged in HBM (ecomm, the node's own stretch of an nnz-long array); the
// first entry of a community in the row walks the rest of the row for it: O(d^2 / 256) per lane
template <bool CON>
__global__ __launch_bounds__(LV_THREADS) void lv_move_long_kernel(LvGraph G, LvState S, LvRefine R, double w, double gamma, const int *list,
                                                                  int *ecomm, int *next, LvCounters *cnt) {
    __shared__ double s_kX;
    const int tid = threadIdx.x;
    const int i = list[blockIdx.x], e0 = G.indptr[i], d = G.indptr[i + 1] - e0, X = S.comm[i];
    if constexpr (CON)
        if (!lv_decides(R, i, X, S.size)) {
            if (tid == 0) next[i] = X;
            return;
        }
    int *ec = ecomm + e0;
    const double *val = G.val + e0;
    for (int p = tid; p < d; p += LV_THREADS) {
        const int j = G.col[e0 + p];
        int c = j == i ? -1 : S.comm[j];
        if constexpr (CON)
            if (R.parent[j] != R.parent[i]) c = -1;
        ec[p] = c;
    }
    if (tid == 0) s_kX = 0.0;
    __syncthreads();
    double g = 0.0;
    int C = -1;
    for (int phase = 0; phase < 2; ++phase) {
        for (int p = tid; p < d; p += LV_THREADS) {
            const int c = ec[p];
            if (c < 0 || (c == X) != (phase == 0)) continue;
            if constexpr (CON)
                if (!R.sub_ok[c]) continue;
            bool head = true;
            for (int q = 0; q < p; ++q)
                if (ec[q] == c) { head = false; break; }
            if (!head) continue;
            double k = 0.0;
            for (int q = p; q < d; ++q)
                if (ec[q] == c) k = __dadd_rn(k, val[q]);
            if (phase == 0) s_kX = k;
            else {
                const double gc = lv_gain(w, gamma, k, s_kX, G.out[i], G.in[i], S.Out[c], S.In[c], S.Out[X], S.In[X]);
                if (lv_better(gc, c, g, C)) { g = gc; C = c; }
            }
        }
        __syncthreads();
    }
    lv_reduce_decide<CON>(i, X, g, C, S.size, next, cnt);
}

// ---- a bitonic sort in HBM of P = 2^x elements with distinct keys (pads excepted), ascending -------------------------------------------
__device__ inline bool lv_gt(lv_u64 a, lv_u64 b) { return a > b; }
__device__ inline bool lv_gt(const LvEdge &a, const LvEdge &b) { return a.key > b.key || (a.key == b.key && a.e > b.e); }

// one compare-exchange step (k, j) over the whole array: thread t < P / 2
template <typename T> __global__ void lv_bitonic_global_kernel(T *a, long half, long k, long j) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= half) return;
    const long lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
    const T x = a[lo], y = a[hi];
    if (lv_gt(x, y) == ((lo & k) == 0)) { a[lo] = y; a[hi] = x; }
}
// every step with j < tile of the merges k_lo .. k_hi, a tile of `tile` consecutive elements per workgroup in LDS
template <typename T> __global__ __launch_bounds__(LV_THREADS) void lv_bitonic_tile_kernel(T *a, int tile, long k_lo, long k_hi) {
    T *s = static_cast<T *>(lv_dyn_lds());
    const long base = (long)blockIdx.x * tile;
    for (int p = threadIdx.x; p < tile; p += LV_THREADS) s[p] = a[base + p];
    __syncthreads();
    for (long k = k_lo; k <= k_hi; k <<= 1)
        for (int j = (int)((k >> 1) < (long)(tile >> 1) ? (k >> 1) : (long)(tile >> 1)); j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (tile >> 1); t += LV_THREADS) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const T x = s[lo], y = s[hi];
                if (lv_gt(x, y) == (((base + lo) & k) == 0)) { s[lo] = y; s[hi] = x; }
            }
            __syncthreads();
        }
    for (int p = threadIdx.x; p < tile; p += LV_THREADS) a[base + p] = s[p];
}

// exclusive scan of n ints by ONE workgroup of 1024 threads; *total = their sum
__global__ __launch_bounds__(1024) void lv_scan_kernel(const int *flag, int *pos, long n, int *total) {
    __shared__ int s[1024];
    const int tid = threadIdx.x;
    int carry = 0;
    for (long base = 0; base < n; base += 1024 * LV_SCAN_ITEMS) {
        const long b = base + (long)tid * LV_SCAN_ITEMS;
        int v[LV_SCAN_ITEMS], sum = 0;
        for (int k = 0; k < LV_SCAN_ITEMS; ++k) {
            v[k] = b + k < n ? flag[b + k] : 0;
            sum += v[k];
        }
        s[tid] = sum;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int t = tid >= off ? s[tid - off] : 0;
            __syncthreads();
            s[tid] += t;
            __syncthreads();
        }
        int excl = s[tid] - sum + carry;
        for (int k = 0; k < LV_SCAN_ITEMS; ++k)
            if (b + k < n) {
                pos[b + k] = excl;
                excl += v[k];
            }
        carry += s[1023];
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

// ---- community totals and Qs of an assignment -------------------------------------------------------------------------------------
__global__ void lv_node_keys_kernel(const int *comm, int m, long P, lv_u64 *keys) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < P) keys[t] = t < m ? (((lv_u64)comm[t] << 32) | (lv_u64)t) : LV_PAD;
}
// keys sorted: the members of a community are adjacent, ascending; the thread at a run's head adds them in that order.  Out, In and
// size were zeroed: a community without members keeps 0.
__global__ void lv_runs_kernel(const lv_u64 *keys, int m, const double *out, const double *in, double *Out, double *In, int *size) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const lv_u64 ck = keys[p] >> 32;
    if (p > 0 && (keys[p - 1] >> 32) == ck) return;
    double so = 0.0, si = 0.0;
    int n = 0;
    for (long q = p; q < m && (keys[q] >> 32) == ck; ++q, ++n) {
        const int id = (int)(keys[q] & 0xffffffffu);
        so = __dadd_rn(so, out[id]);
        si = __dadd_rn(si, in[id]);
    }
    Out[ck] = so;
    In[ck] = si;
    size[ck] = n;
}
// internal[i] = the stored S_ij of row i (the diagonal included) inside i's community, in stored order; prod[c] = Out_c In_c
__global__ void lv_internal_kernel(LvGraph G, const int *comm, const double *Out, const double *In, double *internal, double *prod) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G.m) return;
    const int ci = comm[i];
    double s = 0.0;
    for (int e = G.indptr[i]; e < G.indptr[i + 1]; ++e)
        if (comm[G.col[e]] == ci) s = __dadd_rn(s, G.val[e]);
    internal[i] = s;
    prod[i] = __dmul_rn(Out[i], In[i]);
}
// part_x[c] = x[256 c] + x[256 c + 1] + ..., one thread per chunk, for both arrays
__global__ void lv_chunk_sums_kernel(const double *x, const double *y, int n, double *part_x, double *part_y) {
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long b = c * LV_CHUNK;
    if (b >= n) return;
    const long e = b + LV_CHUNK < n ? b + LV_CHUNK : n;
    double sx = 0.0, sy = 0.0;
    for (long q = b; q < e; ++q) {
        sx = __dadd_rn(sx, x[q]);
        sy = __dadd_rn(sy, y[q]);
    }
    part_x[c] = sx;
    part_y[c] = sy;
}
// Qs = (w / 2) sum(internal) - gamma sum(prod), the chunk sums added in ascending order by one thread
__global__ void lv_qs_kernel(const double *part_x, const double *part_y, int chunks, double w, double gamma, LvCounters *cnt) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double sx = 0.0, sy = 0.0;
    for (int c = 0; c < chunks; ++c) {
        sx = __dadd_rn(sx, part_x[c]);
        sy = __dadd_rn(sy, part_y[c]);
    }
    cnt->qs = __dadd_rn(__dmul_rn(__dmul_rn(w, 0.5), sx), -__dmul_rn(gamma, sy));
}

// ---- aggregation ------------------------------------------------------------------------------------------------------------------
__global__ void lv_alive_kernel(const int *size, int m, int *flag) {
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m) flag[c] = size[c] > 0 ? 1 : 0;
}
// the coarse index of every ORIGINAL node: label[i] is its node of this level
__global__ void lv_relabel_kernel(int *label, int n, const int *comm, const int *rank) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) label[i] = rank[comm[label[i]]];
}
__global__ void lv_coarse_nodes_kernel(int m, const int *size, const int *rank, const double *Out, const double *In, double *out2, double *in2) {
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m && size[c] > 0) {
        out2[rank[c]] = Out[c];
        in2[rank[c]] = In[c];
    }
}
// one record per fine edge, the pads behind them up to P
__global__ void lv_edge_keys_kernel(LvGraph G, const int *comm, const int *rank, int nnz, long P, LvEdge *keys) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < G.m) {
        const lv_u64 cu = (lv_u64)rank[comm[t]] << 32;
        for (int e = G.indptr[t]; e < G.indptr[t + 1]; ++e) keys[e] = LvEdge{cu | (lv_u64)rank[comm[G.col[e]]], (lv_u64)e};
    }
    if (t < P - nnz) keys[nnz + t] = LvEdge{LV_PAD, LV_PAD};
}
__global__ void lv_edge_heads_kernel(const LvEdge *keys, int nnz, int *flag) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < nnz) flag[p] = (p == 0 || keys[p - 1].key != keys[p].key) ? 1 : 0;
}
// records sorted by (coarse row, coarse column, fine edge): the thread at a run's head adds the run's weights in that order and
// writes the coarse entry; the first head of a coarse row also writes the row pointers up to it, the last record those behind it
__global__ void lv_coarse_edges_kernel(const LvEdge *keys, int nnz, const int *flag, const int *pos, const double *val, int m2,
                                       const int *total, int *indptr2, int *col2, double *val2) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const lv_u64 key = keys[p].key;
    const int cu = (int)(key >> 32);
    if (flag[p]) {
        double s = 0.0;
        for (long q = p; q < nnz && keys[q].key == key; ++q) s = __dadd_rn(s, val[keys[q].e]);
        const int o = pos[p];
        col2[o] = (int)(key & 0xffffffffu);
        val2[o] = s;
        const int prev = p == 0 ? -1 : (int)(keys[p - 1].key >> 32);
        for (int r = prev + 1; r <= cu; ++r) indptr2[r] = o;
    }
    if (p == nnz - 1)
        for (int r = cu + 1; r <= m2; ++r) indptr2[r] = *total;
}

// ---- K20: the small kernels of the refinement (the sweep itself: the move kernels above with CON = true) -----------------------------
// is w x - gamma (o (InP - i) + n (OutP - o_)) >= 0, every product and sum rounded on its own, in the order written
__device__ inline bool ld_well_connected(double w, double gamma, double x, double o, double n, double OutP, double InP) {
    const double a = __dmul_rn(o, __dadd_rn(InP, -n));
    const double b = __dmul_rn(n, __dadd_rn(OutP, -o));
    return __dadd_rn(__dmul_rn(w, x), -__dmul_rn(gamma, __dadd_rn(a, b))) >= 0.0;
}
// fixed for the level: e_i = the stored S_ij, j != i, inside i's parent community in stored order, and node_ok_i from it
__global__ void ld_node_ok_kernel(LvGraph G, const int *parent, const double *OutP, const double *InP, double w, double gamma, int *node_ok) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G.m) return;
    const int X = parent[i];
    double e_i = 0.0;
    for (int e = G.indptr[i]; e < G.indptr[i + 1]; ++e) {
        const int j = G.col[e];
        if (j != i && parent[j] == X) e_i = __dadd_rn(e_i, G.val[e]);
    }
    node_ok[i] = ld_well_connected(w, gamma, e_i, G.out[i], G.in[i], OutP[X], InP[X]) ? 1 : 0;
}
// per snapshot: c_i = the stored S_ij, j != i, inside i's parent community and outside i's sub-community, in stored order
__global__ void ld_cut_kernel(LvGraph G, const int *parent, const int *sub, double *c) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G.m) return;
    const int X = parent[i], T = sub[i];
    double s = 0.0;
    for (int e = G.indptr[i]; e < G.indptr[i + 1]; ++e) {
        const int j = G.col[e];
        if (j != i && parent[j] == X && sub[j] != T) s = __dadd_rn(s, G.val[e]);
    }
    c[i] = s;
}
// keys: the snapshot's node keys sorted (sub-community << 32 | node), as lv_runs_kernel reads them; cut[T]: lv_runs_kernel's sum of c
// over T's members.  The thread at a run's head writes sub_ok[T] and, for a T of one member, owner[T]: one writer per entry.  An id
// without members keeps what the arrays held; nothing reads those.
__global__ void ld_sub_ok_kernel(const lv_u64 *keys, int m, const int *parent, const double *OutP, const double *InP, LvState S,
                                 const double *cut, double w, double gamma, int *sub_ok, int *owner) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const lv_u64 ck = keys[p] >> 32;
    if (p > 0 && (keys[p - 1] >> 32) == ck) return;
    const int T = (int)ck, member = (int)(keys[p] & 0xffffffffu), X = parent[member];
    sub_ok[T] = ld_well_connected(w, gamma, cut[T], S.Out[T], S.In[T], OutP[X], InP[X]) ? 1 : 0;
    if (S.size[T] == 1) owner[T] = member;
}
// raw: the sweep's unsettled decisions.  A move into a sub-community of one member stands only if that member did not itself
// decide to leave; next is a separate array (settling in place would race with the reads of raw); counts the moves that stand
__global__ void ld_settle_kernel(int m, const int *sub, const int *size, const int *owner, const int *raw, int *next, LvCounters *cnt) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int X = sub[i];
    int T = raw[i];
    if (T != X && size[T] == 1) {
        const int j = owner[T];
        if (raw[j] != sub[j]) T = X;
    }
    next[i] = T;
    if (T != X) atomicAdd(&cnt->moved, 1);
}

}  // namespace pilot
