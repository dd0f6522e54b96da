// K19: the elastic principal tree of the rows of an n x D matrix (Albergante et al., Entropy 2020) and the pseudotime along it.
// The growth of the tree (which candidates a step tries) is the host's; the device fits a batch of candidate trees to the points.
//
// A candidate is m node positions Y (m x D, f64) and an m x m spring matrix S; nothing here knows its topology.  One fit iteration:
//   pt_partition_kernel  grid (query blocks, candidates): one point per lane, the nodes swept with K16's knn_sweep (the distances
//                        are K16's: direct sums of squared differences in the element type T, against the nodes rounded to T), the
//                        argmin kept in the functor (strict <, nodes ascending: a tie goes to the lowest node).  The block then
//                        orders its lanes by node in LDS (a stable counting sort) and writes its per-node counts, its f64 sums
//                        (one add per point, ascending row) and the f64 sum of squared distances to the assigned nodes.
//   pt_finish_kernel     one workgroup per candidate: the partials added in ascending block order, (diag(cnt) / n + S) Y' = sum / n
//                        solved by Cholesky in LDS (packed lower triangle, D right-hand sides), the change against eps, Y <- Y'.
// A candidate whose change fell below eps, or whose system had a non-positive pivot, carries a state bit and the later launches
// leave at once for it.  The last pair of launches (final_pass) partitions the final Y once more and forms the energy.
// No floating-point atomics; a block's rows and the order of every sum depend on n alone, so a candidate gives the same bits alone
// and in any batch.  pt_moments_kernel / pt_reduce_kernel: the mean and centred cross-products the start of the tree takes;
// pt_projection_kernel: every point onto its nearest edge.
#pragma once
#include <hip/hip_runtime.h>

#include "knn_kernels.hpp"
#include "reduce.hpp"

namespace pilot {

constexpr int PT_MAX_M = 65;                 // nodes of a candidate: a tree of 64 peaks at 65 while it grows
constexpr int PT_MAX_D = KNN_REGQ_D;         // the point stays in registers through the sweep
constexpr int PT_MAX_QBLOCKS = 128;          // partition blocks per candidate: beyond 128 * 256 points a block takes several chunks
constexpr int PT_FIN_THREADS = 256;
constexpr int PT_CONVERGED = 1;              // == PILOT_OT_ELASTIC_CONVERGED
constexpr int PT_SINGULAR = 2;               // == PILOT_OT_ELASTIC_SINGULAR

// Candidate blockIdx.y, rows blockIdx.x * chunks * KNN_THREADS onwards (`chunks` chunks of one point per lane).  YT / Y: the
// candidates' nodes rounded to T / in f64 (m x D each, packed).  Out, for block q of candidate b with Q = gridDim.x:
// p_counts[(b Q + q) m + j], p_sums[((b Q + q) m + j) D + d], p_mse[b Q + q] (the sum, not the mean; 0 unless final_pass).
template <typename T>
__global__ __launch_bounds__(KNN_THREADS, KNN_WAVES) void pt_partition_kernel(const T *__restrict__ X, long long ld, int n, int D, int m,
                                                                   int chunks, const T *__restrict__ YT,
                                                                   const double *__restrict__ Y, const int *__restrict__ state,
                                                                   int final_pass, int *__restrict__ p_counts,
                                                                   double *__restrict__ p_sums, double *__restrict__ p_mse) {
    __shared__ __attribute__((aligned(16))) T ys[KnnTile<T>::CAP];
    __shared__ int sorted[KNN_THREADS], wcnt[KNN_THREADS / 64][PT_MAX_M], cnt[PT_MAX_M], seg[PT_MAX_M + 1];
    __shared__ double red[KNN_THREADS];
    const int b = blockIdx.y, q = blockIdx.x, tid = threadIdx.x;
    const int st = state[b];
    if ((st & PT_SINGULAR) || (!final_pass && (st & PT_CONVERGED))) return;      // the same in every lane
    const T *yt = YT + (size_t)b * m * D;
    const double *y = Y + (size_t)b * m * D;
    const size_t slot = (size_t)b * gridDim.x + q;
    int *pc = p_counts + slot * m;
    double *ps = p_sums + slot * m * D;
    double mse = 0.0;                                                            // lane 0's

    for (int c = 0; c < chunks; ++c) {
        const long long base = ((long long)q * chunks + c) * KNN_THREADS;
        if (c > 0 && base >= n) break;
        const long long row = base + tid;
        const bool active = row < n;
        const T *xq = X + (active ? row : 0) * ld;                               // an idle lane works on a valid row and keeps nothing
        T best = INFINITY;
        int arg = 0;
        knn_sweep<T, true>(yt, (long long)D, m, D, xq, ys, [&](long long j0, const T *acc) {
#pragma unroll
            for (int p = 0; p < KNN_PB; ++p) {
                const int j = (int)j0 + p;
                if (j < m && acc[p] < best) {
                    best = acc[p];
                    arg = j;
                }
            }
        });
        // the f64 squared distance to the assigned node: only the final pass reports it.  Eight loads in flight, the adds in order
        double d2 = 0.0;
        if (final_pass && active) {
            const double *ya = y + (size_t)arg * D;
            int d = 0;
            for (; d + 8 <= D; d += 8) {
                double df[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) df[u] = (double)xq[d + u] - ya[d + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) d2 = fma(df[u], df[u], d2);
            }
            for (; d < D; ++d) {
                const double df = (double)xq[d] - ya[d];
                d2 = fma(df, df, d2);
            }
        }
        red[tid] = d2;
        // the lanes ordered by (node, row), a stable counting sort: a wave's lanes of node j come from one ballot, the waves in order
        const int lane = tid & 63, w = tid >> 6, node = active ? arg : -1;
        int before = 0;                                                          // lanes of this wave below this one at the same node
        for (int j = 0; j < m; ++j) {
            const unsigned long long mask = __ballot(node == j);
            if (node == j) before = __popcll(mask & ((1ull << lane) - 1ull));
            if (lane == 0) wcnt[w][j] = __popcll(mask);
        }
        __syncthreads();
        if (tid < m) {
            int k = 0;
            for (int v = 0; v < KNN_THREADS / 64; ++v) k += wcnt[v][tid];
            cnt[tid] = k;
        }
        __syncthreads();
        if (tid < m) {
            int off = 0;
            for (int j = 0; j < tid; ++j) off += cnt[j];
            seg[tid] = off;
            if (tid == m - 1) seg[m] = off + cnt[tid];
        }
        __syncthreads();
        if (node >= 0) {
            int pos = seg[node] + before;
            for (int v = 0; v < w; ++v) pos += wcnt[v][node];
            sorted[pos] = tid;
        }
        __syncthreads();
        // the chunk's points go through the LDS tile (free since the sweep) in groups of dims: coalesced global reads, and a
        // node's sum takes one add per point in ascending row order
        constexpr int GD = KnnTile<T>::CAP / KNN_THREADS;
        for (int d0 = 0; d0 < D; d0 += GD) {
            const int nd = D - d0 < GD ? D - d0 : GD;
            __syncthreads();
            for (int e = tid; e < KNN_THREADS * nd; e += KNN_THREADS) {
                const int r = e / nd, d = e - r * nd;
                ys[e] = base + r < n ? X[(base + r) * ld + d0 + d] : T(0);
            }
            __syncthreads();
            for (int e = tid; e < m * nd; e += KNN_THREADS) {
                const int j = e / nd, d = e - j * nd, at = j * D + d0 + d;
                double s = c == 0 ? 0.0 : ps[at];
                for (int i = seg[j]; i < seg[j + 1]; ++i) s += (double)ys[sorted[i] * nd + d];
                ps[at] = s;
            }
        }
        if (tid < m) pc[tid] = (c == 0 ? 0 : pc[tid]) + cnt[tid];
        tree_fold<KNN_THREADS>(red, Sum{});                                      // a fixed tree: the same bits every time
        if (tid == 0) mse += red[0];
        __syncthreads();
    }
    if (tid == 0) p_mse[slot] = mse;
}

// element (i, j <= i) of a packed lower triangle
__device__ __forceinline__ int pt_tri(int i, int j) { return i * (i + 1) / 2 + j; }

// Candidate blockIdx.x.  S: m x m, centre: D, partials as pt_partition_kernel wrote them over Q blocks.  A fit pass (final_pass = 0)
// replaces Y / YT by the solution, counts the iteration and sets PT_CONVERGED when max_j |Y'_j - Y_j| / |Y'_j - centre| < eps, or
// sets PT_SINGULAR at a non-positive pivot and leaves Y alone.  The final pass writes counts (m), sums (m x D) and
// energy = (sum of squared distances / n, trace(Y^T S Y)); for a singular candidate the energy is NaN.
template <typename T>
__global__ __launch_bounds__(PT_FIN_THREADS) void pt_finish_kernel(int n, int D, int m, int Q, int final_pass, double eps,
                                                               const double *__restrict__ S, const double *__restrict__ centre,
                                                               const int *__restrict__ p_counts, const double *__restrict__ p_sums,
                                                               const double *__restrict__ p_mse, double *__restrict__ Y,
                                                               T *__restrict__ YT, int *__restrict__ state, int *__restrict__ iters,
                                                               double *__restrict__ energy, int *__restrict__ counts,
                                                               double *__restrict__ sums) {
    __shared__ double L[PT_MAX_M * (PT_MAX_M + 1) / 2];
    __shared__ double R[PT_MAX_M * PT_MAX_D];
    __shared__ double ratio[PT_MAX_M];
    __shared__ int cnt[PT_MAX_M];
    const int b = blockIdx.x, tid = threadIdx.x, md = m * D;
    const int st = state[b];
    if (st & PT_SINGULAR) {
        if (final_pass && tid < 2) energy[2 * (size_t)b + tid] = NAN;
        return;
    }
    if (!final_pass && (st & PT_CONVERGED)) return;
    S += (size_t)b * m * m;
    Y += (size_t)b * md;
    YT += (size_t)b * md;
    const size_t slot0 = (size_t)b * Q;

    for (int e = tid; e < md; e += PT_FIN_THREADS) {
        const double *p = p_sums + slot0 * md + e;
        double s = 0.0;
        int q = 0;
        for (; q + 8 <= Q; q += 8) {                                             // eight loads in flight, the adds in block order
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(q + u) * md];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; q < Q; ++q) s += p[(size_t)q * md];
        R[e] = s;
    }
    if (tid < m) {
        int k = 0;
        for (int q = 0; q < Q; ++q) k += p_counts[(slot0 + q) * m + tid];
        cnt[tid] = k;
    }
    __syncthreads();

    if (final_pass) {
        for (int e = tid; e < md; e += PT_FIN_THREADS) sums[(size_t)b * md + e] = R[e];
        if (tid < m) counts[(size_t)b * m + tid] = cnt[tid];
        if (tid == 0) {
            double s = 0.0;
            for (int q = 0; q < Q; ++q) s += p_mse[slot0 + q];
            energy[2 * (size_t)b] = s / (double)n;
        }
        __syncthreads();
        for (int e = tid; e < md; e += PT_FIN_THREADS) {                         // Y_id (S Y)_id
            const int i = e / D, d = e - i * D;
            double v = 0.0;
            for (int j = 0; j < m; ++j) v += S[i * m + j] * Y[j * D + d];
            R[e] = Y[e] * v;
        }
        __syncthreads();
        tree_fold(R, md, Sum{});
        if (tid == 0) energy[2 * (size_t)b + 1] = R[0];
        return;
    }

    for (int e = tid; e < m * m; e += PT_FIN_THREADS) {
        const int i = e / m, j = e - i * m;
        if (j <= i) L[pt_tri(i, j)] = S[e] + (i == j ? (double)cnt[i] / (double)n : 0.0);
    }
    for (int e = tid; e < md; e += PT_FIN_THREADS) R[e] = R[e] / (double)n;      // the thread that wrote R[e]
    __syncthreads();

    // right-looking Cholesky, column by column; the pivot test is the same in every thread
    for (int k = 0; k < m; ++k) {
        const double pivot = L[pt_tri(k, k)];
        if (!(pivot > 0.0)) {
            if (tid == 0) state[b] = st | PT_SINGULAR;
            return;
        }
        __syncthreads();
        const double dk = sqrt(pivot);
        for (int i = k + 1 + tid; i < m; i += PT_FIN_THREADS) L[pt_tri(i, k)] /= dk;
        if (tid == 0) L[pt_tri(k, k)] = dk;
        __syncthreads();
        const int rem = m - k - 1;
        for (int e = tid; e < rem * rem; e += PT_FIN_THREADS) {
            const int i = k + 1 + e / rem, j = k + 1 + e % rem;
            if (j <= i) L[pt_tri(i, j)] -= L[pt_tri(i, k)] * L[pt_tri(j, k)];
        }
        __syncthreads();
    }
    if (tid < D) {                                                               // one right-hand side per thread
        for (int i = 0; i < m; ++i) {
            double s = R[i * D + tid];
            for (int j = 0; j < i; ++j) s -= L[pt_tri(i, j)] * R[j * D + tid];
            R[i * D + tid] = s / L[pt_tri(i, i)];
        }
        for (int i = m - 1; i >= 0; --i) {
            double s = R[i * D + tid];
            for (int j = i + 1; j < m; ++j) s -= L[pt_tri(j, i)] * R[j * D + tid];
            R[i * D + tid] = s / L[pt_tri(i, i)];
        }
    }
    __syncthreads();
    if (tid < m) {
        double num = 0.0, den = 0.0;
        for (int d = 0; d < D; ++d) {
            const double v = R[tid * D + d], a = v - Y[tid * D + d], c = v - centre[d];
            num = fma(a, a, num);
            den = fma(c, c, den);
        }
        ratio[tid] = den > 0.0 ? sqrt(num) / sqrt(den) : (num > 0.0 ? INFINITY : 0.0);
    }
    __syncthreads();
    if (tid == 0) {
        double change = 0.0;
        for (int j = 0; j < m; ++j) change = fmax(change, ratio[j]);
        iters[b] += 1;
        if (change < eps) state[b] = st | PT_CONVERGED;
    }
    for (int e = tid; e < md; e += PT_FIN_THREADS) {
        Y[e] = R[e];
        YT[e] = (T)R[e];
    }
}

// Rows blockIdx.x * rows_per_block onwards.  centre == nullptr: part[blk * D + a] = sum of x_a; otherwise
// part[blk * D * D + a * D + b] = sum of (x_a - centre_a)(x_b - centre_b).  One add per row, ascending.
template <typename T>
__global__ void pt_moments_kernel(const T *__restrict__ X, long long ld, long long n, int D, long long rows_per_block,
                                  const double *__restrict__ centre, double *__restrict__ part) {
    const int len = centre ? D * D : D;
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
    for (int e = threadIdx.x; e < len; e += blockDim.x) {
        double s = 0.0;
        if (centre) {
            const int a = e / D, c = e - a * D;
            const double ca = centre[a], cc = centre[c];
            for (long long r = r0; r < r1; ++r) s += ((double)X[r * ld + a] - ca) * ((double)X[r * ld + c] - cc);
        } else {
            for (long long r = r0; r < r1; ++r) s += (double)X[r * ld + e];
        }
        part[(size_t)blockIdx.x * len + e] = s;
    }
}

// out[e] = (part[0][e] + part[1][e] + ... + part[G - 1][e]) / divisor, e < len
__global__ void pt_reduce_kernel(const double *__restrict__ part, int G, int len, double divisor, double *__restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= len) return;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[(size_t)g * len + e];
    out[e] = s / divisor;
}

// Every point onto its nearest edge.  nodes: m x D; edges: ne pairs (a, b) with a the end nearer the source; base[j]: the tree
// distance from the source to node j.  For point i: t = the clipped parameter of its projection p = y_a + t (y_b - y_a) onto the
// edge with the smallest |x_i - p|^2 (strict <, edges ascending: a tie goes to the lowest edge), all in f64.
template <typename T>
__global__ __launch_bounds__(256) void pt_projection_kernel(const T *__restrict__ X, long long ld, long long n, int D, int m,
                                                            const double *__restrict__ nodes, int ne, const int *__restrict__ edges,
                                                            const double *__restrict__ base, double *__restrict__ pseudotime,
                                                            double *__restrict__ d2_out, int *__restrict__ edge_out,
                                                            double *__restrict__ t_out) {
    __shared__ double ny[PT_MAX_M * PT_MAX_D];
    __shared__ double len2[PT_MAX_M];
    __shared__ int ea[PT_MAX_M], eb[PT_MAX_M];
    for (int e = threadIdx.x; e < m * D; e += blockDim.x) ny[e] = nodes[e];
    __syncthreads();
    if ((int)threadIdx.x < ne) {
        const int a = edges[2 * threadIdx.x], c = edges[2 * threadIdx.x + 1];
        double s = 0.0;
        for (int d = 0; d < D; ++d) {
            const double v = ny[c * D + d] - ny[a * D + d];
            s = fma(v, v, s);
        }
        ea[threadIdx.x] = a;
        eb[threadIdx.x] = c;
        len2[threadIdx.x] = s;
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T *x = X + i * ld;
    double best = INFINITY, bt = 0.0;
    int be = 0;
    for (int e = 0; e < ne; ++e) {
        const double *ya = ny + ea[e] * D, *yb = ny + eb[e] * D;
        double dot = 0.0;
        for (int d = 0; d < D; ++d) dot = fma((double)x[d] - ya[d], yb[d] - ya[d], dot);
        double t = len2[e] > 0.0 ? dot / len2[e] : 0.0;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        double dd = 0.0;
        for (int d = 0; d < D; ++d) {
            const double r = (double)x[d] - fma(t, yb[d] - ya[d], ya[d]);
            dd = fma(r, r, dd);
        }
        if (dd < best) {
            best = dd;
            be = e;
            bt = t;
        }
    }
    pseudotime[i] = base[ea[be]] + bt * sqrt(len2[be]);
    d2_out[i] = best;
    edge_out[i] = be;
    t_out[i] = bt;
}

}  // namespace pilot
