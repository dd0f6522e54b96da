// K11: gene curve clustering (pilotpy's genes_selection_analysis, plot/gene_selection_analysis.py:86-203, 360-415 and
// plot/curve_activity.py): the per-time-point spread of the cells (K11a), the fitted and standardised curves, the Euclidean
// distance matrix of the curves with agglomerative linkage over it (K11b) and the curve activities.  f64 throughout.  Every sum
// is taken in a fixed order -- strided partials per lane or wave slice, then a fixed shuffle or LDS tree -- and nothing uses a
// floating-point atomic, so a repeated call returns the same bits whatever the route.
#pragma once
#include <hip/hip_runtime.h>

#include "reduce.hpp"

namespace pilot {

// ---- K11a: sample standard deviation (ddof 1) of every selected column over each contiguous row segment --------------------------
// Grid (column tiles of 64, segments); one lane per column (64 consecutive elements of a row per wave: coalesced along the genes),
// CV_STD_SLICES waves splitting the segment's rows into fixed slices.  Two passes over the block's slab, mean then squared
// deviations (the second re-reads what the first just brought into L2: one pass over Y from HBM); slice partials meet in LDS in
// slice order.  A segment of one row gives 0 / 0 = NaN, as pandas' std does.
constexpr int CV_STD_SLICES = 8;
constexpr int CV_STD_BLOCK = 64 * CV_STD_SLICES;

template <typename T>
__global__ void __launch_bounds__(CV_STD_BLOCK) segment_std_kernel(const T *__restrict__ Y, long long ld,
                                                                   const long long *__restrict__ offsets,
                                                                   const int *__restrict__ cols, int n_sel,
                                                                   double *__restrict__ out) {
    __shared__ double part[CV_STD_SLICES][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane, seg = blockIdx.y;
    const bool valid = j < n_sel;
    const long long r0 = offsets[seg], m = offsets[seg + 1] - r0;
    const long long i0 = r0 + m * slice / CV_STD_SLICES, i1 = r0 + m * (slice + 1) / CV_STD_SLICES;
    const T *col = Y + (valid ? (cols ? cols[j] : j) : 0);
    double s = 0.0;
    if (valid)
        for (long long i = i0; i < i1; ++i) s += (double)col[i * ld];
    part[slice][lane] = s;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int q = 0; q < CV_STD_SLICES; ++q) tot += part[q][lane];
    const double mean = tot / (double)m;
    __syncthreads();
    double ss = 0.0;
    if (valid)
        for (long long i = i0; i < i1; ++i) {
            const double d = (double)col[i * ld] - mean;
            ss += d * d;
        }
    part[slice][lane] = ss;
    __syncthreads();
    if (slice != 0 || !valid) return;
    double q2 = 0.0;
#pragma unroll
    for (int q = 0; q < CV_STD_SLICES; ++q) q2 += part[q][lane];
    out[(long long)seg * n_sel + j] = sqrt(q2 / (double)(m - 1));
}

// ---- fitted curves: curve = design(model, t) @ coefs (+ noise), standardised per gene ---------------------------------------------
// One wave per gene.  params: G x 3 (Intercept, Treat, Treat2); model 0 linear [1, t], 1 linear_quadratic [1, t, t^2],
// 2 quadratic [1, t^2]; sd (nullable): T x G per-time-point spreads, noise[g, t] = sd[t, g] / 10 * (Treat + Treat2 - Intercept),
// a NaN sum becomes 0 (the reference's fillna(0)).  Then StandardScaler over the time points: population variance, a scale
// below 10 eps becomes 1.  out: G x T.
__global__ void __launch_bounds__(64) fitted_curves_kernel(const double *__restrict__ params, const int *__restrict__ models,
                                                           const double *__restrict__ times, int G, int T,
                                                           const double *__restrict__ sd, double *__restrict__ out) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const double c0 = params[g * 3], c1 = params[g * 3 + 1], c2 = params[g * 3 + 2];
    const int md = models[g];
    const double cov = (c1 + c2) - c0;
    double *o = out + (long long)g * T;
    double s = 0.0;
    for (int t = lane; t < T; t += 64) {
        const double x = times[t];
        double v = md == 0 ? c0 + x * c1 : md == 1 ? c0 + x * c1 + x * x * c2 : c0 + x * x * c1;
        if (sd) {
            v += sd[(long long)t * G + g] / 10.0 * cov;
            if (v != v) v = 0.0;
        }
        o[t] = v;
        s += v;
    }
    const double mean = lanes_sum(s) / T;
    double q = 0.0;
    for (int t = lane; t < T; t += 64) {             // (a lane re-reads only what it wrote)
        const double d = o[t] - mean;
        q += d * d;
    }
    double scale = sqrt(lanes_sum(q) / T);
    if (scale < 10.0 * 2.220446049250313e-16) scale = 1.0;
    for (int t = lane; t < T; t += 64) o[t] = (o[t] - mean) / scale;
}

// ---- K11b, distances: D[i][j] = sqrt(sum_t (Y[i][t] - Y[j][t])^2), the direct form, tiled through LDS -------------------------------
// 64 x 64 outputs per block of 256 threads (4 x 4 per thread), T in chunks of CV_D_KC; only tiles on or above the diagonal are
// computed and each is written to both halves, so D is symmetric to the bit (the sum runs over t ascending either way).  bmax: the
// largest distance of every block (0 for the skipped ones), reduced by the host to d.max().
constexpr int CV_D_TILE = 64, CV_D_KC = 16;

__global__ void __launch_bounds__(256) curve_distance_kernel(const double *__restrict__ Y, int G, int T, double *__restrict__ D,
                                                             double *__restrict__ bmax) {
    __shared__ double sA[CV_D_KC][CV_D_TILE + 1], sB[CV_D_KC][CV_D_TILE + 1];
    __shared__ double wmax[4];
    const int bi = blockIdx.y, bj = blockIdx.x, tid = threadIdx.x;
    if (bj < bi) {
        if (tid == 0) bmax[bi * gridDim.x + bj] = 0.0;
        return;
    }
    const int tx = tid & 15, ty = tid >> 4;
    double acc[4][4] = {};
    for (int k0 = 0; k0 < T; k0 += CV_D_KC) {
        for (int e = tid; e < CV_D_TILE * CV_D_KC; e += 256) {
            const int r = e / CV_D_KC, k = e % CV_D_KC;
            const int ia = bi * CV_D_TILE + r, ib = bj * CV_D_TILE + r;
            const bool in = k0 + k < T;
            sA[k][r] = in && ia < G ? Y[(long long)ia * T + k0 + k] : 0.0;
            sB[k][r] = in && ib < G ? Y[(long long)ib * T + k0 + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CV_D_KC; ++k) {
            double a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { a[r] = sA[k][ty * 4 + r]; b[r] = sB[k][tx * 4 + r]; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double d = a[r] - b[c];
                    acc[r][c] += d * d;
                }
        }
        __syncthreads();
    }
    double mx = 0.0;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            const int i = bi * CV_D_TILE + ty * 4 + r, j = bj * CV_D_TILE + tx * 4 + c;
            if (i >= G || j >= G) continue;
            const double d = sqrt(acc[r][c]);
            D[(long long)i * G + j] = d;
            D[(long long)j * G + i] = d;
            mx = fmax(mx, d);
        }
    const auto larger = [](double a, double b) { return fmax(a, b); };      // (fmax: a NaN distance is passed over)
    mx = waves_in_order<4>(lanes_reduce(mx, larger), wmax, larger);
    if (tid == 0) bmax[bi * gridDim.x + bj] = mx;
}

// ---- K11b, merging: the nearest-neighbour chain over the full G x G matrix in HBM, one persistent workgroup --------------------------
// scipy's nn_chain (cluster/_hierarchy.pyx) step by step: the chain grows by the nearest active cluster of its tip (ties: the
// previous chain element first, then the lowest index) until two clusters are each other's nearest; they merge into the slot of
// the larger index, whose row AND column take the Lance-Williams distances; the row and column of the slot that died are set to
// +inf, so the search reads one contiguous row and needs no list of the living.  Loops: exactly G - 1 merges, and a cap of 4 G
// chain steps in all (the chain makes fewer than 3 G); reaching the cap sets info[0] = 1 and stops.  Z (unsorted, unlabelled):
// per merge x < y, the height, the new size.  info: [0] status, [1] chain steps taken.
constexpr int CV_NN_BLOCK = 1024;
constexpr int CV_LINK_SINGLE = 0, CV_LINK_COMPLETE = 1, CV_LINK_AVERAGE = 2, CV_LINK_WEIGHTED = 3;

__global__ void __launch_bounds__(CV_NN_BLOCK) nn_chain_kernel(double *__restrict__ D, int G, int method, int *__restrict__ chain,
                                                               int *__restrict__ size, double *__restrict__ Z,
                                                               int *__restrict__ info) {
    __shared__ double wv[CV_NN_BLOCK / 64];
    __shared__ int wi[CV_NN_BLOCK / 64];
    __shared__ int s_x, s_y, s_len, s_merge, s_first;
    __shared__ double s_min;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double inf = INFINITY;
    for (int i = tid; i < G; i += CV_NN_BLOCK) size[i] = 1;
    if (tid == 0) { s_len = 0; s_first = 0; }
    __syncthreads();
    const long long cap = 4LL * G;
    long long steps = 0;
    int status = 0;
    for (int k = 0; k < G - 1; ++k) {
        if (tid == 0 && s_len == 0) {                       // restart from the first living cluster (bounded: s_first only grows)
            int f = s_first;
            while (f < G && size[f] == 0) ++f;
            s_first = f;
            chain[0] = f;
            s_len = 1;
        }
        __syncthreads();
        bool merged = false;
        while (!merged) {
            if (steps >= cap) { status = 1; break; }
            ++steps;
            const int len = s_len, x = chain[len - 1], prev = len > 1 ? chain[len - 2] : -1;
            const double *row = D + (long long)x * G;
            double bv = inf;
            int bi = G;
            for (int i = tid; i < G; i += CV_NN_BLOCK) {        // ascending i per thread: a strict < keeps the lowest index
                const double d = row[i];
                if (i != x && d < bv) { bv = d; bi = i; }
            }
            lanes_best(bv, bi, LowestMin{});
            if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < CV_NN_BLOCK / 64; ++w)
                    if (wv[w] < bv || (wv[w] == bv && wi[w] < bi)) { bv = wv[w]; bi = wi[w]; }
                if (prev >= 0 && !(bv < row[prev])) { bv = row[prev]; bi = prev; }      // the previous element wins a tie
                s_merge = bi >= G ? 2 : (prev >= 0 && bi == prev);      // 2: no finite distance in the row (NaN input)
                s_x = x; s_y = bi; s_min = bv;
                if (!s_merge) { chain[len] = bi; s_len = len + 1; }
            }
            __syncthreads();
            if (s_merge == 2) { status = 2; break; }
            merged = s_merge != 0;
        }
        if (status) break;
        int x = s_x, y = s_y;
        const double h = s_min;
        if (x > y) { const int t = x; x = y; y = t; }
        const int nx = size[x], ny = size[y];
        __syncthreads();                                        // every thread has read s_*, size[] before thread 0 changes them
        if (tid == 0) {
            s_len -= 2;
            double *z = Z + (long long)k * 4;
            z[0] = x; z[1] = y; z[2] = h; z[3] = nx + ny;
            size[x] = 0; size[y] = nx + ny;
        }
        const double *rx = D + (long long)x * G;
        double *ry = D + (long long)y * G;
        for (int i = tid; i < G; i += CV_NN_BLOCK) {
            const double dx = rx[i], dy = ry[i];
            double nd;
            if (i == x || i == y || dy == inf) nd = inf;        // dead slots (and the diagonal, never read) stay out of every search
            else if (method == CV_LINK_SINGLE) nd = fmin(dx, dy);
            else if (method == CV_LINK_COMPLETE) nd = fmax(dx, dy);
            else if (method == CV_LINK_AVERAGE) nd = ((double)nx * dx + (double)ny * dy) / (double)(nx + ny);
            else nd = 0.5 * (dx + dy);
            ry[i] = nd;
            D[(long long)i * G + y] = nd;
            D[(long long)i * G + x] = inf;
        }
        __syncthreads();
    }
    if (tid == 0) { info[0] = status; info[1] = (int)(steps > 0x7fffffffLL ? 0x7fffffffLL : steps); }
}

// ---- curve activities (plot/curve_activity.py): terminal logFC, transient logFC, switching time, area ---------------------------------
// One wave per curve; the trapezoid sums as strided lane partials over the intervals, then the fixed tree.  out: G x 4.
__device__ inline double cv_median3(double a, double b, double c) { return fmax(fmin(a, b), fmin(fmax(a, b), c)); }

__global__ void __launch_bounds__(64) curve_activities_kernel(const double *__restrict__ curves, const double *__restrict__ times,
                                                              int G, int T, double *__restrict__ out) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const double *c = curves + (long long)g * T;
    const double c0 = c[0], cT = c[T - 1], t0 = times[0], span = times[T - 1] - times[0];
    double tr = 0.0, sw = 0.0;
    for (int j = lane; j + 1 < T; j += 64) {
        const double dt = (times[j + 1] - t0) / span - (times[j] - t0) / span;
        const double m0 = cv_median3(c[j], c0, cT), m1 = cv_median3(c[j + 1], c0, cT);
        tr += ((c[j + 1] - m1) + (c[j] - m0)) / 2.0 * dt;
        sw += ((m1 - cT) + (m0 - cT)) / 2.0 * dt;
    }
    tr = lanes_sum(tr);
    sw = lanes_sum(sw);
    if (lane != 0) return;
    double *o = out + (long long)g * 4;
    o[0] = (cT - c0) / span;
    o[1] = tr;
    o[2] = sw / (c0 - cT + 1e-300);
    o[3] = fabs(c0 + cT) * fabs(span);
}

}  // namespace pilot
