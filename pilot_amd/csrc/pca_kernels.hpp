// K15: principal components of a cells x genes matrix that is never made dense (sparse route) or standardised in place (dense
// route): the operator of a symmetric Lanczos run (lanczos_kernels.hpp), the column statistics in front of it and the scores
// behind it.
//
// Y is n x D (the selected columns).  Per column j, in f64: mu_j the mean, sigma_j = sqrt(m2_j / (n - 1)) with 0 -> 1 (both from
// the group-moments kernels, one group), and with scaling
//     z_ij = min((y_ij - mu_j) / sigma_j, max_value)                 (pca_z; the clip is on the upper side only)
// or z = y without (mu = 0, sigma = 1, max_value = +inf give exactly that).  PCA centres the columns of Z again.  With
// c_j = pca_z(0, ...) the value of an implicit zero, S has the pattern of Y and the entries s_ij = z_ij - c_j (a stored 0 gives
// exactly 0: the same expression minus itself), sbar_j = (sum_i s_ij) / n, and the centred matrix is Zc = S - 1 sbar^T.  The
// dense route is the same with c = 0 and every entry stored: S = Z.
//
// The transform is applied ONCE: the s values are written as f64 arrays beside the matrix (row order with the selected position
// of every entry's column, and column order for the sparse route), so a Lanczos step streams 12 bytes per stored entry and form
// and gathers one vector; both storage dtypes run the same f64 arithmetic from there on, and the row and the column form hold
// the same bits.  An entry of an unselected column is kept as (position 0, value 0.0): it adds +0.0.
//
// Operator on D-vectors, A v = Zc^T (Zc v):      t = S v - (sbar . v) 1,      w = S^T t - sbar (1 . t).
// Every sum is taken in f64 in a fixed order and nothing uses a floating-point atomic: the same bits from every run.
//   forward (sparse):     one wave per row; lane l adds the row's entries l, l + 64, ... in that order, then the wave butterfly
//   transposed (sparse):  one workgroup of 256 per selected column over its entries (rows ascending); thread t adds entries
//                         t, t + 256, ...; butterfly per wave, the four waves in wave order
//   1 . t:                PCA_SUM_BLOCKS workgroups each sum a contiguous chunk; every consumer adds the block sums by one tree
//   forward (dense):      one wave per row, lanes stride the columns
//   transposed (dense):   row slices of PCA_DENSE_SLICE; a workgroup owns 64 columns of a slice, wave q adds rows q, q + 4, ...
//                         and the four partials are added in wave order; the slices are joined in slice order
//   scores:               one wave per row, lane c owns component c and adds s_ij V[j][c] over the row's entries in stored order
#pragma once
#include <hip/hip_runtime.h>

#include "lanczos_kernels.hpp"
#include "reduce.hpp"

namespace pilot {

constexpr int PCA_ROW_WAVES = 4;        // rows (waves) per workgroup of the row kernels
constexpr int PCA_COL_THREADS = 256;    // threads of the per-column workgroups
constexpr int PCA_SUM_BLOCKS = 128;     // workgroups (of 256) of the 1 . t reduction
constexpr int PCA_DENSE_SLICE = 1024;   // rows per slice of the dense transposed product
constexpr int PCA_START_STREAM = -1;    // the start vector: entry j = lz_restart_entry(j, -1), then normalised

__device__ inline double pca_z(double y, double mu, double sg, double maxv) { return fmin((y - mu) / sg, maxv); }

// 1 . t from the block sums of pca_sum_kernel (blockDim.x == 256 >= PCA_SUM_BLOCKS)
__device__ inline double pca_total(const double *__restrict__ part, double *red4) {
    return block_sum<4>((int)threadIdx.x < PCA_SUM_BLOCKS ? part[threadIdx.x] : 0.0, red4);
}

// mean / m2 (one group's column moments over n rows) -> mu, sigma, c.  scale == 0: 0, 1, 0.  implicit == 0 (dense): c = 0.
static __global__ void pca_constants_kernel(const double *__restrict__ mean, const double *__restrict__ m2, long long n, int n_sel,
                                            int scale, int implicit, double maxv, double *__restrict__ mu, double *__restrict__ sg,
                                            double *__restrict__ cc) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_sel) return;
    double m = 0.0, g = 1.0;
    if (scale) {
        m = mean[j];
        g = sqrt(m2[j] / (double)(n - 1));
        if (g == 0.0) g = 1.0;
    }
    mu[j] = m;
    sg[j] = g;
    cc[j] = implicit ? pca_z(0.0, m, g, maxv) : 0.0;
}

// row form of S: per stored entry its column's selected position (pos nullable: the column itself) and s; unselected: (0, 0.0)
template <typename T>
__global__ void __launch_bounds__(256) pca_row_values_kernel(const int *__restrict__ indices, const T *__restrict__ data, long long nnz,
                                                             const int *__restrict__ pos, const double *__restrict__ mu,
                                                             const double *__restrict__ sg, const double *__restrict__ cc, double maxv,
                                                             int *__restrict__ sidx, double *__restrict__ sval) {
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += step) {
        const int c = indices[p];
        const int j = pos ? pos[c] : c;
        sidx[p] = j < 0 ? 0 : j;
        sval[p] = j < 0 ? 0.0 : pca_z((double)data[p], mu[j], sg[j], maxv) - cc[j];
    }
}

// column form of S for the selected columns (csval is indexed like cdata), sbar_j and ssq_j = sum_i (z_ij - zbar_j)^2 =
// sum_stored (s - sbar)^2 + (n - stored) sbar^2, every term non-negative.  One workgroup per selected column, two passes.
template <typename T>
__global__ void __launch_bounds__(PCA_COL_THREADS) pca_column_pass_kernel(const long long *__restrict__ colptr, const T *__restrict__ cdata,
                                                                          const int *__restrict__ cols, long long n,
                                                                          const double *__restrict__ mu, const double *__restrict__ sg,
                                                                          const double *__restrict__ cc, double maxv,
                                                                          double *__restrict__ csval, double *__restrict__ sbar,
                                                                          double *__restrict__ ssq) {
    __shared__ double red[4];
    const int j = blockIdx.x, c = cols ? cols[j] : j;
    const long long p0 = colptr[c], p1 = colptr[c + 1];
    const double m = mu[j], g = sg[j], c0 = cc[j];
    double s = 0.0;
    for (long long p = p0 + threadIdx.x; p < p1; p += PCA_COL_THREADS) {
        const double v = pca_z((double)cdata[p], m, g, maxv) - c0;
        csval[p] = v;
        s += v;
    }
    const double sb = block_sum<4>(s, red) / (double)n;
    double q = 0.0;
    for (long long p = p0 + threadIdx.x; p < p1; p += PCA_COL_THREADS) {      // (a thread reads back what it wrote itself)
        const double e = csval[p] - sb;
        q = fma(e, e, q);
    }
    q = block_sum<4>(q, red);
    if (threadIdx.x == 0) {
        const long long absent = n - (p1 - p0);
        sbar[j] = sb;
        ssq[j] = absent > 0 ? q + (double)absent * (sb * sb) : q;
    }
}

// out[0] = a . b over N entries: one workgroup of DM_FIN threads
static __global__ void __launch_bounds__(DM_FIN) pca_dot_kernel(const double *__restrict__ a, const double *__restrict__ b, int N,
                                                                double *__restrict__ out) {
    __shared__ double red[DM_FIN];
    double s = 0.0;
    for (int j = threadIdx.x; j < N; j += DM_FIN) s += a[j] * b[j];
    s = block_tree_sum<DM_FIN>(s, red);
    if (threadIdx.x == 0) out[0] = s;
}

// V[0] = r / |r|, r the documented start vector (not constant over the entries).  One workgroup of DM_FIN threads.
static __global__ void __launch_bounds__(DM_FIN) pca_start_kernel(int N, double *__restrict__ V) {
    __shared__ double red[DM_FIN];
    double s = 0.0;
    for (int j = threadIdx.x; j < N; j += DM_FIN) {
        const double r = lz_restart_entry(j, PCA_START_STREAM);
        s += r * r;
    }
    const double nrm = sqrt(block_tree_sum<DM_FIN>(s, red));
    for (int j = threadIdx.x; j < N; j += DM_FIN) V[j] = lz_restart_entry(j, PCA_START_STREAM) / nrm;
}

// t[r] = sum_p sval[p] v[sidx[p]] - dot[0] over row r's entries
static __global__ void __launch_bounds__(64 * PCA_ROW_WAVES) pca_csr_forward_kernel(const long long *__restrict__ indptr,
                                                                                    const int *__restrict__ sidx,
                                                                                    const double *__restrict__ sval, long long n,
                                                                                    const double *__restrict__ v,
                                                                                    const double *__restrict__ dot, double *__restrict__ t) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * PCA_ROW_WAVES + (threadIdx.x >> 6);
    if (r >= n) return;                                       // (whole waves leave together)
    const long long p1 = indptr[r + 1];
    double s = 0.0;
    for (long long p = indptr[r] + lane; p < p1; p += 64) s += sval[p] * v[sidx[p]];
    s = lanes_sum(s);
    if (lane == 0) t[r] = s - dot[0];
}

// part[b] = the sum of chunk b of t (n entries cut into PCA_SUM_BLOCKS contiguous chunks)
static __global__ void __launch_bounds__(256) pca_sum_kernel(const double *__restrict__ t, long long n, double *__restrict__ part) {
    __shared__ double red[4];
    const long long chunk = (n + PCA_SUM_BLOCKS - 1) / PCA_SUM_BLOCKS;
    const long long b = (long long)blockIdx.x * chunk, e = min(n, b + chunk);
    double s = 0.0;
    for (long long i = b + threadIdx.x; i < e; i += 256) s += t[i];
    s = block_sum<4>(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// w[j] = sum_p csval[p] t[rowidx[p]] - sbar[j] (1 . t) over the entries of selected column j
static __global__ void __launch_bounds__(PCA_COL_THREADS) pca_csr_transposed_kernel(const long long *__restrict__ colptr,
                                                                                    const int *__restrict__ rowidx,
                                                                                    const double *__restrict__ csval,
                                                                                    const int *__restrict__ cols, const double *__restrict__ t,
                                                                                    const double *__restrict__ part,
                                                                                    const double *__restrict__ sbar, double *__restrict__ w) {
    __shared__ double red[4];
    const int j = blockIdx.x, c = cols ? cols[j] : j;
    const long long p1 = colptr[c + 1];
    double s = 0.0;
    for (long long p = colptr[c] + threadIdx.x; p < p1; p += PCA_COL_THREADS) s += csval[p] * t[rowidx[p]];
    s = block_sum<4>(s, red);
    const double tot = pca_total(part, red);
    if (threadIdx.x == 0) w[j] = s - sbar[j] * tot;
}

// off[c] = sum_j sbar[j] Vm[j][c] (j ascending): one thread per component
static __global__ void pca_offsets_kernel(const double *__restrict__ sbar, const double *__restrict__ Vm, int D, int k,
                                          double *__restrict__ off) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= k) return;
    double s = 0.0;
    for (int j = 0; j < D; ++j) s += sbar[j] * Vm[(size_t)j * k + c];
    off[c] = s;
}

// out[r][c] = sum_p sval[p] Vm[sidx[p]][c] - off[c] over row r's entries in stored order (k <= 64: lane c owns component c; the
// lanes load 64 entries at a time and hand them round)
static __global__ void __launch_bounds__(64 * PCA_ROW_WAVES) pca_csr_scores_kernel(const long long *__restrict__ indptr,
                                                                                   const int *__restrict__ sidx,
                                                                                   const double *__restrict__ sval, long long n,
                                                                                   const double *__restrict__ Vm, int k,
                                                                                   const double *__restrict__ off, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * PCA_ROW_WAVES + (threadIdx.x >> 6);
    if (r >= n) return;
    const long long p1 = indptr[r + 1];
    const int c = lane < k ? lane : 0;
    double acc = 0.0;
    for (long long base = indptr[r]; base < p1; base += 64) {
        const bool mine = base + lane < p1;
        const double my_v = mine ? sval[base + lane] : 0.0;
        const int my_j = mine ? sidx[base + lane] : 0;
        const int cnt = (int)min((long long)64, p1 - base);
        for (int e = 0; e < cnt; ++e) {
            const double sv = __shfl(my_v, e, 64);
            const int sj = __shfl(my_j, e, 64);
            acc += sv * Vm[(size_t)sj * k + c];
        }
    }
    if (lane < k) out[r * k + lane] = acc - off[lane];
}

// Component c (one workgroup of DM_RED threads): the score of largest magnitude (lowest row on ties) becomes positive; the
// column of scores (n x k) and of pcs (D x k) flip together.
static __global__ void __launch_bounds__(DM_RED) pca_sign_kernel(double *__restrict__ scores, long long n, int k, double *__restrict__ pcs,
                                                                 int D) {
    __shared__ double bv[DM_RED];
    __shared__ long long bi[DM_RED];
    const int c = blockIdx.x;
    double best = -1.0;
    long long at = n;
    for (long long i = threadIdx.x; i < n; i += DM_RED) {
        const double a = fabs(scores[i * k + c]);
        if (a > best) { best = a; at = i; }                    // (i ascending: the first of equal magnitudes stays)
    }
    bv[threadIdx.x] = best; bi[threadIdx.x] = at;
    __syncthreads();
    tree_best<DM_RED>(bv, bi, LowestMax{});
    if (bi[0] >= n || !(scores[bi[0] * k + c] < 0.0)) return;  // (uniform over the workgroup; an all-NaN column: no index)
    __syncthreads();                                           // (every thread has read the deciding score before it may flip)
    for (long long i = threadIdx.x; i < n; i += DM_RED) scores[i * k + c] = -scores[i * k + c];
    for (int j = threadIdx.x; j < D; j += DM_RED) pcs[(size_t)j * k + c] = -pcs[(size_t)j * k + c];
}

// ---- dense twins: S = Z, n x D row-major f64 -------------------------------------------------------------------------------------
// S[i][j] = pca_z(Y[i][cols[j]])
template <typename T>
__global__ void __launch_bounds__(256) pca_dense_build_kernel(const T *__restrict__ Y, long long ld, const int *__restrict__ cols, long long n,
                                                              int D, const double *__restrict__ mu, const double *__restrict__ sg,
                                                              double maxv, double *__restrict__ S) {
    const long long total = n * D, step = (long long)gridDim.x * blockDim.x;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += step) {
        const long long i = q / D;
        const int j = (int)(q % D);
        S[q] = pca_z((double)Y[i * ld + (cols ? cols[j] : j)], mu[j], sg[j], maxv);
    }
}

// sbar_j and ssq_j = sum_i (s_ij - sbar_j)^2 of column j: one workgroup, thread t takes rows t, t + 256, ...; two passes
static __global__ void __launch_bounds__(PCA_COL_THREADS) pca_dense_column_pass_kernel(const double *__restrict__ S, long long n, int D,
                                                                                       double *__restrict__ sbar, double *__restrict__ ssq) {
    __shared__ double red[4];
    const int j = blockIdx.x;
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += PCA_COL_THREADS) s += S[i * D + j];
    const double sb = block_sum<4>(s, red) / (double)n;
    double q = 0.0;
    for (long long i = threadIdx.x; i < n; i += PCA_COL_THREADS) {
        const double e = S[i * D + j] - sb;
        q = fma(e, e, q);
    }
    q = block_sum<4>(q, red);
    if (threadIdx.x == 0) {
        sbar[j] = sb;
        ssq[j] = q;
    }
}

static __global__ void __launch_bounds__(64 * PCA_ROW_WAVES) pca_dense_forward_kernel(const double *__restrict__ S, long long n, int D,
                                                                                      const double *__restrict__ v,
                                                                                      const double *__restrict__ dot, double *__restrict__ t) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * PCA_ROW_WAVES + (threadIdx.x >> 6);
    if (r >= n) return;
    const double *row = S + r * D;
    double s = 0.0;
    for (int j = lane; j < D; j += 64) s += row[j] * v[j];
    s = lanes_sum(s);
    if (lane == 0) t[r] = s - dot[0];
}

// partw[slice][j] = sum over the slice's rows of S[i][j] t[i].  grid (ceil(D / 64), slices), block 256.
static __global__ void __launch_bounds__(256) pca_dense_transposed_kernel(const double *__restrict__ S, long long n, int D,
                                                                          const double *__restrict__ t, double *__restrict__ partw) {
    __shared__ double part[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const long long r0 = (long long)blockIdx.y * PCA_DENSE_SLICE, r1 = min(n, r0 + PCA_DENSE_SLICE);
    double s = 0.0;
    if (j < D)
        for (long long i = r0 + wv; i < r1; i += 4) s += S[i * D + j] * t[i];
    part[wv][lane] = s;
    __syncthreads();
    if (wv == 0 && j < D) partw[(size_t)blockIdx.y * D + j] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// w[j] = sum_slices partw[slice][j] (slice order) - sbar[j] (1 . t)
static __global__ void __launch_bounds__(256) pca_dense_join_kernel(const double *__restrict__ partw, int n_slices, int D,
                                                                    const double *__restrict__ part, const double *__restrict__ sbar,
                                                                    double *__restrict__ w) {
    __shared__ double red[4];
    const double tot = pca_total(part, red);
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= D) return;
    double s = 0.0;
    for (int q = 0; q < n_slices; ++q) s += partw[(size_t)q * D + j];
    w[j] = s - sbar[j] * tot;
}

// out[r][c] = sum_j S[r][j] Vm[j][c] - off[c], j ascending
static __global__ void __launch_bounds__(64 * PCA_ROW_WAVES) pca_dense_scores_kernel(const double *__restrict__ S, long long n, int D,
                                                                                     const double *__restrict__ Vm, int k,
                                                                                     const double *__restrict__ off, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * PCA_ROW_WAVES + (threadIdx.x >> 6);
    if (r >= n) return;
    const double *row = S + r * D;
    const int c = lane < k ? lane : 0;
    double acc = 0.0;
    for (int base = 0; base < D; base += 64) {
        const double my_v = base + lane < D ? row[base + lane] : 0.0;
        const int cnt = min(64, D - base);
        for (int e = 0; e < cnt; ++e) acc += __shfl(my_v, e, 64) * Vm[(size_t)(base + e) * k + c];
    }
    if (lane < k) out[r * k + lane] = acc - off[lane];
}

}  // namespace pilot
