// K13: a sparse cells x genes matrix resident in HBM as CSR (indptr int64, indices int32, data f32 / f64) and the four operations
// the gene-level consumers need of it: normalize_total + log1p in place, a column-major copy (CSC) built on the device, per-group
// column moments from that copy, and per-column non-zero counts / a dense copy of chosen columns.  Every sum is taken in f64 in a
// fixed order and nothing uses a floating-point atomic (integer atomics count), so every result has the same bits on every run.
//
// Row kernels (normalise, densify): one wave per row, CSR_ROW_WAVES rows per workgroup; the lanes stride over the row's stored
// values.  A row's total is 64 per-lane partial sums (lane l adds entries l, l + 64, ... in that order) joined by the wave
// butterfly (lanes_sum, reduce.hpp), which leaves the same bits in every lane.
//
// Column form: the rows are cut into slices of CSR_SLICE_ROWS.  (1) every slice counts its entries per column (integer atomics
// into counts[slice][column]); (2) one thread per column turns its counts into an exclusive prefix over the slices and the
// column's total, one workgroup scans the totals into colptr; (3) one wave per slice walks its rows IN ORDER, the lanes take one
// row's entries, and an entry of column c goes to colptr[c] + counts[slice][c]++.  Slices own disjoint ranges of every column
// and a slice fills its range in row order, so every column comes out in ascending row order whatever the launch timing.  The
// cursor is bumped with an integer atomic that returns the old value; the wave consumes every returned value (a ballot) before it
// issues the next row's, so two rows of a slice never race for a cursor.  Within one row the columns are distinct (upload refuses
// duplicates), so no two lanes of a step share a cursor.
//
// Column moments: one workgroup of CSR_COL_THREADS per selected column, two passes over the column's contiguous stored entries.
// Thread t takes entries t, t + 256, ... in that order; per group the 256 partials are joined by the wave butterfly and then over
// the four waves in wave order.  With n_g the group's row count (counted on the host from the codes) and s_g its stored entries
//     mean = sum_stored t(y) / n_g,        m2 = sum_stored (t(y) - mean)^2 + (n_g - s_g) mean^2,
// every term of m2 non-negative; no sum(y^2) - n mean^2 is formed.  A group's accumulators see only that group's entries, at
// positions that do not depend on the group's number, so renumbering the groups permutes the results bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "reduce.hpp"

namespace pilot {

constexpr int CSR_SLICE_ROWS = 512;     // rows per slice of the column-form build (pilot_ot_csr_slice_rows)
constexpr int CSR_ROW_WAVES = 4;        // rows (waves) per workgroup of the row kernels
constexpr int CSR_COL_THREADS = 256;    // threads per column of the moments kernel
constexpr int CSR_SCAN_THREADS = 1024;
constexpr int CSR_MAX_GROUPS = 8;

// normalize_total(target_sum) then log1p on the stored values of every row: the expressions of trajfit_normalize_kernel
template <typename T>
__global__ void __launch_bounds__(64 * CSR_ROW_WAVES) csr_normalize_kernel(const long long *__restrict__ indptr, T *__restrict__ data,
                                                                           long long n, double target_sum) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * CSR_ROW_WAVES + (threadIdx.x >> 6);
    if (r >= n) return;
    const long long p0 = indptr[r], p1 = indptr[r + 1];
    double s = 0.0;
    for (long long p = p0 + lane; p < p1; p += 64) s += (double)data[p];
    const double total = lanes_sum(s);
    const double scale = total > 0.0 ? target_sum / total : 0.0;
    for (long long p = p0 + lane; p < p1; p += 64) data[p] = (T)log1p((double)data[p] * scale);
}

// stored values != 0 per column (nnz zeroed by the host)
template <typename T>
__global__ void __launch_bounds__(256) csr_column_nnz_kernel(const int *__restrict__ indices, const T *__restrict__ data, long long nnz_total,
                                                             unsigned long long *__restrict__ nnz) {
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < nnz_total; p += step)
        if (data[p] != (T)0) atomicAdd(&nnz[indices[p]], 1ULL);
}

// out (n x n_sel, zeroed by the host): row r scatters its entries through pos[column] (-1: column not selected)
template <typename T>
__global__ void __launch_bounds__(64 * CSR_ROW_WAVES) csr_densify_kernel(const long long *__restrict__ indptr, const int *__restrict__ indices,
                                                                         const T *__restrict__ data, long long n, const int *__restrict__ pos,
                                                                         int n_sel, T *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * CSR_ROW_WAVES + (threadIdx.x >> 6);
    if (r >= n) return;
    const long long p1 = indptr[r + 1];
    T *o = out + r * n_sel;
    for (long long p = indptr[r] + lane; p < p1; p += 64) {
        const int k = pos[indices[p]];
        if (k >= 0) o[k] = data[p];
    }
}

// (1) counts[slice][column] (zeroed by the host): a slice's entries are contiguous in CSR
__global__ void __launch_bounds__(64 * CSR_ROW_WAVES) csr_slice_count_kernel(const long long *__restrict__ indptr, const int *__restrict__ indices,
                                                                             long long n, int n_cols, int n_slices, int *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const long long slice = (long long)blockIdx.x * CSR_ROW_WAVES + (threadIdx.x >> 6);
    if (slice >= n_slices) return;
    const long long r0 = slice * CSR_SLICE_ROWS, r1 = min(n, r0 + CSR_SLICE_ROWS);
    const long long p1 = indptr[r1];
    int *mine = counts + slice * n_cols;
    for (long long p = indptr[r0] + lane; p < p1; p += 64) atomicAdd(&mine[indices[p]], 1);
}

// (2a) per column: counts -> exclusive prefix over the slices, total[column]
__global__ void __launch_bounds__(256) csr_slice_scan_kernel(int *__restrict__ counts, int n_slices, int n_cols, long long *__restrict__ total) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    int run = 0;
    for (int s = 0; s < n_slices; ++s) {
        const long long o = (long long)s * n_cols + c;
        const int v = counts[o];
        counts[o] = run;
        run += v;
    }
    total[c] = run;
}

// (2b) colptr (n_cols + 1) = exclusive scan of total, one workgroup: a contiguous chunk per thread, chunk sums scanned in LDS
__global__ void __launch_bounds__(CSR_SCAN_THREADS) csr_colptr_kernel(const long long *__restrict__ total, int n_cols, long long *__restrict__ colptr) {
    __shared__ long long part[CSR_SCAN_THREADS];
    const int t = threadIdx.x, chunk = (n_cols + CSR_SCAN_THREADS - 1) / CSR_SCAN_THREADS;
    const int b = min(t * chunk, n_cols), e = min(b + chunk, n_cols);
    long long s = 0;
    for (int j = b; j < e; ++j) s += total[j];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < CSR_SCAN_THREADS; off <<= 1) {
        const long long v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = part[t] - s;
    for (int j = b; j < e; ++j) {
        colptr[j] = run;
        run += total[j];
    }
    if (t == CSR_SCAN_THREADS - 1) colptr[n_cols] = part[t];
}

// (3) cursor = the prefixes of (2a).  One wave per slice, rows in order.
template <typename T>
__global__ void __launch_bounds__(64 * CSR_ROW_WAVES) csr_fill_columns_kernel(const long long *__restrict__ indptr, const int *__restrict__ indices,
                                                                              const T *__restrict__ data, long long n, int n_cols, int n_slices,
                                                                              int *__restrict__ cursor, const long long *__restrict__ colptr,
                                                                              int *__restrict__ rowidx, T *__restrict__ cdata) {
    const int lane = threadIdx.x & 63;
    const long long slice = (long long)blockIdx.x * CSR_ROW_WAVES + (threadIdx.x >> 6);
    if (slice >= n_slices) return;
    const long long r0 = slice * CSR_SLICE_ROWS, r1 = min(n, r0 + CSR_SLICE_ROWS);
    int *mine = cursor + slice * n_cols;
    long long p0 = indptr[r0];
    for (long long r = r0; r < r1; ++r) {
        const long long p1 = indptr[r + 1];
        int seen = 0;
        for (long long p = p0 + lane; p < p1; p += 64) {
            const int c = indices[p];
            const int k = atomicAdd(&mine[c], 1);
            const long long dst = colptr[c] + k;
            rowidx[dst] = (int)r;
            cdata[dst] = data[p];
            seen |= k;
        }
        // every cursor value of this row is back before the next row's atomics are issued (a count is never negative)
        if (__ballot(seen < 0)) break;
        p0 = p1;
    }
}

struct CsrGroupCounts {
    long long n[CSR_MAX_GROUPS];
};

template <int NG> struct CsrRed {
    double d[NG][CSR_COL_THREADS / 64];
    int k[NG][CSR_COL_THREADS / 64];
};

// mean / m2: n_groups x n_sel.  codes: one per row, < 0 = skipped, else < n_groups <= NG.  rows.n[g]: rows of group g.
template <typename T, int NG, bool EXPM1>
__global__ void __launch_bounds__(CSR_COL_THREADS) csr_group_moments_kernel(const long long *__restrict__ colptr, const int *__restrict__ rowidx,
                                                                            const T *__restrict__ cdata, const int *__restrict__ codes,
                                                                            const int *__restrict__ cols, CsrGroupCounts rows, int n_groups,
                                                                            int n_sel, double *__restrict__ mean, double *__restrict__ m2) {
    __shared__ CsrRed<NG> red;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, j = blockIdx.x;
    const int c = cols ? cols[j] : j;
    const long long p0 = colptr[c], p1 = colptr[c + 1];
    auto value = [](T y) { return EXPM1 ? expm1((double)y) : (double)y; };

    double s[NG] = {};
    int k[NG] = {};
    for (long long p = p0 + t; p < p1; p += CSR_COL_THREADS) {
        const int g = codes[rowidx[p]];
        const double v = value(cdata[p]);
#pragma unroll
        for (int gg = 0; gg < NG; ++gg)
            if (g == gg) {
                s[gg] += v;
                ++k[gg];
            }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const double ws = lanes_sum(s[g]);
        const int wk = lanes_sum(k[g]);
        if (lane == 0) {
            red.d[g][wave] = ws;
            red.k[g][wave] = wk;
        }
    }
    __syncthreads();
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double mu[NG];
    int stored[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const double a = fold_in_order<CSR_COL_THREADS / 64>(red.d[g], Sum{});
        const int b = fold_in_order<CSR_COL_THREADS / 64>(red.k[g], Sum{});
        mu[g] = rows.n[g] > 0 ? a / (double)rows.n[g] : nan;
        stored[g] = b;
    }
    __syncthreads();

    double q[NG] = {};
    for (long long p = p0 + t; p < p1; p += CSR_COL_THREADS) {
        const int g = codes[rowidx[p]];
        const double v = value(cdata[p]);
#pragma unroll
        for (int gg = 0; gg < NG; ++gg)
            if (g == gg) {
                const double e = v - mu[gg];
                q[gg] = fma(e, e, q[gg]);
            }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const double wq = lanes_sum(q[g]);
        if (lane == 0) red.d[g][wave] = wq;
    }
    __syncthreads();
    if (t < NG && t < n_groups) {
        const double a = fold_in_order<CSR_COL_THREADS / 64>(red.d[t], Sum{});
        double m = nan, v = nan;
#pragma unroll
        for (int g = 0; g < NG; ++g)                       // (mu, stored, rows.n by a constant index: they stay in registers)
            if (g == t) {
                m = mu[g];
                const long long absent = rows.n[g] - stored[g];
                v = rows.n[g] > 0 ? (absent > 0 ? a + (double)absent * (m * m) : a) : nan;
            }
        mean[(long long)t * n_sel + j] = m;
        m2[(long long)t * n_sel + j] = v;
    }
}

}  // namespace pilot
