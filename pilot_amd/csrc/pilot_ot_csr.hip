// C ABI of the device-resident sparse matrix (include/pilot_ot.h, section "sparse matrices"; kernels: csr_kernels.hpp).  The handle
// owns the CSR arrays and, once something per column was asked for, the column form; codes, cols and the results are host arrays.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "abi_common.hpp"
#include "csr_handle.hpp"
#include "csr_kernels.hpp"

namespace {

size_t elem(const pilot_ot_csr *c) { return pilot::elem_size(c->dtype); }
unsigned row_blocks(long long n) { return (unsigned)((n + pilot::CSR_ROW_WAVES - 1) / pilot::CSR_ROW_WAVES); }

int build_columns(pilot_ot_csr *c) {
    if (c->columns) return PILOT_OT_OK;
    const long long n_slices = (c->n + pilot::CSR_SLICE_ROWS - 1) / pilot::CSR_SLICE_ROWS;
    if (!c->colptr) HIP_TRY(hipMalloc(&c->colptr, sizeof(long long) * ((size_t)c->n_cols + 1)));
    if (!c->rowidx) HIP_TRY(hipMalloc(&c->rowidx, sizeof(int) * (size_t)std::max<long long>(c->nnz, 1)));
    if (!c->cdata) HIP_TRY(hipMalloc(&c->cdata, elem(c) * (size_t)std::max<long long>(c->nnz, 1)));
    int *d_counts;
    long long *d_total;
    const size_t n_counts = (size_t)std::max<long long>(n_slices, 1) * c->n_cols;
    HIP_TRY(pilot::ws(pilot::WS_CSR_COUNTS, n_counts, &d_counts));
    HIP_TRY(pilot::ws(pilot::WS_CSR_TOTAL, (size_t)c->n_cols, &d_total));
    HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(int) * n_counts, nullptr));
    const int ns = (int)n_slices;
    if (ns > 0) {
        hipLaunchKernelGGL(pilot::csr_slice_count_kernel, dim3(row_blocks(ns)), dim3(64 * pilot::CSR_ROW_WAVES), 0, nullptr, c->indptr,
                           c->indices, c->n, c->n_cols, ns, d_counts);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(pilot::csr_slice_scan_kernel, dim3((unsigned)((c->n_cols + 255) / 256)), dim3(256), 0, nullptr, d_counts, ns, c->n_cols,
                       d_total);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pilot::csr_colptr_kernel, dim3(1), dim3(pilot::CSR_SCAN_THREADS), 0, nullptr, d_total, c->n_cols, c->colptr);
    HIP_TRY(hipGetLastError());
    if (ns > 0) {
        if (c->dtype == 0)
            hipLaunchKernelGGL(pilot::csr_fill_columns_kernel<float>, dim3(row_blocks(ns)), dim3(64 * pilot::CSR_ROW_WAVES), 0, nullptr, c->indptr,
                               c->indices, static_cast<const float *>(c->data), c->n, c->n_cols, ns, d_counts, c->colptr, c->rowidx,
                               static_cast<float *>(c->cdata));
        else
            hipLaunchKernelGGL(pilot::csr_fill_columns_kernel<double>, dim3(row_blocks(ns)), dim3(64 * pilot::CSR_ROW_WAVES), 0, nullptr, c->indptr,
                               c->indices, static_cast<const double *>(c->data), c->n, c->n_cols, ns, d_counts, c->colptr, c->rowidx,
                               static_cast<double *>(c->cdata));
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    c->columns = true;
    return PILOT_OT_OK;
}

struct MomentsArgs {
    const pilot_ot_csr *c;
    const int *codes, *cols;
    pilot::CsrGroupCounts rows;
    int n_groups, n_sel;
    double *mean, *m2;
};

template <typename T, int NG> void launch_ng(const MomentsArgs &a, int transform) {
    const pilot_ot_csr *c = a.c;
    if (transform)
        hipLaunchKernelGGL((pilot::csr_group_moments_kernel<T, NG, true>), dim3((unsigned)a.n_sel), dim3(pilot::CSR_COL_THREADS), 0, nullptr,
                           c->colptr, c->rowidx, static_cast<const T *>(c->cdata), a.codes, a.cols, a.rows, a.n_groups, a.n_sel, a.mean, a.m2);
    else
        hipLaunchKernelGGL((pilot::csr_group_moments_kernel<T, NG, false>), dim3((unsigned)a.n_sel), dim3(pilot::CSR_COL_THREADS), 0, nullptr,
                           c->colptr, c->rowidx, static_cast<const T *>(c->cdata), a.codes, a.cols, a.rows, a.n_groups, a.n_sel, a.mean, a.m2);
}

template <typename T> void launch(const MomentsArgs &a, int transform) {
    if (a.n_groups <= 1) launch_ng<T, 1>(a, transform);
    else if (a.n_groups <= 2) launch_ng<T, 2>(a, transform);
    else if (a.n_groups <= 4) launch_ng<T, 4>(a, transform);
    else launch_ng<T, 8>(a, transform);
}

}  // namespace

PILOT_API int pilot_ot_csr_slice_rows(void) { return pilot::CSR_SLICE_ROWS; }

PILOT_API int pilot_ot_csr_upload(const long long *indptr, const int *indices, const void *data, int dtype, long long n_rows, int n_cols,
                                  pilot_ot_csr **csr) {
    if (!indptr || !csr) return fail(PILOT_OT_EINVAL, "NULL pointer (indptr or csr)");
    if (int rc = pilot::check_dtype(dtype)) return rc;
    if (n_rows < 0 || n_rows > INT_MAX || n_cols < 1) return fail(PILOT_OT_EINVAL, "n_rows=%lld (at most %d), n_cols=%d", n_rows, INT_MAX, n_cols);
    if (indptr[0] != 0) return fail(PILOT_OT_EINVAL, "indptr[0]=%lld must be 0", indptr[0]);
    for (long long i = 0; i < n_rows; ++i)
        if (indptr[i + 1] < indptr[i])
            return fail(PILOT_OT_EINVAL, "indptr is not non-decreasing: indptr[%lld]=%lld after %lld", i + 1, indptr[i + 1], indptr[i]);
    const long long nnz = indptr[n_rows];
    if (nnz > 0 && (!indices || !data)) return fail(PILOT_OT_EINVAL, "NULL pointer (indices or data)");
    {
        std::vector<int> last((size_t)n_cols, -1);                 // the last row that stored each column
        for (long long i = 0; i < n_rows; ++i)
            for (long long p = indptr[i]; p < indptr[i + 1]; ++p) {
                const int j = indices[p];
                if (j < 0 || j >= n_cols) return fail(PILOT_OT_EINVAL, "indices[%lld]=%d outside [0, %d)", p, j, n_cols);
                if (last[j] == (int)i) return fail(PILOT_OT_EINVAL, "duplicate entry: row %lld stores column %d twice (indices[%lld])", i, j, p);
                last[j] = (int)i;
            }
    }
    pilot_ot_csr *c = new (std::nothrow) pilot_ot_csr();
    if (!c) return fail(PILOT_OT_EINVAL, "out of host memory");
    c->n = n_rows; c->nnz = nnz; c->n_cols = n_cols; c->dtype = dtype;
    const size_t es = elem(c), m = (size_t)std::max<long long>(nnz, 1);
    hipError_t e = hipGetDevice(&c->device);
    if (e == hipSuccess) e = hipMalloc(&c->indptr, sizeof(long long) * ((size_t)n_rows + 1));
    if (e == hipSuccess) e = hipMalloc(&c->indices, sizeof(int) * m);
    if (e == hipSuccess) e = hipMalloc(&c->data, es * m);
    if (e == hipSuccess) e = hipMemcpy(c->indptr, indptr, sizeof(long long) * ((size_t)n_rows + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz > 0) e = hipMemcpy(c->indices, indices, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz > 0) e = hipMemcpy(c->data, data, es * (size_t)nnz, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        pilot_ot_csr_destroy(c);
        return fail(PILOT_OT_EHIP, "sparse upload failed: %s", hipGetErrorString(e));
    }
    *csr = c;
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_csr_destroy(pilot_ot_csr *c) {
    if (!c) return PILOT_OT_OK;
    for (void *p : {(void *)c->indptr, (void *)c->indices, c->data, (void *)c->colptr, (void *)c->rowidx, c->cdata})
        if (p) (void)hipFree(p);
    delete c;
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_csr_normalize_log1p(pilot_ot_csr *c, double target_sum) {
    if (!(target_sum > 0.0) || !std::isfinite(target_sum)) return fail(PILOT_OT_EINVAL, "target_sum=%g must be positive", target_sum);
    if (!c) return fail(PILOT_OT_EINVAL, "NULL pointer (csr)");
    c->columns = false;
    if (c->n == 0 || c->nnz == 0) return PILOT_OT_OK;
    if (c->dtype == 0)
        hipLaunchKernelGGL(pilot::csr_normalize_kernel<float>, dim3(row_blocks(c->n)), dim3(64 * pilot::CSR_ROW_WAVES), 0, nullptr, c->indptr,
                           static_cast<float *>(c->data), c->n, target_sum);
    else
        hipLaunchKernelGGL(pilot::csr_normalize_kernel<double>, dim3(row_blocks(c->n)), dim3(64 * pilot::CSR_ROW_WAVES), 0, nullptr, c->indptr,
                           static_cast<double *>(c->data), c->n, target_sum);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_csr_build_columns(pilot_ot_csr *c) {
    if (!c) return fail(PILOT_OT_EINVAL, "NULL pointer (csr)");
    return build_columns(c);
}

PILOT_API int pilot_ot_csr_column_nnz(pilot_ot_csr *c, long long *nnz) {
    if (!c || !nnz) return fail(PILOT_OT_EINVAL, "NULL pointer (csr or nnz)");
    unsigned long long *d_nnz;
    HIP_TRY(pilot::ws(pilot::WS_CSR_OUT, (size_t)c->n_cols, &d_nnz));
    HIP_TRY(hipMemsetAsync(d_nnz, 0, sizeof(unsigned long long) * (size_t)c->n_cols, nullptr));
    if (c->nnz > 0) {
        const int grid = pilot::grid_for((long)c->nnz, 256, pilot::cu_count());
        if (c->dtype == 0)
            hipLaunchKernelGGL(pilot::csr_column_nnz_kernel<float>, dim3(grid), dim3(256), 0, nullptr, c->indices, static_cast<const float *>(c->data),
                               c->nnz, d_nnz);
        else
            hipLaunchKernelGGL(pilot::csr_column_nnz_kernel<double>, dim3(grid), dim3(256), 0, nullptr, c->indices,
                               static_cast<const double *>(c->data), c->nnz, d_nnz);
        HIP_TRY(hipGetLastError());
    }
    static_assert(sizeof(long long) == sizeof(unsigned long long), "the counts are copied as they are");
    HIP_TRY(hipMemcpy(nnz, d_nnz, sizeof(long long) * (size_t)c->n_cols, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_csr_group_moments(pilot_ot_csr *c, const int *codes, int n_groups, const int *cols, int n_cols, int transform,
                                         long long *count, double *mean, double *m2) {
    if (n_groups < 1 || n_groups > pilot::CSR_MAX_GROUPS) return fail(PILOT_OT_EINVAL, "n_groups=%d must be in [1, %d]", n_groups, pilot::CSR_MAX_GROUPS);
    if (transform != 0 && transform != 1) return fail(PILOT_OT_EINVAL, "transform=%d must be 0 (none) or 1 (expm1)", transform);
    if (!c || !count || !mean || !m2 || (!codes && c->n > 0)) return fail(PILOT_OT_EINVAL, "NULL pointer (csr, codes, count, mean or m2)");
    if (int rc = pilot::check_cols(cols, n_cols, c->n_cols)) return rc;
    MomentsArgs a;
    a.c = c;
    for (long long &v : a.rows.n) v = 0;
    for (long long i = 0; i < c->n; ++i) {
        if (codes[i] >= n_groups)
            return fail(PILOT_OT_EINVAL, "codes[%lld]=%d: a code is negative (row skipped) or below n_groups=%d", i, codes[i], n_groups);
        if (codes[i] >= 0) ++a.rows.n[codes[i]];
    }
    for (int g = 0; g < n_groups; ++g) count[g] = a.rows.n[g];
    if (n_cols == 0) return PILOT_OT_OK;
    const int rc = build_columns(c);
    if (rc != PILOT_OT_OK) return rc;
    int *d_codes, *d_cols = nullptr;
    double *d_out;
    HIP_TRY(pilot::ws(pilot::WS_CSR_CODES, (size_t)c->n, &d_codes));
    if (c->n > 0) HIP_TRY(hipMemcpy(d_codes, codes, sizeof(int) * (size_t)c->n, hipMemcpyHostToDevice));
    if (cols) {
        HIP_TRY(pilot::ws(pilot::WS_CSR_COLS, (size_t)n_cols, &d_cols));
        HIP_TRY(hipMemcpy(d_cols, cols, sizeof(int) * (size_t)n_cols, hipMemcpyHostToDevice));
    }
    const size_t n_out = (size_t)n_groups * n_cols;
    HIP_TRY(pilot::ws(pilot::WS_CSR_OUT, 2 * n_out, &d_out));
    a.codes = d_codes;
    a.cols = d_cols;
    a.n_groups = n_groups;
    a.n_sel = n_cols;
    a.mean = d_out;
    a.m2 = d_out + n_out;
    if (c->dtype == 0) launch<float>(a, transform);
    else launch<double>(a, transform);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(mean, a.mean, sizeof(double) * n_out, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(m2, a.m2, sizeof(double) * n_out, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_csr_densify(pilot_ot_csr *c, const int *cols, int n_cols, void *out) {
    if (!c || (!out && n_cols > 0)) return fail(PILOT_OT_EINVAL, "NULL pointer (csr or out)");
    if (int rc = pilot::check_cols(cols, n_cols, c->n_cols)) return rc;
    std::vector<int> pos((size_t)c->n_cols, -1);
    for (int j = 0; j < n_cols; ++j) {
        const int col = cols ? cols[j] : j;
        if (pos[col] >= 0) return fail(PILOT_OT_EINVAL, "cols[%d]=%d repeats cols[%d]: a column is written once", j, col, pos[col]);
        pos[col] = j;
    }
    if (c->n == 0 || n_cols == 0) return PILOT_OT_OK;
    int *d_pos;
    HIP_TRY(pilot::ws(pilot::WS_CSR_COLS, (size_t)c->n_cols, &d_pos));
    HIP_TRY(hipMemcpy(d_pos, pos.data(), sizeof(int) * (size_t)c->n_cols, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(out, 0, elem(c) * (size_t)c->n * n_cols, nullptr));
    if (c->nnz > 0) {
        if (c->dtype == 0)
            hipLaunchKernelGGL(pilot::csr_densify_kernel<float>, dim3(row_blocks(c->n)), dim3(64 * pilot::CSR_ROW_WAVES), 0, nullptr, c->indptr,
                               c->indices, static_cast<const float *>(c->data), c->n, d_pos, n_cols, static_cast<float *>(out));
        else
            hipLaunchKernelGGL(pilot::csr_densify_kernel<double>, dim3(row_blocks(c->n)), dim3(64 * pilot::CSR_ROW_WAVES), 0, nullptr, c->indptr,
                               c->indices, static_cast<const double *>(c->data), c->n, d_pos, n_cols, static_cast<double *>(out));
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    return PILOT_OT_OK;
}
