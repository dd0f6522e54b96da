// C ABI of the per-group rank sums (include/pilot_ot.h, section "rank sums"; kernels: rank_sums_kernels.hpp).  Y is a host array
// (copied whole, packed), a row-major buffer in HBM with its own leading dimension, or a sparse handle's column form; codes, cols
// and the results are host arrays.  The host bins the columns by their number of non-zero used entries between the two scans.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <vector>

#include "abi_common.hpp"
#include "csr_handle.hpp"
#include "rank_sums_kernels.hpp"

namespace {

using pilot::rs_u64;

// count[g]; PILOT_OT_EINVAL for a code >= n_groups, PILOT_OT_ENOTSUP for more used rows than the tie term allows.  No HIP call.
int count_rows(const int *codes, long long n, int n_groups, long long *count, long long *n_used) {
    if (n > INT_MAX) return fail(PILOT_OT_ENOTSUP, "n=%lld rows need more than 32-bit row indices", n);
    for (int g = 0; g < n_groups; ++g) count[g] = 0;
    long long used = 0;
    for (long long i = 0; i < n; ++i) {
        if (codes[i] >= n_groups)
            return fail(PILOT_OT_EINVAL, "codes[%lld]=%d: a code is negative (row skipped) or below n_groups=%d", i, codes[i], n_groups);
        if (codes[i] >= 0) { ++count[codes[i]]; ++used; }
    }
    if (used > pilot::RS_MAX_ROWS)
        return fail(PILOT_OT_ENOTSUP, "%lld used rows: the tie term t^3 - t is exact up to %lld", used, pilot::RS_MAX_ROWS);
    *n_used = used;
    return PILOT_OT_OK;
}

int check_groups(int n_groups) {
    if (n_groups < 1 || n_groups > pilot::RS_MAX_GROUPS)
        return fail(PILOT_OT_EINVAL, "n_groups=%d must be in [1, %d]", n_groups, pilot::RS_MAX_GROUPS);
    return PILOT_OT_OK;
}

// what the scans read and write besides the matrix
struct DevScan {
    const int *codes, *cols;
    int *len;
    const long long *off;
    void *rec;
    rs_u64 *bad;
};

template <typename T> int launch_rank(const int *list, int n_list, int threads, int cap, const DevScan &d, const long long *d_count,
                                      int n_groups, long long n_used, int n_sel, long long *rank2, long long *ties) {
    if (n_list == 0) return PILOT_OT_OK;
    typedef typename pilot::RsKey<T>::Rec Rec;
    const size_t lds = sizeof(Rec) * (size_t)cap + 8 * ((size_t)n_groups + 1) + 4 * (size_t)n_groups;
    auto kern = threads == 64 ? pilot::rs_rank_kernel<T, 64> : pilot::rs_rank_kernel<T, pilot::RS_THREADS>;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)n_list), dim3((unsigned)threads), lds, nullptr, list, d.len, d.off, static_cast<Rec *>(d.rec), cap,
                       d_count, n_groups, n_used, n_sel, rank2, ties);
    HIP_TRY(hipGetLastError());
    return PILOT_OT_OK;
}

// `scan(fill, d)` enqueues the counting or the filling scan of the caller's matrix.  cols (nullable, host): what a bad position
// is translated through.
template <typename T, typename Scan>
int run(const int *codes, long long n, const long long *count, long long n_used, int n_groups, const int *cols, int n_sel, long long *rank2,
        long long *ties, long long *bad_row, int *bad_col, Scan scan) {
    typedef typename pilot::RsKey<T>::Rec Rec;
    // ints: codes[n] | cols[n_sel] | len[n_sel] | cursor[n_sel] | list[n_sel];  int64: off[n_sel] | count[n_groups] | bad
    int *d_int;
    long long *d_ll;
    const size_t ns = (size_t)n_sel;
    HIP_TRY(pilot::ws(pilot::WS_RS_INT, (size_t)n + 4 * ns, &d_int));
    HIP_TRY(pilot::ws(pilot::WS_RS_LL, ns + (size_t)n_groups + 1, &d_ll));
    int *d_codes = d_int, *d_cols = d_codes + n, *d_len = d_cols + ns, *d_cursor = d_len + ns, *d_list = d_cursor + ns;
    long long *d_off = d_ll, *d_count = d_off + ns;
    rs_u64 *d_bad = reinterpret_cast<rs_u64 *>(d_count + n_groups);
    HIP_TRY(hipMemcpy(d_codes, codes, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    if (cols) HIP_TRY(hipMemcpy(d_cols, cols, sizeof(int) * ns, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_count, count, sizeof(long long) * (size_t)n_groups, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(d_len, 0, sizeof(int) * 2 * ns, nullptr));                 // len and cursor
    HIP_TRY(hipMemsetAsync(d_bad, 0xFF, sizeof(rs_u64), nullptr));
    DevScan d{d_codes, cols ? d_cols : nullptr, d_len, d_off, nullptr, d_bad};
    scan(false, d);
    HIP_TRY(hipGetLastError());
    std::vector<int> len(ns);
    rs_u64 bad = 0;
    HIP_TRY(hipMemcpy(len.data(), d_len, sizeof(int) * ns, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost));
    if (bad != pilot::RS_NO_BAD) {
        const int pos = (int)(bad >> 32), col = cols ? cols[pos] : pos;
        const long long row = (long long)(bad & 0xFFFFFFFFull);
        if (bad_row) *bad_row = row;
        if (bad_col) *bad_col = col;
        return fail(PILOT_OT_EINVAL, "Y[%lld, %d] is NaN or infinite (row %lld is used, the column is cols[%d])", row, col, row, pos);
    }
    // the bins and every position's slice of the records
    std::vector<long long> off(ns);
    std::vector<int> list(ns);
    int n_wave = 0, n_wg = 0, n_long = 0;
    for (int j = 0; j < n_sel; ++j) n_wave += len[j] <= pilot::RS_WAVE_MAX, n_wg += len[j] > pilot::RS_WAVE_MAX && len[j] <= pilot::RS_WG_MAX;
    n_long = n_sel - n_wave - n_wg;
    long long total = 0;
    int at[3] = {0, n_wave, n_wave + n_wg};
    for (int j = 0; j < n_sel; ++j) {
        const int L = len[j], bin = L <= pilot::RS_WAVE_MAX ? 0 : L <= pilot::RS_WG_MAX ? 1 : 2;
        list[at[bin]++] = j;
        off[j] = total;
        long long P = L;
        if (bin == 2)
            for (P = 1; P < L; P <<= 1) {}
        total += P;
    }
    Rec *d_rec;
    HIP_TRY(pilot::ws(pilot::WS_RS_REC, (size_t)total, &d_rec));
    HIP_TRY(hipMemcpy(d_off, off.data(), sizeof(long long) * ns, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_list, list.data(), sizeof(int) * ns, hipMemcpyHostToDevice));
    d.len = d_cursor;
    d.rec = d_rec;
    if (total > 0) {
        scan(true, d);
        HIP_TRY(hipGetLastError());
    }
    d.len = d_len;
    long long *d_out;
    const size_t n_out = (size_t)n_groups * ns;
    HIP_TRY(pilot::ws(pilot::WS_RS_OUT, n_out + ns, &d_out));
    if (int rc = launch_rank<T>(d_list, n_wave, 64, pilot::RS_WAVE_MAX, d, d_count, n_groups, n_used, n_sel, d_out, d_out + n_out)) return rc;
    if (int rc = launch_rank<T>(d_list + n_wave, n_wg, pilot::RS_THREADS, pilot::RS_WG_MAX, d, d_count, n_groups, n_used, n_sel, d_out,
                                d_out + n_out))
        return rc;
    if (int rc = launch_rank<T>(d_list + n_wave + n_wg, n_long, pilot::RS_THREADS, pilot::RS_SORT_TILE, d, d_count, n_groups, n_used, n_sel,
                                d_out, d_out + n_out))
        return rc;
    HIP_TRY(hipMemcpy(rank2, d_out, sizeof(long long) * n_out, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ties, d_out + n_out, sizeof(long long) * ns, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}

// the results when there is nothing to rank
void nothing_used(int n_groups, int n_cols, long long *rank2, long long *ties) {
    std::fill(rank2, rank2 + (size_t)n_groups * n_cols, 0LL);
    std::fill(ties, ties + n_cols, 0LL);
}

template <typename T>
int dense(const void *y, long long y_ld, long long n, const int *codes, const long long *count, long long n_used, int n_groups, const int *cols,
          int n_cols, long long *rank2, long long *ties, long long *bad_row, int *bad_col) {
    typedef typename pilot::RsKey<T>::Rec Rec;
    const long long rows_per = std::max<long long>(pilot::RS_SCAN_ROWS, (n + 65534) / 65535);
    const dim3 grid((unsigned)((n_cols + 63) / 64), (unsigned)((n + rows_per - 1) / rows_per));
    return run<T>(codes, n, count, n_used, n_groups, cols, n_cols, rank2, ties, bad_row, bad_col, [&](bool fill, const DevScan &d) {
        if (fill)
            hipLaunchKernelGGL((pilot::rs_dense_scan_kernel<T, true>), grid, dim3(256), 0, nullptr, static_cast<const T *>(y), y_ld, n, rows_per,
                               d.codes, d.cols, n_cols, d.len, d.off, static_cast<Rec *>(d.rec), d.bad);
        else
            hipLaunchKernelGGL((pilot::rs_dense_scan_kernel<T, false>), grid, dim3(256), 0, nullptr, static_cast<const T *>(y), y_ld, n, rows_per,
                               d.codes, d.cols, n_cols, d.len, d.off, static_cast<Rec *>(d.rec), d.bad);
    });
}

template <typename T>
int sparse(const pilot_ot_csr *c, const int *codes, const long long *count, long long n_used, int n_groups, const int *cols, int n_cols,
           long long *rank2, long long *ties, long long *bad_row, int *bad_col) {
    typedef typename pilot::RsKey<T>::Rec Rec;
    return run<T>(codes, c->n, count, n_used, n_groups, cols, n_cols, rank2, ties, bad_row, bad_col, [&](bool fill, const DevScan &d) {
        if (fill)
            hipLaunchKernelGGL((pilot::rs_csr_scan_kernel<T, true>), dim3((unsigned)n_cols), dim3(256), 0, nullptr, c->colptr, c->rowidx,
                               static_cast<const T *>(c->cdata), d.codes, d.cols, d.len, d.off, static_cast<Rec *>(d.rec), d.bad);
        else
            hipLaunchKernelGGL((pilot::rs_csr_scan_kernel<T, false>), dim3((unsigned)n_cols), dim3(256), 0, nullptr, c->colptr, c->rowidx,
                               static_cast<const T *>(c->cdata), d.codes, d.cols, d.len, d.off, static_cast<Rec *>(d.rec), d.bad);
    });
}

}  // namespace

PILOT_API int pilot_ot_rank_sums_wave_max(void) { return pilot::RS_WAVE_MAX; }
PILOT_API int pilot_ot_rank_sums_wg_max(void) { return pilot::RS_WG_MAX; }
PILOT_API int pilot_ot_rank_sums_sort_tile(void) { return pilot::RS_SORT_TILE; }

PILOT_API int pilot_ot_rank_sums(const void *Y, int Y_is_device, int dtype, long long n, int n_cols_total, long long ld, const int *codes,
                                 int n_groups, const int *cols, int n_cols, long long *count, long long *rank2, long long *ties,
                                 long long *bad_row, int *bad_col) {
    if (bad_row) *bad_row = -1;
    if (bad_col) *bad_col = -1;
    if (!Y || !count || !rank2 || !ties || (!codes && n > 0)) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (n < 0 || n_cols_total < 1) return fail(PILOT_OT_EINVAL, "n=%lld, n_cols_total=%d", n, n_cols_total);
    if (int rc = pilot::check_ld(ld, n_cols_total)) return rc;
    if (int rc = pilot::check_dtype(dtype)) return rc;
    if (int rc = check_groups(n_groups)) return rc;
    if (int rc = pilot::check_cols(cols, n_cols, n_cols_total)) return rc;
    long long n_used = 0;
    if (int rc = count_rows(codes, n, n_groups, count, &n_used)) return rc;
    if (n_cols == 0) return PILOT_OT_OK;
    if (n_used == 0) {
        nothing_used(n_groups, n_cols, rank2, ties);
        return PILOT_OT_OK;
    }
    const void *y;
    long long y_ld;
    if (int rc = pilot::stage_dense(Y, Y_is_device, pilot::elem_size(dtype), n, n_cols_total, ld, pilot::WS_RS_Y, &y, &y_ld)) return rc;
    return dtype == 0 ? dense<float>(y, y_ld, n, codes, count, n_used, n_groups, cols, n_cols, rank2, ties, bad_row, bad_col)
                      : dense<double>(y, y_ld, n, codes, count, n_used, n_groups, cols, n_cols, rank2, ties, bad_row, bad_col);
}

PILOT_API int pilot_ot_csr_rank_sums(pilot_ot_csr *c, const int *codes, int n_groups, const int *cols, int n_cols, long long *count,
                                     long long *rank2, long long *ties, long long *bad_row, int *bad_col) {
    if (bad_row) *bad_row = -1;
    if (bad_col) *bad_col = -1;
    if (int rc = check_groups(n_groups)) return rc;
    if (n_cols < 0) return fail(PILOT_OT_EINVAL, "n_cols=%d", n_cols);
    if (!c || !count || !rank2 || !ties || (!codes && c->n > 0)) return fail(PILOT_OT_EINVAL, "NULL pointer (csr, codes, count, rank2 or ties)");
    if (int rc = pilot::check_cols(cols, n_cols, c->n_cols)) return rc;
    long long n_used = 0;
    if (int rc = count_rows(codes, c->n, n_groups, count, &n_used)) return rc;
    if (n_cols == 0) return PILOT_OT_OK;
    if (n_used == 0) {
        nothing_used(n_groups, n_cols, rank2, ties);
        return PILOT_OT_OK;
    }
    if (int rc = pilot_ot_csr_build_columns(c)) return rc;
    return c->dtype == 0 ? sparse<float>(c, codes, count, n_used, n_groups, cols, n_cols, rank2, ties, bad_row, bad_col)
                         : sparse<double>(c, codes, count, n_used, n_groups, cols, n_cols, rank2, ties, bad_row, bad_col);
}
