// C ABI of PERMANOVA (include/pilot_ot.h, section "PERMANOVA"; kernels: permanova_kernels.hpp).  The distance matrix is a host
// array or a buffer in HBM; rows, Q, the term offsets, the strata and the results are host arrays.  A consumer of the distance
// matrix: its temporaries are the WS_CONS_* slots, which no other call holds while this one runs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "abi_common.hpp"
#include "permanova_kernels.hpp"

namespace {

using pilot::rs_u64;

long long chunk_perms() {
    long long chunk = pilot::PM_CHUNK_PERMS;
    if (const char *e = pilot::test_switch("PILOT_OT_PERMANOVA_CHUNK")) { const long v = atol(e); if (v > 0 && v < chunk) chunk = v; }   // (tests)
    return chunk;
}

// n, strata, the window of permutations.  No HIP call.
int check_perm_args(int n, const int *strata, long long start, long long count) {
    if (n < 1) return fail(PILOT_OT_EINVAL, "n=%d samples", n);
    if (n > pilot::PM_MAX_N) return fail(PILOT_OT_ENOTSUP, "n=%d samples do not fit the LDS sort (at most %d)", n, pilot::PM_MAX_N);
    if (start < 0 || count < 0) return fail(PILOT_OT_EINVAL, "start=%lld, count=%lld", start, count);
    for (int i = 0; strata && i < n; ++i)
        if (strata[i] < 0) return fail(PILOT_OT_EINVAL, "strata[%d]=%d is negative", i, strata[i]);
    return PILOT_OT_OK;
}

// strata[n] | rorder[n] (the rows ordered by (stratum, i)) | rows[n] (when given) in WS_CONS_SIZES
struct DevInts {
    int *strata, *rorder, *rows;
};
int upload_ints(int n, const int *strata, const int *rows, DevInts *d) {
    std::vector<int> h(3 * (size_t)n, 0);
    int *order = h.data() + n;
    std::iota(order, order + n, 0);
    if (strata) {
        std::copy(strata, strata + n, h.data());
        std::stable_sort(order, order + n, [&](int a, int b) { return strata[a] < strata[b]; });
    }
    if (rows) std::copy(rows, rows + n, h.data() + 2 * (size_t)n);
    int *dev;
    HIP_TRY(pilot::ws(pilot::WS_CONS_SIZES, h.size(), &dev));
    HIP_TRY(hipMemcpy(dev, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice));
    d->strata = dev;
    d->rorder = dev + n;
    d->rows = rows ? dev + 2 * (size_t)n : nullptr;
    return PILOT_OT_OK;
}

int launch_permute(int n, const DevInts &d, rs_u64 seed, long long start, long long count, int *perm) {
    int P = 1;
    while (P < n) P <<= 1;
    const size_t lds = sizeof(pilot::PmRec) * (size_t)P;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pilot::pm_permute_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(pilot::pm_permute_kernel, dim3((unsigned)count), dim3(pilot::PM_THREADS), lds, nullptr, n, P, d.strata, d.rorder, seed, start,
                       perm);
    HIP_TRY(hipGetLastError());
    return PILOT_OT_OK;
}

struct Clock {      // device time between two points of the launch stream, when the caller asks for it
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool on;
    explicit Clock(bool want) : on(want) {
        if (on && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)) on = false;
    }
    ~Clock() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
    void start() { if (on) (void)hipEventRecord(ev[0], nullptr); }
    void stop(float *sum) {
        float ms = 0.f;
        if (on && hipEventRecord(ev[1], nullptr) == hipSuccess && hipEventSynchronize(ev[1]) == hipSuccess &&
            hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
            *sum += ms;
    }
};

template <typename T>
int run(const void *D, long long ld, int n, const double *Q, int c, const int *term_off, int n_terms, const DevInts &ints, rs_u64 seed,
        long long start, long long count, double *ss_total, double *ss, long long *bad_row, long long *bad_col, float *kernel_ms) {
    const int NP = (n + pilot::PM_RB - 1) / pilot::PM_RB * pilot::PM_RB, n_blocks = NP / pilot::PM_RB;
    // at most PM_CHUNK_COLS columns a pass: what bounds the partial sums whatever c is
    const long long chunk = std::min({chunk_perms(), std::max<long long>(count, 1), std::max<long long>(pilot::PM_CHUNK_COLS / c, 1)});
    const long long max_cols = chunk * c, max_pad = (max_cols + pilot::PM_COLS - 1) / pilot::PM_COLS * pilot::PM_COLS;
    double *d_A, *d_aux, *d_q, *d_partial;
    int *d_perm, *d_off;
    // aux: rowsum[NP] | total | bad;   q: Q[n c] | ss[chunk n_terms] | term_off (ints)
    HIP_TRY(pilot::ws(pilot::WS_CONS_E, (size_t)NP * NP, &d_A));
    HIP_TRY(pilot::ws(pilot::WS_CONS_MAX, (size_t)NP + 2, &d_aux));
    const size_t n_q = (size_t)n * c, n_ss = (size_t)chunk * n_terms;
    HIP_TRY(pilot::ws(pilot::WS_CONS_K, n_q + n_ss + ((size_t)n_terms + 2) / 2 + 1, &d_q));
    HIP_TRY(pilot::ws(pilot::WS_CONS_SCORES, (size_t)n_blocks * max_pad, &d_partial));
    HIP_TRY(pilot::ws(pilot::WS_CONS_LABELS, (size_t)chunk * n, &d_perm));
    double *d_ss = d_q + n_q;
    d_off = reinterpret_cast<int *>(d_ss + n_ss);
    rs_u64 *d_bad = reinterpret_cast<rs_u64 *>(d_aux + NP + 1);
    HIP_TRY(hipMemcpy(d_q, Q, sizeof(double) * n_q, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_off, term_off, sizeof(int) * ((size_t)n_terms + 1), hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(d_bad, 0xFF, sizeof(rs_u64), nullptr));
    Clock clock(kernel_ms != nullptr);
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0.f;
    clock.start();
    hipLaunchKernelGGL(pilot::pm_prepare_kernel<T>, dim3((unsigned)NP), dim3(pilot::PM_THREADS), 0, nullptr, static_cast<const T *>(D), ld, ints.rows,
                       n, NP, d_A, d_aux, d_bad);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pilot::pm_total_kernel, dim3(1), dim3(pilot::PM_THREADS), 0, nullptr, d_aux, n, d_aux + NP);
    HIP_TRY(hipGetLastError());
    if (kernel_ms) clock.stop(&kernel_ms[0]);
    double total = 0.0;
    rs_u64 bad = 0;
    HIP_TRY(hipMemcpy(&total, d_aux + NP, sizeof total, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost));
    if (bad != pilot::PM_NO_BAD) {
        const long long r = (long long)(bad >> 32), cidx = (long long)(bad & 0xFFFFFFFFull);
        if (bad_row) *bad_row = r;
        if (bad_col) *bad_col = cidx;
        return fail(PILOT_OT_EINVAL, "D[%lld, %lld] is NaN or infinite (both samples are used)", r, cidx);
    }
    *ss_total = -(1.0 / (double)n) * total;
    for (long long done = 0; done < count; done += chunk) {
        const long long m = std::min(chunk, count - done), ncols = m * c;
        const long long ncols_pad = (ncols + pilot::PM_COLS - 1) / pilot::PM_COLS * pilot::PM_COLS;
        clock.start();
        if (int rc = launch_permute(n, ints, seed, start + done, m, d_perm)) return rc;
        if (kernel_ms) clock.stop(&kernel_ms[1]);
        clock.start();
        hipLaunchKernelGGL(pilot::pm_quad_kernel, dim3((unsigned)(ncols_pad / pilot::PM_COLS), (unsigned)n_blocks), dim3(pilot::PM_THREADS), 0,
                           nullptr, d_A, NP, n, d_q, c, d_perm, ncols, d_partial, ncols_pad);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(pilot::pm_terms_kernel, dim3((unsigned)((m * n_terms + 255) / 256)), dim3(256), 0, nullptr, d_partial, ncols_pad, n_blocks,
                           c, d_off, n_terms, m, d_ss);
        HIP_TRY(hipGetLastError());
        if (kernel_ms) clock.stop(&kernel_ms[2]);
        HIP_TRY(hipMemcpy(ss + (size_t)done * n_terms, d_ss, sizeof(double) * (size_t)m * n_terms, hipMemcpyDeviceToHost));
    }
    return PILOT_OT_OK;
}

}  // namespace

PILOT_API int pilot_ot_permanova_limits(int *max_n, int *chunk, int *tile_cols, int *row_block) {
    if (max_n) *max_n = pilot::PM_MAX_N;
    if (chunk) *chunk = (int)chunk_perms();
    if (tile_cols) *tile_cols = pilot::PM_COLS;
    if (row_block) *row_block = pilot::PM_RB;
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_permanova_permutations(int n, const int *strata, unsigned long long seed, long long start, long long count, int *perm) {
    if (int rc = check_perm_args(n, strata, start, count)) return rc;
    if (!perm && count > 0) return fail(PILOT_OT_EINVAL, "NULL pointer (perm)");
    if (count == 0) return PILOT_OT_OK;
    DevInts ints;
    if (int rc = upload_ints(n, strata, nullptr, &ints)) return rc;
    const long long chunk = std::min(chunk_perms(), count);
    int *d_perm;
    HIP_TRY(pilot::ws(pilot::WS_CONS_LABELS, (size_t)chunk * n, &d_perm));
    for (long long done = 0; done < count; done += chunk) {
        const long long m = std::min(chunk, count - done);
        if (int rc = launch_permute(n, ints, seed, start + done, m, d_perm)) return rc;
        HIP_TRY(hipMemcpy(perm + (size_t)done * n, d_perm, sizeof(int) * (size_t)m * n, hipMemcpyDeviceToHost));
    }
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_permanova(const void *D, int D_is_device, int dtype, int N, long long ld, const int *rows, int n, const double *Q, int c,
                                 const int *term_off, int n_terms, const int *strata, unsigned long long seed, long long start, long long count,
                                 double *ss_total, double *ss, long long *bad_row, long long *bad_col, float *kernel_ms) {
    if (bad_row) *bad_row = -1;
    if (bad_col) *bad_col = -1;
    if (!D || !Q || !term_off || !ss_total || (!ss && count > 0)) return fail(PILOT_OT_EINVAL, "NULL pointer (D, Q, term_off, ss_total or ss)");
    if (N < 1) return fail(PILOT_OT_EINVAL, "N=%d", N);
    if (int rc = pilot::check_ld(ld, N)) return rc;
    if (int rc = pilot::check_dtype(dtype)) return rc;
    if (!rows && n != N) return fail(PILOT_OT_EINVAL, "n=%d samples without rows (it must be N=%d)", n, N);
    if (int rc = check_perm_args(n, strata, start, count)) return rc;
    for (int i = 0; rows && i < n; ++i)
        if (rows[i] < 0 || rows[i] >= N || (i > 0 && rows[i] <= rows[i - 1]))
            return fail(PILOT_OT_EINVAL, "rows[%d]=%d: the used rows are ascending and inside [0, %d)", i, rows[i], N);
    if (c < 1 || c > pilot::PM_MAX_COLS || n_terms < 1 || n_terms > c)
        return fail(PILOT_OT_EINVAL, "c=%d columns (1 to %d) in n_terms=%d terms (1 to c)", c, pilot::PM_MAX_COLS, n_terms);
    if (term_off[0] != 0 || term_off[n_terms] != c) return fail(PILOT_OT_EINVAL, "term_off runs from 0 to c=%d", c);
    for (int t = 0; t < n_terms; ++t)
        if (term_off[t + 1] <= term_off[t]) return fail(PILOT_OT_EINVAL, "term %d has no column (term_off ascends strictly)", t);
    for (int j = 0; j < c; ++j) {      // centred columns: what makes z^T A z the centred form
        double s = 0.0, a = 0.0;
        for (int i = 0; i < n; ++i) { const double q = Q[(size_t)i * c + j]; s += q; a += std::fabs(q); }
        if (!(std::fabs(s) <= 1e-8 * (1.0 + a))) return fail(PILOT_OT_EINVAL, "column %d of Q is not centred (sum %g) or not finite", j, s);
    }
    DevInts ints;
    if (int rc = upload_ints(n, strata, rows, &ints)) return rc;
    const void *d;
    long long d_ld;
    if (int rc = pilot::stage_dense(D, D_is_device, pilot::elem_size(dtype), N, N, ld, pilot::WS_CONS_D, &d, &d_ld)) return rc;
    return dtype == 0 ? run<float>(d, d_ld, n, Q, c, term_off, n_terms, ints, seed, start, count, ss_total, ss, bad_row, bad_col, kernel_ms)
                      : run<double>(d, d_ld, n, Q, c, term_off, n_terms, ints, seed, start, count, ss_total, ss, bad_row, bad_col, kernel_ms);
}
