// C ABI of the elastic principal tree (include/pilot_ot.h, section "elastic principal tree"; kernels: principal_tree_kernels.hpp on
// top of knn_kernels.hpp).  The points are a dense row-major matrix on the host or in HBM; the candidates and every result are
// host arrays, so each call synchronises once, at its read-back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "abi_common.hpp"
#include "knn_host.hpp"
#include "principal_tree_kernels.hpp"

static_assert(pilot::PT_CONVERGED == PILOT_OT_ELASTIC_CONVERGED && pilot::PT_SINGULAR == PILOT_OT_ELASTIC_SINGULAR, "state bits");
static_assert(pilot::PT_MAX_M == PILOT_OT_ELASTIC_MAX_NODES && pilot::PT_MAX_D == PILOT_OT_ELASTIC_MAX_D, "limits");

namespace {

constexpr size_t PARTIAL_BYTES = (size_t)512 << 20;      // the per-block partials of the candidates in flight

bool all_finite(const double *v, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// what the three entry points check of their matrix argument, before any HIP call
int check_points(const void *X, int dtype, long long n, int D, long long ld) {
    if (!X) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (D < 1 || D > pilot::PT_MAX_D) return fail(PILOT_OT_EINVAL, "D=%d columns outside [1, %d]", D, pilot::PT_MAX_D);
    if (int rc = pilot::check_ld(ld, D)) return rc;
    if (int rc = pilot::check_dtype(dtype)) return rc;
    if (n < 1) return fail(PILOT_OT_EINVAL, "n=%lld rows", n);
    if (n > INT_MAX) return fail(PILOT_OT_ENOTSUP, "n=%lld rows need more than 32-bit row indices", n);
    return PILOT_OT_OK;
}

template <typename T> hipError_t upload(pilot::WsSlot slot, const T *src, size_t count, T **dst) {
    hipError_t e = pilot::ws(slot, count, dst);
    return e != hipSuccess ? e : hipMemcpy(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice);
}

template <typename T>
int elastic_fit(const void *x, long long ld, int n, int D, int B, int m, const double *Y0, const double *S, const double *centre,
                int max_iter, double eps, double *Y, double *energy, int *iters, int *flags, int *counts, double *sums) {
    const T *X = static_cast<const T *>(x);
    hipStream_t s = nullptr;
    if (int rc = pilot::knn_checked_rows(&X, &ld, n, D, 0, pilot::WS_PT_FLAGS, pilot::WS_PT_FLAGS)) return rc;

    const size_t md = (size_t)m * D, nY = (size_t)B * md;
    const int n_chunks = (int)(((long long)n + pilot::KNN_THREADS - 1) / pilot::KNN_THREADS);
    const int chunks = (n_chunks + pilot::PT_MAX_QBLOCKS - 1) / pilot::PT_MAX_QBLOCKS;
    const int Q = (n_chunks + chunks - 1) / chunks;
    const size_t per_cand = (size_t)Q * (md * sizeof(double) + (size_t)m * sizeof(int) + sizeof(double));
    const int Bc = (int)std::min<size_t>(std::max<size_t>(PARTIAL_BYTES / per_cand, 1), (size_t)std::min(B, 65535));

    std::vector<T> yt(nY);
    for (size_t i = 0; i < nY; ++i) yt[i] = (T)Y0[i];
    double *d_Y, *d_S, *d_c, *d_energy, *d_sums, *p_sums, *p_mse;
    T *d_YT;
    int *d_state, *d_iters, *d_counts, *p_counts;
    HIP_TRY(upload(pilot::WS_PT_Y, Y0, nY, &d_Y));
    HIP_TRY(upload(pilot::WS_PT_YT, yt.data(), nY, &d_YT));
    HIP_TRY(upload(pilot::WS_PT_S, S, (size_t)B * m * m, &d_S));
    HIP_TRY(upload(pilot::WS_PT_CENTRE, centre, (size_t)D, &d_c));
    HIP_TRY(pilot::ws(pilot::WS_PT_STATE, (size_t)B, &d_state));
    HIP_TRY(pilot::ws(pilot::WS_PT_ITERS, (size_t)B, &d_iters));
    HIP_TRY(pilot::ws(pilot::WS_PT_ENERGY, (size_t)B * 2, &d_energy));
    HIP_TRY(pilot::ws(pilot::WS_PT_COUNTS, (size_t)B * m, &d_counts));
    HIP_TRY(pilot::ws(pilot::WS_PT_SUMS, nY, &d_sums));
    HIP_TRY(pilot::ws(pilot::WS_PT_PCOUNTS, (size_t)Bc * Q * m, &p_counts));
    HIP_TRY(pilot::ws(pilot::WS_PT_PSUMS, (size_t)Bc * Q * md, &p_sums));
    HIP_TRY(pilot::ws(pilot::WS_PT_PMSE, (size_t)Bc * Q, &p_mse));
    HIP_TRY(hipMemsetAsync(d_state, 0, sizeof(int) * (size_t)B, s));
    HIP_TRY(hipMemsetAsync(d_iters, 0, sizeof(int) * (size_t)B, s));
    HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(int) * (size_t)B * m, s));
    HIP_TRY(hipMemsetAsync(d_sums, 0, sizeof(double) * nY, s));

    for (int b0 = 0; b0 < B; b0 += Bc) {
        const int nb = std::min(Bc, B - b0);
        for (int it = 0; it <= max_iter; ++it) {
            const int final_pass = it == max_iter;
            hipLaunchKernelGGL(pilot::pt_partition_kernel<T>, dim3((unsigned)Q, (unsigned)nb), dim3(pilot::KNN_THREADS), 0, s, X, ld, n, D, m,
                               chunks, d_YT + (size_t)b0 * md, d_Y + (size_t)b0 * md, d_state + b0, final_pass, p_counts, p_sums, p_mse);
            hipLaunchKernelGGL(pilot::pt_finish_kernel<T>, dim3((unsigned)nb), dim3(pilot::PT_FIN_THREADS), 0, s, n, D, m, Q, final_pass, eps,
                               d_S + (size_t)b0 * m * m, d_c, p_counts, p_sums, p_mse, d_Y + (size_t)b0 * md, d_YT + (size_t)b0 * md,
                               d_state + b0, d_iters + b0, d_energy + 2 * (size_t)b0, d_counts + (size_t)b0 * m,
                               d_sums + (size_t)b0 * md);
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(Y, d_Y, sizeof(double) * nY, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(energy, d_energy, sizeof(double) * 2 * (size_t)B, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(iters, d_iters, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(flags, d_state, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counts, d_counts, sizeof(int) * (size_t)B * m, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sums, d_sums, sizeof(double) * nY, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}

template <typename T> int point_moments(const void *x, long long ld, int n, int D, double *mean, double *cross) {
    const T *X = static_cast<const T *>(x);
    hipStream_t s = nullptr;
    if (int rc = pilot::knn_checked_rows(&X, &ld, n, D, 0, pilot::WS_PT_FLAGS, pilot::WS_PT_FLAGS)) return rc;
    // blocks of at least 1024 rows, at most 1024 of them: the order of every sum depends on n alone
    const long long rows_per_block = std::max<long long>(1024, ((long long)n + 1023) / 1024);
    const int G = (int)((n + rows_per_block - 1) / rows_per_block);
    double *part, *out;
    HIP_TRY(pilot::ws(pilot::WS_PT_PART, (size_t)G * D * D, &part));
    HIP_TRY(pilot::ws(pilot::WS_PT_OUT, (size_t)D + (size_t)D * D, &out));
    hipLaunchKernelGGL(pilot::pt_moments_kernel<T>, dim3((unsigned)G), dim3(256), 0, s, X, ld, (long long)n, D, rows_per_block,
                       (const double *)nullptr, part);
    hipLaunchKernelGGL(pilot::pt_reduce_kernel, dim3(1), dim3(64), 0, s, part, G, D, (double)n, out);
    hipLaunchKernelGGL(pilot::pt_moments_kernel<T>, dim3((unsigned)G), dim3(256), 0, s, X, ld, (long long)n, D, rows_per_block,
                       (const double *)out, part);
    hipLaunchKernelGGL(pilot::pt_reduce_kernel, dim3((unsigned)((D * D + 255) / 256)), dim3(256), 0, s, part, G, D * D, 1.0, out + D);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(mean, out, sizeof(double) * (size_t)D, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cross, out + D, sizeof(double) * (size_t)D * D, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}

template <typename T>
int tree_projection(const void *x, long long ld, int n, int D, int m, const double *nodes, int n_edges, const int *edges,
                    const double *base, double *pseudotime, double *d2, int *edge, double *t) {
    const T *X = static_cast<const T *>(x);
    hipStream_t s = nullptr;
    if (int rc = pilot::knn_checked_rows(&X, &ld, n, D, 0, pilot::WS_PT_FLAGS, pilot::WS_PT_FLAGS)) return rc;
    // the fit's slots, free here: a projection and a fit are never in flight together on one thread
    double *d_nodes, *d_base, *res;
    int *d_edges, *d_edge;
    HIP_TRY(upload(pilot::WS_PT_Y, nodes, (size_t)m * D, &d_nodes));
    HIP_TRY(upload(pilot::WS_PT_CENTRE, base, (size_t)m, &d_base));
    HIP_TRY(upload(pilot::WS_PT_STATE, edges, (size_t)2 * n_edges, &d_edges));
    HIP_TRY(pilot::ws(pilot::WS_PT_OUT, (size_t)3 * n, &res));
    HIP_TRY(pilot::ws(pilot::WS_PT_COUNTS, (size_t)n, &d_edge));
    hipLaunchKernelGGL(pilot::pt_projection_kernel<T>, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, s, X, ld, (long long)n, D, m, d_nodes,
                       n_edges, d_edges, d_base, res, res + n, d_edge, res + 2 * (size_t)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(pseudotime, res, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(d2, res + n, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(t, res + 2 * (size_t)n, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(edge, d_edge, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}

}  // namespace

PILOT_API int pilot_ot_elastic_fit_batch(const void *X, int X_is_device, int dtype, long long n, int D, long long ld, int B, int m,
                                         const double *Y0, const double *S, const double *centre, int max_iter, double eps, double *Y,
                                         double *energy, int *iters, int *flags, int *counts, double *sums) {
    if (!Y0 || !S || !centre || !Y || !energy || !iters || !flags || !counts || !sums) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (int rc = check_points(X, dtype, n, D, ld)) return rc;
    if (m < 2 || m > pilot::PT_MAX_M) return fail(PILOT_OT_EINVAL, "m=%d nodes outside [2, %d]", m, pilot::PT_MAX_M);
    if (B < 1) return fail(PILOT_OT_EINVAL, "B=%d candidates", B);
    if (max_iter < 1) return fail(PILOT_OT_EINVAL, "max_iter=%d must be at least 1", max_iter);
    if (!(eps >= 0.0)) return fail(PILOT_OT_EINVAL, "eps=%g must be at least 0", eps);
    if (!all_finite(Y0, (size_t)B * m * D)) return fail(PILOT_OT_EINVAL, "a start position is not finite");
    if (!all_finite(S, (size_t)B * m * m)) return fail(PILOT_OT_EINVAL, "a spring matrix entry is not finite");
    if (!all_finite(centre, (size_t)D)) return fail(PILOT_OT_EINVAL, "the centre is not finite");
    const void *x;
    long long x_ld;
    if (int rc = pilot::stage_dense(X, X_is_device, pilot::elem_size(dtype), n, D, ld, pilot::WS_PT_X, &x, &x_ld)) return rc;
    return dtype == 0 ? elastic_fit<float>(x, x_ld, (int)n, D, B, m, Y0, S, centre, max_iter, eps, Y, energy, iters, flags, counts, sums)
                      : elastic_fit<double>(x, x_ld, (int)n, D, B, m, Y0, S, centre, max_iter, eps, Y, energy, iters, flags, counts, sums);
}

PILOT_API int pilot_ot_point_moments(const void *X, int X_is_device, int dtype, long long n, int D, long long ld, double *mean,
                                     double *cross) {
    if (!mean || !cross) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (int rc = check_points(X, dtype, n, D, ld)) return rc;
    const void *x;
    long long x_ld;
    if (int rc = pilot::stage_dense(X, X_is_device, pilot::elem_size(dtype), n, D, ld, pilot::WS_PT_X, &x, &x_ld)) return rc;
    return dtype == 0 ? point_moments<float>(x, x_ld, (int)n, D, mean, cross) : point_moments<double>(x, x_ld, (int)n, D, mean, cross);
}

PILOT_API int pilot_ot_tree_projection(const void *X, int X_is_device, int dtype, long long n, int D, long long ld, int m,
                                       const double *nodes, int n_edges, const int *edges, const double *base, double *pseudotime,
                                       double *d2, int *edge, double *t) {
    if (!nodes || !edges || !base || !pseudotime || !d2 || !edge || !t) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (int rc = check_points(X, dtype, n, D, ld)) return rc;
    if (m < 2 || m > pilot::PT_MAX_M) return fail(PILOT_OT_EINVAL, "m=%d nodes outside [2, %d]", m, pilot::PT_MAX_M);
    if (n_edges < 1 || n_edges >= m) return fail(PILOT_OT_EINVAL, "n_edges=%d outside [1, m - 1 = %d]", n_edges, m - 1);
    for (int e = 0; e < 2 * n_edges; ++e)
        if (edges[e] < 0 || edges[e] >= m) return fail(PILOT_OT_EINVAL, "edge %d names node %d outside [0, %d)", e / 2, edges[e], m);
    if (!all_finite(nodes, (size_t)m * D)) return fail(PILOT_OT_EINVAL, "a node position is not finite");
    if (!all_finite(base, (size_t)m)) return fail(PILOT_OT_EINVAL, "a base distance is not finite");
    const void *x;
    long long x_ld;
    if (int rc = pilot::stage_dense(X, X_is_device, pilot::elem_size(dtype), n, D, ld, pilot::WS_PT_X, &x, &x_ld)) return rc;
    return dtype == 0 ? tree_projection<float>(x, x_ld, (int)n, D, m, nodes, n_edges, edges, base, pseudotime, d2, edge, t)
                      : tree_projection<double>(x, x_ld, (int)n, D, m, nodes, n_edges, edges, base, pseudotime, d2, edge, t);
}
