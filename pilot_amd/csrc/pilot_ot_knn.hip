// C ABI of the cell neighbour graph (include/pilot_ot.h, section "cell neighbours"; kernels: knn_kernels.hpp, knn_smooth_kernel.hpp).
// The matrix is a dense row-major one on the host or in HBM; the results are host arrays, so the calls synchronise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "abi_common.hpp"
#include "knn_host.hpp"
#include "knn_smooth_kernel.hpp"

namespace {

template <typename T>
int knn_rows(const void *x, long long ld, int n, int D, int metric, int k, long long row_begin, int m, int *indices, double *distances) {
    const T *X = static_cast<const T *>(x);
    hipStream_t s = nullptr;
    if (int rc = pilot::knn_checked_rows(&X, &ld, n, D, metric, pilot::WS_KNN_FLAGS, pilot::WS_KNN_UNIT)) return rc;
    T *best_d;
    int *best_i, *out_i;
    double *out_d;
    HIP_TRY(pilot::ws(pilot::WS_KNN_BEST_D, (size_t)m * k, &best_d));
    HIP_TRY(pilot::ws(pilot::WS_KNN_BEST_I, (size_t)m * k, &best_i));
    HIP_TRY(pilot::ws(pilot::WS_KNN_OUT_I, (size_t)m * k, &out_i));
    HIP_TRY(pilot::ws(pilot::WS_KNN_OUT_D, (size_t)m * k, &out_d));
    const long long blocks = ((long long)m + pilot::KNN_THREADS - 1) / pilot::KNN_THREADS;
    for (long long b0 = 0; b0 < blocks; b0 += pilot::KNN_GRID_MAX) {
        const unsigned grid = (unsigned)std::min<long long>(pilot::KNN_GRID_MAX, blocks - b0);
        const int q0 = (int)(b0 * pilot::KNN_THREADS);
        if (D <= pilot::KNN_REGQ_D)
            hipLaunchKernelGGL((pilot::knn_rows_kernel<T, true>), dim3(grid), dim3(pilot::KNN_THREADS), 0, s, X, ld, n, D, k, metric, row_begin, m,
                               q0, best_d, best_i, out_i, out_d);
        else
            hipLaunchKernelGGL((pilot::knn_rows_kernel<T, false>), dim3(grid), dim3(pilot::KNN_THREADS), 0, s, X, ld, n, D, k, metric, row_begin, m,
                               q0, best_d, best_i, out_i, out_d);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(indices, out_i, sizeof(int) * (size_t)m * k, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(distances, out_d, sizeof(double) * (size_t)m * k, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}

}  // namespace

PILOT_API int pilot_ot_knn_rows(const void *X, int X_is_device, int dtype, long long n, int D, long long ld, int metric, int k,
                                long long row_begin, long long row_end, int *indices, double *distances) {
    if (!X || !indices || !distances) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (D < 1) return fail(PILOT_OT_EINVAL, "D=%d columns", D);
    if (int rc = pilot::check_ld(ld, D)) return rc;
    if (int rc = pilot::check_dtype(dtype)) return rc;
    if (metric != 0 && metric != 1) return fail(PILOT_OT_EINVAL, "metric=%d must be 0 (euclidean) or 1 (cosine)", metric);
    if (k < 1) return fail(PILOT_OT_EINVAL, "k=%d neighbours", k);
    if (k > PILOT_OT_KNN_ROWS_MAX_K) return fail(PILOT_OT_ENOTSUP, "k=%d neighbours: at most %d", k, PILOT_OT_KNN_ROWS_MAX_K);
    if (n < (long long)k + 1) return fail(PILOT_OT_EINVAL, "n=%lld rows: k=%d neighbours need at least k + 1", n, k);
    if (n > INT_MAX) return fail(PILOT_OT_ENOTSUP, "n=%lld rows need more than 32-bit row indices", n);
    if (row_begin < 0 || row_end > n || row_begin >= row_end)
        return fail(PILOT_OT_EINVAL, "row range [%lld, %lld) outside [0, %lld) or empty", row_begin, row_end, n);

    const void *x;
    long long x_ld;
    if (int rc = pilot::stage_dense(X, X_is_device, pilot::elem_size(dtype), n, D, ld, pilot::WS_KNN_X, &x, &x_ld)) return rc;
    const int m = (int)(row_end - row_begin);
    return dtype == 0 ? knn_rows<float>(x, x_ld, (int)n, D, metric, k, row_begin, m, indices, distances)
                      : knn_rows<double>(x, x_ld, (int)n, D, metric, k, row_begin, m, indices, distances);
}

PILOT_API int pilot_ot_knn_smooth(const double *distances, long long n, int k, double *weights, double *sigma, double *rho) {
    if (!distances || !weights || !sigma || !rho) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (k < 1) return fail(PILOT_OT_EINVAL, "k=%d neighbours", k);
    if (k > PILOT_OT_KNN_ROWS_MAX_K) return fail(PILOT_OT_ENOTSUP, "k=%d neighbours: at most %d", k, PILOT_OT_KNN_ROWS_MAX_K);
    if (n < 1) return fail(PILOT_OT_EINVAL, "n=%lld rows", n);
    if (n > INT_MAX) return fail(PILOT_OT_ENOTSUP, "n=%lld rows need more than 32-bit row indices", n);
    const size_t count = (size_t)n * k;
    double total = 0.0;                                        // the global mean distance: the sigma floor of rows with rho = 0
    for (size_t e = 0; e < count; ++e) {
        if (!(distances[e] >= 0.0) || std::isinf(distances[e]))
            return fail(PILOT_OT_EINVAL, "distances[%lld, %d]=%g must be finite and not negative", (long long)(e / k), (int)(e % k), distances[e]);
        total += distances[e];
    }
    double *in, *out;
    HIP_TRY(pilot::ws(pilot::WS_KNN_SM_IN, count, &in));
    HIP_TRY(pilot::ws(pilot::WS_KNN_SM_OUT, count + 2 * (size_t)n, &out));
    HIP_TRY(hipMemcpy(in, distances, sizeof(double) * count, hipMemcpyHostToDevice));
    double *d_sigma = out + count, *d_rho = d_sigma + n;
    hipLaunchKernelGGL(pilot::knn_smooth_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, in, n, k, total / (double)count, out,
                       d_sigma, d_rho);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(weights, out, sizeof(double) * count, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sigma, d_sigma, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rho, d_rho, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}
