// C ABI of the silhouette of labelled rows (include/pilot_ot.h, section "silhouette of labelled rows"; kernels:
// silhouette_kernels.hpp on top of knn_kernels.hpp).  The matrix is a dense row-major one on the host or in HBM; the results are
// host arrays, so the call synchronises.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <vector>

#include "abi_common.hpp"
#include "knn_host.hpp"
#include "silhouette_kernels.hpp"

namespace {

template <typename T>
int silhouette_points(const void *x, long long ld, int n, int D, int metric, const int *order, const int *offsets, int n_clusters,
                      double *samples) {
    const T *X = static_cast<const T *>(x);
    hipStream_t s = nullptr;
    // K16's first pass, on the rows in their original order so that a refusal names the caller's row; under cosine the unit rows
    if (int rc = pilot::knn_checked_rows(&X, &ld, n, D, metric, pilot::WS_SIL_FLAGS, pilot::WS_SIL_UNIT)) return rc;
    T *S;
    int *d_order, *d_offsets;
    double *out;
    HIP_TRY(pilot::ws(pilot::WS_SIL_SORTED, (size_t)n * D, &S));
    HIP_TRY(pilot::ws(pilot::WS_SIL_ORDER, (size_t)n, &d_order));
    HIP_TRY(pilot::ws(pilot::WS_SIL_OFFSETS, (size_t)n_clusters + 1, &d_offsets));
    HIP_TRY(pilot::ws(pilot::WS_SIL_OUT, (size_t)n, &out));
    HIP_TRY(hipMemcpy(d_order, order, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_offsets, offsets, sizeof(int) * ((size_t)n_clusters + 1), hipMemcpyHostToDevice));
    const long long elems = (long long)n * D;
    hipLaunchKernelGGL(pilot::silhouette_gather_kernel<T>, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, s, X, ld, (long long)n, D,
                       d_order, S);
    const long long blocks = ((long long)n + pilot::KNN_THREADS - 1) / pilot::KNN_THREADS;
    for (long long b0 = 0; b0 < blocks; b0 += pilot::KNN_GRID_MAX) {
        const unsigned grid = (unsigned)std::min<long long>(pilot::KNN_GRID_MAX, blocks - b0);
        const int q0 = (int)(b0 * pilot::KNN_THREADS);
        if (D <= pilot::KNN_REGQ_D)
            hipLaunchKernelGGL((pilot::silhouette_rows_kernel<T, true>), dim3(grid), dim3(pilot::KNN_THREADS), 0, s, S, n, D, metric, d_offsets,
                               d_order, q0, out);
        else
            hipLaunchKernelGGL((pilot::silhouette_rows_kernel<T, false>), dim3(grid), dim3(pilot::KNN_THREADS), 0, s, S, n, D, metric, d_offsets,
                               d_order, q0, out);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(samples, out, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}

}  // namespace

PILOT_API int pilot_ot_silhouette_points(const void *X, int X_is_device, int dtype, long long n, int D, long long ld, int metric,
                                         const int *codes, int n_clusters, double *samples, double *score) {
    if (!X || !codes || !samples || !score) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (D < 1) return fail(PILOT_OT_EINVAL, "D=%d columns", D);
    if (int rc = pilot::check_ld(ld, D)) return rc;
    if (int rc = pilot::check_dtype(dtype)) return rc;
    if (metric != 0 && metric != 1) return fail(PILOT_OT_EINVAL, "metric=%d must be 0 (euclidean) or 1 (cosine)", metric);
    if (n > INT_MAX) return fail(PILOT_OT_ENOTSUP, "n=%lld rows need more than 32-bit row indices", n);
    if (n_clusters < 2 || (long long)n_clusters > n - 1)
        return fail(PILOT_OT_EINVAL, "n_clusters=%d: valid values are 2 to n - 1 = %lld (inclusive)", n_clusters, n - 1);

    // the rows ordered by (code, row): a counting sort, stable in the row
    std::vector<int> offsets((size_t)n_clusters + 1, 0), order((size_t)n);
    for (long long i = 0; i < n; ++i) {
        if (codes[i] < 0 || codes[i] >= n_clusters)
            return fail(PILOT_OT_EINVAL, "codes[%lld]=%d outside [0, %d)", i, codes[i], n_clusters);
        ++offsets[(size_t)codes[i] + 1];
    }
    for (int c = 0; c < n_clusters; ++c) {
        if (offsets[(size_t)c + 1] == 0) return fail(PILOT_OT_EINVAL, "code %d has no rows", c);
        offsets[(size_t)c + 1] += offsets[c];
    }
    {
        std::vector<int> next(offsets.begin(), offsets.end() - 1);
        for (long long i = 0; i < n; ++i) order[(size_t)next[codes[i]]++] = (int)i;
    }

    const void *x;
    long long x_ld;
    if (int rc = pilot::stage_dense(X, X_is_device, pilot::elem_size(dtype), n, D, ld, pilot::WS_SIL_X, &x, &x_ld)) return rc;
    const int rc = dtype == 0 ? silhouette_points<float>(x, x_ld, (int)n, D, metric, order.data(), offsets.data(), n_clusters, samples)
                              : silhouette_points<double>(x, x_ld, (int)n, D, metric, order.data(), offsets.data(), n_clusters, samples);
    if (rc) return rc;
    double total = 0.0;
    for (long long i = 0; i < n; ++i) total += samples[i];
    *score = total / (double)n;
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_silhouette_points_geometry(int D, int dtype, int *queries_per_block, int *tile_rows) {
    if (!queries_per_block || !tile_rows) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (D < 1) return fail(PILOT_OT_EINVAL, "D=%d columns", D);
    if (int rc = pilot::check_dtype(dtype)) return rc;
    *queries_per_block = pilot::KNN_THREADS;
    *tile_rows = pilot::KNN_PB * (dtype == 0 ? pilot::KnnTile<float>(D).ns : pilot::KnnTile<double>(D).ns);
    return PILOT_OT_OK;
}
