// C ABI of the gene curve clustering step (include/pilot_ot.h, section "gene curve clustering"; kernels: curve_kernels.hpp).
// Every matrix argument is a host array or (its *_is_device flag) a dense row-major buffer in HBM; small vectors (times,
// parameters, offsets) are host arrays.  The G x G distance matrix lives in an allocation of its own for the length of one
// linkage call and never reaches the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "abi_common.hpp"
#include "curve_kernels.hpp"

namespace {

int check_times(const double *times, int T) {
    if (T < 2) return fail(PILOT_OT_EINVAL, "times must be increasing and have at least 2 values (got %d)", T);
    for (int t = 0; t < T; ++t)
        if (!std::isfinite(times[t])) return fail(PILOT_OT_EINVAL, "times[%d]=%g is not finite", t, times[t]);
    for (int t = 1; t < T; ++t)
        if (!(times[t] > times[t - 1])) return fail(PILOT_OT_EINVAL, "times must be increasing and have at least 2 values (times[%d]=%g after %g)", t, times[t], times[t - 1]);
    return PILOT_OT_OK;
}

}  // namespace

PILOT_API int pilot_ot_segment_std(const void *Y, int Y_is_device, int dtype, long long n, int n_cols, long long ld,
                                   const long long *offsets, int n_segments, const int *cols, int n_sel, double *out,
                                   int out_is_device) {
    if (!Y || !offsets || !out) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (n < 0 || n_cols < 1) return fail(PILOT_OT_EINVAL, "n=%lld, n_cols=%d", n, n_cols);
    if (int rc = pilot::check_ld(ld, n_cols)) return rc;
    if (int rc = pilot::check_dtype(dtype)) return rc;
    if (n_segments < 0 || n_segments > 65535) return fail(PILOT_OT_EINVAL, "n_segments=%d must be in [0, 65535]", n_segments);
    if (offsets[0] < 0 || offsets[n_segments] > n) return fail(PILOT_OT_EINVAL, "offsets must lie in [0, n=%lld]", n);
    for (int s = 0; s < n_segments; ++s)
        if (offsets[s + 1] < offsets[s]) return fail(PILOT_OT_EINVAL, "offsets[%d]=%lld after %lld: must not decrease", s + 1, offsets[s + 1], offsets[s]);
    if (int rc = pilot::check_cols(cols, n_sel, n_cols)) return rc;
    if (n_segments == 0 || n_sel == 0) return PILOT_OT_OK;
    const size_t es = pilot::elem_size(dtype);
    std::vector<long long> off(offsets, offsets + n_segments + 1);
    const long long r0 = Y_is_device ? 0 : offsets[0];           // a host Y: only the rows the segments cover go up
    for (long long &o : off) o -= r0;
    const void *yd;
    long long ldd;
    if (int rc = pilot::stage_dense(static_cast<const unsigned char *>(Y) + (size_t)r0 * ld * es, Y_is_device, es, offsets[n_segments] - r0,
                                    n_cols, ld, pilot::WS_CV_Y, &yd, &ldd))
        return rc;
    long long *d_off;
    int *d_cols = nullptr;
    HIP_TRY(pilot::ws(pilot::WS_CV_AUX, (size_t)n_segments + 1 + (size_t)(n_sel + 1) / 2, &d_off));
    HIP_TRY(hipMemcpy(d_off, off.data(), sizeof(long long) * ((size_t)n_segments + 1), hipMemcpyHostToDevice));
    if (cols) {
        d_cols = reinterpret_cast<int *>(d_off + n_segments + 1);
        HIP_TRY(hipMemcpy(d_cols, cols, sizeof(int) * (size_t)n_sel, hipMemcpyHostToDevice));
    }
    double *d_out = out;
    if (!out_is_device) HIP_TRY(pilot::ws(pilot::WS_CV_OUT, (size_t)n_segments * n_sel, &d_out));
    const dim3 grid((unsigned)((n_sel + 63) / 64), (unsigned)n_segments);
    if (dtype == 0)
        hipLaunchKernelGGL(pilot::segment_std_kernel<float>, grid, dim3(pilot::CV_STD_BLOCK), 0, nullptr, static_cast<const float *>(yd),
                           ldd, d_off, d_cols, n_sel, d_out);
    else
        hipLaunchKernelGGL(pilot::segment_std_kernel<double>, grid, dim3(pilot::CV_STD_BLOCK), 0, nullptr, static_cast<const double *>(yd),
                           ldd, d_off, d_cols, n_sel, d_out);
    HIP_TRY(hipGetLastError());
    if (!out_is_device) HIP_TRY(hipMemcpy(out, d_out, sizeof(double) * (size_t)n_segments * n_sel, hipMemcpyDeviceToHost));
    else HIP_TRY(hipStreamSynchronize(nullptr));
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_fitted_curves(const double *params, const int *models, int G, const double *times, int T, const double *sd,
                                     int sd_is_device, double *out, int out_is_device) {
    if (!params || !models || !times || !out) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (G < 0 || T < 1) return fail(PILOT_OT_EINVAL, "G=%d, T=%d", G, T);
    for (int g = 0; g < G; ++g)
        if (models[g] < 0 || models[g] > 2) return fail(PILOT_OT_EINVAL, "models[%d]=%d must be 0, 1 or 2", g, models[g]);
    for (size_t j = 0; j < (size_t)G * 3; ++j)
        if (!std::isfinite(params[j])) return fail(PILOT_OT_EINVAL, "params[%zu]=%g is not finite", j, params[j]);
    for (int t = 0; t < T; ++t)
        if (!std::isfinite(times[t])) return fail(PILOT_OT_EINVAL, "times[%d]=%g is not finite", t, times[t]);
    if (G == 0) return PILOT_OT_OK;
    double *d_in;
    HIP_TRY(pilot::ws(pilot::WS_CV_IN, (size_t)G * 3 + T + (size_t)(G + 1) / 2, &d_in));
    double *d_times = d_in + (size_t)G * 3;
    int *d_models = reinterpret_cast<int *>(d_times + T);
    HIP_TRY(hipMemcpy(d_in, params, sizeof(double) * (size_t)G * 3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_times, times, sizeof(double) * (size_t)T, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_models, models, sizeof(int) * (size_t)G, hipMemcpyHostToDevice));
    const double *d_sd = nullptr;
    if (sd) {
        int rc = pilot::stage_f64(sd, sd_is_device, (size_t)T * G, pilot::WS_CV_Y, &d_sd);
        if (rc != PILOT_OT_OK) return rc;
    }
    double *d_out = out;
    if (!out_is_device) HIP_TRY(pilot::ws(pilot::WS_CV_OUT, (size_t)G * T, &d_out));
    hipLaunchKernelGGL(pilot::fitted_curves_kernel, dim3((unsigned)G), dim3(64), 0, nullptr, d_in, d_models, d_times, G, T, d_sd, d_out);
    HIP_TRY(hipGetLastError());
    if (!out_is_device) HIP_TRY(hipMemcpy(out, d_out, sizeof(double) * (size_t)G * T, hipMemcpyDeviceToHost));
    else HIP_TRY(hipStreamSynchronize(nullptr));
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_linkage_of_rows(const double *Y, int Y_is_device, int G, int T, int method, double *Z, double *dmax,
                                       int *chain_steps) {
    if (!Y || !Z) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (G < 2) return fail(PILOT_OT_EINVAL, "G=%d: a linkage needs at least 2 rows", G);
    if (T < 1) return fail(PILOT_OT_EINVAL, "T=%d must be positive", T);
    if (method < pilot::CV_LINK_SINGLE || method > pilot::CV_LINK_WEIGHTED)
        return fail(PILOT_OT_ENOTSUP, "linkage method %d: single (0), complete (1), average (2) and weighted (3) are implemented", method);
    if (G > PILOT_OT_LINKAGE_MAX_G)
        return fail(PILOT_OT_EINVAL, "G=%d rows: the G x G float64 distance matrix is held in HBM, at most %d rows (8 GiB)", G,
                    PILOT_OT_LINKAGE_MAX_G);
    if (!Y_is_device)
        for (size_t j = 0; j < (size_t)G * T; ++j)
            if (!std::isfinite(Y[j])) return fail(PILOT_OT_EINVAL, "Y[%zu]=%g is not finite", j, Y[j]);
    const double *d_y;
    int rc = pilot::stage_f64(Y, Y_is_device, (size_t)G * T, pilot::WS_CV_Y, &d_y);
    if (rc != PILOT_OT_OK) return rc;
    const unsigned nb = (unsigned)((G + pilot::CV_D_TILE - 1) / pilot::CV_D_TILE);
    double *d_bmax, *d_z;
    int *d_chain;
    HIP_TRY(pilot::ws(pilot::WS_CV_BMAX, (size_t)nb * nb, &d_bmax));
    HIP_TRY(pilot::ws(pilot::WS_CV_CHAIN, 2 * (size_t)G + 4, &d_chain));      // chain (G + 1), size (G), info (2)
    HIP_TRY(pilot::ws(pilot::WS_CV_Z, 4 * (size_t)(G - 1), &d_z));
    int *d_size = d_chain + G + 1, *d_info = d_size + G;
    struct Matrix {                                               // the distance matrix: this call's own allocation
        double *p = nullptr;
        ~Matrix() { if (p) (void)hipFree(p); }
    } D;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&D.p), sizeof(double) * (size_t)G * G));
    hipLaunchKernelGGL(pilot::curve_distance_kernel, dim3(nb, nb), dim3(256), 0, nullptr, d_y, G, T, D.p, d_bmax);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pilot::nn_chain_kernel, dim3(1), dim3(pilot::CV_NN_BLOCK), 0, nullptr, D.p, G, method, d_chain, d_size, d_z, d_info);
    HIP_TRY(hipGetLastError());
    std::vector<double> bmax((size_t)nb * nb), raw(4 * (size_t)(G - 1));
    int info[2] = {0, 0};
    HIP_TRY(hipMemcpy(info, d_info, sizeof(info), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(bmax.data(), d_bmax, sizeof(double) * bmax.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(raw.data(), d_z, sizeof(double) * raw.size(), hipMemcpyDeviceToHost));
    if (chain_steps) *chain_steps = info[1];
    if (info[0] == 1) return fail(PILOT_OT_EHIP, "linkage: the nearest-neighbour chain reached its cap of %lld steps for G=%d", 4LL * G, G);
    if (info[0] != 0) return fail(PILOT_OT_EINVAL, "linkage: a row has no finite distance to any other (NaN or inf in Y)");
    if (dmax) *dmax = *std::max_element(bmax.begin(), bmax.end());

    // scipy's finish: a stable sort by height, then labels by union-find -- roots in ascending order, new ids G + i, sizes
    std::vector<int> order(G - 1);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return raw[4 * (size_t)a + 2] < raw[4 * (size_t)b + 2]; });
    std::vector<int> parent(2 * (size_t)G - 1), size(2 * (size_t)G - 1, 1);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int x) {
        int r = x;
        while (parent[r] != r) r = parent[r];
        while (parent[x] != r) { const int nx = parent[x]; parent[x] = r; x = nx; }
        return r;
    };
    for (int i = 0; i < G - 1; ++i) {
        const double *r = raw.data() + 4 * (size_t)order[i];
        const int a = find((int)r[0]), b = find((int)r[1]), id = G + i;
        parent[a] = parent[b] = id;
        size[id] = size[a] + size[b];
        double *z = Z + 4 * (size_t)i;
        z[0] = std::min(a, b); z[1] = std::max(a, b); z[2] = r[2]; z[3] = size[id];
    }
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_curve_activities(const double *curves, int curves_is_device, int G, int T, const double *times, double *out) {
    if (!curves || !times || !out) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (G < 0) return fail(PILOT_OT_EINVAL, "G=%d is negative", G);
    int rc = check_times(times, T);
    if (rc != PILOT_OT_OK) return rc;
    if (G == 0) return PILOT_OT_OK;
    const double *d_c;
    rc = pilot::stage_f64(curves, curves_is_device, (size_t)G * T, pilot::WS_CV_Y, &d_c);
    if (rc != PILOT_OT_OK) return rc;
    double *d_times, *d_out;
    HIP_TRY(pilot::ws(pilot::WS_CV_IN, (size_t)T, &d_times));
    HIP_TRY(pilot::ws(pilot::WS_CV_OUT, (size_t)G * 4, &d_out));
    HIP_TRY(hipMemcpy(d_times, times, sizeof(double) * (size_t)T, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(pilot::curve_activities_kernel, dim3((unsigned)G), dim3(64), 0, nullptr, d_c, d_times, G, T, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out, sizeof(double) * (size_t)G * 4, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}
