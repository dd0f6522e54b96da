// C ABI of the per-group moments (include/pilot_ot.h, section "group moments"; kernels: moments_kernels.hpp).  Y is a host array
// (copied whole, packed) or a row-major buffer in HBM with its own leading dimension; codes, cols and the results are host arrays.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "abi_common.hpp"
#include "moments_kernels.hpp"

namespace {

struct MomentsArgs {
    const void *y;
    long long ld, n;
    const int *codes, *cols;
    int n_sel, vec, n_slices;
    long long *pcount;
    double *pmean, *pm2;
};

template <typename T, int NG> void launch_ng(const MomentsArgs &a, int transform) {
    const dim3 grid((unsigned)((a.n_sel + pilot::GM_TILE - 1) / pilot::GM_TILE), (unsigned)a.n_slices);
    if (transform)
        hipLaunchKernelGGL((pilot::group_moments_kernel<T, NG, true>), grid, dim3(64), 0, nullptr, static_cast<const T *>(a.y), a.ld, a.n,
                           a.codes, a.cols, a.n_sel, a.vec, a.pcount, a.pmean, a.pm2);
    else
        hipLaunchKernelGGL((pilot::group_moments_kernel<T, NG, false>), grid, dim3(64), 0, nullptr, static_cast<const T *>(a.y), a.ld, a.n,
                           a.codes, a.cols, a.n_sel, a.vec, a.pcount, a.pmean, a.pm2);
}

template <typename T> void launch(const MomentsArgs &a, int ng, int transform) {
    switch (ng) {
        case 1: launch_ng<T, 1>(a, transform); break;
        case 2: launch_ng<T, 2>(a, transform); break;
        case 4: launch_ng<T, 4>(a, transform); break;
        default: launch_ng<T, 8>(a, transform); break;
    }
}

}  // namespace

PILOT_API int pilot_ot_group_moments(const void *Y, int Y_is_device, int dtype, long long n, int n_cols_total, long long ld,
                                     const int *codes, int n_groups, const int *cols, int n_cols, int transform, long long *count,
                                     double *mean, double *m2) {
    if (!Y || !count || !mean || !m2 || (!codes && n > 0)) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (n < 0 || n_cols_total < 1) return fail(PILOT_OT_EINVAL, "n=%lld, n_cols_total=%d", n, n_cols_total);
    if (int rc = pilot::check_ld(ld, n_cols_total)) return rc;
    if (int rc = pilot::check_dtype(dtype)) return rc;
    if (n_groups < 1 || n_groups > pilot::GM_MAX_GROUPS) return fail(PILOT_OT_EINVAL, "n_groups=%d must be in [1, %d]", n_groups, pilot::GM_MAX_GROUPS);
    if (transform != 0 && transform != 1) return fail(PILOT_OT_EINVAL, "transform=%d must be 0 (none) or 1 (expm1)", transform);
    if (int rc = pilot::check_cols(cols, n_cols, n_cols_total)) return rc;
    for (long long i = 0; i < n; ++i)
        if (codes[i] >= n_groups) return fail(PILOT_OT_EINVAL, "codes[%lld]=%d: a code is negative (row skipped) or below n_groups=%d", i, codes[i], n_groups);
    if (n_cols == 0) {
        for (int g = 0; g < n_groups; ++g) count[g] = 0;
        for (long long i = 0; i < n; ++i)
            if (codes[i] >= 0) ++count[codes[i]];
        return PILOT_OT_OK;
    }
    const size_t es = pilot::elem_size(dtype);
    MomentsArgs a;
    a.n = n;
    a.n_sel = n_cols;
    if (int rc = pilot::stage_dense(Y, Y_is_device, es, n, n_cols_total, ld, pilot::WS_GM_Y, &a.y, &a.ld)) return rc;
    // 16-byte row reads: every row start and every lane's first column on a 16-byte boundary
    const long long per16 = (long long)(16 / es);
    a.vec = !cols && a.ld % per16 == 0 && reinterpret_cast<uintptr_t>(a.y) % 16 == 0;
    int *d_codes;
    HIP_TRY(pilot::ws(pilot::WS_GM_AUX, (size_t)n + (size_t)n_cols, &d_codes));
    if (n > 0) HIP_TRY(hipMemcpy(d_codes, codes, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    int *d_cols = nullptr;
    if (cols) {
        d_cols = d_codes + n;
        HIP_TRY(hipMemcpy(d_cols, cols, sizeof(int) * (size_t)n_cols, hipMemcpyHostToDevice));
    }
    a.codes = d_codes;
    a.cols = d_cols;
    // slices: about 8 one-wave workgroups per CU over the whole grid, each of at least GM_MIN_SLICE_ROWS rows (n below that: one)
    const int tiles = (n_cols + pilot::GM_TILE - 1) / pilot::GM_TILE;
    const long long by_rows = n / pilot::GM_MIN_SLICE_ROWS;
    const long long by_cus = ((long long)pilot::cu_count() * 8 + tiles - 1) / tiles;
    a.n_slices = (int)std::max<long long>(1, std::min<long long>({by_rows, by_cus, 65535}));
    const int ng = n_groups <= 1 ? 1 : n_groups <= 2 ? 2 : n_groups <= 4 ? 4 : 8;
    const size_t per_slice = (size_t)ng * n_cols;
    double *d_part, *d_out;
    long long *d_pcount;
    HIP_TRY(pilot::ws(pilot::WS_GM_PART, 2 * per_slice * a.n_slices, &d_part));
    HIP_TRY(pilot::ws(pilot::WS_GM_COUNT, (size_t)ng * a.n_slices + n_groups, &d_pcount));
    HIP_TRY(pilot::ws(pilot::WS_GM_OUT, 2 * (size_t)n_groups * n_cols, &d_out));
    a.pcount = d_pcount;
    a.pmean = d_part;
    a.pm2 = d_part + per_slice * a.n_slices;
    if (dtype == 0) launch<float>(a, ng, transform);
    else launch<double>(a, ng, transform);
    HIP_TRY(hipGetLastError());
    long long *d_count = d_pcount + (size_t)ng * a.n_slices;
    const size_t n_out = (size_t)n_groups * n_cols;
    hipLaunchKernelGGL(pilot::group_moments_join_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, nullptr, a.pcount, a.pmean,
                       a.pm2, a.n_slices, ng, n_groups, n_cols, d_count, d_out, d_out + n_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(count, d_count, sizeof(long long) * (size_t)n_groups, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mean, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(m2, d_out + n_out, sizeof(double) * n_out, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}
