// C ABI of the batched bootstrap Huber fits (include/pilot_ot.h, section "bootstrap Huber fits"; kernel: bootfit_kernels.hpp).
// The host maps the base times once (trajfit_host.hpp: K9's scaled basis, back-transform and penalty; no Gram: each resample forms
// its own in the kernel), copies Y once and streams the index vectors through the device in bounded chunks of problems.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "abi_common.hpp"
#include "bootfit_kernels.hpp"
#include "trajfit_host.hpp"

namespace {

constexpr size_t CHUNK_BYTES = size_t(256) << 20;      // index vectors on the device: at most this many bytes at a time

int check_args(const void *Y, int dtype, int n, int n_cols, long long ld, const double *x, int n_problems, const int *cols,
               const int *models, int B, const int *idx, double epsilon, const double *params) {
    if (!Y || !x || !params || (n_problems > 0 && (!cols || !models || !idx))) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (n < 1) return fail(PILOT_OT_EINVAL, "n=%d: the fits need at least 1 observation", n);
    if (n_cols < 1) return fail(PILOT_OT_EINVAL, "n_cols=%d must be positive", n_cols);
    if (int rc = pilot::check_ld(ld, n_cols)) return rc;
    if (int rc = pilot::check_dtype(dtype)) return rc;
    if (n_problems < 0) return fail(PILOT_OT_EINVAL, "n_problems=%d is negative", n_problems);
    if (B < 1 || B > 64 * 65535) return fail(PILOT_OT_EINVAL, "B=%d must be in [1, %d]", B, 64 * 65535);
    if (!(epsilon >= 1.0) || !std::isfinite(epsilon)) return fail(PILOT_OT_EINVAL, "epsilon=%g must be finite and >= 1", epsilon);
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(x[i])) return fail(PILOT_OT_EINVAL, "x[%d]=%g is not finite", i, x[i]);
    if (n_problems > 0)                                          // (one column per problem; none given: nothing to judge)
        if (int rc = pilot::check_cols(cols, n_problems, n_cols)) return rc;
    for (int q = 0; q < n_problems; ++q)
        if (models[q] < 0 || models[q] > 2) return fail(PILOT_OT_EINVAL, "models[%d]=%d must be 0, 1 or 2", q, models[q]);
    const size_t total = (size_t)n_problems * n * B;
    for (size_t j = 0; j < total; ++j)
        if ((unsigned)idx[j] >= (unsigned)n)
            return fail(PILOT_OT_EINVAL, "idx[%zu]=%d outside [0, %d) (problem %zu, observation %zu, bootstrap %zu)", j, idx[j], n,
                        j / ((size_t)n * B), j / B % n, j % B);
    return PILOT_OT_OK;
}

}  // namespace

PILOT_API int pilot_ot_bootstrap_huber_fits(const void *Y, int Y_is_device, int dtype, int n, int n_cols, long long ld, const double *x,
                                            int n_problems, const int *cols, const int *models, int B, const int *idx, double epsilon,
                                            double *params, double *sigma, int *steps, int *flags, int *n_not_converged) {
    int rc = check_args(Y, dtype, n, n_cols, ld, x, n_problems, cols, models, B, idx, epsilon, params);
    if (rc != PILOT_OT_OK) return rc;
    if (n_not_converged) *n_not_converged = 0;
    if (n_problems == 0) return PILOT_OT_OK;
    pilot::TrajfitArgs a;
    std::vector<double> u;
    pilot::trajfit_time_map(x, n, u, a);
    a.huber = 1;
    a.epsilon = epsilon;
    a.max_iter = pilot::trajfit_max_iter();
    const size_t per_problem = (size_t)n * B * sizeof(int);
    long long pc = (long long)std::max<size_t>(1, CHUNK_BYTES / per_problem);
    if (const char *sw = pilot::test_switch("PILOT_OT_BOOTFIT_CHUNK_PROBLEMS")) {  // (tests: many chunks)
        const long long v = atoll(sw);
        if (v > 0) pc = v;
    }
    pc = std::min<long long>(pc, n_problems);

    const double *d_u;
    const pilot::TrajfitArgs *d_args;
    double *d_out;
    int *d_idx, *d_pm;
    rc = pilot::trajfit_stage(pilot::WS_BOOT_U, u, a, &d_u, &d_args);
    if (rc != PILOT_OT_OK) return rc;
    HIP_TRY(pilot::ws(pilot::WS_BOOT_OUT, (size_t)pc * B * pilot::BF_NOUT, &d_out));
    HIP_TRY(pilot::ws(pilot::WS_BOOT_IDX, (size_t)pc * n * B + 2 * (size_t)n_problems, &d_idx));    // the chunk's indices, then cols and models
    d_pm = d_idx + (size_t)pc * n * B;
    HIP_TRY(hipMemcpy(d_pm, cols, sizeof(int) * n_problems, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_pm + n_problems, models, sizeof(int) * n_problems, hipMemcpyHostToDevice));
    const void *yd;                                              // a host Y is copied whole (its n x n_cols part)
    long long ldd;
    rc = pilot::stage_dense(Y, Y_is_device, pilot::elem_size(dtype), n, n_cols, ld, pilot::WS_BOOT_Y, &yd, &ldd);
    if (rc != PILOT_OT_OK) return rc;
    std::vector<double> rec((size_t)pc * B * pilot::BF_NOUT);
    int not_conv = 0;
    for (long long q0 = 0; q0 < n_problems; q0 += pc) {
        const int nq = (int)std::min<long long>(pc, n_problems - q0);
        HIP_TRY(hipMemcpy(d_idx, idx + (size_t)q0 * n * B, (size_t)nq * per_problem, hipMemcpyHostToDevice));
        const dim3 grid((unsigned)nq, (unsigned)((B + 63) / 64));
        if (dtype == 0)
            hipLaunchKernelGGL(pilot::bootfit_kernel<float>, grid, dim3(pilot::TF_BLOCK), 0, nullptr, static_cast<const float *>(yd), ldd,
                               d_u, d_idx, d_pm + q0, d_pm + n_problems + q0, B, d_args, d_out);
        else
            hipLaunchKernelGGL(pilot::bootfit_kernel<double>, grid, dim3(pilot::TF_BLOCK), 0, nullptr, static_cast<const double *>(yd),
                               ldd, d_u, d_idx, d_pm + q0, d_pm + n_problems + q0, B, d_args, d_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(rec.data(), d_out, sizeof(double) * (size_t)nq * B * pilot::BF_NOUT, hipMemcpyDeviceToHost));
        for (size_t j = 0; j < (size_t)nq * B; ++j) {
            const double *r = rec.data() + j * pilot::BF_NOUT;
            const size_t f = (size_t)q0 * B + j;
            for (int c = 0; c < 3; ++c) params[f * 3 + c] = r[pilot::BF_O_PARAMS + c];
            if (sigma) sigma[f] = r[pilot::BF_O_SIGMA];
            if (steps) steps[f] = (int)r[pilot::BF_O_STEPS];
            if (flags) flags[f] = (int)r[pilot::BF_O_FLAGS];
            not_conv += ((int)r[pilot::BF_O_FLAGS] & PILOT_OT_TRAJFIT_NOT_CONVERGED) != 0;
        }
    }
    if (n_not_converged) *n_not_converged = not_conv;
    return PILOT_OT_OK;
}
