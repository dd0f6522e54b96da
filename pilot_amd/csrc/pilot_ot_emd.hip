// Exact OT over the pair grid (C ABI: pilot_ot_emd_grid*, pilot_ot_mirror_upper_dev; include/pilot_ot.h).  Kernels:
// emd_kernels.hpp (one pair per wave), emd_multi_kernels.hpp (K <= 16), emd_generic_kernel.hpp (K > 256).
#include <hip/hip_runtime.h>

#include "abi_common.hpp"
#include "grid_plan.hpp"
#include "emd_kernels.hpp"
#include "emd_multi_kernels.hpp"
#include "emd_generic_kernel.hpp"

using pilot::LDS_BYTES, pilot::EMD_MAX_K, pilot::EMD_MULTI_MAX_K, pilot::emd_nk, pilot::emd_wgs_per_cu, pilot::emd_multi_mode;

size_t pilot::emd_counter_bytes() { return sizeof(int) * pilot::EMD_NQ * pilot::EMD_Q_STRIDE; }

PILOT_API int pilot_ot_emd_grid_dev(pilot_ot_plan *pl, const double *d_P, const double *d_M, int mode, int row_begin,
                                    int row_end, int row_step, double *d_emd, int *d_n_aug, void *stream) {
    if (!pl || !d_P || !d_M || !d_emd) return fail(PILOT_OT_EINVAL, "NULL pointer");
    const int N = pl->N, K = pl->K;
    if (mode < PILOT_OT_EMD_ALL || mode > PILOT_OT_EMD_MIRROR) return fail(PILOT_OT_EINVAL, "unknown mode %d", mode);
    if (row_step < 1 || row_begin < 0 || row_end > N || row_begin > row_end)
        return fail(PILOT_OT_EINVAL, "bad row range [%d, %d) step %d for N=%d", row_begin, row_end, row_step, N);
    if (mode == PILOT_OT_EMD_MIRROR && !(row_begin == 0 && row_end == N && row_step == 1))
        return fail(PILOT_OT_EINVAL, "PILOT_OT_EMD_MIRROR needs the full square grid");
    const int n_rows = (row_end - row_begin + row_step - 1) / row_step;
    if (n_rows == 0) return PILOT_OT_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    pilot::EmdParams p;
    p.P = d_P; p.M = d_M; p.N = N; p.K = K;
    p.n_rows = n_rows; p.row_begin = row_begin; p.row_step = row_step;
    p.upper_only = mode != PILOT_OT_EMD_ALL;
    p.emd = d_emd; p.n_aug = d_n_aug; p.f_slab = nullptr; p.queue = pl->emd_counter;
    // the flow slab of the wave-per-pair kernels: allocated ONCE, by the plan's first exact call that needs it, at the largest
    // size any kernel variant of this K asks for (several pairs per wave with the flows in the slab; one pair per wave) -- never
    // freed or regrown by a later call (a call made under stream capture after the first one allocates nothing)
    auto need_slab = [&](size_t bytes) -> int {
        if (!pl->f_slab) {
            size_t most = bytes;
            if (K <= EMD_MAX_K) {
                const size_t one = sizeof(double) * (size_t)K * K * emd_wgs_per_cu(K) * pl->n_cu * pilot::emd_waves(emd_nk(K));
                most = one > most ? one : most;
            }
            if (K <= EMD_MULTI_MAX_K) {
                const pilot::EmdMultiGeom g = pilot::emd_multi_geom(K, false);
                const size_t multi = sizeof(double) * (size_t)K * K * 4 * g.waves * g.wgs_per_cu * pl->n_cu;
                most = multi > most ? multi : most;
            }
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&pl->f_slab), most));
            pl->f_slab_bytes = most;
        }
        if (pl->f_slab_bytes < bytes) return fail(PILOT_OT_EHIP, "exact OT: the plan's flow slab (%zu bytes) is smaller than this call needs (%zu)", pl->f_slab_bytes, bytes);
        p.f_slab = pl->f_slab;
        return PILOT_OT_OK;
    };
    HIP_TRY(hipMemsetAsync(pl->emd_counter, 0, sizeof(int) * pilot::EMD_NQ * pilot::EMD_Q_STRIDE, s));
    const long total = (long)n_rows * N;
    if (K > EMD_MAX_K) {
        // beyond the one-wave-per-pair kernel: one workgroup per pair, vectors in LDS, flows in a global slab per resident
        // workgroup (emd_generic_kernel.hpp) -- the reference has no limit on the number of cell types
        if (K > pilot::EMDG_MAX_K) return fail(PILOT_OT_ENOTSUP, "exact OT: K=%d > %d cell types", K, pilot::EMDG_MAX_K);
        const size_t per_wg = sizeof(double) * pilot::emdg_slab_doubles(K);
        const long n_items = p.upper_only ? (long)n_rows * (N - row_begin) - (long)row_step * n_rows * (n_rows - 1) / 2 : total;
        long wgs = 2L * pl->n_cu;
        while (wgs > 1 && per_wg * (size_t)wgs > ((size_t)8 << 30)) wgs /= 2;
        if (!pl->emdg_slab || pl->emdg_wgs < wgs) {          // (first call that needs this kernel: the one allocation of the path)
            if (pl->emdg_slab) HIP_TRY(hipFree(pl->emdg_slab));
            pl->emdg_slab = nullptr;
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&pl->emdg_slab), per_wg * (size_t)wgs + sizeof(double) * (size_t)K));
            pl->emdg_wgs = (int)wgs;
        }
        if (wgs > n_items) wgs = n_items > 0 ? n_items : 1;
        double *rowmin = pl->emdg_slab + pilot::emdg_slab_doubles(K) * (size_t)pl->emdg_wgs;
        hipLaunchKernelGGL(pilot::emd_rowmin_kernel, dim3((K + 255) / 256), dim3(256), 0, s, d_M, K, rowmin);
        p.f_slab = pl->emdg_slab;
        const size_t lds = pilot::emdg_lds_bytes(K);
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pilot::emd_generic_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(pilot::emd_generic_kernel, dim3((unsigned)wgs), dim3(pilot::EMDG_WG), lds, s, p, rowmin);
    } else if (K <= EMD_MULTI_MAX_K && emd_multi_mode(K) != 0) {
        // four pairs per wavefront
        const pilot::EmdMultiGeom m = pilot::emd_multi_geom(K, emd_multi_mode(K) != 2);
        if (!m.flds) {      // (flow values in the global slab: a K x K block per 16-lane group of every resident wave)
            const int rc = need_slab(sizeof(double) * (size_t)K * K * 4 * m.waves * m.wgs_per_cu * pl->n_cu);
            if (rc != PILOT_OT_OK) return rc;
        }
        const long groups = (total + (64 / m.G) - 1) / (64 / m.G);
        long wgs = (groups + m.waves - 1) / m.waves;
        const long cap = (long)pl->n_cu * m.wgs_per_cu;
        if (wgs > cap) wgs = cap;
        auto kern = m.flds ? pilot::emd_multi_kernel<16, true> : pilot::emd_multi_kernel<16, false>;
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)m.lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(64 * m.waves), m.lds, s, p);
    } else {
        {
            const int rc = need_slab(sizeof(double) * (size_t)K * K * emd_wgs_per_cu(K) * pl->n_cu * pilot::emd_waves(emd_nk(K)));
            if (rc != PILOT_OT_OK) return rc;
        }
        const size_t lds = pilot::emd_lds_bytes(K);
        if (lds > LDS_BYTES) return fail(PILOT_OT_ENOTSUP, "K=%d does not fit the LDS layout", K);
        const int waves = pilot::emd_waves(emd_nk(K));
        long wgs = (total + waves - 1) / waves;
        const long cap = (long)pl->n_cu * emd_wgs_per_cu(K);
        if (wgs > cap) wgs = cap;
        constexpr bool UL = pilot::emd_ul(128);      // (labels without the column potential: always beyond 64 cell types)
        if (K > 192) {
            hipLaunchKernelGGL((pilot::emd_grid_kernel<4, true, UL>), dim3((unsigned)wgs), dim3(64 * waves), lds, s, p);
        } else if (K > 128) {
            hipLaunchKernelGGL((pilot::emd_grid_kernel<3, true, UL>), dim3((unsigned)wgs), dim3(64 * waves), lds, s, p);
        } else if (K <= 64) {
            auto kern = pilot::emd_ul(K) ? pilot::emd_grid_kernel<1, false, true> : pilot::emd_grid_kernel<1, false, false>;
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(64 * waves), lds, s, p);
        } else {
            auto kern = pilot::emd_grid_kernel<2, false, UL>;
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(64 * waves), lds, s, p);
        }
    }
    HIP_TRY(hipGetLastError());
    if (mode == PILOT_OT_EMD_MIRROR) {
        hipLaunchKernelGGL(pilot::emd_mirror_kernel, dim3(1024), dim3(256), 0, s, d_emd, N);
        HIP_TRY(hipGetLastError());
    }
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_mirror_upper_dev(double *d_emd, int N, void *stream) {
    if (!d_emd || N <= 0) return fail(PILOT_OT_EINVAL, "bad argument");
    hipLaunchKernelGGL(pilot::emd_mirror_kernel, dim3(1024), dim3(256), 0, static_cast<hipStream_t>(stream), d_emd, N);
    HIP_TRY(hipGetLastError());
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_emd_grid(const double *P, int N, int K, const double *M, int mode, int row_begin, int row_end,
                                int row_step, double *emd, int *n_aug) {
    if (!P || !M || !emd) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (N <= 0 || K <= 0) return fail(PILOT_OT_EINVAL, "N=%d K=%d must be positive", N, K);
    if (row_step < 1 || row_begin < 0 || row_end > N || row_begin > row_end)
        return fail(PILOT_OT_EINVAL, "bad row range [%d, %d) step %d for N=%d", row_begin, row_end, row_step, N);
    const int n_rows = (row_end - row_begin + row_step - 1) / row_step;
    const size_t n_out = (size_t)n_rows * N;
    if (n_out == 0) return PILOT_OT_OK;
    int rc = pilot::host_ctx_prepare(N, K, n_out);
    if (rc != PILOT_OT_OK) return rc;
    pilot::HostCtx &h = pilot::thread_host();
    hipError_t e = hipMemcpy(h.dP, P, sizeof(double) * (size_t)N * K, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h.dM, M, sizeof(double) * (size_t)K * K, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(h.dE, 0, sizeof(double) * n_out);
    if (e == hipSuccess) e = hipMemset(h.dIt, 0, sizeof(int) * n_out);
    if (e != hipSuccess) return fail(PILOT_OT_EHIP, "device staging failed: %s", hipGetErrorString(e));
    rc = pilot_ot_emd_grid_dev(h.plan, h.dP, h.dM, mode, row_begin, row_end, row_step, h.dE, h.dIt, nullptr);
    if (rc != PILOT_OT_OK) return rc;
    const pilot::Fetch f[2] = {{emd, h.dE, sizeof(double) * n_out}, {n_aug, h.dIt, sizeof(int) * n_out}};
    return pilot::host_fetch(f, 2);
}
