// Transport plans (optimal couplings) of selected ordered pairs: pilot_ot_transport_plans (include/pilot_ot.h).
//
// The pair grid computes every pair's plan and keeps only <M, Gamma>.  This translation unit compiles the same kernel sources
// once more with PILOT_PLAN_TU defined, which turns them into plan-emitting variants with their own names (emd_grid_plan_kernel,
// emd_generic_plan_kernel, sinkhorn_generic_plan_kernel) and an explicit pair list; the pair-grid kernels themselves are
// defined in pilot_ot_emd.hip / pilot_ot_sinkhorn.hip only and their code does not depend on this file.
//
// Pairs run in chunks: a chunk's plans land in a device scratch of at most PLAN_CHUNK_BYTES, and then either go to the host
// (per-pair mode) or are added into the group accumulators (group mode, plan_group_sum_kernel) before the next chunk reuses it.
#define PILOT_PLAN_TU
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "abi_common.hpp"
#include "emd_kernels.hpp"
#include "emd_generic_kernel.hpp"
#include "generic_kernels.hpp"

namespace pilot {

// Group sums: thread (g, e) adds entry e of the plans of group g's pairs in this chunk, in list order, to acc[g][e].
// gidx holds the pair indices sorted by group and, within a group, ascending (goff: where each group starts), so a group's
// pairs of the chunk [c0, c1) are a contiguous run found by a binary search.  One f64 sum per entry in a fixed order: the
// result is that of a host loop acc += plan over the list, bit for bit, and the same on every run.  Eight loads are issued
// before their adds (the adds keep their order): a single group has only K^2 threads to hide HBM latency with.
__global__ void __launch_bounds__(256) plan_group_sum_kernel(const double *__restrict__ plans, long c0, long c1, int KK,
                                                             const int *__restrict__ goff, const int *__restrict__ gidx,
                                                             long n_groups, double *__restrict__ acc) {
    const long total = n_groups * KK;
    for (long t = blockIdx.x * 256L + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int g = (int)(t / KK), e = (int)(t % KK);
        int lo = goff[g];
        const int hi = goff[g + 1];
        for (int h = hi; lo < h;) {
            const int mid = lo + (h - lo) / 2;
            if (gidx[mid] < c0) lo = mid + 1; else h = mid;
        }
        double s = acc[t];
        int k = lo;
        for (; k + 8 <= hi && gidx[k + 7] < c1; k += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = plans[(size_t)(gidx[k + u] - c0) * KK + e];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; k < hi && gidx[k] < c1; ++k) s += plans[(size_t)(gidx[k] - c0) * KK + e];
        acc[t] = s;
    }
}

}  // namespace pilot

namespace {

// at most this many bytes of plans on the device at a time (the pool adds a quarter on top: under 1 GiB in all)
constexpr size_t PLAN_CHUNK_BYTES = (size_t)768 << 20;
// the device limits and the launch geometry of pilot_ot_emd_grid_dev's one-wave-per-pair kernel (emd_kernels.hpp)
using pilot::LDS_BYTES, pilot::EMD_MAX_K, pilot::GENERIC_MAX_K, pilot::emd_nk, pilot::emd_wgs_per_cu;

}  // namespace

PILOT_API int pilot_ot_transport_plans(const double *P, int N, int K, const double *M, int regularized, double reg,
                                       int num_iter_max, double stop_thr, double tau, int check_period,
                                       const int *pair_i, const int *pair_j, long long n_pairs,
                                       const int *pair_group, int n_groups,
                                       double *plans, double *values, int *iters, int *flags) {
    // ---- arguments (no HIP call before they are all checked) ----
    if (!P || !M || !pair_i || !pair_j || !plans) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (N <= 0 || K <= 0) return fail(PILOT_OT_EINVAL, "N=%d K=%d must be positive", N, K);
    if (regularized != 0 && regularized != 1) return fail(PILOT_OT_EINVAL, "regularized=%d must be 0 (exact) or 1 (entropic)", regularized);
    if (regularized) {
        if (!(reg > 0.0) || !std::isfinite(reg)) return fail(PILOT_OT_EINVAL, "reg=%g must be positive and finite", reg);
        if (num_iter_max < 1) return fail(PILOT_OT_EINVAL, "num_iter_max=%d must be >= 1", num_iter_max);
        if (check_period < 1) return fail(PILOT_OT_EINVAL, "check_period=%d must be >= 1", check_period);
        if (!(stop_thr >= 0.0) || !(stop_thr < 1.0)) return fail(PILOT_OT_EINVAL, "stop_thr=%g must be in [0, 1)", stop_thr);
        if (!(tau > 1.0)) return fail(PILOT_OT_EINVAL, "tau=%g must be > 1", tau);
    }
    if (n_pairs < 0) return fail(PILOT_OT_EINVAL, "n_pairs=%lld must be >= 0", n_pairs);
    if (n_pairs > (long long)INT32_MAX) return fail(PILOT_OT_EINVAL, "n_pairs=%lld > %d", n_pairs, INT32_MAX);
    if (pair_group && n_groups <= 0) return fail(PILOT_OT_EINVAL, "n_groups=%d must be positive", n_groups);
    for (long long t = 0; t < n_pairs; ++t) {
        if (pair_i[t] < 0 || pair_i[t] >= N || pair_j[t] < 0 || pair_j[t] >= N)
            return fail(PILOT_OT_EINVAL, "pair %lld = (%d, %d) out of range for N=%d", t, pair_i[t], pair_j[t], N);
        if (pair_group && (pair_group[t] < 0 || pair_group[t] >= n_groups))
            return fail(PILOT_OT_EINVAL, "group %d of pair %lld out of range for n_groups=%d", pair_group[t], t, n_groups);
    }
    if (K > GENERIC_MAX_K) return fail(PILOT_OT_ENOTSUP, "transport plans: K=%d > %d cell types", K, GENERIC_MAX_K);
    if (n_pairs == 0) return PILOT_OT_OK;

    const long n = (long)n_pairs, KK = (long)K * K;
    long chunk = (long)(PLAN_CHUNK_BYTES / (sizeof(double) * (size_t)KK));
    if (chunk < 1) chunk = 1;
    if (const char *e = pilot::test_switch("PILOT_OT_PLAN_CHUNK_PAIRS")) { const long v = atol(e); if (v > 0 && v < chunk) chunk = v; }   // (tests)
    if (chunk > n) chunk = n;
    const int cus = pilot::cu_count();

    double *dP, *dM, *dVal, *dPlans;
    int *dPI, *dPJ, *dIt, *dFl, *dQ;
    HIP_TRY(pilot::ws(pilot::WS_PLAN_P, (size_t)N * K, &dP));
    HIP_TRY(pilot::ws(pilot::WS_PLAN_M, (size_t)KK, &dM));
    HIP_TRY(pilot::ws(pilot::WS_PLAN_PI, (size_t)n, &dPI));
    HIP_TRY(pilot::ws(pilot::WS_PLAN_PJ, (size_t)n, &dPJ));
    HIP_TRY(pilot::ws(pilot::WS_PLAN_VAL, (size_t)n, &dVal));
    HIP_TRY(pilot::ws(pilot::WS_PLAN_IT, (size_t)n, &dIt));
    HIP_TRY(pilot::ws(pilot::WS_PLAN_FL, (size_t)n, &dFl));
    HIP_TRY(pilot::ws(pilot::WS_PLAN_Q, (size_t)pilot::EMD_NQ * pilot::EMD_Q_STRIDE, &dQ));
    HIP_TRY(pilot::ws(pilot::WS_PLAN_PLANS, (size_t)chunk * KK, &dPlans));
    HIP_TRY(hipMemcpy(dP, P, sizeof(double) * (size_t)N * K, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dM, M, sizeof(double) * (size_t)KK, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dPI, pair_i, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dPJ, pair_j, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(dFl, 0, sizeof(int) * (size_t)n, nullptr));

    // group mode: pair indices sorted by group (stable: list order within a group) and the accumulators
    double *dAcc = nullptr;
    int *dGoff = nullptr, *dGidx = nullptr;
    if (pair_group) {
        std::vector<int> goff((size_t)n_groups + 1, 0), gidx((size_t)n);
        for (long t = 0; t < n; ++t) ++goff[(size_t)pair_group[t] + 1];
        for (int g = 0; g < n_groups; ++g) goff[(size_t)g + 1] += goff[(size_t)g];
        std::vector<int> cur(goff.begin(), goff.end() - 1);
        for (long t = 0; t < n; ++t) gidx[(size_t)cur[(size_t)pair_group[t]]++] = (int)t;
        HIP_TRY(pilot::ws(pilot::WS_PLAN_ACC, (size_t)n_groups * KK, &dAcc));
        HIP_TRY(pilot::ws(pilot::WS_PLAN_GOFF, goff.size(), &dGoff));
        HIP_TRY(pilot::ws(pilot::WS_PLAN_GIDX, (size_t)n, &dGidx));
        HIP_TRY(hipMemcpy(dGoff, goff.data(), sizeof(int) * goff.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dGidx, gidx.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemsetAsync(dAcc, 0, sizeof(double) * (size_t)n_groups * KK, nullptr));
    }

    // ---- per-solver set-up: the launch geometry of the pair grid's kernel for this K ----
    pilot::EmdParams ep{};
    pilot::GenericParams gp{};
    size_t lds = 0;
    long wgs = 0;
    double *dRowmin = nullptr;
    if (!regularized) {
        ep.P = dP; ep.M = dM; ep.N = N; ep.K = K;
        ep.n_rows = 0; ep.row_begin = 0; ep.row_step = 1; ep.upper_only = 0;
        ep.queue = dQ;
        if (K <= EMD_MAX_K) {
            const int waves = pilot::emd_waves(emd_nk(K));
            lds = pilot::emd_lds_bytes(K);
            if (lds > LDS_BYTES) return fail(PILOT_OT_ENOTSUP, "K=%d does not fit the LDS layout", K);
            wgs = (chunk + waves - 1) / waves;
            const long cap = (long)cus * emd_wgs_per_cu(K);
            if (wgs > cap) wgs = cap;
            HIP_TRY(pilot::ws(pilot::WS_PLAN_SLAB, (size_t)wgs * waves * KK, &ep.f_slab));   // (each wave zeroes its own block first)
        } else {
            const size_t per_wg = sizeof(double) * pilot::emdg_slab_doubles(K);
            wgs = 2L * cus;
            while (wgs > 1 && per_wg * (size_t)wgs > ((size_t)8 << 30)) wgs /= 2;
            if (wgs > chunk) wgs = chunk;
            lds = pilot::emdg_lds_bytes(K);
            HIP_TRY(pilot::ws(pilot::WS_PLAN_SLAB, pilot::emdg_slab_doubles(K) * (size_t)wgs, &ep.f_slab));
            std::vector<double> rowmin((size_t)K);         // the initial row potentials min_j M_ij (exact on the host)
            for (int i = 0; i < K; ++i) {
                double m = INFINITY;
                for (int j = 0; j < K; ++j) m = M[(size_t)i * K + j] < m ? M[(size_t)i * K + j] : m;
                rowmin[(size_t)i] = m;
            }
            HIP_TRY(pilot::ws(pilot::WS_PLAN_ROWMIN, (size_t)K, &dRowmin));
            HIP_TRY(hipMemcpy(dRowmin, rowmin.data(), sizeof(double) * (size_t)K, hipMemcpyHostToDevice));
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pilot::emd_generic_plan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
    } else {
        int nsplit = pilot::GENERIC_WAVES;
        auto lds_for = [&](int ns) { return sizeof(double) * ((8 + (size_t)ns) * (size_t)K + pilot::GENERIC_WAVES) + 16; };
        while (nsplit > 1 && lds_for(nsplit) > LDS_BYTES) nsplit /= 2;
        lds = lds_for(nsplit);
        if (lds > LDS_BYTES) return fail(PILOT_OT_ENOTSUP, "K=%d does not fit the generic kernel's LDS vectors", K);
        wgs = 3L * cus;
        const size_t per = sizeof(double) * 2 * (size_t)KK;
        while (wgs > 1 && per * (size_t)wgs > ((size_t)8 << 30)) wgs /= 2;
        if (wgs > chunk) wgs = chunk;
        gp.P = dP; gp.M = dM; gp.N = N; gp.K = K; gp.n_pairs = 0; gp.row_begin = 0; gp.row_step = 1;
        gp.reg = reg; gp.tau = tau; gp.stop_thr = stop_thr; gp.max_iter = num_iter_max; gp.period = check_period;
        gp.err = nullptr; gp.queue = dQ; gp.list = nullptr; gp.list_len = nullptr; gp.nsplit = nsplit;
        HIP_TRY(pilot::ws(pilot::WS_PLAN_KWS, per / sizeof(double) * (size_t)wgs, &gp.kws));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pilot::sinkhorn_generic_plan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }

    // ---- chunks ----
    for (long c0 = 0; c0 < n; c0 += chunk) {
        const long nc = std::min(chunk, n - c0);
        pilot::PlanArgs pa;
        pa.pair_i = dPI + c0; pa.pair_j = dPJ + c0; pa.n_pairs = nc; pa.plans = dPlans;
        const unsigned grid = (unsigned)std::min(wgs, nc);
        if (!regularized) {
            ep.emd = dVal + c0; ep.n_aug = dIt + c0;
            if (K <= EMD_MAX_K) {      // (the support walk writes the nonzero flows only)
                HIP_TRY(hipMemsetAsync(dPlans, 0, sizeof(double) * (size_t)nc * KK, nullptr));
                HIP_TRY(hipMemsetAsync(dQ, 0, sizeof(int) * pilot::EMD_NQ * pilot::EMD_Q_STRIDE, nullptr));
                const int waves = pilot::emd_waves(emd_nk(K));
                const unsigned g = (unsigned)std::min(wgs, (nc + waves - 1) / waves);
                constexpr bool UL = pilot::emd_ul(128);
                if (K > 192) {
                    hipLaunchKernelGGL((pilot::emd_grid_plan_kernel<4, true, UL>), dim3(g), dim3(64 * waves), lds, nullptr, ep, pa);
                } else if (K > 128) {
                    hipLaunchKernelGGL((pilot::emd_grid_plan_kernel<3, true, UL>), dim3(g), dim3(64 * waves), lds, nullptr, ep, pa);
                } else if (K <= 64) {
                    auto kern = pilot::emd_ul(K) ? pilot::emd_grid_plan_kernel<1, false, true> : pilot::emd_grid_plan_kernel<1, false, false>;
                    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                    hipLaunchKernelGGL(kern, dim3(g), dim3(64 * waves), lds, nullptr, ep, pa);
                } else {
                    auto kern = pilot::emd_grid_plan_kernel<2, false, UL>;
                    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                    hipLaunchKernelGGL(kern, dim3(g), dim3(64 * waves), lds, nullptr, ep, pa);
                }
            } else {                   // (the final pass writes every entry)
                HIP_TRY(hipMemsetAsync(dQ, 0, sizeof(int), nullptr));
                hipLaunchKernelGGL(pilot::emd_generic_plan_kernel, dim3(grid), dim3(pilot::EMDG_WG), lds, nullptr, ep, dRowmin, pa);
            }
        } else {
            gp.emd = dVal + c0; gp.iters = dIt + c0; gp.flags = dFl + c0;
            HIP_TRY(hipMemsetAsync(dQ, 0, sizeof(int), nullptr));
            hipLaunchKernelGGL(pilot::sinkhorn_generic_plan_kernel, dim3(grid), dim3(pilot::GENERIC_WG), lds, nullptr, gp, pa);
        }
        HIP_TRY(hipGetLastError());
        if (pair_group) {
            const long total = (long)n_groups * KK;
            const unsigned g = (unsigned)std::min<long>((total + 255) / 256, 1L << 20);
            hipLaunchKernelGGL(pilot::plan_group_sum_kernel, dim3(g), dim3(256), 0, nullptr, dPlans, c0, c0 + nc, (int)KK, dGoff, dGidx,
                               (long)n_groups, dAcc);
            HIP_TRY(hipGetLastError());
        } else {
            HIP_TRY(hipMemcpy(plans + (size_t)c0 * KK, dPlans, sizeof(double) * (size_t)nc * KK, hipMemcpyDeviceToHost));
        }
    }
    if (pair_group) HIP_TRY(hipMemcpy(plans, dAcc, sizeof(double) * (size_t)n_groups * KK, hipMemcpyDeviceToHost));
    if (values) HIP_TRY(hipMemcpy(values, dVal, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    if (iters) HIP_TRY(hipMemcpy(iters, dIt, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    if (flags) HIP_TRY(hipMemcpy(flags, dFl, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    return PILOT_OT_OK;
}
