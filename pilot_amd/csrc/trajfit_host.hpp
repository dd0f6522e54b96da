// The host side that the trajectory fits (pilot_ot_trajfit.hip) and the bootstrap fits (pilot_ot_bootfit.hip) share: the
// solver's constants, the map of the times to u with the per-model matrices that do not depend on a Gram, the step cap and
// the staging of u and the arguments struct (kernels: trajfit_kernels.hpp, bootfit_kernels.hpp).  Host-side only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "abi_common.hpp"
#include "trajfit_kernels.hpp"

namespace pilot {

constexpr int TF_MAX_ITER = 100;             // Newton steps per fit before PILOT_OT_TRAJFIT_NOT_CONVERGED
constexpr double TF_HUBER_ALPHA = 1e-4;      // scikit-learn's HuberRegressor default penalty

// u = (x - m) / s (m = mean(x), s = max |x - m|, 1 when every time is the same) and what of TrajfitArgs follows from m and s
// alone: per model the basis (C, quad_k, quad_scale), the coefficients on [1, f(x)] (R) and the penalty alpha ||w||^2 written
// on gamma (pen); sigma_min and n.  Everything else of `a` is zero afterwards.
inline void trajfit_time_map(const double *x, int n, std::vector<double> &u, TrajfitArgs &a) {
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum += x[i];
    const double m = sum / n;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s = std::max(s, std::fabs(x[i] - m));
    if (!(s > 0.0)) s = 1.0;
    u.resize(n);
    for (int i = 0; i < n; ++i) u[i] = (x[i] - m) / s;
    const double kappa = 2.0 * m / s, qs = 1.0 / (1.0 + std::fabs(kappa));
    // delta (prediction polynomial in u) -> coefficients of 1, x, x^2
    const double E[3][3] = {{1.0, -m / s, m * m / (s * s)}, {0.0, 1.0 / s, -2.0 * m / (s * s)}, {0.0, 0.0, 1.0 / (s * s)}};
    std::memset(&a, 0, sizeof(a));
    for (int md = 0; md < 3; ++md) {
        TrajfitModel &M = a.mod[md];
        const int p = md == 1 ? 3 : 2;
        double C[3][3] = {};
        C[0][0] = 1.0;
        if (md == 0) C[1][1] = 1.0;
        else if (md == 1) { C[1][1] = 1.0; C[2][2] = 1.0; }
        else { C[1][1] = kappa * qs; C[2][1] = qs; }
        std::memcpy(M.C, C, sizeof(C));
        double EC[3][3] = {};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < p; ++j)
                for (int k = 0; k < 3; ++k) EC[i][j] += E[i][k] * C[k][j];
        const int rows[3] = {0, md == 2 ? 2 : 1, 2};                                   // quadratic: [1, x^2]
        for (int i = 0; i < p; ++i)
            for (int j = 0; j < p; ++j) M.R[i][j] = EC[rows[i]][j];
        for (int i = 0; i < p; ++i)
            for (int j = 0; j < p; ++j)
                for (int r = 1; r < p; ++r) M.pen[i][j] += TF_HUBER_ALPHA * M.R[r][i] * M.R[r][j];
    }
    a.quad_k = kappa;
    a.quad_scale = qs;
    a.sigma_min = 10.0 * DBL_EPSILON;
    a.n = n;
}

// the step cap: TF_MAX_ITER, or the lower value of the PILOT_OT_TRAJFIT_MAX_ITER switch (tests: the NOT_CONVERGED path)
inline int trajfit_max_iter() {
    if (const char *sw = test_switch("PILOT_OT_TRAJFIT_MAX_ITER")) {
        const int v = atoi(sw);
        if (v >= 0 && v < TF_MAX_ITER) return v;
    }
    return TF_MAX_ITER;
}

// u, then the arguments struct, in one buffer of `slot`
inline int trajfit_stage(WsSlot slot, const std::vector<double> &u, const TrajfitArgs &a, const double **d_u,
                         const TrajfitArgs **d_args) {
    const size_t n = u.size(), n_args = (sizeof(TrajfitArgs) + sizeof(double) - 1) / sizeof(double);
    double *buf;
    HIP_TRY(ws(slot, n + n_args, &buf));
    HIP_TRY(hipMemcpy(buf, u.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(buf + n, &a, sizeof(a), hipMemcpyHostToDevice));
    *d_u = buf;
    *d_args = reinterpret_cast<const TrajfitArgs *>(buf + n);
    return PILOT_OT_OK;
}

}  // namespace pilot
