// K27: the apeglm-style shrunken coefficient of the negative-binomial GLM for a GENERAL design (include/pilot_ot.h, "negative-binomial
// GLM for a general design", pilot_ot_nb_design_shrink): K23's rule with K26's model.  Per gene, with c_j the counts,
// eta_j = x_j^T beta + log s_j, mu_j = e^{eta_j}, ONE column k of X shrunk and every other coefficient under a normal of scale sigma0:
//   P(beta) = sum_j [c log(a mu) - (c + 1/a) log1p(a mu)] - sum_{l != k} beta_l^2 / (2 sigma0^2) - log1p(beta_k^2 / S^2)
//   p(b)    = max over beta_{-k} of P(beta_{-k}, beta_k = b)      (strictly concave in beta_{-k}: the normal prior is its ridge)
// p can have two local maxima between 0 and the maximum-likelihood beta_k, so the estimate is DEFINED by K23's search.
//
// THE HOST MOVES COLUMN k LAST before the upload (X and beta_mle), so P stays the only template parameter and no register array is
// indexed by a variable (the warning at the top of nb_design_kernels.hpp); `coef` is only where the results are written.
//
// nb_design_shrink_kernel<T, P>   one wave per gene, A LANE IS A GRID POINT of t in [0, asinh(E / S)], b = sg S sinh(t).  c, log s and X
//                    are staged once in LDS as in nb_design_dispersion_kernel (8 m (2 + P) bytes) and read as broadcasts.  The search
//                    is K22's nb_grid_rounds.  Every lane fits the P - 1 other coefficients at its own b with nb_design_solve<P - 1>
//                    (b x_jk is folded into the sample's log size factor; the ridge is 1 / sigma0^2), round 0 from the maximum-
//                    likelihood coefficients passed in, a later round from the lane's own last point, then evaluates P once with
//                    K23's compensated sum.  The winner of the last round sums X^T W X over all P columns,
//                    w = mu (1 + a c) / (1 + a mu)^2.  No floating-point sum crosses lanes: the argmax is the only cross-lane step
//                    (the step count is an integer sum), so a gene gives the same bits alone and in any batch.
#pragma once
#include <hip/hip_runtime.h>

#include "nb_design_kernels.hpp"
#include "nb_shrink_kernel.hpp"

namespace pilot {

// Grid: n_genes workgroups of one wave.  Dynamic LDS: m (2 + P) doubles.  sf: the m size factors, then their m logarithms, then X
// (m x P, row-major, the shrunk column LAST).  beta_mle: n_genes x P in that column order.  coef: the caller's position of the shrunk
// column (1 .. P - 1).  beta_out: n_genes x P in the CALLER's column order; info: n_genes x P (P + 1) / 2, the packed upper triangle
// of X^T W X in the kernel's column order.  A NaN dispersion, a gene of zeros or a non-finite beta_mle leaves the gene out: NaN
// everywhere, flags 0.
template <typename T, int P>
__global__ void __launch_bounds__(64) nb_design_shrink_kernel(const T *__restrict__ Y, long long ld, int m, const double *__restrict__ sf,
                                                               const double *__restrict__ dispersion, const double *__restrict__ beta_mle,
                                                               const double *__restrict__ far_end, double S, double inv_var, int coef,
                                                               double *__restrict__ beta_out, double *__restrict__ objective,
                                                               double *__restrict__ info, int *__restrict__ flags_out) {
    static_assert(P >= 2 && P <= NB_DESIGN_MAX_COLS, "an intercept and 1 to 7 more columns");
    constexpr int Q = P - 1;                                 // the coefficients of the inner fit
    extern __shared__ double nb_design_shrink_lds[];
    double *sc = nb_design_shrink_lds, *sl = sc + m, *sx = sl + m;
    const int gene = blockIdx.x, lane = threadIdx.x;
    const double alpha = dispersion[gene];

    // (both tests are wave-uniform: the whole wave leaves before the barrier; the first one before any sample is read)
    const auto left_out = [&]() {
        if (lane == 0) {
            objective[gene] = __builtin_nan("");
            flags_out[gene] = 0;
        }
        if (lane < P) beta_out[(long long)gene * P + lane] = __builtin_nan("");
        if (lane < NB_TRI<P>) info[(long long)gene * NB_TRI<P> + lane] = __builtin_nan("");
    };
    double start[Q];
    bool usable = alpha == alpha;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        start[k] = beta_mle[(long long)gene * P + k];
        usable = usable && __builtin_isfinite(start[k]);
    }
    if (!usable) { left_out(); return; }
    int any = 0;
    for (int j = lane; j < m; j += 64) {
        const double c = rint((double)Y[(long long)j * ld + gene]);
        sc[j] = c;
        sl[j] = sf[m + j];
        any |= c > 0.0;
    }
    for (int t = lane; t < m * P; t += 64) sx[t] = sf[2 * m + t];
    any = lanes_reduce(any, Max{});
    if (!any) { left_out(); return; }
    __syncthreads();

    const double inv_alpha = 1.0 / alpha, fe = far_end[gene], t_end = asinh(fabs(fe) / S);
    double beta[Q], b = 0.0, value = 0.0;
#pragma unroll
    for (int k = 0; k < Q; ++k) beta[k] = start[k];
    bool at_end = true;
    int flags = 0, steps = 0;
    nb_grid_rounds(0.0, t_end, lane, [&](int, double t) {
        b = nb_shrink_beta1(fe, S, t);                       // (round 0 starts from beta_mle, a later round from the lane's last point)
        const double bk = b;
        bool done;
        steps += nb_design_solve<Q>(m, alpha, inv_var, beta, done, [&](int j, double &c, double &ls, double (&x)[Q]) {
            c = sc[j];
            ls = fma(bk, sx[j * P + Q], sl[j]);
#pragma unroll
            for (int k = 0; k < Q; ++k) x[k] = sx[j * P + k];
        });
        if (!done) flags |= NB_FLAG_NOT_CONVERGED;
        double L = 0.0, carry = 0.0;
        for (int j = 0; j < m; ++j) {
            double x[Q];
#pragma unroll
            for (int k = 0; k < Q; ++k) x[k] = sx[j * P + k];
            const double cc = sc[j], am = alpha * exp(nb_design_eta<Q>(x, beta, fma(bk, sx[j * P + Q], sl[j]))), l1p = log1p(am);
            // K23's compensated sum: near its top p is compared across lanes at the level of its rounding
            const double term = (cc > 0.0 ? cc * log(am) - (cc + inv_alpha) * l1p : -inv_alpha * l1p) - carry, next = L + term;
            carry = (next - L) - term;
            L = next;
        }
        double ridge = 0.0;
#pragma unroll
        for (int k = 0; k < Q; ++k) ridge = fma(beta[k], beta[k], ridge);
        const double z = b / S;
        value = L - 0.5 * ridge * inv_var - log1p(z * z);
        return value;
    }, [&](int round, int w) {
        if (w == 63 && at_end) flags |= NB_FLAG_AT_BOUND;
        at_end = at_end && w == 63;
        if (round == NB_ROUNDS - 1) {
            flags = lanes_reduce(flags, Max{});              // (AT_BOUND is uniform, so the largest value is the OR)
            steps = lanes_reduce(steps, Sum{});
            if (lane == w) {
                double M[NB_TRI<P>], full[P];
#pragma unroll
                for (int t = 0; t < NB_TRI<P>; ++t) M[t] = 0.0;
#pragma unroll
                for (int k = 0; k < Q; ++k) full[k] = beta[k];
                full[Q] = b;
                for (int j = 0; j < m; ++j) {
                    double x[P];
#pragma unroll
                    for (int k = 0; k < P; ++k) x[k] = sx[j * P + k];
                    const double cc = sc[j], mu = exp(nb_design_eta<P>(x, full, sl[j])), inv = 1.0 / (1.0 + alpha * mu);
                    nb_design_rank1<P>(M, x, (mu * inv) * ((1.0 + alpha * cc) * inv));
                }
#pragma unroll
                for (int k = 0; k < Q; ++k) beta_out[(long long)gene * P + (k < coef ? k : k + 1)] = beta[k];
                beta_out[(long long)gene * P + coef] = b;
                objective[gene] = value;
#pragma unroll
                for (int t = 0; t < NB_TRI<P>; ++t) info[(long long)gene * NB_TRI<P> + t] = M[t];
                flags_out[gene] = flags | (steps << NB_SHRINK_STEPS_SHIFT);
            }
        }
    });
}

}  // namespace pilot
