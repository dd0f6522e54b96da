// K23: the apeglm-style shrunken fold change of the two-group negative-binomial model (Zhu, Ibrahim, Love 2019; include/pilot_ot.h,
// "negative-binomial GLM", pilot_ot_nb_shrink).  Per gene, with c_p the counts and s_p the size factors in K22's
// sorted order (group 0 at positions 0 .. n0 - 1, group 1 at n0 .. m - 1), eta_0 = b0, eta_1 = b0 + b1, mu_p = s_p exp(eta_g(p)):
//   P(b0, b1) = sum_p [c log(a mu) - (c + 1/a) log1p(a mu)] - b0^2 / (2 sigma0^2) - log1p(b1^2 / S^2)
//   p(b1)     = max_b0 P(b0, b1),   the root in b0 of   sum_p (c - mu) / (1 + a mu) - b0 / sigma0^2   (strictly decreasing)
// p can have two local maxima between 0 and the maximum-likelihood b1, so the estimate is DEFINED by a search:
//
// nb_shrink_kernel   one wave per gene, A LANE IS A GRID POINT of t in [0, asinh(E / S)], b1 = sg S sinh(t).  The gene's c_p and s_p
//                    are staged once in LDS and read as broadcasts.  The search is K22's nb_grid_rounds: every lane solves its own
//                    b0 (nb_shrink_solve: K22's nb_bracketed_root, warm-started from the lane's last b0: one exp per group and one
//                    divide per sample a step), then evaluates p once (nb_shrink_value: the only log / log1p).
//                    No floating-point sum crosses lanes, and a group's part of every sum is closed on its own.
//                    LDS: 16 m bytes.
// The per-lane arithmetic is __host__ __device__: a stand-alone host program that includes this header runs nb_shrink_solve on fixed
// inputs, which is how a change to the shared root finder is compared bit for bit before it reaches a GPU.
#pragma once
#include <hip/hip_runtime.h>

#include "nb_glm_kernels.hpp"

namespace pilot {

constexpr int NB_FLAG_AT_BOUND = 4;         // PILOT_OT_NB_AT_BOUND
constexpr int NB_SHRINK_STEPS_SHIFT = 8;    // PILOT_OT_NB_SHRINK_STEPS_SHIFT: flags >> 8 = the gene's inner steps, all lanes and rounds

// what a lane needs of its gene beside the staged samples
struct NbShrinkGene {
    int m, n0;
    double alpha, inv_alpha, inv_var0;      // the dispersion, 1 / alpha, 1 / sigma0^2
    double s_sum[2], c_sum, log_qmax[2];    // per group sum s; sum c; log max c / s (-inf for a group of zeros)
};

__host__ __device__ inline void nb_shrink_gene(const double *c, const double *s, int m, int n0, double alpha, double sigma0, NbShrinkGene &g) {
    g.m = m;
    g.n0 = n0;
    g.alpha = alpha;
    g.inv_alpha = 1.0 / alpha;
    g.inv_var0 = 1.0 / (sigma0 * sigma0);
    g.c_sum = 0.0;
    int p = 0;
    for (int k = 0; k < 2; ++k) {
        const int end = k ? m : n0;
        double ss = 0.0, cs = 0.0, qmax = 0.0;
        for (; p < end; ++p) {
            const double q = c[p] / s[p];
            ss += s[p];
            cs += c[p];
            qmax = q > qmax ? q : qmax;
        }
        g.s_sum[k] = ss;
        g.c_sum += cs;
        g.log_qmax[k] = log(qmax);
    }
}

// the score in b0 at (u, b1) and its derivative (negative)
__host__ __device__ inline void nb_shrink_score(const double *c, const double *s, const NbShrinkGene &g, double u, double b1, double &f, double &df) {
    double sf = 0.0, sd = 0.0;
    int p = 0;
    for (int k = 0; k < 2; ++k) {
        const int end = k ? g.m : g.n0;
        const double e = exp(k ? u + b1 : u);
        double gf = 0.0, gd = 0.0;
        for (; p < end; ++p) {
            const double cc = c[p], mu = s[p] * e, r = 1.0 / (1.0 + g.alpha * mu);
            gf += (cc - mu) * r;
            gd += mu * (1.0 + g.alpha * cc) * (r * r);
        }
        sf += gf;
        sd += gd;
    }
    f = sf - u * g.inv_var0;
    df = -(sd + g.inv_var0);
}

// a bracket of the root in b0 at b1, one unit wider than what holds it:  above max(0, log max_p c_p / (s_p e^{b1 [g = 1]})) every
// term of the score is <= 0;  below -max(1, log(sigma0^2 (sum_0 s + e^{b1} sum_1 s))) the terms sum to more than -sum mu >= u / sigma0^2
__host__ __device__ inline void nb_shrink_bracket(const NbShrinkGene &g, double b1, double &ulo, double &uhi) {
    const double q1 = g.log_qmax[1] - b1, top = g.log_qmax[0] > q1 ? g.log_qmax[0] : q1;
    const double low = log((g.s_sum[0] + exp(b1) * g.s_sum[1]) / g.inv_var0);
    uhi = (top > 0.0 ? top : 0.0) + 1.0;
    ulo = -(low > 1.0 ? low : 1.0) - 1.0;
}

// where a lane without a previous b0 starts: the Poisson estimate at b1
__host__ __device__ inline double nb_shrink_start(const NbShrinkGene &g, double b1) { return log(g.c_sum / (g.s_sum[0] + exp(b1) * g.s_sum[1])); }

// the root in b0 at b1 from u (moved into the bracket) by nb_bracketed_root, the ends counting as inside.  Returns the steps taken;
// converged = false after NB_FIT_MAX_STEPS.
__host__ __device__ inline int nb_shrink_solve(const double *c, const double *s, const NbShrinkGene &g, double b1, double &u, bool &converged) {
    double ulo, uhi;
    nb_shrink_bracket(g, b1, ulo, uhi);
    u = u > ulo ? (u < uhi ? u : uhi) : ulo;                 // (a NaN start goes to ulo)
    return nb_bracketed_root<true>(ulo, uhi, u, converged, [&](double at, double &f, double &df) { nb_shrink_score(c, s, g, at, b1, f, df); });
}

// P(u, b1) and the two groups' observed information there
__host__ __device__ inline double nb_shrink_value(const double *c, const double *s, const NbShrinkGene &g, double u, double b1, double S,
                                                  double &w0, double &w1) {
    double L = 0.0, w[2];
    int p = 0;
    for (int k = 0; k < 2; ++k) {
        const int end = k ? g.m : g.n0;
        const double e = exp(k ? u + b1 : u);
        double Lg = 0.0, carry = 0.0, wg = 0.0;
        for (; p < end; ++p) {
            const double cc = c[p], mu = s[p] * e, am = g.alpha * mu, l1p = log1p(am), den = 1.0 + am;
            // a compensated sum: near its top p is compared across lanes at the level of its rounding, and a plain sum of 4096 terms
            // of mixed sign loses more than the terms themselves carry (four adds beside a log1p and a log)
            const double term = (cc > 0.0 ? cc * log(am) - (cc + g.inv_alpha) * l1p : -g.inv_alpha * l1p) - carry, next = Lg + term;
            carry = (next - Lg) - term;
            Lg = next;
            wg += mu * (1.0 + g.alpha * cc) / (den * den);
        }
        L += Lg;
        w[k] = wg;
    }
    w0 = w[0];
    w1 = w[1];
    const double z = b1 / S;
    return L - 0.5 * u * u * g.inv_var0 - log1p(z * z);
}

__host__ __device__ inline double nb_shrink_beta1(double far_end, double S, double t) { return (far_end >= 0.0 ? S : -S) * sinh(t); }

// Grid: n_genes workgroups of one wave.  Dynamic LDS: 2 m doubles.  order, ss: K22's sorted design of two groups, n0 samples in
// group 0.  info: n_genes x 2 (w0, w1).  A NaN dispersion leaves its gene out: NaN everywhere, flags 0.
template <typename T>
__global__ void __launch_bounds__(64) nb_shrink_kernel(const T *__restrict__ Y, long long ld, int m, int n0, const int *__restrict__ order,
                                                        const double *__restrict__ ss, const double *__restrict__ dispersion,
                                                        const double *__restrict__ far_end, double S, double sigma0,
                                                        double *__restrict__ beta0, double *__restrict__ beta1, double *__restrict__ objective,
                                                        double *__restrict__ info, int *__restrict__ flags_out) {
    extern __shared__ double nb_shrink_lds[];
    double *sc = nb_shrink_lds, *sS = sc + m;
    const int gene = blockIdx.x, lane = threadIdx.x;
    const double alpha = dispersion[gene];
    if (alpha != alpha) {                                    // (uniform: the whole wave leaves before the barrier)
        if (lane == 0) {
            beta0[gene] = beta1[gene] = objective[gene] = info[2 * (long long)gene] = info[2 * (long long)gene + 1] = __builtin_nan("");
            flags_out[gene] = 0;
        }
        return;
    }
    for (int p = lane; p < m; p += 64) {
        sc[p] = rint((double)Y[(long long)order[p] * ld + gene]);
        sS[p] = ss[p];
    }
    __syncthreads();

    NbShrinkGene g;
    nb_shrink_gene(sc, sS, m, n0, alpha, sigma0, g);
    const double fe = far_end[gene], t_end = asinh(fabs(fe) / S);
    double u = 0.0, b1 = 0.0, P = 0.0, w0 = 0.0, w1 = 0.0;
    bool at_end = true;
    int flags = 0, steps = 0;
    nb_grid_rounds(0.0, t_end, lane, [&](int round, double t) {
        b1 = nb_shrink_beta1(fe, S, t);
        if (round == 0) u = nb_shrink_start(g, b1);          // (later rounds start from the lane's last b0)
        bool converged;
        steps += nb_shrink_solve(sc, sS, g, b1, u, converged);
        if (!converged) flags |= NB_FLAG_NOT_CONVERGED;
        P = nb_shrink_value(sc, sS, g, u, b1, S, w0, w1);
        return P;
    }, [&](int round, int b) {
        if (b == 63 && at_end) flags |= NB_FLAG_AT_BOUND;
        at_end = at_end && b == 63;
        if (round == NB_ROUNDS - 1) {
            flags = lanes_reduce(flags, Max{});              // (AT_BOUND is uniform, so the largest value is the OR)
            steps = lanes_reduce(steps, Sum{});
            if (lane == b) {
                beta0[gene] = u;
                beta1[gene] = b1;
                objective[gene] = P;
                info[2 * (long long)gene] = w0;
                info[2 * (long long)gene + 1] = w1;
                flags_out[gene] = flags | (steps << NB_SHRINK_STEPS_SHIFT);
            }
        }
    });
}

}  // namespace pilot
