// K22: the negative-binomial GLM of DESeq2 for a one-factor design (an intercept plus a group indicator), where every piece
// decouples by group: the dispersion of a gene by a grid search on its Cox-Reid adjusted profile likelihood, and the normalised
// mean of every (gene, group) as the root of one monotone score equation.  Y is samples x genes, row-major; c = rint(Y).  All
// arithmetic is f64 with the device lgamma / log1p / log / exp.  The host (pilot_ot_nb_glm.hip) orders the samples by group once:
//   order[p]  the sample at sorted position p (group ascending, sample ascending within a group)
//   gof[p]    its group,   ss[p] its size factor,   gstart[g] .. gstart[g + 1]  the positions of group g
//
// nb_check_kernel       the first negative or non-finite count as min((gene << 32) | sample).
// nb_dispersion_kernel  one wave per gene, A LANE IS A GRID POINT.  The gene's c_p and mu_p = max(s_p * mean_{g(p)} c / s, minmu) are
//                       staged once in LDS in sorted order (the group means by one lane per group, one add per sample in sorted
//                       order); then every lane walks the samples in that order, reading them as broadcasts, and evaluates
//                         L(x) = sum_p [lgamma(c + r) - lgamma(r) - (c + r) log1p(a mu) + c log(a mu)] - 1/2 sum_g log(sum_{p in g} w_p)
//                                [- (x - prior_mean)^2 / (2 prior_var)],    a = exp(x), r = 1 / a, w = mu / (1 + a mu)
//                       at its own x.  c is wave-uniform, so "c == 0" (where the bracket is -r log1p(a mu): the two lgamma cancel
//                       exactly and c log is 0) is a uniform branch, and so is a group boundary: one running sum of w per lane closes
//                       each group's log term, and L adds the groups' closed parts in group order (so with two groups the result
//                       does not depend on which of them is code 0).  No sum crosses lanes; the only cross-lane step is the first-maximum argmax
//                       of nb_grid_rounds.  LDS: 8 (2 m + k) bytes.
// nb_group_fit_kernel   one lane per (gene, group), genes along the lanes so that a sample's row is read coalesced.  The root of
//                         f(q) = sum_{p in g} (c_p - s_p q) / (1 + a s_p q)
//                       in u = log q by nb_bracketed_root, from the Poisson estimate sum c / sum s.
//
// The two pieces K23 (nb_shrink_kernel.hpp) shares:
// nb_grid_rounds        the search of a wave whose lanes are grid points: NB_ROUNDS rounds of the NB_GRID-point grid
//                       x_i = lo + (hi - lo) * i / 63 inside one launch, the first largest value winning (reduce.hpp's lanes_best with
//                       LowestMax) and the next bracket being [x_{max(b-1,0)}, x_{min(b+1,63)}].
// nb_bracketed_root     the root of a decreasing score by Newton steps kept inside a shrinking bracket, bisection when a step leaves
//                       it or gains too little; to NB_FIT_TOL in at most NB_FIT_MAX_STEPS steps.
#pragma once
#include <hip/hip_runtime.h>

#include "reduce.hpp"

namespace pilot {

typedef unsigned long long nb_u64;

constexpr int NB_GRID = 64;                 // grid points = lanes
constexpr int NB_ROUNDS = 6;
constexpr int NB_MAX_SAMPLES = 4096;        // pilot_ot_nb_glm_max_samples: 8 (2 m + k) <= 96 KiB of the CU's 160 KiB
constexpr double NB_MIN_DISP = 1e-8;
constexpr double NB_MIN_MU = 0.5;
constexpr int NB_FIT_MAX_STEPS = 100;
constexpr double NB_FIT_TOL = 1e-12;
constexpr int NB_FLAG_NOT_CONVERGED = 1;    // PILOT_OT_NB_NOT_CONVERGED
constexpr int NB_FLAG_FLOORED = 2;          // PILOT_OT_NB_FLOORED
constexpr nb_u64 NB_NO_BAD = ~0ull;

__host__ __device__ inline double nb_max_disp(long long m) { return m > 10 ? (double)m : 10.0; }

// One wave, lane = grid point.  eval(round, x): the value at this lane's point x;  won(round, b): lane b holds the round's first largest
// value (b is wave-uniform; the caller keeps what its eval computed and writes its results from lane b of round NB_ROUNDS - 1).
template <typename Eval, typename Won>
__device__ inline void nb_grid_rounds(double lo, double hi, int lane, Eval eval, Won won) {
    for (int round = 0; round < NB_ROUNDS; ++round) {
        double best = eval(round, lo + (hi - lo) * (double)lane / 63.0);
        int b = lane;
        lanes_best(best, b, LowestMax{});
        const int bl = b > 0 ? b - 1 : 0, bh = b < 63 ? b + 1 : 63;
        const double nlo = lo + (hi - lo) * (double)bl / 63.0, nhi = lo + (hi - lo) * (double)bh / 63.0;
        won(round, b);
        lo = nlo;
        hi = nhi;
    }
}

// The root in [ulo, uhi] of score(u, f, df) (f >= 0 at ulo, f <= 0 at uhi, df < 0) from u inside the bracket.  Returns the steps taken,
// NB_FIT_MAX_STEPS with converged = false when the last step is still longer than NB_FIT_TOL.
// ENDS_INSIDE: whether a Newton step that lands ON an end of the bracket is taken (true) or replaced by a bisection (false).
//   false  nb_group_fit_kernel (K22), on purpose: the rule decides the last bits of q and the step counts of a fit that ends on a
//          step of 0, and K22's were recorded with it (one solve per
//          (gene, group): the bisection a rejected step restarts costs a few steps, not the convergence).
//   true   nb_shrink_solve (K23).  One end of the bracket is always u itself, so a Newton step below the last bit of u, un == u, lands
//          on an end: it is a step of 0 and ends the loop -- rejected, it would restart a bisection of whatever bracket the
//          one-sided iterates have left, which K23 pays 384 times a gene.
template <bool ENDS_INSIDE, typename Score>
__host__ __device__ inline int nb_bracketed_root(double ulo, double uhi, double &u, bool &converged, Score score) {
    double dxold = uhi - ulo, dx = dxold, f, df;
    score(u, f, df);
    converged = false;
    int steps;
    for (steps = 1; steps <= NB_FIT_MAX_STEPS; ++steps) {
        if (f > 0.0) ulo = u; else uhi = u;
        const double un = u - f / df;
        dxold = dx;
        if (!(ENDS_INSIDE ? un >= ulo && un <= uhi : un > ulo && un < uhi) || fabs(2.0 * f) > fabs(dxold * df)) {
            dx = 0.5 * (uhi - ulo);
            u = ulo + dx;
        } else {
            dx = un - u;
            u = un;
        }
        if (fabs(dx) <= NB_FIT_TOL) { converged = true; break; }
        score(u, f, df);
    }
    return converged ? steps : NB_FIT_MAX_STEPS;
}

template <typename T>
__global__ void __launch_bounds__(256) nb_check_kernel(const T *__restrict__ Y, long long ld, long long m, int n_genes, nb_u64 *bad) {
    const long long total = m * (long long)n_genes;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long i = t / n_genes;
        const int j = (int)(t - i * n_genes);
        const double v = (double)Y[i * ld + j];
        if (!(__builtin_isfinite(v) && rint(v) >= 0.0)) atomicMin(bad, ((nb_u64)(unsigned)j << 32) | (nb_u64)i);
    }
}

// Grid: n_genes workgroups of one wave.  Dynamic LDS: (2 m + k) doubles.  log_prior_mean: nullable (no prior term).
// A gene of zeros, or one whose prior mean is not finite, gets NaN in log_disp and objective.
template <typename T>
__global__ void __launch_bounds__(64) nb_dispersion_kernel(const T *__restrict__ Y, long long ld, int m, int k, const int *__restrict__ order,
                                                            const int *__restrict__ gof, const double *__restrict__ ss,
                                                            const int *__restrict__ gstart, const double *__restrict__ log_prior_mean,
                                                            double prior_var, double *__restrict__ log_disp, double *__restrict__ objective,
                                                            double *__restrict__ fitted_mean) {
    extern __shared__ double nb_lds[];
    double *sc = nb_lds, *smu = sc + m, *smean = smu + m;
    const int gene = blockIdx.x, lane = threadIdx.x;

    int any = 0;
    for (int p = lane; p < m; p += 64) {
        const double c = rint((double)Y[(long long)order[p] * ld + gene]);
        sc[p] = c;
        smu[p] = c / ss[p];
        any |= c > 0.0;
    }
    any = lanes_reduce(any, Max{});
    __syncthreads();
    for (int g = lane; g < k; g += 64) {
        const int a = gstart[g], b = gstart[g + 1];
        double sum = 0.0;
        for (int p = a; p < b; ++p) sum += smu[p];
        const double mean = sum / (double)(b - a);
        smean[g] = mean;
        if (fitted_mean) fitted_mean[(long long)gene * k + g] = mean;
    }
    __syncthreads();
    for (int p = lane; p < m; p += 64) {
        const double mu = ss[p] * smean[gof[p]];
        smu[p] = mu > NB_MIN_MU ? mu : NB_MIN_MU;
    }
    __syncthreads();

    const double lpm = log_prior_mean ? log_prior_mean[gene] : 0.0;
    if (!any || !__builtin_isfinite(lpm)) {
        if (lane == 0) log_disp[gene] = objective[gene] = __builtin_nan("");
        return;
    }
    const double half_inv_var = log_prior_mean ? 0.5 / prior_var : 0.0;
    double x = 0.0, L = 0.0;
    nb_grid_rounds(log(NB_MIN_DISP), log(nb_max_disp(m)), lane, [&](int, double at) {
        x = at;
        const double alpha = exp(x), r = 1.0 / alpha, lg_r = lgamma(r);
        L = 0.0;
        int p = 0;
        for (int g = 0; g < k; ++g) {
            const int end = gstart[g + 1];
            double sw = 0.0, Lg = 0.0;
            for (; p < end; ++p) {
                const double c = sc[p], mu = smu[p], am = alpha * mu, l1p = log1p(am);
                if (c > 0.0) Lg += lgamma(c + r) - lg_r - (c + r) * l1p + c * log(am);
                else Lg -= r * l1p;
                sw += mu / (1.0 + am);
            }
            L += Lg - 0.5 * log(sw);                 // a group's part is closed on its own: two groups may swap codes, bit for bit
        }
        if (log_prior_mean) L -= (x - lpm) * (x - lpm) * half_inv_var;
        return L;
    }, [&](int round, int b) {
        if (round == NB_ROUNDS - 1 && lane == b) { log_disp[gene] = x; objective[gene] = L; }
    });
}

// f(q) and q f'(q) of one group: its samples are the sorted positions a .. b - 1
template <typename T>
__device__ inline void nb_score(const T *__restrict__ Y, long long ld, int gene, const int *__restrict__ order, const double *__restrict__ ss,
                                int a, int b, double alpha, double q, double &f, double &qdf) {
    double sf = 0.0, sd = 0.0;
    for (int p = a; p < b; ++p) {
        const double c = rint((double)Y[(long long)order[p] * ld + gene]), sq = ss[p] * q, den = 1.0 + alpha * sq;
        sf += (c - sq) / den;
        sd += sq * (1.0 + alpha * c) / (den * den);
    }
    f = sf;
    qdf = -sd;
}

// Grid: ceil(n_genes * k / 256) workgroups; thread t: gene t % n_genes, group t / n_genes.  q, w: n_genes x k.  A NaN dispersion
// leaves its gene out (q = w = NaN, steps = flags = 0).
template <typename T>
__global__ void __launch_bounds__(256) nb_group_fit_kernel(const T *__restrict__ Y, long long ld, int n_genes, int k,
                                                           const int *__restrict__ order, const double *__restrict__ ss,
                                                           const int *__restrict__ gstart, const double *__restrict__ dispersion,
                                                           double *__restrict__ q_out, double *__restrict__ w_out, int *__restrict__ steps_out,
                                                           int *__restrict__ flags_out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n_genes * k) return;
    const int g = (int)(t / n_genes), gene = (int)(t - (long long)g * n_genes);
    const long long at = (long long)gene * k + g;
    const double alpha = dispersion[gene];
    if (alpha != alpha) {
        q_out[at] = w_out[at] = __builtin_nan("");
        steps_out[at] = flags_out[at] = 0;
        return;
    }
    const int a = gstart[g], b = gstart[g + 1];
    double qmin = __builtin_inf(), qmax = 0.0, sum_c = 0.0, sum_s = 0.0, smax = 0.0;
    for (int p = a; p < b; ++p) {
        const double c = rint((double)Y[(long long)order[p] * ld + gene]), s = ss[p], qp = c / s;
        qmin = qp < qmin ? qp : qmin;
        qmax = qp > qmax ? qp : qmax;
        smax = s > smax ? s : smax;
        sum_c += c;
        sum_s += s;
    }
    double q = qmax;
    int steps = 0, flags = 0;
    if (qmax > qmin) {
        // the root lies in [max(qmin, sum c / (sum s (1 + alpha smax qmax))), qmax]: f >= 0 at the lower end, f <= 0 at the upper
        const double lower = sum_c / (sum_s * (1.0 + alpha * smax * qmax));
        double ulo = log(qmin > lower ? qmin : lower), uhi = log(qmax);
        double u = log(sum_c / sum_s);
        u = u < ulo ? ulo : (u > uhi ? uhi : u);
        bool done;
        steps = nb_bracketed_root<false>(ulo, uhi, u, done, [&](double at, double &f, double &qdf) {
            nb_score(Y, ld, gene, order, ss, a, b, alpha, exp(at), f, qdf);
        });
        if (!done) flags |= NB_FLAG_NOT_CONVERGED;
        q = exp(u);
    }
    const double floor_q = NB_MIN_MU / smax;
    if (q < floor_q) { q = floor_q; flags |= NB_FLAG_FLOORED; }
    double w = 0.0;
    for (int p = a; p < b; ++p) {
        double mu = ss[p] * q;
        mu = mu > NB_MIN_MU ? mu : NB_MIN_MU;
        w += mu / (1.0 + alpha * mu);
    }
    q_out[at] = q;
    w_out[at] = w;
    steps_out[at] = steps;
    flags_out[at] = flags;
}

}  // namespace pilot
