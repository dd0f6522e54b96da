// K10: batched bootstrap Huber fits (pilotpy's gene_cluster_differentiation, Gene_cluster_specific.py: 50 HuberRegressor fits
// per side of every (gene, cell type) row).  A problem is one target column y of a shared n x T matrix Y, one trajectory model
// (linear / linear_quadratic / quadratic, as in K9) and B resampled index vectors; fit b regresses y (in its own order) on the
// gathered times x[idx_b] -- only x is resampled, as the reference does.  Every fit goes to the optimum of scikit-learn's
// HuberRegressor objective with K9's method: the same basis, penalty, Newton direction, bracketing line search, stop rule and
// step cap (trajfit_kernels.hpp; its device functions are used as they are).
//
// Layout: one lane per bootstrap (a lane group of 64 per blockIdx.y), one workgroup per problem (blockIdx.x), TF_WAVES waves
// splitting the observations into fixed slices.  y[i] is the same for every lane (a broadcast load); the lane's time is
// u[idx[i][b]] (idx observation-major: 64 lanes read 64 consecutive ints).  Partials meet in LDS in wave order (tf_reduce):
// no value atomics, so results are bit-identical whatever the route or chunking.
//
// Conditioning: every resampled time is a base time, so the host maps the BASE x to u = (x - m) / s once (|u| <= 1 for every
// resample) and passes K9's per-model basis, back-transform R and penalty; the Gram of each resample is formed here.  A resample
// can have fewer distinct times than the model has coefficients: the start then solves the penalised normal equations
// (B^T B + pen) gamma = B^T y, which are positive definite (pen is positive definite on w, the intercept sees n > 0), and the
// Newton steps carry the same penalty, so the fit is the unique penalised optimum rather than a refusal or NaN.
#pragma once
#include "trajfit_kernels.hpp"

namespace pilot {

constexpr int BF_NOUT = 6;                        // doubles per (problem, bootstrap): params[3], sigma, steps, flags
constexpr int BF_O_PARAMS = 0, BF_O_SIGMA = 3, BF_O_STEPS = 4, BF_O_FLAGS = 5;

// One launch per chunk of problems.  Y: n rows of `ld` elements; u: the n mapped base times; idx: the chunk's problems, n x B
// ints each (observation-major); cols / models: per problem of the chunk; out: BF_NOUT doubles per (problem, bootstrap).
template <typename T>
__global__ void __launch_bounds__(TF_BLOCK) bootfit_kernel(const T *__restrict__ Y, long long ld, const double *__restrict__ u,
                                                           const int *__restrict__ idx, const int *__restrict__ cols,
                                                           const int *__restrict__ models, int B, const TrajfitArgs *__restrict__ args,
                                                           double *__restrict__ out) {
    const TrajfitArgs &a = *args;
    __shared__ double lds[TF_WAVES][TF_NACC][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int prob = blockIdx.x;
    const int b = blockIdx.y * 64 + lane;
    const bool valid = b < B;
    const int n = a.n, m = models[prob], p = tf_p(m), k = p + 1;
    const long long i0 = (long long)n * wave / TF_WAVES, i1 = (long long)n * (wave + 1) / TF_WAVES;
    const T *col = Y + cols[prob];
    const int *ix = idx + (long long)prob * n * B + (valid ? b : 0);
    auto yat = [&](long long i) -> double { return (double)col[i * ld]; };
    auto uat = [&](long long i) -> double { return u[ix[i * B]]; };

    // pass 1: the resample's Gram of the basis, B^T y, sum y^2, values different from the first
    double part[TF_NACC], tot[TF_NACC];
    const double y0 = yat(0);
    {
        for (int q = 0; q < 11; ++q) part[q] = 0.0;
        for (long long i = i0; i < i1; ++i) {
            const double y = yat(i);
            double bs[3];
            tf_basis(a, m, uat(i), bs);
            part[0] += bs[0] * bs[0]; part[1] += bs[0] * bs[1]; part[2] += bs[0] * bs[2];
            part[3] += bs[1] * bs[1]; part[4] += bs[1] * bs[2]; part[5] += bs[2] * bs[2];
            part[6] += bs[0] * y; part[7] += bs[1] * y; part[8] += bs[2] * y;
            part[9] += y * y;
            part[10] += y != y0 ? 1.0 : 0.0;
        }
        tf_reduce(lds, part, tot, 11, wave, lane);
    }
    const int pk[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    const double syy = tot[9];
    const bool constant = tot[10] == 0.0;

    double cg[3] = {0.0, 0.0, 0.0}, cs;
    bool done = !valid;
    if (constant) {                               // the optimum: the constant itself, sigma at its bound (as K9)
        cg[0] = y0;
        cs = a.sigma_min;
        done = true;
    } else {                                      // start: the penalised least-squares fit, sigma = its rms residual
        double G[4][4] = {}, r[3];
        for (int i = 0; i < p; ++i) {
            for (int j = 0; j < p; ++j) G[i][j] = tot[pk[i][j]] + a.mod[m].pen[i][j];
            r[i] = tot[6 + i];
        }
        tf_spd_solve(G, r, cg, p);
        double sse = syy;
        for (int i = 0; i < p; ++i) {
            sse -= 2.0 * cg[i] * r[i];
            for (int j = 0; j < p; ++j) sse += cg[i] * tot[pk[i][j]] * cg[j];
        }
        cs = fmax(sse > 1e-8 * syy ? sqrt(fmax(sse, 0.0) / n) : sqrt(syy / n), a.sigma_min);
    }

    // Newton steps with a bracketing line search: trajfit_kernel's Huber loop, the basis at the lane's resampled time (a copy, kept
    // identical to it: as one shared function the loop compiles to other FMA fusions and the fits' last bits move)
    double cF = 0.0, d[4] = {0.0, 0.0, 0.0, 0.0}, s0 = 0.0, t = 0.0, tmax = 0.0, lo = 0.0, flo = 0.0, hi = -1.0, fhi = 0.0;
    double bt = 0.0, bF = 0.0, bg[4] = {}, bH[4][4] = {};
    bool start = true, have_best = false;
    int it = 0, fl = 0, evals = 0;
    while (__any(!done)) {
        const double es = start ? cs : fmax(cs + t * d[p], a.sigma_min);
        double eg[3];
        for (int i = 0; i < 3; ++i) eg[i] = start ? cg[i] : cg[i] + t * d[i];
        double S[TF_NACC];
        for (int q = 0; q < TF_NACC; ++q) S[q] = 0.0;
        if (!done) {
            const double thr = a.epsilon * es;
            for (long long i = i0; i < i1; ++i) {
                double bs[3];
                tf_basis(a, m, uat(i), bs);
                const double r = yat(i) - (eg[0] * bs[0] + eg[1] * bs[1] + eg[2] * bs[2]);
                if (fabs(r) <= thr) {
                    S[0] += r * r;
                    S[1] += r * bs[0]; S[2] += r * bs[1]; S[3] += r * bs[2];
                    S[4] += bs[0] * bs[0]; S[5] += bs[0] * bs[1]; S[6] += bs[0] * bs[2];
                    S[7] += bs[1] * bs[1]; S[8] += bs[1] * bs[2]; S[9] += bs[2] * bs[2];
                } else {
                    const double sg = r > 0.0 ? 1.0 : -1.0;
                    S[10] += fabs(r);
                    S[11] += sg * bs[0]; S[12] += sg * bs[1]; S[13] += sg * bs[2];
                    S[14] += 1.0;
                }
            }
        }
        double St[TF_NACC];
        tf_reduce(lds, S, St, TF_NACC, wave, lane);
        if (done) continue;
        double F, g[4], H[4][4];
        tf_huber_eval(a, m, eg, es, St, F, g, H);
        bool accept = start;
        if (!start) {                                 // line search: bracket the zero of phi'(t) = g . d
            double st = 0.0;
            for (int i = 0; i < k; ++i) st += g[i] * d[i];
            ++evals;
            if (F <= cF && fabs(st) <= 0.1 * fabs(s0)) {
                have_best = true; bt = t; bF = F;
                for (int i = 0; i < 4; ++i) { bg[i] = g[i]; for (int j = 0; j < 4; ++j) bH[i][j] = H[i][j]; }
            } else {
                bool finish = evals >= TF_LS_EVALS;
                if (st < 0.0) {
                    if (F <= cF) {
                        have_best = true; bt = t; bF = F;
                        for (int i = 0; i < 4; ++i) { bg[i] = g[i]; for (int j = 0; j < 4; ++j) bH[i][j] = H[i][j]; }
                    }
                    lo = t; flo = st;
                    if (hi < 0.0) {
                        if (t >= tmax) finish = true;
                        else if (!finish) { t = fmin(4.0 * t, tmax); continue; }
                    }
                } else {
                    hi = t; fhi = st;
                }
                if (!finish) {
                    t = lo + (hi - lo) * fmin(fmax(-flo / (fhi - flo), 0.05), 0.95);
                    continue;
                }
                if (!have_best) { done = true; continue; }       // no lower objective in floating point: at the optimum
            }
            for (int i = 0; i < p; ++i) cg[i] += bt * d[i];
            cs = fmax(cs + bt * d[p], a.sigma_min);
            F = bF;
            for (int i = 0; i < 4; ++i) { g[i] = bg[i]; for (int j = 0; j < 4; ++j) H[i][j] = bH[i][j]; }
            accept = true;
        }
        if (accept) {
            start = false;
            cF = F;
            const bool bound = cs <= a.sigma_min && g[p] > 0.0;     // sigma held at its bound: projected gradient
            if (bound) {
                g[p] = 0.0;
                for (int i = 0; i < k; ++i) H[i][p] = H[p][i] = 0.0;
                H[p][p] = 1.0;
            }
            double gn = 0.0;
            for (int i = 0; i < k; ++i) gn += fabs(g[i]);
            if (gn * cs <= TF_HUBER_TOL * fabs(F)) { done = true; continue; }          // the optimality test
            if (it >= a.max_iter) { done = true; fl = TF_FLAG_NOT_CONVERGED; continue; }
            ++it;
            double mg[4];
            for (int i = 0; i < k; ++i) mg[i] = -g[i];
            tf_spd_solve(H, mg, d, k);
            if (bound) d[p] = 0.0;
            s0 = 0.0;
            for (int i = 0; i < k; ++i) s0 += g[i] * d[i];
            if (!(s0 < 0.0)) {                                      // (not a descent direction: steepest descent)
                for (int i = 0; i < k; ++i) d[i] = -g[i];
                s0 = 0.0;
                for (int i = 0; i < k; ++i) s0 -= g[i] * g[i];
            }
            for (int i = k; i < 4; ++i) d[i] = 0.0;
            tmax = d[p] < 0.0 ? (cs - a.sigma_min) / -d[p] : INFINITY;
            t = fmin(1.0, tmax);
            lo = 0.0; flo = s0; hi = -1.0; evals = 0; have_best = false;
        }
    }
    if (wave != 0 || !valid) return;
    double *o = out + ((long long)prob * B + b) * BF_NOUT;
    for (int j = 0; j < 3; ++j)
        o[BF_O_PARAMS + j] = j < p ? a.mod[m].R[j][0] * cg[0] + a.mod[m].R[j][1] * cg[1] + a.mod[m].R[j][2] * cg[2] : NAN;
    o[BF_O_SIGMA] = cs;
    o[BF_O_STEPS] = it;
    o[BF_O_FLAGS] = fl;
}

}  // namespace pilot
