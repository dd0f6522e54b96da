// C ABI of the diffusion map (include/pilot_ot.h, section "diffusion map"; kernels: diffmap_kernels.hpp).  The eigen-part of
// pl.trajectory (pilotpy/plot/ploting.py:109-110) on the device: symmetrised, alpha-normalised kNN kernel -> symmetric Lanczos with
// full re-orthogonalisation -> Ritz vectors -> pydiffmap's diffusion coordinates.  The tridiagonal Ritz problem is solved here on
// the host (implicit QL), so the entry points synchronise their stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "abi_common.hpp"
#include "diffmap_kernels.hpp"
#include "lanczos_host.hpp"

namespace {

constexpr int MAX_BASIS = pilot::LZ_MAX_BASIS, MAX_EVECS = pilot::LZ_MAX_EVECS;
constexpr double BREAKDOWN_TOL = pilot::LZ_BREAKDOWN_TOL;
constexpr double DEGENERATE_MU = 1.0 - 1e-10;
using pilot::order_desc;
using pilot::tridiag_ql;

int check_args(int N, double epsilon, double alpha, int n_evecs) {
    if (N < 2) return fail(PILOT_OT_EINVAL, "N=%d: a diffusion map needs at least 2 points", N);
    const int cap = std::min(N - 1, MAX_EVECS);
    if (n_evecs < 1 || n_evecs > cap) return fail(PILOT_OT_EINVAL, "n_evecs=%d outside [1, min(N - 1, %d)] = [1, %d]", n_evecs, MAX_EVECS, cap);
    if (!(epsilon > 0.0) || !std::isfinite(epsilon)) return fail(PILOT_OT_EINVAL, "epsilon=%g must be positive and finite", epsilon);
    if (!std::isfinite(alpha)) return fail(PILOT_OT_EINVAL, "alpha=%g must be finite", alpha);
    return PILOT_OT_OK;
}

}  // namespace

PILOT_API int pilot_ot_diffusion_map_dev(const double *d_K, int N, double epsilon, double alpha, int n_evecs, double *d_dmap,
                                         double *d_evecs, double *d_evals, int *info, void *stream) {
    if (!d_K || !d_dmap || !d_evals || !info) return fail(PILOT_OT_EINVAL, "NULL pointer");
    int rc = check_args(N, epsilon, alpha, n_evecs);
    if (rc != PILOT_OT_OK) return rc;
    info[0] = 0;
    info[1] = 0;
    const int m = n_evecs + 1;                                 // wanted Ritz pairs: the trivial mu = 1 and n_evecs more
    int B = std::min(N, MAX_BASIS);
    if (const char *sw = pilot::test_switch("PILOT_OT_DIFFMAP_BASIS")) {      // (tests: a basis too small to converge)
        const int b = atoi(sw);
        if (b > 0 && b < B) B = b;
    }
    B = std::max(B, m);
    hipStream_t s = static_cast<hipStream_t>(stream);

    double *S, *V, *vec, *Zs, *psi;
    HIP_TRY(pilot::ws(pilot::WS_DM_S, (size_t)N * N, &S));
    HIP_TRY(pilot::ws(pilot::WS_DM_V, (size_t)B * N, &V));
    HIP_TRY(pilot::ws(pilot::WS_DM_VEC, 5 * (size_t)N + 4 * (size_t)B + 1, &vec));
    HIP_TRY(pilot::ws(pilot::WS_DM_Z, (size_t)B * n_evecs + n_evecs, &Zs));
    HIP_TRY(pilot::ws(pilot::WS_DM_PSI, (size_t)N * n_evecs, &psi));
    double *w = vec, *qa = w + N, *wsc = qa + N, *dis = wsc + N, *phi = dis + N;
    double *h1 = phi + N, *h2 = h1 + B, *al = h2 + B, *be = al + B;
    int *n_restart = reinterpret_cast<int *>(be + B);

    // S from K (K itself is only read)
    const unsigned tg = (unsigned)((N + pilot::DM_TILE - 1) / pilot::DM_TILE);
    hipLaunchKernelGGL(pilot::dm_symmetrize_kernel, dim3(tg, tg), dim3(pilot::DM_TILE, 8), 0, s, d_K, N, S);
    hipLaunchKernelGGL(pilot::dm_row_kernel, dim3(N), dim3(pilot::DM_RED), 0, s, S, N, 0, alpha, qa, wsc, dis, phi);
    hipLaunchKernelGGL(pilot::dm_row_kernel, dim3(N), dim3(pilot::DM_RED), 0, s, S, N, 1, alpha, qa, wsc, dis, phi);
    const size_t nn = (size_t)N * N;
    const unsigned sb = (unsigned)std::min<size_t>((nn + 255) / 256, 4096);
    hipLaunchKernelGGL(pilot::dm_scale_kernel, dim3(sb), dim3(256), 0, s, S, N, wsc);
    hipLaunchKernelGGL(pilot::lz_start_kernel, dim3(1), dim3(pilot::DM_FIN), 0, s, phi, N, V);
    HIP_TRY(hipMemsetAsync(n_restart, 0, sizeof(int), s));
    HIP_TRY(hipGetLastError());

    // Lanczos (lanczos_run: the steps, the look at T every LZ_CHECK_EVERY steps from step m on, and the acceptance rule).  Step 0
    // always breaks down (V[0] is an eigenvector); converged wanted pairs only begin the verification block, whose steps are not
    // part of the result unless it found something and the basis went on to become complete.
    pilot::LanczosSpec spec;
    spec.N = N;
    spec.B = B;
    spec.want = m;
    spec.breakdown = BREAKDOWN_TOL;
    spec.norm = 1.0;                                           // |S| = 1
    spec.floor_rel = 0.0;
    spec.start_is_eigenvector = true;
    pilot::LanczosRun run;
    HIP_TRY(pilot::lanczos_run(spec, V, w, h1, h2, al, be, n_restart, s, [&](const double *vj, double *wj) {
        hipLaunchKernelGGL(pilot::lz_gemv_kernel, dim3((N + 3) / 4), dim3(256), 0, s, S, N, vj, wj);
    }, &run));
    const std::vector<double> &ha = run.ha, &hb = run.hb;
    const int steps = run.steps;
    const bool converged = run.converged;
    std::vector<double> d, e, z;

    // the Ritz pairs of the final basis: eigenvectors of T as columns
    const int nk = run.nk;
    d.assign(ha.begin(), ha.begin() + nk);
    e.assign(hb.begin(), hb.begin() + nk);
    z.assign((size_t)nk * nk, 0.0);
    for (int k = 0; k < nk; ++k) z[(size_t)k * nk + k] = 1.0;
    if (!tridiag_ql(nk, d.data(), e.data(), z.data(), nk)) return fail(PILOT_OT_EHIP, "tridiagonal QL did not converge (%d steps)", nk);
    const std::vector<int> ix = order_desc(d);
    int n_one = 0;
    for (int k = 0; k < nk; ++k) n_one += d[k] >= DEGENERATE_MU;
    std::vector<double> zs((size_t)nk * n_evecs + n_evecs);
    for (int c = 0; c < n_evecs; ++c) {                        // drop the first (mu = 1, lambda = 0): pydiffmap's evecs[:, 1:]
        const int col = ix[c + 1];
        for (int k = 0; k < nk; ++k) zs[(size_t)k * n_evecs + c] = z[(size_t)k * nk + col];
        zs[(size_t)nk * n_evecs + c] = (d[col] - 1.0) / epsilon;      // lambda of L = (P - I) / epsilon
    }
    double *lam_dev = Zs + (size_t)nk * n_evecs;                   // (Z: nk x n_evecs, then the n_evecs lambdas)
    HIP_TRY(hipMemcpyAsync(Zs, zs.data(), sizeof(double) * zs.size(), hipMemcpyHostToDevice, s));
    const long nt = (long)N * n_evecs;
    hipLaunchKernelGGL(pilot::lz_ritz_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, V, N, nk, Zs, n_evecs, dis, psi);
    hipLaunchKernelGGL(pilot::dm_finalize_kernel, dim3(n_evecs), dim3(pilot::DM_RED), 0, s, psi, N, n_evecs, lam_dev, d_dmap, d_evecs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(d_evals, lam_dev, sizeof(double) * n_evecs, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    info[0] = steps;
    info[1] = (converged ? 0 : PILOT_OT_DIFFMAP_NOT_CONVERGED) | (n_one > 1 ? PILOT_OT_DIFFMAP_DEGENERATE : 0);
    return PILOT_OT_OK;
}

// pl.trajectory's embedding from E (ploting.py:95-110): E / max(E) -> Euclidean row distances -> k-nn Gaussian kernel (K7) -> the
// diffusion map above.  E on the host or (E_is_device) already in HBM; dmap / evecs (nullable) / evals / info on the host.
PILOT_API int pilot_ot_diffusion_map_of_rows(const double *E, int E_is_device, int N, int k, double epsilon, double alpha, int n_evecs,
                                             double *dmap, double *evecs, double *evals, int *info) {
    if (!E || !dmap || !evals || !info) return fail(PILOT_OT_EINVAL, "NULL pointer");
    int rc = check_args(N, epsilon, alpha, n_evecs);
    if (rc != PILOT_OT_OK) return rc;
    if (k < 1) return fail(PILOT_OT_EINVAL, "k=%d must be positive", k);
    if ((rc = pilot::knn_rows_supported(N)) != PILOT_OT_OK) return rc;
    const size_t nn = (size_t)N * N, no = (size_t)N * n_evecs;
    const double *dE;
    double *dD, *dK, *dM, *dOut;
    HIP_TRY(pilot::ws(pilot::WS_DM_D, nn, &dD));
    HIP_TRY(pilot::ws(pilot::WS_DM_K, nn, &dK));
    HIP_TRY(pilot::ws(pilot::WS_DM_MAX, 1, &dM));
    HIP_TRY(pilot::ws(pilot::WS_DM_OUT, 2 * no + n_evecs, &dOut));
    rc = pilot::stage_f64(E, E_is_device, nn, pilot::WS_DM_E, &dE);
    if (rc == PILOT_OT_OK) rc = pilot_ot_row_distances_dev(dE, N, 1, PILOT_OT_ROWMETRIC_EUCLIDEAN, dD, dM, nullptr);
    if (rc == PILOT_OT_OK) rc = pilot_ot_knn_kernel_dev(dD, N, k, epsilon, dK, nullptr);
    if (rc == PILOT_OT_OK) rc = pilot_ot_diffusion_map_dev(dK, N, epsilon, alpha, n_evecs, dOut, dOut + no, dOut + 2 * no, info, nullptr);
    if (rc != PILOT_OT_OK) return rc;
    HIP_TRY(hipMemcpy(dmap, dOut, sizeof(double) * no, hipMemcpyDeviceToHost));
    if (evecs) HIP_TRY(hipMemcpy(evecs, dOut + no, sizeof(double) * no, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(evals, dOut + 2 * no, sizeof(double) * n_evecs, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}
