// K4 / K5: the device pre-pass (C ABI: proportions, the resident embedding, centroid medians, the whole pre-pass;
// include/pilot_ot.h).  Kernels: prepass_kernels.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "abi_common.hpp"
#include "prepass_kernels.hpp"

// pre-pass (host-buffer entry points; the inputs are read once, so they are staged per call)
namespace {
// ---- the device pre-pass, carved out of ONE pooled workspace (WS_PREPASS of the calling thread's pool) --------------------
// head (cleared by one memset): counts N*K | first_row N | n_k K | cursor K | n_items 1 | global histograms K*D*2*256
// then: prior K | P N*K | segment starts K | select items | select state | centroids K*D | codes | grouped keys
inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
struct PrepassWs {
    // what the caller asks for
    bool want_counts = false, want_medians = false;
    long long C = 0; int N = 0, K = 0, D = 0, n_cu = 256; size_t key_bytes = 4;
    int n_code_cols = 1;
    // derived
    long R = 0, max_items = 0;
    size_t o_counts = 0, o_first = 0, o_nk = 0, o_cursor = 0, o_nitems = 0, o_hist = 0, clear_bytes = 0, o_prior = 0, o_P = 0, o_offs = 0,
           o_items = 0, o_st = 0, o_out = 0, o_code = 0, o_y = 0, total = 0;
    void carve() {
        size_t o = 0;
        auto take = [&](size_t bytes) { const size_t at = o; o += al256(bytes); return at; };
        o_counts = take(want_counts ? sizeof(unsigned int) * (size_t)N * K : 0);
        o_first = take(want_counts ? sizeof(unsigned int) * (size_t)N : 0);
        o_nk = take(sizeof(unsigned int) * K);
        o_cursor = take(sizeof(unsigned int) * K);
        o_nitems = take(sizeof(unsigned int));
        if (want_medians) {
            // rows per select item (the unit the passes are balanced in; a block takes a run of items): 256, more only to
            // keep the list below 64 K items; a multiple of 4
            R = 256;
            if (C / R > 65536) R = (long)(((C / 65536) + 3) & ~3LL);
            max_items = (long)(C / R) + K + 1;
            o_hist = take(sizeof(unsigned int) * (size_t)K * D * 2 * 256);
        } else {
            o_hist = o;
        }
        clear_bytes = o;
        o_prior = take(want_counts ? sizeof(double) * (size_t)K : 0);
        o_P = take(want_counts ? sizeof(double) * (size_t)N * K : 0);
        o_offs = take(sizeof(unsigned int) * K);
        o_items = take(want_medians ? sizeof(pilot::SelectItem) * (size_t)max_items : 0);
        o_st = take(want_medians ? (key_bytes + 8) * (size_t)K * D * 2 : 0);
        o_out = take(want_medians ? sizeof(double) * (size_t)K * D : 0);
        o_code = take(sizeof(int) * (size_t)C * n_code_cols);
        o_y = take(want_medians ? key_bytes * ((size_t)C + 4 * (size_t)K) * D : 0);
        total = o;
    }
};

// counts + first rows + n_k from device-resident codes, then the proportions: three launches
void launch_counts(const PrepassWs &ws, unsigned char *w, const int *d_cell, const int *d_sample, long long n_total, double regulizer,
                   int normalization, bool want_first) {
    const long nchunks = (long)((ws.C + pilot::COUNT_CHUNK - 1) / pilot::COUNT_CHUNK);
    long grid = 4L * ws.n_cu;
    if (grid > nchunks) grid = nchunks;
    if (grid < 1) grid = 1;
    unsigned int *counts = reinterpret_cast<unsigned int *>(w + ws.o_counts);
    const size_t lds = sizeof(unsigned int) * ((size_t)pilot::COUNT_LDS_BINS + pilot::COUNT_LDS_ROWS + ws.K + 16);
    hipLaunchKernelGGL(pilot::count_kernel, dim3((unsigned)grid), dim3(256), lds, nullptr, d_cell, d_sample, (long)ws.C, ws.N, ws.K, counts,
                       reinterpret_cast<unsigned int *>(w + ws.o_nk), want_first ? reinterpret_cast<unsigned int *>(w + ws.o_first) : nullptr);
    hipLaunchKernelGGL(pilot::prior_kernel, dim3((unsigned)((ws.K + 3) / 4)), dim3(256), 0, nullptr, counts, ws.N, ws.K, (long)n_total, regulizer,
                       reinterpret_cast<double *>(w + ws.o_prior));
    hipLaunchKernelGGL(pilot::proportions_kernel, dim3((unsigned)((ws.N + 3) / 4)), dim3(256), 0, nullptr, counts, ws.N, ws.K,
                       reinterpret_cast<const double *>(w + ws.o_prior), normalization, reinterpret_cast<double *>(w + ws.o_P));
}

// the general median path (prepass_kernels.hpp): [count,] prep, group the rows by type, BITS/8 x (histogram, pick)
template <typename T>
int launch_medians(const PrepassWs &ws, unsigned char *w, const T *dXp, const int *d_cell, bool have_nk) {
    using U = typename pilot::OrderedKey<T>::U;
    using State = pilot::SelectState<U>;
    static_assert(sizeof(State) <= sizeof(U) + 8, "select state larger than its carve");
    const int K = ws.K, D = ws.D;
    const long long C = ws.C;
    unsigned int *d_nk = reinterpret_cast<unsigned int *>(w + ws.o_nk), *d_cursor = reinterpret_cast<unsigned int *>(w + ws.o_cursor),
                 *d_nitems = reinterpret_cast<unsigned int *>(w + ws.o_nitems), *d_hist = reinterpret_cast<unsigned int *>(w + ws.o_hist),
                 *d_offs = reinterpret_cast<unsigned int *>(w + ws.o_offs);
    pilot::SelectItem *d_items = reinterpret_cast<pilot::SelectItem *>(w + ws.o_items);
    State *d_st = reinterpret_cast<State *>(w + ws.o_st);
    double *d_out = reinterpret_cast<double *>(w + ws.o_out);
    U *d_y = reinterpret_cast<U *>(w + ws.o_y);
    const long nb = (long)((C + pilot::GROUP_ROWS_PER_BLOCK - 1) / pilot::GROUP_ROWS_PER_BLOCK);
    if (!have_nk) {
        long g = 2L * ws.n_cu;
        if (g > nb) g = nb;
        hipLaunchKernelGGL(pilot::type_count_kernel, dim3((unsigned)g), dim3(256), sizeof(unsigned int) * K, nullptr, d_cell, (long)C, K, d_nk);
    }
    hipLaunchKernelGGL(pilot::median_prep_kernel, dim3(1), dim3(256), sizeof(unsigned int) * (2 * (size_t)K + 2 + 257), nullptr, d_nk, K,
                       (unsigned int)ws.R, d_offs, d_nitems, d_items);
    hipLaunchKernelGGL(pilot::group_rows_kernel<T>, dim3((unsigned)nb), dim3(256),
                       sizeof(unsigned int) * (2 * (size_t)K + pilot::GROUP_ROWS_PER_BLOCK), nullptr, dXp, D, d_cell, (long)C, K, d_offs, d_cursor, d_y);
    const int Dw_max = D < pilot::SELECT_MAX_DIMS ? D : pilot::SELECT_MAX_DIMS;      // dimensions per histogram launch
    const size_t lds = sizeof(U) * 2 * (size_t)Dw_max + sizeof(unsigned int) * (size_t)Dw_max * 2 * 256;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pilot::select_hist_kernel<T>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // as many histogram blocks as the chip holds at once (LDS-bound), each with an equal run of the work list
    long hist_grid = (long)ws.n_cu * (long)((160 * 1024) / (lds + 256) < (size_t)(2048 / pilot::SELECT_THREADS) ? (160 * 1024) / (lds + 256)
                                                                                                                 : (size_t)(2048 / pilot::SELECT_THREADS));
    if (hist_grid > ws.max_items) hist_grid = ws.max_items;
    if (hist_grid < 1) hist_grid = 1;
    const unsigned pick_blocks = (unsigned)(((size_t)K * D * 64 + 255) / 256);
    for (int shift = pilot::OrderedKey<T>::BITS - 8; shift >= 0; shift -= 8) {
        for (int dbeg = 0; dbeg < D; dbeg += Dw_max) {           // any D: the dimensions in windows that fit the LDS histograms
            const int Dw = D - dbeg < Dw_max ? D - dbeg : Dw_max;
            hipLaunchKernelGGL(pilot::select_hist_kernel<T>, dim3((unsigned)hist_grid), dim3(pilot::SELECT_THREADS),
                               sizeof(U) * 2 * (size_t)Dw + sizeof(unsigned int) * (size_t)Dw * 2 * 256, nullptr, d_y, D, dbeg, Dw,
                               d_nitems, d_items, shift, d_st, d_hist);
        }
        hipLaunchKernelGGL(pilot::select_pick_kernel<T>, dim3(pick_blocks), dim3(256), 0, nullptr, d_nk, K, D, shift, d_st, d_hist, d_out);
    }
    HIP_TRY(hipGetLastError());
    return PILOT_OT_OK;
}

// small cohorts: one launch, the selection in LDS (small_medians_kernel) -- when every type fits its key buffer and the
// K x D workgroups reading all C codes is a small amount of traffic (PILOT_OT_NO_SMALL_MEDIANS=1: the general path, tests)
bool small_medians_fit(long long C, int D, const int *cell_code, int K, unsigned int *n_max_out) {
    if (!(C > 0 && (double)C * K * D <= 3.2e7) || pilot::test_switch("PILOT_OT_NO_SMALL_MEDIANS")) return false;
    std::vector<unsigned int> n_k((size_t)K, 0u);
    for (long long c = 0; c < C; ++c) { const int k = cell_code[c]; if (k >= 0 && k < K) ++n_k[(size_t)k]; }
    unsigned int n_max = 0;
    for (unsigned int v : n_k) n_max = v > n_max ? v : n_max;
    *n_max_out = n_max;
    return n_max <= (unsigned int)pilot::SMALL_MEDIANS_CAP;
}
template <typename T>
int launch_small_medians(const T *dXp, long long C, int D, const int *d_cell, int K, unsigned int n_max, double *d_out) {
    using U = typename pilot::OrderedKey<T>::U;
    const size_t lds = sizeof(U) * (size_t)(n_max ? n_max : 1);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pilot::small_medians_kernel<T>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(U) * pilot::SMALL_MEDIANS_CAP)));
    hipLaunchKernelGGL(pilot::small_medians_kernel<T>, dim3((unsigned)(K * D)), dim3(256), lds, nullptr, dXp, D, d_cell, (long)C, K, d_out);
    HIP_TRY(hipGetLastError());
    return PILOT_OT_OK;
}
}  // namespace

PILOT_API int pilot_ot_proportions(const int *cell_code, const int *sample_code, long long n_cells, long long n_total,
                                   int N, int K, double regulizer, int normalization, double *P) {
    return pilot_ot_proportions_ex(cell_code, sample_code, n_cells, n_total, N, K, regulizer, normalization, P, nullptr);
}

PILOT_API int pilot_ot_proportions_ex(const int *cell_code, const int *sample_code, long long n_cells, long long n_total,
                                      int N, int K, double regulizer, int normalization, double *P, long long *first_row) {
    if (!cell_code || !sample_code || !P) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (first_row && n_cells > 0xfffffffeLL) return fail(PILOT_OT_ENOTSUP, "n_cells=%lld exceeds the 32-bit row index", n_cells);
    if (N <= 0 || K <= 0 || n_cells < 0 || n_total < 2)
        return fail(PILOT_OT_EINVAL, "N=%d K=%d n_cells=%lld n_total=%lld out of range", N, K, n_cells, n_total);
    if (K > 4096) return fail(PILOT_OT_ENOTSUP, "K=%d > 4096 cell types", K);
    PrepassWs ws;
    ws.want_counts = true; ws.C = n_cells; ws.N = N; ws.K = K; ws.n_cu = pilot::cu_count(); ws.n_code_cols = 2;
    ws.carve();
    unsigned char *w = nullptr;
    hipError_t e = pilot::ws(pilot::WS_PREPASS, ws.total, &w);
    int *d_cell = reinterpret_cast<int *>(w + ws.o_code), *d_sample = d_cell + n_cells;
    if (e == hipSuccess) e = hipMemcpy(d_cell, cell_code, sizeof(int) * (size_t)n_cells, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_sample, sample_code, sizeof(int) * (size_t)n_cells, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemsetAsync(w, 0, ws.clear_bytes, nullptr);
    if (e != hipSuccess) return fail(PILOT_OT_EHIP, "device staging failed: %s", hipGetErrorString(e));
    launch_counts(ws, w, d_cell, d_sample, n_total, regulizer, normalization, first_row != nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(P, w + ws.o_P, sizeof(double) * (size_t)N * K, hipMemcpyDeviceToHost));
    if (first_row) {
        std::vector<unsigned int> fr((size_t)N);
        HIP_TRY(hipMemcpy(fr.data(), w + ws.o_first, sizeof(unsigned int) * (size_t)N, hipMemcpyDeviceToHost));
        for (int n = 0; n < N; ++n) first_row[n] = fr[(size_t)n] == 0u ? -1 : (long long)(0xffffffffu - fr[(size_t)n]);
    }
    return PILOT_OT_OK;
}

// the embedding resident on the device: uploaded once (from a helper thread of the host language, beside its own work on
// the label columns), read by pilot_ot_centroid_medians_dev / pilot_ot_prepass_dev
struct pilot_ot_embedding {
    void *dX = nullptr;
    int dtype = 0, D = 0, device = 0;
    long long C = 0;
};

PILOT_API int pilot_ot_embedding_upload(const void *X, int dtype, long long n_cells, int D, pilot_ot_embedding **emb) {
    if (!X || !emb) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (n_cells <= 0 || D <= 0) return fail(PILOT_OT_EINVAL, "n_cells=%lld D=%d must be positive", n_cells, D);
    if (dtype != PILOT_OT_F32 && dtype != PILOT_OT_F64) return fail(PILOT_OT_EINVAL, "unknown dtype id %d", dtype);
    pilot_ot_embedding *e = new (std::nothrow) pilot_ot_embedding();
    if (!e) return fail(PILOT_OT_EINVAL, "out of host memory");
    e->dtype = dtype; e->D = D; e->C = n_cells;
    const size_t bytes = (size_t)n_cells * D * (dtype == PILOT_OT_F32 ? 4 : 8);
    hipError_t he = hipGetDevice(&e->device);
    if (he == hipSuccess) he = hipMalloc(&e->dX, bytes);
    if (he == hipSuccess) he = hipMemcpy(e->dX, X, bytes, hipMemcpyHostToDevice);
    if (he != hipSuccess) { pilot_ot_embedding_destroy(e); return fail(PILOT_OT_EHIP, "embedding upload failed: %s", hipGetErrorString(he)); }
    *emb = e;
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_embedding_destroy(pilot_ot_embedding *e) {
    if (!e) return PILOT_OT_OK;
    if (e->dX) (void)hipFree(e->dX);
    delete e;
    return PILOT_OT_OK;
}

namespace {
// dXdev (nullable): the embedding already on the device; else X is copied in
template <typename T>
int centroid_medians_impl(const void *X, const void *dXdev, long long C, int D, const int *cell_code, int K, double *centroids) {
    unsigned int n_max = 0;
    const bool small = small_medians_fit(C, D, cell_code, K, &n_max);
    PrepassWs ws;
    ws.want_medians = !small; ws.C = C; ws.K = K; ws.D = D; ws.n_cu = pilot::cu_count(); ws.key_bytes = sizeof(T);
    ws.carve();
    T *dX = nullptr;
    unsigned char *w = nullptr;
    hipError_t e = dXdev ? hipSuccess : pilot::ws(pilot::WS_PREPASS_X, (size_t)C * D, &dX);
    if (e == hipSuccess) e = pilot::ws(pilot::WS_PREPASS, ws.total + al256(sizeof(double) * (size_t)K * D), &w);
    if (e != hipSuccess) return fail(PILOT_OT_EHIP, "device staging failed: %s", hipGetErrorString(e));
    int *d_cell = reinterpret_cast<int *>(w + ws.o_code);
    double *d_out = small ? reinterpret_cast<double *>(w + ws.total) : reinterpret_cast<double *>(w + ws.o_out);
    if (!dXdev) e = hipMemcpy(dX, X, sizeof(T) * (size_t)C * D, hipMemcpyHostToDevice);
    const T *dXp = dXdev ? static_cast<const T *>(dXdev) : dX;
    if (e == hipSuccess) e = hipMemcpy(d_cell, cell_code, sizeof(int) * (size_t)C, hipMemcpyHostToDevice);
    if (e == hipSuccess && !small) e = hipMemsetAsync(w, 0, ws.clear_bytes, nullptr);
    if (e != hipSuccess) return fail(PILOT_OT_EHIP, "device staging failed: %s", hipGetErrorString(e));
    pilot::thread_clock().start();
    const int rc = small ? launch_small_medians<T>(dXp, C, D, d_cell, K, n_max, d_out) : launch_medians<T>(ws, w, dXp, d_cell, false);
    pilot::thread_clock().stop();
    if (rc != PILOT_OT_OK) return rc;
    HIP_TRY(hipMemcpy(centroids, d_out, sizeof(double) * (size_t)K * D, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}

// the whole pre-pass from one upload of the two code columns
template <typename T>
int prepass_impl(const pilot_ot_embedding *emb, const int *cell_code, const int *sample_code, long long n_total, int N, int K,
                 double regulizer, int normalization, double *P, long long *first_row, double *centroids) {
    const long long C = emb->C;
    const int D = emb->D;
    unsigned int n_max = 0;
    const bool small = small_medians_fit(C, D, cell_code, K, &n_max);
    PrepassWs ws;
    ws.want_counts = true; ws.want_medians = !small; ws.C = C; ws.N = N; ws.K = K; ws.D = D; ws.n_cu = pilot::cu_count();
    ws.key_bytes = sizeof(T); ws.n_code_cols = 2;
    ws.carve();
    // results leave in one copy: P | centroids | first rows, packed behind the workspace
    const size_t r_P = sizeof(double) * (size_t)N * K, r_cen = sizeof(double) * (size_t)K * D, r_first = sizeof(unsigned int) * (size_t)N;
    unsigned char *w = nullptr;
    hipError_t e = pilot::ws(pilot::WS_PREPASS, ws.total + al256(r_P + r_cen + r_first), &w);
    if (e != hipSuccess) return fail(PILOT_OT_EHIP, "device staging failed: %s", hipGetErrorString(e));
    unsigned char *res = w + ws.total;
    int *d_cell = reinterpret_cast<int *>(w + ws.o_code), *d_sample = d_cell + C;
    e = hipMemcpy(d_cell, cell_code, sizeof(int) * (size_t)C, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_sample, sample_code, sizeof(int) * (size_t)C, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemsetAsync(w, 0, ws.clear_bytes, nullptr);
    if (e != hipSuccess) return fail(PILOT_OT_EHIP, "device staging failed: %s", hipGetErrorString(e));
    pilot::thread_clock().start();
    launch_counts(ws, w, d_cell, d_sample, n_total, regulizer, normalization, true);
    const T *dXp = static_cast<const T *>(emb->dX);
    double *d_cen = reinterpret_cast<double *>(res + r_P);
    int rc = small ? launch_small_medians<T>(dXp, C, D, d_cell, K, n_max, d_cen) : launch_medians<T>(ws, w, dXp, d_cell, true);
    pilot::thread_clock().stop();
    if (rc != PILOT_OT_OK) return rc;
    hipError_t he = hipMemcpyAsync(res, w + ws.o_P, r_P, hipMemcpyDeviceToDevice, nullptr);
    if (he == hipSuccess && !small) he = hipMemcpyAsync(d_cen, w + ws.o_out, r_cen, hipMemcpyDeviceToDevice, nullptr);
    if (he == hipSuccess) he = hipMemcpyAsync(res + r_P + r_cen, w + ws.o_first, r_first, hipMemcpyDeviceToDevice, nullptr);
    std::vector<unsigned char> host(r_P + r_cen + r_first);
    if (he == hipSuccess) he = hipMemcpy(host.data(), res, host.size(), hipMemcpyDeviceToHost);
    if (he != hipSuccess) return fail(PILOT_OT_EHIP, "pre-pass results: %s", hipGetErrorString(he));
    memcpy(P, host.data(), r_P);
    memcpy(centroids, host.data() + r_P, r_cen);
    const unsigned int *fr = reinterpret_cast<const unsigned int *>(host.data() + r_P + r_cen);
    if (first_row) for (int n = 0; n < N; ++n) first_row[n] = fr[n] == 0u ? -1 : (long long)(0xffffffffu - fr[n]);
    return PILOT_OT_OK;
}
}  // namespace

PILOT_API int pilot_ot_centroid_medians(const void *X, int dtype, long long n_cells, int D, const int *cell_code, int K,
                                        double *centroids) {
    if (!X || !cell_code || !centroids) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (n_cells <= 0 || D <= 0 || K <= 0) return fail(PILOT_OT_EINVAL, "n_cells=%lld D=%d K=%d must be positive", n_cells, D, K);
    if (n_cells > 0xfffffffeLL) return fail(PILOT_OT_ENOTSUP, "n_cells=%lld exceeds the 32-bit row index", n_cells);
    if (K > 4096) return fail(PILOT_OT_ENOTSUP, "K=%d > 4096 cell types", K);
    if (dtype == PILOT_OT_F32) return centroid_medians_impl<float>(X, nullptr, n_cells, D, cell_code, K, centroids);
    if (dtype == PILOT_OT_F64) return centroid_medians_impl<double>(X, nullptr, n_cells, D, cell_code, K, centroids);
    return fail(PILOT_OT_EINVAL, "unknown dtype id %d", dtype);
}

PILOT_API int pilot_ot_centroid_medians_dev(pilot_ot_embedding *e, const int *cell_code, int K, double *centroids) {
    if (!e || !cell_code || !centroids) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (K <= 0) return fail(PILOT_OT_EINVAL, "K=%d must be positive", K);
    if (K > 4096) return fail(PILOT_OT_ENOTSUP, "K=%d > 4096 cell types", K);
    if (e->C > 0xfffffffeLL) return fail(PILOT_OT_ENOTSUP, "n_cells=%lld exceeds the 32-bit row index", e->C);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != e->device) return fail(PILOT_OT_EINVAL, "the embedding lives on device %d, the current device is %d", e->device, dev);
    if (e->dtype == PILOT_OT_F32) return centroid_medians_impl<float>(nullptr, e->dX, e->C, e->D, cell_code, K, centroids);
    return centroid_medians_impl<double>(nullptr, e->dX, e->C, e->D, cell_code, K, centroids);
}

PILOT_API int pilot_ot_prepass_device_ms(float *ms) {
    if (!ms) return fail(PILOT_OT_EINVAL, "NULL pointer");
    pilot::PrepassClock &c = pilot::thread_clock();
    if (!c.valid) return fail(PILOT_OT_EINVAL, "no pre-pass has run on this thread");
    HIP_TRY(hipEventSynchronize(c.ev[1]));
    HIP_TRY(hipEventElapsedTime(ms, c.ev[0], c.ev[1]));
    return PILOT_OT_OK;
}

PILOT_API int pilot_ot_prepass_dev(pilot_ot_embedding *e, const int *cell_code, const int *sample_code, long long n_total, int N, int K,
                                   double regulizer, int normalization, double *P, long long *first_row, double *centroids) {
    if (!e || !cell_code || !sample_code || !P || !centroids) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (N <= 0 || K <= 0 || n_total < 2) return fail(PILOT_OT_EINVAL, "N=%d K=%d n_total=%lld out of range", N, K, n_total);
    if (K > 4096) return fail(PILOT_OT_ENOTSUP, "K=%d > 4096 cell types", K);
    if (e->C > 0xfffffffeLL) return fail(PILOT_OT_ENOTSUP, "n_cells=%lld exceeds the 32-bit row index", e->C);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != e->device) return fail(PILOT_OT_EINVAL, "the embedding lives on device %d, the current device is %d", e->device, dev);
    if (e->dtype == PILOT_OT_F32) return prepass_impl<float>(e, cell_code, sample_code, n_total, N, K, regulizer, normalization, P, first_row, centroids);
    return prepass_impl<double>(e, cell_code, sample_code, n_total, N, K, regulizer, normalization, P, first_row, centroids);
}
