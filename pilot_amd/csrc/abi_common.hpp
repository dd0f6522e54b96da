// Shared by the translation units that implement the C ABI: error reporting, test switches, the per-thread pool of device
// temporaries and the device limits every launch decision reads.  Host-side only.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pilot_ot.h"
#include "sinkhorn_layout.hpp"     // LDS_BYTES

#define PILOT_API extern "C" __attribute__((visibility("default")))

namespace pilot {

// record the calling thread's error message (pilot_ot_last_error) and return `code`
int abi_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// value of a test switch (pilot_ot_test_switch), or nullptr: how the GPU tests and the A/B tools force a kernel variant.  The
// library reads NO environment variable that changes what it computes.
const char *test_switch(const char *name);
// release every cached multi-GPU context of the host-buffer entry points (called by pilot_ot_shutdown)
void abi_multi_release();

// The calling thread's pool of device temporaries: one buffer per slot, grown on demand, released by pilot_ot_shutdown.  Every
// buffer of every translation unit has a slot of its own here, so two buffers that are live together (diffmap chains into the
// consumer entry points) never share one.
enum WsSlot {
    WS_PREPASS_X, WS_PREPASS,                                                   // pilot_ot_prepass.hip
    WS_COST_X, WS_COST_C, WS_COST_AUX,                                          // pilot_ot_cost.hip
    WS_CONS_E, WS_CONS_D, WS_CONS_MAX, WS_CONS_LABELS, WS_CONS_SIZES, WS_CONS_SCORES, WS_CONS_K,   // pilot_ot_consumers.hip
    WS_PLAN_P, WS_PLAN_M, WS_PLAN_PI, WS_PLAN_PJ, WS_PLAN_VAL, WS_PLAN_IT, WS_PLAN_FL, WS_PLAN_Q,    // pilot_ot_plans.hip
    WS_PLAN_PLANS, WS_PLAN_SLAB, WS_PLAN_ROWMIN, WS_PLAN_KWS, WS_PLAN_ACC, WS_PLAN_GOFF, WS_PLAN_GIDX,
    WS_DM_S, WS_DM_V, WS_DM_VEC, WS_DM_Z, WS_DM_PSI, WS_DM_E, WS_DM_D, WS_DM_K, WS_DM_MAX, WS_DM_OUT,  // pilot_ot_diffmap.hip
    WS_TF_U, WS_TF_Y, WS_TF_OUT, WS_TF_COLS,                                    // pilot_ot_trajfit.hip
    WS_BOOT_U, WS_BOOT_OUT, WS_BOOT_IDX, WS_BOOT_Y,                             // pilot_ot_bootfit.hip
    WS_CV_Y, WS_CV_IN, WS_CV_AUX, WS_CV_OUT, WS_CV_BMAX, WS_CV_CHAIN, WS_CV_Z,   // pilot_ot_curves.hip
    WS_GM_Y, WS_GM_AUX, WS_GM_PART, WS_GM_COUNT, WS_GM_OUT,                      // pilot_ot_moments.hip
    WS_CSR_COUNTS, WS_CSR_TOTAL, WS_CSR_CODES, WS_CSR_COLS, WS_CSR_OUT,          // pilot_ot_csr.hip
    WS_GS_Y, WS_GS_AUX, WS_GS_PART, WS_GS_OUT,                                   // pilot_ot_group_sums.hip
    WS_PCA_V, WS_PCA_VEC, WS_PCA_Z, WS_PCA_PCS, WS_PCA_SCORES, WS_PCA_STATS, WS_PCA_COLS, WS_PCA_POS,   // pilot_ot_pca.hip
    WS_PCA_SIDX, WS_PCA_SVAL, WS_PCA_CSVAL, WS_PCA_Y, WS_PCA_S, WS_PCA_PARTW,
    WS_KNN_X, WS_KNN_UNIT, WS_KNN_FLAGS, WS_KNN_BEST_D, WS_KNN_BEST_I, WS_KNN_OUT_D, WS_KNN_OUT_I, WS_KNN_SM_IN, WS_KNN_SM_OUT,   // pilot_ot_knn.hip
    WS_LV_VAL0, WS_LV_VAL1, WS_LV_DEG0, WS_LV_DEG1, WS_LV_IDX0, WS_LV_IDX1, WS_LV_TOT, WS_LV_SUMS, WS_LV_INT, WS_LV_FLAG, WS_LV_ECOMM,   // pilot_ot_louvain.hip
    WS_LV_NKEYS, WS_LV_EKEYS, WS_LV_CNT, WS_LD_INT, WS_LD_DBL,                   // (WS_LD_*: the refinement of pilot_ot_leiden)
    WS_SIL_X, WS_SIL_UNIT, WS_SIL_FLAGS, WS_SIL_SORTED, WS_SIL_ORDER, WS_SIL_OFFSETS, WS_SIL_OUT,   // pilot_ot_silhouette_points.hip
    WS_PT_X, WS_PT_FLAGS, WS_PT_Y, WS_PT_YT, WS_PT_S, WS_PT_CENTRE, WS_PT_STATE, WS_PT_ITERS, WS_PT_ENERGY, WS_PT_COUNTS, WS_PT_SUMS,   // pilot_ot_principal_tree.hip
    WS_PT_PCOUNTS, WS_PT_PSUMS, WS_PT_PMSE, WS_PT_PART, WS_PT_OUT,
    WS_RS_Y, WS_RS_INT, WS_RS_LL, WS_RS_REC, WS_RS_OUT,                          // pilot_ot_rank_sums.hip
    WS_NB_Y, WS_NB_INT, WS_NB_SF, WS_NB_BAD, WS_NB_PRIOR, WS_NB_OUT, WS_NB_FIT_INT,   // pilot_ot_nb_glm.hip
    WS_SLOTS
};
hipError_t ws_buffer(WsSlot slot, size_t bytes, void **out);
// n elements of T (at least one) from `slot`
template <typename T> hipError_t ws(WsSlot slot, size_t n, T **out) {
    void *p = nullptr;
    const hipError_t e = ws_buffer(slot, sizeof(T) * (n ? n : 1), &p);
    *out = static_cast<T *>(p);
    return e;
}

// ---- dense matrix arguments: what every entry point that takes a row-major matrix (dtype code, columns, leading dimension, an
// optional column selection; on the host or in HBM) checks and stages.  The checks make no HIP call.
inline size_t elem_size(int dtype) { return dtype == 0 ? sizeof(float) : sizeof(double); }
int check_dtype(int dtype);
int check_ld(long long ld, int n_cols);
// a selection of n_sel columns out of n_cols: every cols[j] in range; without cols the selection is all of them
int check_cols(const int *cols, int n_sel, int n_cols);
// `rows` x `n_cols` elements of `es` bytes at Y, leading dimension ld, as a device pointer: Y and ld themselves when Y is in HBM,
// else a packed copy (leading dimension n_cols) in `slot`.  Chunked callers pass each chunk's first element and row count.
int stage_dense(const void *Y, int is_device, size_t es, long long rows, long long n_cols, long long ld, WsSlot slot, const void **ptr,
                long long *ld_out);
// the same for a whole packed float64 matrix of `count` elements
int stage_f64(const double *src, int is_device, size_t count, WsSlot slot, const double **out);

// device time of the calling thread's last pre-pass (pilot_ot_prepass_device_ms): two events on the launch stream
struct PrepassClock {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool valid = false;
    void release() { for (auto &e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; } valid = false; }
    void start() {
        valid = false;
        if (!ev[0] && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)) { release(); return; }
        (void)hipEventRecord(ev[0], nullptr);
    }
    void stop() { if (ev[1]) valid = hipEventRecord(ev[1], nullptr) == hipSuccess; }
};
PrepassClock &thread_clock();

// compute units of the current device (256 if the runtime cannot tell)
int cu_count();
// blocks of `block` threads for n items, at most 8 per CU
inline int grid_for(long n, int block, int n_cu) {
    long g = (n + block - 1) / block;
    const long cap = (long)n_cu * 8;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

constexpr int MAX_K = 128;          // the MFMA pair-grid kernels (8 row-tiles of 16 cell types)
constexpr int GENERIC_MAX_K = 2048;  // the reference-semantics fallback kernel (vectors in LDS)
constexpr int EMD_MAX_K = 256;       // exact-OT kernel: 4 rows / columns per lane
constexpr int WIDE_MAX_K = 256;      // sinkhorn_wide_kernel: 128 < K <= 256, eight waves per 16-pair tile

// the kNN kernel sorts a row in LDS, padded to the next power of two: 16384 doubles = 128 KiB is the largest that fits.  Every
// entry point that reaches the kernel asks this first, the host forms before they stage their N x N buffers.
inline int knn_rows_supported(int N) {
    return N <= PILOT_OT_KNN_MAX_N ? PILOT_OT_OK
                                   : abi_fail(PILOT_OT_ENOTSUP, "N=%d rows do not fit the LDS sort (at most %d)", N, PILOT_OT_KNN_MAX_N);
}

// cell-level cohort, internal face used by the multi-device form (pilot_ot_multi.hip)
int cell_enqueue_rows(pilot_ot_cell_cohort *c, double scale, double reg, int num_iter_max, double stop_thr, int check_period,
                      double f32_floor_ulps, int row_begin, int row_end, int row_step, size_t *n_out);
int cell_collect(pilot_ot_cell_cohort *c, size_t n_out, double *w2 /* nullable */, int *iters, double *err, float *kernel_ms);
void cell_buffers(pilot_ot_cell_cohort *c, double **d_w2, hipStream_t *stream);

}  // namespace pilot

#define fail(...) pilot::abi_fail(__VA_ARGS__)

#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return pilot::abi_fail(PILOT_OT_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                   __FILE__, __LINE__);                                                    \
    } while (0)
