/*
 * pilot_ot.h -- C ABI of libpilot_ot.so, the MI355X (gfx950) pairwise-Wasserstein engine.
 *
 * Drop-in boundary.  The reference (CostaLab/PILOT, pilotpy 2.0.6) has no FFI layer: the hot
 * path sits behind two Python call signatures,
 *     wasserstein_d(Clu_rep, cost, regularized, reg)   pilotpy/tools/Trajectory.py:479-523
 *     cost_matrix(annot, data, metric)                 pilotpy/tools/Trajectory.py:441-475
 * whose inner arithmetic is one POT call per ordered sample pair
 *     ot.sinkhorn2(a, b, M, reg, method="sinkhorn_stabilized")     Trajectory.py:515
 *     ot.emd2(a, b, M)                                             Trajectory.py:511
 * and one scipy call  pdist(centroids, metric) + squareform        Trajectory.py:468-469.
 * The entry points below are what a ctypes binding for that path binds (INTEGRATION.md shows
 * the binding).  Plain pointers and sizes only; no torch / numpy types.
 *
 * Conventions
 *   - every function returns PILOT_OT_OK (0) or a negative PILOT_OT_E* code; the message of the
 *     last failure on the calling thread is pilot_ot_last_error().  No exceptions cross the ABI.
 *   - "host" entry points take caller-owned host buffers, copy in/out internally and retain no
 *     pointer to them after returning (device workspace is cached per thread: pilot_ot_shutdown).  "_dev" entry points take device pointers (hipMalloc'ed by the
 *     caller or by pilot_ot_dev_alloc) and enqueue on the given hipStream_t without synchronising.
 *   - there is NO CPU implementation behind this ABI: without a gfx950 device every compute entry
 *     point fails with PILOT_OT_EHIP.
 *   - matrices are row-major; P is N x K (one proportion vector per sample, rows sum to 1,
 *     Trajectory.py:428-430); M is K x K, already divided by its max (Trajectory.py:101).
 *   - rows of the pair grid are selected as row_begin, row_begin+row_step, ... < row_end; every
 *     selected row is paired with ALL N columns (diagonal included, no symmetry shortcut,
 *     Trajectory.py:508-515).  Outputs hold n_rows x N values, n_rows = ceil((row_end-row_begin)/row_step).
 */
#ifndef PILOT_OT_H
#define PILOT_OT_H

#ifdef __cplusplus
extern "C" {
#endif

#define PILOT_OT_VERSION 100 /* 0.1.0 */

/* return codes */
#define PILOT_OT_OK 0
#define PILOT_OT_EINVAL (-1)  /* bad argument                                              */
#define PILOT_OT_EHIP (-2)    /* HIP runtime error / no gfx950 device                      */
#define PILOT_OT_ENOTSUP (-3) /* shape outside what the kernels support (K > 2048, ...) */
#define PILOT_OT_ERCCL (-4)   /* RCCL error / librccl missing (multi-GPU entry points only) */

/* precision of the Sinkhorn pair-grid kernel */
#define PILOT_OT_MAX_COST_OVER_REG 600.0 /* beyond it exp(-M/reg) leaves the f64 range: every entry point runs PREC_GENERIC */
#define PILOT_OT_PREC_AUTO 0 /* F16X2 while max(M)/reg <= 16, BF16X3 (both f32 values) while exp(-max(M)/reg) stays a normal f32
                              * far from underflow (<= 60), else AUTO_MIXED / f64 */
#define PILOT_OT_PREC_F32 1    /* f32 values, products on the f32-input MFMA (v_mfma_f32_16x16x4_f32): IEEE f32 FMA chains */
#define PILOT_OT_PREC_F64 2
#define PILOT_OT_PREC_AUTO_MIXED 4 /* what AUTO resolves to beyond the f32 range (60 < max(M)/reg <= 140): every pair is iterated in
                                   * f32 (BF16X3 tau-tracking kernel) with the Gibbs kernel held in TWO EXPONENT BANDS (entries
                                   * below 2^-110 are kept times 2^128 in a second operand image, so exp(-M/reg) is faithful down
                                   * to exp(-165)); a pair that still goes NaN / inf is solved again in f64 (PILOT_OT_FLAG_F64
                                   * tells which).  Falls back to F64 where the images do not fit LDS or max(M)/reg > 140. */
#define PILOT_OT_PREC_GENERIC 5 /* reference-semantics fallback: POT's sinkhorn_stabilized loop literally in fp64, one workgroup per
                                * pair, absorbed kernel exp(-(M - alpha - beta)/reg) rebuilt at every tau-absorption.  Taken
                                * automatically when K > 256, when 128 < K <= 256 falls outside the range of the eight-waves-per-tile
                                * kernel (below), or max(M)/reg > 600 (where the fixed Gibbs image of the fast kernels leaves the
                                * f64 range); NaN handling is POT's (revert to the last good iterate). */
#define PILOT_OT_PREC_BF16X3 3 /* f32 values, products on v_mfma_f32_16x16x32_bf16 through exact 3-way bf16 operand splits
                                * (six piece products per term, f32 accumulation): f32-level rounding, not bit-identical
                                * to PREC_F32, ~2x its speed */
#define PILOT_OT_PREC_F16X2 6  /* f32 values, products on v_mfma_f32_16x16x32_f16 through 2-way fp16 operand splits (11 + 11
                                * significant bits, three piece products per term) in a fixed scaled domain (2^15 G, 32 u, 32 v):
                                * valid while max(M)/reg <= 16 and tau <= 2000 (PILOT's defaults: reg 0.1 on cost/max, tau 1e3);
                                * outside that range the call runs BF16X3.  Pairs in which POT would tau-absorb are redone by
                                * the BF16X3 tracking kernel.  Same stopping checks as BF16X3 on 99.9 % of the pairs. */

/* per-pair flag bits (flags output) */
#define PILOT_OT_FLAG_CONVERGED 1      /* stopped on err <= stop_thr                              */
#define PILOT_OT_FLAG_NAN 2            /* a scaling became NaN (POT: "Numerical errors"): the pair was re-solved by the
                                        * POT-literal kernel, emd = cost of the last good iterate like POT returns
                                        * (also: histograms with empty bins that reach a tau-absorption, where POT's
                                        * log(0) leads to 0/0 one update later; and pairs of unequal mass whose total
                                        * scalings leave the exact range of the fast kernels) */
#define PILOT_OT_FLAG_ABSORB_LAST 4    /* POT tau-absorption fell on the final update (plan /K^2)   */
#define PILOT_OT_FLAG_ABSORBED 8       /* at least one POT tau-absorption happened                  */
#define PILOT_OT_FLAG_F64 16           /* pair was solved by the f64 kernel                         */

/* ground metrics of pilot_ot_cost_matrix (scipy.spatial.distance.pdist names, Trajectory.py:468) */
#define PILOT_OT_METRIC_COSINE 0
#define PILOT_OT_METRIC_EUCLIDEAN 1
#define PILOT_OT_METRIC_SQEUCLIDEAN 2
#define PILOT_OT_METRIC_CITYBLOCK 3
#define PILOT_OT_METRIC_CHEBYSHEV 4
#define PILOT_OT_METRIC_CORRELATION 5
#define PILOT_OT_METRIC_MINKOWSKI 6   /* p = 2, scipy's default (the reference forwards only the metric name) */
#define PILOT_OT_METRIC_SEUCLIDEAN 7  /* V = per-dimension variance of the centroids, ddof = 1 (scipy's default) */
#define PILOT_OT_METRIC_BRAYCURTIS 8
#define PILOT_OT_METRIC_CANBERRA 9
#define PILOT_OT_METRIC_HAMMING 10
/* scipy's boolean dissimilarities (pdist converts the rows to bool: non-zero = True) and the rest of scipy 1.15's pdist names */
#define PILOT_OT_METRIC_JACCARD 11
#define PILOT_OT_METRIC_DICE 12           /* (evaluated on the values, like scipy: ntt = sum u v, ...) */
#define PILOT_OT_METRIC_YULE 13
#define PILOT_OT_METRIC_RUSSELLRAO 14
#define PILOT_OT_METRIC_SOKALSNEATH 15
#define PILOT_OT_METRIC_ROGERSTANIMOTO 16
#define PILOT_OT_METRIC_SOKALMICHENER 17
#define PILOT_OT_METRIC_KULCZYNSKI1 18
#define PILOT_OT_METRIC_JENSENSHANNON 19
#define PILOT_OT_METRIC_MAHALANOBIS 20    /* needs aux = VI, the D x D inverse covariance (cost_matrix_ex) */

/* ---- library / device --------------------------------------------------------------------- */
int pilot_ot_version(void);
const char *pilot_ot_last_error(void);
int pilot_ot_device_count(int *count);            /* number of visible HIP devices (0 is not an error) */
int pilot_ot_set_device(int device);              /* device used by the calling thread's later calls   */
int pilot_ot_get_device(int *device);             /* the calling thread's current device (a new host thread starts on device 0) */
int pilot_ot_device_name(char *buf, int buflen);  /* gcnArchName of the current device                 */
int pilot_ot_shutdown(void);                      /* free the calling thread's cached host-API workspace */

/* TEST HOOK, not part of the drop-in surface: forces a kernel variant or an out-of-range configuration for the GPU tests and the
 * A/B tools (names as the tests use them, e.g. "PILOT_OT_NO_SMALL_MEDIANS", "PILOT_OT_RAW_PRECISION"); some settings return results
 * OUTSIDE the stated tolerance -- that is what they are for.  Process-wide; value NULL clears one switch, name NULL clears all.
 * The library reads no environment variable that changes what it computes. */
int pilot_ot_test_switch(const char *name, const char *value);

/* TEST HOOK: the workspace guard.  Every device temporary of the feature entry points comes from the calling thread's pool, one
 * buffer per slot.  With the test switch "PILOT_OT_WS_GUARD" set to "1" every hand-out synchronises the device, fills the bytes
 * requested with 0xFF (float and double NaN, int -1), keeps at least 256 bytes of slack behind them filled with the canary 0xA5,
 * and first verifies the canary of the slot's previous hand-out; a result that changes under the guard read scratch nobody wrote,
 * a damaged canary is an access past the request.  The value "selftest" also damages the canary byte at offset 7 of the first
 * slot handed out (the control of the check itself).  Unset, the pool makes no extra HIP call. */
int pilot_ot_ws_slot_count(void);              /* number of slots; no HIP call */
const char *pilot_ot_ws_slot_name(int slot);   /* "WS_GS_PART", ...; NULL out of range; no HIP call */
/* checks every slot's canary now; seen (nullable, slot_count bytes): 1 where the slot was handed out under guard since the last
 * reset; bad_slot = -1 when intact, else the damaged slot, the first damaged offset past the request and the request's size;
 * reset != 0 clears seen and the damage record afterwards */
int pilot_ot_ws_guard_report(unsigned char *seen, int *bad_slot, long long *bad_offset, long long *bad_request, int reset);

/* thin device-memory helpers so a host language without a HIP binding can keep data resident */
int pilot_ot_dev_alloc(void **dptr, unsigned long long bytes);
int pilot_ot_dev_free(void *dptr);
int pilot_ot_memcpy_h2d(void *dst, const void *src, unsigned long long bytes);
int pilot_ot_memcpy_d2h(void *dst, const void *src, unsigned long long bytes);
int pilot_ot_stream_sync(void *stream);

/* ---- label columns -> codes (host only, no device work) -------------------------------------- */
/* Numbers the n labels of one column in order of first appearance: what annot.cell_type.unique() /
 * annot.sampleID.unique() plus one boolean mask per label amount to (Trajectory.py:402-425).
 * ids: the labels as fixed-width integers: id_bytes = 1, 2, 4 -- signed, negative = missing (the codes of a pandas
 *      Categorical, what AnnData stores for obs labels); id_bytes = 8 -- opaque 64-bit identities, 0 = missing (the object
 *      pointers of an object column: a cohort's 1.8 M labels are a few hundred distinct Python objects).
 * codes: n int32 out, -1 for missing; first_rows[j]: row where code j first appears (max_uniques entries);
 * *n_uniques: how many codes.  More than max_uniques distinct labels -> PILOT_OT_ENOTSUP.
 * n_threads >= 1 host threads share the pass (slices side by side, their first-appearance lists merged in order). */
int pilot_ot_label_codes(const void *ids, int id_bytes, long long n, int max_uniques, int n_threads, int *codes,
                         long long *first_rows, int *n_uniques);

/* ---- pre-pass: replaces the pandas loops of Cluster_Representations and cost_matrix ---------- */
/* cell_code / sample_code: per cell, index of its cell type / sample in FIRST-APPEARANCE order
 * (what Series.unique() yields, Trajectory.py:402,412); negative codes (missing values) are skipped.
 * n_total = len(df) (the prior's denominator is n_total - 1, Trajectory.py:407).
 * P: N x K fp64, bit-identical to the reference's dict values (every fp64 operation in the same order). */
int pilot_ot_proportions(const int *cell_code, const int *sample_code, long long n_cells, long long n_total,
                         int N, int K, double regulizer, int normalization, double *P);
/* first_row (nullable, N entries): additionally the smallest row number of every sample (-1: no row), i.e. the row whose
 * status return_real_labels reports (Trajectory.py:617-642) -- one more atomic in the same pass over the codes. */
int pilot_ot_proportions_ex(const int *cell_code, const int *sample_code, long long n_cells, long long n_total,
                            int N, int K, double regulizer, int normalization, double *P, long long *first_row);
/* Per-cell-type column-wise median of the n_cells x D embedding X (Trajectory.py:465-466), exact.
 * dtype: 0 = float32, 1 = float64 (the median of an even count is averaged in that dtype, like
 * numpy/pandas, then widened).  centroids: K x D fp64; a cell type without cells yields NaN. */
#define PILOT_OT_F32 0
#define PILOT_OT_F64 1
int pilot_ot_centroid_medians(const void *X, int dtype, long long n_cells, int D, const int *cell_code, int K,
                              double *centroids);
/* The same with the embedding already resident: pilot_ot_embedding_upload copies the C x D array to the current device
 * (synchronously -- call it from a helper thread to overlap the transfer with host work on the label columns, which is
 * what pilot_amd.tl does); _medians_dev then only moves the codes. */
typedef struct pilot_ot_embedding pilot_ot_embedding;
int pilot_ot_embedding_upload(const void *X, int dtype, long long n_cells, int D, pilot_ot_embedding **emb);
int pilot_ot_embedding_destroy(pilot_ot_embedding *emb);
int pilot_ot_centroid_medians_dev(pilot_ot_embedding *emb, const int *cell_code, int K, double *centroids);
/* The whole device pre-pass of wasserstein_distance from ONE upload of the two code columns (emb->C entries each):
 * proportions P (N x K), first rows (nullable) and centroids (K x D) as the three calls above give them, bit for bit --
 * Cluster_Representations (Trajectory.py:377-436), return_real_labels (:617-642), the medians of cost_matrix (:462-466). */
int pilot_ot_prepass_dev(pilot_ot_embedding *emb, const int *cell_code, const int *sample_code, long long n_total, int N, int K,
                         double regulizer, int normalization, double *P, long long *first_row, double *centroids);
/* Device time (HIP events on the launch stream, first kernel to last; transfers excluded) of the calling thread's last
 * pilot_ot_prepass_dev / pilot_ot_centroid_medians(_dev) call -- what bench.py's `prepass.roofline` is computed from. */
int pilot_ot_prepass_device_ms(float *ms);

/* ---- cost matrix: replaces scipy pdist+squareform at Trajectory.py:468-469 ------------------ */
/* centroids: K x D row-major (per-cell-type medians, Trajectory.py:465-466).  cost: K x K,
 * symmetric, zero diagonal, NOT normalised (the reference stores the raw matrix, :98-99). */
int pilot_ot_cost_matrix(const double *centroids, int K, int D, int metric, double *cost);
int pilot_ot_cost_matrix_dev(const double *d_centroids, int K, int D, int metric, double *d_cost,
                             void *stream);
/* aux: metric-specific extra input, NULL otherwise -- mahalanobis: VI = inv(cov(centroids^T))^T, D x D, which the host
 * computes like scipy does (numpy.linalg.inv) */
int pilot_ot_cost_matrix_ex(const double *centroids, int K, int D, int metric, const double *aux, double *cost);
int pilot_ot_cost_matrix_dev_ex(const double *d_centroids, int K, int D, int metric, const double *d_aux, double *d_cost,
                                void *stream);

/* ---- Sinkhorn pair grid: replaces the loop at Trajectory.py:512-515 ------------------------- */
/* Each pair follows POT 0.9.x sinkhorn_stabilized control flow (v-update then u-update; marginal
 * error ||Gamma^T 1 - b||_2 evaluated when ii % check_period == 0; stop on err <= stop_thr or
 * after num_iter_max updates) and returns <Gamma, M> like ot.sinkhorn2.  POT defaults:
 * num_iter_max=1000, stop_thr=1e-9, tau=1e3, check_period=20.  In f32 the stop threshold is
 * floored at f32_floor_ulps * FLT_EPSILON * ||b||_2 (pass 0 for the default of 8).
 * cost_is_symmetric: 1 if M == M^T exactly (always true for pdist output), 0 otherwise.
 * Range: K <= 128 and max(M)/reg <= 600 run on the one-wave-per-tile MFMA kernels (they keep total scalings against the fixed
 * exp(-M/reg), so the ratio must fit the f64 exponent range).  128 < K <= 256 with a symmetric cost, max(M)/reg <= 16 and
 * tau <= 2000 runs the fp16-split products with a tile's cell types spread over the eight waves of a workgroup (any f32-class
 * precision request, AUTO included; f32 tolerance; PILOT_OT_PREC_F64 / _GENERIC keep the POT-literal kernel).  Larger K
 * (<= 2048), the rest of 128 < K <= 256, or a smaller reg run PILOT_OT_PREC_GENERIC, whatever precision was asked for.  The device-resident form cannot see max(M): it judges the range by the plan's max_cost / reg, which is
 * 1/reg (M divided by its max, Trajectory.py:101) until pilot_ot_plan_set_max_cost says otherwise.
 * emd / iters / err / flags: n_rows x N; iters, err, flags may be NULL. */
int pilot_ot_sinkhorn_grid(const double *P, int N, int K, const double *M, double reg,
                           int num_iter_max, double stop_thr, double tau, int check_period,
                           int precision, double f32_floor_ulps, int cost_is_symmetric,
                           int row_begin, int row_end, int row_step,
                           double *emd, int *iters, double *err, int *flags);

/* Device-resident form.  A plan owns the device workspace for one (N, K) shape so the call itself
 * allocates nothing (HIP-graph capturable) -- with two exceptions, each ONE allocation made by the first call that needs it
 * and kept until pilot_ot_plan_destroy (so make that first call outside a stream capture): the scratch of the POT-literal
 * kernel (PREC_GENERIC, 2 K^2 doubles per resident workgroup), and the flow slab of the exact-OT kernels
 * (pilot_ot_emd_grid_dev: K^2 doubles per resident pair, sized once for every kernel variant of the plan's K). */
typedef struct pilot_ot_plan pilot_ot_plan;
int pilot_ot_plan_create(int N, int K, pilot_ot_plan **plan);
int pilot_ot_plan_destroy(pilot_ot_plan *plan);
/* max(M) of the cost matrix the caller keeps on the device (default 1: the cost divided by its maximum, what
 * Trajectory.py:101 hands to the pair loop).  Every range decision of pilot_ot_sinkhorn_grid_dev -- which precision AUTO
 * means, the fp16-split domain (max(M)/reg <= 16), the hand-over and two-band thresholds, the POT-literal fallback -- is
 * taken on max_cost / reg.  A caller whose M is not normalised MUST set it: with max(M) = 3 and reg = 0.1 the Gibbs entries
 * of the fp16-split images would underflow and the call would return finite but wrong distances. */
int pilot_ot_plan_set_max_cost(pilot_ot_plan *plan, double max_cost);
int pilot_ot_sinkhorn_grid_dev(pilot_ot_plan *plan, const double *d_P, const double *d_M, double reg,
                               int num_iter_max, double stop_thr, double tau, int check_period,
                               int precision, double f32_floor_ulps, int cost_is_symmetric,
                               int row_begin, int row_end, int row_step,
                               double *d_emd, int *d_iters, double *d_err, int *d_flags,
                               void *stream);
/* Per-launch kernel timing (HIP events recorded on the call's own stream, around the main pair-grid
 * kernel and around the tau-tracking kernel).  A ring of the 64 most recent sinkhorn_grid_dev calls is
 * kept; read it after synchronising the stream.  main_ms / track_ms receive up to max_n entries, oldest
 * first; *n_out = entries written.  enable = n > 1 records every n-th call only (the four event records of a call cost a
 * 0.7 ms call about 2 %). */
int pilot_ot_plan_enable_timing(pilot_ot_plan *plan, int enable);
int pilot_ot_plan_kernel_times(pilot_ot_plan *plan, int max_n, float *main_ms, float *track_ms, int *n_out);
/* hipGraph replay for a caller that repeats one sinkhorn_grid_dev call (same buffers and arguments; the CONTENTS of
 * P and M may change): the call's launch sequence (control-block memset, prep, order scatter, pair-grid kernel, tracking
 * kernel, NaN hand-over) is captured on the second identical call and replayed as one graph launch from the third on.
 * Any change of arguments falls back to ordinary launches and re-captures.  Off while kernel timing is enabled. */
int pilot_ot_plan_enable_graph(pilot_ot_plan *plan, int enable);

/* ---- exact OT pair grid: replaces the loop at Trajectory.py:507-511 (the reference default) ---- */
/* Each pair returns the exact transportation-LP optimum, the value ot.emd2(a, b, M) returns
 * (after POT's own pre-step b *= sum(a)/sum(b)).  fp64 throughout.
 * mode: PILOT_OT_EMD_ALL    every selected (row, column) pair is solved;
 *       PILOT_OT_EMD_UPPER  only pairs with column >= row are solved, the rest of emd is left
 *                           untouched (valid when M is symmetric AND all histograms carry the same mass -- emd2 rescales
 *                           b to the mass of a, so the value scales with sum(a): the caller mirrors);
 *       PILOT_OT_EMD_MIRROR like UPPER, then the lower triangle is filled from the upper one on the
 *                           device (requires the full square grid: rows 0..N step 1).
 * n_aug (nullable): augmenting paths used per pair (negative: iteration guard tripped, emd = NaN). */
#define PILOT_OT_EMD_ALL 0
#define PILOT_OT_EMD_UPPER 1
#define PILOT_OT_EMD_MIRROR 2
int pilot_ot_emd_grid(const double *P, int N, int K, const double *M, int mode,
                      int row_begin, int row_end, int row_step, double *emd, int *n_aug);
int pilot_ot_emd_grid_dev(pilot_ot_plan *plan, const double *d_P, const double *d_M, int mode,
                          int row_begin, int row_end, int row_step, double *d_emd, int *d_n_aug,
                          void *stream);

/* fill the strictly-lower triangle of the N x N device matrix from the upper one (what PILOT_OT_EMD_MIRROR runs) */
int pilot_ot_mirror_upper_dev(double *d_emd, int N, void *stream);

/* ---- multi-GPU: the pair grid row-sharded over the GPUs of one node ---------------------------------------------------
 * The N^2 pair problems of Trajectory.py:505-515 are independent given the replicated proportions and cost, so the
 * grid is partitioned, never exchanged: shard s of G solves rows s, s+G, s+2G, ... against all N columns; the only
 * exchange step is ONE all-gather of the row blocks (RCCL over xGMI) followed by a device-side row interleave.  A pair
 * is solved by the same kernel with the same arithmetic whichever shard owns it: the assembled matrix is bit-identical
 * to the single-device one.  librccl is loaded (dlopen) by the first call that needs it.
 *
 * (1) one process drives G devices: pilot_ot_multi_*  (ncclCommInitAll, one plan + one stream per device, grouped
 *     ncclAllGather).  devices[s] is the HIP device of shard s.  gather: PILOT_OT_GATHER_RCCL needs G distinct devices
 *     and leaves the full matrix on EVERY device; PILOT_OT_GATHER_COPY assembles it on the device of shard 0 with
 *     peer copies and also accepts repeated device ids (logical shards on one GPU); PILOT_OT_GATHER_AUTO picks RCCL
 *     when the devices are distinct.  All calls are asynchronous on the shards' own streams until _sync / _fetch; every
 *     shard's launches are enqueued by a host thread of its own (PILOT_OT_MULTI_SERIAL=1: by the calling thread).
 *     _sinkhorn resolves the precision once for all shards from max(M) of the inputs given to _set_inputs. */
#define PILOT_OT_GATHER_AUTO 0
#define PILOT_OT_GATHER_RCCL 1
#define PILOT_OT_GATHER_COPY 2
typedef struct pilot_ot_multi pilot_ot_multi;
int pilot_ot_multi_create(int N, int K, const int *devices, int n_shards, int gather, pilot_ot_multi **m);
int pilot_ot_multi_destroy(pilot_ot_multi *m);
int pilot_ot_multi_set_inputs(pilot_ot_multi *m, const double *P, const double *M);   /* host -> every device */
int pilot_ot_multi_sinkhorn(pilot_ot_multi *m, double reg, int num_iter_max, double stop_thr, double tau,
                            int check_period, int precision, double f32_floor_ulps, int cost_is_symmetric);
int pilot_ot_multi_emd(pilot_ot_multi *m, int cost_is_symmetric);  /* symmetric (and equal masses, see PILOT_OT_EMD_UPPER): columns >= row solved, mirrored after the gather */
int pilot_ot_multi_sync(pilot_ot_multi *m);
/* emd: N x N from the device of shard 0; iters / err / flags (nullable; exact mode: iters = n_aug) are fetched shard by
 * shard and interleaved on the host */
int pilot_ot_multi_fetch(pilot_ot_multi *m, double *emd, int *iters, double *err, int *flags);
int pilot_ot_multi_device_matrix(pilot_ot_multi *m, int shard, double **d_full);      /* the assembled matrix in HBM */
/* HIP-event times of the last call: grid_ms[s] = shard s's kernels; gather_ms = all-gather (or peer copies) + interleave: the
 * smallest per-shard (gather start -> matrix assembled) time, since a shard's collective also waits for its slower peers */
int pilot_ot_multi_times(pilot_ot_multi *m, float *grid_ms, float *gather_ms);
/* what RCCL itself reports for every shard's communicator (ncclCommCount / ncclCommUserRank): n_ranks[s], ranks[s], G entries
 * each; 0 / -1 with the peer-copy gather (no communicator).  A record that says "8 GPUs" can prove RCCL saw 8 ranks. */
int pilot_ot_multi_rccl_info(pilot_ot_multi *m, int *n_ranks, int *ranks);
/* host-buffer forms (context cached per calling thread, released by pilot_ot_shutdown) */
int pilot_ot_sinkhorn_grid_multi(const double *P, int N, int K, const double *M, double reg, int num_iter_max,
                                 double stop_thr, double tau, int check_period, int precision, double f32_floor_ulps,
                                 int cost_is_symmetric, const int *devices, int n_devices, int gather,
                                 double *emd, int *iters, double *err, int *flags);
int pilot_ot_emd_grid_multi(const double *P, int N, int K, const double *M, int cost_is_symmetric,
                            const int *devices, int n_devices, int gather, double *emd, int *n_aug);

/* (2) one process PER device (a launcher starts G of them): every rank calls the single-device *_dev entry points on
 *     its own rows (row_begin = rank, row_step = n_ranks) and assembles the matrix with pilot_ot_comm_all_gather_rows.
 *     Rank 0 creates the id and hands its 128 bytes to the others by whatever means the host language has. */
#define PILOT_OT_UNIQUE_ID_BYTES 128
typedef struct pilot_ot_comm pilot_ot_comm;
int pilot_ot_comm_unique_id(char *uid);                                   /* PILOT_OT_UNIQUE_ID_BYTES bytes out */
int pilot_ot_comm_init_rank(const char *uid, int n_ranks, int rank, pilot_ot_comm **comm);   /* on the current device */
int pilot_ot_comm_destroy(pilot_ot_comm *comm);
int pilot_ot_comm_info(pilot_ot_comm *comm, int *n_ranks, int *rank);     /* ncclCommCount / ncclCommUserRank of this communicator */
/* d_local: n_pad x N row block of this rank (n_pad = ceil(N / n_ranks), unused rows zero); d_stage: n_ranks * n_pad x N
 * scratch; d_full: N x N result on every rank.  Enqueued on `stream`. */
int pilot_ot_comm_all_gather_rows(pilot_ot_comm *comm, const double *d_local, int n_pad, int N, double *d_stage,
                                  double *d_full, void *stream);
int pilot_ot_comm_all_reduce_max(pilot_ot_comm *comm, double *d_vals, int n, void *stream);  /* in place; also the barrier */

/* ---- consumers of the finished matrix: what pilotpy does with adata.uns['EMD'] next, kept on the device ----
 * The ROWS of the N x N matrix are the data points of pl.trajectory's diffusion map (pilotpy/plot/ploting.py:95-110, after
 * EMD / EMD.max()) and of the silhouette scores (Sil_computing, pilotpy/tools/Trajectory.py:592-612; ploting.py:324, :425-431).
 * row_distances: D[i][j] = distance between rows i and j (of E / max(E) when normalize_by_max), Euclidean (scipy cdist) or
 *                cosine (sklearn cosine_distances: clipped to [0, 2], zero diagonal).
 * silhouette:    sklearn.metrics.silhouette_score(D, labels, metric="precomputed"); labels in [0, n_clusters);
 *                samples (nullable, N) receives silhouette_samples.
 * knn_kernel:    Kmat[i][j] = exp(-D[i][j]^2 / (4 epsilon)) for the k smallest entries of row i (the point itself included,
 *                like sklearn's kneighbors_graph on the fitted data), 0 elsewhere: the kernel matrix pydiffmap builds.
 *                A row is sorted in LDS: N > PILOT_OT_KNN_MAX_N -> PILOT_OT_ENOTSUP, from every entry point that reaches the
 *                kNN kernel, before anything is allocated or copied. */
#define PILOT_OT_KNN_MAX_N 16384
#define PILOT_OT_ROWMETRIC_EUCLIDEAN 0
#define PILOT_OT_ROWMETRIC_COSINE 1
int pilot_ot_row_distances(const double *E, int N, int normalize_by_max, int metric, double *D);
int pilot_ot_row_distances_dev(const double *d_E, int N, int normalize_by_max, int metric, double *d_D,
                               double *d_max_scratch /* 8 bytes, needed when normalize_by_max */, void *stream);
int pilot_ot_silhouette(const double *D, const int *labels, int N, int n_clusters, double *score, double *samples);
int pilot_ot_knn_kernel(const double *D, int N, int k, double epsilon, double *Kmat);
/* device-resident forms: device pointers + a stream, nothing allocated, nothing synchronised.  d_sizes_scratch: n_clusters
 * ints; d_samples: N doubles (silhouette_samples; the score is their mean).  knn_kernel keeps EXACTLY k entries per row
 * (rows tied at the k-th distance in index order). */
int pilot_ot_silhouette_dev(const double *d_D, const int *d_labels, int N, int n_clusters, int *d_sizes_scratch,
                            double *d_samples, void *stream);
int pilot_ot_knn_kernel_dev(const double *d_D, int N, int k, double epsilon, double *d_Kmat, void *stream);
/* fused chains: the matrix goes to the device once (E_is_device != 0: it is there already, e.g. the pair grid's output or
 * pilot_ot_multi_device_matrix), the N x N row distances never leave it.
 * silhouette_of_rows       = Sil_computing(E [/ max(E)], labels, metric)                    (Trajectory.py:592-612, ploting.py:324)
 * diffusion_kernel_of_rows = E / max(E) -> Euclidean row distances -> k-nn Gaussian kernel   (ploting.py:95-110); D_out nullable */
int pilot_ot_silhouette_of_rows(const double *E, int E_is_device, int N, int normalize_by_max, int metric, const int *labels,
                                int n_clusters, double *score, double *samples);
int pilot_ot_diffusion_kernel_of_rows(const double *E, int E_is_device, int N, int k, double epsilon, double *D_out, double *Kmat);

/* ---- diffusion map: pl.trajectory's embedding, pydiffmap's DiffusionMap.from_sklearn(n_evecs, epsilon, alpha, k)
 * .fit_transform(E / max(E)) (pilotpy/plot/ploting.py:95-110) with a numeric epsilon, no weight function, no bandwidth
 * normalisation.  From a non-negative N x N kernel K (e.g. what pilot_ot_knn_kernel_dev left): Ks = max(K, K^T), q = Ks.sum(1),
 * A = diag(q^-alpha) Ks diag(q^-alpha), P = diag(1 / A.sum(1)) A, L = (P - I) / epsilon.  The n_evecs + 1 eigenpairs of L of
 * largest real part come from a symmetric Lanczos run (full re-orthogonalisation) on the matrix similar to P; the first
 * (lambda = 0) is dropped.  evals (n_evecs, descending): lambda of L; evecs (N x n_evecs row-major, nullable): the right
 * eigenvectors of P, unit 2-norm, the entry of largest magnitude of each column positive (lowest index on ties); dmap
 * (N x n_evecs row-major) = evecs * sqrt(-1 / evals).  Every row of K must have a positive sum.
 * info[0] = Lanczos steps, info[1] = PILOT_OT_DIFFMAP_* flags.  All in f64, fixed-order sums: repeated calls give identical bits.
 * PILOT_OT_EINVAL (before any HIP call): N < 2, n_evecs outside [1, min(N - 1, 64)], epsilon not positive and finite, alpha not
 * finite, k < 1, a required pointer NULL.  N beyond the kNN kernel's LDS sort: PILOT_OT_ENOTSUP.
 * _dev: device pointers, synchronises `stream` (the tridiagonal problem is solved on the host); info on the host.
 * _of_rows: the whole chain from E (on the host, or in HBM when E_is_device): E / max(E) -> Euclidean row distances -> k-nn
 * Gaussian kernel -> the above; dmap / evecs / evals / info on the host. */
#define PILOT_OT_DIFFMAP_NOT_CONVERGED 1  /* the basis cap (min(N, 1024) vectors) was reached before every wanted Ritz pair converged
                                           * and a verification block showed that no copy of a wanted eigenvalue is hidden */
#define PILOT_OT_DIFFMAP_DEGENERATE 2     /* more than one eigenvalue mu of P with mu >= 1 - 1e-10: a (nearly) disconnected graph */
int pilot_ot_diffusion_map_dev(const double *d_K, int N, double epsilon, double alpha, int n_evecs, double *d_dmap, double *d_evecs,
                               double *d_evals, int *info, void *stream);
int pilot_ot_diffusion_map_of_rows(const double *E, int E_is_device, int N, int k, double epsilon, double alpha, int n_evecs,
                                   double *dmap, double *evecs, double *evals, int *info);

/* ---- trajectory model fits: pilotpy's fit_best_model / fit_model_activity (tools/Cell_gene_selection.py),
 * the regression engine of cell_importance and genes_importance.  Y: n observations x n_targets, row-major with leading dimension
 * ld (elements), float32 (dtype 0) or float64 (dtype 1), on the host or (Y_is_device) in HBM; x: the n time values (host).
 * For every target column y, three models with an intercept, in this order: linear [x], linear_quadratic [x, x^2], quadratic
 * [x^2]; OLS (model OLS, LinearRegression), or (model HUBER) the optimum of scikit-learn's HuberRegressor objective over
 * (w, c, sigma >= 10 DBL_EPSILON)
 *   n sigma + sum_{|r| <= eps sigma} r^2 / sigma + sum_{|r| > eps sigma} (2 eps |r| - eps^2 sigma) + 1e-4 ||w||^2
 * found by Newton steps with a bracketing line search, stopped when (sum of |projected gradient|) * sigma <= 1e-12 * objective
 * (gradient over the fit in a scaled basis and sigma) or when no lower objective exists in floating point along a descent
 * direction; after 100 steps the (target, model) is PILOT_OT_TRAJFIT_NOT_CONVERGED and ineligible.  Per (target, model):
 * params (c, w) (3 slots, the third NaN for the two-coefficient models), t-test p-values 2 (1 - Tcdf(|t|, n - p)) with
 * t_j = params_j / sqrt(SSE / (n - p) diag((Z^T Z)^-1)_j) for both models (third slot NaN likewise), rsquared_adj (r2_score's rule
 * when SST = 0), mod_rsquared_adj (modified SSE with the fixed threshold 1.35, IEEE division), and sigma (NaN for OLS), Newton steps,
 * flags.  Per target: chosen model (0 / 1 / 2 in the order above, -1 none: eligible = not flagged and every p-value <= pval_thr,
 * the largest adjusted R^2 -- the modified one with modify_r2 -- wins on a strict >), slope over [min x, max x], pattern (bit 0:
 * params[1] < 0, bit 1: params[2] < 0 for linear_quadratic; -1 when none is chosen), Pearson r and its two-sided p, zero fraction,
 * mean.  A constant target has SST = 0 and NaN Pearson results.  Arrays are n_targets x 3 x 3 (params, pvalues), n_targets x 3
 * (R^2, sigma, steps, flags) and n_targets; every output pointer may be NULL.  All in f64 with fixed-order sums: bit-reproducible.
 * PILOT_OT_EINVAL (before any HIP call): a NULL Y / x / out, n < 4, n_targets < 0, ld < n_targets, dtype not 0 / 1, model not
 * OLS / HUBER, epsilon not finite or < 1 (checked for both models), pval_thr NaN, x not finite or with fewer than 3 distinct values.
 * A host Y moves through the device in chunks of columns of at most 256 MiB.  n_not_converged (nullable): the flagged count. */
#define PILOT_OT_TRAJFIT_OLS 0
#define PILOT_OT_TRAJFIT_HUBER 1
#define PILOT_OT_TRAJFIT_NOT_CONVERGED 1
typedef struct pilot_ot_trajfit_out {
    double *params, *pvalues;                 /* n_targets x 3 x 3 */
    double *rsquared_adj, *mod_rsquared_adj;  /* n_targets x 3 */
    double *sigma;                            /* n_targets x 3: Huber scale (NaN for OLS) */
    int *steps, *flags;                       /* n_targets x 3: Huber Newton steps, PILOT_OT_TRAJFIT_* flags */
    int *chosen, *pattern;                    /* n_targets */
    double *slope, *pearson_r, *pearson_p, *zero_fraction, *mean;   /* n_targets */
} pilot_ot_trajfit_out;
int pilot_ot_trajectory_fits(const void *Y, int Y_is_device, int dtype, int n, int n_targets, long long ld, const double *x,
                             int model, double epsilon, double pval_thr, int modify_r2, pilot_ot_trajfit_out *out,
                             int *n_not_converged);
/* genes_importance's optional normalisation (scanpy's normalize_total(target_sum) then log1p, restated): X n x n_genes dense
 * row-major float32 / float64 on the host; out (n x n_cols, same dtype, host) = log1p(X[i, cols[j]] * target_sum / sum_g X[i, g]),
 * the row total in f64 over every gene; a row without counts stays 0. */
int pilot_ot_normalize_log1p(const void *X, int dtype, int n, int n_genes, double target_sum, const int *cols, int n_cols, void *out);

/* ---- bootstrap Huber fits: the 2 x 50 HuberRegressor fits behind every row of pilotpy's
 * gene_cluster_differentiation (tools/Gene_cluster_specific.py).  Y: n observations x n_cols, row-major with leading dimension ld
 * (elements), float32 (dtype 0) or float64 (dtype 1), on the host (copied whole) or (Y_is_device) in HBM; x: the n base times
 * (host).  Problem q fits column cols[q] of Y with model models[q] (0 linear [x], 1 linear_quadratic [x, x^2], 2 quadratic [x^2],
 * each with an intercept) B times: fit b regresses y (in its own order) on x[idx[q][i][b]], i = 0 .. n-1 -- only the times are
 * resampled.  idx: n_problems x n x B ints in [0, n), observation-major (host; streamed through the device in chunks of at most
 * 256 MiB).  Every fit goes to the optimum of scikit-learn's HuberRegressor objective (alpha 1e-4, sigma >= 10 DBL_EPSILON) by the
 * method of pilot_ot_trajectory_fits: Newton steps from the penalised least-squares fit, bracketing line search, the same stop rule,
 * after 100 steps PILOT_OT_TRAJFIT_NOT_CONVERGED.  A resample with fewer distinct times than coefficients still has one optimum
 * (alpha > 0) and gets it.  Out, per (problem, bootstrap), problem-major: params (n_problems x B x 3, on [1, f(x)]; the third slot
 * NaN for the two-coefficient models), and the nullable sigma, steps (Newton steps), flags (PILOT_OT_TRAJFIT_* bits).
 * n_not_converged (nullable): the flagged count.  All in f64 with fixed-order sums: bit-reproducible across routes and chunkings.
 * PILOT_OT_EINVAL (before any HIP call): a NULL Y / x / params (cols / models / idx when n_problems > 0), n < 1, n_cols < 1,
 * ld < n_cols, dtype not 0 / 1, n_problems < 0, B outside [1, 64 * 65535], epsilon not finite or < 1, x not finite, cols[q] outside
 * [0, n_cols), models[q] not 0 / 1 / 2, idx values outside [0, n). */
int pilot_ot_bootstrap_huber_fits(const void *Y, int Y_is_device, int dtype, int n, int n_cols, long long ld, const double *x,
                                  int n_problems, const int *cols, const int *models, int B, const int *idx, double epsilon,
                                  double *params, double *sigma, int *steps, int *flags, int *n_not_converged);

/* ---- gene curve clustering (K11): the numerical core of pilotpy's genes_selection_analysis (plot/gene_selection_analysis.py:
 * get_noised_curves, cluster_genes_curves, compute_curves_activities; plot/curve_activity.py).  All in f64 with fixed-order sums
 * and no floating-point atomics: a repeated call, and the host and device routes of an argument, return the same bits.  A matrix
 * argument with an *_is_device flag is a host array or a dense row-major buffer in HBM; vectors are host arrays. */
#define PILOT_OT_LINKAGE_MAX_G 32768   /* rows of a linkage: its G x G float64 distance matrix (8 GiB here) is held in HBM */
#define PILOT_OT_LINKAGE_SINGLE 0
#define PILOT_OT_LINKAGE_COMPLETE 1
#define PILOT_OT_LINKAGE_AVERAGE 2
#define PILOT_OT_LINKAGE_WEIGHTED 3
/* Sample standard deviation (ddof 1, two passes: mean, then squared deviations) of column cols[j] (cols NULL: every column,
 * n_sel = n_cols) of Y over each row segment offsets[s] .. offsets[s + 1] (n_segments + 1 non-decreasing entries in [0, n];
 * n_segments <= 65535).  Y: n x n_cols, leading dimension ld (elements), float32 (dtype 0) or float64 (1).  out: n_segments x
 * n_sel; a segment of one row (or none) gives NaN. */
int pilot_ot_segment_std(const void *Y, int Y_is_device, int dtype, long long n, int n_cols, long long ld, const long long *offsets,
                         int n_segments, const int *cols, int n_sel, double *out, int out_is_device);
/* out[g][t] = design(models[g], times[t]) . params[g] (params: G x 3 = Intercept, Treat, Treat2; model 0 linear [1, t],
 * 1 linear_quadratic [1, t, t^2], 2 quadratic [1, t^2]) + (sd, nullable, T x G) sd[t][g] / 10 * (Treat + Treat2 - Intercept), a
 * NaN entry then set to 0; each row standardised over its T values like scikit-learn's StandardScaler (population variance, a
 * scale below 10 DBL_EPSILON becomes 1).  out: G x T. */
int pilot_ot_fitted_curves(const double *params, const int *models, int G, const double *times, int T, const double *sd,
                           int sd_is_device, double *out, int out_is_device);
/* scipy.cluster.hierarchy.linkage(pdist(Y), method) of the G rows of Y (G x T): Euclidean distances in the direct form
 * sqrt(sum (a - b)^2), the nearest-neighbour chain over the full distance matrix in HBM (one persistent workgroup; ties towards
 * the previous chain element, then the lowest index; exactly G - 1 merges and at most 4 G chain steps, PILOT_OT_EHIP if that cap
 * is ever reached), then scipy's stable sort by height and labelling.  Z (host): (G - 1) x 4 = smaller root id, larger root id,
 * height, size; new clusters are numbered G + i.  dmax (nullable): the largest pairwise distance; chain_steps (nullable).
 * PILOT_OT_EINVAL: G < 2, G > PILOT_OT_LINKAGE_MAX_G, T < 1, a non-finite value; PILOT_OT_ENOTSUP: any other method. */
int pilot_ot_linkage_of_rows(const double *Y, int Y_is_device, int G, int T, int method, double *Z, double *dmax, int *chain_steps);
/* Per row of curves (G x T) over the strictly increasing times (T >= 2, else PILOT_OT_EINVAL): out (host, G x 4) = terminal logFC,
 * transient logFC, switching time, area, as plot/curve_activity.py defines them (median-of-three clamp, trapezoid rule over the
 * times scaled to [0, 1], + 1e-300 in the switching time's denominator), unrounded. */
int pilot_ot_curve_activities(const double *curves, int curves_is_device, int G, int T, const double *times, double *out);

/* ---- group moments (K12): what pilotpy's patient sub-group workflow needs of a cells x genes matrix (tools/patients_sub_clustering.py:
 * compute_diff_expressions hands two groups of cells to limma; scanpy's highly_variable_genes; plot/ploting.py's Welch t-test).  For
 * a two-group design all of limma's arithmetic, scanpy's dispersion statistics and Welch's t follow from per-group count, mean and
 * centred sum of squares, which one pass over Y gives.
 * Y: n x n_cols_total, row-major with leading dimension ld (elements), float32 (dtype 0) or float64 (1), on the host (copied whole)
 * or (Y_is_device) in HBM.  codes (host, n): the group of every row, 0 .. n_groups - 1, or negative for a row that is skipped
 * (its values, finite or not and on whatever scale, enter no result); n_groups in [1, 8].  cols (host, nullable): the n_cols selected columns, any order, repeats allowed; NULL: every column
 * (n_cols = n_cols_total).  transform: 0 t(y) = y, 1 t(y) = expm1(y) in f64.
 * Out (host): count[g] = rows with codes == g; mean[g][j] = their mean of t(y) and m2[g][j] = sum (t(y) - mean)^2 over column
 * cols[j], both n_groups x n_cols in f64.  A group without rows: count 0, NaN, NaN; a group of one row: m2 = 0 exactly.
 * The squares are centred throughout (per chunk of rows about the chunk's mean, chunks and row slices joined by Chan's update in a
 * fixed order); no sum(y^2) - n mean^2 is formed and nothing uses a floating-point atomic: the same bits from every run and
 * from the host and device routes.
 * PILOT_OT_EINVAL (before any HIP call): a NULL pointer, n < 0, n_cols_total < 1, ld < n_cols_total, dtype not 0 / 1, n_groups
 * outside [1, 8], transform not 0 / 1, n_cols < 0 (or != n_cols_total without cols), a column outside [0, n_cols_total), a code
 * >= n_groups. */
int pilot_ot_group_moments(const void *Y, int Y_is_device, int dtype, long long n, int n_cols_total, long long ld, const int *codes,
                           int n_groups, const int *cols, int n_cols, int transform, long long *count, double *mean, double *m2);

/* ---- sparse matrices (K13): a cells x genes matrix resident in HBM as CSR, for the gene-level consumers above.  scRNA-seq counts
 * are a few percent non-zero; the handle keeps indptr (int64, n_rows + 1), indices (int32) and data (float32: dtype 0, float64: 1)
 * on the current device and never forms the dense matrix unless pilot_ot_csr_densify is asked for some columns.
 * pilot_ot_csr_upload copies the three host arrays.  Indices within a row may come in any order; a row must not store a column
 * twice.  PILOT_OT_EINVAL (before any HIP call): a NULL pointer, dtype not 0 / 1, n_rows < 0 or > INT_MAX, n_cols < 1,
 * indptr[0] != 0, indptr not non-decreasing, an index outside [0, n_cols), a duplicate entry.
 * Every sum below is taken in f64 in a fixed order and nothing uses a floating-point atomic: the same bits from every run. */
typedef struct pilot_ot_csr pilot_ot_csr;
int pilot_ot_csr_upload(const long long *indptr, const int *indices, const void *data, int dtype, long long n_rows, int n_cols,
                        pilot_ot_csr **csr);
int pilot_ot_csr_destroy(pilot_ot_csr *csr);
/* In place: every stored value v of a row becomes log1p(v * target_sum / total) with total the row's sum over its stored values
 * (pilot_ot_normalize_log1p's expressions; a row without counts stays 0; zeros stay implicit).  Drops the column form.
 * PILOT_OT_EINVAL: target_sum not positive and finite, a NULL handle. */
int pilot_ot_csr_normalize_log1p(pilot_ot_csr *csr, double target_sum);
/* The column-major copy (per column its entries in ascending row order) the per-column calls read.  It is built on the device
 * by the first call that needs it and kept until the values change; this call only builds it ahead of time.  The build cuts the
 * rows into slices of pilot_ot_csr_slice_rows() rows. */
int pilot_ot_csr_build_columns(pilot_ot_csr *csr);
int pilot_ot_csr_slice_rows(void);
/* nnz (host, n_cols): per column the stored values that are != 0 (an explicitly stored 0 is a zero). */
int pilot_ot_csr_column_nnz(pilot_ot_csr *csr, long long *nnz);
/* pilot_ot_group_moments of the matrix (same codes, n_groups, cols, transform, outputs and error cases), from the column form:
 * mean = sum over the stored entries / count, m2 = sum over the stored entries of (t(y) - mean)^2 + (count - stored) mean^2, every
 * term non-negative.  cols NULL: every column (n_cols = the matrix's). */
int pilot_ot_csr_group_moments(pilot_ot_csr *csr, const int *codes, int n_groups, const int *cols, int n_cols, int transform,
                               long long *count, double *mean, double *m2);
/* out (DEVICE, n_rows x n_cols elements of the matrix's dtype, row-major): the dense copy of the columns cols (host; NULL: every
 * column), zero-filled and every stored entry written once.  PILOT_OT_EINVAL: a column out of range or named twice. */
int pilot_ot_csr_densify(pilot_ot_csr *csr, const int *cols, int n_cols, void *out);

/* ---- group sums (K14): per-group column sums for many groups -- the (cell type, sample) pseudobulk counts that pilotpy's
 * get_pseudobulk_DE forms with groupby().sum() on the densified matrix (plot/pseudobulk_DE_analysis.py:590-594).  Y, dtype, n,
 * n_cols_total, ld, codes, cols and n_cols are pilot_ot_group_moments's; n_groups in [1, 2^20].
 * Out (host): count[g] = rows with codes == g; sum[g][j] = the sum of y over those rows in column cols[j], n_groups x n_cols in
 * f64.  A row with a negative code enters nothing, whatever it holds, and is never read.  A group without rows: count 0, sum 0.0.
 * The used rows are sorted stably by group on the host and every group is cut into slices of pilot_ot_group_sums_slice_rows()
 * rows; a slice adds its rows one after another in ascending row order, a group's slices are added in slice order: the order
 * depends on (n, codes) and that constant alone, nothing uses a floating-point atomic, and the same bits come from every run and
 * from the host and device routes.
 * PILOT_OT_EINVAL (before any HIP call): a NULL pointer, n < 0, n_cols_total < 1, ld < n_cols_total, dtype not 0 / 1, n_groups
 * outside [1, 2^20], n_cols < 0 (or != n_cols_total without cols), a column outside [0, n_cols_total), a code >= n_groups.
 * PILOT_OT_ENOTSUP: n > INT_MAX. */
int pilot_ot_group_sums(const void *Y, int Y_is_device, int dtype, long long n, int n_cols_total, long long ld, const int *codes,
                        int n_groups, const int *cols, int n_cols, long long *count, double *sum);
/* The same of a sparse matrix, from its row form: the column form is neither needed nor built, so the call also serves a matrix
 * whose values were just changed (pilot_ot_csr_normalize_log1p).  One wave takes a slice's rows in order and adds the stored
 * entries of pilot_ot_group_sums_col_block() selected columns into f64 accumulators in LDS; implicit zeros add nothing.  The
 * slices are the dense call's, so the two agree to the bit wherever the matrices do.  cols NULL: every column (n_cols = the
 * matrix's).  Same error cases (n_groups and n_cols < 0 are judged before the handle). */
int pilot_ot_csr_group_sums(pilot_ot_csr *csr, const int *codes, int n_groups, const int *cols, int n_cols, long long *count,
                            double *sum);
int pilot_ot_group_sums_slice_rows(void);
int pilot_ot_group_sums_col_block(void);

/* ---- rank sums (K21): per selected column, the tie-averaged ranks of the used rows summed per group -- what the Wilcoxon /
 * Mann-Whitney rank-sum test of a group against the rest (scanpy's rank_genes_groups(method="wilcoxon")) and the Kruskal-Wallis
 * test over all groups are made of.  Y, dtype, n, n_cols_total, ld, codes, cols and n_cols are pilot_ot_group_moments's; n_groups
 * in [1, 1024].  N = the used rows (code >= 0); an unused row is never read.  Per selected column j, over the used rows:
 * rank_i = the 1-based rank of y_ij, equal values sharing the mean of their positions (scipy.stats.rankdata(method="average"));
 * equality is numeric, -0.0 == 0.0, and in a sparse matrix a stored 0 ties with the implicit ones.
 * Out (host): count[g] = rows with codes == g; rank2[g][j] = 2 * sum_{i in g} rank_i (n_groups x n_cols, an exact integer);
 * ties[j] = sum over the runs of equal values of t^3 - t, t the run's length.  No used rows: all 0.
 * Only a column's non-zero used values are sorted (the zeros are one run whose place follows from the number of negatives), by
 * one wave for up to pilot_ot_rank_sums_wave_max() of them, one workgroup in LDS up to pilot_ot_rank_sums_wg_max(), and one
 * workgroup in HBM with tiles of pilot_ot_rank_sums_sort_tile() in LDS beyond.  Everything on the device is an integer and only
 * integer atomics are used: the dense and sparse routes and a repeated call return the same values.
 * A NaN or infinity in a used row of a selected column: PILOT_OT_EINVAL with *bad_row / *bad_col (nullable; -1 otherwise) the row
 * and the column of Y of the first one -- the lowest position in cols, then the lowest row.
 * PILOT_OT_EINVAL (before any HIP call): a NULL pointer, n < 0, n_cols_total < 1, ld < n_cols_total, dtype not 0 / 1, n_groups
 * outside [1, 1024], n_cols < 0 (or != n_cols_total without cols), a column outside [0, n_cols_total), a code >= n_groups.
 * PILOT_OT_ENOTSUP (before any HIP call): n > INT_MAX, or N > 2^21 - 1 (t^3 must fit 63 bits). */
int pilot_ot_rank_sums(const void *Y, int Y_is_device, int dtype, long long n, int n_cols_total, long long ld, const int *codes,
                       int n_groups, const int *cols, int n_cols, long long *count, long long *rank2, long long *ties,
                       long long *bad_row, int *bad_col);
/* The same of a sparse matrix, from its column form (built by the first call that needs it): the work per column is
 * O(stored log stored), never O(n).  cols NULL: every column (n_cols = the matrix's).  Same error cases (n_groups and n_cols < 0
 * are judged before the handle). */
int pilot_ot_csr_rank_sums(pilot_ot_csr *csr, const int *codes, int n_groups, const int *cols, int n_cols, long long *count,
                           long long *rank2, long long *ties, long long *bad_row, int *bad_col);
int pilot_ot_rank_sums_wave_max(void);
int pilot_ot_rank_sums_wg_max(void);
int pilot_ot_rank_sums_sort_tile(void);

/* ---- PERMANOVA (K29): the permutation test of "does this variable explain the distances between samples" on the distance matrix
 * itself (Anderson 2001; vegan's adonis2, marginal terms).  vegan is not installed where this library is built, so the rule is THIS
 * LIBRARY'S STATEMENT, unpinned.
 * D: N x N, dtype 0 float32 / 1 float64, leading dimension ld, on the host or in HBM.  rows: the n used samples, ascending (NULL: all,
 * n == N).  s_ij = (D_ij + D_ji) / 2 (i != j), s_ii = 0, A_ij = -0.5 s_ij s_ij, in float64; *ss_total = -(1/n) sum_ij A_ij.
 * Q (host, n x c, packed): the model terms, term t being columns term_off[t] .. term_off[t + 1] - 1 (term_off: n_terms + 1 ints from
 * 0 to c); the columns are centred and orthonormal within a term (only the centring is checked).
 * Permutation 0 is the identity.  For b >= 1, row i's key is the first two words of Philox4x32-10(counter (i, b mod 2^32, b div 2^32, 0),
 * key (seed mod 2^32, seed div 2^32)), w0 2^32 + w1; with s_0, s_1, ... the rows ordered by (stratum, key, i) and r_0, r_1, ... by
 * (stratum, i), the permuted design is Z_b[r_t, :] = Q[s_t, :] (strata NULL: one stratum).  A function of (seed, b, n, strata) alone.
 * Out (host): ss[(b - start) * n_terms + t] = sum over the term's columns, in column order, of Z_b[:, c]^T A Z_b[:, c], for
 * b = start .. start + count - 1.  Permutation b's values have the same bits in any batch, at any start, under any chunking; no
 * floating-point atomics.  Device memory does not grow with count: permutations are processed pilot_ot_permanova_limits' chunk at a
 * time.  kernel_ms (nullable, 3 floats): device milliseconds of the prepare, permute and quadratic-form kernels.
 * A NaN or infinity between two used samples: PILOT_OT_EINVAL with *bad_row / *bad_col (nullable; -1 otherwise) one such entry of D.
 * PILOT_OT_EINVAL (before any HIP call): a NULL pointer, N < 1, ld < N, dtype not 0 / 1, n < 1 (or != N without rows), rows not
 * ascending inside [0, N), c outside [1, 4096], n_terms outside [1, c], term_off not strictly ascending from 0 to c, a column of Q
 * whose sum is not 0 to 1e-8 (1 + sum |q|), a negative stratum, start or count.  PILOT_OT_ENOTSUP (before any HIP call): n > 8192,
 * the LDS sort's limit. */
int pilot_ot_permanova(const void *D, int D_is_device, int dtype, int N, long long ld, const int *rows, int n, const double *Q, int c,
                       const int *term_off, int n_terms, const int *strata, unsigned long long seed, long long start, long long count,
                       double *ss_total, double *ss, long long *bad_row, long long *bad_col, float *kernel_ms);
/* The permutations themselves: perm[(b - start) * n + r_t] = s_t (host, count x n int32).  Same checks. */
int pilot_ot_permanova_permutations(int n, const int *strata, unsigned long long seed, long long start, long long count, int *perm);
/* Every pointer nullable: the largest n, the permutations per pass (at most 65536 / c when that is fewer), the columns a workgroup
 * of the quadratic-form kernel owns and the rows of A it reads. */
int pilot_ot_permanova_limits(int *max_n, int *chunk, int *tile_cols, int *row_block);

/* ---- negative-binomial GLM (K22): DESeq2's model (Love, Huber, Anders 2014) for the one design pilotpy's compute_pseudobulk_DE
 * uses, `~ stage` (plot/pseudobulk_DE_analysis.py:96-159): an intercept plus a group indicator, for which every piece decouples by
 * group.  DESeq2 is not installed where this library is built, so the rule is THIS LIBRARY'S STATEMENT, unpinned (DESIGN.md K22;
 * restated in tests/nb_glm_restatement.py).  Y: m samples x n_genes, row-major (Y_is_device / dtype / ld as in
 * pilot_ot_group_moments), c = rint(Y); codes[j] in 0 .. n_groups - 1 (host); size_factors[j] > 0 (host).  minDisp = 1e-8,
 * maxDisp = max(10, m), minmu = 0.5.  All arithmetic is f64; every sum has one fixed order (the samples by group, then by index)
 * and no atomic adds a floating-point value: the same call returns the same bits, from float32 and float64 storage of the same
 * counts, from a host matrix and from HBM.
 *
 * pilot_ot_nb_dispersions: per gene, mu_j = max(s_j * mean_{i in g(j)} c_i / s_i, minmu) and x = log(alpha) maximising
 *     L(x) = sum_j [lgamma(c_j + r) - lgamma(r) - (c_j + r) log1p(alpha mu_j) + c_j log(alpha mu_j)] - 1/2 sum_g log(sum_{j in g} w_j)
 *            [- (x - log_prior_mean)^2 / (2 prior_var)],   r = 1 / alpha,  w_j = mu_j / (1 + alpha mu_j)
 * (the Cox-Reid adjusted profile likelihood; the last term only with log_prior_mean != NULL) BY THIS SEARCH: six rounds of the
 * 64-point grid x_i = lo + (hi - lo) i / 63, from [log minDisp, log maxDisp]; b = the first largest value (lowest index on ties);
 * the next bracket is [x_max(b-1,0), x_min(b+1,63)].  A global search, not DESeq2's line search from a moments start.
 * Out (host): log_disp, objective (n_genes; the last round's x_b and L(x_b)), fitted_mean (nullable; n_genes x n_groups, the
 * normalised group means).  A gene of zeros, or one whose log_prior_mean is not finite, gets NaN in log_disp and objective.
 * pilot_ot_nb_group_fits: with the gene's dispersion alpha (host; NaN leaves the gene out: q = w = NaN), per (gene, group) q = the
 * root of sum_{j in g} (c_j - s_j q) / (1 + alpha s_j q) = 0 by safeguarded Newton / bisection steps in log q (stopped at
 * |step| <= 1e-12, or after 100 steps with PILOT_OT_NB_NOT_CONVERGED), raised to minmu / max_{j in g} s_j if below
 * (PILOT_OT_NB_FLOORED; a group of zeros ends there), and w = sum_{j in g} mu_j / (1 + alpha mu_j) with mu_j = max(s_j q, minmu).
 * Out (host): q, w, steps, flags: n_genes x n_groups; *n_not_converged (nullable).
 * PILOT_OT_EINVAL (before any HIP call): a NULL pointer, n_genes < 1, dtype, ld < n_genes, m < 2, n_groups outside [2, m - 1], a code
 * out of range, a group without samples, a size factor not positive and finite, with a prior a prior_var not positive and finite, a
 * dispersion outside [minDisp, maxDisp]; after the check pass: a negative or non-finite count (the message names it; of
 * pilot_ot_nb_dispersions also *bad_row / *bad_col, nullable, else -1: the lowest column, then the lowest row).
 * PILOT_OT_ENOTSUP: m > INT_MAX; of pilot_ot_nb_dispersions m > pilot_ot_nb_glm_max_samples() (a gene is staged in LDS). */
#define PILOT_OT_NB_NOT_CONVERGED 1
#define PILOT_OT_NB_FLOORED 2
int pilot_ot_nb_dispersions(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const int *codes,
                            int n_groups, const double *size_factors, const double *log_prior_mean, double prior_var, double *log_disp,
                            double *objective, double *fitted_mean, long long *bad_row, int *bad_col);
int pilot_ot_nb_group_fits(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const int *codes,
                           int n_groups, const double *size_factors, const double *dispersion, double *q, double *w, int *steps,
                           int *flags, int *n_not_converged);
int pilot_ot_nb_glm_max_samples(void);

/* pilot_ot_nb_shrink (K23): the shrunken fold change that pilotpy's compute_pseudobulk_DE reads after
 * `lfcShrink(dds, coef, res, type = "apeglm")` (plot/pseudobulk_DE_analysis.py:140-151; Zhu, Ibrahim, Love 2019), for two groups:
 * code 0 the denominator, code 1 the numerator.  apeglm is not installed where this library is built, so the rule is THIS
 * LIBRARY'S STATEMENT, unpinned (restated in tests/nb_shrink_restatement.py).  Y, codes, size_factors as above
 * with n_groups = 2; dispersion: the gene's final dispersion alpha (host; NaN leaves the gene out: NaN everywhere, flags 0).
 * Natural-log scale.  Per gene, eta_j = b0 + b1 [codes[j] = 1] + log s_j, mu_j = exp(eta_j), and the log posterior up to constants
 *     P(b0, b1) = sum_j [c_j log(alpha mu_j) - (c_j + 1/alpha) log1p(alpha mu_j)] - b0^2 / (2 sigma0^2) - log1p(b1^2 / S^2)
 * with sigma0 = intercept_scale (apeglm's prior.no.shrink.scale, 15) and S = prior_scale of the Cauchy prior on b1 (prior.df = 1).
 * P is strictly concave in b0; the profile p(b1) = max_b0 P(b0, b1) has its largest value between 0 and the maximum-likelihood
 * b1 and can have TWO local maxima there, so the estimate is defined BY THIS SEARCH: far_end[gene] = sg E (host, finite; sg the
 * sign of the maximum-likelihood b1, E = |it| + 1, or 30 where a group's fit is PILOT_OT_NB_FLOORED); t in [0, asinh(E / S)] with
 * b1 = sg S sinh(t); six rounds of the 64-point grid t_i = lo + (hi - lo) i / 63; b = the first largest p (lowest index on ties);
 * the next bracket is [t_max(b-1,0), t_min(b+1,63)].  b = 63 in a bracket that still ends at asinh(E / S) sets
 * PILOT_OT_NB_AT_BOUND.  For every grid point b0 is the root of sum_j (c_j - mu_j) / (1 + alpha mu_j) - b0 / sigma0^2 by safeguarded
 * Newton / bisection steps as pilot_ot_nb_group_fits' (|step| <= 1e-12; 100 steps in any of them set PILOT_OT_NB_NOT_CONVERGED),
 * each grid point started from its own b0 of the round before.  Same bits as stated above for the K22 calls.
 * Out (host, n_genes): beta0, beta1, objective = b0, b1 and p at the last round's winner; info (n_genes x 2): the groups' observed
 * information W_g = sum_{j in g} mu_j (1 + alpha c_j) / (1 + alpha mu_j)^2 there; flags: PILOT_OT_NB_* in the low
 * PILOT_OT_NB_SHRINK_STEPS_SHIFT bits, above them the gene's inner steps summed over the grid points and rounds; *n_at_bound
 * (nullable): the genes flagged PILOT_OT_NB_AT_BOUND.
 * PILOT_OT_EINVAL (before any HIP call): the cases of pilot_ot_nb_group_fits with n_groups = 2 (so m >= 3 and both groups have a
 * sample), a prior_scale or intercept_scale not positive and finite, a far_end not finite; after the check pass a negative or
 * non-finite count (*bad_row / *bad_col as pilot_ot_nb_dispersions).  PILOT_OT_ENOTSUP: m > pilot_ot_nb_glm_max_samples() (a gene's
 * counts and size factors are staged in LDS, 16 m bytes). */
#define PILOT_OT_NB_AT_BOUND 4
#define PILOT_OT_NB_SHRINK_STEPS_SHIFT 8
int pilot_ot_nb_shrink(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const int *codes,
                       const double *size_factors, const double *dispersion, const double *far_end, double prior_scale,
                       double intercept_scale, double *beta0, double *beta1, double *objective, double *info, int *flags, int *n_at_bound,
                       long long *bad_row, int *bad_col);

/* pilot_ot_nb_dispersions_blind, pilot_ot_nb_rlog (K24): the two device steps of `rlog(dds, blind = TRUE)`, which pilotpy's
 * compute_pseudobulk_PCA returns (plot/pseudobulk_DE_analysis.py:161-207; Love, Huber, Anders 2014, "regularized logarithm").
 * THIS LIBRARY'S STATEMENT, unpinned (restated in tests/nb_rlog_restatement.py).  Y, size_factors, dtype, ld and
 * the same-bits statement as above; there are no groups: blind means the design `~ 1`.
 *
 * pilot_ot_nb_dispersions_blind: pilot_ot_nb_dispersions with the ONE group of all m >= 2 samples (which that call refuses) and no
 * prior: mu_j = max(s_j mean_i(c_i / s_i), minmu), the same search.  base_mean (nullable, n_genes): mean_j(c_j / s_j).
 *
 * pilot_ot_nb_rlog: per gene, with alpha = dispersion[gene] (host; the trend value; NaN leaves the gene out: NaN in its column and
 * intercept), lambda = ln2^2 / prior_var, lambda0 = 1e-6 ln2^2 and eta_j = b0 + b_j + log s_j, the maximiser over (b0, b_1 .. b_m) of
 *     P = sum_j [c_j eta_j - (c_j + 1/alpha) log1p(alpha e^{eta_j})] - lambda/2 sum_j b_j^2 - lambda0/2 b0^2
 * P is strictly concave, so the result does not depend on the path (DESeq2's IRLS stops at a deviance change of 1e-4 and clamps mu
 * at 0.5 inside its loop; this returns the optimum).  The path: from b0 = log mean_j(c_j / s_j), b = 0, Newton steps on the
 * arrowhead system -- mu = e^eta, r = (c - mu) / (1 + alpha mu), w = mu (1 + alpha c) / (1 + alpha mu)^2, g = r - lambda b,
 * h = w + lambda, d0 = (sum r - lambda0 b0 - sum w g / h) / (sum w + lambda0 - sum w^2 / h), d_j = (g_j - w_j d0) / h_j -- of
 * length t, halved from 1 at most 20 times until P does not fall (a non-finite value counts as a fall; the change of P is summed
 * term by term, not taken as a difference of two sums; a step within 1e-10 at t = 1 is taken whole); stopped once max(|t d0|, max_j |t d_j|) <= 1e-10, or after 100 iterations
 * with PILOT_OT_NB_NOT_CONVERGED.  Every sum is a per-lane partial in sample order (lane l: samples l, l + 64, ...) closed by one
 * fixed butterfly: a gene gives the same bits alone and in any batch.
 * Out: out, m x n_genes float64 with leading dimension ld_out >= n_genes, on the host or in HBM (out_is_device):
 * (b0 + b_j) / ln2; a gene of zeros gives 0 in every sample and a NaN intercept.  Host: intercept (n_genes) = b0 / ln2, steps
 * (iterations), flags (PILOT_OT_NB_NOT_CONVERGED); *n_not_converged (nullable).
 * PILOT_OT_EINVAL (before any HIP call): a NULL pointer, n_genes < 1, dtype, ld < n_genes, ld_out < n_genes, m < 2, a size factor
 * not positive and finite, a prior_var not positive and finite, a dispersion outside [minDisp, maxDisp]; after the check pass a
 * negative or non-finite count (*bad_row / *bad_col as pilot_ot_nb_dispersions).  PILOT_OT_ENOTSUP: m > INT_MAX;
 * m > pilot_ot_nb_glm_max_samples() (a gene's counts, log size factors and coefficients are staged in LDS, 24 m bytes). */
int pilot_ot_nb_dispersions_blind(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld,
                                  const double *size_factors, double *log_disp, double *objective, double *base_mean, long long *bad_row,
                                  int *bad_col);
int pilot_ot_nb_rlog(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const double *size_factors,
                     const double *dispersion, double prior_var, void *out, int out_is_device, long long ld_out, double *intercept,
                     int *steps, int *flags, int *n_not_converged, long long *bad_row, int *bad_col);

/* pilot_ot_nb_cooks (K25): the Cook's distances behind the outlier handling of `DESeq(dds)` and `results(dds)`
 * (plot/pseudobulk_DE_analysis.py:140-145): replaceOutliers and the cooksCutoff filter.  THIS LIBRARY'S STATEMENT, unpinned
 * (restated in tests/nb_cooks_restatement.py).  Y, codes, n_groups = k, size_factors, dtype, ld as
 * pilot_ot_nb_group_fits; dispersion: the gene's FINAL dispersion alpha (host; NaN leaves the gene out); q: n_genes x k, that call's
 * fits at it.  With c = rint(Y), q_j = c_j / s_j and tm(x, d) the mean of the sorted x without its d lowest and d highest values
 * (R's mean(x, trim = r) with d = floor(n r)), per gene:
 *     trimmed_base = tm(q of all m samples, floor(m / 5))
 *     per group of n_g >= 3 samples, (r, scale) = (1/3, 2.04) for n_g <= 3, (1/4, 1.86) for n_g <= 23, else (1/8, 1.51) and
 *     d = floor(n_g r):    v_g = scale tm((q_g - tm(q_g, d))^2, d)
 *     alpha_robust = max((max_g v_g - mean_j q_j) / (mean_j q_j)^2, 0.04)
 *     mu_j = max(s_j q[g(j)], minmu),  w_j = mu_j / (1 + alpha mu_j),  h_j = w_j / sum_{i in g(j)} w_i
 *     D_j = (c_j - mu_j)^2 / (mu_j + alpha_robust mu_j^2)  h_j / (k (1 - h_j)^2),    NaN where n_g(j) = 1
 *     max_cooks = max of D_j over the samples of groups with n_g >= 3; arg_max the lowest sample index that attains it;
 *     n_above = #{j: c_j > c_arg_max};  n_replace = #{j: D_j > cutoff and n_g(j) >= min_replace}
 * Without a group of n_g >= 3: alpha_robust = max_cooks = NaN, every D_j NaN, arg_max = -1, n_above = n_replace = 0 (trimmed_base
 * is still computed).  A gene of zeros or with a NaN dispersion: NaN in every float result, arg_max = -1, counts 0.
 * One wave per gene; the order statistics by a bitonic sort in LDS; every sum a per-lane partial in sorted-sample order closed by
 * one fixed butterfly.  Same bits as stated above for the K22 calls, and for a gene alone or in any batch.
 * Out (host, n_genes): alpha_robust, max_cooks, arg_max, n_above, n_replace, trimmed_base.  D: nullable; m x n_genes float64 with
 * leading dimension ld_D >= n_genes, on the host or in HBM (D_is_device), D[j, gene] = D_j.
 * PILOT_OT_EINVAL (before any HIP call): the cases of pilot_ot_nb_group_fits, a cutoff not positive and finite, min_replace < 3,
 * ld_D < n_genes with a D, a q not positive and finite where the gene's dispersion is not NaN; after the check pass a negative or
 * non-finite count (*bad_row / *bad_col as pilot_ot_nb_dispersions).  PILOT_OT_ENOTSUP: m > pilot_ot_nb_glm_max_samples() (a gene's
 * counts, normalised counts and the sort buffer are staged in LDS: 8 (2 m + P) bytes, P the power of two >= m). */
int pilot_ot_nb_cooks(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const int *codes, int n_groups,
                      const double *size_factors, const double *dispersion, const double *q, double cutoff, int min_replace,
                      double *alpha_robust, double *max_cooks, int *arg_max, int *n_above, int *n_replace, double *trimmed_base, void *D,
                      int D_is_device, long long ld_D, long long *bad_row, int *bad_col);

/* ---- negative-binomial GLM for a general design (K26): the model above with covariates beside the group, `~ batch + stage`.
 * THIS LIBRARY'S STATEMENT, unpinned (restated in tests/nb_design_restatement.py).  Y, dtype, ld, size_factors and
 * the same-bits statement as above.  X: m x p, row-major float64 (host), its first column ones, 2 <= p <=
 * pilot_ot_nb_design_max_cols() = 8, m - p >= 1; the caller vouches for its full column rank.  lambda = 1e-6, the ridge on every
 * coefficient (natural-log scale).  With a covariate nothing decouples by group: mu_j = s_j exp(x_j^T beta).
 *
 * The inner fit, at a dispersion alpha: beta^(alpha) = the maximiser of
 *     l(beta) = sum_j nbinom.logpmf(c_j; mean mu_j, dispersion alpha) - lambda/2 |beta|^2,
 * which is strictly concave, so the result is the optimum whatever the path.  The path: Newton steps with the observed information
 * sum_j w_j x_j x_j^T + lambda I, w = mu (1 + alpha c) / (1 + alpha mu)^2, by a Cholesky solve, the step halved (at most 30 times) while l
 * would fall (read from the change of l summed term by term, as pilot_ot_nb_rlog's); stopped once max_k |step_k| <= 1e-10, or after
 * 100 steps with PILOT_OT_NB_NOT_CONVERGED.  A cold fit starts from (log max(mean_j c_j / s_j, minmu), 0, ...).
 *
 * pilot_ot_nb_design_dispersions: per gene x = log(alpha) maximising the adjusted PROFILE likelihood (beta is re-solved at every x)
 *     L(x) = sum_j [lgamma(c_j + r) - lgamma(r) - (c_j + r) log1p(alpha mu~_j) + c_j log(alpha mu~_j)] - 1/2 log det(X^T W X)
 *            [- (x - log_prior_mean)^2 / (2 prior_var)],  r = 1 / alpha,  mu~_j = max(s_j exp(x_j^T beta^(alpha)), minmu),
 *            W = diag(mu~_j / (1 + alpha mu~_j))
 * BY THE SEARCH of pilot_ot_nb_dispersions (six rounds of the 64-point grid from [log minDisp, log maxDisp]).  One wave per gene, a
 * lane is a grid point; round 0 fits cold, a later round from the coefficients of the round before's winner.  No floating-point sum
 * crosses lanes: a gene gives the same bits alone and in any batch.
 * Out (host, n_genes): log_disp, objective; beta (nullable, n_genes x p: the coefficients at the winner); steps (the Newton steps of
 * all 384 inner fits), flags (PILOT_OT_NB_NOT_CONVERGED if any of them did not converge); *n_not_converged (nullable).  A gene of
 * zeros, or one whose log_prior_mean is not finite: NaN, steps = flags = 0.
 * pilot_ot_nb_design_fits: with the gene's dispersion alpha (host; NaN, or a gene of zeros, leaves the gene out: NaN, steps = flags = 0),
 * one lane per gene: beta (n_genes x p) = beta^(alpha) from a cold start; cov (n_genes x p (p + 1) / 2): the upper triangle, row by
 * row, of Sigma = (X^T W X + lambda I)^-1 with W at mu~ as above (the plain inverse, not DESeq2's sandwich); loglik = sum_j
 * nbinom.logpmf(c_j; mu_j, alpha), unpenalised, at the unfloored mu; steps, flags; *n_not_converged (nullable).
 * PILOT_OT_EINVAL (before any HIP call): a NULL pointer, n_genes < 1, dtype, ld < n_genes, m < 2, a size factor not positive and
 * finite, with a prior a prior_var not positive and finite, a dispersion outside [minDisp, maxDisp], p outside [2, 8], m - p < 1, a
 * first column that is not ones, a non-finite X; after the check pass a negative or non-finite count (*bad_row / *bad_col as
 * pilot_ot_nb_dispersions).  PILOT_OT_ENOTSUP: m > INT_MAX; of pilot_ot_nb_design_dispersions m > pilot_ot_nb_design_max_samples(p)
 * (a gene's counts, log size factors and design rows are staged in LDS, 8 m (2 + p) bytes of 96 KiB: 1228 samples at p = 8).
 * pilot_ot_nb_design_max_samples: that limit, or PILOT_OT_EINVAL for a p outside [2, 8]. */
int pilot_ot_nb_design_max_cols(void);
int pilot_ot_nb_design_max_samples(int p);
int pilot_ot_nb_design_dispersions(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const double *X, int p,
                                   const double *size_factors, const double *log_prior_mean, double prior_var, double *log_disp,
                                   double *objective, double *beta, int *steps, int *flags, int *n_not_converged, long long *bad_row,
                                   int *bad_col);
int pilot_ot_nb_design_fits(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const double *X, int p,
                            const double *size_factors, const double *dispersion, double *beta, double *cov, double *loglik, int *steps,
                            int *flags, int *n_not_converged, long long *bad_row, int *bad_col);

/* pilot_ot_nb_design_shrink (K27): pilot_ot_nb_shrink for the general design, the `lfcShrink(type = "apeglm")` step after a fit with
 * covariates.  THIS LIBRARY'S STATEMENT, unpinned (restated in tests/nb_design_shrink_restatement.py).  Y, X, p,
 * size_factors, dispersion as pilot_ot_nb_design_fits.  coef in [1, p - 1]: the column k of X that is shrunk.  With S = prior_scale,
 * sigma0 = other_scale, eta_j = x_j^T beta + log s_j and mu_j = e^{eta_j}, per gene
 *     P(beta) = sum_j [c_j log(alpha mu_j) - (c_j + 1/alpha) log1p(alpha mu_j)] - sum_{l != k} beta_l^2 / (2 sigma0^2)
 *               - log1p(beta_k^2 / S^2)
 * a Cauchy of scale S on beta_k and a normal of scale sigma0 on EVERY other coefficient, the intercept included (what lfcShrink hands
 * apeglm as no.shrink); no further ridge.  For X = [1, indicator] this is pilot_ot_nb_shrink's P(b0, b1).  The estimate is DEFINED by
 * that call's search: the profile p(b) = max over beta_{-k} of P at beta_k = b, over t in [0, asinh(E / S)] with b = sg S sinh t and
 * far_end[gene] = sg E (from pilot_ot_nb_design_fits' coefficient: sg its sign, + for 0, E = |beta_k| + 1; 1 for a gene left out), by six
 * rounds of the 64-point grid, the first largest value winning.  At every grid point the p - 1 other coefficients are fitted by the
 * Newton iteration of the inner fit above with the ridge 1 / sigma0^2 (to 1e-10, at most 100 steps): round 0 from beta_mle
 * (n_genes x p, that call's coefficients), a later round from the lane's own last point.  One wave per gene, a lane is a grid point;
 * no floating-point sum crosses lanes: a gene gives the same bits alone and in any batch.
 * Out (host): beta (n_genes x p, X's column order) at the winning point; objective = P there; info (n_genes x p (p + 1) / 2): the
 * upper triangle, row by row in X's column order, of X^T W X with w_j = mu_j (1 + alpha c_j) / (1 + alpha mu_j)^2; flags:
 * PILOT_OT_NB_NOT_CONVERGED (an inner fit did not converge), PILOT_OT_NB_AT_BOUND, and above PILOT_OT_NB_SHRINK_STEPS_SHIFT the
 * gene's inner Newton steps over all grid points and rounds; *n_at_bound (nullable).  A NaN dispersion, a gene of zeros or a
 * non-finite beta_mle in an unshrunk column leaves the gene out: NaN everywhere, flags 0.
 * PILOT_OT_EINVAL (before any HIP call): the cases of pilot_ot_nb_design_fits, coef outside [1, p - 1], a prior_scale or other_scale
 * not positive and finite, a non-finite far_end; after the check pass a negative or non-finite count (*bad_row / *bad_col as
 * pilot_ot_nb_dispersions).  PILOT_OT_ENOTSUP: m > INT_MAX; m > pilot_ot_nb_design_max_samples(p) (the staging of
 * pilot_ot_nb_design_dispersions). */
int pilot_ot_nb_design_shrink(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const double *X, int p,
                              int coef, const double *size_factors, const double *dispersion, const double *beta_mle,
                              const double *far_end, double prior_scale, double other_scale, double *beta, double *objective, double *info,
                              int *flags, int *n_at_bound, long long *bad_row, int *bad_col);

/* pilot_ot_nb_design_cooks (K28): pilot_ot_nb_cooks for the general design, the outlier handling of `DESeq(dds)` and `results(dds)`
 * after a fit with covariates.  THIS LIBRARY'S STATEMENT, unpinned (restated in tests/nb_design_cooks_restatement.py).
 * Y, X, p, size_factors as pilot_ot_nb_design_fits; dispersion: the gene's FINAL dispersion alpha (host; NaN leaves the gene out); beta:
 * n_genes x p, that call's coefficients at it; lambda = 1e-6, its ridge.  cells (host, m codes in [0, n_cells)): DESeq2's
 * nOrMoreInCell -- a cell is a maximal set of samples whose rows of X are bit-identical, numbered by first appearance; for
 * X = [1, indicator] the cells are pilot_ot_nb_cooks' groups, with a numeric covariate usually singletons.  With c, q_j, tm as there:
 *     trimmed_base = tm(q of all m samples, floor(m / 5))
 *     v = max over the cells of n >= 3 samples of pilot_ot_nb_cooks' v_g (the same r, scale and d by the cell's size);
 *         without such a cell v = 1.51 tm((q - tm(q, d))^2, d) over all samples, d = floor(m / 8) (DESeq2's trimmedVariance)
 *     alpha_robust = max((v - mean_j q_j) / (mean_j q_j)^2, 0.04)
 *     mu_j = max(s_j exp(x_j^T beta), minmu),  w_j = mu_j / (1 + alpha mu_j),  M = X^T W X + lambda I (the matrix whose inverse
 *     pilot_ot_nb_design_fits reports),  h_j = w_j x_j^T M^-1 x_j
 *     D_j = (c_j - mu_j)^2 / (mu_j + alpha_robust mu_j^2)  h_j / (p (1 - h_j)^2)      (h_j < 1 with the ridge: no NaN rule)
 *     max_cooks = max of D_j over the samples of cells with n >= 3; arg_max the lowest sample index that attains it;
 *     n_above = #{j: c_j > c_arg_max};  n_replace = #{j: D_j > cutoff and n_cell(j) >= min_replace}
 * Without a cell of n >= 3: max_cooks = NaN, arg_max = -1, n_above = 0, and no sample can be replaced or flagged; alpha_robust, D and H
 * are still computed.  A gene of zeros, with a NaN dispersion or a non-finite beta: NaN in every float result, arg_max = -1, counts 0.
 * One wave per gene; c and q staged in LDS in (cell, sample) order beside the bitonic sort buffer; a lane reads the rows of X of its
 * own samples from global memory; M as per-lane partials of the packed upper triangle closed by one fixed butterfly each, factored
 * and inverted in registers.  Same bits as stated above for the K22 calls, and for a gene alone or in any batch.
 * Out (host, n_genes): alpha_robust, max_cooks, arg_max, n_above, n_replace, trimmed_base.  D, H: nullable; m x n_genes float64 with
 * leading dimensions ld_D, ld_H >= n_genes, each on the host or in HBM (D_is_device, H_is_device): D[j, gene] = D_j, H[j, gene] = h_j.
 * PILOT_OT_EINVAL (before any HIP call): the cases of pilot_ot_nb_design_fits, a cutoff not positive and finite, min_replace < 3,
 * ld_D or ld_H < n_genes with that matrix, n_cells outside [1, m], a cell code outside [0, n_cells), a row of X that differs from the
 * first row of its cell, a cell without a sample, a non-finite beta where the gene's dispersion is not NaN; after the check pass a
 * negative or non-finite count (*bad_row / *bad_col as pilot_ot_nb_dispersions).  PILOT_OT_ENOTSUP: m > INT_MAX; m >
 * pilot_ot_nb_design_max_samples(p) (which keeps the LDS, 8 (2 m + P') bytes with P' the power of two >= m, within 96 KiB). */
int pilot_ot_nb_design_cooks(const void *Y, int Y_is_device, int dtype, long long m, int n_genes, long long ld, const double *X, int p,
                             const int *cells, int n_cells, const double *size_factors, const double *dispersion, const double *beta,
                             double cutoff, int min_replace, double *alpha_robust, double *max_cooks, int *arg_max, int *n_above,
                             int *n_replace, double *trimmed_base, void *D, int D_is_device, long long ld_D, void *H, int H_is_device,
                             long long ld_H, long long *bad_row, int *bad_col);

/* ---- principal components (K15): the PCA that pilotpy's extract_annot_expression(reduction=True) and reclustering_data take from
 * scanpy (tools/Trajectory.py:199-208, 1035-1044: scale(max_value) then tl.pca(svd_solver='arpack')), of a matrix that is never
 * standardised in memory.  Y: n rows x the n_sel selected columns (cols: host, distinct, any order; NULL: every column).
 * Per column, in f64 whatever the storage dtype: mu the mean, sigma = sqrt(m2 / (n - 1)) with 0 -> 1; scale = 1:
 * z = min((y - mu) / sigma, max_value), clipped on the upper side only (max_value = INFINITY: no clip); scale = 0: z = y
 * (max_value is only checked).  The columns of Z are centred again and the eigenpairs of Zc^T Zc come from a symmetric Lanczos run
 * with full re-orthogonalisation on the implicit operator v -> Zc^T (Zc v) (basis of min(n_sel, 1024) vectors, a fixed start
 * vector, every sum in f64 in a fixed order, no floating-point atomic: the same bits from every run and from float32 and float64
 * storage of the same values).
 * Out (host, f64), k = n_comps in [1, min(n - 1, n_sel - 1, 64)], largest eigenvalue first: scores n x k = Zc V; pcs n_sel x k = V;
 * variance[c] = lambda_c / (n - 1); variance_ratio[c] = variance[c] / the summed ddof-1 column variances of Z.  Sign: in every
 * component the score of largest magnitude (lowest row on ties) is positive.  info[0] = Lanczos steps, info[1] = PILOT_OT_PCA_*.
 * PILOT_OT_EINVAL (before any HIP call): a NULL pointer, scale not 0 / 1, max_value not positive, a column out of range or named
 * twice, n < 2, n_comps out of range, for the dense call dtype / ld / n_cols_total as in pilot_ot_group_moments; after the moments
 * pass: a non-finite value in a selected column.  PILOT_OT_ENOTSUP: n > INT_MAX. */
#define PILOT_OT_PCA_NOT_CONVERGED 1   /* the basis cap was reached before every wanted Ritz pair converged and a verification
                                        * block showed that no copy of a wanted eigenvalue is hidden */
#define PILOT_OT_PCA_RANK_DEFICIENT 2  /* the Krylov space ended before n_comps pairs, or a wanted lambda <= n_sel * DBL_EPSILON * lambda_0 */
/* of a sparse matrix: the forward product reads the row form, the transposed one the column form (built if need be) */
int pilot_ot_csr_pca(pilot_ot_csr *csr, const int *cols, int n_sel, int scale, double max_value, int n_comps, double *scores,
                     double *pcs, double *variance, double *variance_ratio, int *info);
/* of a dense row-major matrix (Y, Y_is_device, dtype, n, n_cols_total, ld: pilot_ot_group_moments's) */
int pilot_ot_pca(const void *Y, int Y_is_device, int dtype, long long n, int n_cols_total, long long ld, const int *cols, int n_sel,
                 int scale, double max_value, int n_comps, double *scores, double *pcs, double *variance, double *variance_ratio,
                 int *info);

/* ---- cell neighbours (K16): the exact k-nearest-neighbour graph of the rows of X (the cells of an embedding, n x D row-major,
 * X_is_device / dtype / ld as in pilot_ot_group_moments) and the per-row part of UMAP's fuzzy simplicial set -- what pilotpy takes
 * from scanpy's pp.neighbors (tools/Trajectory.py:217-220, 1045-1060).  The n x n distance matrix is never formed.
 * A squared distance is the direct sum over d of (x_d - y_d)^2 in the element type, d ascending; metric 0 (euclidean) returns its
 * IEEE square root, metric 1 (cosine) divides every row by its f64 norm first (quotient rounded to the element type) and returns
 * half the sum, 1 - cos for unit rows.  Row i itself is left out by index.  The neighbours of a row are ordered by (distance,
 * index) ascending; no atomics, the same call returns the same bits.  Every returned distance is within (D + 6) u relative of the
 * exact distance between the stored (for cosine: the normalised and rounded) values, u = 2^-24 / 2^-53.
 * Query rows row_begin .. row_end - 1; the corpus is always all n rows.  indices / distances: (row_end - row_begin) x k, host.
 * PILOT_OT_EINVAL (before any HIP call): a NULL pointer, D < 1, ld < D, dtype, metric, k < 1, n < k + 1, a row range that is empty
 * or not inside [0, n); after the flag pass: a non-finite value, or under cosine an all-zero row (the message names the first such
 * row).  PILOT_OT_ENOTSUP: k > PILOT_OT_KNN_ROWS_MAX_K, n > INT_MAX. */
#define PILOT_OT_KNN_ROWS_MAX_K 64
int pilot_ot_knn_rows(const void *X, int X_is_device, int dtype, long long n, int D, long long ld, int metric, int k,
                      long long row_begin, long long row_end, int *indices, double *distances);
/* distances: n x k (host, finite, >= 0), the distances of every cell to its k = n_neighbors - 1 neighbours.  Per row, in f64:
 * rho = the smallest non-zero distance (0: none); sigma = the value a bisection of at most 64 steps (start 1, doubling while no
 * upper end is known) reaches for sum_j exp(-max(0, d_j - rho) / sigma) = log2(k + 1) within 1e-5, then floored at 1e-3 x the row's
 * mean distance (rho > 0) or x the mean of all distances (rho = 0); weights[j] = 1 where d_j - rho <= 0 or sigma = 0, else
 * exp(-(d_j - rho) / sigma).  weights: n x k, sigma, rho: n (host).  Refusals as above (k, n, NULL; a distance not finite or < 0). */
int pilot_ot_knn_smooth(const double *distances, long long n, int k, double *weights, double *sigma, double *rho);

/* ---- Louvain communities (K17): the communities of the cell graph that pilotpy takes from sknetwork.clustering.Louvain(resolution)
 * on obsp['distances'] / ['connectivities'] (tools/Trajectory.py:217-220, 1050-1060), by a SYNCHRONOUS rule: deterministic, no seed,
 * parallel over nodes (restated in tests/louvain_restatement.py).  It is not sknetwork's sequential sweep.
 * A: n x n CSR on the host (indptr: n + 1 entries from 0), weights finite and >= 0, maybe unsymmetric; the columns of a row may be
 * unsorted or repeated (repeats add), stored zeros are dropped, diagonal entries are allowed.  out_i = sum_j A_ij, in_i = sum_j A_ji,
 * w = sum_i out_i, S = A + A^T.  Q = Qs / w^2 with Qs = (w / 2) sum_{c_i = c_j} S_ij - resolution sum_c Out_c In_c (Dugue-Perez
 * modularity; Newman's when A is symmetric).  A level starts from singletons; a sweep moves every node against one snapshot: node i
 * in X takes the community C != X among those of its stored neighbours j != i with the largest
 *     g(C) = w (k_C - k_X) - resolution (out_i (In_C - (In_X - in_i)) + in_i (Out_C - (Out_X - out_i))),  k_C = sum_{j in C, j != i} S_ij
 * (f64, every product and sum rounded on its own; ties to the lowest C) iff g > 0, except that a singleton never moves to a
 * singleton of higher id.  A sweep that moved nothing ends the level; otherwise it is kept iff Qs_new - Qs_kept > tol w^2, else
 * discarded and the level ends; at most 128 sweeps a level.  Then the surviving communities, ranked by id, become the nodes of the
 * next level (S' = P^T S P, out' / in' the member sums); the run ends when a level merges nothing or after max_levels levels.
 * Every sum has one fixed order and no floating-point atomic is used: the same call returns the same bits.
 * Out (host): labels n ints in 0 .. k-1, numbered by decreasing community size, ties to the smallest member; *modularity = Q of
 * them; info[0] = levels run, info[1] = sweeps run, info[2] = k.  n = 0 writes nothing but info and Q = 0; w = 0: every node its own
 * community, Q = 0, no level.  S goes up once; a level uploads nothing and brings back only its counters.
 * PILOT_OT_EINVAL (before any HIP call): a NULL pointer, n < 0, indptr not non-decreasing from 0, a column outside [0, n), a weight
 * negative or not finite (the message names the entry), resolution not finite or < 0, tol < 0, max_levels < 1, w^2 not finite.
 * PILOT_OT_ENOTSUP (before any HIP call): n > INT_MAX, or more than INT_MAX entries in S. */
int pilot_ot_louvain(long long n, const long long *indptr, const int *indices, const double *weights, double resolution, double tol,
                     int max_levels, int *labels, double *modularity, int *info /* 3 */);

/* ---- Leiden communities (K20): the clustering pilotpy runs on the samples (tools/Trajectory.py:527-588, plot/ploting.py:320-323,
 * 426-427), as Louvain above with Leiden's refinement under the same SYNCHRONOUS rule (restated in
 * tests/leiden_restatement.py), so that every returned community is connected in S.  It is not leidenalg: greedy instead of a random
 * choice, synchronous, and every level restarts from singletons.  Arguments, A, S, Q, the sum orders and the refusals are
 * pilot_ot_louvain's.  A level: (1) the move phase is a level of pilot_ot_louvain as it is, giving P with the totals OutP, InP; if
 * every community of P is one node the run ends, the level's nodes are the communities and Q = Qs(level start) / w^2.
 * (2) Refinement of P.  "Neighbour": a stored neighbour j != i with P_j = P_i.  Fixed for the level, i in X = P_i: e_i = sum S_ij
 * over its neighbours in stored order, node_ok_i = [w e_i - resolution (out_i (InP_X - in_i) + in_i (OutP_X - out_i)) >= 0].  R starts
 * as singletons and is swept like the move phase (at most 128 sweeps, kept iff Qs(R_new) - Qs(R_kept) > tol w^2, ended by a sweep
 * that moves nothing or is discarded).  Per snapshot (R, OutR, InR, sizeR): c_i = sum S_ij over the neighbours with R_j != R_i in
 * stored order, cut_T = sum of c_i over T's members ascending, sub_ok_T = [w cut_T - resolution (OutR_T (InP_X - InR_T) + InR_T
 * (OutP_X - OutR_T)) >= 0].  Node i decides only if sizeR[R_i] = 1 and node_ok_i; its candidates are the T != R_i that hold a
 * neighbour and have sub_ok_T, k_T summed over those neighbours in stored order, g(T) the g above with X = R_i (k_X = 0); largest g,
 * ties to the lowest T; it moves iff g > 0 and not (sizeR_T = 1 and T > R_i).  Settle: a move into a T of one member stands only
 * if that member did not itself decide to leave (read from the unsettled decisions, written to a separate array).  Every product
 * and sum is rounded on its own, in the order written.  (3) If R merged nothing the run ends as in (1); else R's sub-communities
 * become the next level's nodes by pilot_ot_louvain's aggregation; after level max_levels the run ends there with Q = Qs(R kept) /
 * w^2.  Only singletons move and a joiner has an edge to a member that stays, so every community is connected whatever the rounding.
 * Out: labels, *modularity as above; info[0] = levels, info[1] = move sweeps, info[2] = refinement sweeps, info[3] = k. */
int pilot_ot_leiden(long long n, const long long *indptr, const int *indices, const double *weights, double resolution, double tol,
                    int max_levels, int *labels, double *modularity, int *info /* 4 */);

/* ---- silhouette of labelled rows (K18): sklearn.metrics.silhouette_samples of the n rows of X (n x D row-major, X_is_device /
 * dtype / ld as in pilot_ot_knn_rows) under the labels codes[i] in 0 .. n_clusters - 1 -- the score pilotpy's select_best_sil
 * (plot/ploting.py:384-458) takes per resolution, at the cell level.  Neither the n x n distance matrix nor an n x n_clusters table
 * is formed.  The distances are pilot_ot_knn_rows's (metric 0 / 1 as there: direct sums of squared differences in the element
 * type; cosine from the rows normalised and rounded to the element type).  a_i = the mean distance from i to the other members of
 * its cluster (i left out by index, so copies of it count at distance 0), b_i = the smallest mean distance from i to the members
 * of another cluster, samples[i] = (b_i - a_i) / max(a_i, b_i); 0 when i's cluster has one member or max(a_i, b_i) = 0.  The rows
 * are ordered by (code, row) once; every per-cluster sum is float64, one add per member in ascending row order, no atomics: the
 * result does not depend on the launch geometry and the same call returns the same bits.  Every sample is within
 * 4 ((D + 6) u + n 2^-53) of the value the exact distances between the stored values give, u = 2^-24 / 2^-53.
 * samples: n doubles (host); *score: their mean, summed in ascending row order on the host.
 * PILOT_OT_EINVAL (before any HIP call): a NULL pointer, D < 1, ld < D, dtype, metric, n_clusters outside [2, n - 1], a code
 * outside [0, n_clusters), a code without rows; after the flag pass: a non-finite value, or under cosine an all-zero row (the
 * message names the first such row).  PILOT_OT_ENOTSUP: n > INT_MAX. */
int pilot_ot_silhouette_points(const void *X, int X_is_device, int dtype, long long n, int D, long long ld, int metric, const int *codes,
                             int n_clusters, double *samples, double *score);
/* the geometry of that kernel for D columns of `dtype`: query rows per block (one per lane) and corpus rows per staged LDS tile */
int pilot_ot_silhouette_points_geometry(int D, int dtype, int *queries_per_block, int *tile_rows);

/* ---- elastic principal tree (K19): what pilotpy's fit_pricipla_graph (plot/ploting.py:229-282) asks of ElPiGraph -- a tree of
 * nodes fitted to the n rows of X (n x D row-major, X_is_device / dtype / ld as in pilot_ot_knn_rows; D <= 64) and the pseudotime
 * of every row along it.  The growth of the tree is the caller's; these calls fit candidate trees, give the start its moments and
 * project the points.  Every sum has one fixed order that depends on n alone and no floating-point atomic is used: the same call
 * returns the same bits, and a candidate's results are the same bits alone and in any batch, from a host matrix and from HBM.
 *
 * pilot_ot_elastic_fit_batch fits B candidates of m nodes each.  Candidate b: start positions Y0[b] (m x D) and spring matrix
 * S[b] (m x m, symmetric).  At most max_iter times: every point goes to its nearest node (pilot_ot_knn_rows's distances -- direct
 * sums of squared differences in the element type, the nodes rounded to it -- ties to the lowest node); cnt_j / sum_j = the count
 * and the f64 sum of node j's points in ascending row order; (diag(cnt) / n + S) Y' = sum / n is solved by Cholesky;
 * change = max_j |Y'_j - Y_j| / |Y'_j - centre|; Y <- Y'; stop once change < eps.  One more partition of the final Y gives
 * counts (B x m), sums (B x m x D) and energy[b] = (the f64 mean squared distance of the points to their nodes, trace(Y^T S Y)).
 * iters[b]: the solves done.  flags[b]: PILOT_OT_ELASTIC_CONVERGED, or PILOT_OT_ELASTIC_SINGULAR when a pivot was not positive
 * (then Y[b] is the last iterate and energy[b] is NaN).
 * pilot_ot_point_moments: mean (D) = the column means, cross (D x D) = sum_i (x_i - mean)(x_i - mean)^T, f64.
 * pilot_ot_tree_projection: nodes (m x D), n_edges pairs edges[2 e] / edges[2 e + 1] = (a, b) with a the end nearer the source,
 * base[j] = the tree distance from the source to node j.  Row i: p = y_a + t (y_b - y_a), t clipped to [0, 1], on the edge with the
 * smallest f64 |x_i - p|^2 (ties to the lowest edge); pseudotime[i] = base[a] + t |y_b - y_a|, d2[i] = |x_i - p|^2, edge[i], t[i].
 * All outputs are host arrays.
 * PILOT_OT_EINVAL (before any HIP call): a NULL pointer, D outside [1, 64], ld < D, dtype, n < 1, m outside [2, 65], B < 1, a
 * non-finite Y0 / S / centre / nodes / base, max_iter < 1, eps < 0, n_edges outside [1, m - 1], an edge end outside [0, m); after
 * the flag pass: a non-finite value in X (the message names the first such row).  PILOT_OT_ENOTSUP: n > INT_MAX. */
#define PILOT_OT_ELASTIC_CONVERGED 1
#define PILOT_OT_ELASTIC_SINGULAR 2
#define PILOT_OT_ELASTIC_MAX_NODES 65
#define PILOT_OT_ELASTIC_MAX_D 64
int pilot_ot_elastic_fit_batch(const void *X, int X_is_device, int dtype, long long n, int D, long long ld, int B, int m,
                               const double *Y0, const double *S, const double *centre, int max_iter, double eps, double *Y,
                               double *energy, int *iters, int *flags, int *counts, double *sums);
int pilot_ot_point_moments(const void *X, int X_is_device, int dtype, long long n, int D, long long ld, double *mean, double *cross);
int pilot_ot_tree_projection(const void *X, int X_is_device, int dtype, long long n, int D, long long ld, int m, const double *nodes,
                             int n_edges, const int *edges, const double *base, double *pseudotime, double *d2, int *edge, double *t);

/* ---- cell-level W2 pair grid (EXTENSION: not in the reference; BASELINE config 5) ------ */
/* Compares patients by their raw cell clouds instead of cell-type proportions.  X: n_cells x D float32 embedding
 * with the cells of patient i stored contiguously at rows offsets[i] .. offsets[i+1] (offsets: N + 1 entries).
 * Pair (i, j): uniform weights 1/n_i, 1/n_j, cost C = |x - y|^2 / scale, entropic OT solved in the log domain with
 * the control flow of POT's ot.bregman.sinkhorn_log (v-update then u-update; marginal error every check_period
 * updates; stop on err < stop_thr, floored in f32 like the proportion-level kernel, or after num_iter_max updates);
 * the value is <Gamma, C>.  The n_i x n_j cost matrix is never materialised.  D <= 64; patients up to 13 637 cells.
 * PILOT_OT_ENOTSUP when a cell lies so far out that the f32 kernel would miss its 1e-5 relative accuracy:
 * max_i |x_i - mean(X)| * sqrt(2 log2(e) / (scale * reg)) > 50 (the Euclidean norm of the cell farthest from the mean).
 * w2 / iters / err: n_rows x N (iters, err nullable). */
int pilot_ot_cell_w2_grid(const float *X, const long long *offsets, int N, int D, double scale, double reg,
                          int num_iter_max, double stop_thr, int check_period, double f32_floor_ulps,
                          int row_begin, int row_end, int row_step, double *w2, int *iters, double *err);
/* Device-resident form: a cohort keeps the cells (as bf16 operand pieces) in HBM across calls, so a call moves only the
 * result rows.  kernel_ms (nullable): HIP-event time of the pair-grid kernel of this call. */
typedef struct pilot_ot_cell_cohort pilot_ot_cell_cohort;
int pilot_ot_cell_cohort_create(const float *X, const long long *offsets, int N, int D, pilot_ot_cell_cohort **cohort);
int pilot_ot_cell_cohort_destroy(pilot_ot_cell_cohort *cohort);
int pilot_ot_cell_cohort_pieces(pilot_ot_cell_cohort *cohort, int *pieces);   /* operand pieces per coordinate of the last call: 2 (fp16) | 3 (bf16) | 0 */
int pilot_ot_cell_w2_grid_cohort(pilot_ot_cell_cohort *cohort, double scale, double reg, int num_iter_max, double stop_thr,
                                 int check_period, double f32_floor_ulps, int row_begin, int row_end, int row_step,
                                 double *w2, int *iters, double *err, float *kernel_ms);
/* Full N x N grid, rows dealt round-robin over the listed devices (every device holds the cohort; the shards run
 * concurrently; the result rows are assembled on the host -- there is no device-side exchange step to make). */
int pilot_ot_cell_w2_grid_multi(const float *X, const long long *offsets, int N, int D, double scale, double reg,
                                int num_iter_max, double stop_thr, int check_period, double f32_floor_ulps,
                                const int *devices, int n_devices, double *w2, int *iters, double *err);

/* ---- transport plans (EXTENSION: not in the reference; POT's ot.emd / ot.sinkhorn return them, Trajectory.py keeps the values) */
/* Optimal couplings Gamma (K x K) of selected ordered pairs (i, j): rows = a = P[i], columns = b = P[j].
 * regularized 0: exact, the plan of ot.emd(a, b * sum(a) / sum(b), M) (POT's pre-step), solved by the pair grid's exact kernels
 *                (one wave per pair for K <= 256, one workgroup per pair above).  The LP's optimal VALUE is unique, its plan need
 *                not be: the plan returned is AN optimum, the one these kernels reach.
 *             1: entropic, ot.sinkhorn(a, b, M, reg, method="sinkhorn_stabilized") in f64, POT's loop step by step (the pair
 *                grid's PILOT_OT_PREC_GENERIC kernel), Gamma = exp(-(M - alpha_i - beta_j)/reg + log u_i + log v_j).
 *                A pair that hits num_iter_max returns the plan of its last iterate; a pair whose scalings went NaN returns
 *                the plan of its last good iterate, like POT; flags tell which, with the bits the pair grid reports.
 * pair_group == NULL: plans is n_pairs x K x K.  Otherwise plans is n_groups x K x K, the sum of the plans of the pairs of each
 * group (pair_group[t] in [0, n_groups)), added in list order in f64 (bit-reproducible; a group without pairs is 0).
 * values / iters / flags (nullable, n_pairs): what the pair grid returns for that pair -- <M, Gamma>; exact: iters = the
 * augmentations (negative, and the value NaN, if the solver's guard tripped: that pair's plan is not usable), flags = 0;
 * entropic: iterations and PILOT_OT_FLAG_* bits.  Pairs go through a device scratch of at most 1 GiB of plans at a time.
 * Argument errors are reported before the device is touched; K > 2048 -> PILOT_OT_ENOTSUP.  n_pairs = 0 writes nothing. */
int pilot_ot_transport_plans(const double *P, int N, int K, const double *M, int regularized, double reg,
                             int num_iter_max, double stop_thr, double tau, int check_period,
                             const int *pair_i, const int *pair_j, long long n_pairs,
                             const int *pair_group, int n_groups,
                             double *plans, double *values, int *iters, int *flags);

/* precision selected by PILOT_OT_PREC_AUTO for a given max(M)/reg (PILOT_OT_PREC_F16X2, PILOT_OT_PREC_BF16X3 or
 * PILOT_OT_PREC_F64; a shape whose split operand image does not fit LDS runs PILOT_OT_PREC_F32 instead) */
int pilot_ot_auto_precision(double max_cost_over_reg);
int pilot_ot_auto_precision_for(double max_cost_over_reg, int K, int cost_is_symmetric);   /* with the LDS fit of this K */
/* the precision a call with these arguments RUNS (every Sinkhorn entry point goes through it): GENERIC beyond
 * PILOT_OT_MAX_COST_OVER_REG; AUTO by range; an explicit f32-class precision (F32, BF16X3, F16X2) beyond the f32 range
 * (max(M)/reg > 60) runs AUTO_MIXED -- explicit precisions are honoured inside their valid range only; F16X2 outside its
 * scaled domain (max(M)/reg > 16 or tau > 2000) runs BF16X3. */
int pilot_ot_resolve_precision(int precision, double max_cost_over_reg, int K, int cost_is_symmetric, double tau);

#ifdef __cplusplus
}
#endif
#endif /* PILOT_OT_H */
