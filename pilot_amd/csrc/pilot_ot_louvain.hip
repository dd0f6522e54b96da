// C ABI of the Louvain communities (include/pilot_ot.h, section "Louvain communities"; kernels and the rule: louvain_kernels.hpp).
// The host forms S = A + A^T once (transpose by counting sort, then a merge) and renumbers the labels at the end; everything
// between the two runs on the device: a level uploads nothing and brings back only its counters.  pilot_ot_leiden (K20) is the same
// run with a refinement between a level's move phase and its aggregation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "abi_common.hpp"
#include "louvain_kernels.hpp"

namespace {

using pilot::LvCounters;
using pilot::LvEdge;
using pilot::LvGraph;
using pilot::LvRefine;
using pilot::LvState;
using pilot::lv_u64;

struct HostGraph {                     // S as CSR (columns ascending and distinct) with the directed weights of A
    std::vector<int> indptr, col;
    std::vector<double> val, out, in;
    double w = 0.0;
};

// rows of the transpose of the CSR (indptr, col, val) without its stored zeros: a counting sort by column, so the entries of a
// row of the result are in (source row, stored position) order
void transpose(long long n, const std::vector<long long> &indptr, const int *col, const double *val, std::vector<long long> &t_indptr,
               std::vector<int> &t_col, std::vector<double> &t_val) {
    t_indptr.assign((size_t)n + 1, 0);
    for (long long e = 0; e < indptr[n]; ++e)
        if (val[e] != 0.0) ++t_indptr[(size_t)col[e] + 1];
    for (long long j = 0; j < n; ++j) t_indptr[j + 1] += t_indptr[j];
    t_col.resize((size_t)t_indptr[n]);
    t_val.resize((size_t)t_indptr[n]);
    std::vector<long long> at(t_indptr.begin(), t_indptr.end() - 1);
    for (long long i = 0; i < n; ++i)
        for (long long e = indptr[i]; e < indptr[i + 1]; ++e)
            if (val[e] != 0.0) {
                const long long p = at[col[e]]++;
                t_col[p] = (int)i;
                t_val[p] = val[e];
            }
}

// S = A + A^T.  S_ij = (the stored A_ij added in stored order) + (the stored A_ji added in stored order); out_i / in_i add row i /
// column i of A in stored order, w adds out_0, out_1, ...  Returns false when S holds more than max_nnz entries.
bool form_symmetric(long long n, const long long *indptr, const int *indices, const double *weights, long long max_nnz, HostGraph &h) {
    std::vector<long long> a_indptr(indptr, indptr + n + 1), t_indptr, s_indptr;
    std::vector<int> t_col, s_col;
    std::vector<double> t_val, s_val;
    transpose(n, a_indptr, indices, weights, t_indptr, t_col, t_val);                   // A^T, rows sorted
    transpose(n, t_indptr, t_col.data(), t_val.data(), s_indptr, s_col, s_val);        // A again, rows sorted, zeros gone
    h.out.assign((size_t)n, 0.0);
    h.in.assign((size_t)n, 0.0);
    h.indptr.assign((size_t)n + 1, 0);
    h.col.clear();
    h.val.clear();
    h.w = 0.0;
    for (long long i = 0; i < n; ++i) {
        for (long long e = indptr[i]; e < indptr[i + 1]; ++e) h.out[i] += weights[e];
        for (long long e = t_indptr[i]; e < t_indptr[i + 1]; ++e) h.in[i] += t_val[e];
        h.w += h.out[i];
        long long a = s_indptr[i], b = t_indptr[i];
        const long long a_end = s_indptr[i + 1], b_end = t_indptr[i + 1];
        while (a < a_end || b < b_end) {
            const int ca = a < a_end ? s_col[a] : INT_MAX, cb = b < b_end ? t_col[b] : INT_MAX, c = std::min(ca, cb);
            double sa = 0.0, sb = 0.0;
            for (; a < a_end && s_col[a] == c; ++a) sa += s_val[a];
            for (; b < b_end && t_col[b] == c; ++b) sb += t_val[b];
            if ((long long)h.col.size() >= max_nnz) return false;
            h.col.push_back(c);
            h.val.push_back(sa + sb);
        }
        h.indptr[i + 1] = (int)h.col.size();
    }
    return true;
}

// labels 0 .. k-1 by decreasing size, ties to the smallest member; returns k
int renumber(long long n, int *labels) {
    int ids = 0;
    for (long long i = 0; i < n; ++i) ids = std::max(ids, labels[i] + 1);
    std::vector<long long> count((size_t)ids, 0), first((size_t)ids, -1);
    for (long long i = 0; i < n; ++i) {
        if (count[labels[i]]++ == 0) first[labels[i]] = i;
    }
    std::vector<int> order((size_t)ids), name((size_t)ids);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return count[a] != count[b] ? count[a] > count[b] : first[a] < first[b]; });
    for (int r = 0; r < ids; ++r) name[order[r]] = r;
    for (long long i = 0; i < n; ++i) labels[i] = name[labels[i]];
    return ids;
}

long pow2_at_least(long n) {
    long p = 2;
    while (p < n) p <<= 1;
    return p;
}

unsigned blocks_for(long n, int block = 256) { return (unsigned)std::max<long>(1, (n + block - 1) / block); }

// ascending bitonic sort of P = 2^x elements in HBM: the steps inside a tile of LV_SORT_TILE elements run in LDS
template <typename T> hipError_t device_sort(T *a, long P) {
    const int tile = (int)std::min<long>(P, pilot::LV_SORT_TILE);
    const size_t lds = sizeof(T) * (size_t)tile;
    const unsigned tiles = (unsigned)(P / tile);
    hipLaunchKernelGGL(pilot::lv_bitonic_tile_kernel<T>, dim3(tiles), dim3(pilot::LV_THREADS), lds, nullptr, a, tile, 2L, (long)tile);
    for (long k = 2L * tile; k <= P; k <<= 1) {
        for (long j = k >> 1; j >= tile; j >>= 1)
            hipLaunchKernelGGL(pilot::lv_bitonic_global_kernel<T>, dim3(blocks_for(P / 2)), dim3(256), 0, nullptr, a, P / 2, k, j);
        hipLaunchKernelGGL(pilot::lv_bitonic_tile_kernel<T>, dim3(tiles), dim3(pilot::LV_THREADS), lds, nullptr, a, tile, k, k);
    }
    return hipGetLastError();
}

struct DeviceLevel {                   // one of the two graph buffers
    int *indptr, *col;
    double *val, *out, *in;
    LvGraph graph(int m) const { return LvGraph{indptr, col, val, out, in, m}; }
};

struct Totals {                        // community totals of one assignment
    double *Out, *In;
    int *size;
};

// info: levels, sweeps, communities; with `leiden` levels, move sweeps, refinement sweeps, communities
int run(int n, const HostGraph &h, double gamma, double tol, int max_levels, int wave_max, int wg_max, bool leiden, int *labels,
        double *modularity, int *info) {
    const int nnz0 = h.indptr[n];
    const long big = std::max<long>(n, nnz0) + 1;
    const int chunks0 = (n + pilot::LV_CHUNK - 1) / pilot::LV_CHUNK;
    DeviceLevel lev[2];
    double *tot, *sums;
    int *ints, *flags, *ecomm;
    lv_u64 *nkeys;
    LvEdge *ekeys;
    LvCounters *cnt;
    const pilot::WsSlot val_slot[2] = {pilot::WS_LV_VAL0, pilot::WS_LV_VAL1}, deg_slot[2] = {pilot::WS_LV_DEG0, pilot::WS_LV_DEG1},
                        idx_slot[2] = {pilot::WS_LV_IDX0, pilot::WS_LV_IDX1};
    for (int b = 0; b < 2; ++b) {
        HIP_TRY(pilot::ws(val_slot[b], (size_t)nnz0, &lev[b].val));
        HIP_TRY(pilot::ws(deg_slot[b], 2 * (size_t)n, &lev[b].out));
        HIP_TRY(pilot::ws(idx_slot[b], (size_t)n + 1 + (size_t)nnz0, &lev[b].indptr));
        lev[b].in = lev[b].out + n;
        lev[b].col = lev[b].indptr + n + 1;
    }
    HIP_TRY(pilot::ws(pilot::WS_LV_TOT, 4 * (size_t)n, &tot));
    HIP_TRY(pilot::ws(pilot::WS_LV_SUMS, 2 * (size_t)n + 2 * (size_t)chunks0, &sums));
    HIP_TRY(pilot::ws(pilot::WS_LV_INT, 7 * (size_t)n, &ints));
    HIP_TRY(pilot::ws(pilot::WS_LV_FLAG, 2 * (size_t)big, &flags));
    HIP_TRY(pilot::ws(pilot::WS_LV_ECOMM, (size_t)nnz0, &ecomm));
    HIP_TRY(pilot::ws(pilot::WS_LV_NKEYS, (size_t)pow2_at_least(n), &nkeys));
    HIP_TRY(pilot::ws(pilot::WS_LV_EKEYS, (size_t)pow2_at_least(nnz0), &ekeys));
    HIP_TRY(pilot::ws(pilot::WS_LV_CNT, 1, &cnt));
    // K20: the move phase's partition and its totals, kept while its refinement runs through comm / next / kept / fresh
    int *parent = nullptr, *node_ok = nullptr, *sub_ok = nullptr, *owner = nullptr, *raw = nullptr, *spare_size = nullptr;
    double *OutP = nullptr, *InP = nullptr, *cut_node = nullptr, *cut = nullptr, *spare_sum = nullptr;
    if (leiden) {
        HIP_TRY(pilot::ws(pilot::WS_LD_INT, 6 * (size_t)n, &parent));
        HIP_TRY(pilot::ws(pilot::WS_LD_DBL, 5 * (size_t)n, &OutP));
        node_ok = parent + n, sub_ok = parent + 2 * (size_t)n, owner = parent + 3 * (size_t)n, raw = parent + 4 * (size_t)n;
        spare_size = parent + 5 * (size_t)n;
        InP = OutP + n, cut_node = OutP + 2 * (size_t)n, cut = OutP + 3 * (size_t)n, spare_sum = OutP + 4 * (size_t)n;
    }
    int *comm = ints, *next = ints + n, *label = ints + 4 * (size_t)n, *wg_list = ints + 5 * (size_t)n, *long_list = ints + 6 * (size_t)n;
    Totals kept{tot, tot + n, ints + 2 * (size_t)n}, fresh{tot + 2 * (size_t)n, tot + 3 * (size_t)n, ints + 3 * (size_t)n};
    double *internal = sums, *prod = sums + n, *part_x = sums + 2 * (size_t)n, *part_y = part_x + chunks0;
    int *flag = flags, *pos = flags + big;

    HIP_TRY(hipMemcpy(lev[0].indptr, h.indptr.data(), sizeof(int) * ((size_t)n + 1), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(lev[0].col, h.col.data(), sizeof(int) * (size_t)nnz0, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(lev[0].val, h.val.data(), sizeof(double) * (size_t)nnz0, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(lev[0].out, h.out.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(lev[0].in, h.in.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(pilot::lv_iota_kernel, dim3(blocks_for(n)), dim3(256), 0, nullptr, label, n);

    const double w = h.w, w2 = w * w;
    const size_t wg_lds_max = 16 * (size_t)pow2_at_least(wg_max);
    if (wg_lds_max > 64 * 1024) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pilot::lv_move_wg_kernel<false>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)wg_lds_max));
        if (leiden)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pilot::lv_move_wg_kernel<true>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)wg_lds_max));
    }
    int m = n, nnz = nnz0, cur = 0, levels = 0, sweeps = 0, refine_sweeps = 0;
    double qs_kept = 0.0;
    LvCounters hc;
    const LvRefine no_refine{nullptr, nullptr, nullptr};

    // community totals of the assignment c into t, and its Qs into cnt->qs
    auto judge = [&](const LvGraph &G, const int *c, const Totals &t) -> int {
        const long P = pow2_at_least(G.m);
        const int chunks = (G.m + pilot::LV_CHUNK - 1) / pilot::LV_CHUNK;
        hipLaunchKernelGGL(pilot::lv_node_keys_kernel, dim3(blocks_for(P)), dim3(256), 0, nullptr, c, G.m, P, nkeys);
        HIP_TRY(device_sort(nkeys, P));
        HIP_TRY(hipMemsetAsync(t.Out, 0, sizeof(double) * (size_t)G.m, nullptr));
        HIP_TRY(hipMemsetAsync(t.In, 0, sizeof(double) * (size_t)G.m, nullptr));
        HIP_TRY(hipMemsetAsync(t.size, 0, sizeof(int) * (size_t)G.m, nullptr));
        hipLaunchKernelGGL(pilot::lv_runs_kernel, dim3(blocks_for(G.m)), dim3(256), 0, nullptr, nkeys, G.m, G.out, G.in, t.Out, t.In, t.size);
        hipLaunchKernelGGL(pilot::lv_internal_kernel, dim3(blocks_for(G.m)), dim3(256), 0, nullptr, G, c, t.Out, t.In, internal, prod);
        hipLaunchKernelGGL(pilot::lv_chunk_sums_kernel, dim3(blocks_for(chunks)), dim3(256), 0, nullptr, internal, prod, G.m, part_x, part_y);
        hipLaunchKernelGGL(pilot::lv_qs_kernel, dim3(1), dim3(64), 0, nullptr, part_x, part_y, chunks, w, gamma, cnt);
        HIP_TRY(hipGetLastError());
        return PILOT_OT_OK;
    };

    while (levels < max_levels) {
        const LvGraph G = lev[cur].graph(m);
        HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(LvCounters), nullptr));
        hipLaunchKernelGGL(pilot::lv_iota_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, comm, m);
        hipLaunchKernelGGL(pilot::lv_bin_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, G.indptr, m, wave_max, wg_max, wg_list, long_list, cnt);
        if (int rc = judge(G, comm, kept)) return rc;
        HIP_TRY(hipMemcpy(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
        qs_kept = hc.qs;
        const int n_wg = hc.n_wg, n_long = hc.n_long;
        const size_t wg_lds = 16 * (size_t)pow2_at_least(hc.max_wg_degree);
        ++levels;
        const double qs_start = qs_kept;
        for (int s = 0; s < pilot::LV_MAX_SWEEPS; ++s) {
            const LvState S{comm, kept.Out, kept.In, kept.size};
            HIP_TRY(hipMemsetAsync(&cnt->moved, 0, sizeof(int), nullptr));
            hipLaunchKernelGGL(pilot::lv_move_wave_kernel<false>, dim3(blocks_for(m, pilot::LV_THREADS / 64)), dim3(pilot::LV_THREADS), 0, nullptr,
                               G, S, no_refine, w, gamma, wave_max, next, cnt);
            if (n_wg > 0)
                hipLaunchKernelGGL(pilot::lv_move_wg_kernel<false>, dim3((unsigned)n_wg), dim3(pilot::LV_THREADS), wg_lds, nullptr, G, S, no_refine,
                                   w, gamma, wg_list, next, cnt);
            if (n_long > 0)
                hipLaunchKernelGGL(pilot::lv_move_long_kernel<false>, dim3((unsigned)n_long), dim3(pilot::LV_THREADS), 0, nullptr, G, S, no_refine,
                                   w, gamma, long_list, ecomm, next, cnt);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
            ++sweeps;
            if (hc.moved == 0) break;
            if (int rc = judge(G, next, fresh)) return rc;
            HIP_TRY(hipMemcpy(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
            if (!(hc.qs - qs_kept > tol * w2)) break;                          // discarded: the kept assignment stands
            qs_kept = hc.qs;
            std::swap(comm, next);
            std::swap(kept, fresh);
        }

        if (leiden) {
            // every community of the move phase one node: the run ends, the level's nodes are the communities
            hipLaunchKernelGGL(pilot::lv_alive_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, kept.size, m, flag);
            hipLaunchKernelGGL(pilot::lv_scan_kernel, dim3(1), dim3(1024), 0, nullptr, flag, pos, (long)m, &cnt->coarse_m);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
            qs_kept = qs_start;
            if (hc.coarse_m == m) break;
            // the refinement: the move phase's partition becomes the constraint, and the same loop runs from singletons again
            HIP_TRY(hipMemcpyAsync(parent, comm, sizeof(int) * (size_t)m, hipMemcpyDeviceToDevice, nullptr));
            HIP_TRY(hipMemcpyAsync(OutP, kept.Out, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, nullptr));
            HIP_TRY(hipMemcpyAsync(InP, kept.In, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, nullptr));
            hipLaunchKernelGGL(pilot::ld_node_ok_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, G, parent, OutP, InP, w, gamma, node_ok);
            hipLaunchKernelGGL(pilot::lv_iota_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, comm, m);
            if (int rc = judge(G, comm, kept)) return rc;                       // (leaves the sorted node keys of comm in nkeys)
            const LvRefine R{parent, node_ok, sub_ok};
            for (int s = 0; s < pilot::LV_MAX_SWEEPS; ++s) {
                const LvState S{comm, kept.Out, kept.In, kept.size};
                HIP_TRY(hipMemsetAsync(&cnt->moved, 0, sizeof(int), nullptr));
                hipLaunchKernelGGL(pilot::ld_cut_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, G, parent, comm, cut_node);
                hipLaunchKernelGGL(pilot::lv_runs_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, nkeys, m, cut_node, cut_node, cut, spare_sum,
                                   spare_size);
                hipLaunchKernelGGL(pilot::ld_sub_ok_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, nkeys, m, parent, OutP, InP, S, cut, w, gamma,
                                   sub_ok, owner);
                hipLaunchKernelGGL(pilot::lv_move_wave_kernel<true>, dim3(blocks_for(m, pilot::LV_THREADS / 64)), dim3(pilot::LV_THREADS), 0,
                                   nullptr, G, S, R, w, gamma, wave_max, raw, cnt);
                if (n_wg > 0)
                    hipLaunchKernelGGL(pilot::lv_move_wg_kernel<true>, dim3((unsigned)n_wg), dim3(pilot::LV_THREADS), wg_lds, nullptr, G, S, R, w,
                                       gamma, wg_list, raw, cnt);
                if (n_long > 0)
                    hipLaunchKernelGGL(pilot::lv_move_long_kernel<true>, dim3((unsigned)n_long), dim3(pilot::LV_THREADS), 0, nullptr, G, S, R, w,
                                       gamma, long_list, ecomm, raw, cnt);
                hipLaunchKernelGGL(pilot::ld_settle_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, m, comm, kept.size, owner, raw, next, cnt);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpy(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
                ++refine_sweeps;
                if (hc.moved == 0) break;
                if (int rc = judge(G, next, fresh)) return rc;
                HIP_TRY(hipMemcpy(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
                if (!(hc.qs - qs_kept > tol * w2)) break;
                qs_kept = hc.qs;
                std::swap(comm, next);
                std::swap(kept, fresh);
            }
        }

        // aggregation: surviving ids ranked ascending
        int *rank = pos;
        hipLaunchKernelGGL(pilot::lv_alive_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, kept.size, m, flag);
        hipLaunchKernelGGL(pilot::lv_scan_kernel, dim3(1), dim3(1024), 0, nullptr, flag, rank, (long)m, &cnt->coarse_m);
        hipLaunchKernelGGL(pilot::lv_relabel_kernel, dim3(blocks_for(n)), dim3(256), 0, nullptr, label, n, comm, rank);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
        const int m2 = hc.coarse_m;
        if (leiden && m2 == m) qs_kept = qs_start;                              // the refinement merged nothing: the run ends as above
        if (m2 == m || levels == max_levels) break;
        const DeviceLevel &nx = lev[cur ^ 1];
        const long P = pow2_at_least(nnz);
        hipLaunchKernelGGL(pilot::lv_coarse_nodes_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, m, kept.size, rank, kept.Out, kept.In, nx.out,
                           nx.in);
        hipLaunchKernelGGL(pilot::lv_edge_keys_kernel, dim3(blocks_for(std::max<long>(m, P - nnz))), dim3(256), 0, nullptr, G, comm, rank, nnz, P,
                           ekeys);
        HIP_TRY(device_sort(ekeys, P));
        int *epos = ecomm;                                                      // (rank lives in pos; ecomm is free between sweeps)
        hipLaunchKernelGGL(pilot::lv_edge_heads_kernel, dim3(blocks_for(nnz)), dim3(256), 0, nullptr, ekeys, nnz, flag);
        hipLaunchKernelGGL(pilot::lv_scan_kernel, dim3(1), dim3(1024), 0, nullptr, flag, epos, (long)nnz, &cnt->coarse_nnz);
        hipLaunchKernelGGL(pilot::lv_coarse_edges_kernel, dim3(blocks_for(nnz)), dim3(256), 0, nullptr, ekeys, nnz, flag, epos, G.val, m2,
                           &cnt->coarse_nnz, nx.indptr, nx.col, nx.val);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
        m = m2;
        nnz = hc.coarse_nnz;
        cur ^= 1;
    }
    HIP_TRY(hipMemcpy(labels, label, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    info[0] = levels;
    info[1] = sweeps;
    if (leiden) info[2] = refine_sweeps;
    info[leiden ? 3 : 2] = renumber(n, labels);
    *modularity = qs_kept / w2;
    return PILOT_OT_OK;
}

// both entry points: the argument checks, the n = 0 and w = 0 cases and the refusals, all before any HIP call; then the run
int communities(long long n, const long long *indptr, const int *indices, const double *weights, double resolution, double tol, int max_levels,
                bool leiden, int *labels, double *modularity, int *info) {
    const int k_slot = leiden ? 3 : 2;
    if (!indptr || !indices || !weights || !labels || !modularity || !info) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (n < 0) return fail(PILOT_OT_EINVAL, "n=%lld nodes", n);
    if (!std::isfinite(resolution) || resolution < 0.0) return fail(PILOT_OT_EINVAL, "resolution=%g must be finite and not negative", resolution);
    if (!(tol >= 0.0)) return fail(PILOT_OT_EINVAL, "tol=%g must not be negative", tol);
    if (max_levels < 1) return fail(PILOT_OT_EINVAL, "max_levels=%d must be at least 1", max_levels);
    if (n > INT_MAX) return fail(PILOT_OT_ENOTSUP, "n=%lld nodes need more than 32-bit node indices", n);
    if (indptr[0] != 0) return fail(PILOT_OT_EINVAL, "indptr[0]=%lld must be 0", indptr[0]);
    for (long long i = 0; i < n; ++i)
        if (indptr[i + 1] < indptr[i]) return fail(PILOT_OT_EINVAL, "indptr[%lld]=%lld is below indptr[%lld]=%lld", i + 1, indptr[i + 1], i, indptr[i]);
    for (long long i = 0; i < n; ++i)
        for (long long e = indptr[i]; e < indptr[i + 1]; ++e) {
            if (indices[e] < 0 || indices[e] >= n) return fail(PILOT_OT_EINVAL, "indices[%lld]=%d (row %lld) outside [0, %lld)", e, indices[e], i, n);
            if (!(weights[e] >= 0.0) || std::isinf(weights[e]))
                return fail(PILOT_OT_EINVAL, "weights[%lld]=%g (row %lld, column %d) must be finite and not negative", e, weights[e], i, indices[e]);
        }
    for (int s = 0; s <= k_slot; ++s) info[s] = 0;
    *modularity = 0.0;
    if (n == 0) return PILOT_OT_OK;

    long long max_nnz = INT_MAX;
    if (const char *sw = pilot::test_switch("PILOT_OT_LOUVAIN_MAX_NNZ")) {      // (tests: the refusal without 2^31 entries)
        const long long v = atoll(sw);
        if (v > 0 && v < max_nnz) max_nnz = v;
    }
    HostGraph h;
    if (!form_symmetric(n, indptr, indices, weights, max_nnz, h))
        return fail(PILOT_OT_ENOTSUP, "A + A^T holds more than %lld entries: they need more than 32-bit edge indices", max_nnz);
    if (!std::isfinite(h.w * h.w)) return fail(PILOT_OT_EINVAL, "the squared total weight %g^2 overflows", h.w);
    if (h.w == 0.0) {                                                           // no weight: every node its own community, Q = 0
        for (long long i = 0; i < n; ++i) labels[i] = (int)i;
        info[k_slot] = (int)n;
        return PILOT_OT_OK;
    }
    int wave_max = pilot::LV_WAVE_MAX, wg_max = pilot::LV_WG_MAX;
    if (const char *sw = pilot::test_switch("PILOT_OT_LOUVAIN_BINS")) {         // (tests: all three move kernels on a small graph)
        int a = 0, b = 0;
        if (sscanf(sw, "%d,%d", &a, &b) == 2) {
            wave_max = std::min(std::max(a, 0), pilot::LV_WAVE_MAX);
            wg_max = std::min(std::max(b, wave_max), pilot::LV_WG_MAX);
        }
    }
    return run((int)n, h, resolution, tol, max_levels, wave_max, wg_max, leiden, labels, modularity, info);
}

}  // namespace

PILOT_API int pilot_ot_louvain(long long n, const long long *indptr, const int *indices, const double *weights, double resolution, double tol,
                               int max_levels, int *labels, double *modularity, int *info) {
    return communities(n, indptr, indices, weights, resolution, tol, max_levels, false, labels, modularity, info);
}

PILOT_API int pilot_ot_leiden(long long n, const long long *indptr, const int *indices, const double *weights, double resolution, double tol,
                              int max_levels, int *labels, double *modularity, int *info) {
    return communities(n, indptr, indices, weights, resolution, tol, max_levels, true, labels, modularity, info);
}
