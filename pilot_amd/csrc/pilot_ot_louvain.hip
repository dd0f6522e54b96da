// C ABI of the Louvain communities (include/pilot_ot.h, section "Louvain communities"; kernels and the rule: louvain_kernels.hpp).
// The host forms S = A + A^T once (transpose by counting sort, then a merge) and renumbers the labels at the end; everything
// between the two runs on the device: a level uploads nothing and brings back only its counters.  pilot_ot_leiden (K20) is the same
// run with a refinement between a level's move phase and its aggregation.  Run holds a call's device state and the steps of a level
// (layout, judge, sweep_phase<CON> for the move phase and the refinement, survivors, aggregate); run() is the level loop over them.
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

struct Run {                           // the device state of one run and the steps of a level: a step returns a count or 0, or a PILOT_OT_E* (< 0)
    DeviceLevel lev[2];
    int *comm, *next, *label, *wg_list, *long_list, *flag, *pos, *ecomm;      // comm: the level's kept assignment, next: a sweep's proposal
    Totals kept, fresh;                                                        // of comm and of next
    double *internal, *prod, *part_x, *part_y;
    lv_u64 *nkeys;
    LvEdge *ekeys;
    LvCounters *cnt, hc;                                                       // hc: the counters as last read back
    int *parent, *node_ok, *sub_ok, *owner, *raw, *spare_size;                 // K20: the move phase's partition and its totals, kept
    double *OutP, *InP, *cut_node, *cut, *spare_sum;                           // while the refinement runs through comm / next / kept / fresh
    double w, gamma, tol, qs_kept;                                             // qs_kept: Qs of comm
    int wave_max, wg_max, n_wg, n_long, wg_lds;                                // n_wg, n_long, wg_lds (bytes): what lv_bin_kernel found on the level

    // the workspace, slot by slot: its elements and first array, then the arrays that follow in it.  Slots, sizes and order are fixed
    int layout(int n, int nnz0, bool leiden) {
        const size_t N = (size_t)n, E = (size_t)nnz0, big = (size_t)std::max<long>(n, nnz0) + 1, chunks = (n + pilot::LV_CHUNK - 1) / pilot::LV_CHUNK;
        const pilot::WsSlot val_slot[2] = {pilot::WS_LV_VAL0, pilot::WS_LV_VAL1}, deg_slot[2] = {pilot::WS_LV_DEG0, pilot::WS_LV_DEG1},
                            idx_slot[2] = {pilot::WS_LV_IDX0, pilot::WS_LV_IDX1};
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(pilot::ws(val_slot[b], E, &lev[b].val));
            HIP_TRY(pilot::ws(deg_slot[b], 2 * N, &lev[b].out));
            HIP_TRY(pilot::ws(idx_slot[b], N + 1 + E, &lev[b].indptr));
            lev[b].in = lev[b].out + N, lev[b].col = lev[b].indptr + N + 1;
        }
        HIP_TRY(pilot::ws(pilot::WS_LV_TOT, 4 * N, &kept.Out));
        kept.In = kept.Out + N, fresh.Out = kept.In + N, fresh.In = fresh.Out + N;
        HIP_TRY(pilot::ws(pilot::WS_LV_SUMS, 2 * N + 2 * chunks, &internal));
        prod = internal + N, part_x = prod + N, part_y = part_x + chunks;
        HIP_TRY(pilot::ws(pilot::WS_LV_INT, 7 * N, &comm));
        next = comm + N, kept.size = next + N, fresh.size = kept.size + N, label = fresh.size + N, wg_list = label + N, long_list = wg_list + N;
        HIP_TRY(pilot::ws(pilot::WS_LV_FLAG, 2 * big, &flag));
        pos = flag + big;
        HIP_TRY(pilot::ws(pilot::WS_LV_ECOMM, E, &ecomm));
        HIP_TRY(pilot::ws(pilot::WS_LV_NKEYS, (size_t)pow2_at_least(n), &nkeys));
        HIP_TRY(pilot::ws(pilot::WS_LV_EKEYS, (size_t)pow2_at_least(nnz0), &ekeys));
        HIP_TRY(pilot::ws(pilot::WS_LV_CNT, 1, &cnt));
        if (!leiden) return PILOT_OT_OK;
        HIP_TRY(pilot::ws(pilot::WS_LD_INT, 6 * N, &parent));
        node_ok = parent + N, sub_ok = node_ok + N, owner = sub_ok + N, raw = owner + N, spare_size = raw + N;
        HIP_TRY(pilot::ws(pilot::WS_LD_DBL, 5 * N, &OutP));
        InP = OutP + N, cut_node = InP + N, cut = cut_node + N, spare_sum = cut + N;
        return PILOT_OT_OK;
    }

    // community totals of the assignment c into t, and its Qs into cnt->qs
    int judge(const LvGraph &G, const int *c, const Totals &t) {
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
    }

    // Sweeps until nothing moves, a sweep is discarded or LV_MAX_SWEEPS; leaves the kept assignment in comm / kept, its Qs in qs_kept, and
    // returns the sweeps run.  CON, the refinement: sub_ok first (the sorted node keys of comm are those judge left), raw decisions settled
    template <bool CON> int sweep_phase(const LvGraph &G) {
        const int m = G.m;
        const LvRefine R = CON ? LvRefine{parent, node_ok, sub_ok} : LvRefine{nullptr, nullptr, nullptr};
        const dim3 nodes(blocks_for(m)), waves(blocks_for(m, pilot::LV_THREADS / 64)), block(pilot::LV_THREADS);
        int sweeps = 0;
        while (sweeps < pilot::LV_MAX_SWEEPS) {
            const LvState S{comm, kept.Out, kept.In, kept.size};
            int *dest = CON ? raw : next;
            HIP_TRY(hipMemsetAsync(&cnt->moved, 0, sizeof(int), nullptr));
            if (CON) {
                hipLaunchKernelGGL(pilot::ld_cut_kernel, nodes, dim3(256), 0, nullptr, G, parent, comm, cut_node);
                hipLaunchKernelGGL(pilot::lv_runs_kernel, nodes, dim3(256), 0, nullptr, nkeys, m, cut_node, cut_node, cut, spare_sum, spare_size);
                hipLaunchKernelGGL(pilot::ld_sub_ok_kernel, nodes, dim3(256), 0, nullptr, nkeys, m, parent, OutP, InP, S, cut, w, gamma, sub_ok, owner);
            }
            hipLaunchKernelGGL(pilot::lv_move_wave_kernel<CON>, waves, block, 0, nullptr, G, S, R, w, gamma, wave_max, dest, cnt);
            if (n_wg > 0)
                hipLaunchKernelGGL(pilot::lv_move_wg_kernel<CON>, dim3((unsigned)n_wg), block, wg_lds, nullptr, G, S, R, w, gamma, wg_list, dest, cnt);
            if (n_long > 0)
                hipLaunchKernelGGL(pilot::lv_move_long_kernel<CON>, dim3((unsigned)n_long), block, 0, nullptr, G, S, R, w, gamma, long_list, ecomm,
                                   dest, cnt);
            if (CON) hipLaunchKernelGGL(pilot::ld_settle_kernel, nodes, dim3(256), 0, nullptr, m, comm, kept.size, owner, raw, next, cnt);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
            ++sweeps;
            if (hc.moved == 0) break;
            if (int rc = judge(G, next, fresh)) return rc;
            HIP_TRY(hipMemcpy(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
            if (!(hc.qs - qs_kept > tol * (w * w))) break;                     // discarded: the kept assignment stands
            qs_kept = hc.qs;
            std::swap(comm, next);
            std::swap(kept, fresh);
        }
        return sweeps;
    }

    // flags the ids that still have members, ranks them ascending into pos (and renames the labels of n_relabel nodes); returns their number
    int survivors(int m, int n_relabel = 0) {
        hipLaunchKernelGGL(pilot::lv_alive_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, kept.size, m, flag);
        hipLaunchKernelGGL(pilot::lv_scan_kernel, dim3(1), dim3(1024), 0, nullptr, flag, pos, (long)m, &cnt->coarse_m);
        if (n_relabel) hipLaunchKernelGGL(pilot::lv_relabel_kernel, dim3(blocks_for(n_relabel)), dim3(256), 0, nullptr, label, n_relabel, comm, pos);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
        return hc.coarse_m;
    }

    // aggregation; returns the coarse nodes.  Unless nothing merged or the level is the `last`, builds the coarse graph in nx, its entries in *nnz
    int aggregate(const LvGraph &G, int n, bool last, const DeviceLevel &nx, int *nnz) {
        const int m = G.m, m2 = survivors(m, n), nnz1 = *nnz;               // (n: the original nodes' labels are renamed with the ranks)
        if (m2 < 0 || m2 == m || last) return m2;
        const long P = pow2_at_least(nnz1), keys = std::max<long>(m, P - nnz1);
        hipLaunchKernelGGL(pilot::lv_coarse_nodes_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, m, kept.size, pos, kept.Out, kept.In, nx.out,
                           nx.in);
        hipLaunchKernelGGL(pilot::lv_edge_keys_kernel, dim3(blocks_for(keys)), dim3(256), 0, nullptr, G, comm, pos, nnz1, P, ekeys);
        HIP_TRY(device_sort(ekeys, P));
        hipLaunchKernelGGL(pilot::lv_edge_heads_kernel, dim3(blocks_for(nnz1)), dim3(256), 0, nullptr, ekeys, nnz1, flag);
        hipLaunchKernelGGL(pilot::lv_scan_kernel, dim3(1), dim3(1024), 0, nullptr, flag, ecomm, (long)nnz1, &cnt->coarse_nnz);   // (ecomm is free here)
        hipLaunchKernelGGL(pilot::lv_coarse_edges_kernel, dim3(blocks_for(nnz1)), dim3(256), 0, nullptr, ekeys, nnz1, flag, ecomm, G.val, m2,
                           &cnt->coarse_nnz, nx.indptr, nx.col, nx.val);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
        *nnz = hc.coarse_nnz;
        return m2;
    }
};

// the level loop.  info: levels, sweeps, communities; with `leiden` levels, move sweeps, refinement sweeps, communities
int run(int n, const HostGraph &h, double gamma, double tol, int max_levels, int wave_max, int wg_max, bool leiden, int *labels,
        double *modularity, int *info) {
    const int nnz0 = h.indptr[n];
    Run r{};
    r.w = h.w, r.gamma = gamma, r.tol = tol, r.wave_max = wave_max, r.wg_max = wg_max;
    if (int rc = r.layout(n, nnz0, leiden)) return rc;
    HIP_TRY(hipMemcpy(r.lev[0].indptr, h.indptr.data(), sizeof(int) * ((size_t)n + 1), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(r.lev[0].col, h.col.data(), sizeof(int) * (size_t)nnz0, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(r.lev[0].val, h.val.data(), sizeof(double) * (size_t)nnz0, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(r.lev[0].out, h.out.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(r.lev[0].in, h.in.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(pilot::lv_iota_kernel, dim3(blocks_for(n)), dim3(256), 0, nullptr, r.label, n);

    const size_t wg_lds_max = 16 * (size_t)pow2_at_least(wg_max);
    const void *wg_kernel[2] = {(const void *)pilot::lv_move_wg_kernel<false>, (const void *)pilot::lv_move_wg_kernel<true>};
    if (wg_lds_max > 64 * 1024)
        for (int con = 0; con <= (int)leiden; ++con)
            HIP_TRY(hipFuncSetAttribute(wg_kernel[con], hipFuncAttributeMaxDynamicSharedMemorySize, (int)wg_lds_max));
    int m = n, nnz = nnz0, cur = 0, levels = 0, sweeps = 0, refine_sweeps = 0, count;

    while (levels < max_levels) {
        const LvGraph G = r.lev[cur].graph(m);
        HIP_TRY(hipMemsetAsync(r.cnt, 0, sizeof(LvCounters), nullptr));
        hipLaunchKernelGGL(pilot::lv_iota_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, r.comm, m);
        hipLaunchKernelGGL(pilot::lv_bin_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, G.indptr, m, wave_max, wg_max, r.wg_list, r.long_list,
                           r.cnt);
        if (int rc = r.judge(G, r.comm, r.kept)) return rc;
        HIP_TRY(hipMemcpy(&r.hc, r.cnt, sizeof(r.hc), hipMemcpyDeviceToHost));
        const double qs_start = r.qs_kept = r.hc.qs;                            // Qs of the level's nodes as singletons
        r.n_wg = r.hc.n_wg, r.n_long = r.hc.n_long, r.wg_lds = 16 * (int)pow2_at_least(r.hc.max_wg_degree);
        ++levels;
        if ((count = r.sweep_phase<false>(G)) < 0) return count;
        sweeps += count;

        if (leiden) {
            if ((count = r.survivors(m)) < 0) return count;
            r.qs_kept = qs_start;                                               // the singletons' Qs again, whichever way it goes on
            if (count == m) break;                   // Leiden's end 1 of 2: every community of the move phase is one node, and the run ends
            // the refinement: the move phase's partition becomes the constraint, and the same loop runs from singletons again
            HIP_TRY(hipMemcpyAsync(r.parent, r.comm, sizeof(int) * (size_t)m, hipMemcpyDeviceToDevice, nullptr));
            HIP_TRY(hipMemcpyAsync(r.OutP, r.kept.Out, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, nullptr));
            HIP_TRY(hipMemcpyAsync(r.InP, r.kept.In, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, nullptr));
            hipLaunchKernelGGL(pilot::ld_node_ok_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, G, r.parent, r.OutP, r.InP, r.w, gamma, r.node_ok);
            hipLaunchKernelGGL(pilot::lv_iota_kernel, dim3(blocks_for(m)), dim3(256), 0, nullptr, r.comm, m);
            if (int rc = r.judge(G, r.comm, r.kept)) return rc;                 // (leaves the sorted node keys of comm in nkeys)
            if ((count = r.sweep_phase<true>(G)) < 0) return count;
            refine_sweeps += count;
        }

        const int m2 = r.aggregate(G, n, levels == max_levels, r.lev[cur ^ 1], &nnz);
        if (m2 < 0) return m2;
        if (leiden && m2 == m) r.qs_kept = qs_start;                            // Leiden's end 2 of 2: the refinement merged nothing; as end 1
        if (m2 == m || levels == max_levels) break;
        m = m2;
        cur ^= 1;
    }
    HIP_TRY(hipMemcpy(labels, r.label, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    info[0] = levels;
    info[1] = sweeps;
    if (leiden) info[2] = refine_sweeps;
    info[leiden ? 3 : 2] = renumber(n, labels);
    *modularity = r.qs_kept / (r.w * r.w);
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
