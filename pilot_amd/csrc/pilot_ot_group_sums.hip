// C ABI of the per-group column sums (include/pilot_ot.h, section "group sums"; kernels: group_sums_kernels.hpp).  Y is a host array
// (copied whole, packed), a row-major buffer in HBM with its own leading dimension, or a sparse handle's row form; codes, cols and
// the results are host arrays.  The row lists the kernels walk are made here, on the host: O(n) on int32.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <vector>

#include "abi_common.hpp"
#include "csr_handle.hpp"
#include "group_sums_kernels.hpp"

namespace {

// The used rows sorted stably by group and cut into slices (group_sums_kernels.hpp, "Row order").  ints: what the kernels read,
// one array so that one copy takes it up: order[n_used] | sbeg[n_slices + 1] | sdst[n_slices] | jgroup | jfirst | jcount [n_join],
// then `extra` ints of the caller's (the column list or the column -> position map).
struct Plan {
    std::vector<int> ints;
    int n_used = 0, n_slices = 0, n_part = 0, n_join = 0;
    size_t o_sbeg = 0, o_sdst = 0, o_join = 0, o_extra = 0;
};

// count[g] and the plan; PILOT_OT_EINVAL for a code >= n_groups.  No HIP call.
int make_plan(const int *codes, long long n, int n_groups, long long *count, size_t extra, Plan *pl) {
    if (n > INT_MAX) return fail(PILOT_OT_ENOTSUP, "n=%lld rows need more than 32-bit row indices", n);
    for (int g = 0; g < n_groups; ++g) count[g] = 0;
    for (long long i = 0; i < n; ++i) {
        if (codes[i] >= n_groups)
            return fail(PILOT_OT_EINVAL, "codes[%lld]=%d: a code is negative (row skipped) or below n_groups=%d", i, codes[i], n_groups);
        if (codes[i] >= 0) ++count[codes[i]];
    }
    const long long L = pilot::GS_SLICE_ROWS;
    long long used = 0, slices = 0, parts = 0, joins = 0;
    for (int g = 0; g < n_groups; ++g) {
        const long long k = (count[g] + L - 1) / L;
        used += count[g];
        slices += k;
        if (k > 1) { parts += k; ++joins; }
    }
    pl->n_used = (int)used; pl->n_slices = (int)slices; pl->n_part = (int)parts; pl->n_join = (int)joins;
    pl->o_sbeg = (size_t)used;
    pl->o_sdst = pl->o_sbeg + (size_t)slices + 1;
    pl->o_join = pl->o_sdst + (size_t)slices;
    pl->o_extra = pl->o_join + 3 * (size_t)joins;
    pl->ints.assign(pl->o_extra + extra, 0);
    int *order = pl->ints.data(), *sbeg = order + pl->o_sbeg, *sdst = order + pl->o_sdst;
    int *jgroup = order + pl->o_join, *jfirst = jgroup + joins, *jcount = jfirst + joins;
    std::vector<int> cursor((size_t)n_groups);
    int at = 0, s = 0, p = 0, j = 0;
    for (int g = 0; g < n_groups; ++g) {
        cursor[g] = at;
        const int k = (int)((count[g] + L - 1) / L);
        if (k > 1) { jgroup[j] = g; jfirst[j] = p; jcount[j] = k; ++j; }
        for (int q = 0; q < k; ++q, ++s) {
            sbeg[s] = at + q * (int)L;
            sdst[s] = k == 1 ? g : -(p++) - 1;
        }
        at += (int)count[g];
    }
    sbeg[s] = at;
    for (long long i = 0; i < n; ++i)
        if (codes[i] >= 0) order[cursor[codes[i]]++] = (int)i;
    return PILOT_OT_OK;
}

struct DevPlan {
    const int *order, *sbeg, *sdst, *extra;
    double *out, *part;
};

// The plan's arrays and zeroed results (n_groups x n_sel) on the device; `launch` enqueues the slice kernel; then the join and the
// download into sum.
template <typename Launch>
int run(const Plan &pl, int n_groups, int n_sel, int per_slice, double *sum, Launch launch) {
    const long long grid = (long long)pl.n_slices * per_slice;
    if (grid > INT_MAX) return fail(PILOT_OT_ENOTSUP, "%d slices x %d column tiles exceed the grid", pl.n_slices, per_slice);
    int *d_ints;
    HIP_TRY(pilot::ws(pilot::WS_GS_AUX, pl.ints.size(), &d_ints));
    HIP_TRY(hipMemcpy(d_ints, pl.ints.data(), sizeof(int) * pl.ints.size(), hipMemcpyHostToDevice));
    const size_t n_out = (size_t)n_groups * n_sel;
    DevPlan d;
    d.order = d_ints; d.sbeg = d_ints + pl.o_sbeg; d.sdst = d_ints + pl.o_sdst; d.extra = d_ints + pl.o_extra;
    HIP_TRY(pilot::ws(pilot::WS_GS_OUT, n_out, &d.out));
    HIP_TRY(pilot::ws(pilot::WS_GS_PART, (size_t)pl.n_part * n_sel, &d.part));
    HIP_TRY(hipMemsetAsync(d.out, 0, sizeof(double) * n_out, nullptr));
    launch(d, (unsigned)grid);
    HIP_TRY(hipGetLastError());
    if (pl.n_join > 0) {
        const int *jgroup = d_ints + pl.o_join;
        const size_t n_t = (size_t)pl.n_join * n_sel;
        hipLaunchKernelGGL(pilot::group_sums_join_kernel, dim3((unsigned)((n_t + 255) / 256)), dim3(256), 0, nullptr, d.part, jgroup,
                           jgroup + pl.n_join, jgroup + 2 * (size_t)pl.n_join, pl.n_join, n_sel, d.out);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpy(sum, d.out, sizeof(double) * n_out, hipMemcpyDeviceToHost));
    return PILOT_OT_OK;
}

int check_groups(int n_groups) {
    if (n_groups < 1 || n_groups > pilot::GS_MAX_GROUPS)
        return fail(PILOT_OT_EINVAL, "n_groups=%d must be in [1, %d]", n_groups, pilot::GS_MAX_GROUPS);
    return PILOT_OT_OK;
}

}  // namespace

PILOT_API int pilot_ot_group_sums_slice_rows(void) { return pilot::GS_SLICE_ROWS; }
PILOT_API int pilot_ot_group_sums_col_block(void) { return pilot::GS_COL_BLOCK; }

PILOT_API int pilot_ot_group_sums(const void *Y, int Y_is_device, int dtype, long long n, int n_cols_total, long long ld, const int *codes,
                                  int n_groups, const int *cols, int n_cols, long long *count, double *sum) {
    if (!Y || !count || !sum || (!codes && n > 0)) return fail(PILOT_OT_EINVAL, "NULL pointer");
    if (n < 0 || n_cols_total < 1) return fail(PILOT_OT_EINVAL, "n=%lld, n_cols_total=%d", n, n_cols_total);
    if (int rc = pilot::check_ld(ld, n_cols_total)) return rc;
    if (int rc = pilot::check_dtype(dtype)) return rc;
    if (int rc = check_groups(n_groups)) return rc;
    if (int rc = pilot::check_cols(cols, n_cols, n_cols_total)) return rc;
    Plan pl;
    if (int rc = make_plan(codes, n, n_groups, count, cols ? (size_t)n_cols : 0, &pl)) return rc;
    if (n_cols == 0) return PILOT_OT_OK;
    if (pl.n_used == 0) {
        std::fill(sum, sum + (size_t)n_groups * n_cols, 0.0);
        return PILOT_OT_OK;
    }
    if (cols) std::copy(cols, cols + n_cols, pl.ints.begin() + pl.o_extra);
    const size_t es = pilot::elem_size(dtype);
    const void *y;
    long long y_ld;
    if (int rc = pilot::stage_dense(Y, Y_is_device, es, n, n_cols_total, ld, pilot::WS_GS_Y, &y, &y_ld)) return rc;
    // 16-byte row reads: every row start and every lane's first column on a 16-byte boundary
    const int vec = !cols && y_ld % (long long)(16 / es) == 0 && reinterpret_cast<uintptr_t>(y) % 16 == 0;
    const int tiles = (n_cols + pilot::GS_TILE - 1) / pilot::GS_TILE;
    return run(pl, n_groups, n_cols, tiles, sum, [&](const DevPlan &d, unsigned grid) {
        const int *d_cols = cols ? d.extra : nullptr;
        if (dtype == 0)
            hipLaunchKernelGGL(pilot::group_sums_kernel<float>, dim3(grid), dim3(64), 0, nullptr, static_cast<const float *>(y), y_ld, d.order,
                               d.sbeg, d.sdst, d_cols, n_cols, tiles, vec, d.out, d.part);
        else
            hipLaunchKernelGGL(pilot::group_sums_kernel<double>, dim3(grid), dim3(64), 0, nullptr, static_cast<const double *>(y), y_ld, d.order,
                               d.sbeg, d.sdst, d_cols, n_cols, tiles, vec, d.out, d.part);
    });
}

PILOT_API int pilot_ot_csr_group_sums(pilot_ot_csr *c, const int *codes, int n_groups, const int *cols, int n_cols, long long *count,
                                      double *sum) {
    if (int rc = check_groups(n_groups)) return rc;
    if (n_cols < 0) return fail(PILOT_OT_EINVAL, "n_cols=%d", n_cols);
    if (!c || !count || !sum || (!codes && c->n > 0)) return fail(PILOT_OT_EINVAL, "NULL pointer (csr, codes, count or sum)");
    if (int rc = pilot::check_cols(cols, n_cols, c->n_cols)) return rc;
    Plan pl;
    if (int rc = make_plan(codes, c->n, n_groups, count, cols ? (size_t)c->n_cols : 0, &pl)) return rc;
    if (n_cols == 0) return PILOT_OT_OK;
    if (pl.n_used == 0) {
        std::fill(sum, sum + (size_t)n_groups * n_cols, 0.0);
        return PILOT_OT_OK;
    }
    // a column list: the device sums the DISTINCT selected columns, at the position of their first mention among them; a column named
    // again takes a copy of those sums here
    int n_sel = n_cols;
    std::vector<int> where;                                // position among the distinct columns of every cols[j]
    if (cols) {
        int *pos = pl.ints.data() + pl.o_extra;
        std::fill(pos, pos + c->n_cols, -1);
        where.resize((size_t)n_cols);
        n_sel = 0;
        for (int j = 0; j < n_cols; ++j) {
            if (pos[cols[j]] < 0) pos[cols[j]] = n_sel++;
            where[j] = pos[cols[j]];
        }
    }
    std::vector<double> distinct;
    double *dst = sum;
    if (n_sel != n_cols) {
        distinct.resize((size_t)n_groups * n_sel);
        dst = distinct.data();
    }
    const int blocks = (n_sel + pilot::GS_COL_BLOCK - 1) / pilot::GS_COL_BLOCK;
    const int rc = run(pl, n_groups, n_sel, blocks, dst, [&](const DevPlan &d, unsigned grid) {
        const int *d_pos = cols ? d.extra : nullptr;
        if (c->dtype == 0)
            hipLaunchKernelGGL(pilot::csr_group_sums_kernel<float>, dim3(grid), dim3(64), 0, nullptr, c->indptr, c->indices,
                               static_cast<const float *>(c->data), d.order, d.sbeg, d.sdst, d_pos, n_sel, blocks, d.out, d.part);
        else
            hipLaunchKernelGGL(pilot::csr_group_sums_kernel<double>, dim3(grid), dim3(64), 0, nullptr, c->indptr, c->indices,
                               static_cast<const double *>(c->data), d.order, d.sbeg, d.sdst, d_pos, n_sel, blocks, d.out, d.part);
    });
    if (rc != PILOT_OT_OK) return rc;
    if (n_sel != n_cols)
        for (int g = 0; g < n_groups; ++g)
            for (int j = 0; j < n_cols; ++j) sum[(size_t)g * n_cols + j] = distinct[(size_t)g * n_sel + where[j]];
    return PILOT_OT_OK;
}
