// K14: per-group column sums of a cells x genes matrix for hundreds to a million groups -- the (cell type, sample) pseudobulk
// table the reference forms with counts_df.groupby(...).sum() on the densified matrix (plot/pseudobulk_DE_analysis.py:590-594).
// One pass over the used rows of Y, f64 accumulation, no floating-point atomic, a summation order fixed by (n, codes, GS_SLICE_ROWS)
// alone: the same bits from every run and from the host and device routes.
//
// Row order (host, pilot_ot_group_sums.hip): a stable counting sort of the used rows (code >= 0) by group gives `order`, the groups
// contiguous and the rows ascending within a group; a skipped row is in no list and is never read.  Every group is cut into slices
// of GS_SLICE_ROWS rows; slice s covers order[sbeg[s] .. sbeg[s + 1]).  sdst[s] >= 0: the slice is its group's only one and writes
// row sdst[s] of the result; sdst[s] < 0: it writes row -sdst[s] - 1 of the partials, and group_sums_join_kernel adds a group's
// partials IN SLICE ORDER, one thread per (multi-slice group, column).  Groups without rows keep the zeros the host put there.
//
// Dense: one wave per (slice, tile of GS_TILE columns); a lane owns GS_V consecutive columns and reads rows by K12's rules (one
// 16-byte load where there is no column list and rows are 16-byte aligned, scalar loads otherwise).  The row
// index is wave-uniform.  GS_R row loads are issued before the first is used; the rows are added one after another in list order.
// A gathered row is GS_TILE contiguous elements, so the permuted row order costs no coalescing.
//
// CSR: one wave per (slice, block of GS_COL_BLOCK selected columns), from the row form alone (the column form is never built).
// The wave walks its rows in list order; the lanes take one row's stored entries, GS_U batches of 64 loaded before the first is
// used, and an entry whose position lies in the block is added into the block's f64 accumulators in LDS by plain read-modify-write.
// Within a row the columns are distinct (upload refuses duplicates), so no two lanes of a row share an accumulator; a wave's LDS
// operations execute in program order and a wavefront-scope fence (no instruction) keeps the compiler from moving one row's
// accesses past the next row's, so every accumulator sees its rows in list order.  Entries outside the block are skipped.  With a column selection, pos[column] is
// the position of the column among the DISTINCT selected columns or -1 (the host copies a repeated column's sums afterwards).
// GS_COL_BLOCK = 2048 columns = 16 KiB of LDS per one-wave workgroup: ten workgroups fit the 160 KiB of a CU.  A smaller block
// means more waves in flight per CU and more column blocks that each walk the slice's entries; the two cancel for a full 20 000
// gene matrix, and a 2 000-gene selection is one block at ten waves per CU.
#pragma once
#include <hip/hip_runtime.h>

namespace pilot {

constexpr int GS_V = 4;                   // columns per lane (dense)
constexpr int GS_TILE = 64 * GS_V;        // columns per wave of the dense kernel
constexpr int GS_R = 8;                   // row loads in flight per lane (dense)
constexpr int GS_SLICE_ROWS = 256;        // rows per slice (pilot_ot_group_sums_slice_rows)
constexpr int GS_COL_BLOCK = 2048;        // selected columns per wave of the sparse kernel (pilot_ot_group_sums_col_block)
constexpr int GS_U = 4;                   // batches of 64 stored entries in flight per wave (sparse)
constexpr int GS_MAX_GROUPS = 1 << 20;

__device__ inline void gs_load4(const float *p, float (&o)[GS_V]) {
    const float4 v = *reinterpret_cast<const float4 *>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
__device__ inline void gs_load4(const double *p, double (&o)[GS_V]) {
    const double2 a = *reinterpret_cast<const double2 *>(p), b = *reinterpret_cast<const double2 *>(p + 2);
    o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
}

__device__ inline double *gs_row(int dst, long long n_sel, double *__restrict__ out, double *__restrict__ part) {
    return dst >= 0 ? out + (long long)dst * n_sel : part + (long long)(-dst - 1) * n_sel;
}

// Y: row-major, leading dimension ld.  order / sbeg / sdst: see above.  cols (nullable): the selected columns.  vec: rows may be
// read 16 bytes at a time.  Grid: n_slices * tiles one-wave workgroups, the tiles of a slice adjacent.
template <typename T>
__global__ void __launch_bounds__(64) group_sums_kernel(const T *__restrict__ Y, long long ld, const int *__restrict__ order,
                                                        const int *__restrict__ sbeg, const int *__restrict__ sdst,
                                                        const int *__restrict__ cols, int n_sel, int tiles, int vec,
                                                        double *__restrict__ out, double *__restrict__ part) {
    const int lane = threadIdx.x;
    const int slice = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int j0 = tile * GS_TILE + lane * GS_V;
    const int b = sbeg[slice], e = sbeg[slice + 1];
    const bool wide = vec && j0 + GS_V <= n_sel;
    long long cj[GS_V];                                    // this lane's columns; those past the end repeat the last one
#pragma unroll
    for (int v = 0; v < GS_V; ++v) {
        const int j = min(j0 + v, n_sel - 1);
        cj[v] = cols ? cols[j] : j;
    }
    double acc[GS_V] = {};
    for (int ib = b; ib < e; ib += GS_R) {
        T raw[GS_R][GS_V];
#pragma unroll
        for (int r = 0; r < GS_R; ++r) {                   // every load of the chunk is issued before the first use
            const int i = min(ib + r, e - 1);
            const T *row = Y + (long long)__builtin_amdgcn_readfirstlane(order[i]) * ld;
            if (wide) gs_load4(row + j0, raw[r]);
            else {
#pragma unroll
                for (int v = 0; v < GS_V; ++v) raw[r][v] = row[cj[v]];
            }
        }
#pragma unroll
        for (int r = 0; r < GS_R; ++r)
            if (ib + r < e) {                              // wave-uniform
#pragma unroll
                for (int v = 0; v < GS_V; ++v) acc[v] += (double)raw[r][v];
            }
    }
    double *dst = gs_row(sdst[slice], n_sel, out, part);
#pragma unroll
    for (int v = 0; v < GS_V; ++v)
        if (j0 + v < n_sel) dst[j0 + v] = acc[v];
}

// pos (nullable): column -> position among the n_sel distinct selected columns, or -1; NULL: position = column.  Grid: n_slices *
// blocks one-wave workgroups, the blocks of a slice adjacent.
template <typename T>
__global__ void __launch_bounds__(64) csr_group_sums_kernel(const long long *__restrict__ indptr, const int *__restrict__ indices,
                                                            const T *__restrict__ data, const int *__restrict__ order,
                                                            const int *__restrict__ sbeg, const int *__restrict__ sdst,
                                                            const int *__restrict__ pos, int n_sel, int blocks,
                                                            double *__restrict__ out, double *__restrict__ part) {
    __shared__ double acc[GS_COL_BLOCK];
    const int lane = threadIdx.x;
    const int slice = blockIdx.x / blocks, blk = blockIdx.x % blocks;
    const int c0 = blk * GS_COL_BLOCK;
    const unsigned width = (unsigned)min(GS_COL_BLOCK, n_sel - c0);
    for (unsigned k = lane; k < width; k += 64) acc[k] = 0.0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int b = sbeg[slice], e = sbeg[slice + 1];
    for (int i = b; i < e; ++i) {
        const int r = __builtin_amdgcn_readfirstlane(order[i]);
        const long long p1 = indptr[r + 1];
        for (long long p = indptr[r] + lane; p < p1; p += 64 * GS_U) {
            unsigned k[GS_U];
            T y[GS_U];
#pragma unroll
            for (int u = 0; u < GS_U; ++u) {               // every load of the GS_U batches is issued before the first use:
                const long long q = p + 64 * u;            // a batch past the row's end re-reads the row's last entry, unconditionally
                const long long qc = q < p1 ? q : p1 - 1;
                const int c = indices[qc];
                k[u] = q < p1 ? (unsigned)((pos ? pos[c] : c) - c0) : ~0u;      // -1 or a position below c0: past every width
                y[u] = data[qc];
            }
#pragma unroll
            for (int u = 0; u < GS_U; ++u)
                if (k[u] < width) acc[k[u]] += (double)y[u];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // this row's accumulator updates stay ahead of the next row's
    }
    double *dst = gs_row(sdst[slice], n_sel, out, part) + c0;
    for (unsigned k = lane; k < width; k += 64) dst[k] = acc[k];
}

// One thread per (multi-slice group, column): jgroup / jfirst / jcount name the group, its first partial row and how many follow.
__global__ void __launch_bounds__(256) group_sums_join_kernel(const double *__restrict__ part, const int *__restrict__ jgroup,
                                                              const int *__restrict__ jfirst, const int *__restrict__ jcount,
                                                              int n_join, int n_sel, double *__restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n_join * n_sel) return;
    const int m = (int)(t / n_sel), j = (int)(t % n_sel);
    const double *p = part + (long long)jfirst[m] * n_sel + j;
    const int k = jcount[m];
    double s = 0.0;
    for (int i = 0; i < k; ++i) s += p[(long long)i * n_sel];
    out[(long long)jgroup[m] * n_sel + j] = s;
}

}  // namespace pilot
