// Host steps shared by the entry points that run on K16's kernels (pilot_ot_knn.hip, pilot_ot_silhouette_points.hip).
#pragma once
#include <climits>

#include "abi_common.hpp"
#include "knn_kernels.hpp"

namespace pilot {

// K16's first pass over the n x D matrix *X (leading dimension *ld, in HBM): a non-finite value, or under cosine (metric 1) an
// all-zero row, is PILOT_OT_EINVAL naming the first such row.  Under cosine *X / *ld then become the packed unit rows, left in
// `unit_slot`.
template <typename T> int knn_checked_rows(const T **X, long long *ld, int n, int D, int metric, WsSlot flag_slot, WsSlot unit_slot) {
    hipStream_t s = nullptr;
    const unsigned row_grid = (unsigned)((n + 255) / 256);
    int *flags;
    const int none[2] = {INT_MAX, INT_MAX};
    int found[2];
    HIP_TRY(ws(flag_slot, 2, &flags));
    HIP_TRY(hipMemcpy(flags, none, sizeof(none), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(knn_check_kernel<T>, dim3(row_grid), dim3(256), 0, s, *X, *ld, n, D, metric, flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(found, flags, sizeof(found), hipMemcpyDeviceToHost));
    if (found[0] != INT_MAX)
        return fail(PILOT_OT_EINVAL, "row %d holds a non-finite value%s", found[0], metric == 1 ? " (or its sum of squares overflows)" : "");
    if (found[1] != INT_MAX) return fail(PILOT_OT_EINVAL, "row %d is all zero: its cosine distances are undefined", found[1]);
    if (metric == 1) {
        T *U;
        HIP_TRY(ws(unit_slot, (size_t)n * D, &U));
        hipLaunchKernelGGL(knn_normalize_kernel<T>, dim3(row_grid), dim3(256), 0, s, *X, *ld, n, D, U);
        *X = U;
        *ld = D;
    }
    return PILOT_OT_OK;
}

}  // namespace pilot
