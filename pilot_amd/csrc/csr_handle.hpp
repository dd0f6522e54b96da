// The sparse matrix handle of the C ABI (include/pilot_ot.h, "sparse matrices"), shared by the translation units that read it:
// pilot_ot_csr.hip owns its life cycle and the column form, pilot_ot_group_sums.hip reads the row form, pilot_ot_pca.hip both.
// Host-side only.
#pragma once

struct pilot_ot_csr {
    long long n = 0, nnz = 0;
    int n_cols = 0, dtype = 0, device = 0;
    long long *indptr = nullptr;
    int *indices = nullptr;
    void *data = nullptr;
    // the column form: built by the first call that needs it, dropped when the values change
    bool columns = false;
    long long *colptr = nullptr;
    int *rowidx = nullptr;
    void *cdata = nullptr;
};
