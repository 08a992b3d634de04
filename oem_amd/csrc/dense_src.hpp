// dense_src.hpp -- where a dense x lies on the device, and every host-side "which layout?" decision (api.hip has the bodies).
#pragma once

#include "ctx.hpp"

namespace oemgpu {

// A column-major float64 x (dtype < 0, ld the column stride) or a row-major x of OEMGPU_F64 / OEMGPU_F32 elements read where it lies
// (ld the row stride).  What is computed from either is the same bytes for the same values.
struct DenseSrc {
    const void *x;
    int dtype;
    int64_t ld;
    bool colmajor() const { return dtype < 0; }
    const double *cm() const { return (const double *)x; }     // the column-major pointer
};
inline DenseSrc dense_src_cm(const double *x_dev, int64_t ld) { return DenseSrc{x_dev, -1, ld}; }
// (a caller's code below 0 is no element type and must not read as "column-major": it becomes a code that dense_src_check refuses)
inline DenseSrc dense_src_rm(const void *x_dev, int dtype, int64_t ldr) { return DenseSrc{x_dev, dtype < 0 ? INT32_MAX : dtype, ldr}; }

// the one rule of a source, before any device work: ld >= n (column-major); the dtype code, ldr >= p and the element's alignment (row-major)
int dense_src_check(const char *who, const DenseSrc &X, int64_t n, int32_t p);
// launch_shift_sums / launch_shift_sums_rm
int dense_src_shift_sums(hipStream_t s, const DenseSrc &X, int64_t n, int p, const double *y, double *sums);
// rows into fold order: launch_gather_rows / launch_gather_rows_rm.  Either way the copy is column-major float64
int dense_src_gather(hipStream_t s, const DenseSrc &X, int64_t n, int p, const double *y, const int32_t *foldid, int K, const int *pos,
                     double *xo, int64_t ldo, double *yo);
// the moment pass: gram.hip's plan or gram_rm.hip's, and the scratch either needs.  A row-major source with p > GRAM_RM_P_MAX is
// refused in `who`'s name (OEMGPU_ERR_UNSUPPORTED) before the context is looked at
struct MomentPlan {
    GramPlan cm{};          // filled for a column-major source,
    GramRmPlan rm{};        // for a row-major one; the other stays zero
    size_t scratch_bytes = 0;
};
int dense_src_moment_plan(const char *who, const oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, MomentPlan *pl);
// moments of the source into `moments` (overwrite): shard_moments, or its row-major counterpart
int dense_src_moments(oemgpu_ctx *c, const MomentPlan &pl, const DenseSrc &X, int64_t n, const double *y, const double *sums, char *scratch,
                      double *moments);

}  // namespace oemgpu
