// multi.hpp -- many responses on one dense x (multi.hip): the plan of the X'Y pass and its launches; the driver is api.hip's fit_dense_multi_src.
#pragma once

#include "common.hpp"
#include "dense_src.hpp"

namespace oemgpu {

constexpr int MULTI_ROWS = 64;               // rows of one block of 16 k-steps; a row chunk is a multiple of it
constexpr int MULTI_NW = 4;                  // waves per workgroup,
constexpr int MULTI_CPW = 2;                 // 16-column tiles of [X | 1] per wave: a workgroup covers MULTI_NW * MULTI_CPW * 16 = 128 columns

// Y as the caller gave it: element (i, r) at y[i * rs + r * cs]
struct MultiY {
    const double *y;
    int64_t rs, cs;
};

// the one rule of Y's strides (the many-response entries refuse anything else before a device is looked for)
inline int multi_y_check(const char *who, int64_t n, int64_t rs, int64_t cs, int32_t m)
{
    if (m < 1) { set_error("%s: m < 1 (at least one response)", who); return OEMGPU_ERR_ARG; }
    if (!((cs == 1 && rs >= m) || (rs == 1 && cs >= n))) {
        set_error("%s: y strides (%lld, %lld) are neither a row-major n x m matrix (y_cs == 1, y_rs >= m) nor a column-major one (y_rs == 1, y_cs >= n)",
                  who, (long long)rs, (long long)cs);
        return OEMGPU_ERR_ARG;
    }
    return 0;
}

// The X'Y pass as pure host arithmetic (oemgpu_selftest_multi_plan): rows are cut into `nchunk` chunks of `rows` rows (a multiple of
// 64; the last may be short, none is empty), the responses into `npass` blocks of mb = 16 lt, the columns of [X | 1] into `cgroups`
// groups of 128; workgroup (chunk, group, block) writes its part of the chunk's (p + 2) x mb panel:
// part[((chunk * npass + block) * (p + 2) + row) * mb + response], row j < p: sum x_j y, row p: sum y^2, row p + 1: sum y.
struct MultiPlan {
    int64_t n = 0, rows = 0, nchunk = 0;
    int p = 0, m = 0, lt = 0, mb = 0, npass = 0, cgroups = 0;
    size_t part_doubles = 0;
};
MultiPlan multi_plan(int64_t n, int p, int m, int num_cu);

int launch_multi_xty(hipStream_t s, const MultiPlan &pl, const DenseSrc &X, const MultiY &Y, double *part);
// out[b] (b < nb, (p + 2)^2 doubles each) <- base with the y entries of response r0 + b: the partials added in chunk order
int launch_multi_compose(hipStream_t s, const MultiPlan &pl, const double *base, const double *part, int r0, int nb, double *out);
// xval_oem_multi: the same pass over the fold-ordered rows xp (column-major, leading dimension ldp) and Yp (alike), one launch for
// all folds.  pl = multi_plan(n, p, m, ...): its blocks, groups and rows per chunk; fold k owns chunks [cfirst[k], cfirst[k + 1]) (device, K + 1
// ints; nchunk = cfirst[K] <= multi_fold_chunks_max(pl, K), what `part` is sized for), chunk c of a fold its rows [c * rows, (c + 1) * rows).
inline int64_t multi_fold_chunks_max(const MultiPlan &pl, int K) { return pl.nchunk + K; }      // sum_k ceil(n_k / rows) <= n / rows + K
inline size_t multi_fold_part_doubles(const MultiPlan &pl, int K) { return (size_t)multi_fold_chunks_max(pl, K) * pl.npass * (size_t)(pl.p + 2) * pl.mb; }
int launch_multi_fold_xty(hipStream_t s, const MultiPlan &pl, int K, int nchunk, const double *xp, int64_t ldp, const double *Yp,
                          const int64_t *fold_start, const int64_t *fold_n, const int *cfirst, double *part);
// out[r * (K + 1) + ff] (r < nb, ff <= K, (p + 2)^2 doubles each) <- the fold moments mfold[K] summed in fold order without fold ff (0: all),
// response r0 + r's y entries composed in from the chunk partials; single: out[r * K + k] <- fold k's buffer alone
int launch_multi_fold_compose(hipStream_t s, const MultiPlan &pl, int K, const double *mfold, const double *part, const int *cfirst, int r0, int nb,
                              bool single, double *out);
// out[i] <- Y(i, r), i < n: one response as the contiguous vector the single-response passes read
int launch_multi_column(hipStream_t s, const MultiY &Y, int64_t n, int r, double *out);

}  // namespace oemgpu
