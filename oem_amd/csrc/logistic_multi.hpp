// logistic_multi.hpp -- many binomial responses on one dense x: the shared row pass of an IRLS step (logistic_multi.hip); the
// lock-step driver is logistic.hip's logistic_irls_multi.
#pragma once

#include "multi.hpp"

namespace oemgpu {

constexpr int LMULTI_MCH = 64;               // responses of one lock-step chunk: the workspace of a call is that of 64 responses at most
constexpr int LMULTI_NW = 4;                 // waves per workgroup; wave w owns the 16-column tiles w, w + 4, w + 8, ...
constexpr int LMULTI_P_MAX = 1024;           // 64 column tiles: 16 per wave is what a wave's registers hold

// The row pass as pure host arithmetic (oemgpu_selftest_logistic_multi_plan).  Rows are cut into `nchunk` chunks of `rows` rows (a
// multiple of 64 that depends on n and the CU count ALONE: a response's sums are the same bytes whatever it is computed among), the
// mc <= LMULTI_MCH responses of a lock-step chunk into `npass` blocks of mb = 16 lt; workgroup (chunk, block) writes its panel
// part[((chunk * npass + block) * (p + 2) + row) * mb + response]: row 0 sum r, rows 1 .. p X'r, row p + 1 the sum of the loss terms.
struct LogitMultiPlan {
    int64_t n = 0, rows = 0, nchunk = 0;
    int p = 0, mc = 0, tpw = 0, lt = 0, mb = 0, npass = 0, band = 0;   // band = 64 tpw: the columns a workgroup's accumulators cover
    size_t lds_bytes = 0, part_doubles = 0;
};
LogitMultiPlan logit_multi_plan(int64_t n, int p, int mc, int num_cu);

// The fold mask of a row pass: column t is response ycol[t] of Y (t itself when ycol is null) on the rows with
// foldid[row] != leave[t].  foldid: n device words; leave, ycol: mc device words.  A leave no row carries (0 among ids in [1, K]) keeps
// every row: the bytes of the unmasked pass.  The columns of a block share the rows they load: x must be finite on every row.
struct LogitMultiFold {
    const int32_t *foldid = nullptr;
    const int *leave = nullptr, *ycol = nullptr;
};

// One row pass for the mc responses Y(., 0 .. mc) (Y.y points at the chunk's first response; with fold->ycol at the columns' base).  bt: mc x q, response r's q = p +
// intercept entries of beta o s contiguous, the intercept's first (mode 1; not read in mode 0: r = y).  live: mc device words; a block
// whose responses are all frozen returns at once.  Every other workgroup writes its whole panel.
int launch_logit_multi_rows(hipStream_t s, const LogitMultiPlan &pl, const DenseSrc &X, const MultiY &Y, const double *bt, int intercept, int mode,
                            const int *live, double *part, const LogitMultiFold *fold = nullptr);
// g[r] (p + 2 doubles: [sum r, X'r, sum loss]) <- the panels added in chunk order, for the live responses only
int launch_logit_multi_reduce(hipStream_t s, const LogitMultiPlan &pl, const double *part, const int *live, double *g);

}  // namespace oemgpu
