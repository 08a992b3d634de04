// common.hpp -- shared declarations of liboemgpu (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/oemgpu.h"
#include "path_large_layout.hpp"
#include "switches.hpp"

namespace oemgpu {

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------ error plumbing
void set_error(const char *fmt, ...);
#define OEM_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t e__ = (call);                                                              \
        if (e__ != hipSuccess) {                                                              \
            oemgpu::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
            return OEMGPU_ERR_HIP;                                                            \
        }                                                                                     \
    } while (0)

// ------------------------------------------------------------------ Gram / moments (gram.hip)
// Tiles are 16x16 (one v_mfma_f64_16x16x4_f64 accumulator); only tiles I >= J are built.
struct GramPlan {
    int p;          // columns of X
    int ntc;        // tile columns = ceil(p/16)
    int ntile;      // ntc*(ntc+1)/2
    int tri;        // 1: one wave holds the whole lower triangle (ntc <= 7); 0: 4x4 tile blocks
    int nblk;       // tile blocks per row chunk (1 when tri)
    int wd_units;   // gram_wd.hip: diagonal units of 16 tile columns per row chunk (1: p <= 256; k: 16 k tile columns, with k (k - 1) off-diagonal 8 x 16-tile blocks)
    int wd;         // 4 / 3: 15-16 / 11-12 tile columns, one eight-wave workgroup per row chunk (gram_wd.hip, groups of 4 / 3 tile columns) instead of the super-blocks below; 0: those
    int n8, n6, n4; // shared-slab kernel: super-block rows of 8, 6 and (at most one) 4 tile columns (gram_sb_deal; 0 when tri)
    int nchunk;     // row chunks (workgroups along rows)
    int steps;      // 64-row steps per chunk
    size_t tpart_doubles;   // nchunk * ntile * 256
    size_t vpart_doubles;   // nchunk * (2*16*ntc + 4)
};
GramPlan gram_plan(int64_t n, int p, int num_cu);
GramPlan gram_plan_bound(int64_t nmax, int p, int num_cu);   // sizes that hold the plan of any n <= nmax
void gram_sb_deal(int ntc, int *n8, int *n6, int *n4);
// the kernel form a pass takes (gram.hip: gram_form, the one place it is decided): OEMGPU_GRAM_FORM_* and the ring's strip count
enum { GRAM_FORM_TRI = OEMGPU_GRAM_FORM_TRI, GRAM_FORM_RING_SADDR = OEMGPU_GRAM_FORM_RING_SADDR, GRAM_FORM_RING_LANE = OEMGPU_GRAM_FORM_RING_LANE,
       GRAM_FORM_SB = OEMGPU_GRAM_FORM_SB, GRAM_FORM_WD3 = OEMGPU_GRAM_FORM_WD3, GRAM_FORM_WD4 = OEMGPU_GRAM_FORM_WD4,
       GRAM_FORM_WD_UNITS = OEMGPU_GRAM_FORM_WD_UNITS, GRAM_FORM_BLK = OEMGPU_GRAM_FORM_BLK };
struct GramForm { int form, strips; };
GramForm gram_form(const GramPlan &pl, int64_t n, int64_t ld, bool aligned);

int launch_shift_sums(hipStream_t s, const double *x, int64_t n, int64_t ld, int p, const double *y, double *sums);
int launch_gram(hipStream_t s, const GramPlan &pl, const double *x, int64_t n, int64_t ld, const double *y,
                const double *sums /* p+2 or null */, double *tpart, double *vpart);
int launch_moments_reduce(hipStream_t s, const GramPlan &pl, const double *tpart, const double *vpart, double *moments);

// ------------------------------------------------------------------ Gram / moments of a row-major X (gram_rm.hip)
// 4 x 4 tile blocks of the lower triangle of Z = [X | y | 1] over row chunks of `steps` 16-row steps; a block's partial is 16 tile slots
constexpr int GRAM_RM_P_MAX = 1024;        // columns of X the row-major pass takes (the engines behind it: p <= 1024 never goes the p >= n way)
constexpr int GRAM_RM_MIN_ROWS = 1024;     // a row chunk is no shorter (but for the matrix's own end)
constexpr int64_t GRAM_RM_PART_BYTES = 512 << 20;   // the chunk partials in all, unless ~4 workgroups per CU need more
constexpr int64_t GRAM_RM_CHUNK_BYTES = 16 << 20;   // ... and no longer than this many bytes of float64 rows, unless that leaves fewer than ~4 workgroups per CU
struct GramRmPlan {
    int p;          // columns of X
    int ntc;        // tile columns = ceil((p + 2) / 16)
    int nb;         // block rows = ceil(ntc / 4)
    int nblk;       // blocks per row chunk = nb (nb + 1) / 2
    int nchunk;     // row chunks
    int64_t steps;  // 16-row steps per chunk
    size_t tpart_doubles;   // nchunk * nblk * 16 * 256
};
GramRmPlan gram_rm_plan(int64_t n, int p, int num_cu);
int launch_shift_sums_rm(hipStream_t s, const void *x, int dtype, int64_t n, int64_t ldr, int p, const double *y, double *sums);
int launch_gram_rm(hipStream_t s, const GramRmPlan &pl, const void *x, int dtype, int64_t n, int64_t ldr, const double *y,
                   const double *sums /* or null */, double *tpart);
int launch_gram_rm_reduce(hipStream_t s, const GramRmPlan &pl, const double *tpart, double *moments);

// stats layout written by finalize (doubles): [0] meanY [1] scaleY [2] yy (sum of squared standardised y)
// [3] nobs [4..4+p) meanX [4+p..4+2p) scaleX (dense) or colsq_inv (big) [4+2p] 1 if the moments were read as shifted [4+2p+1] 0
__host__ __device__ static inline int stats_len(int p) { return 4 + 2 * p + 2; }
__host__ __device__ static inline int stats_shift_flag(int p) { return 4 + 2 * p; }
int launch_finalize(hipStream_t s, const double *moments, const double *sums, int p, int sem, int standardize,
                    int intercept, double *xx /* q x q */, double *xy /* q */, double *stats);
int launch_xtx_prepare(hipStream_t s, const double *xtx, const double *xty, const double *sf_inv /* or null */, int p,
                       double *xx, double *xy, double *stats);

// moments of one device-resident shard into `moments` (overwrite), timed as OEMGPU_T_GRAMK (api.hip)
int shard_moments(oemgpu_ctx *c, const GramPlan &pl, const double *x, int64_t n, int64_t ld, const double *y, const double *sums,
                  double *tpart, double *vpart, double *moments);
int launch_moments_add(hipStream_t s, double *acc, const double *m, size_t len, bool first);   // acc = m (first) or acc + m (sparse.hip)

// ------------------------------------------------------------------ sparse x (sparse.hip): moments of a compressed-sparse-column matrix
// both sparse fits, before any device lookup: colptr[0] = 0 and non-decreasing, row indices in [0, n) and strictly increasing inside a
// column.  The longest column, or OEMGPU_ERR_ARG (error text prefixed by `who`); rowcount (or null): [i + 1] = non-zeros of row i
int64_t csc_check(const char *who, int64_t n, int p, const int64_t *colptr, const int32_t *rowidx, const double *values,
                  std::vector<int64_t> *rowcount);
// the route to the moments: compressed columns when the kernel fits in LDS, nnz <= 2 % of n p (there it beats the n p^2 dense pass)
// and n < 2^31; else zero-filled row tiles of `rows` rows (<= 2 GiB; set on both routes) and leading dimension ld
constexpr int CSC_CHUNK = 8192;     // rows per chunk of the compressed-column kernels: 64 KB of LDS
struct SparseRoute { bool csc; int64_t rows, ld; };
SparseRoute sparse_route(int64_t n, int p, int64_t nnz);
// n <= p: does the fit run from the non-zeros (sparse_wide.hip) instead of the dense copy?  nnz <= 2 % of n p (sparse_route's density
// limit) and p > 1024 (wide_pays's bound: below it the register engines run the p x p Gram form and the dense copy is small);
// OEM_SPARSE_GRAM=wide forces it for any n <= p, =nowide forbids it
bool sparse_wide_route(int64_t n, int p, int64_t nnz);
// the tile route: per tile of R.rows rows zero it, densify (times sqrt(w[row]) if w), shard_moments -> mtile, add into M in row order.
// y: the Gaussian fit's y, or null; tpart / vpart: the scratch of gram_plan_bound(R.rows, p)
int csc_tile_moments(oemgpu_ctx *c, const SparseRoute &R, const int64_t *colptr, const int32_t *rowidx, const double *val, const double *w,
                     const double *y, int64_t n, int p, int64_t maxcol, double *tile, double *tpart, double *vpart, double *mtile, double *M,
                     int64_t row0 = 0, int64_t nrows = -1);       // nrows >= 0: the rows [row0, row0 + nrows) only
int64_t csc_tiles(const SparseRoute &R, int64_t nrows);           // tiles of a row range, and the rows [*r0, *r1) of tile t of the range from row0
void csc_tile_rows(const SparseRoute &R, int64_t row0, int64_t nrows, int64_t t, int64_t *r0, int64_t *r1);
size_t csc_moments_work_bytes(int64_t n, int p);
bool csc_moments_fits(int p);
int launch_csc_moments(hipStream_t s, const int64_t *colptr, const int32_t *rowidx, const double *val, const double *y, int64_t n, int p,
                       void *work, double *moments);
// the binomial fit (logistic_sparse.hip): chunk pointers once, a compressed-row copy once, X'WX at every IRLS step
int csc_chunks(int64_t n);
size_t csc_wgram_work_bytes(int64_t n, int p);
int launch_csc_chunk_ptr(hipStream_t s, const int64_t *colptr, const int32_t *rowidx, int64_t n, int p, int32_t *cptr);
int launch_csc_to_csr(hipStream_t s, const int64_t *colptr, const int32_t *rowidx, const double *val, const int32_t *cptr, int64_t n, int p,
                      const int64_t *rowptr, int32_t *ccol, double *cval);
int launch_csc_wgram(hipStream_t s, const int64_t *colptr, const int32_t *rowidx, const double *val, const double *w, const int32_t *cptr,
                     int64_t n, int p, double *part, double *M);
// observation weights of oemDense (weighted.hip): DataStd's weighted statistics, the scaled copy, its constants into `stats`
int launch_weighted_stats(hipStream_t s, const double *x, int64_t n, int64_t ld, int p, const double *y, const double *w, int flag, double *ws);
int launch_weighted_apply(hipStream_t s, const double *x, int64_t n, int64_t ld, int p, const double *y, const double *w, int flag, const double *ws,
                          int squared, double *z, int64_t ldz, double *yz);
int launch_weighted_patch_stats(hipStream_t s, const double *ws, int p, double *stats);
int launch_gram_loss(hipStream_t s, const double *xx, const double *xy, const double *stats, int q, const double *beta, const double *sinv,
                     const int *niter, double *loss, int nk);                       // oemSparse's compute.loss behind the larger engines
int launch_resid_loss(hipStream_t s, const double *x, int64_t n, int64_t ld, int p, const double *y, const double *beta, int rows, int nk,
                      double *part, double *loss);                                  // ... and with p >= n

// ------------------------------------------------------------------ xval.oem (xval.hip)
size_t fold_layout_ints(int64_t n, int K);
int launch_fold_layout(hipStream_t s, const int *foldid, int64_t n, int K, int *blockcnt, int64_t *fold_n, int64_t *fold_start,
                       int *pos, int *bad, int align = 16);   // align: fold segments start on multiples of it (16: the MFMA kernels; CSC_CHUNK: a sparse x)
int launch_gather_rows(hipStream_t s, const double *x, int64_t n, int64_t ld, int p, const double *y, const int *pos,
                       double *xo, int64_t ldo, double *yo);
// the same from a row-major x of OEMGPU_F64 / OEMGPU_F32 elements (row stride ldr); a row whose foldid is outside 1..K writes nothing
int launch_gather_rows_rm(hipStream_t s, const void *x, int dtype, int64_t n, int64_t ldr, int p, const double *y, const int *foldid, int K,
                          const int *pos, double *xo, int64_t ldo, double *yo);
// xval_oem_multi: Yp[pos[i] + r * ldo] <- Y(i, r) = y[i * rs + r * cs], every response into fold order (after the fold ids were found valid)
int launch_gather_responses(hipStream_t s, const double *y, int64_t rs, int64_t cs, int64_t n, int m, const int *pos, double *yo, int64_t ldo);
int launch_fold_sum(hipStream_t s, const double *M, int K, size_t len, int skip /* 1-based, 0: none */, double *out);
// the shape of the CV-error launch (xval.hip: cv_error_plan; pure host arithmetic): K4 = p + 1 rounded up to a k-step of 4, ntile 16-lambda
// tiles in `passes` passes of lt each, form CV_FORM_*, lds dynamic bytes, the coefficient rows in `chunks` LDS chunks of which the last
// holds `last` (chunks = 1, last = K4 unless CHUNK), nwg workgroups per fold
enum { CV_FORM_SINGLE = 0, CV_FORM_MULTI = 1, CV_FORM_CHUNK = 2 };
struct CvErrPlan {
    int K4, ntile, lt, passes, form, chunks, last, nwg;
    size_t lds;
};
CvErrPlan cv_error_plan(int64_t n, int p, int K, int npen, int nl, int num_cu);
size_t cv_part_doubles(int nwg, int K, int npen, int nl);
int launch_cv_error(hipStream_t s, const double *xp, int64_t ldp, const double *yp, const int64_t *fold_start, const int64_t *fold_n,
                    int K, int p, const double *B, int npen, int nl, int mae, int wmode, const CvErrPlan &P, double n, double *part, double *out,
                    bool triples = false);
int launch_cv_finish(hipStream_t s, const double *part, int nparts, int npen, int nl, double n, double *out, bool triples);
// xval_oem_multi: nb responses on one fold-ordered x in one product launch and one finish launch (xval.hip: CvMany); P from
// cv_error_plan_many, whose nwg divides the CUs by K * npen * nb.  Response r: y = Yp + r * ldp, table B + r * K * npen * nl * (p + 1),
// partials part + r * cv_part_doubles(P.nwg, K, npen, nl), out + r * npen * nl * 2 <- (cvm, cvsd)
CvErrPlan cv_error_plan_many(int64_t n, int p, int K, int npen, int nl, int nb, int num_cu);
int launch_cv_error_many(hipStream_t s, const double *xp, int64_t ldp, const double *Yp, const int64_t *fold_start, const int64_t *fold_n,
                         int K, int p, const double *B, int npen, int nl, int mae, const CvErrPlan &P, double n, int nb, double *part, double *out);
// cv.oem, family = "gaussian": the same product from the same plan with one (count, mean, M2) per FOLD -- triples[K][npen][nl][3], (0, NaN, NaN)
// in columns >= ncol[pen] and for empty folds -- and, with predmat != nullptr, yhat stored through inv (fold position -> caller's row, from
// launch_fold_inverse) into predmat[npen][nl][n], NaN in columns >= ncol[pen]
int launch_fold_inverse(hipStream_t s, const int *pos, int64_t n, int64_t ldp, int *inv);
int launch_cv_fold_error(hipStream_t s, const double *xp, int64_t ldp, const double *yp, const int64_t *fold_start, const int64_t *fold_n,
                         int K, int p, const double *B, int npen, int nl, int mae, const CvErrPlan &P, double *part, const int *ncol,
                         double *triples, double *predmat, const int *inv, int64_t n);
int launch_cv_fold_finish(hipStream_t s, const double *part, int per_fold, int K, int npen, int nl, const int *ncol, double *triples);
// cv_oem_multi: launch_cv_fold_error for nb responses in one product launch and one finish launch (P from cv_error_plan_many).  Response r:
// y = Yp + r * ldp, table B + r * K * npen * nl * (p + 1), ncol + r * npen, triples + r * K * npen * nl * 3, predmat + r * npen * nl * n
int launch_cv_fold_error_many(hipStream_t s, const double *xp, int64_t ldp, const double *Yp, const int64_t *fold_start, const int64_t *fold_n,
                              int K, int p, const double *B, int npen, int nl, int mae, const CvErrPlan &P, int nb, double *part, const int *ncol,
                              double *triples, double *predmat, const int *inv, int64_t n);
// cv_oem_multi: tab[nb][K][npen][nl][p + 1] <- raw[left] frac + raw[right] (1 - frac) per column j < ncol[r][pen] (idx[nb][K][npen][nl]: the
// host's lambda.interp of fold grid k of response r at the full fit's lambda j), zero from ncol on
struct CvInterpIdx { int left, right; double frac; };
int launch_cv_interp(hipStream_t s, const double *raw, const CvInterpIdx *idx, const int *ncol, int nb, int K, int npen, int nl, int p, double *tab);

// ------------------------------------------------------------------ xval.oem on a sparse x (xval_sparse.hip, sparse.hip)
// The ONE host plan of the call (pure arithmetic): the route of sparse_route, the fold-ordered layout (fold segments start on multiples of
// CSC_CHUNK rows: at most nchunk_max = floor(n / CSC_CHUNK) + K chunks, npad_max rows), the chunk ranges of csc_gram_kernel (`per` chunks
// each and never across a fold boundary: at most nrange_max in all, rpf_max in one fold), the CV-error launch over the compressed rows
// (cv_nwg workgroups of XVS_CVW waves x npen x cv_lblk blocks of 64 lambdas; one partial per wave) and the byte offsets of everything the
// call keeps on the device behind the xval layout (api.hip: xval_layout), `bytes` in all.  Nothing of n p doubles on the csc route.
constexpr int XVS_CVW = 4;
struct XvalSparsePlan {
    SparseRoute R;
    int64_t n, nnz, npad_max;
    int p, K, npen, nl, nl16;
    int nchunk_max, per, nrange_max, rpf_max, cv_nwg, cv_waves, cv_lblk;
    GramPlan plmax;                                              // tile route: the scratch of the MFMA pass over one tile (zero on the csc route)
    size_t a_col, a_row, a_val, a_y, a_fid, a_prow, a_pval, a_cfo, a_cptr, a_rowptr, a_ccol, a_cval, a_gpart, a_ypart, a_rtab, a_bt, a_tile,
           a_mtile, bytes;
};
// resident (cv.oem on an oemgpu_sparse_x): the compressed columns are the handle's, y and foldid the caller's -- their five regions are empty
XvalSparsePlan xval_sparse_plan(int64_t n, int p, int64_t nnz, int K, int npen, int nl, int num_cu, bool resident = false);
// the ranges of the folds as they are: rtab[r] .. rtab[r + 1] the chunks of range r, frange[k] .. frange[k + 1] the ranges of fold k; *npad
// <- the rows of the fold-ordered layout.  OEMGPU_ERR_INTERNAL if they exceed the plan's bounds
int xval_sparse_ranges(const XvalSparsePlan &P, const int64_t *fold_n, std::vector<int32_t> &rtab, std::vector<int32_t> &frange, int64_t *npad);
// compressed columns into fold order (stable inside a column and fold): prow / pval, cfo[p][K + 1] where fold k's entries of a column start
// (offsets inside the column), yp[npad] <- y in the same order (padding rows 0)
int launch_csc_fold_permute(hipStream_t s, const int64_t *colptr, const int32_t *rowidx, const double *val, const double *y, const int32_t *foldid,
                            const int *pos, int64_t n, int p, int K, int64_t npad, int32_t *cfo, int32_t *prow, double *pval, double *yp);
// the K moment buffers of the csc route: the range sums of csc_gram_kernel added in range order inside every fold, the per-fold statistics
int launch_csc_fold_moments(hipStream_t s, const int64_t *colptr, const int32_t *prow, const double *pval, const double *yp, const int32_t *cptr,
                            const int32_t *cfo, const int64_t *fold_start, const int64_t *fold_n, int p, int K, int nchunk, int nrange,
                            const int32_t *rtab, const int32_t *frange, double *gpart, double *ypart, double *mfold);
// row pointers of the fold-ordered compressed rows from the chunk pointers (rowptr[nchunk * CSC_CHUNK + 1])
int launch_csr_rowptr(hipStream_t s, const int64_t *colptr, const int32_t *prow, const int32_t *cptr, int p, int nchunk, int64_t *rowptr);
// CV error over the compressed rows: B [K][npen][nl][p + 1] -> bt [K][npen][p + 1][nl16], one partial per wave, then cv_finish_kernel
int launch_csr_cv_error(hipStream_t s, const XvalSparsePlan &P, const int64_t *rowptr, const int32_t *ccol, const double *cval, const double *yp,
                        const int64_t *fold_start, const int64_t *fold_n, const double *B, double *bt, int mae, double *part, double *out,
                        bool triples);
// cv.oem (family = "gaussian") on a resident sparse x: the scoring launch over the fold-ordered compressed rows.  Pure host arithmetic,
// the ONE place its shape is decided: nwg workgroups of XVS_CVW waves x npen x lblk blocks of 64 lambdas -- about four workgroups per CU
// over (penalty, lambda block), a wave no fewer than 16 rows, at most 1024 workgroups, and no more waves than keep the per-fold wave
// partials [K][waves][npen][nl16][4] (part_bytes) under CVS_PART_MAX; never fewer than one workgroup (only K npen nl16 > 500,000
// then exceeds the bound: 512 folds x 100 lambdas x 9 penalties).
constexpr size_t CVS_PART_MAX = 64000000;
struct CvSparseScorePlan {
    int K, npen, nl, nl16, nwg, waves, lblk;
    size_t part_bytes;
};
CvSparseScorePlan cv_sparse_score_plan(int64_t n, int K, int npen, int nl, int num_cu);
// B [K][npen][nl][p + 1] -> bt [K][npen][p + 1][nl16]; csr_cv_fold_score_kernel flushes a wave's (rows, centre, sums) at every fold
// boundary; cv_fold_finish_kernel merges them per fold -> triples[K][npen][nl][3], (0, NaN, NaN) in columns >= ncol[pen] and for empty
// folds.  predmat != nullptr: eta into predmat[npen][nl][n] at the caller's row inv[fold position], NaN in columns >= ncol[pen].
int launch_csr_cv_fold_score(hipStream_t s, const CvSparseScorePlan &P, int p, const int64_t *rowptr, const int32_t *ccol, const double *cval,
                             const double *yp, const int64_t *fold_start, const int64_t *fold_n, const double *B, double *bt, int mae,
                             double *part, const int *ncol, double *triples, double *predmat, const int *inv, int64_t n);
// cv.oem on a resident sparse x with n <= p (oemgpu_cv_sparse_wide_score_res): no fold-ordered layout -- the handle's compressed rows
// in the caller's order, the held-out rows of a fold from a row list, ONE fold's transposed table [npen][p + 1][nl16] staged at a time
// (table_bytes: one penalty's).  Pure host arithmetic, the one place the launch is decided: nwg workgroups of XVS_CVW waves x npen x
// lblk blocks of 64 lambdas per fold -- about four workgroups per CU over (penalty, lambda block), no more waves than a fold of
// ceil(n / K) rows has rows, at most 1024 workgroups, the wave partials of all folds [K][waves][npen][nl16][4] under CVS_PART_MAX,
// never fewer than one workgroup -- and the offsets of the call's pieces in the context's workspace (bytes in all).
struct CvWideScorePlan {
    int K, npen, nl, nl16, nwg, waves, lblk;
    size_t table_bytes, part_bytes, a_list, a_raw, a_bt, a_part, a_tri, a_ncol, bytes;
};
CvWideScorePlan cv_wide_score_plan(int64_t n, int p, int K, int npen, int nl, int num_cu);
int launch_csr_cv_wide_score_fold(hipStream_t s, const CvWideScorePlan &P, int p, const int64_t *rowptr, const int32_t *ccol, const double *cval,
                                  const double *y, const int32_t *list, int nk, const double *raw, double *bt, int mae, const int *ncol,
                                  double *part_k, double *predmat, int64_t n);
int launch_csc_gram_ranges(hipStream_t s, const int64_t *colptr, const int32_t *rowidx, const double *val, const int32_t *cptr, int p, int nchunk,
                           int nrange, const int32_t *rtab, double *part);
size_t csc_gram_lds_bytes(int p);
int csc_range_budget(int64_t n, int p);                           // the ~1024-workgroup range count of launch_csc_moments

// observation weights of xval.oem (ref src/oem_xval_dense.h:486-623): unweighted column sums of squares per fold, then the
// fold-ordered copy times sqrt(w); and the weighted counterpart of launch_finalize
int launch_weight_scale(hipStream_t s, double *xp, int64_t ldp, double *yp, int p, int K, const int64_t *fold_start, const int64_t *fold_n,
                        double *csq);
int launch_finalize_weighted(hipStream_t s, const double *Mw, const double *cs, int p, int standardize, int intercept, double *xx,
                             double *xy, double *stats);

// ------------------------------------------------------------------ eigen + path
struct PathArgs {
    int p;                   // dimension of beta (q)
    int npen, nl, user_lambda, maxit, accelerate, compute_loss;
    int ngroups;             // 0 when no group data
    int lanczos_steps;       // eigen step: number of Lanczos steps (<= p)
    int yscale;              // 1: ilambda = lambda / scaleY and lmax *= scaleY (dense); 0: xtx / big
    int lmax_from;           // lambda_zero = max |xy[j]| over j >= lmax_from (1: xval.oem leaves the intercept slot out, ref src/oem_xval_dense.h:1025-1032)
    double alpha, gamma, tau, tol, lambda_min_ratio;
    const double *xx;        // q x q col-major, ld = q
    const double *xy;        // q
    const double *stats;     // see stats layout
    const int *penalty;      // npen
    const double *lambda_user;   // npen * nl or null
    const double *pf;        // q penalty factors
    const double *sinv;      // q: oemXTX::get_beta in-place rescale (ref src/oem_xtx.h:576-581) or null
    const int *gid;          // q: index of the column's group in unique_groups, -1 if none
    const int *gstart;       // ngroups+1
    const int *gidx;         // members by group, increasing
    const double *gw;        // ngroups weights
    const int *gzero;        // ngroups: unique_groups[g] == 0
    // grp_head = 1, 2, 3 (the launch engines on the packed triangle, path_large.hip: sympk_head_kernel<HB>): every group is a run of <= 32 HB
    // neighbouring coordinates and nothing needs a sum over all coordinates -- the group operators then run in the head of the (head, product)
    // pairs like the element-wise ones.  Per coordinate: grun[2 j] = its group's first coordinate, grun[2 j + 1] = one past its last |
    // (unique_groups[g] == 0) << 30 -- (1, 0): in no group --, gwc[j] = the group's weight
    int grp_head;
    const int *grun;
    const double *gwc;
    // outputs (device)
    double *beta;            // npen * nl * q (standardised scale)
    double *lambda_out;      // npen * nl (unscaled lambda actually used)
    int *niter;              // npen * nl
    double *loss;            // npen * nl
    double *d_out;           // D_OUT_LEN doubles: [0] = d, [1] = lambda_max, [2] shader cycles, [3] 100 MHz ticks of the fused kernel,
                             // [4] Lanczos steps taken, [5] 1 if the step cap ended the recurrence (neither stop rule nor breakdown),
                             // [6] exchange poison: cleared by the host before the launch, set to 1 by ANY workgroup whose exchange
                             //     timed out (a slot nobody else writes: the writer's stores cannot cover it up -- ADVICE r2)
                             // [7], [8] (row-split kernel only) OEM rounds run in the short form / in all, of penalty 0's path
    // workspace for the large-p engine: path_large_work_doubles(p) doubles (its regions: path_large_layout.hpp, LargeWork)
    double *work;
    // q > 1024 on the launch-per-iteration Gram engine: sympk_doubles(q) doubles for the packed lower triangle of XX and what its products
    // keep behind it (path_large_layout.hpp: SpkWork; a buffer of the context, outside the workspace frame); null: the row-streaming product
    double *sympk;
    // nbatch > 1 (p <= SMALL_P_MAX only): blockIdx.y selects one of nbatch independent problems that share everything above
    // except xx, xy, stats (element strides bs_xx, bs_xy, bs_stats), the outputs (byte stride bs_out) and work (bs_work)
    int nbatch;
    long long bs_xx, bs_xy, bs_stats, bs_out, bs_work;
    // pen_split (p <= SMALL_P_MAX only): every penalty of every instance gets a workgroup (set) of its own -- penalties are
    // independent cold starts (ref src/oem_dense.cpp:243-244) -- so blockIdx.y = instance + nbatch * penalty; pen_lo / pen_hi are
    // the penalties this workgroup walks ([0, npen) without the split)
    int pen_split, pen_lo, pen_hi;
    int lmax_group;          // > 0 (nbatch > 1, lmax_xy below = instance 0's xy): instance b takes lambda_zero from instance (b / lmax_group) * lmax_group
                             // instead -- the K + 1 fits of one response among many (xval_oem_multi); 0: all from lmax_xy as it stands.  (In the
                             // padding behind three ints: the size of the struct and every other offset are what they were.)
    const double *lmax_xy;   // not null: every instance takes lambda_zero from THIS xy (xval.oem: the grid of the full-data fit, ref src/oem_xval_dense.cpp:177-194)
    // not null (row-split kernel only): the outputs above point into PINNED HOST memory the device writes directly (the kernel only
    // ever stores to them), and the kernel leaves a copy of `stats` here as well -- no device-to-host copy node behind the kernel
    double *stats_out;
    int stats_n;             // doubles of stats to copy
    double d_fixed;          // > 0 (launch-per-iteration Gram engine only): d handed over, no eigenvalue step (weighted oemDense with nobs <= nvars:
                             // the reference takes d from one matrix and iterates on another, ref src/oem_dense.h:466-483, 513-517)
    // The persistent engines only (one launch for the whole penalty x lambda path): a word in host-coherent pinned memory that the host
    // sets when the caller's interrupt callback fires while it waits for the launch (ref src/oem_dense.cpp:235-238: the reference polls
    // every third lambda).  Every workgroup reads it once per 128 iterations and inside any exchange spin that lasts; whoever sees it
    // stops waiting for anybody, the "leave" bit rides in the workgroup's next vote and the loops are left.  Null: never asked.
    const int *abort_word;
    // path_coop.hip, q <= 512: the cooperating workgroups of an instance all on ONE XCD (8 x as many workgroups are launched and only
    // those with blockIdx.x % 8 == (xcd_base + blockIdx.y) % 8 take part; the kernel proves the placement before it relies on it)
    int one_xcd, xcd_base;
    int no_active_prefix;    // row-split kernel: 1 = never enter the short round (OEM_NO_ACTIVE_PREFIX; the ranked layout stays)
};

// the read of PathArgs::abort_word (system scope: the word lives in host memory)
// (wave-uniform by construction -- every lane reads the same word in the same instruction -- and said so: the engines keep what
// follows from it in scalar registers)
__device__ __forceinline__ bool path_abort_asked(const int *w)
{
    return w && __builtin_amdgcn_readfirstlane(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) != 0;
}
constexpr unsigned PATH_ABORT_SPINS = 1024u;   // an exchange spin looks at the word (and at its timeout) every 1,024 sweeps (~1 ms): never on the way of an exchange that arrives
constexpr unsigned PATH_TIMEOUT_ROUNDS = 1000u; // ... and gives up after that many rounds (~1 s): a partner is gone
constexpr int PATH_FAILED_TIMEOUT = 1, PATH_FAILED_ABORT = 2;

// the problem instance of this workgroup (see PathArgs::nbatch); all scalar arithmetic
// GRP = false: an instantiation that is never launched with a lambda group (PathArgs::lmax_group) and carries no code for one -- the
// row-split kernel keeps the parent's code for single fits and ungrouped batches that way (it spills scalar registers, and one more
// live scalar cost config 1's fit 14 us of 490)
template <bool GRP = true>
__device__ __forceinline__ PathArgs path_instance(PathArgs A)
{
    const int nb = A.nbatch > 1 ? A.nbatch : 1;
    const long long y = blockIdx.y;
    if (A.pen_split) { A.pen_lo = (int)(y / nb); A.pen_hi = A.pen_lo + 1; }
    A.work += y * A.bs_work;                                   // exchange granules: one set per workgroup set
    if (A.nbatch > 1) {
        const long long b = y % nb;
        A.xx += b * A.bs_xx; A.xy += b * A.bs_xy; A.stats += b * A.bs_stats;
        const long long ob = b * A.bs_out;
        A.beta = (double *)((char *)A.beta + ob); A.lambda_out = (double *)((char *)A.lambda_out + ob);
        A.loss = (double *)((char *)A.loss + ob); A.d_out = (double *)((char *)A.d_out + ob);
        A.niter = (int *)((char *)A.niter + ob);
        if constexpr (GRP) { if (A.lmax_group > 0 && A.lmax_xy) A.lmax_xy += (b / A.lmax_group) * A.lmax_group * A.bs_xy; }
    }
    return A;
}

static const int D_OUT_LEN = 9;
// Stop rule of every Lanczos recurrence here: the geometric tail implied by two successive moves of the top Ritz value, relative.
// The reference's own tolerance on this eigenvalue is 1e-10 (Spectra, ref src/oem_dense.h:494-498); the estimate is conservative
// (config 1: it says 3e-13 where the true error is 1e-14), and the tests hold d to 1e-10 against LAPACK and the CPU restatement.  (1e-11 was tried in round 3: config 1 still takes 40 steps, config 4 still 144, and one xval fit moved: no gain.)
#ifndef OEM_LANCZOS_TAIL_TOL
#define OEM_LANCZOS_TAIL_TOL 1e-12
#endif
static const int COOP_MIN_Q = 209, COOP_MIN_Q_GROUPS = 209;      // from here the cooperating-workgroup engine (path_coop.hip) takes the path when it is eligible (element-wise penalties only / a group penalty in the call)
int path_coop_min_q(bool has_groups);
static const int SMALL_P_MAX = 288;     // one workgroup where the matrix fits its registers (+ LDS); else four cooperating workgroups (big.oem's p + 1 = 257 included)
size_t path_small_xchg_bytes();
int launch_path_small(hipStream_t s, const PathArgs &a);          // p <= SMALL_P_MAX: one fused launch
bool path_small_takes_rows(const PathArgs &a);                    // will launch_path_small use the row-split kernel (p <= 208)?
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device, size): the call costs microseconds, and config 1 made it
// in front of every Gram launch with the GPU idle
int lds_limit_once(const void *fn, size_t bytes);
int run_path_large(hipStream_t s, const PathArgs &a, double *host_scratch);   // any p: multi-launch engine
size_t path_large_work_doubles(int p, int nsteps);                // large_work(p).total (path_large_layout.hpp)
size_t sympk_doubles(int q);                                      // spk_work(q).total: 0 for q <= 1024
int sympk_gemv_probe(hipStream_t s, const double *xx, int q, double *pk, const double *vec, double *out, int reps, double *us_per_product);
// 288 < p <= 1024: one persistent launch of cooperating workgroups (path_coop.hip)
bool path_coop_eligible(int q, bool has_sinv, bool compute_loss, int ngroups, int nbatch);
int path_coop_workgroups(int q);
size_t path_coop_xchg_bytes();
int launch_path_coop(hipStream_t s, const PathArgs &a);

// 1024 < p <= 4096, element-wise penalties: one persistent launch with the lower triangle of XX in the register files of <= 192 CUs
// (path_symcoop.hip).  The plan (tiles per wave, blocks per workgroup, senders per block) is pure host arithmetic.
struct SymcoopPlan {
    int q = 0, T = 0, NT = 0, G = 0, nsum = 0, e1n = 0;    // 64-blocks, tiles per wave, workgroups, sender rows of exchange 1, sender sweeps per owner
    bool runs = false;                                      // the owners' slices are cut at group-run boundaries
    int split = 0;                                          // ... and some group (of more than 32 members) lies in several owners' slices: the most owners of one
    std::vector<int> tab;                                   // blkbase[80] then G records (uploaded as is); split groups: + the fragment table [2 q]
};
bool symcoop_plan(int q, int gmax, SymcoopPlan &P, const int *runs = nullptr, int nruns = 0);   // runs: group runs (starts, nruns + 1) the owners' slices are cut at
int symcoop_plan_owners(int q, int gmax, const int *runs, int nruns, int *owner_c0, int *owner_n, int *frag, int *G_out, int *split_out);
size_t symcoop_xchg_bytes(const SymcoopPlan &P);
size_t symcoop_work_bytes(const SymcoopPlan &P);    // ... plus the kernel's copy of its arguments
size_t symcoop_xchg_bytes_max(int q);
bool path_symcoop_eligible(const PathArgs &a, bool group_penalty, bool plan_has_runs);
int launch_path_symcoop(hipStream_t s, const PathArgs &a, const SymcoopPlan &P, const int *plan_dev, void *xchg);

// 1024 < p <= 2048, element-wise penalties: the row-split form, ONE exchange per iteration (path_symcoop.hip: path_rowcoop_kernel)
bool path_rowcoop_eligible(const PathArgs &a, bool group_penalty);
int path_rowcoop_workgroups(int q);
size_t path_rowcoop_xchg_bytes();
int launch_path_rowcoop(hipStream_t s, const PathArgs &a, void *xchg);

// ------------------------------------------------------------------ p >= n (wide.hip, path_large.hip: run_path_wide)
// The reference's own iteration for p >= n: no Gram, two products with the standardised X per iteration
// (ref src/oem_dense.h:363-366, 476-482, 513-521).  Layout of the standardised copy: `nb` row blocks of `rb` rows each (the last
// may hold fewer), every block a column-major (64 nr) x p matrix of its own with zero padding rows -- a column of a block lives in
// the registers of one wave (nr <= 32 doubles per lane).  n <= 2048: one block.
// (struct WideLayout, wide_layout(n), wide_workgroups(n, p): path_large_layout.hpp)
struct WideArgs {
    const double *xs;        // standardised X: block b at xs + b * npad() * p
    const double *ys;        // standardised y, rows() entries in the same blocked order (padding zero)
    WideLayout lay;
    int n;
    double *scratch;         // wide_scratch_doubles(n, p) doubles
    // group penalties where every group is a run of neighbouring columns (the usual case): the runs in column order, dealt to the
    // workgroups of the fused group kernel (path_large.hip: wide_groups_kernel) in whole runs.  grun_W = 0: not available.
    const int *grun_start = nullptr;   // device: nruns + 1 column indices
    const int *grun_gid = nullptr;     // device: group index of each run
    const int *grun_wg = nullptr;      // device: grun_W + 1 run indices
    int grun_W = 0, grun_cpw = 0;      // workgroups; most columns in one workgroup
    // not null: X is a resident sparse x and the two products run over its non-zeros (sparse_wide.hip; path_large.hip:
    // run_path_sparse_wide).  xs, ys, lay and scratch are then unused, and n is bounded by the int32 row indices alone.
    const struct SpwArgs *sparse = nullptr;
};
// ------------------------------------------------------------------ p >= n on a sparse x (sparse_wide.hip)
// Both products are one gather over compressed lines: the row pass t_i = sum_k cval[k] v[ccol[k]] over the compressed rows, the
// column pass g_j = sum_k val[k] w[rowidx[k]] over the compressed columns.  A line is taken by L = 1 .. 64 lanes of a wave (64 / L
// lines to a wave, four waves to a workgroup), or -- longer than SPW_LONG_PER_LANE L entries -- by a whole workgroup (the long
// form, over a list of such lines made once per call).  Every sum has one fixed order.  The plan is pure host arithmetic.
constexpr int SPW_LONG_PER_LANE = 32;
struct SpwPlan {
    int route;               // sparse_wide_route
    int row_L, col_L;        // lanes per row / per column in the short form
    int long_rows, long_cols;    // is the long form used (the longest line exceeds SPW_LONG_PER_LANE L)?
    int row_wgs, col_wgs;    // workgroups of the short form of either pass
    size_t ws_bytes;         // the engine's own vectors, the Lanczos table and the two lists of long lines
};
// force_row_L / force_col_L: 0, or the lanes to use instead of the planned ones (oemgpu_selftest_sparse_wide_pass; the fit passes 0, 0);
// the long flags and the workgroups follow the lanes in force
SpwPlan spw_plan(int64_t n, int p, int64_t nnz, int64_t longest_row, int64_t longest_col, int num_cu, int force_row_L = 0, int force_col_L = 0);
struct SpwArgs {
    const int64_t *colptr, *rowptr;
    const int32_t *rowidx, *ccol;
    const double *val, *cval;
    int n, p;
    SpwPlan plan;
    const int32_t *long_row_list, *long_col_list;    // device: the lines of the long form
    int n_long_rows, n_long_cols;
    double *vec;             // device: spw_vec_doubles(n) doubles (path_large_layout.hpp: SpwVec)
    // cv.oem's fold fit (oemgpu_fit_sparse_wide_fold_res): not null -- the rows with foldid[i] == leave_out are left out of every row
    // pass and of the STATS pass, and nk, the kept rows (2 <= nk < n), stands wherever n enters the arithmetic
    const int32_t *foldid = nullptr;
    int leave_out = 0, nk = 0;
};
// out[i] = scale * sum over compressed row i (n of them) of cval v[ccol]; skipped while *done != 0 (done may be null).  A fold fit
// (A.foldid): a left-out row is not read and out[i] = 0.0 exactly.  The column pass is never masked (its input is 0 in those rows).
int launch_spw_rows(hipStream_t s, const SpwArgs &A, const double *v, double *out, double scale, const int *done);
// out[j] = scale * sum over compressed column j (p of them) of val w[rowidx]
int launch_spw_cols(hipStream_t s, const SpwArgs &A, const double *w, double *out, double scale, const int *done);
int run_path_sparse_wide(hipStream_t s, const PathArgs &a, const SpwArgs &A, double *host_scratch);
// the two lists of long lines (by A.plan's lanes) and the longest row and column: cnt (device, 4 ints) <- rows: number, longest | columns
int launch_spw_scan(hipStream_t s, const SpwArgs &A, int32_t *row_list, int32_t *col_list, int *cnt);
// xy = X'y / n, the scale slots of stats (colsq_inv with standardize, else 1) and xy_std = xy colsq_inv in one pass over the columns
int launch_spw_stats(hipStream_t s, const SpwArgs &A, const double *y, int standardize, double *xy, double *stats, double *xy_std);
// loss[k] = sum (y - X b_k)^2 of the returned coefficients b [nk][rows] (slot 0: the intercept); t: n doubles, part: nk ceil(n / 2048)
int launch_spw_loss(hipStream_t s, const SpwArgs &A, const double *y, const double *b, int rows, int nk, double *t, double *part, double *loss);
static const int WIDE_GRUN_MAX = 64;  // longest run (group) the fused group kernel takes
static const int WIDE_MAX_N = 32768;         // 16 row blocks of 2048 rows
size_t wide_scratch_doubles(int n, int p);      // (its regions: path_large_layout.hpp, WideScratch)
int launch_wide_standardize(hipStream_t s, const double *x, int64_t n, int64_t ld, int p, const double *y, int standardize, int intercept,
                            const WideLayout &lay, double *xs, double *ys, double *xy, double *stats);
int launch_big_wide_scales(hipStream_t s, const double *x, int64_t n, int64_t ld, int p, const double *xy, double *stats, double *xy_std);
int launch_big_gram_scales(hipStream_t s, const double *xx, const double *xy, int p, int standardize, double *stats, double *xy_std);
int run_path_wide(hipStream_t s, const PathArgs &a, const WideArgs &w, double *host_scratch);
// the same iteration as ONE persistent launch of cooperating workgroups with Xs in registers (path_wcoop.hip): element-wise
// penalties, one row block, p <= 4 CW WCOOP_GMAX columns (CW = 16 / 8 / 4 by column height); WCOOP_GMAX = three quarters of the CUs
static const int WCOOP_GMAX = 192, WCOOP_MAX_SETS = 8;
int path_wcoop_workgroups(int n, int p);
int path_wcoop_cpg(int n);                                        // columns per workgroup (0: not this engine)
int path_wcoop_max_workgroups(int n, int p);                     // ... of a partition cut at group boundaries, at most
int path_wcoop_sets(int n, int p, int npen, int num_cu, int G = 0);   // workgroup sets side by side, one penalty each (G: of a cut partition)
size_t path_wcoop_xchg_doubles(int n, int p);
size_t path_wcoop_launch_doubles(int n, int p, int G, int sets);
bool path_wcoop_eligible(const PathArgs &a, const WideArgs &w);
int launch_path_wcoop(hipStream_t s, const PathArgs &a, const WideArgs &w, int sets, const int *cstart = nullptr, int G = 0);   // cstart (device, G + 1 ints): columns cut at group boundaries
// the same where Xs does not fit the registers: G persistent workgroups re-read their column tiles every iteration (path_wcoop.hip: path_wstream_kernel)
size_t path_wstream_xchg_doubles(int n);
// ... and with more column sets of every wave in the accumulator file (path_wres_kernel): Xs up to ~11 M entries in registers
int path_wres_workgroups(int n, int p);
size_t path_wres_xchg_doubles(int n, int p);
bool path_wres_eligible(const PathArgs &a, const WideArgs &wd, int max_wg);
int launch_path_wres(hipStream_t s, const PathArgs &a, const WideArgs &wd);
bool path_wstream_eligible(const PathArgs &a, const WideArgs &w, int G);
int launch_path_wstream(hipStream_t s, const PathArgs &a, const WideArgs &w, int G);

// opts->interrupt of the call in progress on this thread (paths.hip: run_paths sets it around the engines); false if none
bool caller_interrupted();

// api.hip: the argument checks of the Gaussian entry points (check_opts) for other translation units
int check_opts_export(const oemgpu_opts *o, int p, int ngroupvars_expected);
// path_large.hip: out = M vec for a symmetric q x q M (skipped while *done != 0)
int launch_gemv_sym(hipStream_t s, const double *M, int q, const double *vec, double *out, const int *done, int num_cu);

int launch_eig_small(hipStream_t s, const double *a, int p, int steps, double *out /* [d, lambda_max] */);

__host__ __device__ static inline bool pen_is_net(int pen)
{
    return pen == OEMGPU_ELASTIC_NET || pen == OEMGPU_MCP_NET || pen == OEMGPU_SCAD_NET ||
           pen == OEMGPU_GRP_LASSO_NET || pen == OEMGPU_GRP_MCP_NET || pen == OEMGPU_GRP_SCAD_NET;
}
__host__ __device__ static inline bool pen_is_grp(int pen) { return pen >= OEMGPU_GRP_LASSO; }

}  // namespace oemgpu
