/*
 * oemgpu.h -- C ABI of the MI355X-native Orthogonalizing-EM solver (liboemgpu.so).
 *
 * Drop-in boundary for the dense Gaussian hot path of jaredhuling/oem (reference @ 2024_08_07):
 * the three entry points below are what the reference's `.Call` targets would bind instead of
 * their RcppEigen bodies (INTEGRATION.md shows the R-side shim).  Plain pointers and sizes only;
 * everything is IEEE fp64, matrices are column-major, outputs are caller-allocated, inputs are
 * never written.  All "ref:" citations are paths under the reference tree.
 *
 * Return value: 0 on success, <0 on error; oemgpu_last_error() gives the message
 * (thread-local).  There is NO CPU fallback: without a gfx950 device every compute entry
 * point fails with OEMGPU_ERR_NO_DEVICE.
 */
#ifndef OEMGPU_H
#define OEMGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OEMGPU_OK              0
#define OEMGPU_ERR_ARG        -1   /* invalid argument (the R front ends stop() on these: ref R/oem.R:215-431) */
#define OEMGPU_ERR_NO_DEVICE  -2
#define OEMGPU_ERR_HIP        -3   /* a HIP runtime call failed */
#define OEMGPU_ERR_UNSUPPORTED -4  /* outside the restated path (e.g. big.oem with p >= n, ref src/oem_big.h:547-551) */
#define OEMGPU_ERR_INTERNAL   -5
#define OEMGPU_ERR_INTERRUPTED -6  /* opts->interrupt asked to stop (the R shim then raises the pending user interrupt,
                                     ref src/oem_dense.cpp:235-238 Rcpp::checkUserInterrupt); every buffer is already released */

/* penalty codes = position in the R default vector (ref R/oem.R:165-173) */
enum {
    OEMGPU_ELASTIC_NET = 0, OEMGPU_LASSO = 1, OEMGPU_OLS = 2, OEMGPU_MCP = 3, OEMGPU_SCAD = 4,
    OEMGPU_MCP_NET = 5, OEMGPU_SCAD_NET = 6, OEMGPU_GRP_LASSO = 7, OEMGPU_GRP_LASSO_NET = 8,
    OEMGPU_GRP_MCP = 9, OEMGPU_GRP_SCAD = 10, OEMGPU_GRP_MCP_NET = 11, OEMGPU_GRP_SCAD_NET = 12,
    OEMGPU_SPARSE_GRP_LASSO = 13, OEMGPU_NPENALTIES = 14
};

/* Arguments shared by the three entry points: the scalar/vector arguments of
 * oem_fit_dense (ref src/oem_dense.cpp:30-48), oem_xtx (ref src/oem_xtx.cpp:29-44) and
 * oem_fit_big (ref src/oem_big.cpp:30-48) after R's coercions (ref R/oem.R:411-445). */
typedef struct oemgpu_opts {
    int32_t        npen;             /* length(penalty) >= 1 */
    const int32_t *penalty;          /* npen codes */
    int32_t        nlambda;          /* nlambda_, used when no lambda is supplied */
    double         lambda_min_ratio; /* lmin_ratio_ */
    const double  *lambda_user;      /* lambda_: npen x nlambda_user, one row per penalty, each sorted
                                        decreasing (ref R/oem.R:366-404); NULL => generated grid */
    int32_t        nlambda_user;
    double         alpha, gamma, tau;
    double         tol;              /* opts$tol */
    int32_t        maxit;            /* opts$maxit */
    int32_t        accelerate;       /* opts$accelerate (dense only, ref src/oem_dense.h:633-651) */
    int32_t        compute_loss;     /* compute_loss_ (dense only) */
    const double  *penalty_factor;   /* p values */
    const int32_t *groups;           /* ngroupvars values or NULL; big.oem with intercept passes p+1
                                        values with a leading 0 (ref R/big_oem.R:254-257) */
    int32_t        ngroupvars;
    const int32_t *unique_groups;    /* ngroups values, sorted (ref R/oem.R:292) */
    int32_t        ngroups;
    const double  *group_weights;    /* n_group_weights values; 0 => sqrt(group size) (ref src/oem_dense.h:447-454) */
    int32_t        n_group_weights;
    int32_t        device;           /* HIP device ordinal; -1 => current device */
    /* ---- host-resident entry points only (oemgpu_fit_dense, oemgpu_fit_big); zero / NULL = the defaults ---- */
    int32_t        ngpus;            /* G > 1: the rows are split over G devices inside the library, floor(n / G) rows each and
                                        the remainder on the last (as the reference's row blocks, ref src/oem_dense.h:328,343,
                                        src/oem_big.h:329-358); every device builds the moments of its rows and they are summed
                                        in device order on the first one (peer copies over xGMI), which solves.  0 or 1: `device` */
    const int32_t *devices;          /* ngpus ordinals, or NULL => device, device + 1, ... (device = -1 => 0, 1, ...) */
    int32_t        upload_threads;   /* host staging threads per device (pageable rows -> pinned bounce slots -> H2D); 0 => 8 */
    int          (*interrupt)(void *);   /* polled between row blocks and between penalties / batches of iterations;
                                            non-zero => OEMGPU_ERR_INTERRUPTED after cleanup.  NULL => never polled */
    void          *interrupt_arg;
} oemgpu_opts;

/* -------------------------------------------------------------------------------------------
 * Drop-in entry points (host buffers in, host buffers out; exactly the data the .Call carries).
 *
 * nl below = nlambda_user if lambda_user != NULL else nlambda.
 * beta:       npen * nl * (p+1) doubles; beta[(k*nl + i)*(p+1) + j] = coefficient j (0 = intercept)
 *             of penalty k at lambda i, i.e. each penalty's block is the reference's (p+1) x nl
 *             column-major matrix (ref src/oem_dense.cpp:194,252-254).  For "ols" only i = 0 is
 *             meaningful (ref :208-211,282-288).  oemgpu_fit_xtx: p rows, no intercept row
 *             (ref src/oem_xtx.cpp:129).
 * lambda_out: npen * nl, the unscaled lambda actually used (ref src/oem_dense.cpp:278)
 * niter:      npen * nl (maxit+1 when the loop ran out, ref src/oem_base.h:94-109)
 * loss:       npen * nl, 1e99 unless compute_loss (ref src/oem_dense.cpp:229-230,256-260)
 * d:          1.005 * lambda_max(X'X/n) (ref src/oem_dense.h:498)
 * ------------------------------------------------------------------------------------------- */

/* replaces oem_fit_dense, ref src/oem_dense.cpp:30-309 (family "gaussian", weights empty).
 * Both branches of ref src/oem_dense.h:476-482: n > p, and p >= n, where the reference iterates through X twice
 * (u = X'(Y - X b)/n + d b, d from XXt/n, ref :363-366, 513-521).  The library runs that very form -- a standardised copy of x
 * on the device, one read of it per iteration, no p x p matrix -- where it pays (n <= 32768, p > 1024 and 2 n < p: p = 20,000
 * needs 80 MB instead of 3.2 GB), and the same iteration written on the Gram elsewhere. */
int oemgpu_fit_dense(const double *x, int64_t n, int32_t p, const double *y,
                     int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                     double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);

/* replaces oem_xtx, ref src/oem_xtx.cpp:29-219.  scale_factor: p values or NULL. */
int oemgpu_fit_xtx(const double *xtx, const double *xty, int32_t p, const double *scale_factor,
                   const oemgpu_opts *o,
                   double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);

/* replaces oem_fit_big / oem_fit_fb_big, ref src/oem_big.cpp:30-258, src/oem_fb_big.cpp:30-258.
 * The big.matrix is handed over as row shards (the reference itself slices rows,
 * ref src/oem_big.h:319-361): shard s holds n_shard[s] rows, column-major with leading
 * dimension n_shard[s].  One shard of n rows is the plain big.matrix buffer. */
int oemgpu_fit_big(const double *const *x_shards, const int64_t *n_shard, int32_t nshards, int32_t p,
                   const double *const *y_shards,
                   int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                   double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);

/* oem_fit_dense with a non-empty `weights_` (ref src/oem_dense.cpp:34,75,152,162; src/oem_dense.h:368-414, 699-707, 759-770;
 * src/DataStd.h:94-202): the R front end never sends one ("weights not implemented yet", R/oem.R:244), the compiled entry takes it.
 * Computed as the reference computes it (sqrt(w)-weighted DataStd statistics -- unweighted for x under flag 3 --, X'WX / n, X'(Yw) / n,
 * loss = sum w r^2; with nobs <= nvars d from (sqrt(w) X)(sqrt(w) X)'/n but the iteration X'((Y - X beta) w^2)/n + d beta, w SQUARED, as
 * src/oem_dense.h:513-517 has it -- there through the p x p Gram forms on the launch-per-iteration engine).  weights: n values, finite, >= 0. */
int oemgpu_fit_dense_weighted(const double *x, int64_t n, int32_t p, const double *y, const double *weights,
                              int32_t standardize, int32_t intercept, const oemgpu_opts *opts,
                              double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);

/* replaces oem_fit_sparse, ref src/oem_sparse.cpp:30-267 (family "gaussian", weights empty): oem() on a dgCMatrix.
 * colptr[p + 1] with colptr[0] = 0, non-decreasing; rowidx[nnz] in [0, n), strictly increasing inside a column; values[nnz]
 * (the compressed sparse column slots @p, @i, @x; explicit zeros allowed).  Outputs as oemgpu_fit_dense.  The semantics are
 * oemSparse's, not oemDense's: no centring, columns scaled by sqrt(sum x^2 / (n - 1)), the intercept as a Gram column of value
 * sqrt(mean diag / n) whose coefficient is rescaled in place after every lambda (ref src/oem_sparse.h:493-615, 897-917), lambda_zero
 * without the intercept slot (:854-863).  compute_loss (ref :919-944) for p + intercept <= 288.  With n > p the Gram takes one of two
 * routes: the compressed-column kernel when it fits in LDS, nnz <= 2 % of n p and n < 2^31, else the dense FP64-MFMA pass over
 * zero-filled row tiles of x (<= 2 GiB each).  n <= p is served without an intercept (OEMGPU_ERR_UNSUPPORTED with one, said before
 * the arrays are checked and before any device is looked for): with nnz <= 2 % of n p and p > 1024 from the non-zeros themselves
 * (oemgpu_fit_sparse_wide_res on a handle built for the call and freed after it: nothing of n p entries on the host or the device,
 * any n the int32 row indices can name), else through a dense n x p copy and the dense p >= n engines as before.
 * Malformed compressed-column arrays get OEMGPU_ERR_ARG before any device is looked for. */
int oemgpu_fit_sparse(int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values, const double *y,
                      int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                      double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);

/* replaces oem_xval_dense, ref src/oem_xval_dense.cpp:31-482 (family "gaussian", weights empty): xval.oem's fast
 * cross-validation.  foldid: n values in 1..nfolds.  type_measure: 0 "mse", 1 "mae" (ref :378-411).
 * beta, lambda_out, niter, loss, d: the fit on ALL rows, laid out as in oemgpu_fit_dense (loss only if compute_loss,
 * ref :296-301).  cvm, cvsd: npen * nl each -- mean over the n observations of the error of row i under the fit that
 * left row i's fold out, and sqrt(sample variance / n) of the same (ref :452-461; 0 beyond the single "ols" entry). */
int oemgpu_xval_dense(const double *x, int64_t n, int32_t p, const double *y, const double *weights, const int32_t *foldid, int32_t nfolds,
                      int32_t standardize, int32_t intercept, int32_t type_measure, const oemgpu_opts *o,
                      double *beta, double *lambda_out, int32_t *niter, double *loss, double *d,
                      double *cvm, double *cvsd);

/* xval.oem on a dgCMatrix: the call R's front end names (ref R/oem_xval.R:500, .Call("oem_xval_sparse")) and the reference never
 * shipped (ref R/oem_xval.R:196-201 stops with "sparse matrices not supported yet"; src/oem_init.c registers oem_xval_dense only).
 * Host arrays in, the argument order of oemgpu_xval_dense without `weights`; the compressed-column arrays as in oemgpu_fit_sparse.
 * It returns what oemgpu_xval_dense returns on the dense copy of the matrix -- oemXvalDense's semantics (centring and scaling recovered
 * from moments about 0, the folds on the full fit's lambda grid, cvm / cvsd as there), NOT oemSparse's -- to the last bits of the
 * moments, and never builds that copy: the columns are rewritten in fold order on the device (fold segments start on multiples of
 * 8192 rows), the K fold moment buffers come from ONE pass over the non-zeros by the route of oemgpu_fit_sparse (compressed columns
 * with chunk ranges cut at fold boundaries, or zero-filled row tiles per fold), the K + 1 fits are those of the dense call, and the
 * CV error is taken over the compressed rows.  nfolds in 2..512; n + 8192 nfolds >= 2^31 is OEMGPU_ERR_UNSUPPORTED; n <= p, or a fold
 * whose removal leaves <= p rows, is refused like the dense call; a fold id outside 1..nfolds is OEMGPU_ERR_ARG; malformed
 * compressed-column arrays get OEMGPU_ERR_ARG before any device is looked for.  Observation weights and opts.ngpus > 1 are not served
 * on a sparse x (OEMGPU_ERR_UNSUPPORTED for the latter). */
int oemgpu_xval_sparse(int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values, const double *y,
                       const int32_t *foldid, int32_t nfolds, int32_t standardize, int32_t intercept, int32_t type_measure,
                       const oemgpu_opts *o,
                       double *beta, double *lambda_out, int32_t *niter, double *loss, double *d,
                       double *cvm, double *cvsd);
/* HIP-event times (ms) of the phases of this thread's last oemgpu_xval_sparse call: [0] upload, [1] fold order (layout, permuted
 * columns, chunk pointers), [2] fold moments, [3] compressed rows, [4] the K + 1 fits, [5] CV error. */
#define OEMGPU_XVS_NPHASES 6
int oemgpu_last_xval_sparse_timings(double *ms /* OEMGPU_XVS_NPHASES */);
/* Host-only plan of oemgpu_xval_sparse (pure arithmetic, runs without a GPU; the call takes its shape from the same function) for
 * n rows, p columns, nnz non-zeros, nfolds folds, npen penalties, nl lambdas on a device of num_cu CUs:
 * out[0] route (1 compressed columns, 0 row tiles: the rule and switches of oemgpu_fit_sparse), [1] chunks of 8192 rows at most
 * (floor(n / 8192) + nfolds), [2] chunks per range of the Gram launch, [3] ranges per fold at most, [4] ranges in all at most,
 * [5] rows per tile (tile route), [6] CV-error workgroups (x npen x [8]), [7] CV-error waves = partials, [8] blocks of 64 lambdas,
 * [9] device bytes of the whole call, [10] the fold alignment (8192), [11] LDS bytes of the Gram kernel (0 on the tile route); and
 * for the folds (n - nfolds + 1, 1, 1, ...), cut by the function the call uses: [12] ranges of fold 1, [13] ranges in all,
 * [14] rows of the fold-ordered layout, [15] the chunk at which fold 1's last range ends (= its chunks: no range goes beyond),
 * [16] the tiles of fold 1 on the tile route (laid from the fold's first row), [17] the row of the fold at which its last tile ends
 * (= its rows: no tile goes beyond).
 * OEMGPU_ERR_ARG for non-positive arguments, nfolds outside 2..512 or a NULL out; OEMGPU_ERR_UNSUPPORTED for n + 8192 nfolds >= 2^31. */
int oemgpu_selftest_xval_sparse_plan(int64_t n, int32_t p, int64_t nnz, int32_t nfolds, int32_t npen, int32_t nl, int32_t num_cu,
                                     int64_t *out /* 18 */);
/* Test infrastructure: the fold order and the K fold moment buffers of oemgpu_xval_sparse alone (nothing is fitted, n <= p is fine):
 * moments_out[nfolds][(p + 2)^2], the moment buffer about 0 of every fold's rows (an absent fold: zeros). */
int oemgpu_selftest_xval_sparse_fold_moments(int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values,
                                             const double *y, const int32_t *foldid, int32_t nfolds, double *moments_out);
/* Test infrastructure: the fold order, the compressed rows and the CV-error phase of oemgpu_xval_sparse on a coefficient table of the
 * caller's, coef[nfolds][npen][nl][p + 1] (slot 0 the intercept), mirroring oemgpu_selftest_xval_cv_error_dev: cvm / cvsd [npen][nl]
 * (no "ols" masking), or with triples != NULL triples[npen][nl][3] = (count, mean, M2) for oemgpu_xval_merge. */
int oemgpu_selftest_xval_sparse_cv_error(int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values,
                                         const double *y, const int32_t *foldid, int32_t nfolds, const double *coef, int32_t npen,
                                         int32_t nl, int32_t type_measure, double *cvm, double *cvsd, double *triples /* or NULL */);

/* -------------------------------------------------------------------------------------------
 * Device-resident / staged interface.  Used when X already lives in HBM (bench.py, repeated
 * solves) and by the one-process-per-GPU row-sharded driver (oem_amd/distributed.py), which
 * all-reduces the moment buffer between oemgpu_moments_dev and oemgpu_solve_moments_dev.
 * All *_dev pointers are device pointers on the context's device.
 * ------------------------------------------------------------------------------------------- */
typedef struct oemgpu_ctx oemgpu_ctx;

/* stream: a hipStream_t to run on, or NULL for a stream owned by the context */
oemgpu_ctx *oemgpu_create(int32_t device, void *stream);
void        oemgpu_destroy(oemgpu_ctx *ctx);
int         oemgpu_synchronize(oemgpu_ctx *ctx);

/* Moment buffer of the augmented, shifted data Z = [X - 1 c_x' | y - c_y | 1]:
 * q = p + 2; M is q x q column-major, lower triangle valid:
 *   M[i,j] (i>=j, i,j<p) = sum_r (x_ri - c_i)(x_rj - c_j)      M[p,j]   = sum_r (y_r - c_y)(x_rj - c_j)
 *   M[p,p] = sum_r (y_r - c_y)^2     M[p+1,j] = sum_r (x_rj - c_j)     M[p+1,p] = sum_r (y_r - c_y)
 *   M[p+1,p+1] = number of rows.
 * Moments add over row shards that use the same shift, which is what the RCCL all-reduce sums. */
static inline int64_t oemgpu_moments_len(int32_t p) { return (int64_t)(p + 2) * (p + 2); }

/* Sample sums for the provisional shift (oemgpu_sums_len(p) doubles): sums_dev[0..p-1] = sum over the sampled
 * rows of x_j, sums_dev[p] = same for y, sums_dev[p+1] = number of sampled rows, sums_dev[p+2 .. 2p+2] = the
 * sampled sums of squares of the same p+1 columns, sums_dev[2p+3] = 0.  All-reduce the whole buffer across row
 * shards.  The shift in effect is then a pure function of the buffer (identical in every kernel and rank):
 *   c_j = sums[j] / sums[p+1]  if ANY column has mean_j^2 > 2^8 var_j (sample mean / variance), else c = 0
 * -- un-shifted accumulation costs (mean/sd)^2 eps of relative accuracy on the centred moments, and is used when
 * that is < 6e-14 because every x - c is an FP64 VALU op competing with the FP64 MFMA for the DP units. */
static inline int64_t oemgpu_sums_len(int32_t p) { return 2 * (int64_t)(p + 1) + 2; }
int oemgpu_shift_sums_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p,
                          const double *y_dev, double *sums_dev);

/* moments_dev <- moments of rows [0,n) about the shift c defined above (sums_dev: the (all-reduced)
 * output of oemgpu_shift_sums_dev; NULL => c = 0).
 * Replaces DataStd's passes + X'Y + XtX (ref src/DataStd.h:203-265, src/oem_dense.h:318-361,704-707;
 * src/oem_big.h:743-841) with ONE pass over X. */
int oemgpu_moments_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p,
                       const double *y_dev, const double *sums_dev, double *moments_dev);

/* out_dev[i] = ((parts[0][i] + parts[1][i]) + parts[2][i]) + ...: `nparts` buffers of `len` doubles, contiguous one behind the other
 * (an all-gather of the ranks' moment buffers), added in shard order by ONE kernel -- the order the in-library multi-GPU path
 * (opts.ngpus) adds its devices' buffers in, so both forms return the same bits whatever algorithm a collective library would
 * choose for an all-reduce.  The reference's own order is the arrival order of its threads at a critical section
 * (ref src/oem_dense.h:328-358).  Asynchronous on the context's stream. */
int oemgpu_sum_in_order_dev(oemgpu_ctx *ctx, const double *parts_dev, int32_t nparts, int64_t len, double *out_dev);

/* semantics selector for oemgpu_solve_moments_dev */
#define OEMGPU_SEM_DENSE 0   /* DataStd + oemDense (ref src/DataStd.h, src/oem_dense.h) */
#define OEMGPU_SEM_BIG   1   /* oemBig: (n-1)-scaling, intercept as Gram row/column (ref src/oem_big.h:731-842,469-566) */
#define OEMGPU_SEM_XVAL  3   /* oemXvalDense: oemBig's algebra (ref src/oem_xval_dense.h:745-789), lambda_zero without the intercept
                              * slot (:1025-1032), groups scanned over all p + 1 slots (:636), compute_loss allowed (:1088-1117) */

/* From (all-reduced) moments to the full result: standardisation constants, XX, XY, d, lambda grid,
 * penalty x lambda loops, recover.  Outputs are HOST buffers as in oemgpu_fit_dense. */
int oemgpu_solve_moments_dev(oemgpu_ctx *ctx, const double *moments_dev, const double *sums_dev, int32_t p,
                             int32_t semantics, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                             double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);

/* oemgpu_fit_dense with X (n x p, leading dimension ld >= n) and y already on the device. */
int oemgpu_fit_dense_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                         int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                         double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);
/* The same three calls on a ROW-major x that is read where it lies: x_dev is n x p with row stride ldr >= p (in elements) of
 * dtype OEMGPU_F64 or OEMGPU_F32, aligned to its element size only; columns p .. ldr - 1 of a row and everything past element
 * (n - 1) ldr + p - 1 are never read.  y_dev is a contiguous float64 vector.  They replace the copies a caller with such a matrix
 * had to make in front of the column-major calls above -- the float64 conversion and the transposed copy: one n x p float64 temporary
 * for a float64 x, two for a float32 x, each written and read once -- and, as those calls, DataStd's passes + X'Y + XtX (ref src/DataStd.h:203-265,
 * src/oem_dense.h:318-361,704-707) with ONE pass over X.  float32 elements become float64 as they are loaded; every product and sum
 * is FP64 (the FP64 MFMA), in one fixed order: two calls return the same bytes, and a float32 x returns what its float64 copy does.
 *   oemgpu_shift_sums_rm_dev: the sums buffer of oemgpu_shift_sums_dev on the column-major float64 copy, bit for bit.
 *   oemgpu_moments_rm_dev:    the moment buffer above (both triangles written), about the shift sums_dev defines (NULL: 0); equal
 *                             to oemgpu_moments_dev's up to the rounding of another summation order.  1 <= p <= OEMGPU_RM_P_MAX.
 *   oemgpu_fit_dense_rm_dev:  oemgpu_fit_dense_dev with these passes (the second, shifted pass included when the first solve
 *                             advises it; the same timers).  n > p only: where the p >= n engine would take the call, and for
 *                             p > OEMGPU_RM_P_MAX, OEMGPU_ERR_UNSUPPORTED -- those shapes take the column-major entry.
 * OEMGPU_ERR_ARG before any device work: a NULL ctx or pointer, dtype outside {0, 1}, n < 1, p < 1, ldr < p. */
#define OEMGPU_F64 0
#define OEMGPU_F32 1
#define OEMGPU_RM_P_MAX 1024
int oemgpu_shift_sums_rm_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p,
                             const double *y_dev, double *sums_dev);
int oemgpu_moments_rm_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p,
                          const double *y_dev, const double *sums_dev, double *moments_dev);
int oemgpu_fit_dense_rm_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                            int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                            double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);
/* Host-only plan of the row-major pass (pure arithmetic, runs without a GPU; the calls take their shape from the same function) for
 * n rows, p columns on a device of num_cu CUs: out[0] tile columns of [X | y | 1], [1] 4 x 4 tile blocks per row chunk, [2] row
 * chunks, [3] 16-row steps per chunk, [4] workgroups of the pass, [5] doubles of chunk partials, [6] the first row of the last
 * chunk (< n: no chunk is empty), [7] OEMGPU_RM_P_MAX.  OEMGPU_ERR_ARG for n, p, num_cu < 1 or a NULL out; OEMGPU_ERR_UNSUPPORTED for
 * p > OEMGPU_RM_P_MAX. */
int oemgpu_selftest_gram_rm_plan(int64_t n, int32_t p, int32_t num_cu, int64_t *out /* 8 */);

/* Many responses on one resident x: the m fits oemgpu_fit_dense_dev(ctx, x, ..., Y[:, r], ...) returns for r = 0 .. m - 1, from TWO reads
 * of x.  It replaces the loop of m such calls -- the only way so far, and what sklearn.linear_model.Lasso does with a 2-D y -- in
 * which every call runs the whole moment pass again although the Gram block, the column sums and the row count of the moment buffer
 * above depend on x alone: here ONE moment pass about 0 (response 0 riding as y; up to p = OEMGPU_RM_P_MAX the row-major pass's summation order whichever way x
 * lies, so that the fits are the same bytes from every layout of x; beyond, oemgpu_moments_dev's), ONE X'Y pass that forms sum_i x_ij y_ir, sum_i y_ir^2
 * and sum_i y_ir of every response on the FP64 MFMA in a fixed order (no atomics: two calls return the same bytes, and the three
 * layouts of x the same bytes for the same values), and the paths of up to 513 responses side by side in one launch (one workgroup
 * or one cooperating workgroup set per response, all the waiting workgroups of a launch within 3/4 of the CUs), every response with
 * the lambda grid of its own X'y; a user lambda grid is shared by all responses.
 * y_dev is float64, element (i, r) at y_dev[i * y_rs + r * y_cs] with either y_cs == 1 && y_rs >= m (a row-major n x m matrix) or
 * y_rs == 1 && y_cs >= n (a column-major one); nothing in the padding of x or y and nothing past element (n - 1, m - 1) is read.
 * Outputs (host): beta[m][npen][nl][p + 1], lambda_out / niter / loss [m][npen][nl], d[m], and route[m]: 0 the response was solved
 * in a batched launch, 1 one by one from its composed moment buffer (p > 1024, the cooperating engine switched off, or a device too
 * small for one cooperating set), 2 fitted again by the route of oemgpu_fit_dense_dev -- the sample pass and the shifted pass --
 * because its solve advised a shift (oemgpu_last_shift_advised: then x itself advises for every response, or this response does).
 * n > p only: n <= p (the shapes of the p >= n engines) is OEMGPU_ERR_UNSUPPORTED, as is p > OEMGPU_RM_P_MAX on a row-major x;
 * OEMGPU_ERR_ARG before any device is looked for: a NULL pointer, m < 1, a stride pair that is neither form, ld < n, ldr < p, a dtype
 * outside {0, 1}; opts.interrupt is polled between the batched launches (OEMGPU_ERR_INTERRUPTED). */
int oemgpu_fit_dense_multi_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p,
                               const double *y_dev, int64_t y_rs, int64_t y_cs, int32_t m,
                               int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                               double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, int32_t *route);
/* The same on a row-major x read where it lies (the x arguments of oemgpu_fit_dense_rm_dev; float32 widened in the register): it
 * replaces the loop of m oemgpu_fit_dense_rm_dev calls. */
int oemgpu_fit_dense_multi_rm_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p,
                                  const double *y_dev, int64_t y_rs, int64_t y_cs, int32_t m,
                                  int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                                  double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, int32_t *route);
/* Host-only plan of the two calls above (pure arithmetic, runs without a GPU; the calls take their shape from the same function) for
 * n rows, p columns, m responses and npen element-wise penalties of 100 lambdas on a device of num_cu CUs; layout 0: column-major x, 1: row-major.
 * out[0] rows per chunk of the X'Y pass (a multiple of 64), [1] row chunks (none empty), [2] responses per block of the X'Y kernel
 * (16, 32 or 64), [3] X'Y passes = response blocks = reads of x by that kernel, [4] responses per batched launch at most (1 where
 * they are solved one by one), [5] batched launches (or single solves), [6] the batch engine (OEMGPU_ENGINE_ROWS or
 * OEMGPU_ENGINE_COOP; 0: one by one), [7] device bytes of the call's buffers (base moments, one response column, chunk partials, the
 * composed buffers of one launch) plus the workspace reserved for the passes and the paths.
 * OEMGPU_ERR_ARG for n, p, m, npen, num_cu < 1, a layout outside {0, 1} or a NULL out; OEMGPU_ERR_UNSUPPORTED for n <= p and for
 * p > OEMGPU_RM_P_MAX with layout 1.  It stands where oemgpu_selftest_gram_rm_plan stands for the row-major pass. */
int oemgpu_selftest_multi_plan(int64_t n, int32_t p, int32_t m, int32_t npen, int32_t layout, int32_t num_cu, int64_t *out /* 8 */);
/* Test infrastructure: the moment pass, the X'Y pass and the composition of the two calls above alone (nothing is fitted, n <= p is
 * fine): moments_out_dev[m][(p + 2)^2] (device) <- buffer r = the moment buffer about 0 of (x, Y[:, 0]) with M[p, j], M[p, p],
 * M[p + 1, p] and their mirror images replaced by response r's.  dtype < 0: x_dev is column-major float64 with column stride ld;
 * else row-major of that dtype with row stride ld.  It replaces m calls of oemgpu_moments_dev / oemgpu_moments_rm_dev. */
int oemgpu_selftest_multi_moments_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ld, int32_t p,
                                      const double *y_dev, int64_t y_rs, int64_t y_cs, int32_t m, double *moments_out_dev);

/* oemgpu_fit_dense_weighted with X, y and the weights already on the device. */
int oemgpu_fit_dense_weighted_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                                  const double *weights_dev, int32_t standardize, int32_t intercept, const oemgpu_opts *opts,
                                  double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);

/* oemgpu_fit_xtx with xtx (p x p) / xty on the device. */
int oemgpu_fit_xtx_dev(oemgpu_ctx *ctx, const double *xtx_dev, const double *xty_dev, int32_t p,
                       const double *scale_factor, const oemgpu_opts *o,
                       double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);

/* 1 if the most recent oemgpu_solve_moments_dev (OEMGPU_SEM_DENSE) on this context was given moments about 0
 * (sums_dev == NULL) of data in which some column has mean^2 > 2^8 var -- the shift predicate above, evaluated on the
 * full-data moments.  The coefficients just returned may then have lost (mean/sd)^2 eps of relative accuracy to
 * cancellation: redo the pass about a shift (oemgpu_shift_sums_dev, oemgpu_moments_dev and this call with those sums).
 * 0 otherwise, -1 for a NULL context.  oemgpu_fit_dense(_dev) and the row-sharded driver do exactly this, so that the
 * usual data costs one pass and one collective, with no sample pass in front. */
int oemgpu_last_shift_advised(oemgpu_ctx *ctx);

/* oemgpu_xval_dense with X (n x p, leading dimension ld >= n), y, weights and foldid already on the device. */
int oemgpu_xval_dense_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                          const double *weights_dev /* or NULL */, const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept,
                          int32_t type_measure, const oemgpu_opts *o,
                          double *beta, double *lambda_out, int32_t *niter, double *loss, double *d,
                          double *cvm, double *cvsd);

/* xval.oem over row shards (one process per GPU; oem_amd/distributed.py: xval_oem_sharded): the three phases of
 * oemgpu_xval_dense_dev as separate calls, with the caller's collectives between them.  The cross-validation of the
 * reference is additive in exactly the way its fit is: per-fold Gram matrices are sums over rows
 * (ref src/oem_xval_dense.h:358-484), the K + 1 fits need nothing but those sums (ref src/oem_xval_dense.cpp:213-340),
 * and the CV error is a mean and a variance over observations (ref :343-461).  All three calls of one fit take the same
 * (n_local, p, nfolds, weighted, o); the fold-ordered copy of the local rows stays in the context between them.
 *   1. fold_moments_dev[oemgpu_xval_moments_len(p, nfolds, weighted)] <- per-fold moments of the LOCAL rows (device
 *      buffer: all-reduce it, sum), fold_n[nfolds] <- local fold sizes (host: all-reduce, sum);
 *   2. the summed moments and fold sizes in, the replicated fits out (beta ... d as in oemgpu_xval_dense);
 *   3. triples[npen * nl * 3] <- (count, mean, M2 = sum (v - mean)^2) of the LOCAL rows' errors (host: all-gather);
 *   oemgpu_xval_merge: the triples of all ranks, in rank order -> cvm, cvsd (Chan, Golub & LeVeque; pure host code). */
int64_t oemgpu_xval_moments_len(int32_t p, int32_t nfolds, int32_t weighted);
int oemgpu_xval_fold_moments_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n_local, int64_t ld, int32_t p, const double *y_dev,
                                 const double *weights_dev /* or NULL */, const int32_t *foldid_dev, int32_t nfolds, const oemgpu_opts *o,
                                 double *fold_moments_dev, int64_t *fold_n);
int oemgpu_xval_solve_folds_dev(oemgpu_ctx *ctx, const double *fold_moments_dev, const int64_t *fold_n_total, int64_t n_local, int32_t p,
                                int32_t nfolds, int32_t weighted, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                                double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);
int oemgpu_xval_cv_triples_dev(oemgpu_ctx *ctx, int64_t n_local, int32_t p, int32_t nfolds, int32_t weighted, int32_t type_measure,
                               const oemgpu_opts *o, double *triples);
int oemgpu_xval_merge(const double *triples, int32_t nsets, const oemgpu_opts *o, double *cvm, double *cvsd);

/* Test infrastructure (tests/test_gpu_xval_bounds.py): phase 3 of oemgpu_xval_dense_dev -- the cross-validation error -- on a coefficient
 * table of the caller's instead of fitted ones.  x_dev (n x p, leading dimension ld >= n), y_dev, weights_dev (or NULL) and foldid_dev
 * (1 .. nfolds) on the context's device; coef (host): [nfolds][npen][nl][p + 1], slot 0 the intercept, the table of fold k scoring the
 * rows of fold k.  The rows go through the same fold layout, gather and weight scaling, and the same launch, as in oemgpu_xval_dense_dev.
 * With v_i = (y_i - b_0 - x_i . b)^2 (type_measure 0) or |.| (1), times w_i with weights: triples == NULL: cvm[npen][nl] <- mean v,
 * cvsd[npen][nl] <- sqrt(sum (v - cvm)^2 / (n - 1)) / sqrt(n); else triples[npen][nl][3] <- (n, mean, sum (v - mean)^2) and cvm / cvsd
 * are left alone (they may be NULL).  No fit, no options, no "ols" masking, and n <= p is allowed.  The checks of oemgpu_xval_dense_dev on
 * nfolds (2..512), type_measure, n and ld apply (OEMGPU_ERR_ARG before a device is looked for, like NULL pointers and p, npen, nl < 1);
 * a fold id outside 1 .. nfolds is OEMGPU_ERR_ARG from the device. */
int oemgpu_selftest_xval_cv_error_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                                      const double *weights_dev /* or NULL */, const int32_t *foldid_dev, int32_t nfolds,
                                      const double *coef, int32_t npen, int32_t nl, int32_t type_measure, double *cvm, double *cvsd,
                                      double *triples /* or NULL */);
/* cv.oem(family = "gaussian") on a dense x that is resident on the device (R/cv_oem.R:129-175, 349-423; R/utils.R:64-144), in two
 * phases over the fold layout of the xval phases above (oemgpu_ctx keeps the fold-ordered rows between them).  The caller
 * interpolates between the two (lambda.interp, R/utils.R:64-98: pure host arithmetic on K small tables).
 *
 * 1. oemgpu_cv_fold_fits_dev replaces the K calls `oem(x[!which, ], y[!which], ...)` of R/cv_oem.R:155-175: fold ff's fit is
 *    oemgpu_fit_dense_dev on the rows whose id is not ff -- DataStd's constants from those rows, the fold's own lambda grid (unless
 *    opts carries the user's), y scaling -- without gathering them: rows go into fold order once, every fold segment yields one
 *    moment buffer, and fold ff is solved (OEMGPU_SEM_DENSE) from the sum of the others in fold order.  Moments are taken about 0
 *    first; if any fold's solve advises a shift (oemgpu_last_shift_advised), the sample sums of ALL rows are taken once, the K
 *    segment passes are made again about them and every fold is solved again with them (one shift keeps the buffers additive).
 *    Host outputs: beta[nfolds][npen][nl][p + 1], lambda_out / niter / loss [nfolds][npen][nl], d[nfolds], fold_n[nfolds].
 *    An id in 1..nfolds that never occurs is allowed: that fold's fit is the fit of all rows.
 *    Refused before a device is looked for: NULL pointers, the options (as oemgpu_fit_dense_dev), nfolds outside 2..512, n < 1,
 *    ld < n (OEMGPU_ERR_ARG), n + 16 nfolds >= 2^31, and n - ceil(n / nfolds) <= p -- the largest fold then leaves no more rows
 *    than columns whatever the ids are (OEMGPU_ERR_UNSUPPORTED).  From the device: an id outside 1..nfolds (OEMGPU_ERR_ARG), and
 *    n - n_k <= p for some fold k, named in the message (OEMGPU_ERR_UNSUPPORTED: that fit is the wide engine's, not this route's).
 *
 * 2. oemgpu_cv_score_dev replaces the prediction loop and the per-fold means of cv.oemfit_gaussian and cvcompute
 *    (R/cv_oem.R:376-391, R/utils.R:128-144).  coef (host): [nfolds][npen][nl][p + 1], slot 0 the intercept, the caller's table, fold
 *    k's scoring fold k's rows; ncol[npen] (0..nl): the leading columns of a penalty that are valid.  With v = (y - yhat)^2
 *    (type_measure 0) or |y - yhat| (1): triples[nfolds][npen][nl][3] <- (count, mean, M2 = sum (v - mean)^2) over fold k's rows,
 *    merged from the wave partials in a fixed order (two calls give the same bits); columns >= ncol[pen] and empty folds give
 *    (0, NaN, NaN).  predmat_dev: NULL, or a device buffer [npen][nl][n] that receives yhat in the CALLER'S row order, NaN in columns
 *    >= ncol[pen].  It needs the fold layout of a call of oemgpu_cv_fold_fits_dev on the same context with the same
 *    (n, p, nfolds, npen, nl); any xval / cv layout call on that context in between voids it: OEMGPU_ERR_ARG.  Refused before a
 *    device is looked for: NULL pointers, p, npen, nl < 1, an ncol outside 0..nl, nfolds outside 2..512, type_measure not 0 / 1. */
int oemgpu_cv_fold_fits_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                            const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                            double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, int64_t *fold_n);
int oemgpu_cv_score_dev(oemgpu_ctx *ctx, int64_t n, int32_t p, int32_t nfolds, const double *coef, int32_t npen, int32_t nl,
                        const int32_t *ncol, int32_t type_measure, double *triples, double *predmat_dev /* or NULL */);
/* Test infrastructure (tests/test_gpu_cv_gaussian.py): oemgpu_cv_score_dev after the fold layout alone -- the rows of x_dev / y_dev go
 * into fold order as in oemgpu_cv_fold_fits_dev, nothing is fitted (a fold may leave fewer rows than columns), then the scoring entry
 * runs as it is -- so that it can be held against dense random tables.  The row checks of phase 1 and the checks of phase 2. */
int oemgpu_selftest_cv_score_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                                 const int32_t *foldid_dev, int32_t nfolds, const double *coef, int32_t npen, int32_t nl,
                                 const int32_t *ncol, int32_t type_measure, double *triples, double *predmat_dev /* or NULL */);
/* xval.oem and the fold fits of cv.oem(family = "gaussian") on a ROW-major x of float64 or float32 elements, read where it lies (every
 * PyTorch tensor that was not transposed on purpose): x_dev as in oemgpu_fit_dense_rm_dev -- element (i, j) at x_dev[i * ldr + j], ldr
 * >= p, dtype OEMGPU_F64 or OEMGPU_F32, aligned to its element size only; columns p .. ldr - 1 of a row and rows >= n are never read.
 * The rows go into fold order straight from that x (xval.hip: fold_gather_rm_kernel, float32 widened in the register); the
 * fold-ordered copy is column-major float64 as before and holds the bytes the column-major entry builds from the float64 copy of the
 * same values, and everything behind it is that entry's code.  So
 *   oemgpu_xval_dense_rm_dev    gives what oemgpu_xval_dense_dev gives (weights_dev included), and
 *   oemgpu_cv_fold_fits_rm_dev  gives what oemgpu_cv_fold_fits_dev gives (the sample sums of a shifted re-pass come from the rows:
 *                               oemgpu_shift_sums_rm_dev's buffer), and leaves the layout oemgpu_cv_score_dev scores,
 * bit for bit.  There is no limit on p beyond the column-major entries' (OEMGPU_RM_P_MAX is the row-major MOMENT pass's; the moment
 * passes here run on the fold-ordered copy).  Refused before a device is looked for: what the column-major entry refuses, with its
 * codes and messages (its `ld < n` has no counterpart), and OEMGPU_ERR_ARG for a dtype that is neither code, ldr < p and an x_dev
 * that is not a multiple of its element size. */
int oemgpu_xval_dense_rm_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                             const double *weights_dev /* or NULL */, const int32_t *foldid_dev, int32_t nfolds, int32_t standardize,
                             int32_t intercept, int32_t type_measure, const oemgpu_opts *o,
                             double *beta, double *lambda_out, int32_t *niter, double *loss, double *d,
                             double *cvm, double *cvsd);
int oemgpu_cv_fold_fits_rm_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                               const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                               double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, int64_t *fold_n);
/* Test infrastructure (tests/test_gpu_cv_rowmajor.py): the fold layout and the row-major gather alone, into buffers of the caller's.
 * xo_dev: p columns of ldo doubles, ldo >= (n + 16 nfolds) rounded up to 16; yo_dev: ldo doubles; fold_n / fold_start (host, [nfolds])
 * <- the fold sizes and the position at which each fold's segment starts.  Row i of fold k, the r-th of its fold in the caller's
 * order, lands at xo_dev[j * ldo + fold_start[k] + r] and yo_dev[fold_start[k] + r]; nothing else is written.  Nothing is fitted, so
 * any n >= 1 and p >= 1 go.  The refusals of the entries above on dtype, ldr, alignment, nfolds (2..512) and n; OEMGPU_ERR_ARG for a
 * short ldo and, from the device, for a fold id outside 1 .. nfolds (such a row is not written). */
int oemgpu_selftest_fold_gather_rm_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p,
                                       const double *y_dev, const int32_t *foldid_dev, int32_t nfolds, double *xo_dev, int64_t ldo,
                                       double *yo_dev, int64_t *fold_n, int64_t *fold_start);
/* Host-only plan of the CV-error launch (xval.hip: cv_error_plan; pure arithmetic, runs without a GPU; the launch takes its shape from
 * the same function) for n rows, p columns, nfolds folds, npen penalties and nl lambdas on a device of num_cu CUs: out[0] lt = 16-lambda
 * tiles per pass (1..7: all ceil(nl / 16) tiles when there are <= 7, else the fewest passes of at most 7 made even), out[1] passes,
 * out[2] form: 0 SINGLE (the (p + 1 rounded up to 4) x 16 lt coefficient tile of a pass fits 140 KB of LDS and p + 1 <= 56: a lane holds
 * a row's fragments at once), 1 multi (fits, p + 1 > 56), 2 CHUNK (does not fit: 112 coefficient rows at a time), out[3] dynamic LDS
 * bytes, out[4] coefficient chunks (1 unless CHUNK), out[5] coefficient rows of the last chunk (a multiple of 4), out[6] workgroups per
 * (fold, penalty): floor(num_cu / (nfolds npen)), at most ceil(floor(n / nfolds) / 128), at least 1.
 * OEMGPU_ERR_ARG for non-positive arguments, nfolds outside 2..512 or a NULL out. */
int oemgpu_selftest_xval_cv_plan(int64_t n, int32_t p, int32_t nfolds, int32_t npen, int32_t nl, int32_t num_cu, int64_t *out /* 7 */);

/* xval.oem for m responses on ONE dense x: it replaces the loop of m oemgpu_xval_dense_dev calls with the same foldid, every one of
 * which lays out the folds, gathers x into fold order and runs the K fold Gram passes again although none of that depends on the
 * response.  Here: one fold layout, one gather of x and one of Y (read through its strides, as oemgpu_fit_dense_multi_dev reads it),
 * the K fold Gram passes once (response 0 riding as y), ONE X'Y pass over the fold-ordered rows for all responses (row chunks that never
 * straddle a fold; partials added in chunk order, no atomics: two calls return the same bytes, and so do the three layouts of x) --
 * then, per chunk of nb responses: their nb (K + 1) sums "all folds" / "all but fold ff" in one launch (folds in ascending order), the
 * nb (K + 1) paths in one batched launch of at most 513 instances, instance r (K + 1) + ff, every response's K + 1 fits on the lambda
 * grid of ITS full-data X'y, and the CV error of the nb responses in one launch and one finish launch.  A user lambda grid and foldid
 * are shared by all responses; there are no observation weights.
 * Outputs (host): beta[m][npen][nl][p + 1], lambda_out / niter / loss [m][npen][nl], d[m] (loss and d the full-data fit's), cvm / cvsd
 * [m][npen][nl], and route[m]: 0 the response's fits ran in a batched launch, 1 no batch engine takes the shape (q = p + intercept >
 * 1024, the cooperating engine switched off, or a launch too small for K + 1 instances) and its K + 1 sums went the way
 * oemgpu_xval_dense_dev solves them.  Element r is what oemgpu_xval_dense_dev returns for column r to the accuracy of the sums (the y
 * entries are added in another order).
 * Refused before a device is looked for: what oemgpu_xval_dense_dev / _rm_dev and oemgpu_fit_dense_multi_dev refuse of these
 * arguments, with their codes -- a NULL pointer, nfolds outside 2..512, a type_measure outside {0, 1}, m < 1, a stride pair of y that is
 * neither form, bad options -- and OEMGPU_ERR_UNSUPPORTED for n <= p and for n - ceil(n / nfolds) <= p (the largest fold leaves its
 * fit no more rows than columns); from the device: OEMGPU_ERR_ARG for a fold id outside 1..nfolds, OEMGPU_ERR_UNSUPPORTED for a fold
 * that leaves n - fold <= p rows.  opts.interrupt is polled between the chunks (OEMGPU_ERR_INTERRUPTED). */
int oemgpu_xval_dense_multi_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p,
                                const double *y_dev, int64_t y_rs, int64_t y_cs, int32_t m,
                                const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept,
                                int32_t type_measure, const oemgpu_opts *o,
                                double *beta, double *lambda_out, int32_t *niter, double *loss, double *d,
                                double *cvm, double *cvsd, int32_t *route);
/* The same on a row-major x read where it lies (the x arguments of oemgpu_xval_dense_rm_dev): the same bytes. */
int oemgpu_xval_dense_multi_rm_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p,
                                   const double *y_dev, int64_t y_rs, int64_t y_cs, int32_t m,
                                   const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept,
                                   int32_t type_measure, const oemgpu_opts *o,
                                   double *beta, double *lambda_out, int32_t *niter, double *loss, double *d,
                                   double *cvm, double *cvsd, int32_t *route);
/* HIP-event times (ms) of the last such call on this thread, taken while oemgpu_set_timing is on (the clock waits for the end of
 * every phase; a phase that runs once per chunk of responses is added up): [0] fold order and the gathers of x and Y, [1] the fold
 * Gram passes, [2] the fold X'Y pass, [3] the composition of the sums, [4] the paths, [5] the CV error.  All 0 with timing off. */
#define OEMGPU_XVM_NPHASES 6
int oemgpu_last_xval_multi_timings(double *ms /* OEMGPU_XVM_NPHASES */);
/* Host-only plan of the two calls (pure arithmetic; the calls take their shape from the same function) for n rows, p columns, nfolds
 * folds, m responses, npen element-wise penalties of nl lambdas and an intercept on a device of num_cu CUs:
 * out[0] nb = responses per solve chunk, [1] solve chunks (none empty), [2] the batch engine (OEMGPU_ENGINE_ROWS / _COOP; 0: none),
 * [3] route (0 / 1), [4] rows per chunk of the X'Y pass, [5] the most (fold) chunks that pass can have (n / rows rounded up, + nfolds:
 * what its partials are sized for), [6] response blocks = reads of x by that pass, [7] responses per block, [8] workgroups per (fold,
 * penalty, response) of the CV-error launch: floor(num_cu / (nfolds npen nb)), at most oemgpu_selftest_xval_cv_plan's, at least 1,
 * [9] bytes of the single-response layout (fold order, fold-ordered x, fold moments), [10..17] bytes of: response 0 as a vector, the
 * fold-ordered Y, the folds' first chunks, the X'Y partials, one chunk's composed sums (nb (nfolds + 1) (p + 2)^2 8), its fold
 * tables (nb nfolds npen nl (p + 1) 8), its CV-error partials, its (cvm, cvsd); [18] the aux bytes of the call: [9] plus [10..17]
 * each rounded up to 256, [19] the instances a batched launch may hold (multi_solve_plan's cap at q = p + 1).
 * OEMGPU_ERR_ARG for non-positive arguments, nfolds outside 2..512 or a NULL out; OEMGPU_ERR_UNSUPPORTED for n <= p. */
#define OEMGPU_XVM_PLAN_LEN 20
int oemgpu_selftest_xval_multi_plan(int64_t n, int32_t p, int32_t nfolds, int32_t m, int32_t npen, int32_t nl, int32_t num_cu,
                                    int64_t *out /* OEMGPU_XVM_PLAN_LEN */);
/* Test infrastructure: the fold order, the fold Gram passes, the fold X'Y pass and the composition alone (nothing is fitted, n <= p is
 * fine): moments_out_dev[m][nfolds][(p + 2)^2] (device) <- buffer (r, k) = the moment buffer about 0 of fold k's rows of (x, Y[:, r]),
 * both triangles written.  dtype < 0: x_dev is column-major float64 with column stride ld; else row-major of that dtype. */
int oemgpu_selftest_xval_multi_fold_moments_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ld, int32_t p,
                                                const double *y_dev, int64_t y_rs, int64_t y_cs, int32_t m,
                                                const int32_t *foldid_dev, int32_t nfolds, double *moments_out_dev);

/* cv.oem, family = "gaussian", for m responses on ONE dense x: it replaces the loop of m (oemgpu_fit_dense_dev, oemgpu_cv_fold_fits_dev,
 * oemgpu_cv_score_dev) triples with the same foldid -- cv.oem's K + 1 calls of oem() per response (R/cv_oem.R:105, 129-175), the
 * prediction loop and the per-fold means of cv.oemfit_gaussian (R/cv_oem.R:349-423) and predict.oem's lambda.interp (R/utils.R:64-144).
 * Here: the fold layout, the gathers of x and Y, the K fold Gram passes and the ONE fold X'Y pass of oemgpu_xval_dense_multi_dev, once;
 * then, per chunk of nb responses: their nb (K + 1) sums "all folds" / "all but fold ff" in one launch, the nb (K + 1) paths in one
 * batched launch of at most 513 instances under oem()'s own semantics -- every instance its own standardisation, y scale and lambda
 * grid from its own kept rows (instance r (K + 1) + ff) -- the index table of lambda.interp on the host (O(nb K npen nl) scalars:
 * (left, right, frac) of every fold grid at the valid leading lambdas of the full fit's, ncol = the count of full-grid lambdas >= the
 * largest of the folds' smallest), the interpolation beta[left] frac + beta[right] (1 - frac) on the device (rows from ncol on zero),
 * and the held-out rows of the nb responses scored in one launch and one finish launch.  A user lambda grid and foldid are shared by
 * all responses; there are no observation weights.  The sums are taken in a fixed order: two calls return the same bytes, and so do
 * the three layouts of x.
 * Outputs (host): beta[m][npen][nl][p + 1], lambda_out / niter / loss [m][npen][nl], d[m]: the m full fits as
 * oemgpu_fit_dense_multi_dev lays them out; ncol[m][npen]; triples[m][nfolds][npen][nl][3] = (count, mean, M2) of every fold's
 * errors, (0, NaN, NaN) in columns >= ncol and for a fold without rows, as oemgpu_cv_score_dev writes them; fold_n[nfolds]; route[m]:
 * 0 the response's K + 1 fits ran in a batched launch, 1 no batch engine takes the shape (p > 1024, the cooperating engine switched
 * off, or a launch too small for K + 1 instances) and its K + 1 sums were solved one after another, 2 one of its K + 1 solves advised
 * the shifted moment pass (a column or y with mean^2 > 256 var): nothing else is returned for that response (its ncol are 0) and the
 * caller runs the single route with its own shift rule on it (oemgpu_fit_dense_dev, oemgpu_cv_fold_fits_dev, oemgpu_cv_score_dev).
 * Optional (NULL, or host): fold_beta[m][nfolds][npen][nl][p + 1], fold_lambda / fold_niter [m][nfolds][npen][nl], the fold fits
 * themselves; predmat[m][npen][nl][n], yhat of every row from the fit that left its fold out, in the caller's row order, NaN from ncol
 * on (with it every chunk holds nb npen nl n doubles more on the device).
 * Refused before a device is looked for: what oemgpu_xval_dense_multi_dev refuses of these arguments, with its codes -- a NULL
 * pointer, nfolds outside 2..512, a type_measure outside {0, 1}, m < 1, a stride pair of y that is neither form, bad options
 * (OEMGPU_ERR_ARG) -- and OEMGPU_ERR_UNSUPPORTED for n <= p, for n - ceil(n / nfolds) <= p and for OEMGPU_OLS among the penalties (a
 * grid of one lambda: cv.oem's rule for it is served fold by fold, oemgpu_fit_dense_dev); from the device: OEMGPU_ERR_ARG for a
 * fold id outside 1..nfolds, OEMGPU_ERR_UNSUPPORTED naming the fold that leaves n - fold <= p rows.  A fold id in 1..nfolds that never
 * occurs is allowed, as in oemgpu_cv_fold_fits_dev: that fold's fit is the fit of all rows and its triples are (0, NaN, NaN).
 * opts.interrupt is polled between the chunks (OEMGPU_ERR_INTERRUPTED). */
int oemgpu_cv_dense_multi_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p,
                              const double *y_dev, int64_t y_rs, int64_t y_cs, int32_t m,
                              const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept,
                              int32_t type_measure, const oemgpu_opts *o,
                              double *beta, double *lambda_out, int32_t *niter, double *loss, double *d,
                              int32_t *ncol, double *triples, int64_t *fold_n, int32_t *route,
                              double *fold_beta, double *fold_lambda, int32_t *fold_niter, double *predmat);
/* The same on a row-major x read where it lies (the x arguments of oemgpu_xval_dense_multi_rm_dev; R/cv_oem.R:129-175, 349-423): the
 * same bytes, the same refusals and codes, and those of the row-major entries on dtype, ldr and alignment. */
int oemgpu_cv_dense_multi_rm_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p,
                                 const double *y_dev, int64_t y_rs, int64_t y_cs, int32_t m,
                                 const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept,
                                 int32_t type_measure, const oemgpu_opts *o,
                                 double *beta, double *lambda_out, int32_t *niter, double *loss, double *d,
                                 int32_t *ncol, double *triples, int64_t *fold_n, int32_t *route,
                                 double *fold_beta, double *fold_lambda, int32_t *fold_niter, double *predmat);
/* HIP-event times (ms) of the last such call on this thread, taken while oemgpu_set_timing is on (the clock waits for the end of every
 * phase; a phase that runs once per chunk of responses is added up): [0] fold order and the gathers of x and Y, [1] the fold Gram
 * passes, [2] the fold X'Y pass, [3] the composition of the sums, [4] the paths (R/cv_oem.R:129-175), [5] the interpolation
 * (R/utils.R:64-144; its uploads included), [6] the scoring (R/cv_oem.R:349-423; its downloads included).  All 0 with timing off.
 * OEMGPU_ERR_ARG for a NULL ms. */
#define OEMGPU_CVM_NPHASES 7
int oemgpu_last_cv_multi_timings(double *ms /* OEMGPU_CVM_NPHASES */);
/* Host-only plan of the two calls (pure arithmetic, runs without a GPU; the calls take their shape from the same function: how
 * R/cv_oem.R:129-175's K + 1 fits per response are grouped into launches and what R/cv_oem.R:349-423's tables take on the device) for n rows,
 * p columns, nfolds folds, m responses, npen element-wise penalties of nl lambdas on a device of num_cu CUs, with (keep != 0) or without
 * predmat, at most nb_limit responses per chunk (0: no limit of the caller's): out[0..19] the fields of oemgpu_selftest_xval_multi_plan
 * in its order, with the solve plan read at q = p (oem()'s solve centres the intercept out: [0] nb, [1] chunks, [2] engine, [3] route,
 * [8] the CV-error workgroups and [19] the cap are this call's; [4..7] and [9..13] are those of xval_oem_multi), [18] the aux bytes up to
 * there; [20..25] bytes of: one chunk's raw fold tables (= [15]), its index table (nb nfolds npen nl 16), its ncol (nb npen 4), the
 * inverse fold map (4 per fold-ordered row), its prediction block (nb npen nl n 8 with keep, else 0), its per-fold triples (nb nfolds
 * npen nl 24); [26] the aux bytes of the call: [18] plus [20..25] each rounded up to 256.
 * OEMGPU_ERR_ARG for non-positive arguments, a negative nb_limit, nfolds outside 2..512 or a NULL out; OEMGPU_ERR_UNSUPPORTED for n <= p. */
#define OEMGPU_CVM_PLAN_LEN 27
int oemgpu_selftest_cv_multi_plan(int64_t n, int32_t p, int32_t nfolds, int32_t m, int32_t npen, int32_t nl, int32_t num_cu, int32_t keep,
                                  int32_t nb_limit, int64_t *out /* OEMGPU_CVM_PLAN_LEN */);
/* Test infrastructure, host-only: from now on this thread's oemgpu_cv_dense_multi_dev / _rm_dev calls take at most nb_limit responses
 * per chunk (0: no limit again), as if the device's free memory had asked for it -- the path that brings triples and predmat down in
 * several copies (R/cv_oem.R:376-391: the prediction matrix).  OEMGPU_ERR_ARG for a negative nb_limit. */
int oemgpu_selftest_cv_multi_nb_limit(int32_t nb_limit);
/* Host-only (runs without a GPU): the index table of the call above from grids of the caller's -- lam_full[npen][nl] one full fit's
 * lambdas, lam_fold[nfolds][npen][nl] its fold fits' (descending) -> left / right / frac [nfolds][npen][nl] and ncol[npen]:
 * lambda.interp (R/utils.R:64-87) of every fold grid at the ncol leading lambdas of the full grid, (0, 0, 1) from ncol on.
 * OEMGPU_ERR_ARG for a NULL pointer or a non-positive count. */
int oemgpu_selftest_cv_interp(int32_t nfolds, int32_t npen, int32_t nl, const double *lam_full, const double *lam_fold,
                              int32_t *left, int32_t *right, double *frac, int32_t *ncol);
/* Test infrastructure, the many-response form of oemgpu_selftest_cv_score_dev (R/cv_oem.R:376-391): the fold layout, the gathers of x
 * (column-major) and Y, then the interpolation and the scoring of the call above alone, nb responses per launch, on tables of the
 * caller's; nothing is fitted, so a fold may leave fewer rows than columns.  coef[m][nfolds][npen][nl][p + 1] (host), ncol[m][npen]
 * (host).  left / right / frac ([m][nfolds][npen][nl], host) all NULL: coef is scored as it is; else coef goes through the
 * interpolation kernel first and table_out (NULL or host, coef's shape) <- what it wrote.  triples[m][nfolds][npen][nl][3] (host);
 * predmat_dev NULL or DEVICE [m][npen][nl][n].  OEMGPU_ERR_ARG for a NULL pointer, p / npen / nl / nb < 1, nfolds outside 2..512, a
 * type_measure outside {0, 1}, m < 1 or a bad stride pair of y, an ncol outside 0..nl, an index outside 0..nl-1, and, from the device,
 * a fold id outside 1..nfolds. */
int oemgpu_selftest_cv_score_multi_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                                       int64_t y_rs, int64_t y_cs, int32_t m, const int32_t *foldid_dev, int32_t nfolds,
                                       const double *coef, int32_t npen, int32_t nl, const int32_t *ncol, int32_t type_measure, int32_t nb,
                                       const int32_t *left, const int32_t *right, const double *frac, double *table_out,
                                       double *triples, double *predmat_dev);

/* The eigenvalue step of the most recent solve (or oemgpu_eig_max_dev) on this context: *steps = Lanczos steps taken, *capped = 1
 * if the recurrence ran into its step cap (min(2 q, 288) for q <= 288, 256 / 512 on the larger engines) instead of stopping by its
 * rule or by breakdown -- d = 1.005 x the last Ritz value is then a lower estimate (the reference's Spectra call, tol 1e-10 and up
 * to 10000 restarts, ref src/oem_dense.h:485-498, has no such cap; OEM converges for any d > lambda_max / 2).  -1 for a NULL context. */
int oemgpu_last_eigen_info(oemgpu_ctx *ctx, int32_t *steps, int32_t *capped);

/* Which kernel family ran the most recent penalty x lambda path on this context (diagnostics and tests: the engines are chosen by
 * size and options, api.hip: run_paths), and how many calls of a persistent engine so far timed out in their exchanges (somebody
 * else held the CUs) and were made again on the launch-per-iteration engines.  -1 for a NULL context. */
enum {
    OEMGPU_ENGINE_NONE = 0,
    OEMGPU_ENGINE_ROWS = 1,      /* p <= 288: one workgroup per penalty (path_small.hip) */
    OEMGPU_ENGINE_COOP = 2,      /* <= 1024: cooperating workgroups, one exchange per iteration (path_coop.hip) */
    OEMGPU_ENGINE_ROWCOOP = 3,   /* <= 2048, element-wise: the matrix in the accumulator files, one exchange (path_symcoop.hip) */
    OEMGPU_ENGINE_SYMCOOP = 4,   /* <= 4096: the lower triangle in registers, two exchanges (path_symcoop.hip) */
    OEMGPU_ENGINE_LAUNCHES = 5,  /* any p: launch-per-iteration engines on the Gram (path_large.hip) */
    OEMGPU_ENGINE_WCOOP = 6,     /* p >= n: the standardised X in vector registers (path_wcoop.hip) */
    OEMGPU_ENGINE_WRES = 7,      /* p >= n: ... and in the accumulator file (path_wcoop.hip: path_wres_kernel) */
    OEMGPU_ENGINE_WSTREAM = 8,   /* p >= n: persistent, X re-read every iteration (path_wcoop.hip: path_wstream_kernel) */
    OEMGPU_ENGINE_WLAUNCHES = 9, /* p >= n: launch-per-iteration (path_large.hip: run_path_wide) */
    OEMGPU_ENGINE_SPARSE_WIDE = 10 /* p >= n on a sparse x: both products over the non-zeros (sparse_wide.hip) */
};
int oemgpu_last_path_engine(oemgpu_ctx *ctx, int32_t *engine, int32_t *persistent_fallbacks);
/* The same for the entries that take host arrays and run on a context of the library's own (oemgpu_fit_sparse, oemgpu_fit_dense, ...):
 * the engine of the most recent penalty x lambda path run by the calling thread, on whatever context.  -1 for a NULL engine. */
int oemgpu_last_host_path_engine(int32_t *engine);
/* OEMGPU_ENGINE_COOP with q <= 512 puts the cooperating workgroups of an instance on ONE XCD where the device's layout allows (the
 * exchange then stays in that XCD's L2).  Of the most recent path launch on this context: 0 not asked for, 1 ran on one XCD, 2 asked for,
 * refused by the launch's own proof of placement and made again with the exchange at device scope (this context does not ask again),
 * 3 asked for, but an instance's workgroups were not all resident on its XCD (somebody else holds CUs there): made again once with the
 * workgroups anywhere on the device. */
int oemgpu_last_placement(oemgpu_ctx *ctx);

/* The most recent penalty x lambda path on this context, if the single-workgroup row-split kernel ran it (p <= 208; 0, 0 otherwise):
 * how many OEM rounds ran in the short form -- the product over the first ranked columns only, taken while the non-zeros of beta stay
 * within them (path_small.hip; OEM_NO_ACTIVE_PREFIX=1 never takes it: same bits, 0 short rounds) -- and how many rounds in all.
 * Of penalty 0 of instance 0 when the call has several penalties or instances.  -1 for a NULL context. */
int oemgpu_last_path_rounds(oemgpu_ctx *ctx, int64_t *short_rounds, int64_t *rounds);

/* 1 if the most recent oemgpu_solve_moments_dev on this context found the shift predicate above true for its
 * sums_dev (and so read moments_dev as accumulated about c), 0 if not, -1 for a NULL context. */
int oemgpu_last_shift_in_effect(oemgpu_ctx *ctx);

/* lambda_max of a symmetric p x p device matrix (the Spectra call of ref src/oem_dense.h:485-498). */
int oemgpu_eig_max_dev(oemgpu_ctx *ctx, const double *a_dev, int32_t p, double *lambda_max);

/* Time of the most recent kernels on this context, measured with HIP events on the context's
 * stream (milliseconds; 0 if that stage has not run).  Stages: */
#define OEMGPU_T_SHIFT   0
#define OEMGPU_T_MOMENTS 1   /* Gram/moment build (the MFMA kernel + its partial reduction) */
#define OEMGPU_T_FINAL   2   /* moments -> XX, XY, standardisation constants */
#define OEMGPU_T_EIGPATH 3   /* eigenvalue + penalty x lambda loops */
#define OEMGPU_T_GRAMK   4   /* the MFMA Gram kernel alone */
#define OEMGPU_T_FOLDORDER 5 /* xval.oem / cv.oem: the fold layout and the gather of the rows into fold order */
#define OEMGPU_T_PATHCYC 6   /* not a time: shader cycles of the last fused eigen+path kernel (p <= 192) */
#define OEMGPU_T_PATHTICKS 7 /* not a time: the same span in 100 MHz ticks (cycles / ticks * 100 MHz = clock held) */
#define OEMGPU_NTIMERS   8
int oemgpu_last_timings(oemgpu_ctx *ctx, double *ms /* OEMGPU_NTIMERS */);
/* enable (1) / disable (0) event timing of the stages (off by default: events cost a few us) */
int oemgpu_set_timing(oemgpu_ctx *ctx, int32_t on);

/* Row range [*r0, *r1) of device g of G for n rows: floor(n / G) each, the remainder on the last
 * (ref src/oem_dense.h:328,343).  Pure host arithmetic. */
void oemgpu_row_split(int64_t n, int32_t G, int32_t g, int64_t *r0, int64_t *r1);

/* What the most recent host-resident call (oemgpu_fit_dense / oemgpu_fit_big) of THIS thread did, for bench.py and the tests:
 * [0] wall milliseconds of the whole call  [1] of the upload + moment passes  [2] of the solve(s)  [3] bytes staged to the
 * devices  [4] devices used  [5] row blocks streamed (all devices)  [6] 1 if the rows stayed resident in HBM, 0 if two block
 * buffers were recycled  [7] hipMalloc / hipHostMalloc calls made inside the call (0 in the steady state of repeated calls)
 * [8] cross-device hand-overs of the moment buffers that were staged through the host because the two devices cannot access each
 *     other (hipDeviceCanAccessPeer; OEMGPU_NO_PEER=1 forces that route) -- 0 when every pair used one peer copy over xGMI. */
#define OEMGPU_NHOSTSTATS 9
int oemgpu_last_host_stats(double *out /* OEMGPU_NHOSTSTATS */);

/* Frees every cached context (streams, workspaces, pinned staging).  The host-resident entry points keep theirs between
 * calls; nothing else needs this.  Contexts in use by another thread are left alone. */
void oemgpu_release_cache(void);

/* Host-only self-check of the persistent p >= n engine's scratch sizing (pure arithmetic, runs without a GPU): for an n x p problem
 * with npen penalties on a device of num_cu CUs, 0 if every column partition the launch may choose gets at least one workgroup set
 * and never more sets than the exchange scratch was sized for; otherwise +/- the offending workgroup count. */
int oemgpu_selftest_wcoop_sizing(int32_t n, int32_t p, int32_t npen, int32_t num_cu);

/* Host-only self-check of the engine PLAN (pure arithmetic, runs without a GPU): what api.hip: plan_paths decides for a call with
 * these sizes and options on a device of num_cu CUs -- *engine = the OEMGPU_ENGINE_* of the first attempt (+ 256 where the cooperating
 * engine is planned with every instance on ONE XCD: run time still asks the device for its layout; + 512 k, k = 1, 2, 3, where the
 * launch engines would run group operators in the head of their (head, product) pairs with k blocks of 32 coordinates on either side of
 * a workgroup's own: every group a run of <= 32 k neighbouring coordinates) -- and whether the
 * buffers the callers size hold what the launch will carve: *frame_bytes (outputs + parameter blob + engine workspace) against
 * *reserved_bytes, and for p >= n (wide_n > 0 rows, no Gram matrix) the persistent engine's exchange buffers against the scratch
 * (*scratch_need_doubles <= *scratch_have_doubles).  p: columns of x; q: dimension of beta (p + 1 with big.oem's intercept);
 * semantics: OEMGPU_SEM_* (2: oem.xtx). */
int oemgpu_selftest_plan(int32_t p, int32_t q, int32_t semantics, int32_t intercept, const oemgpu_opts *o, int32_t has_scale, int32_t nbatch,
                         int64_t wide_n, int32_t num_cu, int32_t *engine, int64_t *frame_bytes, int64_t *reserved_bytes,
                         int64_t *scratch_need_doubles, int64_t *scratch_have_doubles);

/* Host-only self-check of the MOMENT plan (gram.hip: gram_plan; pure arithmetic, runs without a GPU) for n rows and p columns on
 * a device of num_cu CUs: out[0] = tile columns of 16, out[1] / out[2] / out[7] = super-block rows of eight / six / four tile columns
 * the shared-slab kernel deals them into (all 0: p + 2 <= 112, one wave holds the triangle; all -1: 11-12, 15-16 or 16 k (- 1) tile columns: eight-wave
 * workgroups hold whole units of the triangle, gram_wd.hip), out[3] = row chunks, out[4] = 64-row
 * steps per chunk, out[5] = the multiply time of that deal in tile units (an h1 x h2 off-diagonal super-block h1 h2, a diagonal
 * one 36 / 24 / 12), out[6] = real tiles of the lower triangle.  Also checks that the partial-sum scratch sized for "any row count up
 * to n" (the folds of xval.oem, the row tiles of a sparse x) holds the plans of smaller row counts: OEMGPU_ERR_INTERNAL if not. */
int oemgpu_selftest_gram_plan(int64_t n, int32_t p, int32_t num_cu, int64_t *out /* 8 */);

/* The kernel form the moment pass takes for an n x p column-major x with leading dimension ld (pure host arithmetic, no device; the
 * launch calls the same function): out[0] = OEMGPU_GRAM_FORM_*, out[1] = strip sub-blocks of the ring kernel's last tile row (0, 1, 2;
 * 0 for every other form).  aligned: x and y 16-byte aligned and ld even.  The scalar-base forms (RING_SADDR, SB, WD*) address a
 * fragment as a 64-bit scalar base plus a 32-bit byte offset per lane: RING_SADDR needs p ld 8 + 65536 < 2^32 and whole-column
 * fragments (p >= 16 (tile columns - 1)), SB / WD* need 16 ld 8 < 2^32; all three need aligned input and n >= 64.  Behind those guards
 * the pass takes 64-bit addresses: RING_LANE, TRI (the triangle fits one wave) or BLK. */
enum {
    OEMGPU_GRAM_FORM_TRI = 0,        /* gram_tri_kernel: p + 2 <= 112, unaligned or n < 64 or fewer than 4 tile columns */
    OEMGPU_GRAM_FORM_RING_SADDR = 1, /* gram_ring_kernel, scalar base + 32-bit lane offsets */
    OEMGPU_GRAM_FORM_RING_LANE = 2,  /* gram_ring_kernel, a 64-bit pointer per lane */
    OEMGPU_GRAM_FORM_SB = 3,         /* gram_sb.hip: shared-slab super-blocks */
    OEMGPU_GRAM_FORM_WD3 = 4,        /* gram_wd.hip: 11-12 tile columns, one read of x, groups of three */
    OEMGPU_GRAM_FORM_WD4 = 5,        /* gram_wd.hip: 15-16 tile columns, groups of four */
    OEMGPU_GRAM_FORM_WD_UNITS = 6,   /* gram_wd.hip: 16 k (- 1) tile columns, k >= 2 units */
    OEMGPU_GRAM_FORM_BLK = 7         /* gram_blk_kernel: more than 7 tile columns, unaligned, n < 64 or 16 ld 8 >= 2^32 */
};
int oemgpu_selftest_gram_form(int64_t n, int64_t ld, int32_t p, int32_t aligned, int32_t num_cu, int64_t *out /* 2 */);

/* ---------------------------------------------------------------------------------------------------------- binomial (logistic.hip)
 * `.Call("oem_fit_logistic_dense", ...)` (ref src/oem_logistic_dense.cpp:30-313, src/oem_logistic_dense.h:397-1094): IRLS over the OEM
 * iteration, dense x, n > p + intercept.  opts as for oemgpu_fit_dense (accelerate is ignored: the reference has no Nesterov step here);
 * with an intercept, groups / ngroupvars cover q = p + 1 coordinates with the intercept's group first (R/oem.R:296-338 prepends group 0)
 * and penalty_factor stays p long (the library prepends the intercept's 0, cpp :119-141).  The scalars the opts struct lacks are
 * parameters: hessian_full (0: "upper.bound" -- X'WX, d and A from the first step of a penalty only; 1: "full" -- every step),
 * irls_maxit >= 1 and irls_tol >= 0.  Outputs as oemgpu_fit_dense: beta[npen][nlambda][p + 1] (row 0 the intercept, 0 without one;
 * "ols" fills slot 0 only), lambda_out[npen][nlambda], niter = IRLS steps + 1 at the cap (ref h :1035), loss = the logistic loss of
 * the last prob computed (1e99 unless compute_loss), d = the last d = 1.0005 lambda_max(XX).
 * Checked before any device is looked for: OEMGPU_ERR_ARG for bad arguments (hessian_full not 0 / 1, irls_maxit <= 0, ...),
 * OEMGPU_ERR_UNSUPPORTED for p + intercept >= n (the reference's XWXt branch iterates on the raw labels, ref h :524-566) and p > 8191.
 * opts->interrupt is polled between IRLS steps (OEMGPU_ERR_INTERRUPTED). */
int oemgpu_fit_logistic_dense(const double *x, int64_t n, int32_t p, const double *y, int32_t standardize, int32_t intercept,
                              int32_t hessian_full, int32_t irls_maxit, double irls_tol, const oemgpu_opts *opts,
                              double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);
/* the same with x (column-major, leading dimension ld >= n) and y on the context's device */
int oemgpu_fit_logistic_dense_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                                  int32_t standardize, int32_t intercept, int32_t hessian_full, int32_t irls_maxit, double irls_tol,
                                  const oemgpu_opts *opts, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);
/* cv.oem's fold fit on the resident x: the fit of oemgpu_fit_logistic_dense_dev on the rows with foldid_dev[row] != leave_out, i.e. what
 * `.Call("oem_fit_logistic_dense", ...)` computes on x[keep, ], y[keep] -- X and y are neither gathered nor copied, the passes over the
 * rows leave the fold's rows out, and the number of kept rows stands where n enters the arithmetic (the column scales' n - 1, the / n
 * of XX, XY and the gradient; the W floor tests the IRLS index among the kept rows).  foldid_dev: n int32 on the device, values
 * 1 .. nfolds.  leave_out = 0 leaves nothing out and returns the bits of oemgpu_fit_logistic_dense_dev.  After leave_out the
 * arguments and outputs are those of oemgpu_fit_logistic_dense_dev.  Checked before any device is looked for: OEMGPU_ERR_ARG for a
 * NULL foldid_dev, nfolds < 3 and leave_out outside [0, nfolds], then the checks of oemgpu_fit_logistic_dense.  From the device:
 * OEMGPU_ERR_ARG for a fold id outside [1, nfolds], OEMGPU_ERR_UNSUPPORTED for p + intercept >= the kept rows. */
int oemgpu_fit_logistic_dense_fold_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                                       const int32_t *foldid_dev, int32_t nfolds, int32_t leave_out, int32_t standardize, int32_t intercept,
                                       int32_t hessian_full, int32_t irls_maxit, double irls_tol, const oemgpu_opts *opts,
                                       double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);
/* cv.oemfit_binomial's error terms on the resident x (logistic_cv.hip; ref R/cv_oem.R:315-327).  coef (host): nfolds x ncol x (p + 1),
 * for fold f (1-based f - 1) and column c the intercept and the p coefficients that score the rows of fold f.  Every row with
 * foldid 1 .. nfolds is scored with the columns of its own fold: prob = 1 / (1 + exp(-(beta_0 + x . beta))), y2 = (y == y_hi), and
 * the terms deviance -2 [y2 log pm + (1 - y2) log(1 - pm)] with pm = prob clamped to [1e-5, 1 - 1e-5], class (y2 ? prob <= 0.5 :
 * prob > 0.5), mse 2 (y2 - prob)^2 and mae 2 |y2 - prob|.  sums (host): nfolds x ncol x 8 = [sum, sum of squares] of deviance, class,
 * mse, mae over the fold's rows; counts (host): the fold sizes; predmat_dev (device, n x ncol column-major, or NULL): prob.  Sums are
 * taken in a fixed order: two calls give the same bits.  OEMGPU_ERR_UNSUPPORTED for p > 8191 (the fit's own limit). */
int oemgpu_logistic_cv_score_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev, double y_hi,
                                 const int32_t *foldid_dev, int32_t nfolds, const double *coef, int32_t ncol, double *sums, int64_t *counts,
                                 double *predmat_dev);
/* Host-only plan of oemgpu_logistic_cv_score_dev (pure arithmetic, runs without a GPU; the entry takes its launch shape from the same
 * function): out[0] rows per workgroup (a multiple of 64; a workgroup walks them in tiles of 64), out[1] workgroups of a launch
 * (workgroup c = rows [c out[0], min(n, (c + 1) out[0]))), out[2] 1 if a fold's coefficient table sits in LDS (8 (ncol (p + 9) + 1)
 * bytes fit the 160 KiB of a CU) and 0 if it is read through the cache, out[3] columns per launch, out[4] launches per fold, out[5]
 * dynamic LDS bytes of the largest launch.  OEMGPU_ERR_ARG on n < 1, p outside [1, 8191], ncol < 1 or num_cu < 1. */
int oemgpu_selftest_cv_score_plan(int64_t n, int32_t p, int32_t ncol, int32_t num_cu, int64_t *out /* 6 */);
/* cv.oemfit_binomial's AUC on the device (logistic_auc.hip): what R/cv_oem.R:288-307 asks of auc.mat (R/utils.R:90-125, unit weights) for
 * every fold and column, from the predmat_dev that oemgpu_logistic_cv_score_dev wrote (ncol x n doubles, column c at c n), which stays
 * where it is.  For fold f (the rows with foldid f, in row order) and column c the rows are ordered by prob ascending with tied
 * probabilities in row order -- where the reference draws runif, so this order is one of its draws -- and NaN (a row the scoring did
 * not write) behind every number, NaNs in row order: numpy's stable argsort.  With y2 = (y == y_hi): n1[f] (host, nfolds) = rows with
 * y2 = 1, n0[f] (host, nfolds) = the rest, u[f ncol + c] (host) = the sum over the rows with y2 = 1 of the rows with y2 = 0 in front of
 * it; the AUC is u / (n1 n0).  The three are exact integers: a stable least-significant-digit radix sort per (fold, column) segment,
 * one workgroup each, in LDS when the segment fits and through two workspace buffers otherwise (oemgpu_selftest_cv_auc_plan), no
 * floating-point arithmetic and no atomics outside LDS: two calls give the same integers.  predmat_dev holds probabilities: a sign
 * bit is dropped (-0.0 is 0.0).  A fold without rows is not an error (u = n1 = n0 = 0).  OEMGPU_ERR_ARG for a NULL argument, n < 1,
 * ncol < 1, nfolds < 1 (before any device is looked for) and, from the device, a fold id outside [1, nfolds]; OEMGPU_ERR_UNSUPPORTED
 * for nfolds > 4096 (a chunk's fold counters sit in LDS) and n >= 2^31. */
int oemgpu_logistic_cv_auc_dev(oemgpu_ctx *ctx, const double *predmat_dev, int64_t n, int32_t ncol, const double *y_dev, double y_hi,
                               const int32_t *foldid_dev, int32_t nfolds, int64_t *u, int64_t *n1, int64_t *n0);
/* Host-only plan of oemgpu_logistic_cv_auc_dev (pure arithmetic, runs without a GPU; the entry takes its launch shape from the same
 * function) for a call whose longest fold has longest_fold rows: out[0] keys per tile of a sorting pass, out[1] the longest segment
 * that is sorted in LDS (a longer one goes through the workspace), out[2] columns per batch, out[3] batches, out[4] workspace bytes
 * (perm, the counting sort's tables, n1, and per column of a batch its nfolds results and -- only when out[6] is 1 -- its two key
 * buffers, 16 n bytes: the whole kept under 256 MB while one column fits, so that out[2] below ncol depends on n and nfolds alone), out[5] dynamic LDS bytes of the largest launch, out[6] 1 if the longest fold
 * takes the workspace form, out[7] rows per chunk of the counting sort by fold, out[8] chunks.  OEMGPU_ERR_ARG on n < 1, nfolds
 * outside [1, 4096], ncol < 1, num_cu < 1 or longest_fold outside [0, n]. */
int oemgpu_selftest_cv_auc_plan(int64_t n, int32_t nfolds, int32_t ncol, int32_t num_cu, int64_t longest_fold, int64_t *out /* 9 */);
/* Host-only plan of the binomial fit (pure arithmetic, runs without a GPU): out[0] rows per chunk of the row pass, out[1] chunks
 * (chunk c = rows [c out[0], min(n, (c + 1) out[0]))), out[2] rows per Z block of the moment pass, out[3] Z blocks, out[4] 1 if the
 * inner solve is one persistent workgroup (q <= 1024) and 0 for launch per iteration, out[5] 1 if the row pass stages its sub-blocks
 * in LDS, out[6] device workspace bytes of a call, out[7] the bound out[6] stays within. */
int oemgpu_selftest_logistic_plan(int64_t n, int32_t p, int32_t intercept, int32_t hessian_full, int32_t num_cu, int64_t *out /* 8 */);
/* The binomial entries on a ROW-major x read where it lies (logistic_rm.hip): x_dev is n x p with row stride ldr >= p (elements),
 * dtype OEMGPU_F64 or OEMGPU_F32, aligned to its element size only; columns p .. ldr - 1 of a row, rows >= n and -- in a fold fit and
 * in the scoring -- the rows that are not asked for are never loaded.  float32 elements are widened in the register they were loaded
 * into and all arithmetic is FP64.  Every sum is taken in the order of the column-major kernels with the same chunks and Z blocks, so
 * each entry returns the bits of its column-major counterpart on the same values laid out column-major in float64:
 *   oemgpu_fit_logistic_dense_rm_dev:      oemgpu_fit_logistic_dense_dev, i.e. `.Call("oem_fit_logistic_dense", ...)` (ref
 *                                          src/oem_logistic_dense.cpp:30-313, src/oem_logistic_dense.h:397-1094);
 *   oemgpu_fit_logistic_dense_fold_rm_dev: oemgpu_fit_logistic_dense_fold_dev, the same on x[keep, ], y[keep] (ref R/cv_oem.R:129-175);
 *   oemgpu_logistic_cv_score_rm_dev:       oemgpu_logistic_cv_score_dev, cv.oemfit_binomial's error terms (ref R/cv_oem.R:224-346).
 * The other arguments, the outputs and the checks are the counterpart's, with the same error codes, refused before a device is looked
 * for; then OEMGPU_ERR_ARG for a dtype other than the two, for ldr < p and for an x_dev that is not aligned to its element. */
int oemgpu_fit_logistic_dense_rm_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                                     int32_t standardize, int32_t intercept, int32_t hessian_full, int32_t irls_maxit, double irls_tol,
                                     const oemgpu_opts *opts, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);
int oemgpu_fit_logistic_dense_fold_rm_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                                          const int32_t *foldid_dev, int32_t nfolds, int32_t leave_out, int32_t standardize, int32_t intercept,
                                          int32_t hessian_full, int32_t irls_maxit, double irls_tol, const oemgpu_opts *opts,
                                          double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);
int oemgpu_logistic_cv_score_rm_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                                    double y_hi, const int32_t *foldid_dev, int32_t nfolds, const double *coef, int32_t ncol, double *sums,
                                    int64_t *counts, double *predmat_dev);
/* Host-only plan of the row-major binomial fit (pure arithmetic, runs without a GPU).  The row pass stages a 64-row sub-block in LDS
 * in column bands: band b = columns [b out[1], min(p, (b + 1) out[1])).  out[0] bands, out[1] columns per band (a multiple of 4 unless
 * there is one band, which is then p wide and read once per step; several bands are read twice), out[2] columns of the last band,
 * out[3] LDS bytes of a workgroup (at most the 160 KiB of a CU), out[4 .. 7] = out[0 .. 3] of oemgpu_selftest_logistic_plan: the chunks
 * and Z blocks are the column-major call's.  OEMGPU_ERR_ARG on n, p, num_cu < 1, a dtype other than the two or a NULL out;
 * OEMGPU_ERR_UNSUPPORTED for p > 8191. */
int oemgpu_selftest_logistic_rm_plan(int64_t n, int32_t p, int32_t dtype, int32_t intercept, int32_t num_cu, int64_t *out /* 8 */);
/* Many binomial responses on one resident x: what m calls of oemgpu_fit_logistic_dense_dev / _rm_dev (`.Call("oem_fit_logistic_dense",
 * ...)`, ref src/oem_logistic_dense.cpp:30-313, src/oem_logistic_dense.h:397-1094) with the columns of Y return, for hessian.type
 * "upper.bound".  Y is read through its strides as oemgpu_fit_dense_multi_dev reads it: element (i, r) at y_dev[i y_rs + r y_cs],
 * row-major (y_cs == 1, y_rs >= m) or column-major (y_rs == 1, y_cs >= n), its padding never loaded.  With the upper bound the
 * reference builds X'WX at beta = 0 (h :964-965), where every W is 0.25: XX, d = 1.0005 lambda_max(XX) and A = dI - XX do not depend
 * on y.  They are built ONCE per call (one weighted Gram pass, one Lanczos); the responses then run the reference's loops in
 * lock-step, at most 64 at a time: one row pass over x per IRLS step for all of them (logistic_multi.hip: eta = X Bt and X'R as two
 * FP64 MFMA products), one inner OEM launch with a workgroup per response, one stop launch and one host read.  A response that meets
 * its IRLS stop is frozen for the rest of the lambda (nothing of it is written again; niter is its own step count); the skipped row
 * pass of the first step of a later lambda (h :861) holds for all.  Every response has its own lambda grid (from its own max |X'y|);
 * a user lambda is shared.  A response's results do not depend on the others, on its column index or on m.
 * Outputs, response-major: beta[m][npen][nl][p + 1], lambda_out / niter / loss [m][npen][nl], d[m] (m equal values).
 * Refused before a device is looked for: a NULL argument, m < 1 and Y strides that are neither layout (OEMGPU_ERR_ARG); what
 * oemgpu_fit_logistic_dense_dev / _rm_dev refuse, with their codes; hessian_full = 1 (OEMGPU_ERR_UNSUPPORTED: "a full Hessian is one
 * per response and step: fit each column with fit_logistic_dense"); p + intercept > 1024 (OEMGPU_ERR_UNSUPPORTED: beyond one
 * workgroup the inner solve is a product of all responses).  OEMGPU_ERR_INTERRUPTED when opts->interrupt (polled once per lock-step
 * IRLS step) returns non-zero. */
int oemgpu_fit_logistic_dense_multi_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev, int64_t y_rs,
                                        int64_t y_cs, int32_t m, int32_t standardize, int32_t intercept, int32_t hessian_full, int32_t irls_maxit,
                                        double irls_tol, const oemgpu_opts *opts, double *beta, double *lambda_out, int32_t *niter, double *loss,
                                        double *d);
int oemgpu_fit_logistic_dense_multi_rm_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                                           int64_t y_rs, int64_t y_cs, int32_t m, int32_t standardize, int32_t intercept, int32_t hessian_full,
                                           int32_t irls_maxit, double irls_tol, const oemgpu_opts *opts, double *beta, double *lambda_out,
                                           int32_t *niter, double *loss, double *d);
/* The fold fits of a cross-validation over many binomial responses, in the same lock-step.  Instance i < ninst is
 * response resp[i] of Y fitted on the rows with foldid_dev[row] != leave_out[i] (0: every row) -- what
 * oemgpu_fit_logistic_dense_fold_dev / _fold_rm_dev return for that column and fold, and oemgpu_fit_logistic_dense_dev / _rm_dev
 * for leave_out 0.  foldid_dev: n device words in [1, nfolds]; resp, leave_out: host arrays of ninst words, in any order, repeats
 * allowed.  Per distinct leave_out value (a group) the call builds s, X'WX at beta = 0 on the kept rows, d and A once (one Gram pass
 * and one Lanczos per group); every instance then rides the shared row pass as one column with its own row mask, has its own lambda
 * grid from its own masked X'y (a user lambda is shared) and its group's n_eff wherever n enters.  An instance's results do not depend
 * on the other instances or on the order of the list.  The columns of a row pass share the rows they load: x must be finite on
 * EVERY row, also on rows that only some instances leave out (the single fold entry never loads a left-out row).
 * Outputs, instance-major: beta[ninst][npen][nl][p + 1], lambda_out / niter / loss [ninst][npen][nl], d[ninst] (its group's),
 * nobs[ninst] (the rows of its fit).
 * Refused before any fit, nothing written: what oemgpu_fit_logistic_dense_multi_dev refuses, with its codes (a full Hessian and
 * p + intercept > 1024 included); a NULL foldid_dev, resp, leave_out or nobs, nfolds < 3 ("nfolds must be bigger than 3; nfolds=10
 * recommended"), ninst < 1, a leave_out outside [0, nfolds], a resp outside [0, m) (OEMGPU_ERR_ARG); a fold id outside [1, nfolds]
 * (OEMGPU_ERR_ARG, found on the device); p + intercept >= the rows outside a fold that an instance leaves out (OEMGPU_ERR_UNSUPPORTED,
 * naming the fold).  oemgpu_last_logistic_multi_stats: out[4] = out[5] = the number of groups. */
int oemgpu_fit_logistic_dense_multi_fold_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev, int64_t y_rs,
                                             int64_t y_cs, int32_t m, const int32_t *foldid_dev, int32_t nfolds, int32_t ninst, const int32_t *resp,
                                             const int32_t *leave_out, int32_t standardize, int32_t intercept, int32_t hessian_full, int32_t irls_maxit,
                                             double irls_tol, const oemgpu_opts *opts, double *beta, double *lambda_out, int32_t *niter, double *loss,
                                             double *d, int64_t *nobs);
int oemgpu_fit_logistic_dense_multi_fold_rm_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                                                int64_t y_rs, int64_t y_cs, int32_t m, const int32_t *foldid_dev, int32_t nfolds, int32_t ninst,
                                                const int32_t *resp, const int32_t *leave_out, int32_t standardize, int32_t intercept,
                                                int32_t hessian_full, int32_t irls_maxit, double irls_tol, const oemgpu_opts *opts, double *beta,
                                                double *lambda_out, int32_t *niter, double *loss, double *d, int64_t *nobs);
/* Host-only workspace plan of a fold call with ninst instances in ngroups groups (pure arithmetic).  out[0] rows per chunk of the row
 * pass, out[1] chunks, out[2] instances of the widest lock-step chunk (at most 64), out[3] lock-step chunks, out[4] ngroups,
 * out[5 .. 9] bytes: the panels of a row pass; the groups (s, XX, A and the row count of each: 8 ngroups (p + 2 q^2 + 1)); what the
 * call shares besides; a chunk's state without its per-lambda tables; the Hessian pass's stages; out[10] their sum.  OEMGPU_ERR_ARG
 * on an argument < 1, a layout other than 0 / 1 or a NULL out; OEMGPU_ERR_UNSUPPORTED for p + intercept > 1024. */
#define OEMGPU_LMULTI_FOLD_PLAN_LEN 11
int oemgpu_selftest_logistic_multi_fold_plan(int64_t n, int32_t p, int32_t ninst, int32_t ngroups, int32_t intercept, int32_t layout, int32_t num_cu,
                                             int64_t *out /* OEMGPU_LMULTI_FOLD_PLAN_LEN */);
/* Test infrastructure: ONE masked row pass of ncol columns.  Column t is response ycol[t] of Y (t itself when ycol is NULL, and then
 * ncol == m) on the rows with foldid_dev[row] != leave[t]; leave, ycol, live: host arrays of ncol words; btilde_dev: ncol x (p +
 * intercept); out_dev: [ncol][p + 2].  The rest as oemgpu_selftest_logistic_multi_rows_dev. */
int oemgpu_selftest_logistic_multi_rows_fold_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ld, int32_t p,
                                                 const double *y_dev, int64_t y_rs, int64_t y_cs, int32_t m, const int32_t *foldid_dev, int32_t ncol,
                                                 const int32_t *leave, const int32_t *ycol, const double *btilde_dev, int32_t intercept, int32_t mode,
                                                 const int32_t *live, double *out_dev);
/* Host-only plan of the many-response binomial fit (pure arithmetic, runs without a GPU).  layout: 0 column-major x, 1 row-major.
 * out[0] rows per chunk of the shared row pass (a multiple of 64 that depends on n and num_cu alone), out[1] chunks (chunk c = rows
 * [c out[0], min(n, (c + 1) out[0]))), out[2] responses per block (16 out[3]), out[3] response tiles per block LT, out[4] the column
 * band: the 64 out[9] columns a workgroup's accumulators cover (128, 256, 512 or 1024 by p), out[5] LDS bytes of a workgroup,
 * out[6] MCH = 64, the responses of a lock-step chunk, out[7] lock-step chunks, out[8] response blocks of the widest chunk, out[9]
 * 16-column tiles per wave, out[10 .. 13] workspace bytes: the panels of a row pass, what the call shares (s, XX, A), a chunk's state
 * without its per-lambda tables, the Hessian pass's stages (out[6] of oemgpu_selftest_logistic_plan); out[14] their sum; out[15] 1
 * if the inner solve keeps A in LDS.  OEMGPU_ERR_ARG on n, p, m, num_cu < 1, a layout other than the two or a NULL out;
 * OEMGPU_ERR_UNSUPPORTED for p + intercept > 1024. */
#define OEMGPU_LMULTI_PLAN_LEN 16
int oemgpu_selftest_logistic_multi_plan(int64_t n, int32_t p, int32_t m, int32_t intercept, int32_t layout, int32_t num_cu,
                                        int64_t *out /* OEMGPU_LMULTI_PLAN_LEN */);
/* Test infrastructure: ONE shared row pass.  x_dev: column-major float64 (dtype < 0, ld the column stride) or row-major (dtype
 * OEMGPU_F64 / OEMGPU_F32, ld the row stride); btilde_dev (device, mode 1): m x (p + intercept), response r's entries of beta o s
 * contiguous with the intercept's first; mode 0: r = y (X'Y), mode 1: the IRLS quantities; live (host, m words, or NULL: all live);
 * out_dev (device): [m][p + 2], response r's [sum r, X'r, sum of the loss terms] -- written for the live responses only. */
int oemgpu_selftest_logistic_multi_rows_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                                            int64_t y_rs, int64_t y_cs, int32_t m, const double *btilde_dev, int32_t intercept, int32_t mode,
                                            const int32_t *live, double *out_dev);
/* Of this thread's last many-response binomial call (or row-pass selftest): out[0] lock-step IRLS steps, out[1] row passes (the X'Y
 * passes not counted), out[2] response blocks of those passes that returned without reading x (all their responses frozen), out[3]
 * inner OEM iterations over all responses, out[4] Gram builds, out[5] Lanczos runs, out[6 .. 8] ms of the row passes / the Gram build
 * / the inner launches when the context is timing (else 0), out[9] wall ms. */
int oemgpu_last_logistic_multi_stats(double *out /* 10 */);
/* `.Call("oem_fit_logistic_sparse", ...)` (ref src/oem_logistic_sparse.cpp:30-313, src/oem_logistic_sparse.h): the binomial fit of a
 * compressed-sparse-column x (a dgCMatrix: colptr[p + 1] with colptr[0] = 0, non-decreasing; rowidx[nnz] in [0, n), strictly increasing
 * inside a column; values[nnz]; explicit zeros allowed).  opts, irls_maxit, irls_tol and the outputs as oemgpu_fit_logistic_dense.  The
 * reference's single-thread branch (its default ncores): the Hessian X'WX at every IRLS step but the skipped first of a later lambda
 * (hessian.type is never read), the intercept's coordinate scaled by intval = sqrt(mean diag(S X'WX S) / sum W / n) of the first
 * Hessian build, and get_beta's in-place beta_0 *= intval after every lambda (the next lambda starts from it).
 * Checked before any device is looked for: the checks of oemgpu_fit_logistic_dense; OEMGPU_ERR_UNSUPPORTED for p + intercept >= n,
 * p > 8191 and an intercept without standardize (the reference reads column scales it never computed, h :724, :880); OEMGPU_ERR_ARG
 * for malformed compressed-column arrays.  opts->interrupt is polled between IRLS steps (OEMGPU_ERR_INTERRUPTED). */
int oemgpu_fit_logistic_sparse(int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values, const double *y,
                               int32_t standardize, int32_t intercept, int32_t irls_maxit, double irls_tol, const oemgpu_opts *opts,
                               double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);
/* Host-only plan of the sparse binomial fit (pure arithmetic, runs without a GPU): out[0] 1 if X'WX takes the compressed-column kernel
 * (it fits in LDS, nnz <= 2 % of n p, n < 2^31: the rule of oemgpu_fit_sparse, or the route a call would be forced to by the
 * library's OEM_SPARSE_GRAM test switch) and 0 for zero-filled row tiles through the MFMA moment
 * pass, out[1] 1 if the inner solve is one persistent workgroup (q <= 1024) and 0 for launch per iteration, out[2] device workspace
 * bytes of the fit's data stages, out[3] the bound out[2] stays within, out[4] rows per tile (0 on the compressed-column route),
 * out[5] workgroups of the row pass, out[6] rows per row-pass workgroup, out[7] 8192-row chunks of the compressed-column kernels. */
int oemgpu_selftest_logistic_sparse_plan(int64_t n, int32_t p, int64_t nnz, int32_t intercept, int32_t num_cu, int64_t *out /* 8 */);
/* A sparse x resident on the context's device, for cv.oem on a dgCMatrix (ref R/cv_oem.R:105-175: one oem() on x, then K on
 * x[!which, , drop = FALSE]; R/oem.R:603-624 sends each to oem_fit_logistic_sparse).  create checks the compressed-column arrays as
 * oemgpu_fit_logistic_sparse does (OEMGPU_ERR_ARG with the same sentences, before any device is looked for), uploads them and
 * builds, once, the per-column chunk pointers and the compressed-row copy that a fit otherwise builds per call.  The handle is an
 * allocation of its own (24 B a non-zero, 8 (n + 1) B of row pointers, the chunk pointers), not part of the context's workspace; it
 * may be used with any context of the same device, by one call at a time.  destroy frees it and accepts NULL. */
typedef struct oemgpu_sparse_x oemgpu_sparse_x;
int oemgpu_sparse_x_create(oemgpu_ctx *ctx, int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values,
                           oemgpu_sparse_x **out);
void oemgpu_sparse_x_destroy(oemgpu_sparse_x *x);
/* the bytes of device memory the handle holds (its one allocation); 0 for NULL */
int64_t oemgpu_sparse_x_bytes(const oemgpu_sparse_x *x);
/* The same handle from arrays that are ALREADY on the context's device (a torch sparse_csr / sparse_csc / coalesced sparse_coo tensor's
 * components): compressed columns (layout OEMGPU_SPARSE_CSC: ptr_dev p + 1 pointers, idx_dev row indices) or compressed rows
 * (OEMGPU_SPARSE_CSR: n + 1 pointers, column indices).  Pointers and indices are OEMGPU_I32 or OEMGPU_I64 each, values OEMGPU_F64 or
 * OEMGPU_F32 (widened in the register, exactly); every array need only be aligned to its element.  The handle owns copies of
 * everything: the caller's arrays may be freed when the call returns.  The result is the handle oemgpu_sparse_x_create makes of the
 * same matrix, array for array (oemgpu_sparse_x_export): the other orientation comes from a stable least-significant-digit counting
 * sort of the non-zeros by their index (digits of <= 11 bits: 1 pass up to 2048 target lines, 2 up to 2^22, 3 beyond; integer LDS
 * atomics only, values moved as bit patterns, no floating-point arithmetic: two calls give the same arrays), its pointers from one
 * lower bound per line.  Nothing is copied to the host but a few flag words.
 * OEMGPU_ERR_ARG before any device work: a NULL ctx, ptr_dev or out, a layout or dtype code that is none of the above, n < 1, p < 1,
 * nnz < 0, NULL idx_dev or val_dev with nnz > 0; OEMGPU_ERR_UNSUPPORTED for n >= 2^31 and for nnz >= 2^31.  From the device, with
 * csc_check's sentences (their row-wise counterparts for compressed rows) and nothing of the input used: ptr[0] != 0, ptr[last] != nnz,
 * a decreasing pointer, an index outside its range and a line whose indices are not strictly increasing (duplicates, unsorted
 * lines) -- the message names the first offending entry's line (an integer minimum over the entries).  OEMGPU_ERR_ARG each. */
#define OEMGPU_SPARSE_CSC 0
#define OEMGPU_SPARSE_CSR 1
#define OEMGPU_I32 0
#define OEMGPU_I64 1
int oemgpu_sparse_x_create_dev(oemgpu_ctx *ctx, int64_t n, int32_t p, int32_t layout, const void *ptr_dev, int32_t ptr_dtype,
                               const void *idx_dev, int32_t idx_dtype, const void *val_dev, int32_t val_dtype, int64_t nnz,
                               oemgpu_sparse_x **out);
/* Host-only plan of oemgpu_sparse_x_create_dev (pure arithmetic, runs without a GPU): out[0] passes of the sort, [1] bits per digit,
 * [2] workgroups of a pass, [3] bytes of the context's workspace the call takes (the line numbers and the sorted indices, 4 B a
 * non-zero each; one 16 B-a-non-zero buffer from two passes on, a second from three; the digit table 4 B x 2^bits x workgroups; all
 * in 256-byte granules), [4] bytes of the handle, [5] non-zeros per workgroup (a multiple of 2048), [6] bits of the largest index,
 * [7] target lines (n for compressed columns, p for compressed rows).  OEMGPU_ERR_ARG for n, p or num_cu < 1, nnz < 0, an unknown
 * layout or a NULL out; OEMGPU_ERR_UNSUPPORTED for n >= 2^31 or nnz >= 2^31. */
int oemgpu_selftest_sparse_build_plan(int64_t n, int32_t p, int64_t nnz, int32_t layout, int32_t num_cu, int64_t *out /* 8 */);
/* The handle's arrays copied to host buffers (any pointer may be NULL: that array is skipped): colptr p + 1, rowidx and val nnz (every
 * column's entries by ascending row), rowptr n + 1, ccol and cval nnz (every row's entries by ascending column), cptr
 * (ceil(n / 8192) + 1) x p.  dims: out[0] n, [1] p, [2] nnz, [3] the longest column. */
int oemgpu_sparse_x_export(const oemgpu_sparse_x *x, int64_t *colptr, int32_t *rowidx, double *val, int64_t *rowptr, int32_t *ccol,
                           double *cval, int32_t *cptr);
int oemgpu_sparse_x_dims(const oemgpu_sparse_x *x, int64_t *out /* 4 */);
/* HIP-event times (ms) of this thread's last oemgpu_sparse_x_create_dev with nnz > 0: ms[0] check and widen (with its read-back),
 * ms[1] the sort passes, ms[2] the other orientation's pointers, the chunk pointers and the longest column. */
int oemgpu_last_sparse_build_timings(double *ms /* 3 */);
/* oem() on a resident sparse x: what oemgpu_fit_sparse computes, with y_dev (n doubles) on the device and nothing uploaded.  n > p:
 * the moment buffer from the handle's compressed columns by oemgpu_fit_sparse's route (the same kernels on the same values: without an
 * intercept the results carry the bits of oemgpu_fit_sparse; with one, intval is taken from the moment buffer's diagonal, as
 * oemgpu_cv_sparse_fold_fits_res takes it, and agrees to rounding), then the same solve.  n <= p: oemgpu_fit_sparse_wide_res, and
 * OEMGPU_ERR_UNSUPPORTED with an intercept (oemgpu_fit_sparse's sentence).  OEMGPU_ERR_ARG for a NULL argument, bad options and a
 * handle on another device than the context's. */
int oemgpu_fit_sparse_res(oemgpu_ctx *ctx, const oemgpu_sparse_x *x, const double *y_dev, int32_t standardize, int32_t intercept,
                          const oemgpu_opts *opts, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);
/* xval.oem on a resident sparse x: oemgpu_xval_sparse with its upload phase replaced by the handle's arrays and the caller's y_dev (n
 * doubles) and foldid_dev (n int32, 1 .. nfolds) -- every later phase, output and refusal unchanged (the same kernels on the same
 * values: the same bits); also OEMGPU_ERR_ARG for a handle on another device than the context's. */
int oemgpu_xval_sparse_res(oemgpu_ctx *ctx, const oemgpu_sparse_x *x, const double *y_dev, const int32_t *foldid_dev, int32_t nfolds,
                           int32_t standardize, int32_t intercept, int32_t type_measure, const oemgpu_opts *opts, double *beta,
                           double *lambda_out, int32_t *niter, double *loss, double *d, double *cvm, double *cvsd);
/* cv.oem's fold fit on the resident sparse x (ref R/cv_oem.R:129-175): what `.Call("oem_fit_logistic_sparse", ...)` computes on
 * x[keep, ], y[keep] with keep = foldid_dev != leave_out, every particular of oemgpu_fit_logistic_sparse included.  Nothing is sliced,
 * uploaded or converted: the passes leave the fold's rows out and the number of kept rows stands where n enters the arithmetic (the
 * column scales' n - 1, intval, the / n of XX, XY and the gradient; the W floor tests the IRLS index among the kept rows).  y_dev: n
 * doubles and foldid_dev: n int32 with values 1 .. nfolds, on the device.  leave_out = 0 (foldid_dev may then be NULL) leaves nothing
 * out and returns the bits of oemgpu_fit_logistic_sparse.  A left-out row is excluded exactly -- its y is never read, its stored
 * values only meet a weight of 0 -- as long as those stored values are finite; NaN / Inf in a left-out row are not supported (they
 * would poison the full fit of the same cv.oem anyway).  No floating-point atomics: two calls give the same bits.
 * Checked before any device is looked for: OEMGPU_ERR_ARG for a NULL argument, nfolds < 3, leave_out outside [0, nfolds] and a NULL
 * foldid_dev with leave_out > 0, then the checks of oemgpu_fit_logistic_sparse.  From the device: OEMGPU_ERR_ARG for a fold id outside
 * [1, nfolds], OEMGPU_ERR_UNSUPPORTED (naming the fold) for p + intercept >= the kept rows. */
int oemgpu_fit_logistic_sparse_fold_res(oemgpu_ctx *ctx, const oemgpu_sparse_x *x, const double *y_dev, const int32_t *foldid_dev, int32_t nfolds,
                                        int32_t leave_out, int32_t standardize, int32_t intercept, int32_t irls_maxit, double irls_tol,
                                        const oemgpu_opts *opts, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);
/* oem() on the resident sparse x with n <= p and no intercept (ref src/oem_sparse.h:607-612, 638-647, 932-941; src/oem_big.h:537-541,
 * 568-584, 743-764, 880-897): the data as they are (no centring, no scaling of y), u = X'(y - X beta)/n + d beta with
 * d = 1.005 lambda_max(X X'/n); with standardize only lambda_zero (max |x_j'y| colsq_inv_j / n) and the returned coefficients
 * (beta colsq_inv) carry the column scales, colsq = sum x^2 / (n - 1) with a zero made 1; compute_loss from the residual of the
 * returned coefficients (1e99 where niter is 0).  Both products of an iteration run over the handle's non-zeros -- the compressed rows
 * for X beta, the compressed columns for X't -- a few rows or columns to a wave, a long one to a workgroup, every sum in one fixed
 * order (no floating-point atomics: two calls give the same bits); nothing of n p entries is allocated.  All 14 penalties, any group
 * layout, several penalties in one call; opts.interrupt is polled between batches of iterations.  y_dev: n doubles on the device.
 * Outputs as oemgpu_fit_sparse (row 0 of every coefficient column is the absent intercept, 0).  Checked before any device work:
 * OEMGPU_ERR_ARG for a NULL argument, a handle on another device than the context's and n < 2; OEMGPU_ERR_UNSUPPORTED for n > p
 * (oemgpu_fit_sparse serves that); then the checks of the options.  n is limited by the int32 row indices alone.
 * oemgpu_last_path_engine reports OEMGPU_ENGINE_SPARSE_WIDE. */
int oemgpu_fit_sparse_wide_res(oemgpu_ctx *ctx, const oemgpu_sparse_x *x, const double *y_dev, int32_t standardize, const oemgpu_opts *opts,
                               double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);
/* Host-only plan of oemgpu_fit_sparse_wide_res and of oemgpu_fit_sparse's choice of it (pure arithmetic, runs without a GPU) for n rows,
 * p columns, nnz non-zeros, a longest row / column of that many stored entries, on a device of num_cu CUs: out[0] 1 if
 * oemgpu_fit_sparse sends an n <= p call this way (nnz <= 2 % of n p and p > 1024; OEM_SPARSE_GRAM=wide / nowide forces / forbids it; 0 for
 * n > p), [1] rows per wave of the row pass (64 / lanes per row), [2] columns per wave of the column pass, [3] 1 if the long-row form
 * (a workgroup per row of more than 32 x lanes entries) is used, [4] the same for columns, [5] workgroups of the row pass,
 * [6] of the column pass (short forms), [7] bytes of the engine's own device workspace (four n-vectors, the Lanczos table, the lists
 * of long rows and columns).  OEMGPU_ERR_ARG for non-positive n, p or num_cu, a negative count or a NULL out. */
int oemgpu_selftest_sparse_wide_plan(int64_t n, int32_t p, int64_t nnz, int64_t longest_row, int64_t longest_col, int32_t num_cu,
                                     int64_t *out /* 8 */);
/* cv.oem's fold fit on the resident sparse x with n <= p and no intercept (ref R/cv_oem.R:155-175 calls oem() on x[!which, ], which
 * reaches src/oem_sparse.h:607-612, 638-647, 932-941): what oemgpu_fit_sparse_wide_res computes on x[keep, ], y[keep] with
 * keep = foldid_dev != leave_out.  Nothing is sliced, gathered or uploaded: every row pass (X beta, the second half of the eigen
 * product, the loss) skips a left-out row -- it is not read and its output is an exact 0.0 -- the once-per-fit pass over the columns
 * (x_j'y, sum x_j^2, sum y^2) excludes left-out entries by a select, and the kept-row count n_k stands wherever n enters: X'y / n_k,
 * colsq = sum over the kept rows of x^2 / (n_k - 1) with a column emptied by the fold -> 1, g = X't / n_k,
 * d = 1.005 lambda_max(X_k X_k' / n_k) by Lanczos from a start vector that is zero in the left-out rows (the Krylov space is the kept
 * rows'; n_k in the step cap), the lambda grid from the masked X'y.  The column pass of an iteration is not masked: its input is
 * exactly zero in the left-out rows.  As for oemgpu_fit_logistic_sparse_fold_res, the stored values of a left-out row must therefore
 * be finite (a NaN or Inf there would reach the sums through x * 0); y of a left-out row is never read and may be anything.
 * y_dev: n doubles, foldid_dev: n int32 with values 1..nfolds, on the handle's device; *kept <- n_k.  leave_out = 0 (foldid_dev may
 * then be NULL) leaves nothing out and returns the bits of oemgpu_fit_sparse_wide_res, which is a call of this entry; so does a
 * leave_out that no row carries.  No floating-point atomics, one summation order per line: two calls give the same bits.  The lane
 * that adds an entry follows the entry's position in the STORED line, left-out entries included, so a fold fit matches the fit of
 * the sliced matrix to rounding (tolerance), not bit for bit.
 * Checked before a device is looked for: OEMGPU_ERR_ARG for a NULL argument, nfolds outside 3..512, leave_out outside [0, nfolds], a
 * NULL foldid_dev with leave_out > 0, a handle on another device and n < 2; OEMGPU_ERR_UNSUPPORTED for n > p (oemgpu_fit_sparse serves
 * it); then the checks of the options.  From the device: OEMGPU_ERR_ARG for a fold id outside 1..nfolds and for n_k < 2 (the fold is
 * named). */
int oemgpu_fit_sparse_wide_fold_res(oemgpu_ctx *ctx, const oemgpu_sparse_x *x, const double *y_dev, const int32_t *foldid_dev, int32_t nfolds,
                                    int32_t leave_out, int32_t standardize, const oemgpu_opts *opts, double *beta, double *lambda_out,
                                    int32_t *niter, double *loss, double *d, int64_t *kept);
/* Test infrastructure: ONE pass of the engine of oemgpu_fit_sparse_wide_fold_res, after that entry's own setup (the same internal
 * function: the engine's workspace, the lists of the long rows and columns, the check of the plan against them, the mask only when
 * leave_out > 0 and the fold has rows, the kept rows n_k for n), with the lanes per row and per column forced: row_lanes / col_lanes
 * are 0 -- what oemgpu_selftest_sparse_wide_plan gives for the context's CUs, as in the fit -- or one of 1, 2, 4, 8, 16, 32, 64, and
 * the long form then takes the lines of more than 32 x THAT many entries.  Every pointer ending in _dev is on the handle's device.
 *   OEMGPU_SPW_PASS_ROWS   out_dev[n] <- scale * sum over row i of x_ij in_dev[j] (in_dev: p doubles); masked, a left-out row: +0.0
 *   OEMGPU_SPW_PASS_COLS   out_dev[p] <- scale * sum over column j of x_ij in_dev[i] (in_dev: n doubles); never masked
 *   OEMGPU_SPW_PASS_STATS  in_dev = y: out_dev[p] <- x_j'y / n_k, out2_dev[p] <- that times the column's scale, stats_dev[4 + 2 p + 2]
 *                          <- (0, 1, sum y^2, n_k), p zeros, the p column scales 1 / sqrt(sum x_j^2 / (n_k - 1)) (1 for a zero column
 *                          and without standardize), the two shift flags 0 -- all sums over the kept rows
 *   OEMGPU_SPW_PASS_LOSS   in_dev = y: out_dev[ncoef] <- sum over the kept rows of (y - X b_k)^2 for the ncoef coefficient tables
 *                          coef_dev[ncoef][p + 1] (slot 0 of a table, the intercept, is not read)
 * scale is read by the first two passes, standardize by the third, coef_dev and ncoef by the fourth; out2_dev and stats_dev may be NULL
 * except in the third.  info: [0] the lanes per row in force, [1] per column, [2] the number of long rows, [3] of long columns,
 * [4] the longest row, [5] the longest column (stored entries), [6] n_k, [7] 1 if the pass was masked.  long_rows (n int32) /
 * long_cols (p int32): NULL, or host arrays whose first info[2] / info[3] slots <- the long lines, in no particular order.
 * The call returns after the pass has finished.  Checked before any device work: OEMGPU_ERR_ARG for a NULL argument, a pass or lanes
 * outside the values above, and what oemgpu_fit_sparse_wide_fold_res refuses for nfolds, leave_out, a NULL foldid_dev, a handle on
 * another device and n < 2; OEMGPU_ERR_UNSUPPORTED for n > p.  From the device: a fold id outside 1..nfolds and n_k < 2. */
enum { OEMGPU_SPW_PASS_ROWS = 0, OEMGPU_SPW_PASS_COLS = 1, OEMGPU_SPW_PASS_STATS = 2, OEMGPU_SPW_PASS_LOSS = 3 };
int oemgpu_selftest_sparse_wide_pass(oemgpu_ctx *ctx, const oemgpu_sparse_x *x, int32_t pass, int32_t row_lanes, int32_t col_lanes,
                                     const int32_t *foldid_dev, int32_t nfolds, int32_t leave_out, int32_t standardize, double scale,
                                     const double *in_dev, const double *coef_dev, int32_t ncoef, double *out_dev, double *out2_dev,
                                     double *stats_dev, int64_t *info /* 8 */, int32_t *long_rows, int32_t *long_cols);
/* cv.oem's scoring of the held-out rows on the resident sparse x (ref R/cv_oem.R:376-391, 392-423; R/utils.R:128-144), the companion
 * of the fold fits above: the outputs of oemgpu_cv_sparse_score_res -- triples[nfolds][npen][nl][3] <- (count, mean, M2) of fold k's
 * errors (type_measure 0 mse, 1 mae) over its own rows under ITS coefficients coef[k] (host, [nfolds][npen][nl][p + 1], slot 0 the
 * intercept), (0, NaN, NaN) in columns >= ncol[pen] and for a fold without rows; predmat_dev: NULL, or [npen][nl][n] on the device <-
 * eta in the caller's row order, NaN in columns >= ncol[pen] -- without a fold-ordered layout: the handle's compressed rows are walked
 * where they lie, fold k's rows come from foldid_dev, and ONE fold's transposed tables are on the device at a time.  The context's
 * fold buffer and the layout another cv call left there are neither read nor voided.  Per-wave partials merged in wave order, no
 * atomics: two calls give the same bits.  OEMGPU_ERR_ARG before any device work for a NULL argument, npen or nl < 1, nfolds outside
 * 3..512, a type_measure other than 0 / 1, an ncol outside 0..nl, a handle on another device; from the device for a fold id outside
 * 1..nfolds. */
int oemgpu_cv_sparse_wide_score_res(oemgpu_ctx *ctx, const oemgpu_sparse_x *x, const double *y_dev, const int32_t *foldid_dev, int32_t nfolds,
                                    const double *coef, int32_t npen, int32_t nl, const int32_t *ncol, int32_t type_measure, double *triples,
                                    double *predmat_dev /* or NULL */);
/* Host-only plan of the entry above (pure arithmetic, runs without a GPU; the entry takes its launch from the same function; it
 * replaces nothing of the reference, whose cv.oem predicts in R): out[0] waves per fold (the stride over a fold's held-out rows),
 * [1] workgroups per fold (four waves each; x npen x out[2]) -- about four per CU over (penalty, lambda block), no more waves than a
 * fold of ceil(n / nfolds) rows has rows, at most 1024 workgroups, never fewer than one --, [2] blocks of 64 lambdas, [3] bytes of one
 * staged table (p + 1) out[5] 8 (npen of them per fold), [4] bytes of the wave partials = nfolds out[0] npen out[5] 32 (kept under
 * 64 MB by lowering out[1]), [5] nl rounded up to 16, [6] workspace bytes of the call.  OEMGPU_ERR_ARG on bad arguments and nfolds
 * outside 3..512. */
int oemgpu_selftest_cv_sparse_wide_score_plan(int64_t n, int32_t p, int32_t nfolds, int32_t npen, int32_t nl, int32_t num_cu,
                                              int64_t *out /* 7 */);
/* oemgpu_logistic_cv_score_dev on the resident sparse x (ref R/cv_oem.R:224-346): the same arguments with the handle in place of
 * x_dev, n, ld, p, the same outputs.  Every row is read from the compressed-row copy, its stored entries in column order; for finite
 * tables the sums, counts and predmat are the bits of oemgpu_logistic_cv_score_dev on the same matrix written out densely.  The launch
 * plan is oemgpu_selftest_cv_score_plan's.  OEMGPU_ERR_UNSUPPORTED for p > 8191. */
int oemgpu_logistic_cv_score_sparse_res(oemgpu_ctx *ctx, const oemgpu_sparse_x *x, const double *y_dev, double y_hi, const int32_t *foldid_dev,
                                        int32_t nfolds, const double *coef, int32_t ncol, double *sums, int64_t *counts, double *predmat_dev);
/* oemgpu_selftest_logistic_sparse_plan for a fit on a resident x: the same eight numbers, out[2] (and the bound out[3] it stays
 * within) counting the fit's own pieces only -- W, r, the row partials, X'W, the device words, the moments, the Gram scratch.  The
 * compressed columns, the row copy, the chunk pointers (the handle's) and y (the caller's) are not in it. */
int oemgpu_selftest_logistic_sparse_res_plan(int64_t n, int32_t p, int64_t nnz, int32_t intercept, int32_t num_cu, int64_t *out /* 8 */);
/* cv.oem(family = "gaussian") on the resident sparse x (ref R/cv_oem.R:105, 129-175, 349-423; R/utils.R:64-144; a dgCMatrix reaches
 * oem_fit_sparse, R/oem.R:532-556, src/oem_sparse.{h,cpp}), in two phases like oemgpu_cv_fold_fits_dev / oemgpu_cv_score_dev above; the
 * caller interpolates between the two (lambda.interp).
 *
 * 1. oemgpu_cv_sparse_fold_fits_res replaces cv.oem's K + 1 calls of oem(): slot 0 of every output is the fit of all rows, slot ff what
 *    oemgpu_fit_sparse computes on the rows whose id is not ff -- oemSparse's semantics: no centring, column scales sum x_j^2 / (n - 1)
 *    with 0 -> 1 for a column that is empty among the kept rows, intval = sqrt(mean diag / n) on the intercept's coordinate, get_beta's
 *    in-place intercept scale (ref src/oem_sparse.h:493-508, 577-593, 897-900), every fit on its own lambda grid unless opts carries the
 *    user's -- with the kept-row count wherever n enters.  Nothing is sliced or uploaded: the handle's columns are rewritten in fold
 *    order on the device (fold segments on multiples of 8192 rows), the K fold moment buffers about 0 come from ONE pass over the
 *    non-zeros (compressed columns or zero-filled row tiles: the rule of oemgpu_fit_sparse, OEM_SPARSE_GRAM / OEM_SPARSE_TILE_ROWS
 *    honoured), a fold-ordered compressed-row copy is left for phase 2, and fit ff is solved from the sum of the other folds' buffers
 *    in fold order (slot 0: of all of them).  y_dev: n doubles, foldid_dev: n int32 with values 1..nfolds, on the handle's device.
 *    Host outputs: beta[nfolds + 1][npen][nl][p + 1], lambda_out / niter / loss [nfolds + 1][npen][nl], d[nfolds + 1], fold_n[nfolds].
 *    opts as for oemgpu_fit_sparse: with an intercept, groups / ngroupvars cover p + 1 coordinates with the intercept's group first.
 *    An id in 1..nfolds that never occurs is allowed: that fold's fit is the fit of all rows.
 *    Refused before a device is looked for: NULL pointers, the options (OEMGPU_ERR_ARG), nfolds outside 2..512 (OEMGPU_ERR_ARG),
 *    n + 8192 nfolds >= 2^31 and n - ceil(n / nfolds) <= p (OEMGPU_ERR_UNSUPPORTED).  From the device: an id outside 1..nfolds
 *    (OEMGPU_ERR_ARG), and n - n_k <= p for some fold k, named in the message (OEMGPU_ERR_UNSUPPORTED: that fit is the wide engine's).
 *    oemgpu_last_xval_sparse_timings then holds this call's phases: [1] fold order [2] fold moments [3] compressed rows [4] the fits.
 *
 * 2. oemgpu_cv_sparse_score_res: the arguments, outputs and argument checks of oemgpu_cv_score_dev, over the fold-ordered compressed
 *    rows phase 1 left on the context: eta = b_0 + sum of x_ij b_j over the row's stored entries in column order;
 *    triples[nfolds][npen][nl][3] <- (count, mean, M2) of every fold's errors, merged from per-fold wave partials in a fixed order (no
 *    atomics: two calls give the same bits), (0, NaN, NaN) in columns >= ncol[pen] and for empty folds; predmat_dev: NULL, or
 *    [npen][nl][n] on the device <- eta in the CALLER'S row order, NaN in columns >= ncol[pen].  It needs the layout of a call of
 *    oemgpu_cv_sparse_fold_fits_res on the same context with the same (n, p, nfolds, npen, nl); any call that lays the context's fold
 *    buffer out anew in between (xval.oem, the dense cv entries, a binomial fit) voids it, and a dense layout never passes for a
 *    sparse one nor a sparse one for a dense one: OEMGPU_ERR_ARG, never another call's rows scored. */
int oemgpu_cv_sparse_fold_fits_res(oemgpu_ctx *ctx, const oemgpu_sparse_x *x, const double *y_dev, const int32_t *foldid_dev, int32_t nfolds,
                                   int32_t standardize, int32_t intercept, const oemgpu_opts *opts,
                                   double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, int64_t *fold_n);
int oemgpu_cv_sparse_score_res(oemgpu_ctx *ctx, int64_t n, int32_t p, int32_t nfolds, const double *coef, int32_t npen, int32_t nl,
                               const int32_t *ncol, int32_t type_measure, double *triples, double *predmat_dev /* or NULL */);
/* Test infrastructure (tests/test_gpu_cv_sparse_gaussian.py): oemgpu_cv_sparse_score_res after the fold layout and the compressed rows
 * alone -- no moments, nothing fitted, so a fold may leave fewer rows than columns -- on a table of the caller's: the sparse sibling of
 * oemgpu_selftest_cv_score_dev.  The row checks of phase 1 and the checks of phase 2. */
int oemgpu_selftest_cv_sparse_score(oemgpu_ctx *ctx, const oemgpu_sparse_x *x, const double *y_dev, const int32_t *foldid_dev, int32_t nfolds,
                                    const double *coef, int32_t npen, int32_t nl, const int32_t *ncol, int32_t type_measure, double *triples,
                                    double *predmat_dev /* or NULL */);
/* Host-only plan of the two entries above (pure arithmetic, runs without a GPU; the entries take their layout from the same function):
 * out[0] 1 if the fold moments take the compressed-column kernel and 0 for row tiles, out[1] workgroups of the scoring launch (four waves
 * each; x npen x out[3]), out[2] its waves (the stride over the rows), out[3] blocks of 64 lambdas, out[4] bytes of the per-fold wave
 * partials = nfolds out[2] npen out[10] 32 (kept under 64 MB by lowering out[1], which never falls below 1), out[5] device bytes of
 * the call = out[6] (the xval layout) + out[7] (the sparse fold plan, without upload regions) + out[8] (this route's own: the
 * partials, 24 nfolds npen nl of triples, 4 npen, 4 out[9] of inverse positions, 8 p, each rounded up to 256), out[9] rows of the
 * fold-ordered layout at most, out[10] nl rounded up to 16, out[11] the fold alignment (8192).  OEMGPU_ERR_ARG on bad arguments and
 * nfolds outside 2..512, OEMGPU_ERR_UNSUPPORTED on n + 8192 nfolds >= 2^31. */
int oemgpu_selftest_cv_sparse_plan(int64_t n, int32_t p, int64_t nnz, int32_t nfolds, int32_t npen, int32_t nl, int32_t num_cu,
                                   int64_t *out /* 12 */);
/* Host-only plan of the compressed-column Gram kernel both sparse fits share (pure arithmetic, runs without a GPU): out[0] 8192-row
 * chunks of an n-row matrix, out[1] contiguous chunk ranges the launch splits them into (the range sums cost out[1] p^2 doubles, kept
 * under 256 MB), out[2] chunks per range (range r = chunks [r out[2], min(out[0], (r + 1) out[2])), possibly none for the last ranges),
 * out[3] bytes of LDS a workgroup asks for (the route is open while they fit the 160 KiB of a CU).  OEMGPU_ERR_ARG on n < 1 or p < 1. */
int oemgpu_selftest_csc_plan(int64_t n, int32_t p, int64_t *out /* 4 */);
/* What the most recent binomial fit of THIS thread did (dense or sparse): [0] row-pass ms [1] Z + Gram + Lanczos ms [2] inner-solve ms (the three only
 * with oemgpu_set_timing on the context; 0 otherwise) [3] IRLS steps [4] inner iterations [5] row passes [6] Gram builds [7] wall ms */
int oemgpu_last_logistic_stats(double *out /* 8 */);

/* predict.oem's product on the device (ref R/methods.R:48-109, 346-367; predict.hip): out_dev[c n + i] = f(coef[c][0] + sum_j x_ij
 * coef[c][1 + j]) for i < n, c < ncol -- [ncol][n], i.e. an n x ncol column-major matrix -- with f by type: 0 "link" (identity),
 * 1 "response" (1 / (1 + exp(-eta))), 2 "class" (eta > 0 ? 1.0 : 0.0), applied in the store.  coef (HOST): [ncol][p + 1], slot 0 of a
 * column its intercept (0.0 for none); it may go when the call returns (the call synchronises the context's stream).  x_dev: column-major
 * float64 with column stride ld >= n, read where it lies.  The product runs on the FP64 MFMA pipe, rows of x against 16-column tiles of
 * the table held in LDS -- whole, or in chunks of coefficient rows when it does not fit, so p has no limit -- with the intercept as a
 * pseudo-column of ones; x is read once while ncol <= 112 and ceil(ceil(ncol / 16) / 7) times beyond.  Rows >= n and the padding of the
 * last k-step are never loaded and enter by selection: a NaN or Inf at x[i][j] reaches row i of out and no other element.  No atomics:
 * two calls give the same bits, and so do the three dense layouts for the same values.
 * OEMGPU_ERR_ARG before a device is looked for: a NULL ctx or pointer, n, p or ncol < 1, type outside 0..2, ld < n, an x_dev that is
 * not on an 8-byte boundary. */
int oemgpu_predict_dev(oemgpu_ctx *ctx, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *coef, int32_t ncol, int32_t type,
                       double *out_dev);
/* oemgpu_predict_dev (ref R/methods.R:48-109, 346-367) on a ROW-major x_dev (x[i * ldr + j], ldr >= p) of dtype OEMGPU_F64 or
 * OEMGPU_F32, aligned to its element size only, read where it lies; float32 is widened in the register it was loaded into and all
 * arithmetic is FP64.  Columns p .. ldr - 1 of a row and rows >= n are never read.  The same operand values reach the MFMAs in the
 * same order as from the column-major entry: the same bits for the same values.  OEMGPU_ERR_ARG before a device is looked for: the
 * refusals of oemgpu_predict_dev (its `ld < n` has no counterpart), a dtype that is neither code, ldr < p and an x_dev that is not
 * aligned to its element. */
int oemgpu_predict_rm_dev(oemgpu_ctx *ctx, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *coef, int32_t ncol,
                          int32_t type, double *out_dev);
/* oemgpu_predict_dev (ref R/methods.R:48-109, 346-367: a dgCMatrix newx is multiplied as it is) on the resident sparse x: n and p are
 * the handle's, coef [ncol][x->p + 1], out_dev [ncol][x->n].  Every row is read from the compressed-row copy, its stored entries in
 * column order, with scalar FP64 FMAs from the intercept on; the table sits in LDS when its ncol (p + 1) doubles fit 140 KiB and is read
 * through the cache otherwise.  The summation order is not the dense kernel's, so neither are the last bits; two calls give the same
 * bits.  OEMGPU_ERR_ARG before a device is looked for: a NULL ctx, handle or pointer, ncol < 1, type outside 0..2; and for a handle on
 * another device than the context's. */
int oemgpu_predict_sparse_res(oemgpu_ctx *ctx, const oemgpu_sparse_x *x, const double *coef, int32_t ncol, int32_t type, double *out_dev);
/* Host-only plan of the two dense predict entries (ref R/methods.R:48-109, 346-367 is what they compute; pure arithmetic, runs without a
 * GPU; the entries take their launch shape from the same function).  layout: -1 column-major, OEMGPU_F64 or OEMGPU_F32 row-major (one
 * shape for the three: they differ in their loads only).  out[0] rows per workgroup (a multiple of 128; workgroup g takes rows
 * [g out[0], min(n, (g + 1) out[0]))), out[1] workgroups (none empty; at most two per CU while two fit its LDS, else one), out[2]
 * 16-column tiles per pass (<= 7), out[3] passes over x (1 while ncol <= 112), out[4] 0 if the coefficient tile of a pass -- K4 =
 * (p + 1 rounded up to 4) rows of 16 out[2] doubles -- stays in LDS (it fits 140 KiB) and 1 if it goes through LDS in chunks, out[5]
 * coefficient rows in LDS at once (K4, or 112 per chunk), out[6] dynamic LDS bytes (8 * 16 out[2] out[5], and 17,408 for the eight
 * waves' transposing tiles), out[7] chunks (1 unless out[4]).  OEMGPU_ERR_ARG for n, p, ncol or num_cu < 1, a layout that is none of
 * the three or a NULL out. */
int oemgpu_selftest_predict_plan(int64_t n, int32_t p, int32_t ncol, int32_t layout, int32_t num_cu, int64_t *out /* 8 */);

/* Self-test aid (tests/test_gpu_host.py): enqueue, on the context's stream, `blocks` workgroups that each occupy a whole CU and
 * spin for `ms` milliseconds -- "somebody else holds the CUs", for the fallback of the persistent engines.  Asynchronous. */
int oemgpu_selftest_hold_cus(oemgpu_ctx *ctx, int32_t blocks, double ms);

/* Host-only self-check of the group reordering (api.hip: group_run_permutation; pure arithmetic, runs without a GPU): for the groups of `o`
 * over q coordinates, the permutation (new position -> old position) that makes every group a run of neighbouring coordinates -- groups in
 * the order of their first member, members in their own order (the order the reference sums their squares in, ref src/oem_dense.h:193-315) --
 * which lets the register-resident engine at 1024 < q <= 4096 take group penalties whatever the layout.  Returns q and fills perm[0..q), or 0
 * when no reordering applies: the groups are runs already, a variable is listed in two groups, or the group vector does not cover q
 * coordinates.  (Groups of more than 32 members -- an owner's slice -- are reordered like the others: the engine sums their norms over
 * several owners.) */
int oemgpu_selftest_group_permutation(const oemgpu_opts *o, int32_t q, int32_t *perm);

/* Host-only self-check of how the register-resident engine at 1024 < q <= 4096 deals group runs to its workgroups (path_symcoop.hip:
 * symcoop_plan; pure arithmetic, runs without a GPU).  runs[0 .. nruns]: the starts of the runs of neighbouring coordinates (one per group,
 * ungrouped coordinates runs of one), runs[nruns] = q.  On return *nowners workgroups (0: no plan, the launch-per-iteration engines take the
 * call), workgroup g owning the owner_n[g] coordinates from owner_c0[g] on (<= 32; slices end at run boundaries, or after every fourth
 * coordinate inside a run of more than 32), and per coordinate j frag[2 j] = 2 (first owner of j's run) + (1 if the run does not start that
 * owner's slice), frag[2 j + 1] = the number of owners the run lies in; *split = the most owners of one run (0: no run is split).  The arrays
 * hold 192 / 192 / 2 q entries. */
int oemgpu_selftest_symcoop_owners(int32_t q, int32_t num_cu, const int32_t *runs, int32_t nruns, int32_t *owner_c0, int32_t *owner_n, int32_t *frag,
                                   int32_t *nowners, int32_t *split);

/* Host-only self-check of the CU-slot book of the persistent engines (pure arithmetic, runs without a GPU): `calls` concurrent callers
 * each place `ninst` instances of W cooperating workgroups with every instance on ONE XCD of a device with num_cu CUs (path_coop.hip,
 * q <= 512).  bases[k] = the XCD of call k's first instance (chosen where the XCDs are emptiest), *peak = the most CUs any XCD was
 * booked for while all calls were in flight (<= num_cu / 8 whenever that is possible).  OEMGPU_ERR_ARG if the calls would have to
 * wait for each other (more than 3/4 of the CUs). */
int oemgpu_selftest_coop_slots(int32_t num_cu, int32_t W, int32_t ninst, int32_t calls, int32_t *bases, int32_t *peak);

/* Self-test / measurement aid: out = XX vec for a symmetric q x q matrix (q > 4096, column-major, device) through the packed lower
 * triangle the launch-per-iteration Gram engine streams beyond q = 4096 (path_large.hip: sympk_*; replaces the GEMV of
 * ref src/oem_xtx.h:378-381 / src/oem_dense.h:508-512): the pack, then `reps` products back to back between two HIP events on the
 * context's stream.  *us_per_product = the product kernel's own duration (bench.py prices 4 q^2 + 512 q + 8 q ceil(q / 128) bytes
 * against it).  Synchronises the stream. */
int oemgpu_selftest_sympk_gemv(oemgpu_ctx *ctx, const double *xx_dev, int32_t q, const double *vec_dev, double *out_dev, int32_t reps,
                               double *us_per_product);

/* The OEM_* / OEMGPU_* environment switches (engine selection for tests, knobs of the host-resident upload; none is needed in
 * production: DESIGN.md section 7b) are parsed ONCE, at the first call into the library.  oemgpu_reload_switches() parses the
 * environment again (tests); oemgpu_switch_names() is the space-separated list of every name the library reads. */
void        oemgpu_reload_switches(void);
const char *oemgpu_switch_names(void);

const char *oemgpu_last_error(void);
const char *oemgpu_version(void);
int         oemgpu_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* OEMGPU_H */
