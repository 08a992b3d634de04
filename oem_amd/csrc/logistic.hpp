// logistic.hpp -- the IRLS driver of the binomial fits (logistic.hip) and what a data layout hands it.  The dense fit
// (logistic.hip) and the sparse fit (logistic_sparse.hip) share the driver: the lambda grid, the IRLS loop and its stop, the
// inner OEM loop (one workgroup or the launch form), d from the device Lanczos, A = dI - XX, XY = XX beta + grad and the
// back-transform.  Only the two passes over the data differ.
#pragma once
#include "dense_src.hpp"

#include <vector>

// A sparse x resident on a device (oemgpu_sparse_x_create; cv.oem's fold fits and scoring read it there): the compressed columns as
// they came, the chunk pointers of the compressed-column kernels and the compressed-row copy with every row's entries in column
// order -- what SparseLogitData::bind builds for a single fit, built once.  One allocation of its own (`base`), not the context's.
struct oemgpu_sparse_x {
    int device = 0;
    int64_t n = 0, nnz = 0, maxcol = 0;   // maxcol: the longest column
    int32_t p = 0;
    char *base = nullptr;
    size_t bytes = 0;
    int64_t *colptr = nullptr, *rowptr = nullptr;
    int32_t *rowidx = nullptr, *ccol = nullptr, *cptr = nullptr;
    double *val = nullptr, *cval = nullptr;
};

namespace oemgpu {

// logistic_sparse.hip: the handle from compressed columns csc_check has passed (rowptr: the n + 1 row pointers of the row copy; h_ccol /
// h_cval: that copy where the caller has made it on the host, else it is made on the device)
int sparse_x_build(oemgpu_ctx *c, int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values,
                   const std::vector<int64_t> &rowptr, int64_t maxcol, oemgpu_sparse_x **out, const int32_t *h_ccol = nullptr,
                   const double *h_cval = nullptr);

// The data-dependent stages of an IRLS fit.  Every stage enqueues on the context's stream.  g: p + 2 doubles, laid out as
// [sum r, X'r (p), sum of the loss terms] (logit_xy_kernel and the loss read it so).
struct LogitData {
    bool hess_every = false;          // the Hessian at every IRLS step (dense "full", the sparse fit); else only at the first of a penalty
    const double *intval = nullptr;   // device word: get_beta's in-place intercept scale (the sparse fit), or null
    virtual ~LogitData() {}
    virtual size_t ws_bytes() const = 0;                 // the stage's own workspace, carved out of the driver's buffer
    virtual int bind(char *ws) = 0;                      // the workspace is there: upload what the stages read
    virtual int scale(double *sc) = 0;                   // s, or ones without standardize
    virtual int xy0(const double *sc, double *g) = 0;    // g[1 .. p] = X'Y, g[0] = the intercept's term of the first XY
    // the row pass of IRLS step irls_i at beta -> g; gram: the Hessian build follows at the same beta
    virtual int rows(const double *beta, const double *sc, int64_t irls_i, bool gram, double *g) = 0;
    virtual int hessian(const double *beta, const double *sc, int64_t irls_i, double *g, double *xx) = 0;   // XX (q x q, over n)
};

int logistic_check(int64_t n, int32_t p, int32_t intercept, int32_t hessian_full, int32_t irls_maxit, double irls_tol, const oemgpu_opts *o);
int logistic_irls(oemgpu_ctx *c, LogitData &D, int64_t n, int32_t p, int32_t intercept, int32_t irls_maxit, double irls_tol, const oemgpu_opts *o,
                  double *beta_out, double *lambda_out, int32_t *niter, double *loss_out, double *d_out);
int launch_logit_fill(hipStream_t s, double *a, int n, double v);   // a[0 .. n) = v
// A fold fit's look at foldid (logit_fold_scan_kernel, once per call; scratch: the start of c->ws, read back before anything else uses
// it): *n_eff = rows with foldid != leave_out, kept_row[k] = the row of the k-th kept row for k < min(irls_maxit, n_eff) (the W floor
// tests the IRLS index among the kept rows); OEMGPU_ERR_ARG in `who`'s name when an id is outside [1, nfolds]
int logit_fold_scan(oemgpu_ctx *c, const char *who, const int32_t *foldid, int64_t n, int32_t nfolds, int32_t leave_out, int32_t irls_maxit,
                    int64_t *n_eff, std::vector<int64_t> *kept_row);
// A row-major x of float64 / float32 elements read where it lies (logistic_rm.hip).  The band plan of its row pass, pure host arithmetic:
// band b = columns [b bw, min(p, (b + 1) bw)); bw is a multiple of 4 unless there is one band (bw = p)
struct LogitRmPlan {
    int bw;            // columns per band
    int nband;         // bands
    size_t lds;        // dynamic LDS bytes of the row pass: the p accumulators and a 64-row tile of one band
    size_t lds_total;  // with the kernel's static arrays
};
LogitRmPlan logit_rm_plan(int p);
// logit_rows_kernel's launch (logistic.hip) for the row-major x: chunks c0 .. c0 + nc of ch rows, the Z block from row0 (or z null)
int launch_logit_rows_rm(hipStream_t s, const LogitRmPlan &R, const void *x, int dtype, int64_t n, int64_t ldr, int p, const double *y,
                         const double *beta, const double *sc, int intercept, int mode, int64_t irls_i, int64_t ch, int64_t c0, int64_t nc,
                         int64_t row0, double *z, int64_t ldz, double *part, const int32_t *foldid, int32_t leave_out);
// logit_scale_kernel for the row-major x; sp: 256 p doubles of workspace; fill_row: a row that is in the fit
int launch_logit_scale_rm(hipStream_t s, const void *x, int dtype, int64_t n, int64_t ldr, int p, double *sp, double *sc, const int32_t *foldid,
                          int32_t leave_out, int64_t n_eff, int64_t fill_row);
extern const int LOGIT_WG_MAX_Q;                        // q up to which the inner solve is one persistent workgroup
extern const int LOGIT_P_LIMIT;                          // the largest p served

}  // namespace oemgpu
