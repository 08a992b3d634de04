// logistic.hpp -- the IRLS driver of the binomial fits (logistic.hip) and what a data layout hands it.  The dense fit
// (logistic.hip) and the sparse fit (logistic_sparse.hip) share the driver: the lambda grid, the IRLS loop and its stop, the
// inner OEM loop (one workgroup or the launch form), d from the device Lanczos, A = dI - XX, XY = XX beta + grad and the
// back-transform.  Only the two passes over the data differ.
#pragma once
#include "ctx.hpp"

namespace oemgpu {

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
extern const int LOGIT_WG_MAX_Q;                         // q up to which the inner solve is one persistent workgroup
extern const int LOGIT_P_LIMIT;                          // the largest p served

}  // namespace oemgpu
