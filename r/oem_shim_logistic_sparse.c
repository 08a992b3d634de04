/*
 * oem_shim_logistic_sparse.c -- the R-side binding of the sparse binomial fit: the reference's RcppExport `oem_fit_logistic_sparse`
 * (ref src/oem_logistic_sparse.cpp:29-48, the same unmangled symbol and the same 19 SEXP arguments), so that R/oem.R's
 * oemfit.binomial on a dgCMatrix x (R/oem.R:603-624: `.Call("oem_fit_logistic_sparse", ..., PACKAGE = "oem")`) resolves to it
 * unchanged.  R C API only; the numerics are in liboemgpu.so behind include/oemgpu.h (oemgpu_fit_logistic_sparse).
 *
 * A translation unit of its own next to oem_shim.c and oem_shim_logistic.c (same build, replacing oem_logistic_sparse.cpp).  The
 * dgCMatrix slots are read as oem_shim.c's oem_fit_sparse reads them, the options as oem_shim_logistic.c reads them; its helpers are
 * small copies, kept static here.  opts$hessian.type is not read (the reference's sparse fit never reads it: it rebuilds X'WX at every
 * IRLS step) and neither is opts$ncores (the library serves the reference's single-thread branch, R's default).
 */
#include <R.h>
#include <Rinternals.h>
#include <Rinterface.h>      /* Rf_onintr */
#include <string.h>

#include "oemgpu.h"

static const char *LSP_PENALTIES[OEMGPU_NPENALTIES] = {      /* ref R/oem.R:165-173 */
    "elastic.net", "lasso", "ols", "mcp", "scad", "mcp.net", "scad.net", "grp.lasso", "grp.lasso.net",
    "grp.mcp", "grp.scad", "grp.mcp.net", "grp.scad.net", "sparse.grp.lasso"};

/* interrupts as in oem_shim.c: caught under R_ToplevelExec, re-raised after the library has unwound (polled between IRLS steps) */
static void lsp_check_interrupt(void *unused) { (void)unused; R_CheckUserInterrupt(); }
static int lsp_interrupted(void *unused) { (void)unused; return R_ToplevelExec(lsp_check_interrupt, NULL) == FALSE; }

static SEXP lsp_opt(SEXP list, const char *name)
{
    SEXP names = Rf_getAttrib(list, R_NamesSymbol);
    for (R_xlen_t i = 0; i < XLENGTH(list); i++)
        if (strcmp(CHAR(STRING_ELT(names, i)), name) == 0) return VECTOR_ELT(list, i);
    Rf_error("opts$%s is missing", name);
    return R_NilValue;
}

SEXP oem_fit_logistic_sparse(SEXP x_, SEXP y_, SEXP family_, SEXP penalty_, SEXP weights_, SEXP groups_, SEXP unique_groups_,
                             SEXP group_weights_, SEXP lambda_, SEXP nlambda_, SEXP lmin_ratio_, SEXP alpha_, SEXP gamma_,
                             SEXP tau_, SEXP penalty_factor_, SEXP standardize_, SEXP intercept_, SEXP compute_loss_, SEXP opts_)
{
    (void)family_;                                       /* the reference reads it only to add the intercept (cpp :121-130) */
    if (XLENGTH(weights_) > 0) Rf_error("weights not implemented yet.");                    /* R/oem.R:244 */
    /* a dgCMatrix: Dim, the 32-bit column pointers p (widened here), the row indices i and the values x */
    SEXP dim = R_do_slot(x_, Rf_install("Dim")), ip = R_do_slot(x_, Rf_install("p")), ii = R_do_slot(x_, Rf_install("i")),
         xv = R_do_slot(x_, Rf_install("x"));
    const int64_t n = INTEGER(dim)[0];
    const int p = INTEGER(dim)[1];
    int64_t *colptr = (int64_t *)R_alloc((size_t)p + 1, sizeof(int64_t));
    for (int j = 0; j <= p; j++) colptr[j] = INTEGER(ip)[j];
    oemgpu_opts o;
    memset(&o, 0, sizeof o);
    o.npen = (int32_t)XLENGTH(penalty_);
    int32_t *pen = (int32_t *)R_alloc(o.npen, sizeof(int32_t));
    for (int k = 0; k < o.npen; k++) {
        pen[k] = -1;
        for (int c = 0; c < OEMGPU_NPENALTIES; c++)
            if (strcmp(CHAR(STRING_ELT(penalty_, k)), LSP_PENALTIES[c]) == 0) pen[k] = c;
        if (pen[k] < 0) Rf_error("unknown penalty '%s'", CHAR(STRING_ELT(penalty_, k)));
    }
    o.penalty = pen;
    o.nlambda = Rf_asInteger(nlambda_);
    o.lambda_min_ratio = Rf_asReal(lmin_ratio_);
    R_xlen_t nlu = XLENGTH(VECTOR_ELT(lambda_, 0));              /* list of one vector per penalty, possibly empty (R/oem.R:366-404) */
    if (nlu > 0) {
        double *lam = (double *)R_alloc((size_t)o.npen * nlu, sizeof(double));
        for (int k = 0; k < o.npen; k++) memcpy(lam + (size_t)k * nlu, REAL(VECTOR_ELT(lambda_, k)), sizeof(double) * nlu);
        o.lambda_user = lam;
        o.nlambda_user = (int32_t)nlu;
    }
    o.alpha = Rf_asReal(alpha_); o.gamma = Rf_asReal(gamma_); o.tau = Rf_asReal(tau_);
    o.tol = Rf_asReal(lsp_opt(opts_, "tol"));                                             /* cpp :88-93 */
    o.maxit = Rf_asInteger(lsp_opt(opts_, "maxit"));
    const int irls_maxit = Rf_asInteger(lsp_opt(opts_, "irls_maxit"));
    const double irls_tol = Rf_asReal(lsp_opt(opts_, "irls_tol"));
    o.compute_loss = Rf_asLogical(compute_loss_);
    o.penalty_factor = REAL(penalty_factor_);
    o.groups = XLENGTH(groups_) ? INTEGER(groups_) : NULL;                          o.ngroupvars = (int32_t)XLENGTH(groups_);
    o.unique_groups = XLENGTH(unique_groups_) ? INTEGER(unique_groups_) : NULL;     o.ngroups = (int32_t)XLENGTH(unique_groups_);
    o.group_weights = XLENGTH(group_weights_) ? REAL(group_weights_) : NULL;        o.n_group_weights = (int32_t)XLENGTH(group_weights_);
    o.device = -1;
    o.interrupt = lsp_interrupted;
    const int nl = o.nlambda_user > 0 ? o.nlambda_user : o.nlambda;
    const size_t nk = (size_t)o.npen * nl;
    const int rows = p + 1;
    double *beta = (double *)R_alloc(nk * rows, sizeof(double)), *lamo = (double *)R_alloc(nk, sizeof(double));
    double *loss = (double *)R_alloc(nk, sizeof(double)), d = 0.0;
    int32_t *niter = (int32_t *)R_alloc(nk, sizeof(int32_t));
    const int rc = oemgpu_fit_logistic_sparse(n, p, colptr, INTEGER(ii), REAL(xv), REAL(y_), Rf_asLogical(standardize_), Rf_asLogical(intercept_),
                                              irls_maxit, irls_tol, &o, beta, lamo, niter, loss, &d);
    if (rc == OEMGPU_ERR_INTERRUPTED) Rf_onintr();
    if (rc != 0) Rf_error("%s", oemgpu_last_error());
    /* List(beta, lambda, niter, loss, d) as cpp :302-306; "ols": a vector, one niter, one loss (cpp :281-287) */
    SEXP res = PROTECT(Rf_allocVector(VECSXP, 5)), names = PROTECT(Rf_allocVector(STRSXP, 5));
    const char *nm[5] = {"beta", "lambda", "niter", "loss", "d"};
    for (int i = 0; i < 5; i++) SET_STRING_ELT(names, i, Rf_mkChar(nm[i]));
    SEXP lb = PROTECT(Rf_allocVector(VECSXP, o.npen)), ll = PROTECT(Rf_allocVector(VECSXP, o.npen));
    SEXP ln = PROTECT(Rf_allocVector(VECSXP, o.npen)), lo = PROTECT(Rf_allocVector(VECSXP, o.npen));
    for (int k = 0; k < o.npen; k++) {
        const int ols = pen[k] == OEMGPU_OLS;
        const int nlam = ols ? 1 : nl;
        SEXP b = ols ? Rf_allocVector(REALSXP, rows) : Rf_allocMatrix(REALSXP, rows, nl);
        SET_VECTOR_ELT(lb, k, b);
        memcpy(REAL(b), beta + (size_t)k * nl * rows, sizeof(double) * (size_t)rows * nlam);
        SEXP l = Rf_allocVector(REALSXP, nl);  SET_VECTOR_ELT(ll, k, l);  memcpy(REAL(l), lamo + (size_t)k * nl, sizeof(double) * nl);
        SEXP it = Rf_allocVector(INTSXP, nlam); SET_VECTOR_ELT(ln, k, it); memcpy(INTEGER(it), niter + (size_t)k * nl, sizeof(int) * nlam);
        SEXP ls = Rf_allocVector(REALSXP, nlam); SET_VECTOR_ELT(lo, k, ls); memcpy(REAL(ls), loss + (size_t)k * nl, sizeof(double) * nlam);
    }
    SET_VECTOR_ELT(res, 0, lb); SET_VECTOR_ELT(res, 1, ll); SET_VECTOR_ELT(res, 2, ln); SET_VECTOR_ELT(res, 3, lo);
    SET_VECTOR_ELT(res, 4, Rf_ScalarReal(d));
    Rf_setAttrib(res, R_NamesSymbol, names);
    UNPROTECT(6);
    return res;
}
