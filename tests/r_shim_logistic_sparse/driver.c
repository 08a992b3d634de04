/* tests/r_shim_logistic_sparse/driver.c -- TESTS ONLY.  Calls r/oem_shim_logistic_sparse.c's `oem_fit_logistic_sparse` the way
 * R/oem.R:603-624 does, with a dgCMatrix x, over the stand-in R runtime (tests/r_api_stub/) and the recording fake of this directory,
 * and checks what reaches the C ABI (each of the 19 arguments, the 32-bit column pointers widened), the returned list (names, storage
 * modes, dimensions, "ols" as a vector; ref src/oem_logistic_sparse.cpp:281-306), the protect balance, the error texts and the
 * re-raised interrupt.  Prints "logistic sparse shim driver: N checks passed" or aborts. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "R.h"
#include "fake_logistic_sparse.h"
#include "r_stub_runtime.h"

SEXP oem_fit_logistic_sparse(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);

static int checks;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "logistic sparse shim driver: line %d: %s\n", __LINE__, #c); abort(); } checks++; } while (0)

static SEXP R(SEXP x) { stub_root(x); return x; }
static SEXP real1(double v) { return R(stub_real(&v, 1)); }
static SEXP int1(int v) { return R(stub_int(&v, 1)); }
static SEXP str1(const char *s) { return R(stub_str(&s, 1)); }
static SEXP empty_real(void) { return R(stub_real(NULL, 0)); }
static SEXP empty_int(void) { return R(stub_int(NULL, 0)); }

enum { N = 8, P = 3, NL = 4, NNZ = 5 };
static double Y[N], PF[P] = {1.0, 0.5, 2.0};
static int CP[P + 1] = {0, 2, 3, 5}, RI[NNZ] = {0, 4, 2, 1, 5};
static double XV[NNZ] = {1.5, -2.0, 3.0, 4.0, -5.0};
static SEXP last_i, last_x;

/* a dgCMatrix with the slots Dim, p, i, x */
static SEXP dgc(void)
{
    int dim[2] = {N, P};
    SEXP m = R(stub_s4());
    last_i = R(stub_int(RI, NNZ)); last_x = R(stub_real(XV, NNZ));
    Rf_setAttrib(m, Rf_install("Dim"), R(stub_int(dim, 2)));
    Rf_setAttrib(m, Rf_install("p"), R(stub_int(CP, P + 1)));
    Rf_setAttrib(m, Rf_install("i"), last_i);
    Rf_setAttrib(m, Rf_install("x"), last_x);
    return m;
}

static SEXP make_opts(const char *hess)
{
    const char *names[7] = {"maxit", "tol", "irls_maxit", "irls_tol", "accelerate", "ncores", "hessian.type"};
    SEXP o = R(stub_list(7));
    int maxit = 321, irls = 17, nc = 1;
    double tol = 1e-9, irls_tol = 2e-4;
    SET_VECTOR_ELT(o, 0, stub_int(&maxit, 1));
    SET_VECTOR_ELT(o, 1, stub_real(&tol, 1));
    SET_VECTOR_ELT(o, 2, stub_int(&irls, 1));
    SET_VECTOR_ELT(o, 3, stub_real(&irls_tol, 1));
    SET_VECTOR_ELT(o, 4, stub_lgl(0));
    SET_VECTOR_ELT(o, 5, stub_int(&nc, 1));
    SET_VECTOR_ELT(o, 6, stub_str(&hess, 1));
    stub_set_names(o, names);
    return o;
}

static SEXP lambda_list(int npen, int len)
{
    SEXP l = R(stub_list(npen));
    for (int k = 0; k < npen; k++) {
        double v[8];
        for (int i = 0; i < len; i++) v[i] = 1.0 / (1 + i);
        SET_VECTOR_ELT(l, k, stub_real(v, len));
    }
    return l;
}

static SEXP call(SEXP pens, SEXP w, SEXP g, SEXP ug, SEXP gw, SEXP lam, const char *hess)
{
    SEXP x = dgc(), y = R(stub_real(Y, N));
    return oem_fit_logistic_sparse(x, y, str1("binomial"), pens, w, g, ug, gw, lam, int1(NL), real1(2e-3), real1(0.75), real1(3.5),
                                   real1(0.25), R(stub_real(PF, P)), R(stub_lgl(1)), R(stub_lgl(1)), R(stub_lgl(1)), make_opts(hess));
}

static void check_list(SEXP res, const int *codes, int npen, int nl)
{
    const char *nm[5] = {"beta", "lambda", "niter", "loss", "d"};
    CHECK(TYPEOF(res) == VECSXP && XLENGTH(res) == 5);
    SEXP names = Rf_getAttrib(res, R_NamesSymbol);
    for (int i = 0; i < 5; i++) CHECK(strcmp(CHAR(STRING_ELT(names, i)), nm[i]) == 0);
    for (int i = 0; i < 4; i++) CHECK(TYPEOF(VECTOR_ELT(res, i)) == VECSXP && XLENGTH(VECTOR_ELT(res, i)) == npen);
    CHECK(TYPEOF(VECTOR_ELT(res, 4)) == REALSXP && REAL(VECTOR_ELT(res, 4))[0] == LFAKE_D);
    for (int k = 0; k < npen; k++) {
        const int ols = codes[k] == OEMGPU_OLS, nlam = ols ? 1 : nl;
        SEXP b = VECTOR_ELT(VECTOR_ELT(res, 0), k);
        CHECK(TYPEOF(b) == REALSXP && XLENGTH(b) == (R_xlen_t)(P + 1) * nlam);
        SEXP dim = Rf_getAttrib(b, R_DimSymbol);
        if (ols) CHECK(dim == R_NilValue);
        else CHECK(dim != R_NilValue && INTEGER(dim)[0] == P + 1 && INTEGER(dim)[1] == nl);
        for (int i = 0; i < nlam; i++)
            for (int j = 0; j <= P; j++) CHECK(REAL(b)[i * (P + 1) + j] == lfake_beta(k, i, j));
        CHECK(TYPEOF(VECTOR_ELT(VECTOR_ELT(res, 1), k)) == REALSXP && XLENGTH(VECTOR_ELT(VECTOR_ELT(res, 1), k)) == nl);
        SEXP it = VECTOR_ELT(VECTOR_ELT(res, 2), k), lo = VECTOR_ELT(VECTOR_ELT(res, 3), k);
        CHECK(TYPEOF(it) == INTSXP && XLENGTH(it) == nlam && INTEGER(it)[0] == 3);
        CHECK(TYPEOF(lo) == REALSXP && XLENGTH(lo) == nlam && REAL(lo)[0] == 100.0);
    }
}

int main(void)
{
    for (int i = 0; i < N; i++) Y[i] = i % 2;
    const char *pens[3] = {"lasso", "ols", "grp.lasso"};
    const int codes[3] = {OEMGPU_LASSO, OEMGPU_OLS, OEMGPU_GRP_LASSO};
    const int groups[P + 1] = {0, 1, 1, 2}, ugroups[3] = {0, 1, 2};
    /* ---- three penalties, generated grid, groups with the intercept's 0, hessian.type "full" (not read) ---- */
    {
        SEXP g = R(stub_int(groups, P + 1)), ug = R(stub_int(ugroups, 3));
        if (setjmp(stub_jmp)) { fprintf(stderr, "unexpected R error: %s\n", stub_error_msg); abort(); }
        SEXP res = call(R(stub_str(pens, 3)), empty_real(), g, ug, empty_real(), lambda_list(3, 0), "full");
        CHECK(stub_protect_depth() == 0);
        R(res);
        CHECK(lfake.calls == 1 && lfake.n == N && lfake.p == P && lfake.standardize == 1 && lfake.intercept == 1);
        CHECK(lfake.irls_maxit == 17 && lfake.irls_tol == 2e-4);
        for (int j = 0; j <= P; j++) CHECK(lfake.colptr[j] == (int64_t)CP[j]);        /* the 32-bit slot widened */
        CHECK(lfake.rowidx == INTEGER(last_i) && lfake.values == REAL(last_x) && lfake.y != NULL && lfake.y[1] == 1.0);
        CHECK(lfake.o.lambda_min_ratio == 2e-3 && lfake.o.penalty_factor[2] == 2.0 && lfake.o.device == -1);
        CHECK(lfake.o.maxit == 321 && lfake.o.tol == 1e-9 && lfake.o.npen == 3 && lfake.o.nlambda == NL && lfake.o.nlambda_user == 0);
        for (int k = 0; k < 3; k++) CHECK(lfake.o.penalty[k] == codes[k]);
        CHECK(lfake.o.ngroupvars == P + 1 && lfake.o.ngroups == 3 && lfake.o.groups[0] == 0 && lfake.o.n_group_weights == 0);
        CHECK(lfake.o.alpha == 0.75 && lfake.o.gamma == 3.5 && lfake.o.tau == 0.25 && lfake.o.compute_loss == 1);
        CHECK(lfake.o.interrupt != NULL);
        check_list(res, codes, 3, NL);
        stub_end_call();
    }
    /* ---- user lambdas, "upper.bound" (not read either) ---- */
    {
        if (setjmp(stub_jmp)) { fprintf(stderr, "unexpected R error: %s\n", stub_error_msg); abort(); }
        SEXP res = call(R(stub_str(pens, 2)), empty_real(), empty_int(), empty_int(), empty_real(), lambda_list(2, 3), "upper.bound");
        CHECK(stub_protect_depth() == 0);
        R(res);
        CHECK(lfake.o.nlambda_user == 3 && lfake.o.lambda_user[1] == 0.5 && lfake.o.groups == NULL);
        check_list(res, codes, 2, 3);
        stub_end_call();
    }
    /* ---- errors: weights, an argument error (the library's text; hessian.type "newton" is not read), a refused problem, an unknown penalty ---- */
    for (int variant = 0; variant < 4; variant++) {
        double w[N] = {1, 1, 1, 1, 1, 1, 1, 1};
        const char *bad = "ridge";
        lfake.calls = 0;
        lfake_rc = variant == 2 ? OEMGPU_ERR_UNSUPPORTED : variant == 1 ? OEMGPU_ERR_ARG : 0;
        const int jumped = setjmp(stub_jmp);
        if (!jumped) {
            (void)call(variant == 3 ? str1(bad) : R(stub_str(pens, 1)), variant == 0 ? R(stub_real(w, N)) : empty_real(), empty_int(),
                       empty_int(), empty_real(), lambda_list(1, 0), variant == 1 ? "newton" : "upper.bound");
            CHECK(0);
        }
        CHECK(jumped == 1);
        if (variant == 0) CHECK(strstr(stub_error_msg, "weights not implemented yet") && lfake.calls == 0);
        if (variant == 1) CHECK(strcmp(stub_error_msg, "fake failure -1") == 0 && lfake.calls == 1);
        if (variant == 2) CHECK(strcmp(stub_error_msg, "fake failure -4") == 0);
        if (variant == 3) CHECK(strstr(stub_error_msg, "unknown penalty 'ridge'"));
        CHECK(stub_protect_depth() == 0);
        lfake_rc = 0;
        stub_end_call();
    }
    /* ---- a user interrupt: polled by the library, re-raised by the shim with Rf_onintr ---- */
    for (int pending = 0; pending < 2; pending++) {
        lfake_poll_interrupt = 1; stub_pending_interrupt = pending;
        const int jumped = setjmp(stub_jmp);
        if (!jumped) {
            SEXP res = call(R(stub_str(pens, 1)), empty_real(), empty_int(), empty_int(), empty_real(), lambda_list(1, 0), "upper.bound");
            CHECK(!pending && lfake.interrupt_answer == 0);
            R(res);
            check_list(res, codes, 1, NL);
        } else
            CHECK(pending && jumped == 2 && lfake.interrupt_answer != 0);
        CHECK(stub_protect_depth() == 0);
        lfake_poll_interrupt = 0; stub_pending_interrupt = 0;
        stub_end_call();
    }
    printf("logistic sparse shim driver: %d checks passed\n", checks);
    return 0;
}
