/* tests/r_shim_logistic_sparse/fake_logistic_sparse.c -- TESTS ONLY: a recording fake of liboemgpu's sparse binomial entry for
 * r/oem_shim_logistic_sparse.c (tests/test_logistic_sparse_cpu.py links it with the stand-in R runtime of tests/r_api_stub/ and driver.c). */
#include <stdio.h>
#include <string.h>

#include "fake_logistic_sparse.h"

struct logit_record lfake;
int lfake_rc = 0;
int lfake_poll_interrupt = 0;
static char msg[128] = "";

double lfake_beta(int k, int i, int j) { return 1000.0 * k + 10.0 * i + j + 0.5; }

int oemgpu_fit_logistic_sparse(int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values, const double *y,
                               int32_t standardize, int32_t intercept, int32_t irls_maxit, double irls_tol, const oemgpu_opts *o,
                               double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    memset(&lfake, 0, sizeof lfake);
    lfake.calls = 1;
    lfake.colptr = colptr; lfake.rowidx = rowidx; lfake.values = values; lfake.y = y; lfake.n = n; lfake.p = p;
    lfake.standardize = standardize; lfake.intercept = intercept; lfake.irls_maxit = irls_maxit; lfake.irls_tol = irls_tol; lfake.o = *o;
    if (lfake_poll_interrupt && o->interrupt && (lfake.interrupt_answer = o->interrupt(o->interrupt_arg)) != 0) {
        snprintf(msg, sizeof msg, "interrupted");
        return OEMGPU_ERR_INTERRUPTED;
    }
    if (lfake_rc) { snprintf(msg, sizeof msg, "fake failure %d", lfake_rc); return lfake_rc; }
    const int nl = o->nlambda_user > 0 ? o->nlambda_user : o->nlambda;
    for (int k = 0; k < o->npen; k++)
        for (int i = 0; i < nl; i++) {
            for (int j = 0; j <= p; j++) beta[((size_t)k * nl + i) * (p + 1) + j] = lfake_beta(k, i, j);
            lambda_out[k * nl + i] = 1.0 / (1 + i + k);
            niter[k * nl + i] = 3 + i;
            loss[k * nl + i] = 100.0 + i;
        }
    *d = LFAKE_D;
    return 0;
}

const char *oemgpu_last_error(void) { return msg; }
