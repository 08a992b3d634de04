/* tests/r_shim_logistic_sparse/fake_logistic_sparse.h -- TESTS ONLY: what the recording fake saw in its last call. */
#ifndef OEM_TEST_FAKE_LOGISTIC_SPARSE_H
#define OEM_TEST_FAKE_LOGISTIC_SPARSE_H
#include "oemgpu.h"
struct logit_record {
    int calls;
    const int64_t *colptr; const int32_t *rowidx; const double *values, *y;
    int64_t n; int32_t p, standardize, intercept, irls_maxit;
    double irls_tol;
    oemgpu_opts o;
    int interrupt_answer;
};
extern struct logit_record lfake;
extern int lfake_rc, lfake_poll_interrupt;
double lfake_beta(int k, int i, int j);
#define LFAKE_D 2.5
#endif
