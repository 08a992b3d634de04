// logistic.hip -- the dense binomial fit: what `.Call("oem_fit_logistic_dense", ...)` computes (ref src/oem_logistic_dense.cpp:30-313,
// src/oem_logistic_dense.h:397-1094), restated as it is, quirks included:
//   * standardisation: colsq = sum x^2 / (n - 1), X NOT centred, 0 -> 1, s = 1 / sqrt(colsq) when `standardize` (h :727-738);
//   * the intercept is coordinate 0 of a q = p + 1 problem with penalty factor 0 (cpp :119-141); row / column 0 of XX is
//     [sum W, sum W x_j s_j] / n (h :463-481); without an intercept row 0 of the returned beta is 0 (cpp :246-253);
//   * XY = s o X'Y / n with the raw 0/1 Y, lambda_0 = max |XY| over the non-intercept slots (h :762-805);
//   * penalty -> lambda (warm start) -> IRLS step i < irls_maxit -> OEM iteration j < maxit (h :848-1036), no Nesterov step;
//   * one IRLS step: prob = 1 / (1 + exp(-(X (beta o s) + beta_0))), W = prob (1 - prob) with the floor loop that tests W(i) with the
//     IRLS index i (so at most element i is floored, h :953-959); XX, d = 1.0005 lambda_max(XX) (NOT 1.005, h :514) and A = dI - XX only
//     when (i == 0 && first lambda of the penalty) or hessian.type == "full" (h :964-965); grad = s o X'(y - prob) / n, grad_0 =
//     sum (y - prob) / n; XY = XX beta + grad (h :970-1000).  On a lambda after the first, the FIRST IRLS step skips all of that
//     (h :861): the inner loop runs at the new lambda on the previous step's XY / A / d.  IRLS stop: stopRule(beta, beta_irls,
//     irls_tol); niter = i + 1 (irls_maxit + 1 when the cap is hit, h :1035);
//   * loss: get_loss (the 1e-5 clamps, h :1057-1090) of the LAST prob computed, not of the final beta; d: the last d computed.
// Refused (api: OEMGPU_ERR_UNSUPPORTED): p + intercept >= n -- the reference's XWXt branch (h :490-496, 524-566) iterates on the raw
// labels instead of the IRLS response, least squares on 0/1 -- and p > LOGIT_P_MAX.
//
// Kernels:
//   * logit_rows_kernel: the row pass.  Workgroup c owns rows [c CH, (c + 1) CH) and walks them in sub-blocks of 64; from ONE read of
//     a sub-block (staged in LDS when 64 x p fits, else re-read through the cache) it forms eta, prob, W, r = y - prob and the loss terms,
//     and accumulates its partial of [sum r, X'r, sum loss] in fixed order.  With a Gram due it also writes Z = [sqrt W | sqrt W x s]
//     for the moment pass (gram.hip), in row blocks of RBZ rows so that the workspace stays bounded;
//   * logit_sum_kernel: the partials summed in chunk order (two calls give the same bits);
//   * logit_inner_kernel: q <= LOGIT_WG_MAX: the OEM loop of one lambda from a warm start in ONE workgroup (A in LDS when it fits),
//     to stopRule or maxit; beyond that launch_gemv (path_large.hip) + logit_thresh_kernel per iteration, batches of LOGIT_BATCH
//     launches between looks at the stop word.  The threshold's scratch (u + XY, the new beta, a factor per group) is in LDS when its
//     8 (2 q + ngroups) bytes fit LOGIT_LDS_BYTES, else in the workspace (one group per coordinate at p >= 6826);
//   * small kernels: XX from the moments, A = dI - XX, XY = XX beta + grad, the IRLS stop, the back-transform.
// cv.oem's fold fits (oemgpu_fit_logistic_dense_fold_dev; the scoring of the held-out rows is logistic_cv.hip): DenseLogitData with foldid /
// leave_out is the fit on the rows with foldid != leave_out of the same resident X -- the MASKED row pass leaves those rows out (their Z
// rows are zeros), logit_fold_scan_kernel counts the kept rows (n_eff, which stands where n enters the arithmetic) and maps the W floor's
// IRLS index to the i-th kept row.
// Many responses on one x (oemgpu_fit_logistic_dense_multi_dev / _rm_dev): logistic_irls_multi below runs the same
// algorithm for the m columns of Y in lock-step -- XX, d and A once per call (at beta = 0 they hold no y), the row pass of a step for
// all live responses from logistic_multi.hip, and this file's small kernels with a workgroup (or grid row) per response:
// logit_inner_multi_kernel is logit_inner_kernel's body (logit_inner_solve) per response.
// Their cross-validation (oemgpu_fit_logistic_dense_multi_fold_dev / _rm_dev): the same driver over INSTANCES (response,
// fold left out) -- s, XX, d and A once per distinct fold left out (a group), every instance a masked column of the shared row pass,
// the small kernels picking their instance's group.
// The host driver (logistic_irls) is shared with the sparse fit (logistic_sparse.hip): the passes over the data reach it as the stages of
// a LogitData (logistic.hpp); DenseLogitData below is this file's, over a column-major x or (the readers of logistic_rm.hip) a row-major x of
// float64 / float32 elements read where it lies (oemgpu_fit_logistic_dense_rm_dev, ..._fold_rm_dev; kernels: logistic_rm.hip).
#include "logistic.hpp"
#include "logistic_multi.hpp"
#include "penalty_ops.hpp"

#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

namespace oemgpu {

static const int LOGIT_WG_MAX = 1024;          // q up to which the inner solve is one persistent workgroup
static const int LOGIT_P_MAX = 8191;           // the row pass keeps its X'r accumulators in LDS (8 p bytes)
static const int LOGIT_STAGE_P = 192;          // p up to which a 64-row sub-block is staged in LDS (65 x 8 p bytes)
static const int LOGIT_A_LDS_Q = 110;          // q up to which the inner kernel keeps A in LDS (8 q^2 bytes)
static const int LOGIT_BATCH = 16;             // launch form: iterations enqueued between looks at the stop word
static const size_t LOGIT_Z_BYTES = (size_t)256 << 20;   // Z row blocks: at most this much (or one chunk of rows)
static const size_t LOGIT_LDS_BYTES = (size_t)160 << 10;  // LDS of a gfx950 CU: the most one workgroup may ask for

// state words (doubles) shared between the kernels and the host
enum { ST_LOSS = 0, ST_ITERS = 1, ST_IRLS_STOP = 2, ST_DONE = 3, ST_LEN = 8 };

struct LogitPlan {
    int64_t ch;        // rows per chunk (a multiple of 64)
    int64_t nchunk;    // chunks: chunk c = rows [c ch, min(n, (c + 1) ch))
    int64_t rbz;       // rows per Z block (a multiple of ch; 0: no Gram pass ever, never the case today)
    int64_t nzblk;     // Z blocks
    int inner_wg;      // 1: one persistent workgroup; 0: launch per iteration
    int staged;        // 1: the row pass stages its 64-row sub-blocks in LDS
    size_t ws_bytes;   // device workspace of a call (c->aux)
};

// launch form: the threshold kernel's scratch (us, bn: q each; gf: ngroups) in LDS when it fits, else in the workspace
static bool logit_thr_in_lds(int q, int ngroups)
{
    return 8 * (size_t)(2 * q + (ngroups > 0 ? ngroups : 1)) <= LOGIT_LDS_BYTES;
}

static LogitPlan logit_plan(int64_t n, int p, int intercept, int num_cu)
{
    LogitPlan P;
    const int q = p + (intercept ? 1 : 0);
    int64_t ch = (n + 4 * (int64_t)num_cu - 1) / (4 * (int64_t)num_cu);
    ch = (ch + 63) / 64 * 64;
    if (ch < 64) ch = 64;
    P.ch = ch;
    P.nchunk = (n + ch - 1) / ch;
    int64_t cpb = (int64_t)(LOGIT_Z_BYTES / ((size_t)ch * q * 8));
    if (cpb < 1) cpb = 1;
    if (cpb > P.nchunk) cpb = P.nchunk;
    P.rbz = cpb * ch;
    P.nzblk = (P.nchunk + cpb - 1) / cpb;
    P.inner_wg = q <= LOGIT_WG_MAX;
    P.staged = p <= LOGIT_STAGE_P;
    const GramPlan gp = gram_plan_bound(P.rbz < n ? P.rbz : n, q, num_cu);
    const size_t m2 = (size_t)(q + 2) * (q + 2);
    Bump B;
    B.take(8 * (size_t)p);                                  // s
    B.take(8 * (size_t)q * 4);                              // beta, beta_irls, u, XY
    B.take(8 * (size_t)q * q * 2);                          // XX, A
    B.take(8 * (size_t)(p + 2));                            // g
    B.take(8 * (size_t)P.nchunk * (p + 2));                 // chunk partials
    B.take(8 * (size_t)P.rbz * q);                          // Z block
    B.take(8 * m2 * 2);                                     // moments of a block, their running sum
    B.take(8 * gp.tpart_doubles); B.take(8 * gp.vpart_doubles);
    B.take(8 * ST_LEN); B.take(256);                        // state words, the stop word of the launch form
    B.take(8 * (size_t)q * 2 + 4 * (size_t)q * 3 + 4 * (size_t)(q + 1) + 8);   // pf, group weights, perm / group of / starts, ngroups
    if (!P.inner_wg && !logit_thr_in_lds(q, q)) B.take(8 * (size_t)q * 3);      // threshold scratch at the most groups (one per coordinate)
    P.ws_bytes = B.off;
    return P;
}

namespace {

// stopRule (ref src/utils.cpp:537-549): 1 = this coordinate does NOT stop the loop
__device__ __forceinline__ int stop_violated(double c, double pv, double tol)
{
    const bool cn = fabs(c) > 1e-13, pn = fabs(pv) > 1e-13;
    if (cn != pn) return 1;
    if (cn && pn && fabs((c - pv) / pv) > tol) return 1;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- row pass
// mode 0: r = y (X'Y for XY's first form and lambda_0); mode 1: the IRLS quantities.  zout: Z block (ldz rows), or null.
// MASKED (a fold fit): rows with foldid[row] == leave_out are not in the fit.  Such a row is never loaded; it adds nothing to sum r, X'r
// or the loss, and its Z row is written as zeros (the Z buffer is reused from block to block and from step to step, so it cannot be
// skipped).  irls_i is then the row of the i-th KEPT row.  The unmasked instantiations are the code they were before MASKED existed.
template <bool STAGED, bool MASKED>
__global__ __launch_bounds__(256) void logit_rows_kernel(const double *__restrict__ x, int64_t n, int64_t ld, int p, const double *__restrict__ y,
                                                         const double *__restrict__ beta, const double *__restrict__ s, int intercept, int mode,
                                                         int64_t irls_i, int64_t ch, int64_t chunk0, int64_t row0, double *__restrict__ zout,
                                                         int64_t ldz, double *__restrict__ part, const int32_t *__restrict__ foldid, int32_t leave_out)
{
    extern __shared__ double lsh[];
    double *acc = lsh;                               // p
    double *tile = lsh + p;                          // 65 p (STAGED)
    __shared__ double etap[4][64], rsh[64], wsh[64], red[2][64];
    __shared__ int ksh[64];                          // MASKED, not STAGED: 1 for a kept row of the sub-block
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int o = intercept ? 1 : 0;
    const int64_t c = chunk0 + blockIdx.x;
    const int64_t r_lo = c * ch, r_hi = (r_lo + ch < n) ? r_lo + ch : n;
    for (int j = tid; j < p; j += 256) acc[j] = 0.0;
    const double b0 = (mode && intercept) ? beta[0] : 0.0;
    double rsum = 0.0, lsum = 0.0;                   // wave 0: per-lane sums of r and of the loss terms
    for (int64_t r0 = r_lo; r0 < r_hi; r0 += 64) {
        const int64_t row = r0 + lane;
        const bool ok = row < r_hi;
        bool kept = ok;                              // the row is in the fit
        if (MASKED) kept = ok && foldid[row] != leave_out;
        // phase 1: wave w reads columns j = w (mod 4), lane = row (coalesced); eta partials
        double e = 0.0;
        if (mode) {
            for (int j = w; j < p; j += 4) {
                const double v = kept ? x[(size_t)j * ld + row] : 0.0;
                if (STAGED) tile[j * 65 + lane] = v;
                e = fma(v, beta[o + j] * s[j], e);
            }
        } else if (STAGED) {
            for (int j = w; j < p; j += 4) tile[j * 65 + lane] = kept ? x[(size_t)j * ld + row] : 0.0;
        }
        etap[w][lane] = e;
        __syncthreads();
        // phase 2: one wave forms prob, W, r and the loss terms of its 64 rows
        if (w == 0) {
            double r = 0.0, sw = 0.0;
            if (kept) {
                const double yi = y[row];
                if (mode) {
                    const double eta = ((etap[0][lane] + etap[1][lane]) + (etap[2][lane] + etap[3][lane])) + b0;
                    const double prob = 1.0 / (1.0 + exp(-eta));
                    double W = prob * (1.0 - prob);
                    if (row == irls_i && W < 1e-5) W = 1e-5;          // the reference's floor loop tests W(i), i the IRLS index (h :953-959)
                    sw = sqrt(W);
                    r = yi - prob;
                    double lt;
                    if (yi == 1.0) lt = prob > 1e-5 ? log(1.0 / prob) : log(1.0 / 1e-5);
                    else lt = prob <= 1.0 - 1e-5 ? log(1.0 / (1.0 - prob)) : log(1.0 / 1e-5);
                    lsum += lt;
                } else {
                    r = yi;
                }
                rsum += r;
            }
            if (ok && zout && o) zout[row - row0] = sw;
            rsh[lane] = r; wsh[lane] = sw;
            if (MASKED && !STAGED) ksh[lane] = kept ? 1 : 0;
        }
        __syncthreads();
        // phase 3: thread j accumulates column j over the 64 rows, in row order
        for (int j = tid; j < p; j += 256) {
            double a = acc[j];
            const int lim = (int)((r_hi - r0) < 64 ? (r_hi - r0) : 64);
            if (STAGED) {
                for (int i = 0; i < lim; ++i) a = fma(tile[j * 65 + i], rsh[i], a);
            } else if (MASKED) {
                const double *col = x + (size_t)j * ld + r0;
                for (int i = 0; i < lim; ++i) a = fma(ksh[i] ? col[i] : 0.0, rsh[i], a);
            } else {
                const double *col = x + (size_t)j * ld + r0;
                for (int i = 0; i < lim; ++i) a = fma(col[i], rsh[i], a);
            }
            acc[j] = a;
        }
        // phase 4: Z = sqrt(W) (x s) of these rows, coalesced as in phase 1
        if (zout && ok) {
            for (int j = w; j < p; j += 4) {
                const double v = STAGED ? tile[j * 65 + lane] : (kept ? x[(size_t)j * ld + row] : 0.0);
                zout[(size_t)(o + j) * ldz + (row - row0)] = wsh[lane] * (v * s[j]);
            }
        }
        __syncthreads();
    }
    if (w == 0) { red[0][lane] = rsum; red[1][lane] = lsum; }
    __syncthreads();
    double *pc = part + (size_t)c * (p + 2);
    for (int j = tid; j < p; j += 256) pc[1 + j] = acc[j];
    if (tid == 0) {
        double a = 0.0, b = 0.0;
        for (int i = 0; i < 64; ++i) { a += red[0][i]; b += red[1][i]; }
        pc[0] = a; pc[p + 1] = b;
    }
}

// g[j] = ((part[0][j] + part[1][j]) + part[2][j]) + ... : chunk order
__global__ __launch_bounds__(256) void logit_sum_kernel(const double *__restrict__ part, int64_t nchunk, int len, double *__restrict__ g)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= len) return;
    double a = 0.0;
    for (int64_t c = 0; c < nchunk; ++c) a += part[(size_t)c * len + j];
    g[j] = a;
}

// ---------------------------------------------------------------------------------------------------------------- Gram pieces
// XX = Z'Z / n from the lower triangle of the moments ((q + 2) x (q + 2), column-major)
__global__ __launch_bounds__(256) void logit_xx_kernel(const double *__restrict__ M, int q, double n, double *__restrict__ xx)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= q) return;
    const int hi = i > j ? i : j, lo = i > j ? j : i;
    xx[(size_t)j * q + i] = M[(size_t)lo * (q + 2) + hi] / n;
}

// A = dI - XX (h :518-519: A = -XX, then d added to the diagonal)
__global__ __launch_bounds__(256) void logit_a_kernel(const double *__restrict__ xx, int q, double d, double *__restrict__ a)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= q) return;
    const size_t k = (size_t)j * q + i;
    a[k] = i == j ? -xx[k] + d : -xx[k];
}

// XY = XX beta + grad; grad = s o X'(y - prob) / n, grad_0 = sum (y - prob) / n (h :973-999).  init: the first XY = s o X'Y / n (h :762-792)
__global__ __launch_bounds__(256) void logit_xy_kernel(const double *__restrict__ xx, const double *__restrict__ beta, const double *__restrict__ g,
                                                       const double *__restrict__ s, int p, int intercept, double n, int init, double *__restrict__ xy)
{
    const int q = p + (intercept ? 1 : 0);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= q) return;
    const bool icpt = intercept && i == 0;
    const int j = i - (intercept ? 1 : 0);
    if (init) { xy[i] = icpt ? g[0] / n : (g[1 + j] * s[j]) / n; return; }
    const double gr = icpt ? g[0] / n : (g[1 + j] / n) * s[j];
    double a = 0.0;
    for (int k = 0; k < q; ++k) a = fma(xx[(size_t)k * q + i], beta[k], a);
    xy[i] = a + gr;
}

// ---------------------------------------------------------------------------------------------------------------- threshold
struct LogitPen {
    PenK k;
    const double *pf;         // q
    const double *gw;         // ngroups (group weights, the reference's pen_fact(g) of the group operators)
    const int *perm;          // q: coordinates ordered by group (members in index order)
    const int *gstart;        // ngroups + 1: group g = perm[gstart[g] .. gstart[g + 1])
    const int *gof;           // q: group index of a coordinate, -1 if its id is not among unique_groups (then beta = 0)
    const int *gzero;         // ngroups: 1 if the group id is 0 (unpenalized, factor 1)
    int ngroups;
};

__device__ __forceinline__ double elem_thr(const PenK &k, double u, double pf)
{
    const double tp = pf * k.L;
    switch (k.kind) {
    case K_MCP: return mcp1(u, tp, k.D, k.gamma);
    case K_SCAD: return scad1(u, tp, k.D, k.gamma);
    case K_OLS: return u / k.D;
    default: return soft1(u, tp, k.D);
    }
}

// beta[0..q) <- next_beta(u) (h :569-672) by one workgroup of any size; u is overwritten for the group operators (sparse.grp.lasso: with
// its soft-thresholded copy); gf: LDS scratch of ngroups doubles.  Ends with a barrier.
__device__ void logit_threshold(const LogitPen &P, double *u, double *beta, int q, double *gf)
{
    const PenK &k = P.k;
    const int tid = threadIdx.x, nt = blockDim.x;
    if (k.kind < K_GRP) {
        for (int i = tid; i < q; i += nt) beta[i] = elem_thr(k, u[i], P.pf[i]);
        __syncthreads();
        return;
    }
    if (k.kind == K_SGL) {                       // soft threshold with denominator 1 first (h :653-668)
        for (int i = tid; i < q; i += nt) u[i] = soft1(u[i], P.pf[i] * k.L1, 1.0);
        __syncthreads();
    }
    for (int g = tid; g < P.ngroups; g += nt) {
        double f = 1.0;
        if (!P.gzero[g]) {
            double ss = 0.0;
            for (int m = P.gstart[g]; m < P.gstart[g + 1]; ++m) { const double v = u[P.perm[m]]; ss += v * v; }
            const double nrm = sqrt(ss), pen = k.L * P.gw[g];
            if (k.kind == K_GRP_MCP) f = mcp_norm(nrm, pen, k.D, k.gamma);
            else if (k.kind == K_GRP_SCAD) f = scad_norm(nrm, pen, k.D, k.gamma);
            else f = fmax(0.0, 1.0 - pen / nrm);
        }
        gf[g] = f;
    }
    __syncthreads();
    for (int i = tid; i < q; i += nt) {
        const int g = P.gof[i];
        const double f = g >= 0 ? gf[g] : 0.0;
        beta[i] = f != 0.0 ? u[i] * f / k.D : 0.0;
    }
    __syncthreads();
}

// one workgroup, q <= LOGIT_WG_MAX: u = A beta_prev + XY, next_beta, stopRule -- until the rule or maxit; st[ST_ITERS] += iterations
// (the body of logit_inner_kernel and, with one workgroup per response, of logit_inner_multi_kernel; iters: the word it adds its count to)
template <bool A_LDS>
__device__ __forceinline__ void logit_inner_solve(const double *__restrict__ A, const double *__restrict__ xy, double *__restrict__ beta, int q,
                                                  const LogitPen &P, int maxit, double tol, double *__restrict__ iters)
{
    extern __shared__ double sh[];
    double *bp = sh, *u = sh + q, *bn = sh + 2 * q, *gf = sh + 3 * q, *As = sh + 3 * q + (P.ngroups > 0 ? P.ngroups : 1);
    const int i = threadIdx.x;
    if (A_LDS) for (int k = i; k < q * q; k += 1024) As[k] = A[k];
    if (i < q) bp[i] = beta[i];
    const double xyi = i < q ? xy[i] : 0.0;
    int it = 0;
    for (int j = 0; j < maxit; ++j) {
        __syncthreads();
        if (i < q) {
            double a = 0.0;
            if (A_LDS) for (int k = 0; k < q; ++k) a = fma(As[k * q + i], bp[k], a);
            else for (int k = 0; k < q; ++k) a = fma(A[(size_t)k * q + i], bp[k], a);
            u[i] = a + xyi;
        }
        __syncthreads();
        logit_threshold(P, u, bn, q, gf);
        ++it;
        const int go = __syncthreads_or(i < q && stop_violated(bn[i], bp[i], tol));
        if (i < q) bp[i] = bn[i];
        if (!go) break;
    }
    __syncthreads();
    if (i < q) beta[i] = bp[i];
    if (i == 0) *iters += (double)it;
}

template <bool A_LDS>
__global__ __launch_bounds__(1024) void logit_inner_kernel(const double *__restrict__ A, const double *__restrict__ xy, double *__restrict__ beta,
                                                           int q, LogitPen P, int maxit, double tol, double *__restrict__ st)
{
    logit_inner_solve<A_LDS>(A, xy, beta, q, P, maxit, tol, st + ST_ITERS);
}

// ---------------------------------------------------------------------------------------------------------------- many responses
// logistic_irls_multi's small kernels: workgroup (or grid row) r is response r of the lock-step chunk -- its q entries of beta, xy,
// beta_irls, its p + 2 of g, its PenK (its own lambda), its live word.  A frozen response (live[r] == 0) is skipped by every one.
// grp[r] is the GROUP of instance r: the fold it leaves out decides its s, XX, A and its number of rows nv[grp[r]],
// which lie group after group (p, q q, q q doubles and one double each); the plain call has the one group 0.
template <bool A_LDS>
__global__ __launch_bounds__(1024) void logit_inner_multi_kernel(const double *__restrict__ A, const double *__restrict__ xy, double *__restrict__ beta,
                                                                 int q, LogitPen P, const PenK *__restrict__ pk, int maxit, double tol,
                                                                 const int *__restrict__ live, const int *__restrict__ grp, double *__restrict__ iters)
{
    const int r = blockIdx.x;
    if (!live[r]) return;
    P.k = pk[r];
    logit_inner_solve<A_LDS>(A + (size_t)grp[r] * q * q, xy + (size_t)r * q, beta + (size_t)r * q, q, P, maxit, tol, iters + r);
}

// logit_xy_kernel for response blockIdx.y
__global__ __launch_bounds__(256) void logit_xy_multi_kernel(const double *__restrict__ xx, const double *__restrict__ beta, const double *__restrict__ g,
                                                             const double *__restrict__ s, int p, int intercept, const double *__restrict__ nv, int init,
                                                             const int *__restrict__ live, const int *__restrict__ grp, double *__restrict__ xy)
{
    const int q = p + (intercept ? 1 : 0), r = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= q || !live[r]) return;
    const int gi = grp[r];
    const double n = nv[gi];
    xx += (size_t)gi * q * q; s += (size_t)gi * p;
    beta += (size_t)r * q; g += (size_t)r * (p + 2); xy += (size_t)r * q;
    const bool icpt = intercept && i == 0;
    const int j = i - (intercept ? 1 : 0);
    if (init) { xy[i] = icpt ? g[0] / n : (g[1 + j] * s[j]) / n; return; }
    const double gr = icpt ? g[0] / n : (g[1 + j] / n) * s[j];
    double a = 0.0;
    for (int k = 0; k < q; ++k) a = fma(xx[(size_t)k * q + i], beta[k], a);
    xy[i] = a + gr;
}

// the step's start for the live responses: beta_irls <- beta, and Bt = beta o s with the intercept's entry as it is (the row pass reads it)
__global__ __launch_bounds__(256) void logit_step_multi_kernel(const double *__restrict__ beta, const double *__restrict__ s, int q, int intercept,
                                                               const int *__restrict__ live, const int *__restrict__ grp, double *__restrict__ birls,
                                                               double *__restrict__ bt)
{
    const int r = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= q || !live[r]) return;
    const size_t e = (size_t)r * q + i;
    const double b = beta[e];
    birls[e] = b;
    bt[e] = (intercept && i == 0) ? b : b * s[(size_t)grp[r] * (q - (intercept ? 1 : 0)) + i - (intercept ? 1 : 0)];
}

// IRLS stop of response blockIdx.x: stopw[r] = stopRule(beta, beta_irls, irls_tol); a response that stops is frozen here (live[r] = 0)
__global__ __launch_bounds__(1024) void logit_irls_stop_multi_kernel(const double *__restrict__ b, const double *__restrict__ bi, int q, double tol,
                                                                     int *__restrict__ live, int *__restrict__ stopw)
{
    const int r = blockIdx.x;
    if (!live[r]) return;                                                     // (uniform: the word is written behind the barrier below)
    b += (size_t)r * q; bi += (size_t)r * q;
    int v = 0;
    for (int i = threadIdx.x; i < q; i += 1024) v |= stop_violated(b[i], bi[i], tol);
    const int viol = __syncthreads_or(v);
    if (threadIdx.x == 0) { stopw[r] = viol ? 0 : 1; if (!viol) live[r] = 0; }
}

// logit_back_kernel for response blockIdx.y into its slot of bout; lossw[r] = the loss of its last own row pass
__global__ __launch_bounds__(256) void logit_back_multi_kernel(const double *__restrict__ beta, const double *__restrict__ s, const double *__restrict__ g,
                                                               int p, int intercept, size_t stride, const int *__restrict__ grp, double *__restrict__ out,
                                                               double *__restrict__ lossw)
{
    const int r = blockIdx.y, q = p + (intercept ? 1 : 0);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > p) return;
    beta += (size_t)r * q; out += (size_t)r * stride; s += (size_t)grp[r] * p;
    if (i == 0) { out[0] = intercept ? beta[0] : 0.0; lossw[r] = g[(size_t)r * (p + 2) + p + 1]; return; }
    out[i] = beta[(intercept ? 1 : 0) + i - 1] * s[i - 1];
}

__global__ void logit_fill_int_kernel(int *a, int n, int v)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = v;
}

// launch form, after launch_gemv(A, beta_prev) -> u: u += XY, next_beta, stopRule; beta_prev <- beta; stop word set on convergence.
// LDS: scratch [us | bn | gf] in dynamic LDS; else in gws (2 q + ngroups doubles of the workspace)
template <bool LDS>
__global__ __launch_bounds__(1024) void logit_thresh_kernel(double *__restrict__ u, const double *__restrict__ xy, double *__restrict__ bp,
                                                            int q, LogitPen P, double tol, int maxit, int *__restrict__ done, double *__restrict__ st,
                                                            double *__restrict__ gws)
{
    extern __shared__ double sh[];
    double *const base = LDS ? sh : gws;
    double *us = base, *bn = base + q, *gf = base + 2 * q;
    if (*done) return;
    const int tid = threadIdx.x;
    for (int i = tid; i < q; i += 1024) us[i] = u[i] + xy[i];
    __syncthreads();
    logit_threshold(P, us, bn, q, gf);
    int v = 0;
    for (int i = tid; i < q; i += 1024) v |= stop_violated(bn[i], bp[i], tol);
    const int viol = __syncthreads_or(v);
    for (int i = tid; i < q; i += 1024) bp[i] = bn[i];
    if (tid == 0) {
        st[ST_ITERS] += 1.0;
        const int it = (int)st[ST_DONE] + 1;
        st[ST_DONE] = it;
        if (!viol || it >= maxit) *done = 1;
    }
}

// IRLS stop: st[ST_IRLS_STOP] = stopRule(beta, beta_irls, irls_tol)
__global__ __launch_bounds__(1024) void logit_irls_stop_kernel(const double *__restrict__ b, const double *__restrict__ bi, int q, double tol,
                                                               double *__restrict__ st)
{
    int v = 0;
    for (int i = threadIdx.x; i < q; i += 1024) v |= stop_violated(b[i], bi[i], tol);
    const int viol = __syncthreads_or(v);
    if (threadIdx.x == 0) st[ST_IRLS_STOP] = viol ? 0.0 : 1.0;
}

// get_beta (h :1038-1055): beta_j s_j on the original scale, the intercept as it is; row 0 = 0 without one
__global__ __launch_bounds__(256) void logit_back_kernel(const double *__restrict__ beta, const double *__restrict__ s, int p, int intercept,
                                                         double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > p) return;
    if (i == 0) { out[0] = intercept ? beta[0] : 0.0; return; }
    out[i] = beta[(intercept ? 1 : 0) + i - 1] * s[i - 1];
}

// colsq = sum x^2 / (n - 1), 0 -> 1, s = 1 / sqrt(colsq) (h :734-737); one workgroup per column, rank-order sum.  A fold fit (foldid
// not null): the sum over the kept rows, n_eff of them
__global__ __launch_bounds__(256) void logit_scale_kernel(const double *__restrict__ x, int64_t n, int64_t ld, double *__restrict__ s,
                                                          const int32_t *__restrict__ foldid, int32_t leave_out, int64_t n_eff)
{
    __shared__ double red[256];
    const int j = blockIdx.x;
    const double *col = x + (size_t)j * ld;
    double a = 0.0;
    if (foldid) {
        for (int64_t i = threadIdx.x; i < n; i += 256)
            if (foldid[i] != leave_out) a = fma(col[i], col[i], a);
    } else {
        for (int64_t i = threadIdx.x; i < n; i += 256) a = fma(col[i], col[i], a);
    }
    red[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < 256; ++k) t += red[k];
        double cs = t / ((double)n_eff - 1.0);
        if (cs == 0.0) cs = 1.0;
        s[j] = 1.0 / sqrt(cs);
    }
}

__global__ void logit_fill_kernel(double *a, int n, double v)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = v;
}

// A fold fit's look at foldid, once per call, by ONE workgroup: out[0] = n_eff (rows with foldid != leave_out), out[1] = rows whose id
// is outside [1, nfolds], out[2 + k] = the row of the k-th kept row for k < nmap (the W floor tests the IRLS index among the kept rows).
__global__ __launch_bounds__(1024) void logit_fold_scan_kernel(const int32_t *__restrict__ foldid, int64_t n, int32_t nfolds, int32_t leave_out,
                                                               int64_t nmap, int64_t *__restrict__ out)
{
    __shared__ long long cnt[1024], bad[1024];
    __shared__ int wcount[16];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    long long k = 0, b = 0;
    for (int64_t i = tid; i < n; i += 1024) {
        const int32_t f = foldid[i];
        k += f != leave_out;
        b += f < 1 || f > nfolds;
    }
    cnt[tid] = k; bad[tid] = b;
    __syncthreads();
    if (tid == 0) {
        long long a = 0, c = 0;
        for (int i = 0; i < 1024; ++i) { a += cnt[i]; c += bad[i]; }
        out[0] = a; out[1] = c;
    }
    int64_t base = 0;                                // kept rows before this tile of 1024 rows
    for (int64_t r0 = 0; r0 < n && base < nmap; r0 += 1024) {
        const int64_t row = r0 + tid;
        const bool kept = row < n && foldid[row] != leave_out;
        const unsigned long long m = __ballot(kept);
        if (lane == 0) wcount[w] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int i = 0; i < 16; ++i) { before += i < w ? wcount[i] : 0; total += wcount[i]; }
        const int64_t pos = base + before + __popcll(m & ((1ull << lane) - 1ull));
        if (kept && pos < nmap) out[2 + pos] = row;
        base += total;
        __syncthreads();
    }
}

}  // namespace

int launch_logit_fill(hipStream_t s, double *a, int n, double v)
{
    hipLaunchKernelGGL(logit_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, n, v);
    OEM_HIP(hipGetLastError());
    return 0;
}

int logit_fold_scan(oemgpu_ctx *c, const char *who, const int32_t *foldid, int64_t n, int32_t nfolds, int32_t leave_out, int32_t irls_maxit,
                    int64_t *n_eff, std::vector<int64_t> *kept_row)
{
    const int64_t nmap = std::min<int64_t>(irls_maxit, n);
    if (ctx_reserve(c, 8 * (size_t)(2 + nmap))) return OEMGPU_ERR_HIP;
    int64_t *scan = (int64_t *)c->ws;
    hipLaunchKernelGGL(logit_fold_scan_kernel, dim3(1), dim3(1024), 0, c->stream, foldid, n, nfolds, leave_out, nmap, scan);
    OEM_HIP(hipGetLastError());
    std::vector<int64_t> h((size_t)(2 + nmap), -1);
    OEM_HIP(hipMemcpyAsync(h.data(), scan, 8 * 2, hipMemcpyDeviceToHost, c->stream));
    OEM_HIP(hipStreamSynchronize(c->stream));
    if (h[1] != 0) { set_error("%s: %lld fold ids are outside [1, %d]", who, (long long)h[1], (int)nfolds); return OEMGPU_ERR_ARG; }
    const int64_t nk = std::min<int64_t>(nmap, h[0]);
    if (nk > 0) OEM_HIP(hipMemcpy(h.data() + 2, scan + 2, 8 * (size_t)nk, hipMemcpyDeviceToHost));
    *n_eff = h[0];
    kept_row->assign(h.begin() + 2, h.begin() + 2 + nk);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host driver
struct LogitStats {
    double ms_rows = 0, ms_gram = 0, ms_inner = 0, irls_steps = 0, inner_iters = 0, row_passes = 0, grams = 0, wall_ms = 0;
};
static thread_local LogitStats g_logit_stats;

const int LOGIT_WG_MAX_Q = LOGIT_WG_MAX;
const int LOGIT_P_LIMIT = LOGIT_P_MAX;

template <bool STAGED, bool MASKED>
static int logit_rows_launch(hipStream_t s, const LogitPlan &P, size_t lds, const double *x, int64_t n, int64_t ld, int p, const double *y,
                             const double *beta, const double *sc, int intercept, int mode, int64_t irls_i, int64_t c0, int64_t nc, int64_t row0,
                             double *z, int64_t ldz, double *part, const int32_t *foldid, int32_t leave_out)
{
    if (lds_limit_once(reinterpret_cast<const void *>(&logit_rows_kernel<STAGED, MASKED>), lds)) return OEMGPU_ERR_HIP;
    hipLaunchKernelGGL((logit_rows_kernel<STAGED, MASKED>), dim3((unsigned)nc), dim3(256), lds, s, x, n, ld, p, y, beta, sc, intercept, mode, irls_i,
                       P.ch, c0, row0, z, ldz, part, foldid, leave_out);
    OEM_HIP(hipGetLastError());
    return 0;
}

// foldid null: the fit on every row; else the fold fit that leaves out the rows of fold leave_out
static int logit_rows(hipStream_t s, const LogitPlan &P, const double *x, int64_t n, int64_t ld, int p, const double *y, const double *beta,
                      const double *sc, int intercept, int mode, int64_t irls_i, int64_t c0, int64_t nc, int64_t row0, double *z, int64_t ldz, double *part,
                      const int32_t *foldid, int32_t leave_out)
{
    const size_t lds = 8 * (size_t)p + (P.staged ? 8 * 65 * (size_t)p : 0);
    if (foldid)
        return P.staged ? logit_rows_launch<true, true>(s, P, lds, x, n, ld, p, y, beta, sc, intercept, mode, irls_i, c0, nc, row0, z, ldz, part, foldid, leave_out)
                        : logit_rows_launch<false, true>(s, P, lds, x, n, ld, p, y, beta, sc, intercept, mode, irls_i, c0, nc, row0, z, ldz, part, foldid, leave_out);
    return P.staged ? logit_rows_launch<true, false>(s, P, lds, x, n, ld, p, y, beta, sc, intercept, mode, irls_i, c0, nc, row0, z, ldz, part, nullptr, 0)
                    : logit_rows_launch<false, false>(s, P, lds, x, n, ld, p, y, beta, sc, intercept, mode, irls_i, c0, nc, row0, z, ldz, part, nullptr, 0);
}

// checks that need no device: -1 / -4 before any device is looked for
int logistic_check(int64_t n, int32_t p, int32_t intercept, int32_t hessian_full, int32_t irls_maxit, double irls_tol, const oemgpu_opts *o)
{
    const int q = p + (intercept ? 1 : 0);
    int rc = check_opts_export(o, p, q);
    if (rc) return rc;
    if (n < 1) { set_error("fit_logistic_dense: bad n"); return OEMGPU_ERR_ARG; }
    if (hessian_full != 0 && hessian_full != 1) { set_error("hessian.type must be \"upper.bound\" (0) or \"full\" (1)"); return OEMGPU_ERR_ARG; }
    if (irls_maxit <= 0) { set_error("maxit and irls.maxit should be positive"); return OEMGPU_ERR_ARG; }       // ref R/oem.R:427-430
    if (!(irls_tol >= 0.0)) { set_error("tol and irls.tol should be nonnegative"); return OEMGPU_ERR_ARG; }
    if ((int64_t)q >= n) {
        set_error("fit_logistic_dense: p + intercept >= n is not supported (the reference's XWXt branch iterates on the raw labels, "
                  "ref src/oem_logistic_dense.h:524-566)");
        return OEMGPU_ERR_UNSUPPORTED;
    }
    if (p > LOGIT_P_MAX) { set_error("fit_logistic_dense: p > %d is not supported", LOGIT_P_MAX); return OEMGPU_ERR_UNSUPPORTED; }
    return 0;
}

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- what logistic_irls and logistic_irls_multi share on the host
// penalty factors (0 for the intercept), groups ordered, group weights (default sqrt(size), 0 for group 0)
struct LogitTables {
    std::vector<double> pf, gw;
    std::vector<int> perm, gstart, gof, gzero;
    int ng = 0, nperm = 0;
    int build(const oemgpu_opts *o, int p, int intercept)
    {
        const int o1 = intercept ? 1 : 0, q = p + o1;
        pf.assign(q, 0.0);
        for (int j = 0; j < p; ++j) pf[o1 + j] = o->penalty_factor[j];
        if (intercept) pf[0] = 0.0;
        bool any_grp = false;
        for (int k = 0; k < o->npen; ++k) any_grp |= pen_is_grp(o->penalty[k]);
        ng = any_grp ? o->ngroups : 0;
        perm.clear(); gstart.assign(ng + 1, 0); gof.assign(q, -1); gzero.assign(ng > 0 ? ng : 1, 0);
        gw.assign(ng > 0 ? ng : 1, 0.0);
        if (any_grp) {
            for (int g = 0; g < ng; ++g) {                       // get_group_indexes (h :397-439)
                gstart[g] = (int)perm.size();
                for (int v = 0; v < q; ++v)
                    if (o->groups[v] == o->unique_groups[g]) { perm.push_back(v); if (gof[v] < 0) gof[v] = g; }
                gstart[g + 1] = (int)perm.size();
                gzero[g] = o->unique_groups[g] == 0;
                gw[g] = o->n_group_weights > 0 ? o->group_weights[g] : (gzero[g] ? 0.0 : std::sqrt((double)(gstart[g + 1] - gstart[g])));
            }
        }
        nperm = (int)perm.size();
        if (nperm > q) { set_error("fit_logistic_dense: unique_groups has repeated ids"); return OEMGPU_ERR_ARG; }
        return 0;
    }
};

// cpp :164-171: exp(linspace(log lmax, log lmin))
static void logit_lambda_base(const oemgpu_opts *o, double lmax, int nl, double *base)
{
    const double lmin = o->lambda_min_ratio * lmax, a = std::log(lmax), b = std::log(lmin);
    for (int i = 0; i < nl; ++i) base[i] = std::exp(nl > 1 ? (i == nl - 1 ? b : a + (b - a) / (double)(nl - 1) * (double)i) : a);
}

// the lambda row of penalty k (cpp :205-225): the user's, or the base grid with the .net and nonconvex factors
static void logit_lambda_row(const oemgpu_opts *o, int k, bool provided, const std::vector<double> &base, int nl, double *lam)
{
    if (provided) { for (int i = 0; i < nl; ++i) lam[i] = o->lambda_user[(size_t)k * nl + i]; return; }
    const int pen = o->penalty[k];
    const bool net = pen_is_net(pen), ncv = pen == OEMGPU_MCP || pen == OEMGPU_SCAD || pen == OEMGPU_MCP_NET || pen == OEMGPU_SCAD_NET ||
                                            pen == OEMGPU_GRP_MCP || pen == OEMGPU_GRP_SCAD || pen == OEMGPU_GRP_MCP_NET || pen == OEMGPU_GRP_SCAD_NET;
    for (int i = 0; i < nl; ++i) {
        lam[i] = base[i];
        if (net) {
            lam[i] = base[i] / o->alpha;
            if (ncv) {
                const double fact = 3.5 - std::fmin(3.5, o->gamma) * 5.71425 / 8.0;
                lam[i] = fact * base[i] / std::pow(o->alpha, 0.8);
            }
        }
    }
}

// next_beta's constants of a penalty at lambda lamv (h :569-672)
static PenK logit_penk(const oemgpu_opts *o, int pen, double lamv, double d)
{
    PenK pk;
    const double al = o->alpha, ta = o->tau;
    pk.gamma = o->gamma; pk.L1 = 0.0; pk.L = lamv; pk.D = d; pk.kind = K_SOFT;
    const double Ln = lamv * al, Dn = d + (1.0 - al) * lamv;
    switch (pen) {
    case OEMGPU_LASSO: break;
    case OEMGPU_OLS: pk.kind = K_OLS; break;
    case OEMGPU_ELASTIC_NET: pk.L = Ln; pk.D = Dn; break;
    case OEMGPU_SCAD: pk.kind = K_SCAD; break;
    case OEMGPU_SCAD_NET: pk.kind = K_SCAD; pk.L = Ln; pk.D = Dn; if (al == 0.0) { pk.L = 0.0; pk.D = d + lamv; } break;
    case OEMGPU_MCP: pk.kind = K_MCP; break;
    case OEMGPU_MCP_NET: pk.kind = K_MCP; pk.L = Ln; pk.D = Dn; break;
    case OEMGPU_GRP_LASSO: pk.kind = K_GRP; break;
    case OEMGPU_GRP_LASSO_NET: pk.kind = K_GRP; pk.L = Ln; pk.D = Dn; break;
    case OEMGPU_GRP_MCP: pk.kind = K_GRP_MCP; break;
    case OEMGPU_GRP_SCAD: pk.kind = K_GRP_SCAD; break;
    case OEMGPU_GRP_MCP_NET: pk.kind = K_GRP_MCP; pk.L = Ln; pk.D = Dn; break;
    case OEMGPU_GRP_SCAD_NET: pk.kind = K_GRP_SCAD; pk.L = Ln; pk.D = Dn; break;
    case OEMGPU_SPARSE_GRP_LASSO: pk.kind = K_SGL; pk.L = (1.0 - ta) * lamv; pk.L1 = ta * lamv; break;
    default: break;
    }
    return pk;
}

namespace {

// the dense x: one row pass per IRLS step (logit_rows_kernel); with a Hessian due the same pass writes the Z row blocks of the
// moment pass instead, block after block.  With foldid / leave_out it is the data of the fit on the rows with foldid[row] != leave_out:
// X and y stay where they are, the passes leave those rows out, and n_eff (the kept rows) stands where n enters the arithmetic.
struct DenseLogitData final : LogitData {
    oemgpu_ctx *c;
    DenseSrc X;
    const double *y;
    int64_t n;
    int p, q, intercept, standardize;
    LogitPlan P;
    LogitRmPlan R;                    // a row-major x: the band plan of its row pass
    size_t m2;
    double *part = nullptr, *z = nullptr, *mb = nullptr, *ma = nullptr, *tp = nullptr, *vp = nullptr;
    double *sp = nullptr;             // a row-major x: the scale pass's 256 partials per column
    const int32_t *foldid = nullptr;  // device, n entries; null: every row is in the fit
    int32_t leave_out = 0;
    int64_t n_eff;                    // rows in the fit
    std::vector<int64_t> kept_row;    // fold fit: the row of the k-th kept row, k < min(irls_maxit, n_eff)

    // The row whose W the floor tests at IRLS step i (h :953-959 tests W(i) of the rows it was given)
    int64_t floor_row(int64_t i) const { return foldid ? (i < (int64_t)kept_row.size() ? kept_row[(size_t)i] : -1) : i; }
    // Makes this the fold fit without fold leave_out_: counts n_eff, checks the ids' range and maps the first IRLS indices to rows, on
    // the device, once (logit_fold_scan)
    int set_fold(const int32_t *foldid_, int32_t nfolds, int32_t leave_out_, int32_t irls_maxit)
    {
        const int rc = logit_fold_scan(c, "fit_logistic_dense_fold", foldid_, n, nfolds, leave_out_, irls_maxit, &n_eff, &kept_row);
        if (rc) return rc;
        foldid = foldid_; leave_out = leave_out_;
        return 0;
    }

    DenseLogitData(oemgpu_ctx *c_, const DenseSrc &X_, int64_t n_, int p_, const double *y_, int standardize_, int intercept_, int hessian_full)
        : c(c_), X(X_), y(y_), n(n_), p(p_), q(p_ + (intercept_ ? 1 : 0)), intercept(intercept_), standardize(standardize_),
          P(logit_plan(n_, p_, intercept_, c_->num_cu)), R(X_.colmajor() ? LogitRmPlan{} : logit_rm_plan(p_)), m2((size_t)(q + 2) * (q + 2)), n_eff(n_)
    {
        hess_every = hessian_full != 0;
    }
    bool wants_sp() const { return !X.colmajor() && standardize; }
    size_t ws_bytes() const override
    {
        Bump B;
        const GramPlan gpb = gram_plan_bound(P.rbz < n ? P.rbz : n, q, c->num_cu);
        B.take(8 * (size_t)P.nchunk * (p + 2)); B.take(8 * (size_t)P.rbz * q); B.take(8 * m2); B.take(8 * m2);
        B.take(8 * gpb.tpart_doubles); B.take(8 * gpb.vpart_doubles);
        if (wants_sp()) B.take(8 * (size_t)256 * p);
        return B.off;
    }
    int bind(char *ws) override
    {
        Bump B;
        const GramPlan gpb = gram_plan_bound(P.rbz < n ? P.rbz : n, q, c->num_cu);
        part = (double *)(ws + B.take(8 * (size_t)P.nchunk * (p + 2))); z = (double *)(ws + B.take(8 * (size_t)P.rbz * q));
        mb = (double *)(ws + B.take(8 * m2)); ma = (double *)(ws + B.take(8 * m2));
        tp = (double *)(ws + B.take(8 * gpb.tpart_doubles)); vp = (double *)(ws + B.take(8 * gpb.vpart_doubles));
        if (wants_sp()) sp = (double *)(ws + B.take(8 * (size_t)256 * p));
        return 0;
    }
    int scale(double *sc) override
    {
        if (!standardize) return launch_logit_fill(c->stream, sc, p, 1.0);
        if (!X.colmajor()) return launch_logit_scale_rm(c->stream, X.x, X.dtype, n, X.ld, p, sp, sc, foldid, leave_out, n_eff, foldid ? kept_row[0] : 0);
        hipLaunchKernelGGL(logit_scale_kernel, dim3(p), dim3(256), 0, c->stream, X.cm(), n, X.ld, sc, foldid, leave_out, n_eff);
        OEM_HIP(hipGetLastError());
        return 0;
    }
    // the row pass over chunks c0 .. c0 + nc (logit_rows_kernel, either reader): the one place that reads x besides scale()
    int rows_launch(const double *beta, const double *sc, int mode, int64_t irls_row, int64_t c0, int64_t nc, int64_t row0, double *zb, int64_t ldz)
    {
        if (X.colmajor()) return logit_rows(c->stream, P, X.cm(), n, X.ld, p, y, beta, sc, intercept, mode, irls_row, c0, nc, row0, zb, ldz, part, foldid, leave_out);
        return launch_logit_rows_rm(c->stream, R, X.x, X.dtype, n, X.ld, p, y, beta, sc, intercept, mode, irls_row, P.ch, c0, nc, row0, zb, ldz, part, foldid,
                                    leave_out);
    }
    int xy0(const double *sc, double *g) override
    {
        int rc = rows_launch(nullptr, sc, 0, -1, 0, P.nchunk, 0, nullptr, 0);
        if (rc) return rc;
        hipLaunchKernelGGL(logit_sum_kernel, dim3((p + 2 + 255) / 256), dim3(256), 0, c->stream, part, P.nchunk, p + 2, g);
        OEM_HIP(hipGetLastError());
        return 0;
    }
    int rows(const double *beta, const double *sc, int64_t i, bool gram, double *g) override
    {
        if (gram) return 0;                                  // the Z blocks of the Hessian build carry the row pass
        int rc = rows_launch(beta, sc, 1, floor_row(i), 0, P.nchunk, 0, nullptr, 0);
        if (rc) return rc;
        hipLaunchKernelGGL(logit_sum_kernel, dim3((p + 2 + 255) / 256), dim3(256), 0, c->stream, part, P.nchunk, p + 2, g);
        OEM_HIP(hipGetLastError());
        return 0;
    }
    int hessian(const double *beta, const double *sc, int64_t i, double *g, double *xx) override
    {
        hipStream_t s = c->stream;
        // Z row blocks: row pass (writes Z and the partials of its chunks) -> moment pass -> running sum in block order
        for (int64_t b = 0; b < P.nzblk; ++b) {
            const int64_t c0 = b * (P.rbz / P.ch), c1 = std::min<int64_t>(P.nchunk, c0 + P.rbz / P.ch);
            const int64_t r0 = c0 * P.ch, nrow = std::min<int64_t>(n, c1 * P.ch) - r0;
            int r = rows_launch(beta, sc, 1, floor_row(i), c0, c1 - c0, r0, z, P.rbz);
            if (r) return r;
            const GramPlan gpl = gram_plan(nrow, q, c->num_cu);
            r = launch_gram(s, gpl, z, nrow, P.rbz, z, nullptr, tp, vp);
            if (!r) r = launch_moments_reduce(s, gpl, tp, vp, mb);
            if (!r) r = launch_moments_add(s, ma, mb, m2, b == 0);
            if (r) return r;
        }
        hipLaunchKernelGGL(logit_xx_kernel, dim3((q + 255) / 256, q), dim3(256), 0, s, ma, q, (double)n_eff, xx);
        hipLaunchKernelGGL(logit_sum_kernel, dim3((p + 2 + 255) / 256), dim3(256), 0, s, part, P.nchunk, p + 2, g);
        OEM_HIP(hipGetLastError());
        return 0;
    }
};

// get_beta of the sparse fit (ref src/oem_logistic_sparse.h:1040-1062): beta_0 *= intval on the solver's own beta
__global__ void logit_rescale_kernel(double *beta, const double *intval) { beta[0] *= *intval; }

}  // namespace

int logistic_irls(oemgpu_ctx *c, LogitData &D, int64_t n, int32_t p, int32_t intercept, int32_t irls_maxit, double irls_tol, const oemgpu_opts *o,
                  double *beta_out, double *lambda_out, int32_t *niter, double *loss_out, double *d_out)
{
    const double t_start = now_ms();
    g_logit_stats = LogitStats();
    const int q = p + (intercept ? 1 : 0), o1 = intercept ? 1 : 0;
    const int nl = (o->lambda_user && o->nlambda_user > 0) ? o->nlambda_user : o->nlambda;
    const bool provided = o->lambda_user && o->nlambda_user > 0;
    const bool inner_wg = q <= LOGIT_WG_MAX;
    LogitTables T;
    if (int trc = T.build(o, p, intercept)) return trc;
    const std::vector<double> &pf = T.pf, &gw = T.gw;
    const std::vector<int> &perm = T.perm, &gstart = T.gstart, &gof = T.gof, &gzero = T.gzero;
    const int ng = T.ng, nperm = T.nperm;
    // ---- workspace (c->aux; oemgpu_eig_max_dev takes c->ws from its start): the driver's pieces, then the data stages'
    Bump B;
    const size_t a_s = B.take(8 * (size_t)p), a_b = B.take(8 * (size_t)q), a_bi = B.take(8 * (size_t)q),
                 a_u = B.take(8 * (size_t)q), a_xy = B.take(8 * (size_t)q), a_xx = B.take(8 * (size_t)q * q), a_a = B.take(8 * (size_t)q * q),
                 a_g = B.take(8 * (size_t)(p + 2));
    const size_t a_st = B.take(8 * ST_LEN), a_done = B.take(256);
    const size_t a_pf = B.take(8 * (size_t)q), a_gw = B.take(8 * (size_t)(ng > 0 ? ng : 1)), a_perm = B.take(4 * (size_t)(q + 1)),
                 a_gs = B.take(4 * (size_t)(ng + 1)), a_gof = B.take(4 * (size_t)q), a_gz = B.take(4 * (size_t)(ng > 0 ? ng : 1));
    const bool thr_lds = logit_thr_in_lds(q, ng);
    const size_t a_thr = (!inner_wg && !thr_lds) ? B.take(8 * (size_t)(2 * q + (ng > 0 ? ng : 1))) : 0;
    const size_t a_out = B.take(8 * (size_t)o->npen * nl * (p + 1));
    const size_t a_data = B.take(D.ws_bytes());
    ctx_void_cv(c);
    if (ctx_grow(c, &c->aux, &c->aux_bytes, B.off)) return OEMGPU_ERR_HIP;
    char *W = c->aux;
    double *sc = (double *)(W + a_s), *beta = (double *)(W + a_b), *birls = (double *)(W + a_bi), *u = (double *)(W + a_u),
           *xy = (double *)(W + a_xy), *xx = (double *)(W + a_xx), *A = (double *)(W + a_a), *g = (double *)(W + a_g), *st = (double *)(W + a_st),
           *bout = (double *)(W + a_out);
    int *done = (int *)(W + a_done);
    hipStream_t s = c->stream;
    int rc = D.bind(W + a_data);
    if (rc) return rc;
    OEM_HIP(hipMemcpyAsync(W + a_pf, pf.data(), 8 * (size_t)q, hipMemcpyHostToDevice, s));
    OEM_HIP(hipMemcpyAsync(W + a_gw, gw.data(), 8 * gw.size(), hipMemcpyHostToDevice, s));
    if (nperm) OEM_HIP(hipMemcpyAsync(W + a_perm, perm.data(), 4 * (size_t)nperm, hipMemcpyHostToDevice, s));
    OEM_HIP(hipMemcpyAsync(W + a_gs, gstart.data(), 4 * gstart.size(), hipMemcpyHostToDevice, s));
    OEM_HIP(hipMemcpyAsync(W + a_gof, gof.data(), 4 * (size_t)q, hipMemcpyHostToDevice, s));
    OEM_HIP(hipMemcpyAsync(W + a_gz, gzero.data(), 4 * gzero.size(), hipMemcpyHostToDevice, s));
    OEM_HIP(hipMemsetAsync(bout, 0, 8 * (size_t)o->npen * nl * (p + 1), s));
    OEM_HIP(hipMemsetAsync(st, 0, 8 * ST_LEN, s));
    // ---- init_oem: s, XY = s o X'Y / n, lambda_0
    rc = D.scale(sc);
    if (!rc) rc = D.xy0(sc, g);
    if (rc) return rc;
    hipLaunchKernelGGL(logit_xy_kernel, dim3((q + 255) / 256), dim3(256), 0, s, xx, beta, g, sc, p, intercept, (double)n, 1, xy);
    OEM_HIP(hipGetLastError());
    std::vector<double> hxy(q);
    OEM_HIP(hipMemcpyAsync(hxy.data(), xy, 8 * (size_t)q, hipMemcpyDeviceToHost, s));
    OEM_HIP(hipStreamSynchronize(s));
    double lmax = 0.0;
    for (int j = o1; j < q; ++j) lmax = std::fmax(lmax, std::fabs(hxy[j]));       // h :795-805
    std::vector<double> base(nl);
    if (!provided) logit_lambda_base(o, lmax, nl, base.data());
    LogitPen LP;
    LP.pf = (const double *)(W + a_pf); LP.gw = (const double *)(W + a_gw); LP.perm = (const int *)(W + a_perm);
    LP.gstart = (const int *)(W + a_gs); LP.gof = (const int *)(W + a_gof); LP.gzero = (const int *)(W + a_gz); LP.ngroups = ng;
    double d = 0.0;
    std::vector<double> lam(nl);
    hipEvent_t ev[2];
    const bool timing = c->timing;
    if (timing) { OEM_HIP(hipEventCreate(&ev[0])); OEM_HIP(hipEventCreate(&ev[1])); }
    auto stage = [&](double *acc, auto &&fn) -> int {
        if (timing) (void)hipEventRecord(ev[0], s);
        int r = fn();
        if (r) return r;
        if (timing) {
            (void)hipEventRecord(ev[1], s);
            if (hipEventSynchronize(ev[1]) != hipSuccess) { set_error("hipEventSynchronize failed"); return OEMGPU_ERR_HIP; }
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
            *acc += ms;
        }
        return 0;
    };
    int interrupted = 0;
    for (int k = 0; k < o->npen && !rc && !interrupted; ++k) {
        const int pen = o->penalty[k];
        const bool is_ols = pen == OEMGPU_OLS;
        const int nlk = is_ols ? 1 : nl;
        // the lambda row of this penalty (cpp :205-225)
        logit_lambda_row(o, k, provided, base, nl, lam.data());
        for (int i = 0; i < nl; ++i) lambda_out[(size_t)k * nl + i] = lam[i];
        OEM_HIP(hipMemsetAsync(beta, 0, 8 * (size_t)q, s));                        // init(): cold start (h :813)
        for (int li = 0; li < nlk && !rc && !interrupted; ++li) {
            int i;
            double loss_now = 1e99;
            for (i = 0; i < irls_maxit; ++i) {
                if (o->interrupt && o->interrupt(o->interrupt_arg)) { interrupted = 1; break; }
                OEM_HIP(hipMemcpyAsync(birls, beta, 8 * (size_t)q, hipMemcpyDeviceToDevice, s));
                if (!(i == 0 && li > 0)) {
                    const bool need_xx = (i == 0 && li == 0) || D.hess_every;
                    rc = stage(&g_logit_stats.ms_rows, [&]() -> int { return D.rows(beta, sc, i, need_xx, g); });
                    if (rc) break;
                    if (need_xx) {
                        rc = stage(&g_logit_stats.ms_gram, [&]() -> int {
                            int r = D.hessian(beta, sc, i, g, xx);
                            if (r) return r;
                            double lm = 0.0;
                            r = oemgpu_eig_max_dev(c, xx, q, &lm);                   // (synchronises)
                            if (r) return r;
                            d = lm * 1.0005;                                         // h :514
                            hipLaunchKernelGGL(logit_a_kernel, dim3((q + 255) / 256, q), dim3(256), 0, s, xx, q, d, A);
                            OEM_HIP(hipGetLastError());
                            return 0;
                        });
                        if (rc) break;
                        g_logit_stats.grams += 1;
                    }
                    g_logit_stats.row_passes += 1;
                    hipLaunchKernelGGL(logit_xy_kernel, dim3((q + 255) / 256), dim3(256), 0, s, xx, beta, g, sc, p, intercept, (double)n, 0, xy);
                    OEM_HIP(hipGetLastError());
                }
                // the OEM loop at this lambda (h :1010-1022)
                LP.k = logit_penk(o, pen, lam[li], d);
                rc = stage(&g_logit_stats.ms_inner, [&]() -> int {
                    if (inner_wg) {
                        const bool alds = q <= LOGIT_A_LDS_Q;
                        const size_t lds = 8 * (size_t)(3 * q + (ng > 0 ? ng : 1) + (alds ? q * q : 0));
                        if (alds) {
                            if (lds_limit_once(reinterpret_cast<const void *>(&logit_inner_kernel<true>), lds)) return OEMGPU_ERR_HIP;
                            hipLaunchKernelGGL(logit_inner_kernel<true>, dim3(1), dim3(1024), lds, s, A, xy, beta, q, LP, o->maxit, o->tol, st);
                        } else {
                            if (lds_limit_once(reinterpret_cast<const void *>(&logit_inner_kernel<false>), lds)) return OEMGPU_ERR_HIP;
                            hipLaunchKernelGGL(logit_inner_kernel<false>, dim3(1), dim3(1024), lds, s, A, xy, beta, q, LP, o->maxit, o->tol, st);
                        }
                        OEM_HIP(hipGetLastError());
                        return 0;
                    }
                    // launch per iteration: beta is the loop's beta_prev (bp), u the product
                    OEM_HIP(hipMemsetAsync(done, 0, 4, s));
                    hipLaunchKernelGGL(logit_fill_kernel, dim3(1), dim3(256), 0, s, st + ST_DONE, 1, 0.0);
                    const size_t lds = thr_lds ? 8 * (size_t)(2 * q + (ng > 0 ? ng : 1)) : 0;
                    double *gws = thr_lds ? nullptr : (double *)(W + a_thr);
                    if (thr_lds && lds_limit_once(reinterpret_cast<const void *>(&logit_thresh_kernel<true>), lds)) return OEMGPU_ERR_HIP;
                    for (int j0 = 0; j0 < o->maxit; j0 += LOGIT_BATCH) {
                        const int nb = std::min(LOGIT_BATCH, o->maxit - j0);
                        for (int jj = 0; jj < nb; ++jj) {
                            int r = launch_gemv_sym(s, A, q, beta, u, done, c->num_cu);
                            if (r) return r;
                            if (thr_lds)
                                hipLaunchKernelGGL(logit_thresh_kernel<true>, dim3(1), dim3(1024), lds, s, u, xy, beta, q, LP, o->tol, o->maxit, done, st, gws);
                            else
                                hipLaunchKernelGGL(logit_thresh_kernel<false>, dim3(1), dim3(1024), 0, s, u, xy, beta, q, LP, o->tol, o->maxit, done, st, gws);
                        }
                        OEM_HIP(hipGetLastError());
                        int hd = 0;
                        OEM_HIP(hipMemcpyAsync(&hd, done, 4, hipMemcpyDeviceToHost, s));
                        OEM_HIP(hipStreamSynchronize(s));
                        if (hd) break;
                    }
                    return 0;
                });
                if (rc) break;
                hipLaunchKernelGGL(logit_irls_stop_kernel, dim3(1), dim3(1024), 0, s, beta, birls, q, irls_tol, st);
                OEM_HIP(hipGetLastError());
                double hst[ST_LEN];
                OEM_HIP(hipMemcpyAsync(hst, st, sizeof hst, hipMemcpyDeviceToHost, s));
                OEM_HIP(hipStreamSynchronize(s));                            // the one host sync of an IRLS step
                g_logit_stats.irls_steps += 1;
                if (hst[ST_IRLS_STOP] != 0.0) break;
            }
            if (rc || interrupted) break;
            // the loss of the LAST prob computed: the partials' last entry of the most recent row pass
            if (o->compute_loss) {
                double gl = 0.0;
                OEM_HIP(hipMemcpyAsync(&gl, g + p + 1, 8, hipMemcpyDeviceToHost, s));
                OEM_HIP(hipStreamSynchronize(s));
                loss_now = gl;
            }
            niter[(size_t)k * nl + li] = i + 1;
            loss_out[(size_t)k * nl + li] = loss_now;
            if (D.intval && intercept) hipLaunchKernelGGL(logit_rescale_kernel, dim3(1), dim3(1), 0, s, beta, D.intval);
            hipLaunchKernelGGL(logit_back_kernel, dim3((p + 1 + 255) / 256), dim3(256), 0, s, beta, sc, p, intercept, bout + ((size_t)k * nl + li) * (p + 1));
            OEM_HIP(hipGetLastError());
        }
        if (!rc && !interrupted) {
            for (int li = nlk; li < nl; ++li) { niter[(size_t)k * nl + li] = 0; loss_out[(size_t)k * nl + li] = 0.0; }
        }
    }
    if (timing) { (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]); }
    if (!rc && interrupted) { (void)hipStreamSynchronize(s); set_error("interrupted"); return OEMGPU_ERR_INTERRUPTED; }
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    OEM_HIP(hipMemcpyAsync(beta_out, bout, 8 * (size_t)o->npen * nl * (p + 1), hipMemcpyDeviceToHost, s));
    OEM_HIP(hipStreamSynchronize(s));
    double hst[ST_LEN];
    OEM_HIP(hipMemcpy(hst, st, sizeof hst, hipMemcpyDeviceToHost));
    g_logit_stats.inner_iters = hst[ST_ITERS];
    g_logit_stats.wall_ms = now_ms() - t_start;
    *d_out = d;
    return 0;
}

// The fit on a dense x wherever it lies; with foldid, on the rows with foldid[row] != leave_out (cv.oem's fold fit: what the dense fit
// computes on x[keep, ], y[keep]), refused when p + intercept >= the kept rows
static int logistic_fit_src(oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const double *y, const int32_t *foldid, int32_t nfolds,
                     int32_t leave_out, int32_t standardize, int32_t intercept, int32_t hessian_full, int32_t irls_maxit, double irls_tol,
                     const oemgpu_opts *o, double *beta_out, double *lambda_out, int32_t *niter, double *loss_out, double *d_out)
{
    DenseLogitData D(c, X, n, p, y, standardize, intercept, hessian_full);
    if (foldid) {
        const int rc = D.set_fold(foldid, nfolds, leave_out, irls_maxit);
        if (rc) return rc;
        if ((int64_t)D.q >= D.n_eff) {
            set_error("fit_logistic_dense_fold: p + intercept >= the %lld rows outside fold %d is not supported (the reference's XWXt branch, "
                      "ref src/oem_logistic_dense.h:524-566)", (long long)D.n_eff, (int)leave_out);
            return OEMGPU_ERR_UNSUPPORTED;
        }
    }
    return logistic_irls(c, D, D.n_eff, p, intercept, irls_maxit, irls_tol, o, beta_out, lambda_out, niter, loss_out, d_out);
}

// the checks of the four device entries (foldid_dev null: the plain fit), then the fit
static int logistic_fit_checked(const char *who, bool fold, oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const double *y_dev,
                                const int32_t *foldid_dev, int32_t nfolds, int32_t leave_out, int32_t standardize, int32_t intercept,
                                int32_t hessian_full, int32_t irls_maxit, double irls_tol, const oemgpu_opts *o,
                                double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    if (!c || !X.x || !y_dev || (fold && !foldid_dev) || !o || !beta || !lambda_out || !niter || !loss || !d) {
        set_error("%s: NULL argument", who);
        return OEMGPU_ERR_ARG;
    }
    if (fold) {
        if (nfolds < 3) { set_error("nfolds must be bigger than 3; nfolds=10 recommended"); return OEMGPU_ERR_ARG; }            // ref R/cv_oem.R:126-127
        if (leave_out < 0 || leave_out > nfolds) { set_error("%s: leave_out must be in [0, nfolds]", who); return OEMGPU_ERR_ARG; }
    }
    int rc = dense_src_check(who, X, n, p);
    if (!rc) rc = logistic_check(n, p, intercept, hessian_full, irls_maxit, irls_tol, o);
    if (rc) return rc;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    return logistic_fit_src(c, X, n, p, y_dev, foldid_dev, nfolds, leave_out, standardize, intercept, hessian_full, irls_maxit, irls_tol, o, beta,
                            lambda_out, niter, loss, d);
}

// ---------------------------------------------------------------------------------------------------------------- many responses on one x
struct LogitMultiStats {
    double steps = 0, row_passes = 0, blocks_skipped = 0, inner_iters = 0, grams = 0, lanczos = 0, ms_rows = 0, ms_gram = 0, ms_inner = 0, wall_ms = 0;
};
static thread_local LogitMultiStats g_lm_stats;

// response blocks of a row pass whose responses are all frozen (the kernel returns before it reads x)
static int lm_blocks_skipped(const LogitMultiPlan &pl, const std::vector<int> &live)
{
    int k = 0;
    for (int b = 0; b < pl.npass; ++b) {
        bool any = false;
        for (int r = b * pl.mb; r < pl.mc && r < (b + 1) * pl.mb; ++r) any |= live[(size_t)r] != 0;
        k += any ? 0 : 1;
    }
    return k;
}

// logistic_irls (hessian.type "upper.bound") for a list of INSTANCES in lock-step.  Instance i is response
// resp[i] of Y fitted on the rows with foldid != leave[i] (leave 0, or no foldid at all: every row); the plain many-response call is
// the list (r, 0), r < m.  With the upper bound the Hessian is built at beta = 0, where every W is 0.25 and the floor cannot bite: XX, d
// and A hold no y, only the rows kept, and the reference's rebuild at the start of every penalty returns the same matrix.  So, per
// distinct leave value (a GROUP): s, XX (DenseLogitData's own scale and Hessian passes, masked by set_fold as the single fold fit's,
// with response 0 riding as y), ONE Lanczos and A, once per call; then, per chunk of at most LMULTI_MCH instances, the X'Y pass and
// every instance's own lambda grid, and per penalty and lambda the IRLS steps of all its live instances from one row pass
// (logistic_multi.hip, masked per column), one inner launch (a workgroup per instance, on its group's A), one stop launch and ONE
// host read of the stop words.  An instance that meets the IRLS stop is frozen for the rest of the lambda: no kernel writes its beta,
// xy, g or Bt again, and its niter is that step's.  The skipped row pass at (i = 0, li > 0) holds for all at once: every instance
// solves at the new lambda on the xy of its last own pass.  No instance's result depends on the others or on the list's order.
// Outputs are indexed by instance; nobs (or null): the rows of its fit.
static int logistic_irls_multi(const char *who, oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const MultiY &Y, const int32_t *foldid, int32_t nfolds,
                               int32_t ninst, const int32_t *resp, const int32_t *leave, int32_t standardize, int32_t intercept, int32_t irls_maxit,
                               double irls_tol, const oemgpu_opts *o, double *beta_out, double *lambda_out, int32_t *niter, double *loss_out, double *d_out,
                               int64_t *nobs)
{
    const double t_start = now_ms();
    g_lm_stats = LogitMultiStats();
    const int m = ninst;
    const int q = p + (intercept ? 1 : 0), o1 = intercept ? 1 : 0;
    const bool provided = o->lambda_user && o->nlambda_user > 0;
    const int nl = provided ? o->nlambda_user : o->nlambda, npen = o->npen;
    LogitTables T;
    if (int trc = T.build(o, p, intercept)) return trc;
    const int ng = T.ng, ng1 = ng > 0 ? ng : 1;
    const int mch = m < LMULTI_MCH ? m : LMULTI_MCH;
    const LogitMultiPlan PW = logit_multi_plan(n, p, mch, c->num_cu);          // (the widest chunk: its panels bound every chunk's)
    // ---- the groups: the distinct leave values in ascending order; igrp[i]: instance i's
    std::vector<int> gleave, igrp((size_t)m, 0);
    if (foldid) {
        std::vector<int> of((size_t)nfolds + 1, -1);
        for (int i = 0; i < m; ++i) of[(size_t)leave[i]] = 0;
        for (int k = 0; k <= nfolds; ++k)
            if (of[(size_t)k] == 0) { of[(size_t)k] = (int)gleave.size(); gleave.push_back(k); }
        for (int i = 0; i < m; ++i) igrp[(size_t)i] = of[(size_t)leave[i]];
    } else {
        gleave.push_back(0);
    }
    const int G = (int)gleave.size();
    // every group's look at foldid before any fit: the ids' range, its rows, p + intercept < its rows
    std::vector<std::unique_ptr<DenseLogitData>> Ds;
    std::vector<double> hnv((size_t)G), hd((size_t)G, 0.0);
    for (int gi = 0; gi < G; ++gi) {
        Ds.emplace_back(new DenseLogitData(c, X, n, p, nullptr, standardize, intercept, 0));
        DenseLogitData &D = *Ds.back();
        if (foldid) {
            const int k = gleave[(size_t)gi];
            int rc = 0;
            if (k > 0) rc = D.set_fold(foldid, nfolds, k, irls_maxit);
            else { std::vector<int64_t> none; int64_t all = 0; rc = logit_fold_scan(c, who, foldid, n, nfolds, 0, 0, &all, &none); }   // (the ids' range; the fit is the plain one)
            if (rc) return rc;
            if ((int64_t)q >= D.n_eff) {
                set_error("%s: p + intercept >= the %lld rows outside fold %d is not supported (the reference's XWXt branch, "
                          "ref src/oem_logistic_dense.h:524-566)", who, (long long)D.n_eff, k);
                return OEMGPU_ERR_UNSUPPORTED;
            }
        }
        hnv[(size_t)gi] = (double)D.n_eff;
    }
    // ---- workspace (c->aux): what the groups hold, one chunk's state, the Hessian pass's stages
    Bump B;
    const size_t a_s = B.take(8 * (size_t)G * p), a_xx = B.take(8 * (size_t)G * q * q), a_a = B.take(8 * (size_t)G * q * q), a_nv = B.take(8 * (size_t)G),
                 a_z = B.take(8 * (size_t)q), a_g0 = B.take(8 * (size_t)(p + 2)), a_col = Y.rs != 1 ? B.take(8 * (size_t)n) : 0;
    const size_t a_b = B.take(8 * (size_t)mch * q), a_bi = B.take(8 * (size_t)mch * q), a_xy = B.take(8 * (size_t)mch * q),
                 a_bt = B.take(8 * (size_t)mch * q), a_g = B.take(8 * (size_t)mch * (p + 2)), a_live = B.take(4 * (size_t)mch),
                 a_stop = B.take(4 * (size_t)mch), a_grp = B.take(4 * (size_t)mch), a_lv = B.take(4 * (size_t)mch), a_yc = B.take(4 * (size_t)mch),
                 a_it = B.take(8 * (size_t)mch), a_loss = B.take(8 * (size_t)mch),
                 a_pk = B.take(sizeof(PenK) * (size_t)nl * mch), a_part = B.take(8 * PW.part_doubles), a_out = B.take(8 * (size_t)mch * nl * (p + 1));
    const size_t a_pf = B.take(8 * (size_t)q), a_gw = B.take(8 * (size_t)ng1), a_perm = B.take(4 * (size_t)(q + 1)), a_gs = B.take(4 * (size_t)(ng + 1)),
                 a_gof = B.take(4 * (size_t)q), a_gz = B.take(4 * (size_t)ng1);
    const size_t a_data = B.take(Ds[0]->ws_bytes());
    ctx_void_cv(c);
    if (ctx_grow(c, &c->aux, &c->aux_bytes, B.off)) return OEMGPU_ERR_HIP;
    char *W = c->aux;
    double *sc = (double *)(W + a_s), *xx = (double *)(W + a_xx), *A = (double *)(W + a_a), *nv = (double *)(W + a_nv), *zero = (double *)(W + a_z),
           *g0 = (double *)(W + a_g0), *beta = (double *)(W + a_b), *birls = (double *)(W + a_bi), *xy = (double *)(W + a_xy), *bt = (double *)(W + a_bt),
           *g = (double *)(W + a_g), *iters = (double *)(W + a_it), *lossw = (double *)(W + a_loss), *part = (double *)(W + a_part),
           *bout = (double *)(W + a_out);
    int *live = (int *)(W + a_live), *stopw = (int *)(W + a_stop), *grp = (int *)(W + a_grp), *lvd = (int *)(W + a_lv), *ycd = (int *)(W + a_yc);
    PenK *pkd = (PenK *)(W + a_pk);
    hipStream_t s = c->stream;
    OEM_HIP(hipMemcpyAsync(W + a_pf, T.pf.data(), 8 * (size_t)q, hipMemcpyHostToDevice, s));
    OEM_HIP(hipMemcpyAsync(W + a_gw, T.gw.data(), 8 * T.gw.size(), hipMemcpyHostToDevice, s));
    if (T.nperm) OEM_HIP(hipMemcpyAsync(W + a_perm, T.perm.data(), 4 * (size_t)T.nperm, hipMemcpyHostToDevice, s));
    OEM_HIP(hipMemcpyAsync(W + a_gs, T.gstart.data(), 4 * T.gstart.size(), hipMemcpyHostToDevice, s));
    OEM_HIP(hipMemcpyAsync(W + a_gof, T.gof.data(), 4 * (size_t)q, hipMemcpyHostToDevice, s));
    OEM_HIP(hipMemcpyAsync(W + a_gz, T.gzero.data(), 4 * T.gzero.size(), hipMemcpyHostToDevice, s));
    OEM_HIP(hipMemcpyAsync(nv, hnv.data(), 8 * (size_t)G, hipMemcpyHostToDevice, s));
    OEM_HIP(hipStreamSynchronize(s));                                           // (the tables are the host's again)
    LogitPen LP;
    LP.pf = (const double *)(W + a_pf); LP.gw = (const double *)(W + a_gw); LP.perm = (const int *)(W + a_perm);
    LP.gstart = (const int *)(W + a_gs); LP.gof = (const int *)(W + a_gof); LP.gzero = (const int *)(W + a_gz); LP.ngroups = ng;
    LP.k = PenK{K_SOFT, 0.0, 1.0, 0.0, 0.0};
    hipEvent_t ev[2];
    const bool timing = c->timing;
    if (timing) { OEM_HIP(hipEventCreate(&ev[0])); OEM_HIP(hipEventCreate(&ev[1])); }
    auto stage = [&](double *acc, auto &&fn) -> int {
        if (timing) (void)hipEventRecord(ev[0], s);
        int r = fn();
        if (r) return r;
        if (timing) {
            (void)hipEventRecord(ev[1], s);
            if (hipEventSynchronize(ev[1]) != hipSuccess) { set_error("hipEventSynchronize failed"); return OEMGPU_ERR_HIP; }
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
            *acc += ms;
        }
        return 0;
    };
    auto finish = [&](int r) -> int {
        if (timing) { (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]); }
        if (r) (void)hipStreamSynchronize(s);
        return r;
    };
    // ---- once per call and group: s, XX at beta = 0, d = 1.0005 lambda_max (h :514), A = dI - XX
    int rc = 0;
    const double *y0 = Y.y;
    if (Y.rs != 1) {
        double *col = (double *)(W + a_col);
        if ((rc = launch_multi_column(s, Y, n, 0, col))) return finish(rc);
        y0 = col;
    }
    OEM_HIP(hipMemsetAsync(zero, 0, 8 * (size_t)q, s));
    for (int gi = 0; gi < G; ++gi) {
        DenseLogitData &D = *Ds[(size_t)gi];
        double *scg = sc + (size_t)gi * p, *xxg = xx + (size_t)gi * q * q, *Ag = A + (size_t)gi * q * q;
        D.y = y0;
        rc = D.bind(W + a_data);                                                // (the groups take the stages' buffers in turn, on one stream)
        if (!rc) rc = D.scale(scg);
        if (rc) return finish(rc);
        rc = stage(&g_lm_stats.ms_gram, [&]() -> int {
            int r = D.hessian(zero, scg, 0, g0, xxg);
            if (r) return r;
            double lm = 0.0;
            r = oemgpu_eig_max_dev(c, xxg, q, &lm);                             // (synchronises)
            if (r) return r;
            hd[(size_t)gi] = lm * 1.0005;
            hipLaunchKernelGGL(logit_a_kernel, dim3((q + 255) / 256, q), dim3(256), 0, s, xxg, q, hd[(size_t)gi], Ag);
            OEM_HIP(hipGetLastError());
            return 0;
        });
        if (rc) return finish(rc);
        g_lm_stats.grams += 1; g_lm_stats.lanczos += 1;
    }
    const bool alds = q <= LOGIT_A_LDS_Q;
    const size_t lds_inner = 8 * (size_t)(3 * q + ng1 + (alds ? q * q : 0));
    if (lds_limit_once(alds ? reinterpret_cast<const void *>(&logit_inner_multi_kernel<true>) : reinterpret_cast<const void *>(&logit_inner_multi_kernel<false>),
                       lds_inner))
        return finish(OEMGPU_ERR_HIP);
    std::vector<double> hxy((size_t)mch * q), lam((size_t)mch * nl), hloss((size_t)mch), hit((size_t)mch);
    std::vector<std::vector<double>> baser((size_t)mch, std::vector<double>((size_t)nl));
    std::vector<PenK> pkh((size_t)nl * mch);
    std::vector<int> hlive((size_t)mch), hstop((size_t)mch), nit((size_t)mch), hyc((size_t)mch);
    const size_t nk = (size_t)npen * nl, blen = nk * (size_t)(p + 1);
    bool interrupted = false;
    for (int r0 = 0; r0 < m && !interrupted; r0 += mch) {
        const int mc = m - r0 < mch ? m - r0 : mch;
        const LogitMultiPlan pl = logit_multi_plan(n, p, mc, c->num_cu);
        // the plain call reads its chunk's columns of Y where they lie; a fold call reads column resp[i] for instance i, masked
        const MultiY Yc{foldid ? Y.y : Y.y + (int64_t)resp[r0] * Y.cs, Y.rs, Y.cs};
        LogitMultiFold FM;
        const LogitMultiFold *fm = nullptr;
        OEM_HIP(hipMemcpyAsync(grp, igrp.data() + r0, 4 * (size_t)mc, hipMemcpyHostToDevice, s));
        if (foldid) {
            for (int r = 0; r < mc; ++r) hyc[(size_t)r] = resp[r0 + r];
            OEM_HIP(hipMemcpyAsync(lvd, leave + r0, 4 * (size_t)mc, hipMemcpyHostToDevice, s));
            OEM_HIP(hipMemcpyAsync(ycd, hyc.data(), 4 * (size_t)mc, hipMemcpyHostToDevice, s));
            OEM_HIP(hipStreamSynchronize(s));                                   // (hyc is the host's again)
            FM.foldid = foldid; FM.leave = lvd; FM.ycol = ycd;
            fm = &FM;
        }
        const dim3 gq((unsigned)((q + 255) / 256), (unsigned)mc);
        auto set_live = [&]() -> int {
            hipLaunchKernelGGL(logit_fill_int_kernel, dim3((mc + 255) / 256), dim3(256), 0, s, live, mc, 1);
            OEM_HIP(hipGetLastError());
            std::fill(hlive.begin(), hlive.begin() + mc, 1);
            return 0;
        };
        // ---- init_oem per instance: XY = s o X'Y / n, lambda_0 = max |XY| over the non-intercept slots (h :762-805)
        if ((rc = set_live())) return finish(rc);
        OEM_HIP(hipMemsetAsync(iters, 0, 8 * (size_t)mc, s));
        rc = stage(&g_lm_stats.ms_rows, [&]() -> int {
            int r = launch_logit_multi_rows(s, pl, X, Yc, nullptr, intercept, 0, live, part, fm);
            if (!r) r = launch_logit_multi_reduce(s, pl, part, live, g);
            return r;
        });
        if (rc) return finish(rc);
        hipLaunchKernelGGL(logit_xy_multi_kernel, gq, dim3(256), 0, s, xx, beta, g, sc, p, intercept, nv, 1, live, grp, xy);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipMemcpyAsync(hxy.data(), xy, 8 * (size_t)mc * q, hipMemcpyDeviceToHost, s));
        OEM_HIP(hipStreamSynchronize(s));
        for (int r = 0; r < mc; ++r) {
            double lmax = 0.0;
            for (int j = o1; j < q; ++j) lmax = std::fmax(lmax, std::fabs(hxy[(size_t)r * q + j]));
            if (!provided) logit_lambda_base(o, lmax, nl, baser[(size_t)r].data());
        }
        for (int k = 0; k < npen && !interrupted; ++k) {
            const int pen = o->penalty[k];
            const int nlk = pen == OEMGPU_OLS ? 1 : nl;
            for (int r = 0; r < mc; ++r) {
                double *lr = lam.data() + (size_t)r * nl;
                logit_lambda_row(o, k, provided, baser[(size_t)r], nl, lr);
                for (int i = 0; i < nl; ++i) {
                    lambda_out[((size_t)(r0 + r) * npen + k) * nl + i] = lr[i];
                    pkh[(size_t)i * mc + r] = logit_penk(o, pen, lr[i], hd[(size_t)igrp[(size_t)(r0 + r)]]);
                }
            }
            OEM_HIP(hipMemcpy(pkd, pkh.data(), sizeof(PenK) * (size_t)nl * mc, hipMemcpyHostToDevice));
            OEM_HIP(hipMemsetAsync(beta, 0, 8 * (size_t)mc * q, s));                 // init(): cold start (h :813)
            OEM_HIP(hipMemsetAsync(bout, 0, 8 * (size_t)mc * nl * (p + 1), s));
            for (int li = 0; li < nlk && !interrupted; ++li) {
                if ((rc = set_live())) return finish(rc);
                int nlive = mc;
                for (int i = 0; i < irls_maxit && nlive > 0; ++i) {
                    if (o->interrupt && o->interrupt(o->interrupt_arg)) { interrupted = true; break; }
                    hipLaunchKernelGGL(logit_step_multi_kernel, gq, dim3(256), 0, s, beta, sc, q, intercept, live, grp, birls, bt);
                    OEM_HIP(hipGetLastError());
                    if (!(i == 0 && li > 0)) {
                        rc = stage(&g_lm_stats.ms_rows, [&]() -> int {
                            int r = launch_logit_multi_rows(s, pl, X, Yc, bt, intercept, 1, live, part, fm);
                            if (!r) r = launch_logit_multi_reduce(s, pl, part, live, g);
                            return r;
                        });
                        if (rc) return finish(rc);
                        g_lm_stats.row_passes += 1;
                        g_lm_stats.blocks_skipped += lm_blocks_skipped(pl, hlive);
                        hipLaunchKernelGGL(logit_xy_multi_kernel, gq, dim3(256), 0, s, xx, beta, g, sc, p, intercept, nv, 0, live, grp, xy);
                        OEM_HIP(hipGetLastError());
                    }
                    // the OEM loop at this lambda (h :1010-1022): one workgroup per live instance, on its group's A
                    rc = stage(&g_lm_stats.ms_inner, [&]() -> int {
                        const PenK *pk = pkd + (size_t)li * mc;
                        if (alds) {
                            hipLaunchKernelGGL(logit_inner_multi_kernel<true>, dim3(mc), dim3(1024), lds_inner, s, A, xy, beta, q, LP, pk, o->maxit, o->tol, live, grp, iters);
                        } else {
                            hipLaunchKernelGGL(logit_inner_multi_kernel<false>, dim3(mc), dim3(1024), lds_inner, s, A, xy, beta, q, LP, pk, o->maxit, o->tol, live, grp, iters);
                        }
                        OEM_HIP(hipGetLastError());
                        return 0;
                    });
                    if (rc) return finish(rc);
                    hipLaunchKernelGGL(logit_irls_stop_multi_kernel, dim3(mc), dim3(1024), 0, s, beta, birls, q, irls_tol, live, stopw);
                    OEM_HIP(hipGetLastError());
                    OEM_HIP(hipMemcpyAsync(hstop.data(), stopw, 4 * (size_t)mc, hipMemcpyDeviceToHost, s));
                    OEM_HIP(hipStreamSynchronize(s));                              // the one host sync of a lock-step IRLS step
                    g_lm_stats.steps += 1;
                    for (int r = 0; r < mc; ++r)
                        if (hlive[(size_t)r] && hstop[(size_t)r]) { hlive[(size_t)r] = 0; nit[(size_t)r] = i + 1; --nlive; }
                }
                if (interrupted) break;
                for (int r = 0; r < mc; ++r)
                    if (hlive[(size_t)r]) nit[(size_t)r] = irls_maxit + 1;             // the cap (h :1035)
                hipLaunchKernelGGL(logit_back_multi_kernel, dim3((p + 1 + 255) / 256, mc), dim3(256), 0, s, beta, sc, g, p, intercept, (size_t)nl * (p + 1),
                                   grp, bout + (size_t)li * (p + 1), lossw);
                OEM_HIP(hipGetLastError());
                if (o->compute_loss) {                                              // the loss of the LAST prob computed: of its last own row pass
                    OEM_HIP(hipMemcpyAsync(hloss.data(), lossw, 8 * (size_t)mc, hipMemcpyDeviceToHost, s));
                    OEM_HIP(hipStreamSynchronize(s));
                }
                for (int r = 0; r < mc; ++r) {
                    const size_t e = ((size_t)(r0 + r) * npen + k) * nl + li;
                    niter[e] = nit[(size_t)r];
                    loss_out[e] = o->compute_loss ? hloss[(size_t)r] : 1e99;
                }
            }
            if (interrupted) break;
            for (int r = 0; r < mc; ++r)
                for (int li = nlk; li < nl; ++li) { const size_t e = ((size_t)(r0 + r) * npen + k) * nl + li; niter[e] = 0; loss_out[e] = 0.0; }
            OEM_HIP(hipStreamSynchronize(s));
            OEM_HIP(hipMemcpy2D(beta_out + blen * r0 + (size_t)k * nl * (p + 1), 8 * blen, bout, 8 * (size_t)nl * (p + 1), 8 * (size_t)nl * (p + 1), mc,
                                hipMemcpyDeviceToHost));
        }
        if (interrupted) break;
        OEM_HIP(hipMemcpy(hit.data(), iters, 8 * (size_t)mc, hipMemcpyDeviceToHost));
        for (int r = 0; r < mc; ++r) {
            const int gi = igrp[(size_t)(r0 + r)];
            g_lm_stats.inner_iters += hit[(size_t)r];
            d_out[r0 + r] = hd[(size_t)gi];
            if (nobs) nobs[r0 + r] = (int64_t)hnv[(size_t)gi];
        }
    }
    if (interrupted) { (void)finish(1); set_error("interrupted"); return OEMGPU_ERR_INTERRUPTED; }
    g_lm_stats.wall_ms = now_ms() - t_start;
    return finish(0);
}

// the checks of the many-response entries, before a device is looked for; then the fit.  foldid_dev null: the plain call, the
// instances (r, 0) for r < m; else the list (resp[i], leave_out[i]) of ninst instances
static int logistic_multi_checked(const char *who, oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const double *y_dev, int64_t rs, int64_t cs,
                                  int32_t m, bool fold, const int32_t *foldid_dev, int32_t nfolds, int32_t ninst, const int32_t *resp, const int32_t *leave_out,
                                  int32_t standardize, int32_t intercept, int32_t hessian_full, int32_t irls_maxit, double irls_tol,
                                  const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, int64_t *nobs)
{
    if (fold && ninst < 1) { set_error("%s: ninst must be at least 1", who); return OEMGPU_ERR_ARG; }
    if (!c || !X.x || !y_dev || !o || !beta || !lambda_out || !niter || !loss || !d || (fold && (!foldid_dev || !resp || !leave_out || !nobs))) {
        set_error("%s: NULL argument", who);
        return OEMGPU_ERR_ARG;
    }
    int rc = multi_y_check(who, n, rs, cs, m);
    if (rc) return rc;
    if (fold) {
        if (nfolds < 3) { set_error("nfolds must be bigger than 3; nfolds=10 recommended"); return OEMGPU_ERR_ARG; }            // ref R/cv_oem.R:126-127
        for (int i = 0; i < ninst; ++i) {
            if (leave_out[i] < 0 || leave_out[i] > nfolds) { set_error("%s: leave_out must be in [0, nfolds]", who); return OEMGPU_ERR_ARG; }
            if (resp[i] < 0 || resp[i] >= m) { set_error("%s: resp must be in [0, m)", who); return OEMGPU_ERR_ARG; }
        }
    }
    rc = dense_src_check(who, X, n, p);
    if (!rc) rc = logistic_check(n, p, intercept, hessian_full, irls_maxit, irls_tol, o);
    if (rc) return rc;
    if (hessian_full) {
        set_error("%s: a full Hessian is one per response and step: fit each column with fit_logistic_dense", who);
        return OEMGPU_ERR_UNSUPPORTED;
    }
    if (p + (intercept ? 1 : 0) > LOGIT_WG_MAX) {
        set_error("%s: p + intercept > %d is not supported (beyond one workgroup the inner solve is a product of all responses): fit each column with "
                  "fit_logistic_dense", who, LOGIT_WG_MAX);
        return OEMGPU_ERR_UNSUPPORTED;
    }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    if (fold)
        return logistic_irls_multi(who, c, X, n, p, MultiY{y_dev, rs, cs}, foldid_dev, nfolds, ninst, resp, leave_out, standardize, intercept, irls_maxit,
                                   irls_tol, o, beta, lambda_out, niter, loss, d, nobs);
    std::vector<int32_t> all((size_t)m), none((size_t)m, 0);
    for (int r = 0; r < m; ++r) all[(size_t)r] = r;
    return logistic_irls_multi(who, c, X, n, p, MultiY{y_dev, rs, cs}, nullptr, 0, m, all.data(), none.data(), standardize, intercept, irls_maxit, irls_tol,
                               o, beta, lambda_out, niter, loss, d, nullptr);
}

// one row pass of logistic_multi.hip for the kernel tests: out[r] (p + 2 doubles) for the live columns, chunk of columns after chunk.
// foldid null: column r is response r of Y on every row; else column r is response ycol[r] (r without ycol) on the rows with
// foldid != leave[r] (ycol, leave, live_host: host words)
static int logistic_multi_rows_selftest(oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const MultiY &Y, int32_t m, const double *bt, int32_t intercept,
                                        int32_t mode, const int32_t *live_host, double *out, const int32_t *foldid = nullptr, const int32_t *leave = nullptr,
                                        const int32_t *ycol = nullptr)
{
    g_lm_stats = LogitMultiStats();
    const int q = p + (intercept ? 1 : 0);
    const int mch = m < LMULTI_MCH ? m : LMULTI_MCH;
    const LogitMultiPlan PW = logit_multi_plan(n, p, mch, c->num_cu);
    Bump B;
    const size_t a_part = B.take(8 * PW.part_doubles), a_live = B.take(4 * (size_t)m), a_lv = B.take(4 * (size_t)m), a_yc = B.take(4 * (size_t)m);
    ctx_void_cv(c);
    if (ctx_grow(c, &c->aux, &c->aux_bytes, B.off)) return OEMGPU_ERR_HIP;
    double *part = (double *)(c->aux + a_part);
    int *live = (int *)(c->aux + a_live), *lvd = (int *)(c->aux + a_lv), *ycd = (int *)(c->aux + a_yc);
    std::vector<int> hl((size_t)m, 1);
    if (live_host) for (int r = 0; r < m; ++r) hl[(size_t)r] = live_host[r] != 0;
    OEM_HIP(hipMemcpy(live, hl.data(), 4 * (size_t)m, hipMemcpyHostToDevice));
    if (foldid) {
        OEM_HIP(hipMemcpy(lvd, leave, 4 * (size_t)m, hipMemcpyHostToDevice));
        if (ycol) OEM_HIP(hipMemcpy(ycd, ycol, 4 * (size_t)m, hipMemcpyHostToDevice));
    }
    for (int r0 = 0; r0 < m; r0 += mch) {
        const int mc = m - r0 < mch ? m - r0 : mch;
        const LogitMultiPlan pl = logit_multi_plan(n, p, mc, c->num_cu);
        const std::vector<int> lc(hl.begin() + r0, hl.begin() + r0 + mc);
        const LogitMultiFold FM{foldid, lvd + r0, ycol ? ycd + r0 : nullptr};
        const MultiY Yc{(foldid && ycol) ? Y.y : Y.y + (int64_t)r0 * Y.cs, Y.rs, Y.cs};
        int rc = launch_logit_multi_rows(c->stream, pl, X, Yc, mode ? bt + (size_t)r0 * q : nullptr, intercept, mode, live + r0, part, foldid ? &FM : nullptr);
        if (!rc) rc = launch_logit_multi_reduce(c->stream, pl, part, live + r0, out + (size_t)r0 * (p + 2));
        if (rc) return rc;
        g_lm_stats.row_passes += 1;
        g_lm_stats.blocks_skipped += lm_blocks_skipped(pl, lc);
    }
    OEM_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace oemgpu

using namespace oemgpu;

extern "C" {
#pragma GCC visibility push(default)

int oemgpu_fit_logistic_dense_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev, int32_t standardize,
                                  int32_t intercept, int32_t hessian_full, int32_t irls_maxit, double irls_tol, const oemgpu_opts *o,
                                  double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    return logistic_fit_checked("fit_logistic_dense", false, c, dense_src_cm(x_dev, ld), n, p, y_dev, nullptr, 0, 0, standardize, intercept, hessian_full,
                                irls_maxit, irls_tol, o, beta, lambda_out, niter, loss, d);
}

int oemgpu_fit_logistic_dense_fold_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                                       const int32_t *foldid_dev, int32_t nfolds, int32_t leave_out, int32_t standardize, int32_t intercept,
                                       int32_t hessian_full, int32_t irls_maxit, double irls_tol, const oemgpu_opts *o,
                                       double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    return logistic_fit_checked("fit_logistic_dense_fold", true, c, dense_src_cm(x_dev, ld), n, p, y_dev, foldid_dev, nfolds, leave_out, standardize,
                                intercept, hessian_full, irls_maxit, irls_tol, o, beta, lambda_out, niter, loss, d);
}

int oemgpu_fit_logistic_dense_rm_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                                     int32_t standardize, int32_t intercept, int32_t hessian_full, int32_t irls_maxit, double irls_tol,
                                     const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    return logistic_fit_checked("fit_logistic_dense_rm", false, c, dense_src_rm(x_dev, dtype, ldr), n, p, y_dev, nullptr, 0, 0, standardize, intercept,
                                hessian_full, irls_maxit, irls_tol, o, beta, lambda_out, niter, loss, d);
}

int oemgpu_fit_logistic_dense_fold_rm_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                                          const int32_t *foldid_dev, int32_t nfolds, int32_t leave_out, int32_t standardize, int32_t intercept,
                                          int32_t hessian_full, int32_t irls_maxit, double irls_tol, const oemgpu_opts *o,
                                          double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    return logistic_fit_checked("fit_logistic_dense_fold_rm", true, c, dense_src_rm(x_dev, dtype, ldr), n, p, y_dev, foldid_dev, nfolds, leave_out,
                                standardize, intercept, hessian_full, irls_maxit, irls_tol, o, beta, lambda_out, niter, loss, d);
}

int oemgpu_selftest_logistic_rm_plan(int64_t n, int32_t p, int32_t dtype, int32_t intercept, int32_t num_cu, int64_t *out)
{
    if (n < 1 || p < 1 || num_cu < 1 || !out || (dtype != OEMGPU_F64 && dtype != OEMGPU_F32)) { set_error("selftest_logistic_rm_plan: bad argument"); return OEMGPU_ERR_ARG; }
    if (p > LOGIT_P_MAX) { set_error("selftest_logistic_rm_plan: p > %d is not supported", LOGIT_P_MAX); return OEMGPU_ERR_UNSUPPORTED; }
    const LogitPlan P = logit_plan(n, p, intercept, num_cu);
    const LogitRmPlan R = logit_rm_plan(p);
    out[0] = R.nband; out[1] = R.bw; out[2] = p - (int64_t)(R.nband - 1) * R.bw; out[3] = (int64_t)R.lds_total;
    out[4] = P.ch; out[5] = P.nchunk; out[6] = P.rbz; out[7] = P.nzblk;
    return 0;
}

int oemgpu_fit_logistic_dense_multi_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev, int64_t y_rs,
                                        int64_t y_cs, int32_t m, int32_t standardize, int32_t intercept, int32_t hessian_full, int32_t irls_maxit,
                                        double irls_tol, const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    return logistic_multi_checked("fit_logistic_dense_multi", c, dense_src_cm(x_dev, ld), n, p, y_dev, y_rs, y_cs, m, false, nullptr, 0, 0, nullptr, nullptr,
                                  standardize, intercept, hessian_full, irls_maxit, irls_tol, o, beta, lambda_out, niter, loss, d, nullptr);
}

int oemgpu_fit_logistic_dense_multi_rm_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                                           int64_t y_rs, int64_t y_cs, int32_t m, int32_t standardize, int32_t intercept, int32_t hessian_full,
                                           int32_t irls_maxit, double irls_tol, const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter,
                                           double *loss, double *d)
{
    return logistic_multi_checked("fit_logistic_dense_multi_rm", c, dense_src_rm(x_dev, dtype, ldr), n, p, y_dev, y_rs, y_cs, m, false, nullptr, 0, 0, nullptr,
                                  nullptr, standardize, intercept, hessian_full, irls_maxit, irls_tol, o, beta, lambda_out, niter, loss, d, nullptr);
}

int oemgpu_fit_logistic_dense_multi_fold_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev, int64_t y_rs,
                                             int64_t y_cs, int32_t m, const int32_t *foldid_dev, int32_t nfolds, int32_t ninst, const int32_t *resp,
                                             const int32_t *leave_out, int32_t standardize, int32_t intercept, int32_t hessian_full, int32_t irls_maxit,
                                             double irls_tol, const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d,
                                             int64_t *nobs)
{
    return logistic_multi_checked("fit_logistic_dense_multi_fold", c, dense_src_cm(x_dev, ld), n, p, y_dev, y_rs, y_cs, m, true, foldid_dev, nfolds, ninst, resp,
                                  leave_out, standardize, intercept, hessian_full, irls_maxit, irls_tol, o, beta, lambda_out, niter, loss, d, nobs);
}

int oemgpu_fit_logistic_dense_multi_fold_rm_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                                                int64_t y_rs, int64_t y_cs, int32_t m, const int32_t *foldid_dev, int32_t nfolds, int32_t ninst,
                                                const int32_t *resp, const int32_t *leave_out, int32_t standardize, int32_t intercept, int32_t hessian_full,
                                                int32_t irls_maxit, double irls_tol, const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter,
                                                double *loss, double *d, int64_t *nobs)
{
    return logistic_multi_checked("fit_logistic_dense_multi_fold_rm", c, dense_src_rm(x_dev, dtype, ldr), n, p, y_dev, y_rs, y_cs, m, true, foldid_dev, nfolds,
                                  ninst, resp, leave_out, standardize, intercept, hessian_full, irls_maxit, irls_tol, o, beta, lambda_out, niter, loss, d, nobs);
}

// the workspace of a fold call as pure host arithmetic: ninst instances in ngroups groups (the distinct leave_out values)
int oemgpu_selftest_logistic_multi_fold_plan(int64_t n, int32_t p, int32_t ninst, int32_t ngroups, int32_t intercept, int32_t layout, int32_t num_cu,
                                             int64_t *out)
{
    if (n < 1 || p < 1 || ninst < 1 || ngroups < 1 || num_cu < 1 || (layout != 0 && layout != 1) || !out) {
        set_error("selftest_logistic_multi_fold_plan: bad argument");
        return OEMGPU_ERR_ARG;
    }
    const int q = p + (intercept ? 1 : 0);
    if (q > LOGIT_WG_MAX) { set_error("selftest_logistic_multi_fold_plan: p + intercept > %d is not supported", LOGIT_WG_MAX); return OEMGPU_ERR_UNSUPPORTED; }
    const int mch = ninst < LMULTI_MCH ? ninst : LMULTI_MCH;
    const LogitMultiPlan pl = logit_multi_plan(n, p, mch, num_cu);
    const LogitPlan P = logit_plan(n, p, intercept, num_cu);
    const size_t groups = 8 * (size_t)ngroups * ((size_t)p + 2 * (size_t)q * q + 1);                      // s, XX, A and the rows of every group
    const size_t shared = 8 * ((size_t)q + (size_t)(p + 2)) + (layout == 1 ? 8 * (size_t)256 * p : 0);    // beta = 0, g; the scale pass's partials
    const size_t chunk = 8 * ((size_t)mch * q * 4 + (size_t)mch * (p + 2) + 2 * (size_t)mch) + 4 * 5 * (size_t)mch + sizeof(PenK) * (size_t)mch;
    out[0] = pl.rows; out[1] = pl.nchunk; out[2] = mch; out[3] = (ninst + LMULTI_MCH - 1) / LMULTI_MCH; out[4] = ngroups;
    out[5] = (int64_t)(8 * pl.part_doubles); out[6] = (int64_t)groups; out[7] = (int64_t)shared; out[8] = (int64_t)chunk; out[9] = (int64_t)P.ws_bytes;
    out[10] = out[5] + out[6] + out[7] + out[8] + out[9];
    return 0;
}

int oemgpu_selftest_logistic_multi_plan(int64_t n, int32_t p, int32_t m, int32_t intercept, int32_t layout, int32_t num_cu, int64_t *out)
{
    if (n < 1 || p < 1 || m < 1 || num_cu < 1 || (layout != 0 && layout != 1) || !out) { set_error("selftest_logistic_multi_plan: bad argument"); return OEMGPU_ERR_ARG; }
    const int q = p + (intercept ? 1 : 0);
    if (q > LOGIT_WG_MAX) { set_error("selftest_logistic_multi_plan: p + intercept > %d is not supported", LOGIT_WG_MAX); return OEMGPU_ERR_UNSUPPORTED; }
    const int mch = m < LMULTI_MCH ? m : LMULTI_MCH;
    const LogitMultiPlan pl = logit_multi_plan(n, p, mch, num_cu);
    const LogitPlan P = logit_plan(n, p, intercept, num_cu);
    const size_t shared = 8 * ((size_t)p + 2 * (size_t)q * q + (size_t)q + (size_t)(p + 2)) + (layout == 1 ? 8 * (size_t)256 * p : 0);   // s, XX, A, beta = 0, g; the scale pass's partials
    const size_t chunk = 8 * ((size_t)mch * q * 4 + (size_t)mch * (p + 2) + 3 * (size_t)mch) + sizeof(PenK) * (size_t)mch;
    out[0] = pl.rows; out[1] = pl.nchunk; out[2] = pl.mb; out[3] = pl.lt; out[4] = pl.band; out[5] = (int64_t)pl.lds_bytes; out[6] = LMULTI_MCH;
    out[7] = (m + LMULTI_MCH - 1) / LMULTI_MCH; out[8] = pl.npass; out[9] = pl.tpw;
    out[10] = (int64_t)(8 * pl.part_doubles); out[11] = (int64_t)shared; out[12] = (int64_t)chunk; out[13] = (int64_t)P.ws_bytes;
    out[14] = out[10] + out[11] + out[12] + out[13];
    out[15] = q <= LOGIT_A_LDS_Q;
    return 0;
}

int oemgpu_selftest_logistic_multi_rows_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                                            int64_t y_rs, int64_t y_cs, int32_t m, const double *btilde_dev, int32_t intercept, int32_t mode,
                                            const int32_t *live, double *out_dev)
{
    const char *who = "selftest_logistic_multi_rows";
    if (!c || !x_dev || !y_dev || !out_dev || (mode && !btilde_dev)) { set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG; }
    if (n < 1 || p < 1 || (mode != 0 && mode != 1)) { set_error("%s: bad argument", who); return OEMGPU_ERR_ARG; }
    const DenseSrc X = dtype < 0 ? dense_src_cm((const double *)x_dev, ld) : dense_src_rm(x_dev, dtype, ld);
    int rc = multi_y_check(who, n, y_rs, y_cs, m);
    if (!rc) rc = dense_src_check(who, X, n, p);
    if (rc) return rc;
    if (p > LMULTI_P_MAX) { set_error("%s: p > %d is not supported", who, LMULTI_P_MAX); return OEMGPU_ERR_UNSUPPORTED; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    return logistic_multi_rows_selftest(c, X, n, p, MultiY{y_dev, y_rs, y_cs}, m, btilde_dev, intercept, mode, live, out_dev);
}

int oemgpu_selftest_logistic_multi_rows_fold_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                                                 int64_t y_rs, int64_t y_cs, int32_t m, const int32_t *foldid_dev, int32_t ncol, const int32_t *leave,
                                                 const int32_t *ycol, const double *btilde_dev, int32_t intercept, int32_t mode, const int32_t *live,
                                                 double *out_dev)
{
    const char *who = "selftest_logistic_multi_rows_fold";
    if (!c || !x_dev || !y_dev || !foldid_dev || !leave || !out_dev || (mode && !btilde_dev)) { set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG; }
    if (n < 1 || p < 1 || ncol < 1 || (mode != 0 && mode != 1) || (!ycol && ncol != m)) { set_error("%s: bad argument", who); return OEMGPU_ERR_ARG; }
    const DenseSrc X = dtype < 0 ? dense_src_cm((const double *)x_dev, ld) : dense_src_rm(x_dev, dtype, ld);
    int rc = multi_y_check(who, n, y_rs, y_cs, m);
    if (!rc) rc = dense_src_check(who, X, n, p);
    if (rc) return rc;
    if (ycol)
        for (int t = 0; t < ncol; ++t)
            if (ycol[t] < 0 || ycol[t] >= m) { set_error("%s: ycol must be in [0, m)", who); return OEMGPU_ERR_ARG; }
    if (p > LMULTI_P_MAX) { set_error("%s: p > %d is not supported", who, LMULTI_P_MAX); return OEMGPU_ERR_UNSUPPORTED; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    return logistic_multi_rows_selftest(c, X, n, p, MultiY{y_dev, y_rs, y_cs}, ncol, btilde_dev, intercept, mode, live, out_dev, foldid_dev, leave, ycol);
}

int oemgpu_last_logistic_multi_stats(double *out)
{
    if (!out) { set_error("last_logistic_multi_stats: NULL"); return OEMGPU_ERR_ARG; }
    const LogitMultiStats &s = g_lm_stats;
    out[0] = s.steps; out[1] = s.row_passes; out[2] = s.blocks_skipped; out[3] = s.inner_iters; out[4] = s.grams; out[5] = s.lanczos;
    out[6] = s.ms_rows; out[7] = s.ms_gram; out[8] = s.ms_inner; out[9] = s.wall_ms;
    return 0;
}

int oemgpu_fit_logistic_dense(const double *x, int64_t n, int32_t p, const double *y, int32_t standardize, int32_t intercept, int32_t hessian_full,
                              int32_t irls_maxit, double irls_tol, const oemgpu_opts *o,
                              double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    if (!x || !y || !o || !beta || !lambda_out || !niter || !loss || !d) { set_error("fit_logistic_dense: NULL argument"); return OEMGPU_ERR_ARG; }
    int rc = logistic_check(n, p, intercept, hessian_full, irls_maxit, irls_tol, o);
    if (rc) return rc;
    oemgpu_ctx *c = ctx_acquire(o->device);
    if (!c) return OEMGPU_ERR_NO_DEVICE;
    double *xd = nullptr, *yd = nullptr;
    int64_t ld = 0;
    rc = host_upload_resident(c, x, n, p, y, o, &xd, &ld, &yd, 0, true);
    if (!rc) rc = logistic_fit_src(c, dense_src_cm(xd, ld), n, p, yd, nullptr, 0, 0, standardize, intercept, hessian_full, irls_maxit, irls_tol, o, beta,
                                   lambda_out, niter, loss, d);
    (void)hipStreamSynchronize(c->stream);
    ctx_release(c);
    return rc;
}

int oemgpu_selftest_logistic_plan(int64_t n, int32_t p, int32_t intercept, int32_t hessian_full, int32_t num_cu, int64_t *out)
{
    if (n < 1 || p < 1 || num_cu < 1 || !out || (hessian_full != 0 && hessian_full != 1)) { set_error("selftest_logistic_plan: bad argument"); return OEMGPU_ERR_ARG; }
    const LogitPlan P = logit_plan(n, p, intercept, num_cu);
    const int q = p + (intercept ? 1 : 0);
    out[0] = P.ch; out[1] = P.nchunk; out[2] = P.rbz; out[3] = P.nzblk; out[4] = P.inner_wg; out[5] = P.staged;
    out[6] = (int64_t)P.ws_bytes;
    // the bound: the fixed pieces (q^2 matrices, chunk partials, moments) plus a Z block of at most LOGIT_Z_BYTES or one chunk of rows
    const size_t zb = std::max(LOGIT_Z_BYTES, (size_t)P.ch * q * 8);
    out[7] = (int64_t)(zb + 8 * ((size_t)q * q * 2 + (size_t)(q + 2) * (q + 2) * 2 + (size_t)P.nchunk * (p + 2) + 16 * (size_t)q + (size_t)p + 64) +
                       8 * (gram_plan_bound(P.rbz < n ? P.rbz : n, q, num_cu).tpart_doubles + gram_plan_bound(P.rbz < n ? P.rbz : n, q, num_cu).vpart_doubles) + 64 * 256);
    (void)hessian_full;
    return 0;
}

int oemgpu_last_logistic_stats(double *out)
{
    if (!out) { set_error("last_logistic_stats: NULL"); return OEMGPU_ERR_ARG; }
    const LogitStats &s = g_logit_stats;
    out[0] = s.ms_rows; out[1] = s.ms_gram; out[2] = s.ms_inner; out[3] = s.irls_steps; out[4] = s.inner_iters; out[5] = s.row_passes;
    out[6] = s.grams; out[7] = s.wall_ms;
    return 0;
}

#pragma GCC visibility pop
}
