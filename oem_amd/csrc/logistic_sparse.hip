// logistic_sparse.hip -- the sparse binomial fit: what `.Call("oem_fit_logistic_sparse", ...)` computes on a dgCMatrix x (ref
// src/oem_logistic_sparse.cpp:30-313, src/oem_logistic_sparse.h), restated as it is.  The IRLS driver, the inner OEM loop and its
// operators are the dense fit's (logistic.hip: logistic_irls); what differs is here:
//   * the single-thread branch of solve() (ncores = 1, R's default; cpp :88, 107-110; h :869-891): eta = X (beta_tail o s) + beta_0
//     with an intercept (standardize), X (beta o s) or X beta without one.  An intercept without standardize reads colsq_inv, which
//     the reference never wrote (h :724, :880): refused;
//   * s = 1 / sqrt(colsq), colsq = sum x^2 / (n - 1) over the stored values, 0 -> 1, only when standardize (h :735-750); X not centred;
//   * the Hessian at EVERY IRLS step except the skipped first step of a later lambda (h :866, :973; hessian.type is never read);
//   * XX with an intercept (h :456-528): XX[1:, 1:] = S X'WX S, colsums = (X'W) o s (W, not sqrt W); at the first Hessian build
//     xxdiag = mean diag XX[1:, 1:] and intval = sqrt((xxdiag / sum W) / n), recomputed only while xxdiag <= 0 (init_oem, once per
//     call, is the only reset); XX[0, 1:] = intval colsums, XX[0, 0] = xxdiag; then XX /= n;
//   * the first XY's intercept slot is sum y * intval = 0 (intval is still 0 there, h :731-732, :767);
//   * get_beta (h :1040-1062) does beta_0 *= intval on the solver's own beta after every lambda: the next lambda warm-starts from it.
// Refused besides (api: OEMGPU_ERR_UNSUPPORTED): p + intercept >= n (the XWXt branch never forms grad or XY, h :497-502, :978) and
// p > LOGIT_P_LIMIT.
//
// Kernels, once per call: the column scales (one workgroup per column, fixed order); a compressed-ROW copy whose rows hold their
// entries in column order (sparse.hip: csc_to_csr_kernel over the chunk pointers of csc_chunk_ptr_kernel).  At every IRLS step:
//   * lsp_rows_kernel: a thread per row over the row copy (beta o s staged in LDS) forms eta, prob, W (with the floor quirk),
//     r = y - prob and the loss terms; writes W and r and the chunk partials of [sum r, sum W, sum loss];
//   * lsp_cols_kernel: a workgroup per column reads its non-zeros once: X'r and X'W, fixed-order sums; one more workgroup adds the
//     row partials in chunk order;
//   * the weighted Gram X'WX on the route the Gaussian sparse fit takes too (sparse.hip: sparse_route): the compressed-column kernel
//     with the row weight gathered at its scatter (csc_gram_kernel<true>), or csc_tile_moments over zero-filled row tiles of sqrt(W) x;
//   * lsp_intval_kernel + lsp_xx_kernel: xxdiag / intval and XX.
// No float atomics anywhere: two calls give the same bits.
#include "logistic.hpp"

#include <cmath>
#include <vector>

namespace oemgpu {

namespace {

enum { SW_XXDIAG = 0, SW_INTVAL = 1, SW_SUMW = 2, SW_LEN = 4 };    // device words of the sparse fit

// colsq = sum x^2 / (n - 1) over a column's stored values, 0 -> 1, s = 1 / sqrt(colsq) (h :735-750); one workgroup per column
__global__ __launch_bounds__(256) void lsp_scale_kernel(const int64_t *__restrict__ colptr, const double *__restrict__ val, int64_t n,
                                                        double *__restrict__ s)
{
    __shared__ double red[256];
    const int j = blockIdx.x;
    double a = 0.0;
    for (int64_t k = colptr[j] + threadIdx.x; k < colptr[j + 1]; k += 256) a = fma(val[k], val[k], a);
    red[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < 256; ++k) t += red[k];
        double cs = t / ((double)n - 1.0);
        if (cs == 0.0) cs = 1.0;
        s[j] = 1.0 / sqrt(cs);
    }
}

// the row pass: workgroup c owns rows [c ch, (c + 1) ch), a thread per row (rows tid, tid + 256, ...), the row's entries in column order
__global__ __launch_bounds__(256) void lsp_rows_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ ccol, const double *__restrict__ cval,
                                                       int64_t n, int p, const double *__restrict__ y, const double *__restrict__ beta,
                                                       const double *__restrict__ s, int intercept, int64_t irls_i, int64_t ch,
                                                       double *__restrict__ wout, double *__restrict__ rout, double *__restrict__ part)
{
    extern __shared__ double bs[];                     // p: beta o s
    __shared__ double red[3][256];
    const int tid = threadIdx.x, o = intercept ? 1 : 0;
    for (int j = tid; j < p; j += 256) bs[j] = beta[o + j] * s[j];
    const double b0 = intercept ? beta[0] : 0.0;
    __syncthreads();
    const int64_t c = blockIdx.x, r_lo = c * ch, r_hi = (r_lo + ch < n) ? r_lo + ch : n;
    double rs = 0.0, ws = 0.0, ls = 0.0;
    for (int64_t row = r_lo + tid; row < r_hi; row += 256) {
        double e = 0.0;
        for (int64_t k = rowptr[row]; k < rowptr[row + 1]; ++k) e = fma(cval[k], bs[ccol[k]], e);
        const double eta = e + b0;
        const double prob = 1.0 / (1.0 + exp(-eta));
        double W = prob * (1.0 - prob);
        if (row == irls_i && W < 1e-5) W = 1e-5;          // the floor loop tests W(i), i the IRLS index (h :963-969)
        const double yi = y[row], r = yi - prob;
        double lt;
        if (yi == 1.0) lt = prob > 1e-5 ? log(1.0 / prob) : log(1.0 / 1e-5);
        else lt = prob <= 1.0 - 1e-5 ? log(1.0 / (1.0 - prob)) : log(1.0 / 1e-5);
        wout[row] = W; rout[row] = r;
        rs += r; ws += W; ls += lt;
    }
    red[0][tid] = rs; red[1][tid] = ws; red[2][tid] = ls;
    __syncthreads();
    if (tid < 3) {
        double a = 0.0;
        for (int i = 0; i < 256; ++i) a += red[tid][i];
        part[(size_t)c * 3 + tid] = a;
    }
}

// the column pass: workgroup j < p: g[1 + j] = sum val r[row] (X'r, or X'Y when r = y), cw[j] = sum val w[row] (X'W; w may be null);
// workgroup p: the row partials in chunk order -> g[0] = sum r, sw[SW_SUMW] = sum W, g[p + 1] = sum loss (init: g[0] = 0, the first
// XY's intercept slot sum y * intval with intval = 0)
__global__ __launch_bounds__(256) void lsp_cols_kernel(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rowidx, const double *__restrict__ val,
                                                       int p, const double *__restrict__ r, const double *__restrict__ w, const double *__restrict__ part,
                                                       int64_t nchunk, int init, double *__restrict__ g, double *__restrict__ cw, double *__restrict__ sw)
{
    __shared__ double red[2][256];
    const int j = blockIdx.x, tid = threadIdx.x;
    if (j == p) {
        if (tid == 0) {
            if (init) { g[0] = 0.0; g[p + 1] = 0.0; return; }
            double a = 0.0, b = 0.0, l = 0.0;
            for (int64_t c = 0; c < nchunk; ++c) { a += part[(size_t)c * 3]; b += part[(size_t)c * 3 + 1]; l += part[(size_t)c * 3 + 2]; }
            g[0] = a; sw[SW_SUMW] = b; g[p + 1] = l;
        }
        return;
    }
    double a = 0.0, b = 0.0;
    for (int64_t k = colptr[j] + tid; k < colptr[j + 1]; k += 256) {
        const double v = val[k];
        const int32_t i = rowidx[k];
        a = fma(v, r[i], a);
        if (w) b = fma(v, w[i], b);
    }
    red[0][tid] = a; red[1][tid] = b;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) { red[0][tid] += red[0][tid + h]; red[1][tid] += red[1][tid + h]; }
        __syncthreads();
    }
    if (tid == 0) { g[1 + j] = red[0][0]; if (w) cw[j] = red[1][0]; }
}

// xxdiag = mean diag (S X'WX S) and intval = sqrt((xxdiag / sum W) / n), only while xxdiag <= 0 (h :477-481).  One workgroup.
__global__ __launch_bounds__(256) void lsp_intval_kernel(const double *__restrict__ M, int p, const double *__restrict__ s, double n,
                                                         double *__restrict__ sw)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double a = 0.0;
    for (int j = tid; j < p; j += 256) a += (s[j] * M[(size_t)j * (p + 2) + j]) * s[j];
    red[tid] = a;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int k = 0; k < 256; ++k) t += red[k];
        if (sw[SW_XXDIAG] <= 0.0) {
            const double xxdiag = t / (double)p;
            sw[SW_XXDIAG] = xxdiag;
            sw[SW_INTVAL] = sqrt((xxdiag / sw[SW_SUMW]) / n);
        }
    }
}

// XX (q x q, column-major) = [xxdiag, intval colsums'; intval colsums, S G S] / n, G = X'WX from the moment buffer M ((p + 2)^2)
__global__ __launch_bounds__(256) void lsp_xx_kernel(const double *__restrict__ M, int p, int intercept, const double *__restrict__ s,
                                                     const double *__restrict__ cw, const double *__restrict__ sw, double n, double *__restrict__ xx)
{
    const int o = intercept ? 1 : 0, q = p + o;
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= q) return;
    double v;
    if (o && i == 0 && j == 0) v = sw[SW_XXDIAG];
    else if (o && (i == 0 || j == 0)) { const int k = (i > j ? i : j) - 1; v = (cw[k] * s[k]) * sw[SW_INTVAL]; }
    else {
        const int a = i - o, b = j - o, lo = a < b ? a : b, hi = a < b ? b : a;
        v = (s[a] * M[(size_t)lo * (p + 2) + hi]) * s[b];
    }
    xx[(size_t)j * q + i] = v / n;
}

__global__ void lsp_zero_words_kernel(double *sw) { if (threadIdx.x < SW_LEN) sw[threadIdx.x] = 0.0; }

}  // namespace

// the plan of a call: the Gram route, the row pass's chunks, the tile rows, the workspace
struct LspPlan {
    int csc;           // 1: compressed-column weighted Gram; 0: zero-filled row tiles through the MFMA moment pass
    int inner_wg;      // 1: the inner solve is one persistent workgroup; 0: launch form
    int64_t ch;        // rows per row-pass workgroup (a multiple of 64)
    int64_t nchunk;    // row-pass workgroups
    int64_t rcrows;    // tile route: rows per tile (0 on the csc route)
    int64_t ld;        // tile route: the tile's leading dimension
    size_t ws_bytes;   // the fit's own workspace (the driver's pieces come on top: q^2 matrices, the output)
    size_t bound;      // ws_bytes stays within this
};

// the workspace of the fit, piece by piece (offsets into it when off != null)
static size_t lsp_layout(const LspPlan &P, int64_t n, int p, int64_t nnz, int num_cu, size_t *off)
{
    Bump B;
    const size_t m2 = (size_t)(p + 2) * (p + 2);
    size_t t[20];
    int k = 0;
    t[k++] = B.take(8 * (size_t)(p + 1));                   // 0 colptr
    t[k++] = B.take(4 * (size_t)(nnz + 1));                 // 1 rowidx
    t[k++] = B.take(8 * (size_t)(nnz + 1));                 // 2 values
    t[k++] = B.take(8 * (size_t)n);                         // 3 y
    t[k++] = B.take(8 * (size_t)(n + 1));                   // 4 rowptr of the row copy
    t[k++] = B.take(4 * (size_t)(nnz + 1));                 // 5 its columns
    t[k++] = B.take(8 * (size_t)(nnz + 1));                 // 6 its values
    t[k++] = B.take(4 * (size_t)(csc_chunks(n) + 1) * p);   // 7 chunk pointers
    t[k++] = B.take(8 * (size_t)n);                         // 8 W
    t[k++] = B.take(8 * (size_t)n);                         // 9 r
    t[k++] = B.take(8 * 3 * (size_t)P.nchunk);              // 10 row partials
    t[k++] = B.take(8 * (size_t)p);                         // 11 X'W
    t[k++] = B.take(8 * SW_LEN);                            // 12 xxdiag, intval, sum W
    t[k++] = B.take(8 * m2);                                // 13 moments (of a tile)
    t[k++] = B.take(P.csc ? 0 : 8 * m2);                    // 14 tile route: their running sum
    if (P.csc) {
        t[k++] = B.take(csc_wgram_work_bytes(n, p));        // 15 range sums
        t[k++] = B.take(0); t[k++] = B.take(0);
    } else {
        const GramPlan gpb = gram_plan_bound(P.rcrows, p, num_cu);
        t[k++] = B.take(8 * (size_t)P.ld * p);              // 15 the tile
        t[k++] = B.take(8 * gpb.tpart_doubles);             // 16
        t[k++] = B.take(8 * gpb.vpart_doubles);             // 17
    }
    if (off) for (int i = 0; i < k; ++i) off[i] = t[i];
    return B.off;
}

static LspPlan lsp_plan(int64_t n, int p, int64_t nnz, int intercept, int num_cu)
{
    LspPlan P;
    const int q = p + (intercept ? 1 : 0);
    const SparseRoute R = sparse_route(n, p, nnz);
    P.csc = R.csc;
    P.inner_wg = q <= LOGIT_WG_MAX_Q;
    int64_t ch = (n + 4 * (int64_t)num_cu - 1) / (4 * (int64_t)num_cu);
    ch = (ch + 63) / 64 * 64;
    if (ch < 64) ch = 64;
    P.ch = ch;
    P.nchunk = (n + ch - 1) / ch;
    P.rcrows = P.csc ? 0 : R.rows;
    P.ld = P.csc ? 0 : R.ld;
    P.ws_bytes = lsp_layout(P, n, p, nnz, num_cu, nullptr);
    // the bound: 40 bytes a row, 24 a non-zero, the chunk pointers, the moments, and a Gram scratch that does not grow with n
    // (csc: the range sums, at most 256 MB or one p x p; tiles: at most 2 GiB or 64 rows, with their MFMA partials)
    size_t gram;
    if (P.csc) gram = std::max((size_t)256000000, (size_t)8 * p * p);
    else {
        const GramPlan gpb = gram_plan_bound(P.rcrows, p, num_cu);
        gram = std::max((size_t)2147483648ull, (size_t)8 * 66 * p) + 8 * (gpb.tpart_doubles + gpb.vpart_doubles) + 8 * (size_t)(p + 2) * (p + 2);
    }
    P.bound = 40 * (size_t)(n + 1) + 24 * (size_t)(nnz + 1) + 4 * (size_t)(csc_chunks(n) + 1) * p + 24 * (size_t)P.nchunk + 8 * (size_t)(p + 2) * (p + 2) +
              8 * (size_t)(2 * p + 1) + gram + 20 * 256;
    return P;
}

namespace {

struct SparseLogitData final : LogitData {
    oemgpu_ctx *c;
    int64_t n, nnz, maxcol;
    int p, q, intercept, standardize;
    const int64_t *h_colptr, *h_rowptr;
    const int32_t *h_rowidx;
    const double *h_val, *h_y;
    LspPlan P;
    int64_t *colptr = nullptr, *rowptr = nullptr;
    int32_t *rowidx = nullptr, *ccol = nullptr, *cptr = nullptr;
    double *val = nullptr, *y = nullptr, *cval = nullptr, *W = nullptr, *r = nullptr, *part = nullptr, *cw = nullptr, *swd = nullptr,
           *mb = nullptr, *ma = nullptr, *gw = nullptr, *tile = nullptr, *tp = nullptr, *vp = nullptr;

    size_t ws_bytes() const override { return P.ws_bytes; }
    int bind(char *ws) override
    {
        size_t o[20];
        lsp_layout(P, n, p, nnz, c->num_cu, o);
        colptr = (int64_t *)(ws + o[0]); rowidx = (int32_t *)(ws + o[1]); val = (double *)(ws + o[2]); y = (double *)(ws + o[3]);
        rowptr = (int64_t *)(ws + o[4]); ccol = (int32_t *)(ws + o[5]); cval = (double *)(ws + o[6]); cptr = (int32_t *)(ws + o[7]);
        W = (double *)(ws + o[8]); r = (double *)(ws + o[9]); part = (double *)(ws + o[10]); cw = (double *)(ws + o[11]); swd = (double *)(ws + o[12]);
        mb = (double *)(ws + o[13]); ma = (double *)(ws + o[14]);
        if (P.csc) gw = (double *)(ws + o[15]);
        else { tile = (double *)(ws + o[15]); tp = (double *)(ws + o[16]); vp = (double *)(ws + o[17]); }
        intval = swd + SW_INTVAL;
        hipStream_t s = c->stream;
        OEM_HIP(hipMemcpyAsync(colptr, h_colptr, 8 * (size_t)(p + 1), hipMemcpyHostToDevice, s));
        if (nnz > 0) {
            OEM_HIP(hipMemcpyAsync(rowidx, h_rowidx, 4 * (size_t)nnz, hipMemcpyHostToDevice, s));
            OEM_HIP(hipMemcpyAsync(val, h_val, 8 * (size_t)nnz, hipMemcpyHostToDevice, s));
        }
        OEM_HIP(hipMemcpyAsync(y, h_y, 8 * (size_t)n, hipMemcpyHostToDevice, s));
        OEM_HIP(hipMemcpyAsync(rowptr, h_rowptr, 8 * (size_t)(n + 1), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(lsp_zero_words_kernel, dim3(1), dim3(64), 0, s, swd);            // init_oem: xxdiag = intval = 0 (h :731-732)
        OEM_HIP(hipGetLastError());
        int rc = launch_csc_chunk_ptr(s, colptr, rowidx, n, p, cptr);
        if (!rc) rc = launch_csc_to_csr(s, colptr, rowidx, val, cptr, n, p, rowptr, ccol, cval);
        return rc;
    }
    int scale(double *sc) override
    {
        if (!standardize) return launch_logit_fill(c->stream, sc, p, 1.0);
        hipLaunchKernelGGL(lsp_scale_kernel, dim3(p), dim3(256), 0, c->stream, colptr, val, n, sc);
        OEM_HIP(hipGetLastError());
        return 0;
    }
    int xy0(const double *, double *g) override
    {
        hipLaunchKernelGGL(lsp_cols_kernel, dim3(p + 1), dim3(256), 0, c->stream, colptr, rowidx, val, p, y, nullptr, part, P.nchunk, 1, g, cw, swd);
        OEM_HIP(hipGetLastError());
        return 0;
    }
    int rows(const double *beta, const double *sc, int64_t i, bool, double *g) override
    {
        hipStream_t s = c->stream;
        const size_t lds = 8 * (size_t)p;
        if (lds_limit_once(reinterpret_cast<const void *>(&lsp_rows_kernel), lds)) return OEMGPU_ERR_HIP;
        hipLaunchKernelGGL(lsp_rows_kernel, dim3((unsigned)P.nchunk), dim3(256), lds, s, rowptr, ccol, cval, n, p, y, beta, sc, intercept, i, P.ch, W, r, part);
        hipLaunchKernelGGL(lsp_cols_kernel, dim3(p + 1), dim3(256), 0, s, colptr, rowidx, val, p, r, W, part, P.nchunk, 0, g, cw, swd);
        OEM_HIP(hipGetLastError());
        return 0;
    }
    int hessian(const double *, const double *sc, int64_t, double *, double *xx) override
    {
        hipStream_t s = c->stream;
        const SparseRoute R{false, P.rcrows, P.ld};
        const int rc = P.csc ? launch_csc_wgram(s, colptr, rowidx, val, W, cptr, n, p, gw, mb)
                             : csc_tile_moments(c, R, colptr, rowidx, val, W, nullptr, n, p, maxcol, tile, tp, vp, mb, ma);
        if (rc) return rc;
        const double *M = P.csc ? mb : ma;
        if (intercept) hipLaunchKernelGGL(lsp_intval_kernel, dim3(1), dim3(256), 0, s, M, p, sc, (double)n, swd);
        hipLaunchKernelGGL(lsp_xx_kernel, dim3((q + 255) / 256, q), dim3(256), 0, s, M, p, intercept, sc, cw, swd, (double)n, xx);
        OEM_HIP(hipGetLastError());
        return 0;
    }
};

}  // namespace

// the checks that need no device: the refusals, then the compressed-column arrays (csc_check); fills the row pointers of the row copy
// and the longest column
static int lsp_check(int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values, int32_t standardize, int32_t intercept,
                     int32_t irls_maxit, double irls_tol, const oemgpu_opts *o, std::vector<int64_t> *rowptr, int64_t *maxcol)
{
    if (n < 1 || p < 1) { set_error("fit_logistic_sparse: bad dimensions"); return OEMGPU_ERR_ARG; }
    if (intercept && !standardize) {
        set_error("fit_logistic_sparse: intercept = TRUE with standardize = FALSE is not supported (the reference scales the linear predictor by "
                  "colsq_inv, which it never computes without standardize: ref src/oem_logistic_sparse.h:724, :880)");
        return OEMGPU_ERR_UNSUPPORTED;
    }
    if ((int64_t)p + (intercept ? 1 : 0) >= n) {
        set_error("fit_logistic_sparse: p + intercept >= n is not supported (the reference's XWXt branch never forms grad or XY, "
                  "ref src/oem_logistic_sparse.h:497-502, :978)");
        return OEMGPU_ERR_UNSUPPORTED;
    }
    if (p > LOGIT_P_LIMIT) { set_error("fit_logistic_sparse: p > %d is not supported", LOGIT_P_LIMIT); return OEMGPU_ERR_UNSUPPORTED; }
    int rc = logistic_check(n, p, intercept, 0, irls_maxit, irls_tol, o);
    if (rc) return rc;
    const int64_t mc = csc_check("fit_logistic_sparse", n, p, colptr, rowidx, values, rowptr);
    if (mc < 0) return (int)mc;
    for (int64_t i = 0; i < n; ++i) (*rowptr)[(size_t)i + 1] += (*rowptr)[(size_t)i];
    *maxcol = mc;
    return 0;
}

}  // namespace oemgpu

using namespace oemgpu;

extern "C" {
#pragma GCC visibility push(default)

int oemgpu_fit_logistic_sparse(int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values, const double *y,
                               int32_t standardize, int32_t intercept, int32_t irls_maxit, double irls_tol, const oemgpu_opts *o,
                               double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    if (!colptr || !y || !o || !beta || !lambda_out || !niter || !loss || !d) { set_error("fit_logistic_sparse: NULL argument"); return OEMGPU_ERR_ARG; }
    std::vector<int64_t> rowptr;
    int64_t maxcol = 0;
    int rc = lsp_check(n, p, colptr, rowidx, values, standardize, intercept, irls_maxit, irls_tol, o, &rowptr, &maxcol);
    if (rc) return rc;
    oemgpu_ctx *c = ctx_acquire(o->device);
    if (!c) return OEMGPU_ERR_NO_DEVICE;
    const int64_t nnz = colptr[p];
    SparseLogitData D;
    D.hess_every = true;                                   // h :866, :973: every step but the skipped first of a later lambda
    D.c = c; D.n = n; D.nnz = nnz; D.maxcol = maxcol; D.p = p; D.q = p + (intercept ? 1 : 0); D.intercept = intercept; D.standardize = standardize;
    D.h_colptr = colptr; D.h_rowptr = rowptr.data(); D.h_rowidx = rowidx; D.h_val = values; D.h_y = y;
    D.P = lsp_plan(n, p, nnz, intercept, c->num_cu);
    rc = logistic_irls(c, D, n, p, intercept, irls_maxit, irls_tol, o, beta, lambda_out, niter, loss, d);
    (void)hipStreamSynchronize(c->stream);
    ctx_release(c);
    return rc;
}

// out[0] route (1 csc, 0 row tiles), [1] inner solve (1 one workgroup, 0 launch form), [2] workspace bytes of the fit's own pieces,
// [3] the bound they stay within, [4] rows per tile (0 on the csc route), [5] row-pass workgroups, [6] rows per row-pass workgroup,
// [7] chunks of the compressed-column kernels
int oemgpu_selftest_logistic_sparse_plan(int64_t n, int32_t p, int64_t nnz, int32_t intercept, int32_t num_cu, int64_t *out)
{
    if (n < 1 || p < 1 || nnz < 0 || num_cu < 1 || !out) { set_error("selftest_logistic_sparse_plan: bad argument"); return OEMGPU_ERR_ARG; }
    const LspPlan P = lsp_plan(n, p, nnz, intercept, num_cu);
    out[0] = P.csc; out[1] = P.inner_wg; out[2] = (int64_t)P.ws_bytes; out[3] = (int64_t)P.bound; out[4] = P.rcrows; out[5] = P.nchunk;
    out[6] = P.ch; out[7] = csc_chunks(n);
    return 0;
}

#pragma GCC visibility pop
}
