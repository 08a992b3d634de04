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
//
// cv.oem on a sparse x (oemgpu_sparse_x_create, oemgpu_fit_logistic_sparse_fold_res; ref R/cv_oem.R:129-175 slices x[!which, ] and calls
// oem()): the compressed columns, their chunk pointers and the row copy are built ONCE into a handle, and SparseLogitData binds to it
// (resident mode: nothing is uploaded or converted, the workspace holds the fit's own pieces only).  A fold fit is the fit on the rows
// with foldid != leave_out of that x: the MASKED column scales sum kept entries only, the MASKED row pass never reads a left-out row
// and writes W = r = 0 there -- so the column pass and both weighted Gram routes run unchanged (fma(v, 0, a) = a for every finite
// stored v) -- and n_eff, the kept rows (logit_fold_scan), stands where n enters the arithmetic; the W floor tests the i-th KEPT row.
#include "logistic.hpp"

#include <cmath>
#include <vector>

namespace oemgpu {

namespace {

enum { SW_XXDIAG = 0, SW_INTVAL = 1, SW_SUMW = 2, SW_LEN = 4 };    // device words of the sparse fit

// colsq = sum x^2 / (n - 1) over a column's stored values, 0 -> 1, s = 1 / sqrt(colsq) (h :735-750); one workgroup per column.
// MASKED (a fold fit): the entries of the kept rows only, n their number -- a column with none of them gets 0 -> 1 as on x[keep, ]
template <bool MASKED>
__global__ __launch_bounds__(256) void lsp_scale_kernel(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rowidx,
                                                        const double *__restrict__ val, int64_t n, double *__restrict__ s,
                                                        const int32_t *__restrict__ foldid, int32_t leave_out)
{
    __shared__ double red[256];
    const int j = blockIdx.x;
    double a = 0.0;
    if (MASKED) {
        for (int64_t k = colptr[j] + threadIdx.x; k < colptr[j + 1]; k += 256)
            if (foldid[rowidx[k]] != leave_out) a = fma(val[k], val[k], a);
    } else {
        for (int64_t k = colptr[j] + threadIdx.x; k < colptr[j + 1]; k += 256) a = fma(val[k], val[k], a);
    }
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

// the row pass: workgroup c owns rows [c ch, (c + 1) ch), a thread per row (rows tid, tid + 256, ...), the row's entries in column order.
// MASKED (a fold fit): a row with foldid[row] == leave_out is not in the fit: neither its entries nor its y are read, W = r = 0 are
// written there and nothing is added to the sums; irls_i is then the row of the i-th KEPT row (-1: none, the floor is off)
template <bool MASKED>
__global__ __launch_bounds__(256) void lsp_rows_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ ccol, const double *__restrict__ cval,
                                                       int64_t n, int p, const double *__restrict__ y, const double *__restrict__ beta,
                                                       const double *__restrict__ s, int intercept, int64_t irls_i, int64_t ch,
                                                       double *__restrict__ wout, double *__restrict__ rout, double *__restrict__ part,
                                                       const int32_t *__restrict__ foldid, int32_t leave_out)
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
        if (MASKED && foldid[row] == leave_out) { wout[row] = 0.0; rout[row] = 0.0; continue; }
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

// a fold fit's X'y: out = kept ? y : 0 (the column pass then runs on it as on r; y of a left-out row is not read)
__global__ __launch_bounds__(256) void lsp_kept_y_kernel(const double *__restrict__ y, const int32_t *__restrict__ foldid, int32_t leave_out, int64_t n,
                                                         double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = foldid[i] != leave_out ? y[i] : 0.0;
}

}  // namespace

// the plan of a call: the Gram route, the row pass's chunks, the tile rows, the workspace
struct LspPlan {
    int csc;           // 1: compressed-column weighted Gram; 0: zero-filled row tiles through the MFMA moment pass
    int inner_wg;      // 1: the inner solve is one persistent workgroup; 0: launch form
    int64_t ch;        // rows per row-pass workgroup (a multiple of 64)
    int64_t nchunk;    // row-pass workgroups
    int64_t rcrows;    // tile route: rows per tile (0 on the csc route)
    int64_t ld;        // tile route: the tile's leading dimension
    int resident;      // 1: x is an oemgpu_sparse_x and y the caller's device vector; the workspace holds the fit's own pieces only
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
    const bool up = !P.resident;                            // pieces 0 .. 7: the handle's (and the caller's y) in resident mode
    t[k++] = B.take(up ? 8 * (size_t)(p + 1) : 0);                   // 0 colptr
    t[k++] = B.take(up ? 4 * (size_t)(nnz + 1) : 0);                 // 1 rowidx
    t[k++] = B.take(up ? 8 * (size_t)(nnz + 1) : 0);                 // 2 values
    t[k++] = B.take(up ? 8 * (size_t)n : 0);                         // 3 y
    t[k++] = B.take(up ? 8 * (size_t)(n + 1) : 0);                   // 4 rowptr of the row copy
    t[k++] = B.take(up ? 4 * (size_t)(nnz + 1) : 0);                 // 5 its columns
    t[k++] = B.take(up ? 8 * (size_t)(nnz + 1) : 0);                 // 6 its values
    t[k++] = B.take(up ? 4 * (size_t)(csc_chunks(n) + 1) * p : 0);   // 7 chunk pointers
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

static LspPlan lsp_plan(int64_t n, int p, int64_t nnz, int intercept, int num_cu, bool resident = false)
{
    LspPlan P;
    P.resident = resident ? 1 : 0;
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
    const int64_t *h_colptr = nullptr, *h_rowptr = nullptr;
    const int32_t *h_rowidx = nullptr;
    const double *h_val = nullptr, *h_y = nullptr;
    const oemgpu_sparse_x *res = nullptr;   // resident mode: the arrays are the handle's, y_res the caller's device y
    const double *y_res = nullptr;
    const int32_t *foldid = nullptr;        // a fold fit (resident mode): device, n entries; null: every row is in the fit
    int32_t leave_out = 0;
    int64_t n_eff = 0;                      // rows in the fit
    std::vector<int64_t> kept_row;          // fold fit: the row of the k-th kept row, k < min(irls_maxit, n_eff)
    LspPlan P;
    const int64_t *colptr = nullptr, *rowptr = nullptr;
    const int32_t *rowidx = nullptr, *ccol = nullptr, *cptr = nullptr;
    const double *val = nullptr, *y = nullptr, *cval = nullptr;
    double *W = nullptr, *r = nullptr, *part = nullptr, *cw = nullptr, *swd = nullptr,
           *mb = nullptr, *ma = nullptr, *gw = nullptr, *tile = nullptr, *tp = nullptr, *vp = nullptr;

    // The row whose W the floor tests at IRLS step i (h :963-969 tests W(i) of the rows it was given)
    int64_t floor_row(int64_t i) const { return foldid ? (i < (int64_t)kept_row.size() ? kept_row[(size_t)i] : -1) : i; }
    size_t ws_bytes() const override { return P.ws_bytes; }
    int bind(char *ws) override
    {
        size_t o[20];
        lsp_layout(P, n, p, nnz, c->num_cu, o);
        W = (double *)(ws + o[8]); r = (double *)(ws + o[9]); part = (double *)(ws + o[10]); cw = (double *)(ws + o[11]); swd = (double *)(ws + o[12]);
        mb = (double *)(ws + o[13]); ma = (double *)(ws + o[14]);
        if (P.csc) gw = (double *)(ws + o[15]);
        else { tile = (double *)(ws + o[15]); tp = (double *)(ws + o[16]); vp = (double *)(ws + o[17]); }
        intval = swd + SW_INTVAL;
        hipStream_t s = c->stream;
        if (res) {                                        // nothing to upload, nothing to convert
            colptr = res->colptr; rowidx = res->rowidx; val = res->val; y = y_res;
            rowptr = res->rowptr; ccol = res->ccol; cval = res->cval; cptr = res->cptr;
            hipLaunchKernelGGL(lsp_zero_words_kernel, dim3(1), dim3(64), 0, s, swd);        // init_oem: xxdiag = intval = 0 (h :731-732)
            OEM_HIP(hipGetLastError());
            return 0;
        }
        int64_t *d_colptr = (int64_t *)(ws + o[0]), *d_rowptr = (int64_t *)(ws + o[4]);
        int32_t *d_rowidx = (int32_t *)(ws + o[1]), *d_ccol = (int32_t *)(ws + o[5]), *d_cptr = (int32_t *)(ws + o[7]);
        double *d_val = (double *)(ws + o[2]), *d_y = (double *)(ws + o[3]), *d_cval = (double *)(ws + o[6]);
        colptr = d_colptr; rowidx = d_rowidx; val = d_val; y = d_y; rowptr = d_rowptr; ccol = d_ccol; cval = d_cval; cptr = d_cptr;
        OEM_HIP(hipMemcpyAsync(d_colptr, h_colptr, 8 * (size_t)(p + 1), hipMemcpyHostToDevice, s));
        if (nnz > 0) {
            OEM_HIP(hipMemcpyAsync(d_rowidx, h_rowidx, 4 * (size_t)nnz, hipMemcpyHostToDevice, s));
            OEM_HIP(hipMemcpyAsync(d_val, h_val, 8 * (size_t)nnz, hipMemcpyHostToDevice, s));
        }
        OEM_HIP(hipMemcpyAsync(d_y, h_y, 8 * (size_t)n, hipMemcpyHostToDevice, s));
        OEM_HIP(hipMemcpyAsync(d_rowptr, h_rowptr, 8 * (size_t)(n + 1), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(lsp_zero_words_kernel, dim3(1), dim3(64), 0, s, swd);            // init_oem: xxdiag = intval = 0 (h :731-732)
        OEM_HIP(hipGetLastError());
        int rc = launch_csc_chunk_ptr(s, d_colptr, d_rowidx, n, p, d_cptr);
        if (!rc) rc = launch_csc_to_csr(s, d_colptr, d_rowidx, d_val, d_cptr, n, p, d_rowptr, d_ccol, d_cval);
        return rc;
    }
    int scale(double *sc) override
    {
        if (!standardize) return launch_logit_fill(c->stream, sc, p, 1.0);
        if (foldid) hipLaunchKernelGGL(lsp_scale_kernel<true>, dim3(p), dim3(256), 0, c->stream, colptr, rowidx, val, n_eff, sc, foldid, leave_out);
        else hipLaunchKernelGGL(lsp_scale_kernel<false>, dim3(p), dim3(256), 0, c->stream, colptr, rowidx, val, n, sc, nullptr, 0);
        OEM_HIP(hipGetLastError());
        return 0;
    }
    int xy0(const double *, double *g) override
    {
        const double *yk = y;
        if (foldid) {                                      // kept ? y : 0 into the r buffer, which the first row pass overwrites
            hipLaunchKernelGGL(lsp_kept_y_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, y, foldid, leave_out, n, r);
            yk = r;
        }
        hipLaunchKernelGGL(lsp_cols_kernel, dim3(p + 1), dim3(256), 0, c->stream, colptr, rowidx, val, p, yk, nullptr, part, P.nchunk, 1, g, cw, swd);
        OEM_HIP(hipGetLastError());
        return 0;
    }
    int rows(const double *beta, const double *sc, int64_t i, bool, double *g) override
    {
        hipStream_t s = c->stream;
        const size_t lds = 8 * (size_t)p;
        if (foldid) {
            if (lds_limit_once(reinterpret_cast<const void *>(&lsp_rows_kernel<true>), lds)) return OEMGPU_ERR_HIP;
            hipLaunchKernelGGL(lsp_rows_kernel<true>, dim3((unsigned)P.nchunk), dim3(256), lds, s, rowptr, ccol, cval, n, p, y, beta, sc, intercept,
                               floor_row(i), P.ch, W, r, part, foldid, leave_out);
        } else {
            if (lds_limit_once(reinterpret_cast<const void *>(&lsp_rows_kernel<false>), lds)) return OEMGPU_ERR_HIP;
            hipLaunchKernelGGL(lsp_rows_kernel<false>, dim3((unsigned)P.nchunk), dim3(256), lds, s, rowptr, ccol, cval, n, p, y, beta, sc, intercept, i,
                               P.ch, W, r, part, nullptr, 0);
        }
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
        const double ne = (double)(foldid ? n_eff : n);
        if (intercept) hipLaunchKernelGGL(lsp_intval_kernel, dim3(1), dim3(256), 0, s, M, p, sc, ne, swd);
        hipLaunchKernelGGL(lsp_xx_kernel, dim3((q + 255) / 256, q), dim3(256), 0, s, M, p, intercept, sc, cw, swd, ne, xx);
        OEM_HIP(hipGetLastError());
        return 0;
    }
};

}  // namespace

// the refusals that need neither a device nor the arrays, in `who`'s name
static int lsp_check_fit(const char *who, int64_t n, int32_t p, int32_t standardize, int32_t intercept, int32_t irls_maxit, double irls_tol,
                         const oemgpu_opts *o)
{
    if (n < 1 || p < 1) { set_error("%s: bad dimensions", who); return OEMGPU_ERR_ARG; }
    if (intercept && !standardize) {
        set_error("%s: intercept = TRUE with standardize = FALSE is not supported (the reference scales the linear predictor by "
                  "colsq_inv, which it never computes without standardize: ref src/oem_logistic_sparse.h:724, :880)", who);
        return OEMGPU_ERR_UNSUPPORTED;
    }
    if ((int64_t)p + (intercept ? 1 : 0) >= n) {
        set_error("%s: p + intercept >= n is not supported (the reference's XWXt branch never forms grad or XY, "
                  "ref src/oem_logistic_sparse.h:497-502, :978)", who);
        return OEMGPU_ERR_UNSUPPORTED;
    }
    if (p > LOGIT_P_LIMIT) { set_error("%s: p > %d is not supported", who, LOGIT_P_LIMIT); return OEMGPU_ERR_UNSUPPORTED; }
    return logistic_check(n, p, intercept, 0, irls_maxit, irls_tol, o);
}

// the compressed-column arrays (csc_check): fills the row pointers of the row copy and the longest column
static int lsp_check_csc(const char *who, int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values,
                         std::vector<int64_t> *rowptr, int64_t *maxcol)
{
    const int64_t mc = csc_check(who, n, p, colptr, rowidx, values, rowptr);
    if (mc < 0) return (int)mc;
    for (int64_t i = 0; i < n; ++i) (*rowptr)[(size_t)i + 1] += (*rowptr)[(size_t)i];
    *maxcol = mc;
    return 0;
}

// the handle itself from arrays csc_check has passed: rowptr the row pointers of the row copy (n + 1), maxcol the longest column.
// h_ccol / h_cval: the row copy made by the caller on the host (every row's entries in column order), or null: csc_to_csr_kernel
// makes it -- one workgroup per 8192 rows walking the columns in turn, which a wide x (few rows, very many columns) would wait on
int sparse_x_build(oemgpu_ctx *c, int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values,
                   const std::vector<int64_t> &rowptr, int64_t maxcol, oemgpu_sparse_x **out, const int32_t *h_ccol, const double *h_cval)
{
    *out = nullptr;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const int64_t nnz = colptr[p];
    Bump B;
    const size_t a_cp = B.take(8 * (size_t)(p + 1)), a_ri = B.take(4 * (size_t)(nnz + 1)), a_v = B.take(8 * (size_t)(nnz + 1)),
                 a_rp = B.take(8 * (size_t)(n + 1)), a_cc = B.take(4 * (size_t)(nnz + 1)), a_cv = B.take(8 * (size_t)(nnz + 1)),
                 a_ch = B.take(4 * (size_t)(csc_chunks(n) + 1) * p);
    oemgpu_sparse_x *x = new oemgpu_sparse_x;
    x->device = c->device; x->n = n; x->p = p; x->nnz = nnz; x->maxcol = maxcol; x->bytes = B.off;
    if (hipMalloc((void **)&x->base, B.off) != hipSuccess) {
        set_error("sparse_x_create: cannot allocate %zu bytes of device memory", B.off);
        delete x;
        return OEMGPU_ERR_HIP;
    }
    g_alloc_count += 1;
    x->colptr = (int64_t *)(x->base + a_cp); x->rowidx = (int32_t *)(x->base + a_ri); x->val = (double *)(x->base + a_v);
    x->rowptr = (int64_t *)(x->base + a_rp); x->ccol = (int32_t *)(x->base + a_cc); x->cval = (double *)(x->base + a_cv);
    x->cptr = (int32_t *)(x->base + a_ch);
    hipStream_t s = c->stream;
    auto build = [&]() -> int {
        OEM_HIP(hipMemcpyAsync(x->colptr, colptr, 8 * (size_t)(p + 1), hipMemcpyHostToDevice, s));
        if (nnz > 0) {
            OEM_HIP(hipMemcpyAsync(x->rowidx, rowidx, 4 * (size_t)nnz, hipMemcpyHostToDevice, s));
            OEM_HIP(hipMemcpyAsync(x->val, values, 8 * (size_t)nnz, hipMemcpyHostToDevice, s));
        }
        OEM_HIP(hipMemcpyAsync(x->rowptr, rowptr.data(), 8 * (size_t)(n + 1), hipMemcpyHostToDevice, s));
        int r = launch_csc_chunk_ptr(s, x->colptr, x->rowidx, n, p, x->cptr);
        if (!r && h_ccol && h_cval) {
            if (nnz > 0) {
                OEM_HIP(hipMemcpyAsync(x->ccol, h_ccol, 4 * (size_t)nnz, hipMemcpyHostToDevice, s));
                OEM_HIP(hipMemcpyAsync(x->cval, h_cval, 8 * (size_t)nnz, hipMemcpyHostToDevice, s));
            }
        } else if (!r) r = launch_csc_to_csr(s, x->colptr, x->rowidx, x->val, x->cptr, n, p, x->rowptr, x->ccol, x->cval);
        if (r) return r;
        OEM_HIP(hipStreamSynchronize(s));                  // the host arrays (rowptr among them) may go once this returns
        return 0;
    };
    const int rc = build();
    if (rc) { (void)hipStreamSynchronize(s); (void)hipFree(x->base); delete x; return rc; }
    *out = x;
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
    int rc = lsp_check_fit("fit_logistic_sparse", n, p, standardize, intercept, irls_maxit, irls_tol, o);
    if (!rc) rc = lsp_check_csc("fit_logistic_sparse", n, p, colptr, rowidx, values, &rowptr, &maxcol);
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

int oemgpu_sparse_x_create(oemgpu_ctx *c, int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values,
                           oemgpu_sparse_x **out)
{
    if (out) *out = nullptr;
    if (!c || !colptr || !out) { set_error("sparse_x_create: NULL argument"); return OEMGPU_ERR_ARG; }
    if (n < 1 || p < 1) { set_error("sparse_x_create: bad dimensions"); return OEMGPU_ERR_ARG; }
    std::vector<int64_t> rowptr;
    int64_t maxcol = 0;
    int rc = lsp_check_csc("sparse_x_create", n, p, colptr, rowidx, values, &rowptr, &maxcol);
    if (rc) return rc;
    return sparse_x_build(c, n, p, colptr, rowidx, values, rowptr, maxcol, out);
}

void oemgpu_sparse_x_destroy(oemgpu_sparse_x *x)
{
    if (!x) return;
    int cur = 0;
    const bool sw_dev = hipGetDevice(&cur) == hipSuccess && cur != x->device && hipSetDevice(x->device) == hipSuccess;
    (void)hipFree(x->base);                                // (synchronises with the device: nothing still reads the arrays)
    if (sw_dev) (void)hipSetDevice(cur);
    delete x;
}

int64_t oemgpu_sparse_x_bytes(const oemgpu_sparse_x *x) { return x ? (int64_t)x->bytes : 0; }

int oemgpu_fit_logistic_sparse_fold_res(oemgpu_ctx *c, const oemgpu_sparse_x *x, const double *y_dev, const int32_t *foldid_dev, int32_t nfolds,
                                        int32_t leave_out, int32_t standardize, int32_t intercept, int32_t irls_maxit, double irls_tol,
                                        const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    static const char *who = "fit_logistic_sparse_fold";
    if (!c || !x || !y_dev || !o || !beta || !lambda_out || !niter || !loss || !d) { set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG; }
    if (nfolds < 3) { set_error("nfolds must be bigger than 3; nfolds=10 recommended"); return OEMGPU_ERR_ARG; }            // ref R/cv_oem.R:126-127
    if (leave_out < 0 || leave_out > nfolds) { set_error("%s: leave_out must be in [0, nfolds]", who); return OEMGPU_ERR_ARG; }
    if (leave_out > 0 && !foldid_dev) { set_error("%s: NULL foldid with leave_out > 0", who); return OEMGPU_ERR_ARG; }
    int rc = lsp_check_fit(who, x->n, x->p, standardize, intercept, irls_maxit, irls_tol, o);
    if (rc) return rc;
    if (c->device != x->device) { set_error("%s: the context and the sparse x are on different devices", who); return OEMGPU_ERR_ARG; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const int64_t n = x->n;
    const int p = x->p;
    SparseLogitData D;
    D.hess_every = true;
    D.c = c; D.n = n; D.nnz = x->nnz; D.maxcol = x->maxcol; D.p = p; D.q = p + (intercept ? 1 : 0); D.intercept = intercept; D.standardize = standardize;
    D.res = x; D.y_res = y_dev; D.n_eff = n;
    if (foldid_dev) {                                      // the ids' range whatever is left out; the masks only with a fold to leave out
        rc = logit_fold_scan(c, who, foldid_dev, n, nfolds, leave_out, irls_maxit, &D.n_eff, &D.kept_row);
        if (rc) return rc;
        if (leave_out > 0) { D.foldid = foldid_dev; D.leave_out = leave_out; }
    }
    if ((int64_t)D.q >= D.n_eff) {
        set_error("%s: p + intercept >= the %lld rows outside fold %d is not supported (the reference's XWXt branch never forms grad or XY, "
                  "ref src/oem_logistic_sparse.h:497-502, :978)", who, (long long)D.n_eff, (int)leave_out);
        return OEMGPU_ERR_UNSUPPORTED;
    }
    D.P = lsp_plan(n, p, x->nnz, intercept, c->num_cu, true);          // the plan, the route and the chunking see n
    rc = logistic_irls(c, D, D.n_eff, p, intercept, irls_maxit, irls_tol, o, beta, lambda_out, niter, loss, d);
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

// out[0] route (1 csc, 0 row tiles), [1] inner solve (1 one workgroup, 0 launch form), [2] workspace bytes of the fit's own pieces,
// [3] the bound they stay within, [4] rows per tile (0 on the csc route), [5] row-pass workgroups, [6] rows per row-pass workgroup,
// [7] chunks of the compressed-column kernels
static int lsp_plan_out(const char *who, int64_t n, int32_t p, int64_t nnz, int32_t intercept, int32_t num_cu, bool resident, int64_t *out)
{
    if (n < 1 || p < 1 || nnz < 0 || num_cu < 1 || !out) { set_error("%s: bad argument", who); return OEMGPU_ERR_ARG; }
    const LspPlan P = lsp_plan(n, p, nnz, intercept, num_cu, resident);
    out[0] = P.csc; out[1] = P.inner_wg; out[2] = (int64_t)P.ws_bytes; out[3] = (int64_t)P.bound; out[4] = P.rcrows; out[5] = P.nchunk;
    out[6] = P.ch; out[7] = csc_chunks(n);
    return 0;
}

int oemgpu_selftest_logistic_sparse_plan(int64_t n, int32_t p, int64_t nnz, int32_t intercept, int32_t num_cu, int64_t *out)
{
    return lsp_plan_out("selftest_logistic_sparse_plan", n, p, nnz, intercept, num_cu, false, out);
}

// the same for a fit on a resident x (oemgpu_fit_logistic_sparse_fold_res): out[2] without the pieces the handle and the caller hold
int oemgpu_selftest_logistic_sparse_res_plan(int64_t n, int32_t p, int64_t nnz, int32_t intercept, int32_t num_cu, int64_t *out)
{
    return lsp_plan_out("selftest_logistic_sparse_res_plan", n, p, nnz, intercept, num_cu, true, out);
}

#pragma GCC visibility pop
}
