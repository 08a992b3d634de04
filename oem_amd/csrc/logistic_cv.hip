// logistic_cv.hip -- the scoring pass of cv.oem for binomial fits: what cv.oemfit_binomial (ref R/cv_oem.R:224-346) needs from the
// held-out rows, without X leaving the device.  Every row is scored with the coefficient columns of ITS OWN fold (the fit that left
// the row out, interpolated onto the full fit's lambdas by the caller):
//     prob = 1 / (1 + exp(-(beta_0 + x . beta))),  y2 = (y == y_hi)
//     deviance  -2 [y2 log pm + (1 - y2) log(1 - pm)], pm = prob clamped to [1e-5, 1 - 1e-5]        (R/cv_oem.R:320-327)
//     class     y2 ? prob <= 0.5 : prob > 0.5
//     mse       2 (y2 - prob)^2          (both columns of the reference's indicator matrix)
//     mae       2 |y2 - prob|
// and per (fold, column) the sum of each term and of its square come back, with the fold sizes; cvcompute's fold means, the row form
// of grouped = FALSE and both standard errors follow from those on the host.  predmat (n x ncol) is written when asked for (keep, auc).
//
// One launch per fold.  Workgroup c owns rows [c CH, (c + 1) CH) and walks them in tiles of 64 (lane = row); a tile without a row of
// the fold is skipped before X is touched, so a fold's launch reads the fold's rows of X once (the four waves of a workgroup share a
// tile through the cache).  Wave w owns the columns 32 t + 8 w .. + 8: eight linear predictors at a time in registers, the fold's
// coefficient table in LDS when it fits (read through the cache otherwise).  Sums: a fixed butterfly over the 64 lanes, tiles added in
// row order into the workgroup's LDS accumulators, workgroup partials added in chunk order -- no floating-point atomics, two calls give
// the same bits.  Scoring is a small share of a cross-validation, so the kernel is kept plain.
//
// The rows come through a reader (the kernel's ROWS parameter).  CvDenseRows: the column-major x, an entry per column.  CvCsrRows
// (oemgpu_logistic_cv_score_sparse_res): the compressed-row copy of a resident sparse x -- lane = row as before, every lane walks its own
// row's stored entries in column order, one fma each.  The dense reader adds fma(0, beta, eta) = eta for an absent entry, so on
// finite tables the sparse entry returns the bits of the dense entry on the same matrix written out; plan, tiles, tile skip,
// butterfly and sum order are shared.
// CvRmRows<T> (oemgpu_logistic_cv_score_rm_dev): a row-major x of float64 / float32 elements read where it lies -- lane = row, every lane
// walks its own row's consecutive elements with the dense reader's fma in the dense reader's order: the bits of the dense entry on the
// column-major float64 copy.
#include "logistic.hpp"

#include <algorithm>
#include <vector>

namespace oemgpu {

static const size_t CV_LDS_BYTES = (size_t)160 << 10;   // LDS of a gfx950 CU
static const int CV_COL_BATCH = 2048;                   // columns per launch when the table is not in LDS (their accumulators are)

struct CvScorePlan {
    int64_t ch;        // rows per workgroup (a multiple of 64)
    int64_t nchunk;    // workgroups of a launch: workgroup c = rows [c ch, min(n, (c + 1) ch))
    bool tlds;         // a fold's coefficient table sits in LDS beside the accumulators
    int cb;            // columns per launch
    int nlaunch;       // launches per fold
    size_t lds;        // dynamic LDS bytes of the largest launch
};

static CvScorePlan cv_score_plan(int64_t n, int p, int ncol, int num_cu)
{
    CvScorePlan P;
    int64_t ch = (n + 4 * (int64_t)num_cu - 1) / (4 * (int64_t)num_cu);
    P.ch = std::max<int64_t>(64, (ch + 63) / 64 * 64);
    P.nchunk = (n + P.ch - 1) / P.ch;
    P.tlds = 8 * ((size_t)ncol * (p + 1) + 8 * (size_t)ncol + 1) <= CV_LDS_BYTES;
    P.cb = P.tlds ? ncol : std::min<int>(ncol, CV_COL_BATCH);
    P.nlaunch = (ncol + P.cb - 1) / P.cb;
    P.lds = 8 * (8 * (size_t)P.cb + 1 + (P.tlds ? (size_t)P.cb * (p + 1) : 0));
    return P;
}

namespace {

__device__ __forceinline__ double wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

struct CvDenseRows {                 // x column-major, leading dimension ld
    static constexpr bool sparse = false;
    static constexpr bool rowmajor = false;
    const double *x;
    int64_t ld;
};
template <typename T>
struct CvRmRows {                    // x row-major, row stride ldr, float64 / float32 elements widened in the register
    static constexpr bool sparse = false;
    static constexpr bool rowmajor = true;
    const T *x;
    int64_t ldr;
};
struct CvCsrRows {                   // row r: entries rowptr[r] .. rowptr[r + 1] of (ccol, cval), in column order
    static constexpr bool sparse = true;
    const int64_t *rowptr;
    const int32_t *ccol;
    const double *cval;
};

// tab: the fold's table, column c at tab[c (p + 1)]: [beta_0, beta (p)]; part: nchunk x (8 ncol + 1), the last entry the fold's rows
template <bool TLDS, class ROWS>
__global__ __launch_bounds__(256) void logit_cv_score_kernel(const ROWS X, int64_t n, int p, const double *__restrict__ y,
                                                             double y_hi, const int32_t *__restrict__ foldid, int32_t fold,
                                                             const double *__restrict__ tab, int ncol, int64_t ch, double *__restrict__ part,
                                                             double *__restrict__ pred)
{
    extern __shared__ double lsh[];
    double *acc = lsh;                               // 8 ncol + 1
    double *T = lsh + 8 * (size_t)ncol + 1;          // TLDS: ncol (p + 1)
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int nacc = 8 * ncol + 1, q = p + 1;
    for (int k = tid; k < nacc; k += 256) acc[k] = 0.0;
    if (TLDS) for (int k = tid; k < ncol * q; k += 256) T[k] = tab[k];
    __syncthreads();
    const double *tb = TLDS ? T : tab;
    const int64_t r_lo = (int64_t)blockIdx.x * ch, r_hi = (r_lo + ch < n) ? r_lo + ch : n;
    for (int64_t r0 = r_lo; r0 < r_hi; r0 += 64) {
        const int64_t row = r0 + lane;
        const bool in = row < r_hi && foldid[row] == fold;
        const unsigned long long m = __ballot(in);
        if (m == 0ull) continue;                     // (the same for the four waves: no barrier below)
        if (tid == 0) acc[nacc - 1] += (double)__popcll(m);
        const double y2 = (in && y[row] == y_hi) ? 1.0 : 0.0;
        for (int c0 = 8 * w; c0 < ncol; c0 += 32) {  // columns owned by this wave alone
            const double *tc[8];
            double eta[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                tc[k] = tb + (size_t)(c0 + k < ncol ? c0 + k : ncol - 1) * q;
                eta[k] = tc[k][0];
            }
            if constexpr (ROWS::sparse) {
                const int64_t k0 = in ? X.rowptr[row] : 0, k1 = in ? X.rowptr[row + 1] : 0;
                for (int64_t e = k0; e < k1; ++e) {
                    const double v = X.cval[e];
                    const int j = X.ccol[e];
#pragma unroll
                    for (int k = 0; k < 8; ++k) eta[k] = fma(v, tc[k][1 + j], eta[k]);
                }
            } else if constexpr (ROWS::rowmajor) {
                // lane = row as before: every lane walks its own row's consecutive elements (a cache line serves the next 8 or 16
                // columns of the lane); a row outside the fold is not loaded.  The same fma in the same order as the dense reader
                const auto *__restrict__ xr = X.x + (size_t)(in ? row : 0) * X.ldr;
                for (int j = 0; j < p; ++j) {
                    const double v = in ? (double)xr[j] : 0.0;
#pragma unroll
                    for (int k = 0; k < 8; ++k) eta[k] = fma(v, tc[k][1 + j], eta[k]);
                }
            } else {
                const double *__restrict__ x = X.x;
                const int64_t ld = X.ld;
                for (int j = 0; j < p; ++j) {
                    const double v = in ? x[(size_t)j * ld + row] : 0.0;
#pragma unroll
                    for (int k = 0; k < 8; ++k) eta[k] = fma(v, tc[k][1 + j], eta[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (c0 + k >= ncol) break;
                const double prob = 1.0 / (1.0 + exp(-eta[k]));
                double t[4] = {0.0, 0.0, 0.0, 0.0};
                if (in) {
                    const double pm = fmin(fmax(prob, 1e-5), 1.0 - 1e-5);
                    t[0] = -2.0 * log(y2 != 0.0 ? pm : 1.0 - pm);
                    t[1] = (y2 != 0.0 ? prob <= 0.5 : prob > 0.5) ? 1.0 : 0.0;
                    const double e = y2 - prob;
                    t[2] = 2.0 * (e * e);
                    t[3] = 2.0 * fabs(e);
                    if (pred) pred[(size_t)(c0 + k) * n + row] = prob;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double s1 = wave_sum(t[i]), s2 = wave_sum(t[i] * t[i]);
                    if (lane == 0) { acc[(c0 + k) * 8 + 2 * i] += s1; acc[(c0 + k) * 8 + 2 * i + 1] += s2; }
                }
            }
        }
    }
    __syncthreads();
    double *pc = part + (size_t)blockIdx.x * nacc;
    for (int k = tid; k < nacc; k += 256) pc[k] = acc[k];
}

// out[k] = ((part[0][k] + part[1][k]) + ...): chunk order; the last entry of a partial (the fold's rows) goes to *cnt
__global__ __launch_bounds__(256) void logit_cv_sum_kernel(const double *__restrict__ part, int64_t nchunk, int len, double *__restrict__ out,
                                                           double *__restrict__ cnt)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= len) return;
    double a = 0.0;
    for (int64_t c = 0; c < nchunk; ++c) a += part[(size_t)c * len + k];
    if (k == len - 1) *cnt = a;
    else out[k] = a;
}

}  // namespace

template <class ROWS>
static int cv_score_run(oemgpu_ctx *c, const ROWS X, int64_t n, int32_t p, const double *y, double y_hi, const int32_t *foldid,
                        int32_t nfolds, const double *coef, int32_t ncol, double *sums, int64_t *counts, double *pred)
{
    hipStream_t s = c->stream;
    const int q = p + 1;
    const CvScorePlan P = cv_score_plan(n, p, ncol, c->num_cu);
    const int64_t ch = P.ch, nchunk = P.nchunk;
    const size_t tab_f = (size_t)ncol * q;                                               // doubles of a fold's table
    const bool tlds = P.tlds;
    const int cb = P.cb;                                                                 // columns per launch
    const size_t out_f = 8 * (size_t)ncol + 1;
    Bump B;
    const size_t a_tab = B.take(8 * tab_f * nfolds), a_part = B.take(8 * (size_t)nchunk * (8 * (size_t)cb + 1)), a_out = B.take(8 * out_f * nfolds);
    ctx_void_cv(c);
    if (ctx_grow(c, &c->aux, &c->aux_bytes, B.off)) return OEMGPU_ERR_HIP;
    double *tab = (double *)(c->aux + a_tab), *part = (double *)(c->aux + a_part), *out = (double *)(c->aux + a_out);
    OEM_HIP(hipMemcpyAsync(tab, coef, 8 * tab_f * nfolds, hipMemcpyHostToDevice, s));
    for (int f = 0; f < nfolds; ++f) {
        for (int c0 = 0; c0 < ncol; c0 += cb) {
            const int nc = std::min(cb, ncol - c0), nacc = 8 * nc + 1;
            const double *tf = tab + (size_t)f * tab_f + (size_t)c0 * q;
            double *pf = pred ? pred + (size_t)c0 * n : nullptr;
            const size_t lds = 8 * ((size_t)nacc + (tlds ? (size_t)nc * q : 0));
            if (tlds) {
                if (lds_limit_once(reinterpret_cast<const void *>(&logit_cv_score_kernel<true, ROWS>), lds)) return OEMGPU_ERR_HIP;
                hipLaunchKernelGGL((logit_cv_score_kernel<true, ROWS>), dim3((unsigned)nchunk), dim3(256), lds, s, X, n, p, y, y_hi, foldid, f + 1, tf, nc, ch,
                                   part, pf);
            } else {
                if (lds_limit_once(reinterpret_cast<const void *>(&logit_cv_score_kernel<false, ROWS>), lds)) return OEMGPU_ERR_HIP;
                hipLaunchKernelGGL((logit_cv_score_kernel<false, ROWS>), dim3((unsigned)nchunk), dim3(256), lds, s, X, n, p, y, y_hi, foldid, f + 1, tf, nc, ch,
                                   part, pf);
            }
            hipLaunchKernelGGL(logit_cv_sum_kernel, dim3((nacc + 255) / 256), dim3(256), 0, s, part, nchunk, nacc, out + (size_t)f * out_f + 8 * (size_t)c0,
                               out + (size_t)f * out_f + out_f - 1);
            OEM_HIP(hipGetLastError());
        }
    }
    std::vector<double> h(out_f * nfolds);
    OEM_HIP(hipMemcpyAsync(h.data(), out, 8 * h.size(), hipMemcpyDeviceToHost, s));
    OEM_HIP(hipStreamSynchronize(s));
    for (int f = 0; f < nfolds; ++f) {
        std::copy(h.begin() + (size_t)f * out_f, h.begin() + (size_t)f * out_f + out_f - 1, sums + (size_t)f * 8 * ncol);
        counts[f] = (int64_t)h[(size_t)f * out_f + out_f - 1];
    }
    return 0;
}

// the scoring pass with the reader of where the rows lie: the compressed-row copy of sx, or the dense source X; one of the two is null
static int cv_score_rows(oemgpu_ctx *c, const oemgpu_sparse_x *sx, const DenseSrc *X, int64_t n, int32_t p, const double *y, double y_hi,
                         const int32_t *foldid, int32_t nfolds, const double *coef, int32_t ncol, double *sums, int64_t *counts, double *pred)
{
    if (sx) return cv_score_run(c, CvCsrRows{sx->rowptr, sx->ccol, sx->cval}, n, p, y, y_hi, foldid, nfolds, coef, ncol, sums, counts, pred);
    if (X->colmajor()) return cv_score_run(c, CvDenseRows{X->cm(), X->ld}, n, p, y, y_hi, foldid, nfolds, coef, ncol, sums, counts, pred);
    if (X->dtype == OEMGPU_F32) return cv_score_run(c, CvRmRows<float>{(const float *)X->x, X->ld}, n, p, y, y_hi, foldid, nfolds, coef, ncol, sums, counts, pred);
    return cv_score_run(c, CvRmRows<double>{(const double *)X->x, X->ld}, n, p, y, y_hi, foldid, nfolds, coef, ncol, sums, counts, pred);
}

// the checks of the two dense entries, then the scoring pass
static int cv_score_src(const char *who, oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const double *y_dev, double y_hi,
                        const int32_t *foldid_dev, int32_t nfolds, const double *coef, int32_t ncol, double *sums, int64_t *counts, double *pred)
{
    if (!c || !X.x || !y_dev || !foldid_dev || !coef || !sums || !counts) { set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG; }
    if (int rc = dense_src_check(who, X, n, p)) return rc;
    if (n < 1 || p < 1 || ncol < 1) { set_error("%s: bad n, p or ncol", who); return OEMGPU_ERR_ARG; }
    if (nfolds < 3) { set_error("nfolds must be bigger than 3; nfolds=10 recommended"); return OEMGPU_ERR_ARG; }
    if (p > LOGIT_P_LIMIT) { set_error("%s: p > %d is not supported", who, LOGIT_P_LIMIT); return OEMGPU_ERR_UNSUPPORTED; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    return cv_score_rows(c, nullptr, &X, n, p, y_dev, y_hi, foldid_dev, nfolds, coef, ncol, sums, counts, pred);
}

}  // namespace oemgpu

using namespace oemgpu;

extern "C" {
#pragma GCC visibility push(default)

int oemgpu_logistic_cv_score_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev, double y_hi,
                                 const int32_t *foldid_dev, int32_t nfolds, const double *coef, int32_t ncol, double *sums, int64_t *counts,
                                 double *predmat_dev)
{
    return cv_score_src("logistic_cv_score", c, dense_src_cm(x_dev, ld), n, p, y_dev, y_hi, foldid_dev, nfolds, coef, ncol, sums, counts, predmat_dev);
}

int oemgpu_logistic_cv_score_rm_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                                    double y_hi, const int32_t *foldid_dev, int32_t nfolds, const double *coef, int32_t ncol, double *sums,
                                    int64_t *counts, double *predmat_dev)
{
    return cv_score_src("logistic_cv_score_rm", c, dense_src_rm(x_dev, dtype, ldr), n, p, y_dev, y_hi, foldid_dev, nfolds, coef, ncol, sums, counts,
                        predmat_dev);
}

int oemgpu_logistic_cv_score_sparse_res(oemgpu_ctx *c, const oemgpu_sparse_x *x, const double *y_dev, double y_hi, const int32_t *foldid_dev,
                                        int32_t nfolds, const double *coef, int32_t ncol, double *sums, int64_t *counts, double *predmat_dev)
{
    if (!c || !x || !y_dev || !foldid_dev || !coef || !sums || !counts) { set_error("logistic_cv_score_sparse: NULL argument"); return OEMGPU_ERR_ARG; }
    if (ncol < 1) { set_error("logistic_cv_score_sparse: bad ncol"); return OEMGPU_ERR_ARG; }
    if (nfolds < 3) { set_error("nfolds must be bigger than 3; nfolds=10 recommended"); return OEMGPU_ERR_ARG; }
    if (x->p > LOGIT_P_LIMIT) { set_error("logistic_cv_score_sparse: p > %d is not supported", LOGIT_P_LIMIT); return OEMGPU_ERR_UNSUPPORTED; }
    if (c->device != x->device) { set_error("logistic_cv_score_sparse: the context and the sparse x are on different devices"); return OEMGPU_ERR_ARG; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    return cv_score_rows(c, x, nullptr, x->n, x->p, y_dev, y_hi, foldid_dev, nfolds, coef, ncol, sums, counts, predmat_dev);
}

int oemgpu_selftest_cv_score_plan(int64_t n, int32_t p, int32_t ncol, int32_t num_cu, int64_t *out)
{
    if (n < 1 || p < 1 || p > LOGIT_P_LIMIT || ncol < 1 || num_cu < 1 || !out) { set_error("selftest_cv_score_plan: bad argument"); return OEMGPU_ERR_ARG; }
    const CvScorePlan P = cv_score_plan(n, p, ncol, num_cu);
    out[0] = P.ch; out[1] = P.nchunk; out[2] = P.tlds ? 1 : 0; out[3] = P.cb; out[4] = P.nlaunch; out[5] = (int64_t)P.lds;
    return 0;
}

#pragma GCC visibility pop
}
