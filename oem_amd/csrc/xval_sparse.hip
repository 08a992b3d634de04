// xval_sparse.hip -- xval.oem on a compressed-sparse-column x WITHOUT densifying it (the call R's front end names and the reference
// never shipped: ref R/oem_xval.R:196-201 stops, :500 .Call("oem_xval_sparse")).  The semantics are oemXvalDense's
// (ref src/oem_xval_dense.{h,cpp}); only the way the K fold moment buffers and the per-row errors are produced differs from xval.hip:
//   * fold order: the rows get the positions of launch_fold_layout with every fold segment starting on a multiple of CSC_CHUNK rows, so
//     a fold is a run of whole chunks of csc_gram_kernel (padding rows cost a sparse matrix nothing).  csc_fold_permute_kernel rewrites
//     every column in that row order: one workgroup per column, the entries counted per fold (integer LDS counters), an exclusive scan
//     over the folds, then a stable placement 256 entries at a time -- pos is increasing inside a fold, so a stable partition by fold
//     IS the column sorted by new row index, and the result is the same arrays whatever the schedule;
//   * fold moments: csc_gram_kernel<false> (sparse.hip) over chunk ranges the host cuts at fold boundaries (xval_sparse_ranges),
//     csc_fold_finish_kernel adds a fold's range sums in range order, csc_fold_stats_kernel takes sum x_j, sum x_j y, sum y, sum y^2
//     from the fold's contiguous piece of every column.  p nnz / 2 LDS gathers in all, whatever K;
//   * CV error: csr_cv_error_kernel -- a wave per row of the fold-ordered compressed rows, lanes over the lambdas, the fold's
//     coefficients transposed to [p + 1][nl16] so that the lambdas of one column are one 512-byte read; per-wave partials in the layout
//     cv_finish_kernel reads.
// cv.oem(family = "gaussian") on a resident sparse x (api.hip: oemgpu_cv_sparse_*) runs the same fold phases on an oemgpu_sparse_x and scores
// with csr_cv_fold_score_kernel: the same walk over the compressed rows, flushed per fold into the layout cv_fold_finish_kernel merges.
#include "ctx.hpp"

namespace oemgpu {

namespace {

constexpr int SRC = CSC_CHUNK;
constexpr int PT = 256;                  // threads (and entries per round) of csc_fold_permute_kernel
constexpr int NYF = 16;                  // slices of a fold's y in csc_fold_stats_kernel

// ---------------------------------------------------------------------------------------- fold-ordered compressed columns
__global__ __launch_bounds__(PT) void csc_fold_permute_kernel(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rowidx,
                                                              const double *__restrict__ val, const int32_t *__restrict__ foldid,
                                                              const int *__restrict__ pos, int K, int32_t *__restrict__ cfo /* [p][K + 1] */,
                                                              int32_t *__restrict__ prow, double *__restrict__ pval)
{
    extern __shared__ int sh[];
    int *cnt = sh, *off = sh + K, *fid = off + K + 1;             // [K], [K + 1], [PT]
    const int j = blockIdx.x, tid = threadIdx.x;
    const int64_t k0 = colptr[j], k1 = colptr[j + 1];
    for (int k = tid; k < K; k += PT) cnt[k] = 0;
    __syncthreads();
    for (int64_t e = k0 + tid; e < k1; e += PT) atomicAdd(&cnt[foldid[rowidx[e]] - 1], 1);      // integer: the order does not matter
    __syncthreads();
    if (tid < 64) {                                               // exclusive scan over the folds, 64 at a step
        int run = 0;
        for (int b0 = 0; b0 < K; b0 += 64) {
            const int k = b0 + tid;
            const int c = k < K ? cnt[k] : 0;
            int incl = c;
            for (int s = 1; s < 64; s <<= 1) { const int t = __shfl_up(incl, s, 64); if (tid >= s) incl += t; }
            if (k < K) off[k] = run + incl - c;
            run += __shfl(incl, 63, 64);
        }
        if (tid == 0) off[K] = run;
    }
    __syncthreads();
    for (int k = tid; k <= K; k += PT) cfo[(size_t)j * (K + 1) + k] = off[k];
    for (int k = tid; k < K; k += PT) cnt[k] = 0;                 // from here: entries of the fold placed so far
    __syncthreads();
    for (int64_t base = k0; base < k1; base += PT) {
        const int64_t e = base + tid;
        int f = -1, r = 0;
        if (e < k1) { r = rowidx[e]; f = foldid[r] - 1; }
        fid[tid] = f;
        __syncthreads();
        if (f >= 0) {
            int rank = 0;                                         // entries of the same fold in front of this one in the round
            for (int u = 0; u < tid; ++u) rank += fid[u] == f ? 1 : 0;
            const int64_t dst = k0 + off[f] + cnt[f] + rank;
            prow[dst] = pos[r];
            pval[dst] = val[e];
        }
        __syncthreads();                                          // every thread has read cnt
        if (f >= 0) atomicAdd(&cnt[f], 1);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void y_fold_order_kernel(const double *__restrict__ y, const int *__restrict__ pos, int64_t n, double *__restrict__ yp)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) yp[pos[i]] = y[i];
}

// ---------------------------------------------------------------------------------------- per-fold moments (csc route)
// workgroup (j, k): column j < p over its entries of fold k (contiguous after the permutation); j >= p: a slice of the fold's y
__global__ __launch_bounds__(256) void csc_fold_stats_kernel(const int64_t *__restrict__ colptr, const int32_t *__restrict__ prow,
                                                             const double *__restrict__ pval, const double *__restrict__ yp,
                                                             const int32_t *__restrict__ cfo, const int64_t *__restrict__ fold_start,
                                                             const int64_t *__restrict__ fold_n, int p, int K, double *__restrict__ mfold,
                                                             double *__restrict__ ypart /* [K][NYF][2] */)
{
    __shared__ double sh[2][256];
    const int j = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, q = p + 2;
    double *M = mfold + (size_t)k * q * q;
    double s0 = 0.0, s1 = 0.0;
    if (j < p) {
        const int64_t e0 = colptr[j] + cfo[(size_t)j * (K + 1) + k], e1 = colptr[j] + cfo[(size_t)j * (K + 1) + k + 1];
        for (int64_t e = e0 + tid; e < e1; e += 256) { const double v = pval[e]; s0 += v; s1 = fma(v, yp[prow[e]], s1); }
    } else {
        const int64_t st = fold_start[k], nk = fold_n[k];
        const int64_t per = (nk + NYF - 1) / NYF, r0 = (int64_t)(j - p) * per, r1 = r0 + per < nk ? r0 + per : nk;
        for (int64_t r = r0 + tid; r < r1; r += 256) { const double v = yp[st + r]; s0 += v; s1 = fma(v, v, s1); }
    }
    sh[0][tid] = s0; sh[1][tid] = s1;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) { if (tid < h) { sh[0][tid] += sh[0][tid + h]; sh[1][tid] += sh[1][tid + h]; } __syncthreads(); }
    if (tid == 0) {
        if (j < p) {
            M[(size_t)j * q + (p + 1)] = sh[0][0]; M[(size_t)(p + 1) * q + j] = sh[0][0];      // sum x_j
            M[(size_t)j * q + p] = sh[1][0];       M[(size_t)p * q + j] = sh[1][0];            // sum x_j y
        } else { ypart[((size_t)k * NYF + (j - p)) * 2] = sh[0][0]; ypart[((size_t)k * NYF + (j - p)) * 2 + 1] = sh[1][0]; }
    }
}

// fold k: its range sums in range order -> M_k (both triangles); the y slices in slice order -> M_k's y entries
__global__ __launch_bounds__(256) void csc_fold_finish_kernel(const double *__restrict__ part, const int32_t *__restrict__ frange,
                                                              const double *__restrict__ ypart, const int64_t *__restrict__ fold_n, int p,
                                                              double *__restrict__ mfold)
{
    const int q = p + 2, k = blockIdx.y;
    double *M = mfold + (size_t)k * q * q;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < (size_t)p * p) {
        const int a = (int)(t / p), b = (int)(t % p);
        if (b >= a) {
            double g = 0.0;
            for (int r = frange[k]; r < frange[k + 1]; ++r) g += part[(size_t)r * p * p + t];
            M[(size_t)a * q + b] = g;
            M[(size_t)b * q + a] = g;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double s0 = 0.0, s1 = 0.0;
        for (int i = 0; i < NYF; ++i) { s0 += ypart[((size_t)k * NYF + i) * 2]; s1 += ypart[((size_t)k * NYF + i) * 2 + 1]; }
        M[(size_t)p * q + (p + 1)] = s0; M[(size_t)(p + 1) * q + p] = s0;      // sum y
        M[(size_t)p * q + p] = s1;                                             // sum y^2
        M[(size_t)(p + 1) * q + (p + 1)] = (double)fold_n[k];
    }
}

// ---------------------------------------------------------------------------------------- compressed rows
// Workgroup c owns the rows of chunk c.  Compressed rows keep all entries of earlier rows in front, so the chunk's first entry is the
// sum over the columns of where they enter the chunk (cptr); inside the chunk: entries per row (integer LDS counters) and a block scan.
__global__ __launch_bounds__(1024) void csr_rowptr_kernel(const int64_t *__restrict__ colptr, const int32_t *__restrict__ prow,
                                                          const int32_t *__restrict__ cptr, int p, int nchunk, int64_t *__restrict__ rowptr)
{
    __shared__ int cntr[SRC];
    __shared__ int wsum[16];
    __shared__ unsigned long long base_s;
    const int c = blockIdx.x, tid = threadIdx.x, grp = tid >> 4, l16 = tid & 15, w = tid >> 6, lane = tid & 63;
    for (int k = tid; k < SRC; k += 1024) cntr[k] = 0;
    if (tid == 0) base_s = 0ull;
    __syncthreads();
    unsigned long long b = 0ull;
    for (int j = tid; j < p; j += 1024) b += (unsigned long long)cptr[(size_t)c * p + j];
    if (b) atomicAdd(&base_s, b);
    const int rbase = c * SRC;
    for (int j = grp; j < p; j += 64) {
        const int ka = cptr[(size_t)c * p + j], kb = cptr[(size_t)(c + 1) * p + j];
        const int64_t cj = colptr[j];
        for (int k = ka + l16; k < kb; k += 16) atomicAdd(&cntr[prow[cj + k] - rbase], 1);
    }
    __syncthreads();
    int v[8], s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[i] = s; s += cntr[8 * tid + i]; }              // v: exclusive inside the thread's eight rows
    int incl = s;
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int woff = 0;
    for (int ww = 0; ww < w; ++ww) woff += wsum[ww];
    const int64_t base = (int64_t)base_s + woff + incl - s;
#pragma unroll
    for (int i = 0; i < 8; ++i) rowptr[(size_t)rbase + 8 * tid + i] = base + v[i];
    if (c == nchunk - 1 && tid == 1023) rowptr[(size_t)nchunk * SRC] = base + s;
}

// ---------------------------------------------------------------------------------------- CV error over the compressed rows
__global__ __launch_bounds__(256) void coef_transpose_kernel(const double *__restrict__ B, int Kd, int nl, int nl16, size_t total, double *__restrict__ bt)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int lam = (int)(t % nl16);
    const size_t cm = t / nl16, m = cm / Kd;                       // m: (fold, penalty)
    const int c = (int)(cm % Kd);
    bt[t] = lam < nl ? B[(m * nl + lam) * Kd + c] : 0.0;
}

// grid (workgroups, npen, blocks of 64 lambdas), XVS_CVW waves each.  The n rows in fold order are numbered 0 .. n - 1 (padding rows
// have no number: they are never read); wave g of W takes the rows g, g + W, ...  A lane keeps (rows, centre, sum (v - c), sum (v - c)^2)
// of its lambda over its wave's rows in row order -- no cross-lane sum -- and every wave leaves one partial [npen][nl16][4].
__global__ __launch_bounds__(64 * XVS_CVW) void csr_cv_error_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ ccol,
                                                                    const double *__restrict__ cval, const double *__restrict__ yp,
                                                                    const int64_t *__restrict__ fold_start, const int64_t *__restrict__ fold_n,
                                                                    int K, int p, const double *__restrict__ bt, int nl, int mae,
                                                                    double *__restrict__ part)
{
    const int npen = gridDim.y, pen = blockIdx.y, lane = threadIdx.x & 63;
    const int64_t W = (int64_t)gridDim.x * XVS_CVW;
    const int64_t gw = (int64_t)blockIdx.x * XVS_CVW + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nl16 = (nl + 15) & ~15, lam = blockIdx.z * 64 + lane, Kd = p + 1;
    const bool active = lam < nl;
    double cnt = 0.0, cen = 0.0, s1 = 0.0, s2 = 0.0;
    int64_t prefix = 0;
    for (int k = 0; k < K; ++k) {
        const int64_t nk = fold_n[k], st = fold_start[k];
        const double *Bk = bt + ((size_t)k * npen + pen) * Kd * nl16 + (active ? lam : 0);
        const double b0 = Bk[0];
        int64_t r = (gw - prefix % W + W) % W;                     // the first row of fold k whose number is g modulo W
        for (; r < nk; r += W) {
            const int64_t row = st + r, e0 = rowptr[row], e1 = rowptr[row + 1];
            double eta = b0;
            for (int64_t e = e0; e < e1; ++e) eta = fma(cval[e], Bk[(size_t)(ccol[e] + 1) * nl16], eta);
            const double res = yp[row] - eta, v = mae ? fabs(res) : res * res;
            if (cnt == 0.0) cen = v;
            const double dv = v - cen;
            s1 += dv; s2 = fma(dv, dv, s2); cnt += 1.0;
        }
        prefix += nk;
    }
    if (lam < nl16) {
        double *q = part + (((size_t)gw * npen + pen) * nl16 + lam) * 4;
        q[0] = active ? cnt : 0.0; q[1] = active ? cen : 0.0; q[2] = active ? s1 : 0.0; q[3] = active ? s2 : 0.0;
    }
}

// cv.oem, family = "gaussian" (cvcompute's fold means, R/utils.R:128-144, and fit.preval): the kernel above keeps ONE running set per lane
// over all folds; this one FLUSHES the lane's set at every fold boundary -- part [K][waves][npen][nl16][4], zeros from a wave that saw no
// row of the fold: the layout cv_fold_finish_kernel merges with per_fold = waves -- and starts the next fold with an empty one.  The
// wave's fixed stride over the n rows as numbered in fold order stays: folds of very unequal size are balanced, which one grid slice
// per fold would not be.  Columns >= ncol[pen] cost no arithmetic.  PRED: eta goes to predmat[pen][lam][inv[row]] (the caller's row),
// NaN for lam in [ncol[pen], nl): one store instruction writes 64 words n * 8 bytes apart -- the scattered pattern of cv_error_kernel's
// PRED store, priced there and not tuned here; nothing of size n * nl exists without predmat.
// Bound: one read of the compressed rows (12 nnz + 16 n bytes) per (penalty, 64-lambda block); the coefficient rows bt[col][lam] are
// 512-byte reads that stay in L2 (K npen (p + 1) nl16 doubles).
template <bool PRED>
__global__ __launch_bounds__(64 * XVS_CVW) void csr_cv_fold_score_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ ccol,
                                                                         const double *__restrict__ cval, const double *__restrict__ yp,
                                                                         const int64_t *__restrict__ fold_start, const int64_t *__restrict__ fold_n,
                                                                         int K, int p, const double *__restrict__ bt, int nl, int mae,
                                                                         const int *__restrict__ ncol, double *__restrict__ part,
                                                                         double *__restrict__ pred, const int *__restrict__ inv, int64_t n)
{
    const int npen = gridDim.y, pen = blockIdx.y, lane = threadIdx.x & 63;
    const int64_t W = (int64_t)gridDim.x * XVS_CVW;
    const int64_t gw = (int64_t)blockIdx.x * XVS_CVW + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nl16 = (nl + 15) & ~15, lam = blockIdx.z * 64 + lane, Kd = p + 1;
    const int nc = ncol[pen];
    const bool active = lam < nc;                                  // a valid column of this penalty
    const bool any = blockIdx.z * 64 < nc;                         // wave-uniform: some lane of the block is
    int64_t prefix = 0;
    for (int k = 0; k < K; ++k) {
        const int64_t nk = fold_n[k], st = fold_start[k];
        const double *Bk = bt + ((size_t)k * npen + pen) * Kd * nl16 + (active ? lam : 0);
        const double b0 = Bk[0];
        double cnt = 0.0, cen = 0.0, s1 = 0.0, s2 = 0.0;
        int64_t r = (gw - prefix % W + W) % W;                     // the first row of fold k whose number is g modulo W
        for (; r < nk; r += W) {
            const int64_t row = st + r;
            double eta = b0;
            if (any) {
                const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
                for (int64_t e = e0; e < e1; ++e) eta = fma(cval[e], Bk[(size_t)(ccol[e] + 1) * nl16], eta);
                if (active) {
                    const double res = yp[row] - eta, v = mae ? fabs(res) : res * res;
                    if (cnt == 0.0) cen = v;
                    const double dv = v - cen;
                    s1 += dv; s2 = fma(dv, dv, s2); cnt += 1.0;
                }
            }
            if constexpr (PRED) {
                const int64_t orig = inv[row];
                if (lam < nl && orig >= 0 && orig < n) pred[((size_t)pen * nl + lam) * n + orig] = active ? eta : __builtin_nan("");
            }
        }
        if (lam < nl16) {                                          // the fold's flush; a wave without a row of it writes zeros
            double *q = part + ((((size_t)k * W + gw) * npen + pen) * nl16 + lam) * 4;
            q[0] = cnt; q[1] = cen; q[2] = s1; q[3] = s2;
        }
        prefix += nk;
    }
}

// cv.oem on a resident sparse x with n <= p (oemgpu_cv_sparse_wide_score_res; ref R/cv_oem.R:376-391): ONE fold's held-out rows against
// that fold's table, on the handle's compressed rows in the caller's order -- no fold-ordered layout.  The kernel above keeps all K
// tables on the device (K npen (p + 1) nl16 doubles: 1.8 GB at p = 200,000, K = 10, nl = 100); here bt [npen][p + 1][nl16] is one
// fold's, staged fold by fold.  grid (workgroups, npen, blocks of 64 lambdas), XVS_CVW waves each: wave g of W takes the rows
// list[g], list[g + W], .. of the fold's row list (ascending rows), its 64 lanes are 64 lambdas, the loop over the row's stored
// entries reads bt[ccol + 1][lam] (coalesced in lambda), a lane keeps (count, centre, sum (v - c), sum (v - c)^2) in row order and
// every wave leaves one partial [npen][nl16][4] (zeros from a wave without a row): cv_fold_finish_kernel's layout, per_fold = W.
// Bound: 12 bytes per held-out non-zero per (penalty, 64-lambda block), plus the table rows -- 512-byte reads that stay in L2 while
// npen (p + 1) nl16 doubles fit there and are HBM gathers beyond.
template <bool PRED>
__global__ __launch_bounds__(64 * XVS_CVW) void csr_cv_wide_score_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ ccol,
                                                                         const double *__restrict__ cval, const double *__restrict__ y,
                                                                         const int32_t *__restrict__ list, int nk, int p,
                                                                         const double *__restrict__ bt, int nl, int mae,
                                                                         const int *__restrict__ ncol, double *__restrict__ part,
                                                                         double *__restrict__ pred, int64_t n)
{
    const int npen = gridDim.y, pen = blockIdx.y, lane = threadIdx.x & 63;
    const int W = (int)gridDim.x * XVS_CVW;
    const int gw = (int)blockIdx.x * XVS_CVW + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nl16 = (nl + 15) & ~15, lam = blockIdx.z * 64 + lane, Kd = p + 1;
    const int nc = ncol[pen];
    const bool active = lam < nc;                                  // a valid column of this penalty
    const bool any = blockIdx.z * 64 < nc;                         // wave-uniform: some lane of the block is
    const double *Bk = bt + (size_t)pen * Kd * nl16 + (active ? lam : 0);
    const double b0 = Bk[0];
    double cnt = 0.0, cen = 0.0, s1 = 0.0, s2 = 0.0;
    for (int r = gw; r < nk; r += W) {
        const int64_t row = list[r];
        double eta = b0;
        if (any) {
            const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
            for (int64_t e = e0; e < e1; ++e) eta = fma(cval[e], Bk[(size_t)(ccol[e] + 1) * nl16], eta);
            if (active) {
                const double res = y[row] - eta, v = mae ? fabs(res) : res * res;
                if (cnt == 0.0) cen = v;
                const double dv = v - cen;
                s1 += dv; s2 = fma(dv, dv, s2); cnt += 1.0;
            }
        }
        if constexpr (PRED) {
            if (lam < nl) pred[((size_t)pen * nl + lam) * n + row] = active ? eta : __builtin_nan("");
        }
    }
    if (lam < nl16) {
        double *q = part + (((size_t)gw * npen + pen) * nl16 + lam) * 4;
        q[0] = cnt; q[1] = cen; q[2] = s1; q[3] = s2;
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------- the plan
CvWideScorePlan cv_wide_score_plan(int64_t n, int p, int K, int npen, int nl, int num_cu)
{
    CvWideScorePlan P;
    P.K = K; P.npen = npen; P.nl = nl; P.nl16 = (nl + 15) & ~15;
    P.lblk = (nl + 63) / 64;
    int64_t nwg = (int64_t)num_cu * 4 / ((int64_t)npen * P.lblk);
    const int64_t per_fold = (n + K - 1) / K, cap = (per_fold + XVS_CVW - 1) / XVS_CVW;     // a wave per held-out row of a fold of the usual size
    if (nwg > cap) nwg = cap;
    if (nwg > 1024) nwg = 1024;
    const size_t per_wave = (size_t)K * npen * P.nl16 * 4 * sizeof(double);
    const int64_t fit = (int64_t)(CVS_PART_MAX / per_wave) / XVS_CVW;
    if (nwg > fit) nwg = fit;
    P.nwg = nwg < 1 ? 1 : (int)nwg;
    P.waves = P.nwg * XVS_CVW;
    P.table_bytes = (size_t)(p + 1) * P.nl16 * sizeof(double);
    P.part_bytes = per_wave * P.waves;
    Bump B;
    P.a_list = B.take(sizeof(int32_t) * (size_t)n);
    P.a_raw = B.take(sizeof(double) * (size_t)npen * nl * (p + 1));
    P.a_bt = B.take(P.table_bytes * npen);
    P.a_part = B.take(P.part_bytes);
    P.a_tri = B.take(sizeof(double) * 3 * (size_t)K * npen * nl);
    P.a_ncol = B.take(sizeof(int) * (size_t)npen);
    P.bytes = B.off;
    return P;
}

CvSparseScorePlan cv_sparse_score_plan(int64_t n, int K, int npen, int nl, int num_cu)
{
    CvSparseScorePlan P;
    P.K = K; P.npen = npen; P.nl = nl; P.nl16 = (nl + 15) & ~15;
    P.lblk = (nl + 63) / 64;
    int64_t nwg = (int64_t)num_cu * 4 / ((int64_t)npen * P.lblk);
    const int64_t cap = (n + 16 * XVS_CVW - 1) / (16 * XVS_CVW);
    if (nwg > cap) nwg = cap;
    if (nwg > 1024) nwg = 1024;
    const size_t per_wave = (size_t)K * npen * P.nl16 * 4 * sizeof(double);
    const int64_t fit = (int64_t)(CVS_PART_MAX / per_wave) / XVS_CVW;       // workgroups whose waves' partials stay under the bound
    if (nwg > fit) nwg = fit;
    P.nwg = nwg < 1 ? 1 : (int)nwg;
    P.waves = P.nwg * XVS_CVW;
    P.part_bytes = per_wave * P.waves;
    return P;
}

XvalSparsePlan xval_sparse_plan(int64_t n, int p, int64_t nnz, int K, int npen, int nl, int num_cu, bool resident)
{
    XvalSparsePlan P;
    P.n = n; P.nnz = nnz; P.p = p; P.K = K; P.npen = npen; P.nl = nl; P.nl16 = (nl + 15) & ~15;
    P.R = sparse_route(n, p, nnz);
    P.nchunk_max = (int)(n / SRC) + K;                           // sum of ceil(n_k / SRC) over K folds of n rows in all
    P.npad_max = (int64_t)P.nchunk_max * SRC;
    // ranges: about 1024 workgroups over the chunks that hold rows, their sums under 256 MB where K allows (every fold that has rows
    // costs one range at least)
    int budget = csc_range_budget(n, p);
    while (budget > 1 && ((double)budget + K) * p * p * 8.0 > 256e6) --budget;
    const int nchunk = csc_chunks(n);
    P.per = (nchunk + budget - 1) / budget;
    P.rpf_max = (nchunk + P.per - 1) / P.per;
    P.nrange_max = P.nchunk_max / P.per + K;
    if (P.nrange_max > P.nchunk_max) P.nrange_max = P.nchunk_max;
    // CV error: about four workgroups per CU over (penalty, lambda block), a wave no fewer than 16 rows, at most 4096 partials
    P.cv_lblk = (nl + 63) / 64;
    int64_t nwg = (int64_t)num_cu * 4 / ((int64_t)npen * P.cv_lblk);
    const int64_t cap = (n + 16 * XVS_CVW - 1) / (16 * XVS_CVW);
    if (nwg > cap) nwg = cap;
    if (nwg > 1024) nwg = 1024;
    P.cv_nwg = nwg < 1 ? 1 : (int)nwg;
    P.cv_waves = P.cv_nwg * XVS_CVW;
    P.plmax = GramPlan{};
    if (!P.R.csc) P.plmax = gram_plan_bound(P.R.rows, p, num_cu);
    Bump A;
    const size_t ne = (size_t)nnz + 1;
    P.a_col = A.take(resident ? 0 : sizeof(int64_t) * ((size_t)p + 1)); P.a_row = A.take(resident ? 0 : sizeof(int32_t) * ne);
    P.a_val = A.take(resident ? 0 : sizeof(double) * ne);
    P.a_y = A.take(resident ? 0 : sizeof(double) * (size_t)n); P.a_fid = A.take(resident ? 0 : sizeof(int32_t) * (size_t)n);
    P.a_prow = A.take(sizeof(int32_t) * ne); P.a_pval = A.take(sizeof(double) * ne);
    P.a_cfo = A.take(sizeof(int32_t) * (size_t)p * (K + 1));
    P.a_cptr = A.take(sizeof(int32_t) * ((size_t)P.nchunk_max + 1) * p);
    P.a_rowptr = A.take(sizeof(int64_t) * ((size_t)P.npad_max + 1));
    P.a_ccol = A.take(sizeof(int32_t) * ne); P.a_cval = A.take(sizeof(double) * ne);
    P.a_gpart = A.take(P.R.csc ? sizeof(double) * (size_t)P.nrange_max * p * p : 0);
    P.a_ypart = A.take(sizeof(double) * 2 * NYF * (size_t)K);
    P.a_rtab = A.take(sizeof(int32_t) * ((size_t)P.nrange_max + 1 + K + 1));
    P.a_bt = A.take(sizeof(double) * (size_t)K * npen * (p + 1) * P.nl16);
    P.a_tile = A.take(P.R.csc ? 0 : sizeof(double) * (size_t)P.R.ld * p);
    P.a_mtile = A.take(P.R.csc ? 0 : sizeof(double) * (size_t)oemgpu_moments_len(p));
    P.bytes = A.off;
    return P;
}

int xval_sparse_ranges(const XvalSparsePlan &P, const int64_t *fold_n, std::vector<int32_t> &rtab, std::vector<int32_t> &frange, int64_t *npad)
{
    rtab.assign(1, 0);
    frange.assign((size_t)P.K + 1, 0);
    int64_t chunk = 0;
    for (int k = 0; k < P.K; ++k) {
        const int64_t nc = (fold_n[k] + SRC - 1) / SRC;
        frange[k] = (int32_t)rtab.size() - 1;
        for (int64_t c = 0; c < nc; c += P.per) rtab.push_back((int32_t)(chunk + (c + P.per < nc ? c + P.per : nc)));
        if ((int64_t)rtab.size() - 1 - frange[k] > P.rpf_max) { set_error("internal: a fold has more chunk ranges than planned"); return OEMGPU_ERR_INTERNAL; }
        chunk += nc;
    }
    frange[P.K] = (int32_t)rtab.size() - 1;
    if (chunk > P.nchunk_max || frange[P.K] > P.nrange_max) { set_error("internal: fold layout larger than planned"); return OEMGPU_ERR_INTERNAL; }
    *npad = chunk * SRC;
    return 0;
}

// ---------------------------------------------------------------------------------------- launchers
int launch_csc_fold_permute(hipStream_t s, const int64_t *colptr, const int32_t *rowidx, const double *val, const double *y, const int32_t *foldid,
                            const int *pos, int64_t n, int p, int K, int64_t npad, int32_t *cfo, int32_t *prow, double *pval, double *yp)
{
    OEM_HIP(hipMemsetAsync(yp, 0, sizeof(double) * (size_t)npad, s));
    hipLaunchKernelGGL(y_fold_order_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, y, pos, n, yp);
    hipLaunchKernelGGL(csc_fold_permute_kernel, dim3(p), dim3(PT), sizeof(int) * (2 * (size_t)K + 1 + PT), s, colptr, rowidx, val, foldid, pos, K,
                       cfo, prow, pval);
    OEM_HIP(hipGetLastError());
    return 0;
}

int launch_csc_fold_moments(hipStream_t s, const int64_t *colptr, const int32_t *prow, const double *pval, const double *yp, const int32_t *cptr,
                            const int32_t *cfo, const int64_t *fold_start, const int64_t *fold_n, int p, int K, int nchunk, int nrange,
                            const int32_t *rtab, const int32_t *frange, double *gpart, double *ypart, double *mfold)
{
    int rc = launch_csc_gram_ranges(s, colptr, prow, pval, cptr, p, nchunk, nrange, rtab, gpart);
    if (rc) return rc;
    hipLaunchKernelGGL(csc_fold_stats_kernel, dim3(p + NYF, K), dim3(256), 0, s, colptr, prow, pval, yp, cfo, fold_start, fold_n, p, K, mfold, ypart);
    hipLaunchKernelGGL(csc_fold_finish_kernel, dim3((unsigned)(((size_t)p * p + 255) / 256), K), dim3(256), 0, s, gpart, frange, ypart, fold_n, p, mfold);
    OEM_HIP(hipGetLastError());
    return 0;
}

int launch_csr_rowptr(hipStream_t s, const int64_t *colptr, const int32_t *prow, const int32_t *cptr, int p, int nchunk, int64_t *rowptr)
{
    hipLaunchKernelGGL(csr_rowptr_kernel, dim3(nchunk), dim3(1024), 0, s, colptr, prow, cptr, p, nchunk, rowptr);
    OEM_HIP(hipGetLastError());
    return 0;
}

int launch_csr_cv_error(hipStream_t s, const XvalSparsePlan &P, const int64_t *rowptr, const int32_t *ccol, const double *cval, const double *yp,
                        const int64_t *fold_start, const int64_t *fold_n, const double *B, double *bt, int mae, double *part, double *out,
                        bool triples)
{
    const size_t total = (size_t)P.K * P.npen * (P.p + 1) * P.nl16;
    hipLaunchKernelGGL(coef_transpose_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, B, P.p + 1, P.nl, P.nl16, total, bt);
    hipLaunchKernelGGL(csr_cv_error_kernel, dim3(P.cv_nwg, P.npen, P.cv_lblk), dim3(64 * XVS_CVW), 0, s, rowptr, ccol, cval, yp, fold_start,
                       fold_n, P.K, P.p, bt, P.nl, mae, part);
    OEM_HIP(hipGetLastError());
    return launch_cv_finish(s, part, P.cv_waves, P.npen, P.nl, (double)P.n, out, triples);
}

int launch_csr_cv_fold_score(hipStream_t s, const CvSparseScorePlan &P, int p, const int64_t *rowptr, const int32_t *ccol, const double *cval,
                             const double *yp, const int64_t *fold_start, const int64_t *fold_n, const double *B, double *bt, int mae,
                             double *part, const int *ncol, double *triples, double *predmat, const int *inv, int64_t n)
{
    const size_t total = (size_t)P.K * P.npen * (p + 1) * P.nl16;
    hipLaunchKernelGGL(coef_transpose_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, B, p + 1, P.nl, P.nl16, total, bt);
    const dim3 grid(P.nwg, P.npen, P.lblk), block(64 * XVS_CVW);
    if (predmat)
        hipLaunchKernelGGL(csr_cv_fold_score_kernel<true>, grid, block, 0, s, rowptr, ccol, cval, yp, fold_start, fold_n, P.K, p, bt, P.nl, mae, ncol,
                           part, predmat, inv, n);
    else
        hipLaunchKernelGGL(csr_cv_fold_score_kernel<false>, grid, block, 0, s, rowptr, ccol, cval, yp, fold_start, fold_n, P.K, p, bt, P.nl, mae, ncol,
                           part, (double *)nullptr, (const int *)nullptr, n);
    OEM_HIP(hipGetLastError());
    return launch_cv_fold_finish(s, part, P.waves, P.K, P.npen, P.nl, ncol, triples);
}

// fold k of the wide scoring: raw [npen][nl][p + 1] (that fold's coefficients, already on the device) -> bt, then its nk held-out rows
// list[0 .. nk) -> the fold's wave partials part_k [waves][npen][nl16][4].  nk = 0: the partials are zeroed, nothing is read.
int launch_csr_cv_wide_score_fold(hipStream_t s, const CvWideScorePlan &P, int p, const int64_t *rowptr, const int32_t *ccol, const double *cval,
                                  const double *y, const int32_t *list, int nk, const double *raw, double *bt, int mae, const int *ncol,
                                  double *part_k, double *predmat, int64_t n)
{
    if (nk <= 0) {
        OEM_HIP(hipMemsetAsync(part_k, 0, P.part_bytes / P.K, s));
        return 0;
    }
    const size_t total = (size_t)P.npen * (p + 1) * P.nl16;
    hipLaunchKernelGGL(coef_transpose_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, raw, p + 1, P.nl, P.nl16, total, bt);
    const dim3 grid(P.nwg, P.npen, P.lblk), block(64 * XVS_CVW);
    if (predmat) hipLaunchKernelGGL(csr_cv_wide_score_kernel<true>, grid, block, 0, s, rowptr, ccol, cval, y, list, nk, p, bt, P.nl, mae, ncol, part_k, predmat, n);
    else hipLaunchKernelGGL(csr_cv_wide_score_kernel<false>, grid, block, 0, s, rowptr, ccol, cval, y, list, nk, p, bt, P.nl, mae, ncol, part_k, (double *)nullptr, n);
    OEM_HIP(hipGetLastError());
    return 0;
}

}  // namespace oemgpu
