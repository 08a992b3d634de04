// xval.hip -- the device side of xval.oem (ref src/oem_xval_dense.{h,cpp}).
//
// The reference builds one Gram per fold from a gathered copy of the fold's rows (ref src/oem_xval_dense.h:358-484), fits
// K+1 models on sums of them (:733-853) and then walks the observations once more for the cross-validation error
// (ref src/oem_xval_dense.cpp:343-461).  Here:
//   * fold layout: rows are permuted ONCE into fold-contiguous order (stable inside a fold, so every run sums in the same
//     order): block histograms -> per-fold scan -> stable ranks by wave ballots -> a gather pass (coalesced reads, K write
//     streams).  Fold segments start on multiples of 16 rows, so each one meets the alignment the MFMA Gram kernels want;
//   * per-fold moments: the one-pass moment kernels of gram.hip on each segment (launched from api.hip);
//   * leave-one-fold-out sums: fold_sum_kernel, in fold order like the reference;
//   * CV error: predictions of a fold's rows under that fold's K-th fit for ALL lambdas are an (n_k x p) x (p x nlambda)
//     product -- as many flops as the Gram build -- so it runs on the FP64 MFMA pipe: a 16-row tile of X against 16-lambda
//     tiles of the coefficient matrix held in LDS, the intercept riding along as one more column of ones.  The epilogue
//     turns the accumulators into squared / absolute residuals and keeps per-lambda sums of the error and its square;
//     workgroup partials are combined in a fixed order.
#include "common.hpp"

namespace oemgpu {
namespace {

constexpr int FB = 1024;                 // rows per layout block

// ---------------------------------------------------------------------------------------- fold layout
__global__ __launch_bounds__(FB) void fold_count_kernel(const int *__restrict__ foldid, int64_t n, int K,
                                                        int *__restrict__ blockcnt, int *__restrict__ bad)
{
    extern __shared__ int hist[];
    for (int k = threadIdx.x; k < K; k += FB) hist[k] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (i < n) {
        const int f = foldid[i];
        if (f < 1 || f > K) atomicOr(bad, 1);
        else atomicAdd(&hist[f - 1], 1);              // integer: the order of the adds does not matter
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += FB) blockcnt[(size_t)blockIdx.x * K + k] = hist[k];
}

// one wave per fold: exclusive prefix of the fold's block counts, 64 blocks per step
__global__ __launch_bounds__(64) void fold_scan_kernel(int *__restrict__ blockcnt, int nblk, int K, int64_t *__restrict__ fold_n)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    int64_t run = 0;
    for (int b0 = 0; b0 < nblk; b0 += 64) {
        const int b = b0 + lane;
        const int c = b < nblk ? blockcnt[(size_t)b * K + k] : 0;
        int incl = c;
        for (int s = 1; s < 64; s <<= 1) { const int t = __shfl_up(incl, s, 64); if (lane >= s) incl += t; }
        if (b < nblk) blockcnt[(size_t)b * K + k] = (int)(run + incl - c);
        run += __shfl(incl, 63, 64);
    }
    if (lane == 0) fold_n[k] = run;
}

__global__ void fold_start_kernel(const int64_t *__restrict__ fold_n, int K, int64_t *__restrict__ fold_start, int align)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int64_t s = 0;
        for (int k = 0; k < K; ++k) { fold_start[k] = s; s += (fold_n[k] + align - 1) / align * align; }
    }
}

__global__ __launch_bounds__(FB) void fold_pos_kernel(const int *__restrict__ foldid, int64_t n, int K,
                                                      const int *__restrict__ blockoff, const int64_t *__restrict__ fold_start,
                                                      int *__restrict__ pos)
{
    extern __shared__ int wcnt[];                     // [16][K]
    const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int f = -1;
    if (i < n) { f = foldid[i] - 1; if (f < 0 || f >= K) f = -1; }
    int rank = 0;
    for (int k = 0; k < K; ++k) {
        const unsigned long long m = __ballot(f == k);
        if (lane == 0) wcnt[w * K + k] = __popcll(m);
        if (f == k) rank = __popcll(m & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (f >= 0) {
        int pre = 0;
        for (int ww = 0; ww < w; ++ww) pre += wcnt[ww * K + f];
        pos[i] = (int)(fold_start[f] + blockoff[(size_t)blockIdx.x * K + f] + pre + rank);
    }
}

// rows into fold-contiguous order: reads coalesced along the rows of a column, writes in K streams
constexpr int GCB = 8;                   // columns per gather block
__global__ __launch_bounds__(256) void gather_rows_kernel(const double *__restrict__ x, int64_t n, int64_t ld, int p,
                                                          const double *__restrict__ y, const int *__restrict__ pos,
                                                          double *__restrict__ xo, int64_t ldo, double *__restrict__ yo)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t d = pos[i];
    const int c0 = blockIdx.y * GCB;
#pragma unroll
    for (int c = 0; c < GCB; ++c)
        if (c0 + c < p) xo[(size_t)(c0 + c) * ldo + d] = x[(size_t)(c0 + c) * ld + i];
    if (blockIdx.y == 0) yo[d] = y[i];
}

// The same from a ROW-major x of float64 or float32 elements (x[i * ldr + c], read where it lies): the transposing counterpart.  A
// workgroup takes a tile of GRM_ROWS rows x GRM_COLS columns (tile t: row tile t / nct, column tile t % nct, so the column tiles of
// the same rows run side by side and share the lines their row segments straddle).  Read with the lanes along a row -- 32 elements,
// 256 B (float32: 128 B) contiguous per row, two rows per wave and load, one element per lane: no load is wider than the element,
// so x needs its element's alignment only -- widened in the register, through LDS, and written with the lanes along the 64 rows of
// one destination column: the rows of a fold that lie in the tile land in consecutive positions (pos increases within a fold), the
// K write streams of gather_rows_kernel.  LDS: [64][33] doubles.  The stores of a row segment (ds_write_b64: 16-lane groups, 32 banks)
// hit consecutive doubles; the transposed loads (ds_read_b64: 32-lane halves, 64 banks) are 33 doubles apart, lane r on the bank pair
// (2 r + 2 c) mod 64: both without conflicts.  Columns >= p and rows >= n are never loaded; a row whose fold id is outside 1..K has no
// position (fold_pos_kernel leaves it unset) and writes nothing.  No arithmetic, no atomics, every destination written once.
constexpr int GRM_ROWS = 64, GRM_COLS = 32;
template <typename T>
__global__ __launch_bounds__(256) void fold_gather_rm_kernel(const T *__restrict__ x, int64_t n, int64_t ldr, int p, int nct,
                                                             const double *__restrict__ y, const int *__restrict__ foldid, int K,
                                                             const int *__restrict__ pos, double *__restrict__ xo, int64_t ldo,
                                                             double *__restrict__ yo)
{
    __shared__ double tile[GRM_ROWS][GRM_COLS + 1];
    const int64_t rt = (int64_t)blockIdx.x / nct;
    const int ct = (int)((int64_t)blockIdx.x - rt * nct);
    const int64_t i0 = rt * GRM_ROWS;
    const int c0 = ct * GRM_COLS;
    const int tid = threadIdx.x;
    // this lane's destination row first: the fold id and the position are on their way while the tile is loaded
    const int r = tid & (GRM_ROWS - 1), cc = tid >> 6;              // (the store phase: 64 rows of 4 columns per step)
    int64_t d = -1;
    if (i0 + r < n) {
        const int f = foldid[i0 + r];
        if (f >= 1 && f <= K) d = pos[i0 + r];
    }
    {
        const int lc = tid & (GRM_COLS - 1), lr = tid >> 5;         // the load phase: 8 rows of 32 columns per step
        double v[GRM_ROWS / 8];
#pragma unroll
        for (int k = 0; k < GRM_ROWS / 8; ++k) {
            const int64_t i = i0 + lr + 8 * k;
            v[k] = (c0 + lc < p && i < n) ? (double)x[i * ldr + (c0 + lc)] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < GRM_ROWS / 8; ++k) tile[lr + 8 * k][lc] = v[k];
    }
    __syncthreads();
    if (d < 0) return;                                              // a row >= n, or one whose fold id is outside 1..K (its pos is unset)
#pragma unroll
    for (int k = 0; k < GRM_COLS / 4; ++k) {
        const int c = cc + 4 * k;
        if (c0 + c < p) xo[(int64_t)(c0 + c) * ldo + d] = tile[r][c];
    }
    if (ct == 0 && cc == 0) yo[d] = y[i0 + r];
}

// xval_oem_multi: the rows of Y (element (i, r) at y[i * rs + r * cs], read where it lies) into fold order, Yp column-major with
// leading dimension ldp -- a response is then the contiguous vector yp of the kernels above.  Run once the fold ids have been found
// valid (every pos is set); the padding rows between the folds stay unwritten, as in xp, and nothing reads them.
__global__ __launch_bounds__(256) void gather_responses_kernel(const double *__restrict__ y, int64_t rs, int64_t cs, int64_t n, int m,
                                                               const int *__restrict__ pos, double *__restrict__ yo, int64_t ldo)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t d = pos[i];
    const int r0 = blockIdx.y * GCB;
#pragma unroll
    for (int r = 0; r < GCB; ++r)
        if (r0 + r < m) yo[(int64_t)(r0 + r) * ldo + d] = y[i * rs + (int64_t)(r0 + r) * cs];
}

// out = sum of the fold moments except fold `skip` (1-based; 0: none), in fold order (ref src/oem_xval_dense.h:733-742, 801-811)
__global__ __launch_bounds__(256) void fold_sum_kernel(const double *__restrict__ M, int K, size_t len, int skip, double *__restrict__ out)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= len) return;
    double s = 0.0;
    for (int k = 1; k <= K; ++k) if (k != skip) s += M[(size_t)(k - 1) * len + t];
    out[t] = s;
}

// ---------------------------------------------------------------------------------------- observation weights
// xp: the fold-ordered copy with p + 1 columns, column 0 = w (gathered), columns 1..p = x (gathered); yp = y (gathered).
// Workgroup (j, k): column j (1..p: x_j; p + 1: y) over the rows of fold k -- the UNWEIGHTED sum of squares of an x column (the
// reference does not standardise with respect to the weights, ref src/oem_xval_dense.h:533-535, 614) in a fixed order, then the
// column times sqrt(w), in place.  csq: [K][p + 1], entry p of a fold = its number of rows (filled by the y workgroup).
__global__ __launch_bounds__(256) void weight_scale_kernel(double *__restrict__ xp, int64_t ldp, double *__restrict__ yp, int p,
                                                           const int64_t *__restrict__ fold_start, const int64_t *__restrict__ fold_n,
                                                           double *__restrict__ csq)
{
    __shared__ double sh[256];
    const int j = blockIdx.x + 1, k = blockIdx.y, tid = threadIdx.x;
    const int64_t st = fold_start[k], nk = fold_n[k];
    double *col = (j <= p) ? xp + (size_t)j * ldp + st : yp + st;
    const double *wv = xp + st;
    double s = 0.0;
    for (int64_t r = tid; r < nk; r += 256) {
        const double v = col[r];
        s = fma(v, v, s);
        col[r] = v * sqrt(wv[r]);
    }
    sh[tid] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) { if (tid < h) sh[tid] += sh[tid + h]; __syncthreads(); }
    if (tid == 0) csq[(size_t)k * (p + 1) + (j <= p ? j - 1 : p)] = (j <= p) ? sh[0] : (double)nk;
}
// column 0 becomes sqrt(w) once every other column has used w
__global__ __launch_bounds__(256) void weight_sqrt_kernel(double *__restrict__ xp, const int64_t *__restrict__ fold_start,
                                                          const int64_t *__restrict__ fold_n)
{
    const int k = blockIdx.y;
    const int64_t st = fold_start[k], nk = fold_n[k];
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < nk; r += (int64_t)gridDim.x * 256) xp[st + r] = sqrt(xp[st + r]);
}

// Weighted fold sums -> XX, XY of oemXvalDense (ref src/oem_xval_dense.h:733-784 with XtWX_xval(_int), :486-623): Mw = moments of
// the p + 1 data columns [sqrt(w) | sqrt(w) X] and of sqrt(w) y ((p + 3)^2, lower triangle), cs = [sum x_j^2 (unweighted), rows].
// q = p + intercept.  stats as launch_finalize's (colsq_inv in the scale slots).
__global__ __launch_bounds__(256) void finalize_weighted_kernel(const double *__restrict__ Mw, const double *__restrict__ cs, int p,
                                                                int standardize, int intercept, double *__restrict__ xx,
                                                                double *__restrict__ xy, double *__restrict__ stats)
{
    const int q = p + (intercept ? 1 : 0), off = intercept ? 0 : 1, qm = p + 3;
    const double nobs = cs[p];
    auto cinv = [&](int c) -> double {                 // data column c of [sqrt(w) | X]: 1 for the intercept column
        if (c == 0 || !standardize) return 1.0;
        double v = cs[c - 1] / (nobs - 1.0);
        if (v == 0.0) v = 1.0;
        return 1.0 / sqrt(v);
    };
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    for (int t = tid; t < q * q; t += nth) {
        const int a = t % q + off, b = t / q + off;    // data columns
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        xx[t] = cinv(a) * Mw[(size_t)lo * qm + hi] * cinv(b) / nobs;
    }
    for (int t = tid; t < q; t += nth) xy[t] = cinv(t + off) * Mw[(size_t)(t + off) * qm + (p + 1)] / nobs;
    if (tid == 0) {
        stats[0] = 0.0; stats[1] = 1.0; stats[2] = Mw[(size_t)(p + 1) * qm + (p + 1)]; stats[3] = nobs;
        stats[stats_shift_flag(p)] = 0.0; stats[stats_shift_flag(p) + 1] = 0.0;
    }
    for (int t = tid; t < p; t += nth) { stats[4 + t] = 0.0; stats[4 + p + t] = cinv(t + 1); }
}

// ---------------------------------------------------------------------------------------- CV error
typedef double d4 __attribute__((ext_vector_type(4)));

// grid (workgroups per fold, K folds, npen); 512 threads = 2 waves per SIMD sharing one copy of the coefficients in LDS.
// B: [K][npen][nl][p + 1], row 0 of each column the intercept.  part: [K * gridDim.x * CVW][npen][nl16][4] per WAVE: rows, centre c, sum (v - c), sum (v - c)^2 -- merged by Chan's formula in cv_finish_kernel
// KC: k-steps (4 columns each) whose X fragments a lane holds at once (SINGLE: p + 1 <= 4 KC, one chunk per row tile).
// CHUNK (the coefficient tile of all p + 1 rows does not fit LDS beside LT lambda tiles -- p beyond ~160 at 100 lambdas): LDS holds KCH
// coefficient rows at a time; the workgroup's eight waves take one 16-row tile of X each ("round"), keep its LT accumulator tiles
// over the chunks, and the chunk is staged again (from L2: the K x npen x nl x (p + 1) coefficients are a few MB) for every round.
// X is still read ONCE per pass over the lambdas, and p has no limit: the traffic added is 16 LT / 128 bytes of L2 per byte of X.
constexpr int CVW = 8;                   // waves per workgroup
constexpr int CV_KC = 14;                // k-steps of X fragments a lane holds at once
constexpr int CV_KCH = 8 * CV_KC;        // coefficient rows per LDS chunk (CHUNK): two fragment loads of KC = 14 k-steps
constexpr size_t CV_LDS_MAX = 140 * 1024;   // the coefficient tile of a pass stays in LDS up to here
// PRED (cv.oem, family = "gaussian": fit.preval; no weights, wmode = 0): finish() also stores the accumulator tile -- yhat of the tile's
// 16 rows at the pass's lambdas -- into pa.pred[npen][nl][n] at the CALLER'S row, pa.inv[fold position]; columns >= pa.ncol[pen] (the
// penalty's valid leading columns) get NaN.  Without PRED the trailing argument is empty and the kernel is what it was without it.
template <bool PRED> struct CvPred {};
template <> struct CvPred<true> { double *pred; const int *inv; const int *ncol; int64_t n; };
// Many responses on one fold-ordered x (xval_oem_multi): grid.z = npen * nresp, response blockIdx.z / npen with its own y (yp + r * ystride),
// its own table (B + r * bstride) and its own partials (part + r * pstride), each laid out as for one response -- so a response's sums are
// taken in the order of the single-response launch of the same nwg.  nresp = 1 (every other caller): the kernel as it was.
struct CvMany { int nresp; long long ystride, bstride, pstride; };
template <int LT, int KC, bool SINGLE, bool CHUNK, bool PRED = false>
__global__ __launch_bounds__(64 * CVW) void cv_error_kernel(const double *__restrict__ xp, int64_t ldp, const double *__restrict__ yp,
                                                            const int64_t *__restrict__ fold_start, const int64_t *__restrict__ fold_n,
                                                            int p, const double *__restrict__ B, int nl, int mae, int wmode,
                                                            double *__restrict__ part, CvPred<PRED> pa, CvMany many)
{
    // wmode (observation weights): xp has p + 1 data columns -- column 0 = sqrt(w), columns 1..p = sqrt(w) x -- and yp = sqrt(w) y, so
    // the squared residual of the scaled row IS w (y - yhat)^2 (ref src/oem_xval_dense.cpp:389-437); |.| takes one more sqrt(w).
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int npen = gridDim.z / many.nresp, resp = blockIdx.z / npen, pen = blockIdx.z - resp * npen;
    const int k = blockIdx.y, nwg = gridDim.x, wg = blockIdx.x;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l16 = lane & 15, g = lane >> 4;
    const int Kd = p + 1, K4 = (Kd + 3) & ~3, nl16 = (nl + 15) & ~15, ntile = nl16 >> 4;
    constexpr int LW = 16 * LT;                       // lambdas per pass
    double *Bl = lds;                                 // [K4][LW]
    const int64_t start = fold_start[k], nk = fold_n[k];
    const double *Bsrc = B + resp * many.bstride + ((size_t)k * npen + pen) * nl * Kd;
    const double *xk = xp + start, *yk = yp + resp * many.ystride + start;
    double *dst = part + resp * many.pstride + ((((size_t)k * nwg + wg) * CVW + w) * npen + pen) * nl16 * 4;      // this wave's partial
    const int64_t stride = (int64_t)nwg * CVW;

    auto load_a = [&](double (&a)[KC], int64_t rt, int c0) {
        const int64_t arow = rt * 16 + l16;
        const bool avalid = arow < nk;
#pragma unroll
        for (int s_ = 0; s_ < KC; ++s_) {
            const int kk = c0 + 4 * s_ + g;
            double v = (!wmode && kk == p) ? 1.0 : 0.0;
            if (avalid && (wmode ? kk <= p : kk < p)) v = xk[(size_t)kk * ldp + arow];
            a[s_] = v;
        }
    };

    // coefficient rows [cc, cc + ncols) of the lambda tiles from l0 on -> Bl[ncols][LW]
    auto stage = [&](int l0, int cc, int ncols) {
        for (int idx = tid; idx < ncols * LW; idx += 64 * CVW) {
            const int c = cc + idx / LW, j = idx % LW, lam = l0 * 16 + j;
            double v = 0.0;
            if (lam < nl) {
                if (wmode) { if (c <= p) v = Bsrc[(size_t)lam * Kd + c]; }      // column 0 (sqrt(w)) meets the intercept
                else if (c < p) v = Bsrc[(size_t)lam * Kd + c + 1];
                else if (c == p) v = Bsrc[(size_t)lam * Kd];          // intercept: the column of ones
            }
            Bl[idx] = v;
        }
    };

    for (int l0 = 0; l0 < ntile; l0 += LT) {
        if constexpr (!CHUNK) {
            __syncthreads();
            stage(l0, 0, K4);
            __syncthreads();
        }
        // The reference runs Welford's update over the observations (ref src/oem_xval_dense.cpp:420-422,452-461).  Here every wave
        // accumulates sum (v - c) and sum (v - c)^2 about a centre c of its own -- the error of the FIRST row it meets, per lambda --
        // so nothing cancels however small the spread of the errors is next to their mean, and the wave partials
        // (rows, c, sums) are merged pairwise with Chan's formula.
        double s1[LT], s2[LT], cen[LT];
        double cnt = 0.0;
        bool have_c = false;
#pragma unroll
        for (int t = 0; t < LT; ++t) { s1[t] = 0.0; s2[t] = 0.0; cen[t] = 0.0; }
        d4 acc[LT];
        auto clear = [&]() {
#pragma unroll
            for (int t = 0; t < LT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
        };
        auto mac = [&](const double (&a)[KC], int c0, int cc) {       // cc: the coefficient row Bl starts at
#pragma unroll
            for (int s_ = 0; s_ < KC; ++s_) {
                const int kk = c0 + 4 * s_ + g;
                if (SINGLE || c0 + 4 * s_ < K4) {
                    const double *bp = Bl + (size_t)(kk < K4 ? kk - cc : 0) * LW + l16;
                    const double av = (kk < K4) ? a[s_] : 0.0;
#pragma unroll
                    for (int t = 0; t < LT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bp[16 * t], acc[t], 0, 0, 0);
                }
            }
        };
        // accumulator layout: register r of lane (g, l16) is (row 4 r + g, lambda l16) of the tile
        auto err_of = [&](double yv, double a, double sw) { const double res = yv - a; return mae ? fabs(res) * sw : res * res; };
        auto finish = [&](int64_t rt) {
            if (!have_c) {                                      // the tile's first row always exists (rt * 16 < nk): lanes g = 0, r = 0 hold it
                const double y0 = yk[rt * 16], sw0 = (wmode && mae) ? xk[rt * 16] : 1.0;
#pragma unroll
                for (int t = 0; t < LT; ++t) cen[t] = __shfl(err_of(y0, acc[t][0], sw0), l16, 64);
                have_c = true;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = rt * 16 + 4 * r + g;
                const bool ok = row < nk;
                const double yv = ok ? yk[row] : 0.0;
                const double sw = (ok && wmode && mae) ? xk[row] : 1.0;
                if (l16 == 0) cnt += ok ? 1.0 : 0.0;
#pragma unroll
                for (int t = 0; t < LT; ++t) {
                    const double dv = ok ? err_of(yv, acc[t][r], sw) - cen[t] : 0.0;
                    s1[t] += dv; s2[t] = fma(dv, dv, s2[t]);
                }
                if constexpr (PRED) {
                    const int64_t orig = ok ? (int64_t)pa.inv[start + row] : -1;
                    if (orig >= 0 && orig < pa.n) {
                        // blockIdx.z = resp * npen + pen: response resp's block of pred ([npen][nl][n] each) and its row of ncol
                        const int ncolp = pa.ncol[blockIdx.z];
#pragma unroll
                        for (int t = 0; t < LT; ++t) {
                            const int lam = l0 * 16 + 16 * t + l16;
                            if (lam < nl) pa.pred[((size_t)blockIdx.z * nl + lam) * pa.n + orig] = lam < ncolp ? acc[t][r] : __builtin_nan("");
                        }
                    }
                }
            }
        };
        // all fragments of a chunk are requested before its first MFMA; the second wave of the SIMD covers the wait
        if constexpr (!CHUNK) {
            for (int64_t rt = (int64_t)wg * CVW + w; rt * 16 < nk; rt += stride) {
                clear();
                for (int c0 = 0; c0 < K4; c0 += 4 * KC) {
                    double a[KC];
                    load_a(a, rt, c0);
                    mac(a, c0, 0);
                }
                finish(rt);
            }
        } else {
            // rounds: wave w of the workgroup takes row tile r0 + w; the barriers of the staging are met by all eight waves
            for (int64_t r0 = (int64_t)wg * CVW; r0 * 16 < nk; r0 += stride) {
                const int64_t rt = r0 + w;
                const bool valid = rt * 16 < nk;
                clear();
                for (int cc = 0; cc < K4; cc += CV_KCH) {
                    const int ncols = K4 - cc < CV_KCH ? K4 - cc : CV_KCH;
                    double a[KC];
                    if (valid) load_a(a, rt, cc);                       // in flight while the chunk is staged
                    __syncthreads();
                    stage(l0, cc, ncols);
                    __syncthreads();
                    if (valid) {
                        mac(a, cc, cc);
                        for (int c0 = cc + 4 * KC; c0 < cc + ncols; c0 += 4 * KC) { load_a(a, rt, c0); mac(a, c0, cc); }
                    }
                }
                if (valid) finish(rt);
            }
        }
        // the four row groups of a wave (fixed order); every wave leaves its own partial
        cnt += __shfl_xor(cnt, 16, 64); cnt += __shfl_xor(cnt, 32, 64);
        const double rows = __shfl(cnt, 0, 64);
#pragma unroll
        for (int t = 0; t < LT; ++t) {
            s1[t] += __shfl_xor(s1[t], 16, 64); s1[t] += __shfl_xor(s1[t], 32, 64);
            s2[t] += __shfl_xor(s2[t], 16, 64); s2[t] += __shfl_xor(s2[t], 32, 64);
            const int lam = l0 * 16 + 16 * t + l16;
            if (g == 0 && lam < nl16) {
                double *q = dst + (size_t)lam * 4;
                q[0] = rows; q[1] = cen[t]; q[2] = s1[t]; q[3] = s2[t];
            }
        }
    }
}

// (rows, mean, M2 = sum (v - mean)^2) of a set of observations; two sets merge by Chan, Golub & LeVeque's update
struct CvSet {
    double na = 0.0, ma = 0.0, qa = 0.0;
    __device__ void merge(double nb, double mb, double qb)
    {
        if (nb > 0.0) {
            if (na > 0.0) {
                const double nn = na + nb, dl = mb - ma;
                ma += dl * (nb / nn);
                qa += qb + dl * dl * (na * nb / nn);
                na = nn;
            } else { na = nb; ma = mb; qa = qb; }
        }
    }
};
// One wave merges the wave partials [b0, b0 + nparts) of one (penalty, lambda): lanes stride over them, then a fixed butterfly --
// reproducible.  Every lane returns the merged set.
__device__ __forceinline__ CvSet cv_merge_partials(const double *__restrict__ part, int b0, int nparts, int npen, int pen, int nl16, int lam, int lane)
{
    CvSet a;
    for (int b = lane; b < nparts; b += 64) {
        const double *q = part + (((size_t)(b0 + b) * npen + pen) * nl16 + lam) * 4;
        const double nb = q[0];
        if (nb > 0.0) { const double m1 = q[2] / nb; a.merge(nb, q[1] + m1, q[3] - q[2] * m1); }
    }
    for (int s_ = 32; s_ > 0; s_ >>= 1) {                       // fixed butterfly: reproducible
        const double nb = __shfl_xor(a.na, s_, 64), mb = __shfl_xor(a.ma, s_, 64), qb = __shfl_xor(a.qa, s_, 64);
        // both partners must end with the same numbers: merge in lane order (lower lane's set first)
        if (lane & s_) { const CvSet o = a; a.na = nb; a.ma = mb; a.qa = qb; a.merge(o.na, o.ma, o.qa); }
        else a.merge(nb, mb, qb);
    }
    return a;
}

// cvm = mean error, cvsd = sqrt(sample variance / n)  (ref src/oem_xval_dense.cpp:452-461).  One wave per (penalty, lambda) over the
// partials of all folds.
// triples: out[npen][nl][3] <- (count, mean, M2) of the rows seen instead (row shards: the caller merges them, oemgpu_xval_merge).
__global__ __launch_bounds__(64) void cv_finish_kernel(const double *__restrict__ part, int nparts, int npen, int nl, double n,
                                                       double *__restrict__ out /* [npen][nl][2] */, int triples, long long pstride)
{
    // blockIdx.y: the response (one but for xval_oem_multi), its partials pstride doubles and its outputs npen * nl * (2 or 3) further on
    const int t = blockIdx.x, lane = threadIdx.x;
    const int pen = t / nl, lam = t - pen * nl, nl16 = (nl + 15) & ~15;
    part += (long long)blockIdx.y * pstride;
    out += (size_t)blockIdx.y * npen * nl * (triples ? 3 : 2);
    const CvSet a = cv_merge_partials(part, 0, nparts, npen, pen, nl16, lam, lane);
    if (lane == 0) {
        if (triples) { out[(size_t)t * 3] = a.na; out[(size_t)t * 3 + 1] = a.ma; out[(size_t)t * 3 + 2] = a.qa; }
        else {
            out[(size_t)t * 2] = a.ma;                          // all n observations are in: the mean
            out[(size_t)t * 2 + 1] = sqrt((a.qa < 0.0 ? 0.0 : a.qa) / (n - 1.0)) / sqrt(n);
        }
    }
}

// cv.oem, family = "gaussian": cvcompute's fold means (R/utils.R:128-144) need one set per FOLD.  One wave per (fold, penalty, lambda)
// merges that fold's nwg * CVW wave partials -- they are laid out [K][nwg][CVW] -- as above; out[K][npen][nl][3] <- (count, mean, M2),
// (0, NaN, NaN) for a column >= ncol[pen] (not valid for that penalty) and for a fold without rows.
__global__ __launch_bounds__(64) void cv_fold_finish_kernel(const double *__restrict__ part, int per_fold, int npen, int nl,
                                                            const int *__restrict__ ncol, double *__restrict__ out, long long pstride)
{
    // blockIdx.z: the response (one but for cv_oem_multi), its partials pstride doubles, its ncol row npen and its block K npen nl 3 further on
    const int t = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    const int pen = t / nl, lam = t - pen * nl, nl16 = (nl + 15) & ~15;
    part += (long long)blockIdx.z * pstride;
    ncol += (size_t)blockIdx.z * npen;
    out += (size_t)blockIdx.z * gridDim.y * npen * nl * 3;
    CvSet a;
    if (lam < ncol[pen]) a = cv_merge_partials(part, k * per_fold, per_fold, npen, pen, nl16, lam, lane);
    if (lane == 0) {
        double *o = out + ((size_t)k * npen * nl + t) * 3;
        const bool some = a.na > 0.0;
        o[0] = some ? a.na : 0.0; o[1] = some ? a.ma : __builtin_nan(""); o[2] = some ? a.qa : __builtin_nan("");
    }
}

// cv_oem_multi: the fold tables of a chunk of responses, each on ITS OWN lambda grid, onto the grids of the responses' full fits
// (predict.oem's lambda.interp, R/utils.R:64-144, R/cv_oem.R:364-391).  raw / tab: [nb][K][npen][nl][p + 1]; idx[nb][K][npen][nl] the
// (left, right, frac) the host worked out from the grids; ncol[nb][npen] the valid leading columns.  One workgroup per (column, fold,
// response x penalty), threads over the p + 1 coefficients: tab = raw[left] frac + raw[right] (1 - frac), zero from ncol on.  Every
// entry is written by one thread: no atomics, the same bytes every time.
__global__ __launch_bounds__(256) void cv_interp_kernel(const double *__restrict__ raw, const CvInterpIdx *__restrict__ idx,
                                                        const int *__restrict__ ncol, int npen, int nl, int Kd, double *__restrict__ tab)
{
    const int j = blockIdx.x, k = blockIdx.y, K = gridDim.y, z = blockIdx.z, resp = z / npen, pen = z - resp * npen;
    const size_t col0 = (((size_t)resp * K + k) * npen + pen) * nl;         // column 0 of this (response, fold, penalty)
    double *dst = tab + (col0 + j) * Kd;
    if (j >= ncol[z]) {
        for (int i = threadIdx.x; i < Kd; i += blockDim.x) dst[i] = 0.0;
        return;
    }
    const CvInterpIdx e = idx[col0 + j];
    const bool ok = e.left >= 0 && e.left < nl && e.right >= 0 && e.right < nl;       // (the host's table: never read beyond the block)
    const double *bl = raw + (col0 + (ok ? e.left : 0)) * Kd, *br = raw + (col0 + (ok ? e.right : 0)) * Kd;
    const double f = e.frac, g = 1.0 - e.frac;
    for (int i = threadIdx.x; i < Kd; i += blockDim.x) dst[i] = ok ? bl[i] * f + br[i] * g : __builtin_nan("");
}

// inv[fold position] = the caller's row (the inverse of fold_pos_kernel's map; the padding between the folds stays unset and is never read)
__global__ __launch_bounds__(256) void fold_inverse_kernel(const int *__restrict__ pos, int64_t n, int64_t ldp, int *__restrict__ inv)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t d = pos[i];
    if (d >= 0 && d < ldp) inv[d] = (int)i;
}

}  // namespace

// ---------------------------------------------------------------------------------------- launchers
size_t fold_layout_ints(int64_t n, int K) { return (size_t)((n + FB - 1) / FB) * K + 8; }

int launch_fold_layout(hipStream_t s, const int *foldid, int64_t n, int K, int *blockcnt, int64_t *fold_n, int64_t *fold_start,
                       int *pos, int *bad, int align)
{
    const int nblk = (int)((n + FB - 1) / FB);
    OEM_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
    hipLaunchKernelGGL(fold_count_kernel, dim3(nblk), dim3(FB), sizeof(int) * K, s, foldid, n, K, blockcnt, bad);
    hipLaunchKernelGGL(fold_scan_kernel, dim3(K), dim3(64), 0, s, blockcnt, nblk, K, fold_n);
    hipLaunchKernelGGL(fold_start_kernel, dim3(1), dim3(64), 0, s, fold_n, K, fold_start, align);
    hipLaunchKernelGGL(fold_pos_kernel, dim3(nblk), dim3(FB), sizeof(int) * 16 * K, s, foldid, n, K, blockcnt, fold_start, pos);
    OEM_HIP(hipGetLastError());
    return 0;
}

int launch_gather_rows(hipStream_t s, const double *x, int64_t n, int64_t ld, int p, const double *y, const int *pos,
                       double *xo, int64_t ldo, double *yo)
{
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((n + 255) / 256), (p + GCB - 1) / GCB), dim3(256), 0, s, x, n, ld, p,
                       y, pos, xo, ldo, yo);
    OEM_HIP(hipGetLastError());
    return 0;
}

int launch_gather_responses(hipStream_t s, const double *y, int64_t rs, int64_t cs, int64_t n, int m, const int *pos, double *yo, int64_t ldo)
{
    if ((m + GCB - 1) / GCB > 65535) { set_error("xval_multi: more responses than the gather of Y takes in one launch"); return OEMGPU_ERR_UNSUPPORTED; }
    hipLaunchKernelGGL(gather_responses_kernel, dim3((unsigned)((n + 255) / 256), (m + GCB - 1) / GCB), dim3(256), 0, s, y, rs, cs, n, m, pos, yo, ldo);
    OEM_HIP(hipGetLastError());
    return 0;
}

int launch_gather_rows_rm(hipStream_t s, const void *x, int dtype, int64_t n, int64_t ldr, int p, const double *y, const int *foldid, int K,
                          const int *pos, double *xo, int64_t ldo, double *yo)
{
    const int nct = (p + GRM_COLS - 1) / GRM_COLS;
    const int64_t tiles = ((n + GRM_ROWS - 1) / GRM_ROWS) * nct;
    if (tiles > 0x7fffffff) { set_error("fold gather of a row-major x: %lld x %d is more tiles than one launch takes", (long long)n, p); return OEMGPU_ERR_UNSUPPORTED; }
    if (dtype == OEMGPU_F32)
        hipLaunchKernelGGL(fold_gather_rm_kernel<float>, dim3((unsigned)tiles), dim3(256), 0, s, (const float *)x, n, ldr, p, nct, y, foldid, K,
                           pos, xo, ldo, yo);
    else
        hipLaunchKernelGGL(fold_gather_rm_kernel<double>, dim3((unsigned)tiles), dim3(256), 0, s, (const double *)x, n, ldr, p, nct, y, foldid, K,
                           pos, xo, ldo, yo);
    OEM_HIP(hipGetLastError());
    return 0;
}

int launch_weight_scale(hipStream_t s, double *xp, int64_t ldp, double *yp, int p, int K, const int64_t *fold_start, const int64_t *fold_n,
                        double *csq)
{
    hipLaunchKernelGGL(weight_scale_kernel, dim3(p + 1, K), dim3(256), 0, s, xp, ldp, yp, p, fold_start, fold_n, csq);
    hipLaunchKernelGGL(weight_sqrt_kernel, dim3(64, K), dim3(256), 0, s, xp, fold_start, fold_n);
    OEM_HIP(hipGetLastError());
    return 0;
}

int launch_finalize_weighted(hipStream_t s, const double *Mw, const double *cs, int p, int standardize, int intercept, double *xx,
                             double *xy, double *stats)
{
    const int q = p + (intercept ? 1 : 0);
    int blocks = (q * q + 255) / 256;
    if (blocks > 512) blocks = 512;
    hipLaunchKernelGGL(finalize_weighted_kernel, dim3(blocks), dim3(256), 0, s, Mw, cs, p, standardize, intercept, xx, xy, stats);
    OEM_HIP(hipGetLastError());
    return 0;
}

int launch_fold_sum(hipStream_t s, const double *M, int K, size_t len, int skip, double *out)
{
    hipLaunchKernelGGL(fold_sum_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s, M, K, len, skip, out);
    OEM_HIP(hipGetLastError());
    return 0;
}

// The host plan of the CV-error launch, the ONE place its shape is decided (launch_cv_error and oemgpu_selftest_xval_cv_plan read it).
//   workgroups per fold: one workgroup fills a CU (LDS), and all of them carry the same work: the grid must not exceed the CU count
//     by a few (260 workgroups on 256 CUs take two rounds), so round DOWN;
//   lambdas per pass: at most 7 16-wide tiles (accumulator registers), in even passes; all of them in one pass whenever there are
//     <= 112 lambdas, so that X is read once;
//   form: the coefficient tile of those lambdas stays in LDS for the whole pass when it fits 140 KB (SINGLE when a lane holds all
//     the k-steps of a row at once, p + 1 <= 56); beyond that (p + 1 > ~160 at 100 lambdas) it goes through LDS in chunks of CV_KCH
//     rows (CHUNK above) -- no limit on p (this used to shrink the lambda tile instead, re-reading X up to seven times, and to
//     refuse p > 1,183).
CvErrPlan cv_error_plan(int64_t n, int p, int K, int npen, int nl, int num_cu)
{
    CvErrPlan P;
    P.K4 = (p + 1 + 3) & ~3;
    P.ntile = (nl + 15) >> 4;
    int lt = P.ntile < 7 ? P.ntile : 7;
    if (P.ntile > lt) { const int np_ = (P.ntile + lt - 1) / lt; lt = (P.ntile + np_ - 1) / np_; }   // even passes
    P.lt = lt;
    P.passes = (P.ntile + lt - 1) / lt;                                                  // the kernel's loop over l0
    const bool chunk = (size_t)P.K4 * 16 * lt * sizeof(double) > CV_LDS_MAX;
    P.form = chunk ? CV_FORM_CHUNK : (P.K4 / 4 <= CV_KC ? CV_FORM_SINGLE : CV_FORM_MULTI);
    P.lds = (size_t)(chunk ? CV_KCH : P.K4) * 16 * lt * sizeof(double);
    P.chunks = chunk ? (P.K4 + CV_KCH - 1) / CV_KCH : 1;
    P.last = P.K4 - (P.chunks - 1) * CV_KCH;
    int nwg = num_cu / (K * npen);
    const int64_t tiles = (n / K + 16 * CVW - 1) / (16 * CVW);
    if (nwg > tiles) nwg = (int)tiles;
    P.nwg = nwg < 1 ? 1 : nwg;
    return P;
}
// nb responses in the grid: the CUs are divided among K * npen * nb (fold, penalty, response) triples, floored at one workgroup
CvErrPlan cv_error_plan_many(int64_t n, int p, int K, int npen, int nl, int nb, int num_cu)
{
    CvErrPlan P = cv_error_plan(n, p, K, npen, nl, num_cu);
    int nwg = (int)((int64_t)num_cu / ((int64_t)K * npen * (nb < 1 ? 1 : nb)));
    if (nwg > P.nwg) nwg = P.nwg;                                                        // (the row-tile bound of cv_error_plan)
    P.nwg = nwg < 1 ? 1 : nwg;
    return P;
}
size_t cv_part_doubles(int nwg, int K, int npen, int nl) { return (size_t)nwg * K * CVW * npen * ((nl + 15) & ~15) * 4; }

// pred != nullptr: the PRED instantiation (no weights there)
template <int LT>
static int launch_cv_lt(hipStream_t s, dim3 grid, size_t lds, int form, const double *xp, int64_t ldp, const double *yp,
                        const int64_t *fold_start, const int64_t *fold_n, int p, const double *B, int nl, int mae, int wmode, double *part,
                        double *pred = nullptr, const int *inv = nullptr, const int *ncol = nullptr, int64_t n = 0, CvMany many = CvMany{1, 0, 0, 0})
{
#define OEM_CVK(KC, SINGLE, CHUNK)                                                                                                   \
    do {                                                                                                                             \
        if (pred) {                                                                                                                  \
            OEM_HIP(hipFuncSetAttribute((const void *)cv_error_kernel<LT, KC, SINGLE, CHUNK, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
            hipLaunchKernelGGL((cv_error_kernel<LT, KC, SINGLE, CHUNK, true>), grid, dim3(64 * CVW), lds, s, xp, ldp, yp, fold_start, fold_n, p, B, nl, mae, 0, part, CvPred<true>{pred, inv, ncol, n}, many); \
        } else {                                                                                                                     \
            OEM_HIP(hipFuncSetAttribute((const void *)cv_error_kernel<LT, KC, SINGLE, CHUNK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
            hipLaunchKernelGGL((cv_error_kernel<LT, KC, SINGLE, CHUNK>), grid, dim3(64 * CVW), lds, s, xp, ldp, yp, fold_start, fold_n, p, B, nl, mae, wmode, part, CvPred<false>{}, many); \
        }                                                                                                                            \
    } while (0)
    if (form == CV_FORM_CHUNK) OEM_CVK(CV_KC, false, true);
    else if (form == CV_FORM_SINGLE) OEM_CVK(CV_KC, true, false);
    else OEM_CVK(CV_KC, false, false);   // 28 fragments at once spill next to 7 accumulator tiles
#undef OEM_CVK
    OEM_HIP(hipGetLastError());
    return 0;
}

// the product alone: every wave's partial into part
static int launch_cv_product(hipStream_t s, const double *xp, int64_t ldp, const double *yp, const int64_t *fold_start, const int64_t *fold_n,
                             int K, int p, const double *B, int npen, int nl, int mae, int wmode, const CvErrPlan &P, double *part,
                             double *pred = nullptr, const int *inv = nullptr, const int *ncol = nullptr, int64_t n = 0, CvMany many = CvMany{1, 0, 0, 0})
{
    dim3 grid(P.nwg, K, npen * many.nresp);
    int rc;
#define OEM_CVLT(LT) case LT: rc = launch_cv_lt<LT>(s, grid, P.lds, P.form, xp, ldp, yp, fold_start, fold_n, p, B, nl, mae, wmode, part, pred, inv, ncol, n, many); break
    switch (P.lt) {
    OEM_CVLT(1); OEM_CVLT(2); OEM_CVLT(3); OEM_CVLT(4); OEM_CVLT(5); OEM_CVLT(6); OEM_CVLT(7);
    default: return OEMGPU_ERR_INTERNAL;
    }
#undef OEM_CVLT
    return rc;
}

int launch_cv_error(hipStream_t s, const double *xp, int64_t ldp, const double *yp, const int64_t *fold_start, const int64_t *fold_n,
                    int K, int p, const double *B, int npen, int nl, int mae, int wmode, const CvErrPlan &P, double n, double *part, double *out,
                    bool triples)
{
    int rc = launch_cv_product(s, xp, ldp, yp, fold_start, fold_n, K, p, B, npen, nl, mae, wmode, P, part);
    if (rc) return rc;
    hipLaunchKernelGGL(cv_finish_kernel, dim3(npen * nl), dim3(64), 0, s, part, P.nwg * K * CVW, npen, nl, n, out, triples ? 1 : 0, 0LL);
    OEM_HIP(hipGetLastError());
    return 0;
}

// nb responses in one product launch and one finish launch: response r reads yp + r * ldp (a column of the fold-ordered Yp) and
// B + r * K * npen * nl * (p + 1), leaves its partials at part + r * cv_part_doubles(P.nwg, ...) and (cvm, cvsd) at out + r * npen * nl * 2.
// P: cv_error_plan_many's (nwg divided among the responses).
int launch_cv_error_many(hipStream_t s, const double *xp, int64_t ldp, const double *Yp, const int64_t *fold_start, const int64_t *fold_n,
                         int K, int p, const double *B, int npen, int nl, int mae, const CvErrPlan &P, double n, int nb, double *part, double *out)
{
    if ((long long)npen * nb > 65535) { set_error("xval_multi: the CV-error launch has more (penalty, response) pairs than a launch takes"); return OEMGPU_ERR_UNSUPPORTED; }
    const long long pstride = (long long)cv_part_doubles(P.nwg, K, npen, nl);
    const CvMany many{nb, (long long)ldp, (long long)K * npen * nl * (p + 1), pstride};
    int rc = launch_cv_product(s, xp, ldp, Yp, fold_start, fold_n, K, p, B, npen, nl, mae, 0, P, part, nullptr, nullptr, nullptr, 0, many);
    if (rc) return rc;
    hipLaunchKernelGGL(cv_finish_kernel, dim3(npen * nl, nb), dim3(64), 0, s, part, P.nwg * K * CVW, npen, nl, n, out, 0, pstride);
    OEM_HIP(hipGetLastError());
    return 0;
}

int launch_fold_inverse(hipStream_t s, const int *pos, int64_t n, int64_t ldp, int *inv)
{
    hipLaunchKernelGGL(fold_inverse_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pos, n, ldp, inv);
    OEM_HIP(hipGetLastError());
    return 0;
}

int launch_cv_fold_error(hipStream_t s, const double *xp, int64_t ldp, const double *yp, const int64_t *fold_start, const int64_t *fold_n,
                         int K, int p, const double *B, int npen, int nl, int mae, const CvErrPlan &P, double *part, const int *ncol,
                         double *triples, double *predmat, const int *inv, int64_t n)
{
    int rc = launch_cv_product(s, xp, ldp, yp, fold_start, fold_n, K, p, B, npen, nl, mae, 0, P, part, predmat, inv, ncol, n);
    if (rc) return rc;
    return launch_cv_fold_finish(s, part, P.nwg * CVW, K, npen, nl, ncol, triples);
}

// the per-fold merge of launch_cv_fold_error alone, for partials [K][per_fold][npen][nl16][4] some other kernel wrote (xval_sparse.hip)
int launch_cv_fold_finish(hipStream_t s, const double *part, int per_fold, int K, int npen, int nl, const int *ncol, double *triples)
{
    hipLaunchKernelGGL(cv_fold_finish_kernel, dim3(npen * nl, K), dim3(64), 0, s, part, per_fold, npen, nl, ncol, triples, 0LL);
    OEM_HIP(hipGetLastError());
    return 0;
}

// launch_cv_fold_error for nb responses in one product launch and one finish launch (cv_oem_multi): response r reads Yp + r * ldp and
// B + r * K * npen * nl * (p + 1) and ncol + r * npen, leaves its partials at part + r * cv_part_doubles(P.nwg, ...), its triples at
// triples + r * K * npen * nl * 3 and, with predmat, yhat of its rows at predmat + r * npen * nl * n.  P: cv_error_plan_many's.
int launch_cv_fold_error_many(hipStream_t s, const double *xp, int64_t ldp, const double *Yp, const int64_t *fold_start, const int64_t *fold_n,
                              int K, int p, const double *B, int npen, int nl, int mae, const CvErrPlan &P, int nb, double *part, const int *ncol,
                              double *triples, double *predmat, const int *inv, int64_t n)
{
    if ((long long)npen * nb > 65535 || nb > 65535) { set_error("cv_multi: the CV-error launch has more (penalty, response) pairs than a launch takes"); return OEMGPU_ERR_UNSUPPORTED; }
    const long long pstride = (long long)cv_part_doubles(P.nwg, K, npen, nl);
    const CvMany many{nb, (long long)ldp, (long long)K * npen * nl * (p + 1), pstride};
    int rc = launch_cv_product(s, xp, ldp, Yp, fold_start, fold_n, K, p, B, npen, nl, mae, 0, P, part, predmat, inv, ncol, n, many);
    if (rc) return rc;
    hipLaunchKernelGGL(cv_fold_finish_kernel, dim3(npen * nl, K, nb), dim3(64), 0, s, part, P.nwg * CVW, npen, nl, ncol, triples, pstride);
    OEM_HIP(hipGetLastError());
    return 0;
}

int launch_cv_interp(hipStream_t s, const double *raw, const CvInterpIdx *idx, const int *ncol, int nb, int K, int npen, int nl, int p, double *tab)
{
    if ((long long)npen * nb > 65535 || K > 65535) { set_error("cv_multi: the interpolation launch has more (penalty, response) pairs than a launch takes"); return OEMGPU_ERR_UNSUPPORTED; }
    const int Kd = p + 1, threads = Kd >= 256 ? 256 : (Kd + 63) / 64 * 64;
    hipLaunchKernelGGL(cv_interp_kernel, dim3(nl, K, npen * nb), dim3(threads), 0, s, raw, idx, ncol, npen, nl, Kd, tab);
    OEM_HIP(hipGetLastError());
    return 0;
}

// the merge of launch_cv_error alone, for partials some other kernel wrote in the same layout (xval_sparse.hip)
int launch_cv_finish(hipStream_t s, const double *part, int nparts, int npen, int nl, double n, double *out, bool triples)
{
    hipLaunchKernelGGL(cv_finish_kernel, dim3(npen * nl), dim3(64), 0, s, part, nparts, npen, nl, n, out, triples ? 1 : 0, 0LL);
    OEM_HIP(hipGetLastError());
    return 0;
}

}  // namespace oemgpu

using namespace oemgpu;

extern "C" {
#pragma GCC visibility push(default)

int oemgpu_selftest_xval_cv_plan(int64_t n, int32_t p, int32_t nfolds, int32_t npen, int32_t nl, int32_t num_cu, int64_t *out)
{
    if (n < 1 || p < 1 || npen < 1 || nl < 1 || num_cu < 1 || !out) { set_error("selftest_xval_cv_plan: bad argument"); return OEMGPU_ERR_ARG; }
    if (nfolds < 2 || nfolds > 512) { set_error("selftest_xval_cv_plan: nfolds must be in 2..512"); return OEMGPU_ERR_ARG; }
    const CvErrPlan P = cv_error_plan(n, p, nfolds, npen, nl, num_cu);
    out[0] = P.lt; out[1] = P.passes; out[2] = P.form; out[3] = (int64_t)P.lds; out[4] = P.chunks; out[5] = P.last; out[6] = P.nwg;
    return 0;
}

#pragma GCC visibility pop
}
