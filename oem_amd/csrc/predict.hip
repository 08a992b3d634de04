// predict.hip -- predict.oem's product on the device (ref R/methods.R:48-109, 346-367): out[c][i] = f(b0_c + sum_j x_ij b_jc) for a dense x
// read where it lies (dense_src.hpp: column-major float64, row-major float64 / float32) or a resident sparse x (oemgpu_sparse_x), f one of
// identity ("link"), 1 / (1 + exp(-eta)) ("response") and eta > 0 ("class"), applied in the store.
//
// Dense: the product of xval.hip's cv_error_kernel without its fold layout and its error sums.  v_mfma_f64_16x16x4_f64 with 16 rows of x
// as the A operand (lane (l16, g) holds row l16, k slot g) and a 16-column tile of the coefficient table as B, the intercept riding along
// as the constant-1 pseudo-column p; register r of lane (g, l16) of the accumulator is (row 4 r + g, column l16).  The table is
// transposed once per call into bt[K4][nc16] (row k < p: the coefficients of x column k; row p: the intercepts; rows p + 1 .. K4 - 1 and
// columns >= ncol: zero) and staged into LDS from there with coalesced reads: the whole of it for the tiles of a pass when that fits
// PR_LDS_MAX, else PR_KCH rows at a time (CHUNK: the eight waves of a workgroup take one 16-row tile each per round and meet at the
// barriers of the staging; p has no limit).  A pass covers at most 7 tiles (accumulator registers), cv_error_plan's rule: x is read once
// while ncol <= 112.
//
// A workgroup owns a contiguous range of rows (a multiple of 128), its waves the 16-row tiles of it in turn.  A lane loads ONE element per
// k-step straight into operand layout -- column-major: 16 lanes along 128 contiguous bytes of a column; row-major: 4 consecutive elements
// of each of 16 rows, every cache line used whole over the 14 k-steps a lane holds at once -- so x needs its element's alignment only, and
// float32 is widened in the register it was loaded into.  The three layouts hand the MFMAs the same operand values in the same k order:
// the same bits.  Padding is made by SELECTION: rows >= n, columns >= p of the last k-step and columns p .. ldr - 1 of a row are never
// loaded, the lane's value is 0 (1 for the pseudo-column) instead, and the table's padding is zero: a NaN at x[i][j] reaches row i of out
// and nothing else (columns >= ncol of the last tile may see it; they are not stored).
//
// The store: each wave turns its 16 x 16 accumulator tile through 17-double rows of LDS of its own, so that 16 lanes write 128 contiguous
// bytes of one column of out ([ncol][n]); every element of out is written once.  No atomics; one order for every sum.
//
// Sparse: lane = row over the handle's compressed-row copy, stored entries in column order, scalar FP64 FMAs from b0 on (the walk of
// logit_cv_score_kernel), eight columns per walk; the waves of a workgroup share a row block's columns when there are more than eight of
// them and take row blocks of their own otherwise.  The table ([ncol][p + 1] as the caller gave it) sits in LDS when it fits PR_LDS_MAX
// and is read through the cache otherwise.
#include "logistic.hpp"

#include <algorithm>

namespace oemgpu {
namespace {

constexpr int PRW = 8;                       // waves per workgroup
constexpr int PR_KC = 14;                    // k-steps (4 columns each) of x fragments a lane has in flight at once
constexpr int PR_KCH = 8 * PR_KC;            // coefficient rows per LDS chunk (CHUNK)
constexpr size_t PR_LDS_MAX = 140 * 1024;    // the coefficient tile of a pass stays in LDS up to here
constexpr int PR_TS = 17;                    // doubles per row of a wave's transposing tile
constexpr size_t PR_LDS_TURN = sizeof(double) * PRW * 16 * PR_TS;

struct PredCm {                              // column-major float64, column stride ld
    const double *x;
    int64_t ld;
    __device__ __forceinline__ double at(int64_t row, int col) const { return x[(int64_t)col * ld + row]; }
};
template <typename T>
struct PredRm {                              // row-major float64 / float32, row stride ldr
    const T *x;
    int64_t ldr;
    __device__ __forceinline__ double at(int64_t row, int col) const { return (double)x[row * ldr + col]; }
};

__device__ __forceinline__ double pred_f(double eta, int type)
{
    if (type == 1) return 1.0 / (1.0 + exp(-eta));
    if (type == 2) return eta > 0.0 ? 1.0 : 0.0;
    return eta;
}

// raw: the caller's [ncol][p + 1] (slot 0 the intercept) -> bt[K4][nc16], the intercepts in row p, zero padding
__global__ __launch_bounds__(256) void predict_table_kernel(const double *__restrict__ raw, int p, int ncol, int K4, int nc16,
                                                            double *__restrict__ bt)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)K4 * nc16) return;
    const int r = (int)(idx / nc16), c = (int)(idx - (size_t)r * nc16);
    double v = 0.0;
    if (c < ncol) {
        if (r < p) v = raw[(size_t)c * (p + 1) + r + 1];
        else if (r == p) v = raw[(size_t)c * (p + 1)];
    }
    bt[idx] = v;
}

// One pass: the tiles l0 .. l0 + LT - 1 of the table's columns for all rows.  grid: workgroups of rpw rows; dynamic LDS: the staged
// coefficient rows [K4 or PR_KCH][16 LT], then the waves' transposing tiles.
template <int LT, bool CHUNK, class SRC>
__global__ __launch_bounds__(64 * PRW) void predict_kernel(const SRC X, int64_t n, int p, const double *__restrict__ bt, int nc16, int ncol,
                                                           int l0, int type, int64_t rpw, double *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    // (two sets of 7 k-steps where they are double-buffered; of 4 next to five and more accumulator tiles, which 7 would spill)
    constexpr int KC = CHUNK ? PR_KC : LT >= 5 ? 4 : PR_KC / 2, LW = 16 * LT;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l16 = lane & 15, g = lane >> 4;
    const int K4 = (p + 1 + 3) & ~3;
    double *Bl = lds;                                                        // [K4 or PR_KCH][LW]
    double *tr = lds + (size_t)(CHUNK ? PR_KCH : K4) * LW + (size_t)w * 16 * PR_TS;   // this wave's transposing tile
    const int64_t r_lo = (int64_t)blockIdx.x * rpw, r_hi = r_lo + rpw < n ? r_lo + rpw : n;

    auto load_a = [&](double (&a)[KC], int64_t rt, int c0) {
        const int64_t arow = rt * 16 + l16;
        const bool avalid = arow < n;
#pragma unroll
        for (int s_ = 0; s_ < KC; ++s_) {
            const int kk = c0 + 4 * s_ + g;
            double v = kk == p ? 1.0 : 0.0;                                  // the intercept's column of ones; padding
            if (avalid && kk < p) v = X.at(arow, kk);
            a[s_] = v;
        }
    };
    // coefficient rows [cc, cc + nrows) of this pass's tiles -> Bl[nrows][LW]
    auto stage = [&](int cc, int nrows) {
        for (int idx = tid; idx < nrows * LW; idx += 64 * PRW) {
            const int r = idx / LW, col = l0 * 16 + (idx - r * LW);
            Bl[idx] = col < nc16 ? bt[(size_t)(cc + r) * nc16 + col] : 0.0;
        }
    };
    v4d acc[LT];
    auto clear = [&]() {
#pragma unroll
        for (int t = 0; t < LT; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
    };
    auto mac = [&](const double (&a)[KC], int c0, int cc) {                  // cc: the coefficient row Bl starts at
#pragma unroll
        for (int s_ = 0; s_ < KC; ++s_) {
            if (c0 + 4 * s_ < K4) {                                          // (wave-uniform)
                const double *bp = Bl + (size_t)(c0 + 4 * s_ + g - cc) * LW + l16;
#pragma unroll
                for (int t = 0; t < LT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s_], bp[16 * t], acc[t], 0, 0, 0);
            }
        }
    };
    // register r of lane (g, l16) is (row 4 r + g, column l16) of a tile: through the wave's own LDS tile, so that 16 lanes store 16
    // consecutive rows of one column (LDS operations of a wave complete in order; the fences keep the compiler from reordering them)
    auto finish = [&](int64_t rt) {
        const int64_t row = rt * 16 + l16;
#pragma unroll
        for (int t = 0; t < LT; ++t) {
            const int cb = (l0 + t) * 16;
            if (cb >= ncol) break;                                           // (wave-uniform)
#pragma unroll
            for (int r = 0; r < 4; ++r) tr[(4 * r + g) * PR_TS + l16] = pred_f(acc[t][r], type);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = cb + g + 4 * r;
                const double v = tr[l16 * PR_TS + g + 4 * r];
                if (row < n && col < ncol) out[(int64_t)col * n + row] = v;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    };

    if constexpr (!CHUNK) {
        stage(0, K4);
        __syncthreads();
        // two sets of fragments: the loads of the next set are on their way while the MFMAs of this one run
        for (int64_t rt = r_lo / 16 + w; rt * 16 < r_hi; rt += PRW) {
            clear();
            double a0[KC], a1[KC];
            load_a(a0, rt, 0);
            for (int c0 = 0; c0 < K4; c0 += 8 * KC) {
                const bool second = c0 + 4 * KC < K4;
                if (second) load_a(a1, rt, c0 + 4 * KC);
                mac(a0, c0, 0);
                if (c0 + 8 * KC < K4) load_a(a0, rt, c0 + 8 * KC);
                if (second) mac(a1, c0 + 4 * KC, 0);
            }
            finish(rt);
        }
    } else {
        // rounds: wave w takes row tile r0 + w; the barriers of the staging are met by all eight waves (r0 and r_hi are the workgroup's)
        // One loop over (round, chunk): the fragments of a chunk's two halves are loaded while the MFMAs of the chunk before run -- the
        // first half's behind the first half's MFMAs, the second's behind the second's -- and are in flight over the staging and its
        // barriers, across the end of a round too.  The order of the MFMAs of a tile is that of the whole-table form.
        int64_t r0 = r_lo / 16;
        int cc = 0;
        double a0[KC], a1[KC];
        if ((r0 + w) * 16 < r_hi) {
            load_a(a0, r0 + w, 0);
            if (4 * KC < K4) load_a(a1, r0 + w, 4 * KC);
        }
        while (r0 * 16 < r_hi) {
            const int64_t rt = r0 + w;
            const bool valid = rt * 16 < r_hi;
            const int nrows = K4 - cc < PR_KCH ? K4 - cc : PR_KCH;
            const bool last = cc + PR_KCH >= K4;                             // the round's last chunk
            const int ncc = last ? 0 : cc + PR_KCH;
            const int64_t nr0 = last ? r0 + PRW : r0, nrt = nr0 + w;
            const bool nvalid = nrt * 16 < r_hi;
            if (cc == 0) clear();
            __syncthreads();
            stage(cc, nrows);
            __syncthreads();
            if (valid) mac(a0, cc, cc);
            if (nvalid) load_a(a0, nrt, ncc);
            if (valid && 4 * KC < nrows) mac(a1, cc + 4 * KC, cc);
            if (nvalid && ncc + 4 * KC < K4) load_a(a1, nrt, ncc + 4 * KC);
            if (valid && last) finish(rt);
            cc = ncc;
            r0 = nr0;
        }
    }
}

// ------------------------------------------------------------------------------------------------ resident sparse x
// tab: [ncol][p + 1], slot 0 the intercept.  WPR waves (1, 2 or 4) share the columns of a 64-row block, eight columns per walk.
template <bool TLDS>
__global__ __launch_bounds__(256) void predict_csr_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ ccol,
                                                          const double *__restrict__ cval, int64_t n, int p, const double *__restrict__ tab,
                                                          int ncol, int type, int wpr, int64_t ch, double *__restrict__ out)
{
    extern __shared__ double tl[];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, q = p + 1;
    if (TLDS) {
        for (int k = tid; k < ncol * q; k += 256) tl[k] = tab[k];
        __syncthreads();
    }
    const double *tb = TLDS ? tl : tab;
    const int rb = w / wpr, cg = w - rb * wpr, nrb = 4 / wpr;
    const int64_t r_lo = (int64_t)blockIdx.x * ch, r_hi = r_lo + ch < n ? r_lo + ch : n;
    for (int64_t r0 = r_lo + 64 * rb; r0 < r_hi; r0 += 64 * nrb) {
        const int64_t row = r0 + lane;
        const bool in = row < r_hi;
        const int64_t k0 = in ? rowptr[row] : 0, k1 = in ? rowptr[row + 1] : 0;
        for (int c0 = 8 * cg; c0 < ncol; c0 += 8 * wpr) {
            const double *tc[8];
            double eta[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                tc[k] = tb + (size_t)(c0 + k < ncol ? c0 + k : ncol - 1) * q;
                eta[k] = tc[k][0];
            }
            for (int64_t e = k0; e < k1; ++e) {
                const double v = cval[e];
                const int j = ccol[e];
#pragma unroll
                for (int k = 0; k < 8; ++k) eta[k] = fma(v, tc[k][1 + j], eta[k]);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (in && c0 + k < ncol) out[(int64_t)(c0 + k) * n + row] = pred_f(eta[k], type);
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ the plan (host arithmetic)
// the ONE place the dense launch is shaped (predict_dense and oemgpu_selftest_predict_plan read it)
struct PredictPlan {
    int K4, ntile, lt, passes, chunk, krows, nchunks;
    size_t lds;
    int64_t rpw, nwg;
};
static PredictPlan predict_plan(int64_t n, int p, int ncol, int num_cu)
{
    PredictPlan P;
    P.K4 = (p + 1 + 3) & ~3;
    P.ntile = (ncol + 15) >> 4;
    int lt = P.ntile < 7 ? P.ntile : 7;                                         // cv_error_plan's rule: at most 7 tiles, even passes
    if (P.ntile > lt) { const int np_ = (P.ntile + lt - 1) / lt; lt = (P.ntile + np_ - 1) / np_; }
    P.lt = lt;
    P.passes = (P.ntile + lt - 1) / lt;
    P.chunk = (size_t)P.K4 * 16 * lt * sizeof(double) > PR_LDS_MAX ? 1 : 0;
    P.krows = P.chunk ? PR_KCH : P.K4;
    P.nchunks = P.chunk ? (P.K4 + PR_KCH - 1) / PR_KCH : 1;
    P.lds = (size_t)P.krows * 16 * lt * sizeof(double) + PR_LDS_TURN;
    // workgroups of equal, contiguous row ranges (multiples of the 128 rows a workgroup's waves take at once): two on a CU while two
    // fit its LDS, and never more than one round of them
    const int per_cu = 2 * P.lds <= (size_t)160 * 1024 ? 2 : 1;
    const int64_t blocks = (n + 16 * PRW - 1) / (16 * PRW), target = (int64_t)num_cu * per_cu;
    P.rpw = (blocks + target - 1) / target * (16 * PRW);
    P.nwg = (n + P.rpw - 1) / P.rpw;
    return P;
}

template <int LT, bool CHUNK, class SRC>
static int predict_launch(hipStream_t s, const PredictPlan &P, const SRC X, int64_t n, int p, const double *bt, int nc16, int ncol, int l0, int type,
                          double *out)
{
    if (lds_limit_once(reinterpret_cast<const void *>(&predict_kernel<LT, CHUNK, SRC>), P.lds)) return OEMGPU_ERR_HIP;
    hipLaunchKernelGGL((predict_kernel<LT, CHUNK, SRC>), dim3((unsigned)P.nwg), dim3(64 * PRW), P.lds, s, X, n, p, bt, nc16, ncol, l0, type, P.rpw, out);
    return 0;
}

template <class SRC>
static int predict_passes(hipStream_t s, const PredictPlan &P, const SRC X, int64_t n, int p, const double *bt, int nc16, int ncol, int type,
                          double *out)
{
    for (int l0 = 0; l0 < P.ntile; l0 += P.lt) {
        int rc;
#define OEM_PRLT(LT)                                                                                               \
    case LT:                                                                                                       \
        rc = P.chunk ? predict_launch<LT, true, SRC>(s, P, X, n, p, bt, nc16, ncol, l0, type, out)                 \
                     : predict_launch<LT, false, SRC>(s, P, X, n, p, bt, nc16, ncol, l0, type, out);               \
        break
        switch (P.lt) {
        OEM_PRLT(1); OEM_PRLT(2); OEM_PRLT(3); OEM_PRLT(4); OEM_PRLT(5); OEM_PRLT(6); OEM_PRLT(7);
        default: return OEMGPU_ERR_INTERNAL;
        }
#undef OEM_PRLT
        if (rc) return rc;
    }
    OEM_HIP(hipGetLastError());
    return 0;
}

// what every entry asks of its table and its output, before any device is looked for
static int predict_common_check(const char *who, const void *c, const void *x, const double *coef, int32_t ncol, int32_t type, const double *out)
{
    if (!c || !x || !coef || !out) { set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG; }
    if (ncol < 1) { set_error("%s: bad ncol (ncol >= 1)", who); return OEMGPU_ERR_ARG; }
    if (type < 0 || type > 2) { set_error("%s: type must be 0 (link), 1 (response) or 2 (class)", who); return OEMGPU_ERR_ARG; }
    return 0;
}

// the one body of the two dense entries
static int predict_dense(const char *who, oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const double *coef, int32_t ncol, int32_t type,
                         double *out)
{
    if (int rc = predict_common_check(who, c, X.x, coef, ncol, type, out)) return rc;
    if (n < 1 || p < 1) { set_error("%s: bad n / p (n >= 1, p >= 1)", who); return OEMGPU_ERR_ARG; }
    if (int rc = dense_src_check(who, X, n, p)) return rc;
    if (X.colmajor() && (uintptr_t)X.x % 8) { set_error("%s: x_dev is not aligned to its 8-byte elements", who); return OEMGPU_ERR_ARG; }
    if (p > INT32_MAX - 8 || ncol > INT32_MAX - 16) { set_error("%s: p / ncol beyond int32", who); return OEMGPU_ERR_UNSUPPORTED; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    hipStream_t s = c->stream;
    const PredictPlan P = predict_plan(n, p, ncol, c->num_cu);
    const int nc16 = P.ntile * 16;
    Bump B;
    const size_t a_raw = B.take(sizeof(double) * (size_t)ncol * (p + 1)), a_bt = B.take(sizeof(double) * (size_t)P.K4 * nc16);
    if (ctx_reserve(c, B.off)) return OEMGPU_ERR_HIP;
    double *raw = (double *)(c->ws + a_raw), *bt = (double *)(c->ws + a_bt);
    OEM_HIP(hipMemcpyAsync(raw, coef, sizeof(double) * (size_t)ncol * (p + 1), hipMemcpyHostToDevice, s));
    const size_t cells = (size_t)P.K4 * nc16;
    hipLaunchKernelGGL(predict_table_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, raw, p, ncol, P.K4, nc16, bt);
    int rc;
    if (X.colmajor()) rc = predict_passes(s, P, PredCm{X.cm(), X.ld}, n, p, bt, nc16, ncol, type, out);
    else if (X.dtype == OEMGPU_F32) rc = predict_passes(s, P, PredRm<float>{(const float *)X.x, X.ld}, n, p, bt, nc16, ncol, type, out);
    else rc = predict_passes(s, P, PredRm<double>{(const double *)X.x, X.ld}, n, p, bt, nc16, ncol, type, out);
    if (rc) return rc;
    OEM_HIP(hipStreamSynchronize(s));                                           // the caller's table may go once this returns
    return 0;
}

}  // namespace oemgpu

using namespace oemgpu;

extern "C" {
#pragma GCC visibility push(default)

int oemgpu_predict_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *coef, int32_t ncol, int32_t type,
                       double *out_dev)
{
    return predict_dense("predict", c, dense_src_cm(x_dev, ld), n, p, coef, ncol, type, out_dev);
}

int oemgpu_predict_rm_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *coef, int32_t ncol,
                          int32_t type, double *out_dev)
{
    return predict_dense("predict_rm", c, dense_src_rm(x_dev, dtype, ldr), n, p, coef, ncol, type, out_dev);
}

int oemgpu_predict_sparse_res(oemgpu_ctx *c, const oemgpu_sparse_x *x, const double *coef, int32_t ncol, int32_t type, double *out_dev)
{
    if (int rc = predict_common_check("predict_sparse", c, x, coef, ncol, type, out_dev)) return rc;
    if (c->device != x->device) { set_error("predict_sparse: the context and the sparse x are on different devices"); return OEMGPU_ERR_ARG; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    hipStream_t s = c->stream;
    const int64_t n = x->n;
    const int p = x->p;
    const size_t tab_bytes = sizeof(double) * (size_t)ncol * (p + 1);
    if (ctx_reserve(c, tab_bytes)) return OEMGPU_ERR_HIP;
    double *tab = (double *)c->ws;
    OEM_HIP(hipMemcpyAsync(tab, coef, tab_bytes, hipMemcpyHostToDevice, s));
    // rows per workgroup: a multiple of 256 (four row blocks), about four workgroups per CU
    const bool tlds = tab_bytes <= PR_LDS_MAX;
    const int groups = (ncol + 7) / 8, wpr = groups >= 4 ? 4 : groups >= 2 ? 2 : 1;
    const int64_t want = 4 * (int64_t)c->num_cu;
    const int64_t ch = std::max<int64_t>(256, ((n + want - 1) / want + 255) / 256 * 256), nchunk = (n + ch - 1) / ch;
    if (tlds) {
        if (lds_limit_once(reinterpret_cast<const void *>(&predict_csr_kernel<true>), tab_bytes)) return OEMGPU_ERR_HIP;
        hipLaunchKernelGGL(predict_csr_kernel<true>, dim3((unsigned)nchunk), dim3(256), tab_bytes, s, x->rowptr, x->ccol, x->cval, n, p, tab, ncol, type,
                           wpr, ch, out_dev);
    } else {
        hipLaunchKernelGGL(predict_csr_kernel<false>, dim3((unsigned)nchunk), dim3(256), 0, s, x->rowptr, x->ccol, x->cval, n, p, tab, ncol, type, wpr,
                           ch, out_dev);
    }
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipStreamSynchronize(s));                                           // the caller's table may go once this returns
    return 0;
}

int oemgpu_selftest_predict_plan(int64_t n, int32_t p, int32_t ncol, int32_t layout, int32_t num_cu, int64_t *out)
{
    if (n < 1 || p < 1 || p > INT32_MAX - 8 || ncol < 1 || ncol > INT32_MAX - 16 || num_cu < 1 || !out) { set_error("selftest_predict_plan: bad argument"); return OEMGPU_ERR_ARG; }
    if (layout != -1 && layout != OEMGPU_F64 && layout != OEMGPU_F32) { set_error("selftest_predict_plan: layout is -1, OEMGPU_F64 or OEMGPU_F32"); return OEMGPU_ERR_ARG; }
    const PredictPlan P = predict_plan(n, p, ncol, num_cu);                     // (one shape for the three layouts: they differ in the loads only)
    out[0] = P.rpw; out[1] = P.nwg; out[2] = P.lt; out[3] = P.passes; out[4] = P.chunk; out[5] = P.krows; out[6] = (int64_t)P.lds; out[7] = P.nchunks;
    return 0;
}

#pragma GCC visibility pop
}
