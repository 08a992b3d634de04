// logistic_multi.hip -- many binomial responses on one dense x: the row pass of ONE IRLS step for a block of responses.
//
// For every response r of a block the pass forms eta_r = X (beta_r o s) + beta_r0, prob, r = y_r - prob and the loss terms, and from
// them g_r = [sum r, X'r, sum loss] -- logit_rows_kernel's mode 1 (logistic.hip), the 1e-5 loss clamps included, for 16 LT responses
// from one read of the rows.  There is no W floor here: the floor (row == irls_i && W < 1e-5) only feeds the Hessian's Z, and this
// pass never builds a Hessian.  Mode 0 is the same kernel without the link: r = y, for X'Y and lambda_0.
//
// Both products run on v_mfma_f64_16x16x4_f64 (A: lane (l16, g) holds row l16 of a 16 x 4 tile, k slot g; B: lane (l16, g) column l16,
// k slot g; register rr of lane (g, l16) of the accumulator is (row 4 rr + g, column l16)):
//   eta tile  = X[16 rows, 4 columns] . Bt[4 columns, 16 responses]     register rr: (row 4 rr + g, response l16)
//   X'r tile  = X'[16 columns, 4 rows] . R[4 rows, 16 responses]        register rr: (column 4 rr + g, response l16)
// The X'r accumulators of all p columns do not fit one wave (4 LT doubles per 16 columns: 256 LT at p = 1024), so the COLUMNS are
// split over the four waves of a workgroup -- wave w owns the 16-column tiles w, w + 4, ... (TPW of them: 2, 4, 8 or 16 by p) -- and
// each wave keeps, for the whole chunk of rows, its slice of Bt (4 TPW LT doubles, the B operands of the eta product, loaded once)
// and its X'r accumulators (4 TPW LT doubles) in registers.  A sub-block of 16 RT rows (RT LT = 4; RT = 2 at TPW = 16) then goes through three steps:
//   A  every wave multiplies its columns of the sub-block into a partial eta (RT x LT tiles) and writes it to LDS;
//   L  the 256 threads add the four partials in wave order, ((w0 + w1) + (w2 + w3)) + beta_0, apply the link to 4 elements each,
//      and write r to LDS as [row][response]: k-step (rt, rr) of the second product reads rows 4 rr .. 4 rr + 3 of it at slots g, which
//      is the accumulator layout of the first product -- the exchange moves no element to another slot, only to the other waves;
//   B  every wave multiplies its columns of the sub-block with r.
// x is read where it lies in all three layouts of a DenseSrc (float32 widened in the register) and read TWICE, once per product: the
// two products want a 16 x 16 tile of x in transposed operand layouts, and the second read of a sub-block (16 RT rows x p: 8 to
// 512 KiB) comes from the caches rather than from a staged copy (DESIGN.md 3.20 has the reason).  All layouts hand the MFMAs the same
// operand values in the same order: the same bytes.
//
// Padding is made by SELECTION, never by a predicated load: a lane without a row, column or response loads a clamped element that
// exists -- the chunk's last row, column p - 1, response m - 1 -- and takes 0.  Nothing in the padding of x or Y and nothing past
// their last element is read.  No atomics: every workgroup writes its whole (chunk, block) panel, logit_multi_reduce_kernel adds the
// panels in chunk order and writes g_r for the LIVE responses only (a frozen response keeps the g, and the loss, of its last own
// pass); a block whose responses are all frozen returns before it reads a byte of x.
//
// What a response's sums are does not depend on the block it sits in, on LT or on the number of responses: rows per chunk come from
// n and the CU count alone, the column split from p alone, and the per-thread sums of r and of the loss terms run over the rows
// = rsub (mod 16) of the chunk in row order whatever RT is.
//
// The bound: 8 n (p blocks + m) bytes -- x once per response block if the second read hits, Y once -- against
// 4 n (p + 1) m flops.
#include "logistic_multi.hpp"
#include "common.hpp"

#include <cmath>

namespace oemgpu {
namespace {

struct LmCm {                                // column-major float64, column stride ld
    const double *x;
    int64_t ld;
    __device__ __forceinline__ double at(int64_t row, int col) const { return x[(int64_t)col * ld + row]; }
};
template <typename T>
struct LmRm {                                // row-major float64 / float32, row stride ldr
    const T *x;
    int64_t ldr;
    __device__ __forceinline__ double at(int64_t row, int col) const { return (double)x[row * ldr + col]; }
};

// grid: (row chunks, response blocks)
// MASKED (the fold instances of a cross-validation): column t of the pass is response F.ycol[t] of Y (t itself without
// F.ycol) on the rows with F.foldid[row] != F.leave[t].  The mask is one more term of step L's selection -- a left-out row takes r = 0
// and adds nothing to the sums of r and of the loss -- and the two products are what they were: such a row adds x . 0 to the X'r chain,
// which is why a column with leave = 0, or with an id no row carries, has the bytes of the unmasked pass, and why a column's bytes do
// not depend on its companions' leave.  The columns of a block share their A operand: a row that one column leaves out is still loaded
// for the others, so x must be finite on every row of the call (a NaN in a left-out row reaches X'r as NaN . 0).  The unmasked
// instantiations are the code they were before MASKED existed.
template <int TPW, int LT, class SRC, bool MASKED>
__global__ __launch_bounds__(64 * LMULTI_NW) void logit_multi_rows_kernel(const SRC X, const double *__restrict__ y, int64_t rs, int64_t cs, int64_t n,
                                                                          int p, int m, const double *__restrict__ bt, int intercept, int mode,
                                                                          const int *__restrict__ live, int64_t rows, int npass,
                                                                          double *__restrict__ part, const LogitMultiFold F)
{
    constexpr int RT = TPW == 16 ? 2 : 4 / LT, MB = 16 * LT, SB = 16 * RT;     // SB MB <= 1024; 32 rows at TPW = 16, whose Bt and X'r fill the registers
    __shared__ double lds[5 * 1024];
    double *etap = lds;                                                       // [wave][row of the sub-block][response]: 4 x 1024
    double *rsh = lds + 4096;                                                 // [row of the sub-block][response]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l16 = lane & 15, g = lane >> 4;
    const int64_t chunk = blockIdx.x;
    const int blk = blockIdx.y, rbase = blk * MB;
    {
        const int r = rbase + tid;
        if (!__syncthreads_or(tid < MB && r < m && live[r] != 0)) return;      // every response of the block is frozen
    }
    const int q = p + (intercept ? 1 : 0), o = intercept ? 1 : 0;
    const int64_t r_lo = chunk * rows, r_end = r_lo + rows < n ? r_lo + rows : n, r_last = r_end - 1;
    // this wave's slice of Bt, in the B operand layout of the eta product: tile j, k-step s, response tile t
    double bb[TPW][4][LT];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < LT; ++t) bb[j][s][t] = 0.0;
    if (mode) {
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int col = 16 * (w + LMULTI_NW * j) + 4 * s + g, colc = col < p ? col : p - 1;
#pragma unroll
                for (int t = 0; t < LT; ++t) {
                    const int r = rbase + 16 * t + l16, rc = r < m ? r : m - 1;
                    const double v = bt[(size_t)rc * q + o + colc];
                    bb[j][s][t] = (col < p && r < m) ? v : 0.0;
                }
            }
        }
    }
    // the link's threads: response l16 of every tile, rows rsub (mod 16) of the chunk
    const int rsub = tid >> 4, ll = tid & 15;
    double b0[LT], rsum[LT], lsum[LT];
    int64_t yoff[LT];
    bool yok[LT];
    int lv[LT];                                                               // MASKED: the fold this column leaves out
#pragma unroll
    for (int t = 0; t < LT; ++t) {
        const int r = rbase + 16 * t + ll, rc = r < m ? r : m - 1;
        yok[t] = r < m;
        yoff[t] = (int64_t)((MASKED && F.ycol) ? F.ycol[rc] : rc) * cs;
        lv[t] = MASKED ? F.leave[rc] : 0;
        b0[t] = (mode && intercept) ? bt[(size_t)rc * q] : 0.0;
        rsum[t] = 0.0; lsum[t] = 0.0;
    }
    v4d xacc[TPW][LT];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int t = 0; t < LT; ++t) xacc[j][t] = v4d{0.0, 0.0, 0.0, 0.0};

    for (int64_t sb0 = r_lo; sb0 < r_end; sb0 += SB) {
        // (p as the loop sees it: hipcc otherwise keeps the clamped 64-bit offset of every (tile, k-step) of the wave alive across the
        // loop -- 2 VGPRs each, 160 at TPW = 16 -- where recomputing one costs two VALU instructions next to an 8-pass MFMA)
        int pv = p;
        asm volatile("" : "+s"(pv));
        // ---- A: partial eta of this wave's columns
        if (mode) {
            v4d eacc[RT][LT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int t = 0; t < LT; ++t) eacc[rt][t] = v4d{0.0, 0.0, 0.0, 0.0};
            int64_t rowc[RT];
            bool rok[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const int64_t row = sb0 + 16 * rt + l16;
                rok[rt] = row < r_end;
                rowc[rt] = rok[rt] ? row : r_last;
            }
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                const int c0 = 16 * (w + LMULTI_NW * j);
                if (c0 >= pv) continue;                                        // (wave-uniform: no column of x in this tile)
                double a[4][RT];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int col = c0 + 4 * s + g, colc = col < pv ? col : pv - 1;
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) a[s][rt] = X.at(rowc[rt], colc);
                }
                // (the values count as used here, whatever is selected below: hipcc otherwise sinks each load under the branch of its
                // selection and waits for it there -- multi.hip)
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) asm volatile("" : "+v"(a[s][rt]));
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const bool cok = c0 + 4 * s + g < pv;
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const double av = (cok && rok[rt]) ? a[s][rt] : 0.0;
#pragma unroll
                        for (int t = 0; t < LT; ++t) eacc[rt][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bb[j][s][t], eacc[rt][t], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);                            // (one tile's loads in flight, not all TPW: the registers are Bt's and X'r's)
            }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int t = 0; t < LT; ++t)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) etap[(w * SB + 16 * rt + 4 * rr + g) * MB + 16 * t + l16] = eacc[rt][t][rr];
        }
        __syncthreads();
        // ---- L: eta, the link, r and the loss terms; 4 elements per thread
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int rl = 16 * rt + rsub;
            const int64_t row = sb0 + rl;
            const bool ok = row < r_end;
            const int64_t rc = ok ? row : r_last;
            const int fid = MASKED ? F.foldid[rc] : 0;
#pragma unroll
            for (int t = 0; t < LT; ++t) {
                const double yi = y[rc * rs + yoff[t]];
                const int e = rl * MB + 16 * t + ll;
                double r = yi, lt = 0.0;
                if (mode) {
                    const double eta = ((etap[e] + etap[SB * MB + e]) + (etap[2 * SB * MB + e] + etap[3 * SB * MB + e])) + b0[t];
                    const double prob = 1.0 / (1.0 + exp(-eta));
                    r = yi - prob;
                    if (yi == 1.0) lt = prob > 1e-5 ? log(1.0 / prob) : log(1.0 / 1e-5);
                    else lt = prob <= 1.0 - 1e-5 ? log(1.0 / (1.0 - prob)) : log(1.0 / 1e-5);
                }
                const bool use = MASKED ? (ok && yok[t] && fid != lv[t]) : (ok && yok[t]);
                r = use ? r : 0.0;
                rsum[t] += r;
                lsum[t] += use ? lt : 0.0;
                rsh[e] = r;
            }
        }
        __syncthreads();
        // ---- B: X'r of this wave's columns; k-step (rt, rr) takes rows 4 rr .. 4 rr + 3 of row tile rt at slots g
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            const int c0 = 16 * (w + LMULTI_NW * j);
            if (c0 >= pv) continue;
            const int col = c0 + l16, colc = col < pv ? col : pv - 1;
            double a[RT][4];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int64_t row = sb0 + 16 * rt + 4 * rr + g;
                    a[rt][rr] = X.at(row < r_end ? row : r_last, colc);
                }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) asm volatile("" : "+v"(a[rt][rr]));
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int64_t row = sb0 + 16 * rt + 4 * rr + g;
                    const double av = (row < r_end && col < pv) ? a[rt][rr] : 0.0;
#pragma unroll
                    for (int t = 0; t < LT; ++t)
                        xacc[j][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, rsh[(16 * rt + 4 * rr + g) * MB + 16 * t + l16], xacc[j][t], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // ---- the panel
    double *panel = part + ((size_t)chunk * npass + blk) * (size_t)(p + 2) * MB;
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int c = 16 * (w + LMULTI_NW * j) + 4 * rr + g;
            if (c >= p) continue;
#pragma unroll
            for (int t = 0; t < LT; ++t) panel[(size_t)(1 + c) * MB + 16 * t + l16] = xacc[j][t][rr];
        }
    // sum r and the loss: the 16 row classes of a response in class order (etap is free: its last readers are behind a barrier)
    double *red = lds;                                                        // [2][16][MB]
#pragma unroll
    for (int t = 0; t < LT; ++t) {
        red[rsub * MB + 16 * t + ll] = rsum[t];
        red[(16 + rsub) * MB + 16 * t + ll] = lsum[t];
    }
    __syncthreads();
    if (tid < MB) {
        double a = 0.0, b = 0.0;
        for (int i = 0; i < 16; ++i) { a += red[i * MB + tid]; b += red[(16 + i) * MB + tid]; }
        panel[tid] = a;
        panel[(size_t)(p + 1) * MB + tid] = b;
    }
}

// grid: (ceil((p + 2) / 256), responses)
__global__ __launch_bounds__(256) void logit_multi_reduce_kernel(const double *__restrict__ part, int64_t nchunk, int npass, int p, int mb,
                                                                 const int *__restrict__ live, double *__restrict__ g)
{
    const int r = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= p + 2 || !live[r]) return;
    const int blk = r / mb, within = r - blk * mb;
    const double *src = part + ((size_t)blk * (p + 2) + j) * mb + within;
    const size_t stride = (size_t)npass * (p + 2) * mb;
    double v = src[0];
    for (int64_t c = 1; c < nchunk; ++c) v += src[(size_t)c * stride];        // in chunk order
    g[(size_t)r * (p + 2) + j] = v;
}

template <int TPW, int LT, class SRC>
int rows_launch(hipStream_t s, const LogitMultiPlan &pl, const SRC &X, const MultiY &Y, const double *bt, int intercept, int mode, const int *live,
                double *part, const LogitMultiFold *fold)
{
    const dim3 grid((unsigned)pl.nchunk, (unsigned)pl.npass), wg(64 * LMULTI_NW);
    if (fold)
        hipLaunchKernelGGL((logit_multi_rows_kernel<TPW, LT, SRC, true>), grid, wg, 0, s, X, Y.y, Y.rs, Y.cs, pl.n, pl.p, pl.mc, bt, intercept, mode, live,
                           pl.rows, pl.npass, part, *fold);
    else
        hipLaunchKernelGGL((logit_multi_rows_kernel<TPW, LT, SRC, false>), grid, wg, 0, s, X, Y.y, Y.rs, Y.cs, pl.n, pl.p, pl.mc, bt, intercept, mode, live,
                           pl.rows, pl.npass, part, LogitMultiFold{});
    OEM_HIP(hipGetLastError());
    return 0;
}

template <class SRC>
int rows_src(hipStream_t s, const LogitMultiPlan &pl, const SRC &X, const MultiY &Y, const double *bt, int intercept, int mode, const int *live, double *part,
             const LogitMultiFold *fold)
{
    switch (pl.tpw * 8 + pl.lt) {
    case 2 * 8 + 1: return rows_launch<2, 1>(s, pl, X, Y, bt, intercept, mode, live, part, fold);
    case 2 * 8 + 4: return rows_launch<2, 4>(s, pl, X, Y, bt, intercept, mode, live, part, fold);
    case 4 * 8 + 1: return rows_launch<4, 1>(s, pl, X, Y, bt, intercept, mode, live, part, fold);
    case 4 * 8 + 4: return rows_launch<4, 4>(s, pl, X, Y, bt, intercept, mode, live, part, fold);
    case 8 * 8 + 1: return rows_launch<8, 1>(s, pl, X, Y, bt, intercept, mode, live, part, fold);
    case 8 * 8 + 2: return rows_launch<8, 2>(s, pl, X, Y, bt, intercept, mode, live, part, fold);
    case 16 * 8 + 1: return rows_launch<16, 1>(s, pl, X, Y, bt, intercept, mode, live, part, fold);
    default: set_error("internal: logistic multi plan with %d column tiles per wave and %d response tiles", pl.tpw, pl.lt); return OEMGPU_ERR_INTERNAL;
    }
}

}  // namespace

LogitMultiPlan logit_multi_plan(int64_t n, int p, int mc, int num_cu)
{
    LogitMultiPlan pl;
    pl.n = n; pl.p = p; pl.mc = mc;
    pl.tpw = p <= 128 ? 2 : (p <= 256 ? 4 : (p <= 512 ? 8 : 16));
    pl.band = 16 * LMULTI_NW * pl.tpw;
    // 4 tpw lt doubles of Bt and as many of X'r accumulators per lane: tpw lt <= 16 keeps both within 128 doubles
    pl.lt = mc <= 16 ? 1 : (16 / pl.tpw < 4 ? 16 / pl.tpw : 4);
    pl.mb = 16 * pl.lt;
    pl.npass = (mc + pl.mb - 1) / pl.mb;
    // two workgroups of four waves per CU and response block; n and the CU count alone decide the chunk
    int64_t rows = ((n + 2 * (int64_t)num_cu - 1) / (2 * (int64_t)num_cu) + 63) / 64 * 64;
    if (rows < 64) rows = 64;
    pl.rows = rows;
    pl.nchunk = (n + rows - 1) / rows;
    pl.lds_bytes = 8 * 5 * 1024;
    pl.part_doubles = (size_t)pl.nchunk * pl.npass * (size_t)(p + 2) * pl.mb;
    return pl;
}

int launch_logit_multi_rows(hipStream_t s, const LogitMultiPlan &pl, const DenseSrc &X, const MultiY &Y, const double *bt, int intercept, int mode,
                            const int *live, double *part, const LogitMultiFold *fold)
{
    if (pl.nchunk > 0x7fffffffLL || pl.npass > 65535) { set_error("logistic_multi: the row pass has more workgroups than a launch takes"); return OEMGPU_ERR_UNSUPPORTED; }
    if (X.colmajor()) return rows_src(s, pl, LmCm{X.cm(), X.ld}, Y, bt, intercept, mode, live, part, fold);
    if (X.dtype == OEMGPU_F32) return rows_src(s, pl, LmRm<float>{(const float *)X.x, X.ld}, Y, bt, intercept, mode, live, part, fold);
    return rows_src(s, pl, LmRm<double>{(const double *)X.x, X.ld}, Y, bt, intercept, mode, live, part, fold);
}

int launch_logit_multi_reduce(hipStream_t s, const LogitMultiPlan &pl, const double *part, const int *live, double *g)
{
    hipLaunchKernelGGL(logit_multi_reduce_kernel, dim3((unsigned)((pl.p + 2 + 255) / 256), (unsigned)pl.mc), dim3(256), 0, s, part, pl.nchunk, pl.npass, pl.p,
                       pl.mb, live, g);
    OEM_HIP(hipGetLastError());
    return 0;
}

}  // namespace oemgpu
