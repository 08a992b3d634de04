// multi.hip -- many responses on one dense x: the X'Y pass of oemgpu_fit_dense_multi_dev / _rm_dev (api.hip: fit_dense_multi_src).
//
// A moment buffer (oemgpu.h) separates into what depends on x alone -- the Gram block, the column sums, the row count: ONE moment pass,
// whatever the number of responses -- and three kinds of entry per response r: sum_i x_ij y_ir, sum_i y_ir^2 and sum_i y_ir.  This pass
// forms them for all m responses as the product [X | 1]' Y on v_mfma_f64_16x16x4_f64: the A operand is 16 columns of [X | 1] by 4 rows
// (lane (l16, g) holds column l16 of the tile, k slot g), the B operand the same 4 rows by 16 responses (lane (l16, g): response l16,
// k slot g), register r of lane (g, l16) of the accumulator is (column 4 r + g, response l16).  The column of ones rides as
// pseudo-column p and yields sum y; sum y^2 is a chain of FP64 FMAs over the B values of one wave, added over the four k slots in slot
// order at the end.
//
// Rows are cut into chunks of MultiPlan::rows rows (host plan: a multiple of 64), responses into blocks of 16 LT (LT = 1, 2, 4
// accumulator tiles per column tile), the columns of [X | 1] into groups of 128: a workgroup of four waves takes one (chunk, group,
// block), each wave two 16-column tiles of the group against the block's LT response tiles.  Within a block of 64 rows, k-step s
// (0 .. 15) puts row 16 g + s into slot g: a lane then walks 16 CONSECUTIVE rows, so a column-major x is read 128 contiguous bytes per lane
// and column (every cache line used whole) and a row-major x 16 neighbouring columns of four rows per load; Y alike in either of its
// layouts.  A lane loads one element at a time straight into operand layout, so x and Y need their element's alignment only, and
// float32 is widened in the register it was loaded into.  All three layouts of x hand the MFMAs the same operand values in the same
// order: the same bits.  Padding is made by SELECTION: a lane whose row (>= n), column (> p) or response (>= m) does not exist loads an
// element that does -- the last row, column p - 1, response m - 1 -- and takes 0 (1 for the pseudo-column of a row that exists) instead;
// nothing in the padding of x or Y and nothing behind their last element is ever read.
//
// Every workgroup writes its part of the chunk's (p + 2) x 16 LT panel (no atomics; every entry that is read is written once);
// multi_compose_kernel adds the panels in chunk order -- one fixed order for every sum, two calls return the same bytes -- into the
// y entries (and their mirror images) of copies of the one moment buffer, one solve chunk of responses at a time.
//
// The bound: 8 n (p passes + m) bytes -- x once per response block, Y once -- and 2 n (p + 2) m flops.
#include "multi.hpp"
#include "common.hpp"

namespace oemgpu {
namespace {

struct MultiCm {                             // column-major float64, column stride ld
    const double *x;
    int64_t ld;
    __device__ __forceinline__ double at(int64_t row, int col) const { return x[(int64_t)col * ld + row]; }
};
template <typename T>
struct MultiRm {                             // row-major float64 / float32, row stride ldr
    const T *x;
    int64_t ldr;
    __device__ __forceinline__ double at(int64_t row, int col) const { return (double)x[row * ldr + col]; }
};

// FOLD (xval_oem_multi: X is the fold-ordered copy xp, y the fold-ordered Yp): the row chunks are those of the fold segments, fold k
// owning chunks [cfirst[k], cfirst[k + 1]) of `rows` rows from fold_start[k] on -- none straddles a fold, none is empty (the host cuts
// them from the fold sizes; an empty fold owns none), a segment may start on any row and have any length.  A lane without a row clamps
// to the chunk's last row, so the padding rows between the segments (the gathers never write them) are never read.
template <bool FOLD> struct MultiFolds {};
template <> struct MultiFolds<true> { const int64_t *fold_start, *fold_n; const int *cfirst; int K; };

// grid: (row chunks, column groups, response blocks)
template <int LT, class SRC, bool FOLD = false>
__global__ __launch_bounds__(64 * MULTI_NW) void multi_xty_kernel(const SRC X, const double *__restrict__ y, int64_t rs, int64_t cs, int64_t n,
                                                                  int p, int m, int64_t rows, int npass, double *__restrict__ part,
                                                                  MultiFolds<FOLD> F)
{
    constexpr int KC = LT >= 4 ? 4 : 8, MB = 16 * LT, CPW = MULTI_CPW;       // k-steps a lane has in flight at once
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l16 = lane & 15, g = lane >> 4;
    const int64_t chunk = blockIdx.x;
    const int cg = blockIdx.y, blk = blockIdx.z;
    const int c0 = (cg * MULTI_NW + w) * CPW * 16;                           // this wave's first column of [X | 1]
    if (c0 > p) return;                                                       // (wave-uniform: nothing of [X | 1] here; wave 0 of group 0 always stays)
    const bool do_sq = cg == 0 && w == 0;
    int64_t r_lo = chunk * rows, r_end = r_lo + rows < n ? r_lo + rows : n, r_last = n - 1;
    if constexpr (FOLD) {
        int k = 0;
        while (F.cfirst[k + 1] <= chunk) ++k;                                // (cfirst[K] = the number of chunks > chunk: k < K)
        const int64_t seg_end = F.fold_start[k] + F.fold_n[k];
        r_lo = F.fold_start[k] + (chunk - F.cfirst[k]) * rows;
        r_end = r_lo + rows < seg_end ? r_lo + rows : seg_end;
        r_last = r_end - 1;
    }
    // Loads are never predicated: a lane whose element does not exist loads a clamped one that does (never padding) and SELECTS 0
    // instead, so every load of a batch of k-steps is in flight before the first MFMA waits (a load under a branch is waited for at the
    // branch's end, one load after the other: 3 to 4 times the kernel's time)
    int col[CPW], colc[CPW];
#pragma unroll
    for (int ct = 0; ct < CPW; ++ct) { col[ct] = c0 + 16 * ct + l16; colc[ct] = col[ct] < p ? col[ct] : p - 1; }
    int64_t yoff[LT];
    bool yok[LT];
#pragma unroll
    for (int t = 0; t < LT; ++t) {
        const int r = blk * MB + 16 * t + l16;
        yok[t] = r < m;
        yoff[t] = (int64_t)(yok[t] ? r : m - 1) * cs;
    }
    v4d acc[CPW][LT];
    double sq[LT];
#pragma unroll
    for (int t = 0; t < LT; ++t) {
        sq[t] = 0.0;
#pragma unroll
        for (int ct = 0; ct < CPW; ++ct) acc[ct][t] = v4d{0.0, 0.0, 0.0, 0.0};
    }
    for (int64_t rb = r_lo; rb < r_end; rb += MULTI_ROWS) {
#pragma unroll 1
        for (int s0 = 0; s0 < 16; s0 += KC) {
            double a[CPW][KC], b[LT][KC];
            bool rok[KC];
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const int64_t row = rb + 16 * g + s0 + k;
                rok[k] = row < r_end;
                const int64_t rowc = rok[k] ? row : r_last;
#pragma unroll
                for (int ct = 0; ct < CPW; ++ct) a[ct][k] = X.at(rowc, colc[ct]);
#pragma unroll
                for (int t = 0; t < LT; ++t) b[t][k] = y[rowc * rs + yoff[t]];
            }
            // (the values count as used here, whatever is selected below: hipcc otherwise sinks each load under the branch of its
            // selection and waits for it there)
#pragma unroll
            for (int k = 0; k < KC; ++k) {
#pragma unroll
                for (int ct = 0; ct < CPW; ++ct) asm volatile("" : "+v"(a[ct][k]));
#pragma unroll
                for (int t = 0; t < LT; ++t) asm volatile("" : "+v"(b[t][k]));
            }
#pragma unroll
            for (int k = 0; k < KC; ++k) {
#pragma unroll
                for (int ct = 0; ct < CPW; ++ct)                             // an element; the column of ones; padding
                    a[ct][k] = (rok[k] && col[ct] < p) ? a[ct][k] : ((rok[k] && col[ct] == p) ? 1.0 : 0.0);
#pragma unroll
                for (int t = 0; t < LT; ++t) b[t][k] = (rok[k] && yok[t]) ? b[t][k] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < KC; ++k) {
#pragma unroll
                for (int ct = 0; ct < CPW; ++ct)
#pragma unroll
                    for (int t = 0; t < LT; ++t) acc[ct][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ct][k], b[t][k], acc[ct][t], 0, 0, 0);
                if (do_sq) {
#pragma unroll
                    for (int t = 0; t < LT; ++t) sq[t] = fma(b[t][k], b[t][k], sq[t]);
                }
            }
        }
    }
    const int q = p + 2;
    double *panel = part + ((size_t)chunk * npass + blk) * (size_t)q * MB;
#pragma unroll
    for (int ct = 0; ct < CPW; ++ct)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int c = c0 + 16 * ct + 4 * rr + g;
            if (c > p) continue;
            const int prow = c < p ? c : p + 1;                              // x column c; the ones: sum y
#pragma unroll
            for (int t = 0; t < LT; ++t) panel[(size_t)prow * MB + 16 * t + l16] = acc[ct][t][rr];
        }
    if (do_sq) {
#pragma unroll
        for (int t = 0; t < LT; ++t) {
            const double v0 = __shfl(sq[t], l16, 64), v1 = __shfl(sq[t], l16 + 16, 64), v2 = __shfl(sq[t], l16 + 32, 64), v3 = __shfl(sq[t], l16 + 48, 64);
            if (g == 0) panel[(size_t)p * MB + 16 * t + l16] = ((v0 + v1) + v2) + v3;
        }
    }
}

// grid: (ceil((p + 2)^2 / 256), responses of the solve chunk)
__global__ __launch_bounds__(256) void multi_compose_kernel(const double *__restrict__ base, const double *__restrict__ part, int p, int mb, int npass,
                                                            int64_t nchunk, int r0, double *__restrict__ out)
{
    const int q = p + 2;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, len = (size_t)q * q;
    if (e >= len) return;
    const int i = (int)(e % q), j = (int)(e / q), lo = i < j ? i : j, hi = i < j ? j : i;
    int yrow = -1;                                                           // the panel row this entry comes from, if it is a y entry
    if (hi == p) yrow = lo;                                                  // M[p, j] and its mirror image; lo == p: sum y^2
    else if (hi == p + 1 && lo == p) yrow = p + 1;                           // sum y
    double v;
    if (yrow < 0) v = base[e];
    else {
        const int r = r0 + blockIdx.y, blk = r / mb, within = r - blk * mb;
        const double *src = part + ((size_t)blk * q + yrow) * mb + within;
        const size_t stride = (size_t)npass * q * mb;
        v = src[0];
        for (int64_t c = 1; c < nchunk; ++c) v += src[(size_t)c * stride];   // in chunk order
    }
    out[(size_t)blockIdx.y * len + e] = v;
}

// xval_oem_multi.  grid: (ceil((p + 2)^2 / 256), instances).  Instance r * (K + 1) + ff of the solve chunk (r0 its first response):
// "all folds" (ff = 0) or "all but fold ff" of response r0 + r -- the sum over the folds in ascending order, as xval.hip's
// fold_sum_kernel takes it, of fold k's moment buffer mfold[k] with the y entries of the response composed in: fold k's chunk
// partials added in chunk order first.  single: instance r * K + k is fold k's buffer alone (the selftest entry).  The x entries are
// read from the valid (lower) triangle and written to both.
__global__ __launch_bounds__(256) void multi_fold_compose_kernel(const double *__restrict__ mfold, const double *__restrict__ part, int p, int mb,
                                                                 int npass, const int *__restrict__ cfirst, int K, int r0, int single,
                                                                 double *__restrict__ out)
{
    const int q = p + 2;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, len = (size_t)q * q;
    if (e >= len) return;
    const int i = (int)(e % q), j = (int)(e / q), lo = i < j ? i : j, hi = i < j ? j : i;
    int yrow = -1;
    if (hi == p) yrow = lo;
    else if (hi == p + 1 && lo == p) yrow = p + 1;
    const int per = single ? K : K + 1, rl = blockIdx.y / per, ff = blockIdx.y - rl * per;
    const int r = r0 + rl, blk = r / mb, within = r - blk * mb;
    const double *src = part + ((size_t)blk * q + (yrow < 0 ? 0 : yrow)) * mb + within;
    const size_t stride = (size_t)npass * q * mb, elo = (size_t)lo * q + hi;
    double s = 0.0;
    for (int k = 0; k < K; ++k) {
        if (single ? k != ff : k + 1 == ff) continue;
        double v;
        if (yrow < 0) v = mfold[(size_t)k * len + elo];
        else {
            v = 0.0;
            for (int c = cfirst[k]; c < cfirst[k + 1]; ++c) v = c == cfirst[k] ? src[(size_t)c * stride] : v + src[(size_t)c * stride];
        }
        s += v;
    }
    out[(size_t)blockIdx.y * len + e] = s;
}

__global__ __launch_bounds__(256) void multi_column_kernel(const double *__restrict__ y, int64_t rs, int64_t cs, int64_t n, int r, double *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = y[i * rs + (int64_t)r * cs];
}

template <class SRC>
int launch_xty_src(hipStream_t s, const MultiPlan &pl, const SRC &X, const MultiY &Y, double *part)
{
    const dim3 grid((unsigned)pl.nchunk, (unsigned)pl.cgroups, (unsigned)pl.npass), block(64 * MULTI_NW);
    switch (pl.lt) {
    case 1: hipLaunchKernelGGL((multi_xty_kernel<1, SRC>), grid, block, 0, s, X, Y.y, Y.rs, Y.cs, pl.n, pl.p, pl.m, pl.rows, pl.npass, part, MultiFolds<false>{}); break;
    case 2: hipLaunchKernelGGL((multi_xty_kernel<2, SRC>), grid, block, 0, s, X, Y.y, Y.rs, Y.cs, pl.n, pl.p, pl.m, pl.rows, pl.npass, part, MultiFolds<false>{}); break;
    case 4: hipLaunchKernelGGL((multi_xty_kernel<4, SRC>), grid, block, 0, s, X, Y.y, Y.rs, Y.cs, pl.n, pl.p, pl.m, pl.rows, pl.npass, part, MultiFolds<false>{}); break;
    default: set_error("internal: multi plan with %d response tiles", pl.lt); return OEMGPU_ERR_INTERNAL;
    }
    OEM_HIP(hipGetLastError());
    return 0;
}

template <int LT>
int launch_fold_xty_lt(hipStream_t s, const MultiPlan &pl, int nchunk, const double *xp, int64_t ldp, const double *Yp, const MultiFolds<true> &F, double *part)
{
    const dim3 grid((unsigned)nchunk, (unsigned)pl.cgroups, (unsigned)pl.npass), block(64 * MULTI_NW);
    hipLaunchKernelGGL((multi_xty_kernel<LT, MultiCm, true>), grid, block, 0, s, MultiCm{xp, ldp}, Yp, (int64_t)1, ldp, ldp, pl.p, pl.m, pl.rows,
                       pl.npass, part, F);
    OEM_HIP(hipGetLastError());
    return 0;
}

}  // namespace

int launch_multi_fold_xty(hipStream_t s, const MultiPlan &pl, int K, int nchunk, const double *xp, int64_t ldp, const double *Yp,
                          const int64_t *fold_start, const int64_t *fold_n, const int *cfirst, double *part)
{
    if (nchunk < 1) return 0;                                                // (no row in any fold: nothing to add)
    if (pl.cgroups > 65535 || pl.npass > 65535) { set_error("xval_multi: the X'Y pass has more workgroups than a launch takes"); return OEMGPU_ERR_UNSUPPORTED; }
    const MultiFolds<true> F{fold_start, fold_n, cfirst, K};
    switch (pl.lt) {
    case 1: return launch_fold_xty_lt<1>(s, pl, nchunk, xp, ldp, Yp, F, part);
    case 2: return launch_fold_xty_lt<2>(s, pl, nchunk, xp, ldp, Yp, F, part);
    case 4: return launch_fold_xty_lt<4>(s, pl, nchunk, xp, ldp, Yp, F, part);
    default: set_error("internal: multi plan with %d response tiles", pl.lt); return OEMGPU_ERR_INTERNAL;
    }
}

int launch_multi_fold_compose(hipStream_t s, const MultiPlan &pl, int K, const double *mfold, const double *part, const int *cfirst, int r0, int nb,
                              bool single, double *out)
{
    const size_t len = (size_t)(pl.p + 2) * (pl.p + 2);
    const long long ninst = (long long)nb * (single ? K : K + 1);
    if (ninst > 65535) { set_error("xval_multi: %lld composed buffers are more than a launch takes", ninst); return OEMGPU_ERR_UNSUPPORTED; }
    hipLaunchKernelGGL(multi_fold_compose_kernel, dim3((unsigned)((len + 255) / 256), (unsigned)ninst), dim3(256), 0, s, mfold, part, pl.p, pl.mb,
                       pl.npass, cfirst, K, r0, single ? 1 : 0, out);
    OEM_HIP(hipGetLastError());
    return 0;
}

MultiPlan multi_plan(int64_t n, int p, int m, int num_cu)
{
    MultiPlan pl;
    pl.n = n; pl.p = p; pl.m = m;
    pl.lt = m <= 16 ? 1 : (m <= 32 ? 2 : 4);
    pl.mb = 16 * pl.lt;
    pl.npass = (m + pl.mb - 1) / pl.mb;
    pl.cgroups = (p + 1 + MULTI_NW * MULTI_CPW * 16 - 1) / (MULTI_NW * MULTI_CPW * 16);
    // four workgroups of four waves per CU over all (group, block) pairs; a chunk of at least 256 rows
    int64_t target = (int64_t)4 * num_cu / ((int64_t)pl.npass * pl.cgroups);
    if (target < 1) target = 1;
    int64_t rows = ((n + target - 1) / target + MULTI_ROWS - 1) / MULTI_ROWS * MULTI_ROWS;
    if (rows < 4 * MULTI_ROWS) rows = 4 * MULTI_ROWS;
    pl.rows = rows;
    pl.nchunk = (n + rows - 1) / rows;
    pl.part_doubles = (size_t)pl.nchunk * pl.npass * (size_t)(p + 2) * pl.mb;
    return pl;
}

int launch_multi_xty(hipStream_t s, const MultiPlan &pl, const DenseSrc &X, const MultiY &Y, double *part)
{
    if (pl.nchunk > 0x7fffffffLL || pl.cgroups > 65535 || pl.npass > 65535) { set_error("multi: the X'Y pass has more workgroups than a launch takes"); return OEMGPU_ERR_UNSUPPORTED; }
    if (X.colmajor()) return launch_xty_src(s, pl, MultiCm{X.cm(), X.ld}, Y, part);
    if (X.dtype == OEMGPU_F32) return launch_xty_src(s, pl, MultiRm<float>{(const float *)X.x, X.ld}, Y, part);
    return launch_xty_src(s, pl, MultiRm<double>{(const double *)X.x, X.ld}, Y, part);
}

int launch_multi_compose(hipStream_t s, const MultiPlan &pl, const double *base, const double *part, int r0, int nb, double *out)
{
    const size_t len = (size_t)(pl.p + 2) * (pl.p + 2);
    hipLaunchKernelGGL(multi_compose_kernel, dim3((unsigned)((len + 255) / 256), (unsigned)nb), dim3(256), 0, s, base, part, pl.p, pl.mb, pl.npass,
                       pl.nchunk, r0, out);
    OEM_HIP(hipGetLastError());
    return 0;
}

int launch_multi_column(hipStream_t s, const MultiY &Y, int64_t n, int r, double *out)
{
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(multi_column_kernel, dim3((unsigned)blocks), dim3(256), 0, s, Y.y, Y.rs, Y.cs, n, r, out);
    OEM_HIP(hipGetLastError());
    return 0;
}

}  // namespace oemgpu
