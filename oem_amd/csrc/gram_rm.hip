// gram_rm.hip -- the one-pass moment build of gram.hip for a ROW-major X of float64 or float32 elements, read where it lies.
//
// Replaces, for a caller whose matrix is row-major (every PyTorch tensor that was not transposed on purpose), the two copies that
// stood in front of gram.hip's pass -- the float64 conversion and the transposed copy -- and, like gram.hip, with ONE pass over X:
//   DataStd::standardize   ref src/DataStd.h:203-265   (column means / scales, never materialised)
//   XY = X'Y / n           ref src/oem_dense.h:699-707
//   XtX()                  ref src/oem_dense.h:318-361
//
// Layout: v_mfma_f64_16x16x4_f64 takes A[i][k] from lane i + 16 k and B[k][j] from lane j + 16 k (gram.hip:9-17), so the fragment
// f_T(lane) = z[row r0 + (lane >> 4)][16 T + (lane & 15)] of the augmented matrix Z = [X | y | 1] is the A operand of every tile in
// tile row T and the B operand of every tile in tile column T.  In a row-major matrix the sixteen lanes of one k slot read 128
// (float32: 64) contiguous bytes of one row, so a fragment is ONE element load per lane -- no LDS, no transpose, no alignment beyond
// the element's own (a float32 view on a 4-byte boundary and a float64 row of odd p are read as they are), and float32 elements
// become float64 in the register they were loaded into (v_cvt_f64_f32); every product and sum is FP64.
//
// Work split: the lower triangle of the ntc x ntc tile grid is cut into 4 x 4 tile blocks (64 x 64 columns); a workgroup owns one block
// over one row chunk, its four waves take the 4-row steps of the chunk in turn (wave w: steps w, w + 4, ...), three steps of loads in
// flight per wave and two workgroups on a CU.  Workgroups of the same chunk have neighbouring ids, so the blocks of a chunk run side by side and X comes from
// memory about once however many blocks read it.  The waves' tiles are added as (w0 + w1) + (w2 + w3) through LDS, the chunk partials
// in chunk order by gram_rm_reduce_kernel: one fixed order for every sum, no atomics.
//
// Padding: columns p .. ldr - 1 and rows >= n are never loaded (the address is clamped to the last valid column / row) and the lane's
// value is SELECTED (y, 1 or 0), never multiplied by zero, so NaN next to the data stays out of the result.
#include "common.hpp"
#include "gram_dev.hpp"

namespace oemgpu {

// ------------------------------------------------------------------------------------------------
// provisional shift: shift_sums_kernel (gram.hip) on rows -- the same sampled rows (<= 256 evenly spaced 16-row chunks), the same
// per-thread order and the same tree, so the sums buffer equals that of the column-major float64 copy bit for bit
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void shift_sums_rm_kernel(const T *__restrict__ x, int64_t n, int64_t ldr, int p,
                                                             const double *__restrict__ y, double *__restrict__ sums)
{
    __shared__ double sh[3][256];
    const int j = blockIdx.x;
    const int64_t nch = (n + 15) / 16;
    const int64_t nsamp = nch < 256 ? nch : 256;
    const int k = threadIdx.x;
    double s = 0.0, ss = 0.0, cnt = 0.0;
    if (k < nsamp) {
        const int64_t c = (nsamp > 1) ? ((int64_t)k * (nch - 1)) / (nsamp - 1) : 0;
        const int64_t r0 = c * 16;
        if (r0 + 16 <= n) {
            double v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = (j < p) ? (double)x[(size_t)(r0 + r) * ldr + j] : y[r0 + r];
#pragma unroll
            for (int r = 0; r < 16; ++r) { s += v[r]; ss = fma(v[r], v[r], ss); }
            cnt = 16.0;
        } else {
            for (int64_t r = r0; r < n; ++r) {
                const double v = (j < p) ? (double)x[(size_t)r * ldr + j] : y[r];
                s += v; ss = fma(v, v, ss); cnt += 1.0;
            }
        }
    }
    sh[0][k] = s; sh[1][k] = ss; sh[2][k] = cnt;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (k < w) { sh[0][k] += sh[0][k + w]; sh[1][k] += sh[1][k + w]; sh[2][k] += sh[2][k + w]; }
        __syncthreads();
    }
    if (k == 0) {
        sums[j] = sh[0][0];
        sums[p + 2 + j] = sh[1][0];
        if (j == 0) { sums[p + 1] = sh[2][0]; sums[2 * p + 3] = 0.0; }
    }
}

int launch_shift_sums_rm(hipStream_t s, const void *x, int dtype, int64_t n, int64_t ldr, int p, const double *y, double *sums)
{
    if (dtype == OEMGPU_F32)
        hipLaunchKernelGGL(shift_sums_rm_kernel<float>, dim3(p + 1), dim3(256), 0, s, (const float *)x, n, ldr, p, y, sums);
    else
        hipLaunchKernelGGL(shift_sums_rm_kernel<double>, dim3(p + 1), dim3(256), 0, s, (const double *)x, n, ldr, p, y, sums);
    OEM_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// the plan: pure host arithmetic, the one place the launch shape is decided
// ------------------------------------------------------------------------------------------------
GramRmPlan gram_rm_plan(int64_t n, int p, int num_cu)
{
    GramRmPlan pl;
    pl.p = p;
    pl.ntc = (p + 2 + 15) / 16;
    pl.nb = (pl.ntc + 3) / 4;
    pl.nblk = pl.nb * (pl.nb + 1) / 2;
    // about four workgroups per CU over (chunk, block), and a chunk of no more than GRAM_RM_CHUNK_BYTES of float64 rows: the blocks of a
    // chunk read the same rows side by side, and what the slowest of them has not read yet should still be in the cache; but a chunk
    // no shorter than GRAM_RM_MIN_ROWS rows (a block's partial is 32 KB, its rows at least 64 columns x 8 B x 1024), and no more chunks
    // for the sake of the cache than keep the partials under GRAM_RM_PART_BYTES
    const int64_t target = (4 * (int64_t)num_cu + pl.nblk - 1) / pl.nblk;
    int64_t cap_rows = GRAM_RM_CHUNK_BYTES / (8 * (int64_t)(p + 2));
    if (cap_rows < GRAM_RM_MIN_ROWS) cap_rows = GRAM_RM_MIN_ROWS;
    const int64_t by_bytes = (n + cap_rows - 1) / cap_rows;
    const int64_t by_rows = n / GRAM_RM_MIN_ROWS;
    const int64_t by_part = GRAM_RM_PART_BYTES / ((int64_t)pl.nblk * 16 * 256 * 8);      // the chunk partials stay under GRAM_RM_PART_BYTES
    int64_t nchunk = by_bytes < by_part ? by_bytes : by_part;
    if (nchunk < target) nchunk = target;
    if (nchunk > by_rows) nchunk = by_rows;
    if (nchunk < 1) nchunk = 1;
    const int64_t nstep = (n + 15) / 16;                // 16-row steps: four waves x four rows
    pl.steps = (nstep + nchunk - 1) / nchunk;
    pl.nchunk = (int)((nstep + pl.steps - 1) / pl.steps);      // (no empty chunk)
    pl.tpart_doubles = (size_t)pl.nchunk * pl.nblk * 16 * 256;
    return pl;
}

struct RmDims {
    int64_t n, ldr, steps;
    int p, ntc, nblk;
};

// CM: the same pass -- the same fragments, steps, waves and sums, so the same bits -- over a COLUMN-major float64 x (ldr its column stride):
// the many-response call (api.hip: multi_passes) takes its Gram block from here whichever way x lies, so that its fits do not depend on
// the layout; a lane then reads 8 bytes of each of 16 columns, which is why oem() itself keeps gram.hip for such an x
template <typename T, bool DIAG, bool CM = false>
__device__ __forceinline__ void gram_rm_body(const T *__restrict__ x, const double *__restrict__ y, const double *__restrict__ sums,
                                             double *__restrict__ tdst, const RmDims &a, int bi, int bj, int64_t row_begin,
                                             int64_t row_end, double *lds)
{
    constexpr int NF = DIAG ? 4 : 8;
    constexpr int DEPTH = 3;                                    // steps of loads in flight per wave (4 spills at two waves per SIMD)
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, i = lane & 15, k = lane >> 4;
    const int p = a.p;
    const int64_t n = a.n, ldr = a.ldr;
    const bool shift = shift_needed_wave(sums, p);
    const double cnt = shift ? sums[p + 1] : 1.0;

    // per fragment: the lane's column (clamped into the data), what the lane holds, its shift; live / spec are wave-uniform
    int colc[NF], kind[NF];
    double cf[NF];
    bool live[NF], spec[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int Tc = f < 4 ? 4 * bi + f : 4 * bj + (f - 4);
        const int col = 16 * Tc + i;
        live[f] = Tc < a.ntc;
        spec[f] = live[f] && 16 * Tc + 15 >= p;                 // the tile column holds y, the ones column or nothing
        kind[f] = col < p ? 0 : col == p ? 1 : col == p + 1 ? 2 : 3;
        colc[f] = col < p ? col : p - 1;
        cf[f] = (shift && col <= p) ? sums[col] / cnt : 0.0;
    }

    v4d acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};

    // Loads are unconditional -- the row is clamped to n - 1 and a dead fragment reads column p - 1 -- so the steady-state loop is
    // straight-line code whose outstanding loads hipcc can count: it then waits for the oldest step only (a guarded prefetch makes it
    // wait for everything in flight, which leaves one step of loads to hide the memory latency).
    double buf[DEPTH][NF], ybuf[DEPTH];
    auto load = [&](double (&v)[NF], double &yv, int64_t r0) {
        const int64_t r = r0 + k, rl = r < n ? r : n - 1;
        if constexpr (CM) {
#pragma unroll
            for (int f = 0; f < NF; ++f) v[f] = (double)x[(size_t)colc[f] * ldr + rl];
        } else {
            const T *__restrict__ xr = x + (size_t)rl * ldr;
#pragma unroll
            for (int f = 0; f < NF; ++f) v[f] = (double)xr[colc[f]];
        }
        yv = y[rl];
    };
    auto consume = [&](double (&v)[NF], double yv, int64_t r0) {
        const bool inside = r0 + k < n;
        const bool ragged = r0 + 4 > n;                         // wave-uniform: the last step of the matrix only
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            if (!live[f]) continue;
            double t = v[f];
            if (spec[f]) t = kind[f] == 0 ? t : kind[f] == 1 ? yv : kind[f] == 2 ? 1.0 : 0.0;
            if (shift) t -= cf[f];
            if (ragged) t = inside ? t : 0.0;
            v[f] = t;
        }
#pragma unroll
        for (int ta = 0; ta < 4; ++ta) {
            if (!live[ta]) continue;
#pragma unroll
            for (int tb = 0; tb < 4; ++tb) {
                if (DIAG) {
                    if (tb > ta) continue;
                    acc[ta * 4 + tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[ta], v[tb], acc[ta * 4 + tb], 0, 0, 0);
                } else {
                    if (!live[NF - 4 + tb]) continue;
                    acc[ta * 4 + tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[ta], v[NF - 4 + tb], acc[ta * 4 + tb], 0, 0, 0);
                }
            }
        }
    };

    const int64_t rbase = row_begin + 4 * w;
    const int64_t nst = rbase < row_end ? (row_end - rbase + 15) / 16 : 0;      // 4-row steps of this wave
#pragma unroll
    for (int u = 0; u < DEPTH - 1; ++u) load(buf[u], ybuf[u], rbase + 16 * u);
    int64_t s = 0;
    for (; s + DEPTH <= nst; s += DEPTH) {
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            load(buf[(u + DEPTH - 1) % DEPTH], ybuf[(u + DEPTH - 1) % DEPTH], rbase + 16 * (s + u + DEPTH - 1));
            consume(buf[u], ybuf[u], rbase + 16 * (s + u));
        }
    }
#pragma unroll
    for (int u = 0; u < DEPTH - 1; ++u)                          // fewer than DEPTH steps are left, and their loads are on the way
        if (s + u < nst) consume(buf[u], ybuf[u], rbase + 16 * (s + u));

    // (w0 + w1) + (w2 + w3) through one 32 KB slot: element e = 64 reg + lane of tile t at lds[256 t + e]
    auto put = [&]() {
#pragma unroll
        for (int t = 0; t < 16; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) lds[256 * t + 64 * g + lane] = acc[t][g];
    };
    auto add = [&]() {
#pragma unroll
        for (int t = 0; t < 16; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[t][g] += lds[256 * t + 64 * g + lane];
    };
    if (w == 1) put();
    __syncthreads();
    if (w == 0) add();
    __syncthreads();
    if (w == 3) put();
    __syncthreads();
    if (w == 2) add();
    __syncthreads();
    if (w == 2) put();
    __syncthreads();
    if (w == 0) {
        add();
#pragma unroll
        for (int t = 0; t < 16; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) tdst[256 * t + 64 * g + lane] = acc[t][g];
    }
}

template <typename T, bool CM = false>
__global__ __launch_bounds__(256, 2) void gram_rm_kernel(const T *__restrict__ x, const double *__restrict__ y,
                                                       const double *__restrict__ sums, double *__restrict__ tpart, RmDims a)
{
    __shared__ double lds[16 * 256];
    const int chunk = blockIdx.x / a.nblk, blk = blockIdx.x % a.nblk;
    int bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= blk) ++bi;
    const int bj = blk - bi * (bi + 1) / 2;
    const int64_t row_begin = (int64_t)chunk * a.steps * 16;
    int64_t row_end = row_begin + a.steps * 16;
    if (row_end > a.n) row_end = a.n;
    double *tdst = tpart + (size_t)blockIdx.x * 16 * 256;
    if (bi == bj) gram_rm_body<T, true, CM>(x, y, sums, tdst, a, bi, bj, row_begin, row_end, lds);
    else gram_rm_body<T, false, CM>(x, y, sums, tdst, a, bi, bj, row_begin, row_end, lds);
}

// chunk partials -> the (p + 2)^2 moment buffer: one workgroup per tile slot, four thread groups over the chunks (c = g mod 4, each in
// ascending order, eight loads in flight) combined as (g0 + g1) + (g2 + g3), as moments_reduce_kernel (gram.hip) does; the MFMA
// accumulator layout (row = (lane >> 4) + 4 reg, col = lane & 15) is scattered into both triangles
__global__ __launch_bounds__(1024) void gram_rm_reduce_kernel(const double *__restrict__ tpart, int p, int ntc, int nblk, int nchunk,
                                                               double *__restrict__ M)
{
    __shared__ double part[4][256];
    const int q = p + 2;
    const int blk = blockIdx.x / 16, t = blockIdx.x % 16, ta = t / 4, tb = t % 4;
    int bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= blk) ++bi;
    const int bj = blk - bi * (bi + 1) / 2;
    const int I = 4 * bi + ta, J = 4 * bj + tb;
    if (I >= ntc || J >= ntc || J > I) return;                  // (slots the pass never wrote; the whole workgroup leaves)
    const int e = threadIdx.x & 255, grp = threadIdx.x >> 8;
    const double *src = tpart + (size_t)blockIdx.x * 256 + e;
    const size_t stride = (size_t)nblk * 16 * 256;
    double s = 0.0;
    int c = grp;
    for (; c + 28 < nchunk; c += 32) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(c + 4 * u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; c < nchunk; c += 4) s += src[(size_t)c * stride];
    part[grp][e] = s;
    __syncthreads();
    s = (part[0][e] + part[1][e]) + (part[2][e] + part[3][e]);
    const int reg = e >> 6, lane = e & 63;
    const int row = 16 * I + (lane >> 4) + 4 * reg, col = 16 * J + (lane & 15);
    if (grp == 0 && row < q && col < q && row >= col) {
        M[(size_t)col * q + row] = s;
        M[(size_t)row * q + col] = s;
    }
}

int launch_gram_rm(hipStream_t s, const GramRmPlan &pl, const void *x, int dtype, int64_t n, int64_t ldr, const double *y,
                   const double *sums, double *tpart)
{
    RmDims a;
    a.n = n; a.ldr = ldr; a.steps = pl.steps; a.p = pl.p; a.ntc = pl.ntc; a.nblk = pl.nblk;
    const dim3 grid((unsigned)((size_t)pl.nchunk * pl.nblk));
    if (dtype < 0) hipLaunchKernelGGL((gram_rm_kernel<double, true>), grid, dim3(256), 0, s, (const double *)x, y, sums, tpart, a);      // column-major, ldr the column stride
    else if (dtype == OEMGPU_F32) hipLaunchKernelGGL(gram_rm_kernel<float>, grid, dim3(256), 0, s, (const float *)x, y, sums, tpart, a);
    else hipLaunchKernelGGL(gram_rm_kernel<double>, grid, dim3(256), 0, s, (const double *)x, y, sums, tpart, a);
    OEM_HIP(hipGetLastError());
    return 0;
}

int launch_gram_rm_reduce(hipStream_t s, const GramRmPlan &pl, const double *tpart, double *moments)
{
    hipLaunchKernelGGL(gram_rm_reduce_kernel, dim3(pl.nblk * 16), dim3(1024), 0, s, tpart, pl.p, pl.ntc, pl.nblk, pl.nchunk, moments);
    OEM_HIP(hipGetLastError());
    return 0;
}

}  // namespace oemgpu
