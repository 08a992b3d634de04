// logistic_rm.hip -- the row pass and the scale pass of the dense binomial fit (logistic.hip: logit_rows_kernel, logit_scale_kernel) for
// an x that is n x p ROW-major with row stride ldr >= p, float64 or float32 elements, aligned to its element only, read where it lies.
// What they stand in for is what logistic.hip states: the IRLS quantities of `.Call("oem_fit_logistic_dense", ...)` (ref
// src/oem_logistic_dense.h:727-738 the column scales, :762-805 the first XY, :940-1000 prob, W, the floor loop, X'(y - prob) and the
// Z = sqrt(W) X s of X'WX).
//
// Bits: every sum is taken in the order of the column-major kernels, so a fit on a row-major tensor is the column-major fit on the
// same values bit for bit (float32 elements are widened in the register they were loaded into; all arithmetic is FP64):
//   * eta of a row: four partials over the columns j = 0, 1, 2, 3 (mod 4), each in ascending j as fma(v, beta[o + j] s[j], e), combined
//     as ((e0 + e1) + (e2 + e3)) + b0;
//   * X'r: accumulator j takes the rows of a chunk in ascending order, fma(x, r, a) from 0; chunks are summed in chunk order by
//     logit_sum_kernel; the chunk and Z-block boundaries are the caller's LogitPlan, i.e. the column-major call's;
//   * sum r and the loss sum: per lane (row mod 64) over the chunk's sub-blocks, then the 64 lanes in lane order;
//   * Z = sw (v s[j]), column 0 = sw with an intercept, column-major with ldz rows per block; rows left out of a fold fit are zeros;
//   * the column scale: 256 partials per column, partial t the fma sum of x^2 over the rows i = t (mod 256) in ascending i, added in t
//     order, then t / (n_eff - 1), 0 -> 1, 1 / sqrt.
//
// Layout.  A workgroup owns a chunk and walks it in sub-blocks of 64 rows.  A sub-block is staged into LDS as tile[j 65 + i] (column j,
// row i: the layout of the column-major kernel's staged form) by coalesced ROW reads: a wave takes a row and its lanes take
// consecutive columns -- 512 B per wave load for float64, 256 B for float32 -- sixteen or thirty-two loads in flight per wave.  From
// the tile the phases run as in logit_rows_kernel: lane = row for eta (phase 1) and Z (phase 4), thread = column for X'r (phase 3);
// the odd pitch 65 keeps the row-wise writes and both kinds of reads off each other's banks.  When 64 x p does not fit the LDS of a
// CU beside the p accumulators the columns go in bands (logit_rm_plan: every band but the last a multiple of 4 wide, so the four eta
// partials carry across bands in their order); phases 3 and 4 then read the bands a second time, once r and sqrt W of the sub-block
// are known -- two reads of the sub-block, as the unstaged column-major form makes.
//
// What is never loaded: columns p .. ldr - 1, rows >= n, and the rows a fold fit leaves out.  The loads are not guarded: the column is
// clamped to the band's last and the row of a lane that has none to load is replaced by the sub-block's first row that is in the fit
// (a row the same pass loads anyway), and the value is then SELECTED (0), never multiplied by zero, so NaN next to the data stays
// out.  A sub-block without any row in the fit is not read at all.
#include "logistic.hpp"

namespace oemgpu {

static const size_t LOGIT_RM_LDS_BYTES = (size_t)160 << 10;   // LDS of a gfx950 CU
static const size_t LOGIT_RM_STATIC = 4096;                  // the kernel's static arrays: etap (2048), rsh, wsh (512 each), red (1024)

LogitRmPlan logit_rm_plan(int p)
{
    LogitRmPlan R;
    int bw = (int)((LOGIT_RM_LDS_BYTES - LOGIT_RM_STATIC - 8 * (size_t)p) / (8 * 65));   // columns whose 64-row tile fits beside the accumulators
    bw = bw >= p ? p : bw / 4 * 4;                     // one band (the sub-block is read once), else the widest multiple of 4
    R.bw = bw;
    R.nband = (p + bw - 1) / bw;
    R.lds = 8 * (size_t)p + 8 * 65 * (size_t)bw;
    R.lds_total = R.lds + LOGIT_RM_STATIC;
    return R;
}

namespace {

// Stages NC x 64 columns [c0 + cb, ...) of the band (bw wide, starting at column c0 of x) for the 64 rows from r0: wave w loads the rows
// i = w (mod 4), a lane a column.  mask: the rows of the sub-block that are in the fit (bit i), not 0; rfill: the first of them.
template <typename T, int NC>
__device__ __forceinline__ void stage_cols(const T *__restrict__ x, int64_t ldr, int64_t r0, int c0, int bw, int cb, unsigned long long mask,
                                           int rfill, int w, int lane, double *__restrict__ tile)
{
    T v[NC][16];
    int jj[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        jj[c] = cb + 64 * c + lane;
        const int jc = jj[c] < bw ? jj[c] : bw - 1;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int i = w + 4 * u;
            const int il = ((mask >> i) & 1ull) ? i : rfill;
            v[c][u] = x[(size_t)(r0 + il) * ldr + (c0 + jc)];
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (jj[c] >= bw) continue;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int i = w + 4 * u;
            tile[jj[c] * 65 + i] = ((mask >> i) & 1ull) ? (double)v[c][u] : 0.0;
        }
    }
}

template <typename T>
__device__ __forceinline__ void stage_band(const T *__restrict__ x, int64_t ldr, int64_t r0, int c0, int bw, unsigned long long mask, int w, int lane,
                                           double *__restrict__ tile)
{
    if (mask == 0ull) {                                  // (wave-uniform) no row of the sub-block is in the fit: nothing is read
        for (int jj = lane; jj < bw; jj += 64)
#pragma unroll
            for (int u = 0; u < 16; ++u) tile[jj * 65 + w + 4 * u] = 0.0;
        return;
    }
    const int rfill = __builtin_ctzll(mask);
    int cb = 0;
    for (; cb + 128 <= bw; cb += 128) stage_cols<T, 2>(x, ldr, r0, c0, bw, cb, mask, rfill, w, lane, tile);
    for (; cb < bw; cb += 64) stage_cols<T, 1>(x, ldr, r0, c0, bw, cb, mask, rfill, w, lane, tile);
}

// logit_rows_kernel (logistic.hip) on a row-major x: the same arguments with (x, ldr) and the band plan (bw, nband).  mode 0: r = y;
// mode 1: the IRLS quantities.  zout: Z block (ldz rows), or null.  MASKED: rows with foldid[row] == leave_out are not in the fit.
template <typename T, bool MASKED>
__global__ __launch_bounds__(256) void logit_rows_rm_kernel(const T *__restrict__ x, int64_t n, int64_t ldr, int p, int bw, int nband,
                                                            const double *__restrict__ y, const double *__restrict__ beta,
                                                            const double *__restrict__ s, int intercept, int mode, int64_t irls_i, int64_t ch,
                                                            int64_t chunk0, int64_t row0, double *__restrict__ zout, int64_t ldz,
                                                            double *__restrict__ part, const int32_t *__restrict__ foldid, int32_t leave_out)
{
    extern __shared__ double lsh[];
    double *acc = lsh;                               // p
    double *tile = lsh + p;                          // 65 bw
    __shared__ double etap[4][64], rsh[64], wsh[64], red[2][64];
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
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
        const unsigned long long mask = __ballot(kept);
        // phase 1: the bands staged in turn; wave w adds the columns j = w (mod 4) of a band to its eta partial (lane = row).  With one
        // band the tile stays for phases 3 and 4; mode 0 with several bands needs no first walk
        double e = 0.0;
        if (mode || nband == 1) {
            for (int b = 0; b < nband; ++b) {
                const int c0 = b * bw, wb = (p - c0 < bw) ? p - c0 : bw;
                if (b) __syncthreads();              // (the tile's readers of the band before)
                stage_band<T>(x, ldr, r0, c0, wb, mask, w, lane, tile);
                __syncthreads();
                if (mode)
                    for (int j = w; j < wb; j += 4) e = fma(tile[j * 65 + lane], beta[o + c0 + j] * s[c0 + j], e);
            }
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
        }
        __syncthreads();
        const int lim = (int)((r_hi - r0) < 64 ? (r_hi - r0) : 64);
        for (int b = 0; b < nband; ++b) {
            const int c0 = b * bw, wb = (p - c0 < bw) ? p - c0 : bw;
            if (nband > 1) {
                stage_band<T>(x, ldr, r0, c0, wb, mask, w, lane, tile);
                __syncthreads();
            }
            // phase 3: thread j accumulates column j over the 64 rows, in row order
            for (int j = tid; j < wb; j += 256) {
                double a = acc[c0 + j];
                for (int i = 0; i < lim; ++i) a = fma(tile[j * 65 + i], rsh[i], a);
                acc[c0 + j] = a;
            }
            // phase 4: Z = sqrt(W) (x s) of these rows, lane = row
            if (zout && ok)
                for (int j = w; j < wb; j += 4) zout[(size_t)(o + c0 + j) * ldz + (row - row0)] = wsh[lane] * (tile[j * 65 + lane] * s[c0 + j]);
            __syncthreads();
        }
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

// The 256 partials of logit_scale_kernel's columns: workgroup (bx, by) owns the columns 64 bx .. + 64 (lane = column) and the residues
// t = 4 by + w (wave = residue); sp[t p + j] = the fma sum of x[i][j]^2 over the rows i = t (mod 256) in ascending i that are in the fit.
// Eight rows of loads in flight per wave, none of them guarded: a row that is past n or left out is replaced by fill_row (a row that
// is in the fit) and its value dropped, so it is never loaded.
template <typename T>
__global__ __launch_bounds__(256) void logit_scale_rm_part_kernel(const T *__restrict__ x, int64_t n, int64_t ldr, int p, double *__restrict__ sp,
                                                                  const int32_t *__restrict__ foldid, int32_t leave_out, int64_t fill_row)
{
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int t = 4 * blockIdx.y + w;
    const int j = 64 * blockIdx.x + lane, jc = j < p ? j : p - 1;
    double a = 0.0;
    for (int64_t i0 = t; i0 < n; i0 += 8 * 256) {
        T v[8];
        bool keep[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t i = i0 + 256 * u;
            keep[u] = i < n && (!foldid || foldid[i < n ? i : n - 1] != leave_out);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = x[(size_t)(keep[u] ? i0 + 256 * u : fill_row) * ldr + jc];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (keep[u]) { const double d = (double)v[u]; a = fma(d, d, a); }
    }
    if (j < p) sp[(size_t)t * p + j] = a;
}

// the partials added in t order, then colsq = t / (n_eff - 1), 0 -> 1, s = 1 / sqrt(colsq) (h :734-737)
__global__ __launch_bounds__(256) void logit_scale_rm_sum_kernel(const double *__restrict__ sp, int p, double *__restrict__ s, int64_t n_eff)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= p) return;
    double t = 0.0;
    for (int k = 0; k < 256; ++k) t += sp[(size_t)k * p + j];
    double cs = t / ((double)n_eff - 1.0);
    if (cs == 0.0) cs = 1.0;
    s[j] = 1.0 / sqrt(cs);
}

template <typename T, bool MASKED>
int rows_rm_launch(hipStream_t s, const LogitRmPlan &R, const T *x, int64_t n, int64_t ldr, int p, const double *y, const double *beta,
                   const double *sc, int intercept, int mode, int64_t irls_i, int64_t ch, int64_t c0, int64_t nc, int64_t row0, double *z,
                   int64_t ldz, double *part, const int32_t *foldid, int32_t leave_out)
{
    if (lds_limit_once(reinterpret_cast<const void *>(&logit_rows_rm_kernel<T, MASKED>), R.lds)) return OEMGPU_ERR_HIP;
    hipLaunchKernelGGL((logit_rows_rm_kernel<T, MASKED>), dim3((unsigned)nc), dim3(256), R.lds, s, x, n, ldr, p, R.bw, R.nband, y, beta, sc, intercept,
                       mode, irls_i, ch, c0, row0, z, ldz, part, foldid, leave_out);
    OEM_HIP(hipGetLastError());
    return 0;
}

}  // namespace

int launch_logit_rows_rm(hipStream_t s, const LogitRmPlan &R, const void *x, int dtype, int64_t n, int64_t ldr, int p, const double *y,
                         const double *beta, const double *sc, int intercept, int mode, int64_t irls_i, int64_t ch, int64_t c0, int64_t nc,
                         int64_t row0, double *z, int64_t ldz, double *part, const int32_t *foldid, int32_t leave_out)
{
    if (dtype == OEMGPU_F32) {
        const float *xf = (const float *)x;
        return foldid ? rows_rm_launch<float, true>(s, R, xf, n, ldr, p, y, beta, sc, intercept, mode, irls_i, ch, c0, nc, row0, z, ldz, part, foldid, leave_out)
                      : rows_rm_launch<float, false>(s, R, xf, n, ldr, p, y, beta, sc, intercept, mode, irls_i, ch, c0, nc, row0, z, ldz, part, nullptr, 0);
    }
    const double *xd = (const double *)x;
    return foldid ? rows_rm_launch<double, true>(s, R, xd, n, ldr, p, y, beta, sc, intercept, mode, irls_i, ch, c0, nc, row0, z, ldz, part, foldid, leave_out)
                  : rows_rm_launch<double, false>(s, R, xd, n, ldr, p, y, beta, sc, intercept, mode, irls_i, ch, c0, nc, row0, z, ldz, part, nullptr, 0);
}

// sp: 256 p doubles of workspace; fill_row: a row that is in the fit
int launch_logit_scale_rm(hipStream_t s, const void *x, int dtype, int64_t n, int64_t ldr, int p, double *sp, double *sc, const int32_t *foldid,
                          int32_t leave_out, int64_t n_eff, int64_t fill_row)
{
    const dim3 grid((unsigned)((p + 63) / 64), 64);
    if (dtype == OEMGPU_F32) hipLaunchKernelGGL(logit_scale_rm_part_kernel<float>, grid, dim3(256), 0, s, (const float *)x, n, ldr, p, sp, foldid, leave_out, fill_row);
    else hipLaunchKernelGGL(logit_scale_rm_part_kernel<double>, grid, dim3(256), 0, s, (const double *)x, n, ldr, p, sp, foldid, leave_out, fill_row);
    hipLaunchKernelGGL(logit_scale_rm_sum_kernel, dim3((p + 255) / 256), dim3(256), 0, s, sp, p, sc, n_eff);
    OEM_HIP(hipGetLastError());
    return 0;
}

}  // namespace oemgpu
