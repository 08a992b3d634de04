// sparse_wide.hip -- the p >= n fit of a sparse x from its non-zeros (ref src/oem_sparse.h:607-612, 638-647; src/oem_big.h:537-541,
// 568-584, 743-764, 880-897): u = X'(y - X beta)/n + d beta on the data as they are, d = 1.005 lambda_max(X X'/n).
//
// oemgpu_fit_sparse used to fill an n x p matrix of doubles on the host for this branch and hand it to the dense wide engine:
// 8 n p bytes on the host, again on the device, and read every iteration whatever the density.  Here both products of an
// iteration run over the resident compressed arrays of an oemgpu_sparse_x (logistic.hpp):
//   row pass      t_i = sum_k cval[k] v[ccol[k]]      over the compressed rows (entries in column order),
//   column pass   g_j = sum_k val[k]  w[rowidx[k]]    over the compressed columns (entries in row order),
// 12 bytes per non-zero per pass plus the vectors.  Both are ONE kernel, spw_gather_kernel<L>: a line (row or column) belongs to
// L = 1, 2, .. 64 neighbouring lanes of a wave, lane s of them takes the entries s, s + L, .. of the line, and a butterfly over
// the L lanes adds their sums -- one fixed order, no floating-point atomics, the same bits on every call.  L comes from the mean
// line length (about four entries per lane) and is raised while the launch would leave CUs idle (spw_plan).  A line of more than
// SPW_LONG_PER_LANE L entries (a full row, an all-ones column) is left out by that kernel and taken by a workgroup of
// spw_long_kernel, whose 256 threads stride over it and add their sums wave by wave, then in wave order.  The long lines are
// listed once per call (spw_scan_kernel: an integer counter hands out the slots, so the ORDER of the list may differ between calls;
// every line's sum is its own and lands in its own slot, so no result depends on it).
// The iteration around the passes is path_large.hip: run_path_sparse_wide.  This file also holds what else the fit reads from
// the data: X'y / n, colsq and the scaled lambda_zero vector from the compressed columns in one pass (the gather with STATS), and
// the loss of the returned coefficients as a row pass and a sum in row-chunk order.
//
// cv.oem's fold fit (oemgpu_fit_sparse_wide_fold_res; ref R/cv_oem.R:155-175 slices x[!which, ] and calls oem()): the same kernels with
// MASK, on the handle as it lies.  SpwMask names the rows with foldid == leave_out.
//   row pass      a left-out row is not read and its output is an exact 0.0 (the gather writes it whatever the row's length; a
//                 left-out long row's workgroup returns at once).  EVERY row pass of a fold fit is masked: t = X beta, the second
//                 half of the eigen product, the loss.
//   column pass   not masked in the iteration and the eigen product: its input vector is exactly zero in the left-out rows, so a
//                 finite stored value contributes fma(x, 0, s) = s.  (Stored values of a left-out row must be finite.)
//   STATS pass    a left-out entry is excluded by a select on foldid[idx[k]] -- from x_j'y and from sum x_j^2 -- so y of a left-out
//                 row is never read; spw_y_kernel and spw_resid_sq_kernel select the same way.
// The lane of an entry follows its position in the stored line, left-out entries included, so a column's sum over the kept rows is
// added in another order than on the sliced matrix: a fold fit matches the fit of x[keep, ] to tolerance, not bit for bit.  The
// unmasked instantiations are what they were (the mask is a trailing argument they never touch).
#include "ctx.hpp"
#include "path_dev.hpp"

namespace oemgpu {

namespace {

// what the STATS form of the gather leaves per column (ref src/oem_big.h:743-764, 810-826): xy = x_j'y / n, colsq_inv_j =
// 1 / sqrt(sum x_j^2 / (n - 1)) (a zero column: 1; without standardize: 1) in the scale slot of `stats`, xy_std = xy colsq_inv
struct SpwStats {
    double *xy, *stats, *xy_std;
    int standardize, p;
    double n;
};

__device__ __forceinline__ void spw_store_stats(const SpwStats &S, int j, double dot, double ss)
{
    const double xy = dot / S.n;
    double cs = ss / (S.n - 1.0);
    if (cs == 0.0) cs = 1.0;
    const double inv = S.standardize ? 1.0 / sqrt(cs) : 1.0;
    S.xy[j] = xy;
    S.stats[4 + j] = 0.0;
    S.stats[4 + S.p + j] = inv;
    S.xy_std[j] = xy * inv;
}

// the rows a fold fit leaves out: foldid[row] == leave_out (MASK forms only)
struct SpwMask {
    const int32_t *foldid;
    int leave_out;
};

// MASK without STATS: the lines are ROWS and a left-out line is not read, its output an exact 0.0 (a long one's too: written here).
// MASK with STATS: the lines are columns and a left-out ENTRY is excluded by a select; vec (y) is not read there.
template <int L, bool STATS, bool MASK>
__global__ __launch_bounds__(256) void spw_gather_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                                         const double *__restrict__ val, int nlines, const double *__restrict__ vec,
                                                         double *__restrict__ out, double scale, const int *__restrict__ done, SpwStats S,
                                                         SpwMask M)
{
    if (done && *done) return;
    const int64_t gt = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t line = gt / L;
    const int sub = (int)(gt % L);
    double s = 0.0, s2 = 0.0;
    bool mine = false;
    if (line < nlines) {
        if (MASK && !STATS && M.foldid[line] == M.leave_out) {
            if (sub == 0) out[line] = 0.0;
        } else {
            const int64_t k0 = ptr[line], k1 = ptr[line + 1];
            mine = k1 - k0 <= (int64_t)SPW_LONG_PER_LANE * L;             // (a longer line: spw_long_kernel's)
            if (mine) {
#pragma unroll 4
                for (int64_t k = k0 + sub; k < k1; k += L) {
                    const double x = val[k];
                    if (MASK && STATS) {
                        const int32_t r = idx[k];
                        if (M.foldid[r] != M.leave_out) { s = fma(x, vec[r], s); s2 = fma(x, x, s2); }
                    } else {
                        s = fma(x, vec[idx[k]], s);
                        if (STATS) s2 = fma(x, x, s2);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        if (STATS) s2 += __shfl_xor(s2, o, 64);
    }
    if (mine && sub == 0) {
        if (STATS) spw_store_stats(S, (int)line, s, s2);
        else out[line] = s * scale;
    }
}

template <bool STATS, bool MASK>
__global__ __launch_bounds__(256) void spw_long_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                                       const double *__restrict__ val, const int32_t *__restrict__ list,
                                                       const double *__restrict__ vec, double *__restrict__ out, double scale,
                                                       const int *__restrict__ done, SpwStats S, SpwMask M)
{
    if (done && *done) return;
    __shared__ double sh[2][4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int line = list[blockIdx.x];
    if (MASK && !STATS && M.foldid[line] == M.leave_out) return;          // (its 0.0 is the gather's; uniform over the workgroup)
    const int64_t k0 = ptr[line], k1 = ptr[line + 1];
    double s = 0.0, s2 = 0.0;
#pragma unroll 4
    for (int64_t k = k0 + tid; k < k1; k += 256) {
        const double x = val[k];
        if (MASK && STATS) {
            const int32_t r = idx[k];
            if (M.foldid[r] != M.leave_out) { s = fma(x, vec[r], s); s2 = fma(x, x, s2); }
        } else {
            s = fma(x, vec[idx[k]], s);
            if (STATS) s2 = fma(x, x, s2);
        }
    }
    s = wave_sum(s);
    if (STATS) s2 = wave_sum(s2);
    if (lane == 0) { sh[0][w] = s; sh[1][w] = s2; }
    __syncthreads();
    if (tid == 0) {
        const double t = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
        if (STATS) spw_store_stats(S, line, t, (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]));
        else out[line] = t * scale;
    }
}

// the lines of more than `thr` entries into `list` (at most nlines of them), their number in cnt[0]; cnt[1] = the longest line
__global__ __launch_bounds__(256) void spw_scan_kernel(const int64_t *__restrict__ ptr, int nlines, int64_t thr, int32_t *__restrict__ list,
                                                       int *__restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int len = 0;
    if (i < nlines) {
        const int64_t l = ptr[i + 1] - ptr[i];
        len = l > 2147483647LL ? 2147483647 : (int)l;
        if (l > thr) list[atomicAdd(&cnt[0], 1)] = (int32_t)i;
    }
    for (int o = 32; o > 0; o >>= 1) { const int other = __shfl_xor(len, o, 64); len = other > len ? other : len; }
    if ((threadIdx.x & 63) == 0 && len > 0) atomicMax(&cnt[1], len);
}

// stats[0 .. 3] of the data as they are: no centring and no scaling of y (0, 1, sum y^2, n); the shift flags 0.  MASK: the sum over
// the kept rows (y of a left-out row is not read) and nobs = the kept rows in stats[3]
template <bool MASK>
__global__ __launch_bounds__(1024) void spw_y_kernel(const double *__restrict__ y, int n, int p, double *__restrict__ stats, SpwMask M, int nobs)
{
    __shared__ double sh[16];
    const int tid = threadIdx.x;
    double yy = 0.0;
    for (int i = tid; i < n; i += 1024) {
        if (MASK) { if (M.foldid[i] != M.leave_out) yy = fma(y[i], y[i], yy); }
        else yy = fma(y[i], y[i], yy);
    }
    yy = wave_sum(yy);
    if ((tid & 63) == 0) sh[tid >> 6] = yy;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += sh[k];
        stats[0] = 0.0; stats[1] = 1.0; stats[2] = t; stats[3] = (double)(MASK ? nobs : n);
        stats[stats_shift_flag(p)] = 0.0; stats[stats_shift_flag(p) + 1] = 0.0;
    }
}

// sum over the chunk's 2048 rows of (y - t)^2 -> part[c]; MASK: over its kept rows (the chunks and their order stay)
template <bool MASK>
__global__ __launch_bounds__(256) void spw_resid_sq_kernel(const double *__restrict__ y, const double *__restrict__ t, int n, double *__restrict__ part,
                                                           SpwMask M)
{
    __shared__ double ws[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int64_t i = (int64_t)c * 2048 + m * 256 + tid;
        if (i < n && !(MASK && M.foldid[i] == M.leave_out)) { const double r = y[i] - t[i]; s = fma(r, r, s); }
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) ws[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) part[c] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// loss[k] = the chunk sums of (penalty, lambda) k in chunk order
__global__ void spw_loss_sum_kernel(const double *__restrict__ part, int nchunk, int nk, double *__restrict__ loss)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nk) return;
    double t = 0.0;
    for (int c = 0; c < nchunk; ++c) t += part[(size_t)k * nchunk + c];
    loss[k] = t;
}

int spw_lanes(int64_t lines, int64_t nnz, int num_cu)
{
    const double avg = lines > 0 ? (double)nnz / (double)lines : 0.0;
    int L = 1;
    while (L < 64 && 4.0 * L < avg) L *= 2;                              // about four entries per lane
    while (L < 64 && (lines * L + 255) / 256 < (int64_t)num_cu) L *= 2;  // no CU idle where more lanes per line can fill it
    return L;
}

template <bool STATS, bool MASK>
int spw_launch(hipStream_t s, const int64_t *ptr, const int32_t *idx, const double *val, int nlines, int L, const int32_t *list, int nlong,
               const double *vec, double *out, double scale, const int *done, const SpwStats &S, const SpwMask &M = SpwMask{nullptr, 0})
{
    const unsigned wgs = (unsigned)(((int64_t)nlines * L + 255) / 256);
#define OEM_SPW_CASE(LL) case LL: hipLaunchKernelGGL((spw_gather_kernel<LL, STATS, MASK>), dim3(wgs), dim3(256), 0, s, ptr, idx, val, nlines, vec, out, scale, done, S, M); break
    switch (L) {
    OEM_SPW_CASE(1); OEM_SPW_CASE(2); OEM_SPW_CASE(4); OEM_SPW_CASE(8); OEM_SPW_CASE(16); OEM_SPW_CASE(32); OEM_SPW_CASE(64);
    default: set_error("internal: sparse wide engine lanes"); return OEMGPU_ERR_INTERNAL;
    }
#undef OEM_SPW_CASE
    if (nlong > 0) hipLaunchKernelGGL((spw_long_kernel<STATS, MASK>), dim3(nlong), dim3(256), 0, s, ptr, idx, val, list, vec, out, scale, done, S, M);
    return 0;
}

}  // namespace

SpwPlan spw_plan(int64_t n, int p, int64_t nnz, int64_t longest_row, int64_t longest_col, int num_cu, int force_row_L, int force_col_L)
{
    SpwPlan P;
    P.route = sparse_wide_route(n, p, nnz) ? 1 : 0;
    P.row_L = force_row_L ? force_row_L : spw_lanes(n, nnz, num_cu);
    P.col_L = force_col_L ? force_col_L : spw_lanes(p, nnz, num_cu);
    P.long_rows = longest_row > (int64_t)SPW_LONG_PER_LANE * P.row_L ? 1 : 0;
    P.long_cols = longest_col > (int64_t)SPW_LONG_PER_LANE * P.col_L ? 1 : 0;
    P.row_wgs = (int)((n * P.row_L + 255) / 256);
    P.col_wgs = (int)(((int64_t)p * P.col_L + 255) / 256);
    Bump B;
    B.take(sizeof(double) * spw_vec_doubles(n));
    B.take(sizeof(int32_t) * ((size_t)n + 1));
    B.take(sizeof(int32_t) * ((size_t)p + 1));
    B.take(64);
    P.ws_bytes = B.off;
    return P;
}

int launch_spw_rows(hipStream_t s, const SpwArgs &A, const double *v, double *out, double scale, const int *done)
{
    if (A.foldid)                                            // a fold fit: every row pass leaves the fold's rows out
        return spw_launch<false, true>(s, A.rowptr, A.ccol, A.cval, A.n, A.plan.row_L, A.long_row_list, A.n_long_rows, v, out, scale, done, SpwStats(),
                                       SpwMask{A.foldid, A.leave_out});
    return spw_launch<false, false>(s, A.rowptr, A.ccol, A.cval, A.n, A.plan.row_L, A.long_row_list, A.n_long_rows, v, out, scale, done, SpwStats());
}

int launch_spw_cols(hipStream_t s, const SpwArgs &A, const double *w, double *out, double scale, const int *done)
{
    return spw_launch<false, false>(s, A.colptr, A.rowidx, A.val, A.p, A.plan.col_L, A.long_col_list, A.n_long_cols, w, out, scale, done, SpwStats());
}

// the two lists of long lines and the longest row and column: cnt (device, 4 ints) <- rows: number, longest | columns: number, longest
int launch_spw_scan(hipStream_t s, const SpwArgs &A, int32_t *row_list, int32_t *col_list, int *cnt)
{
    OEM_HIP(hipMemsetAsync(cnt, 0, 4 * sizeof(int), s));
    hipLaunchKernelGGL(spw_scan_kernel, dim3((unsigned)(((int64_t)A.n + 255) / 256)), dim3(256), 0, s, A.rowptr, A.n,
                       (int64_t)SPW_LONG_PER_LANE * A.plan.row_L, row_list, cnt);
    hipLaunchKernelGGL(spw_scan_kernel, dim3((unsigned)(((int64_t)A.p + 255) / 256)), dim3(256), 0, s, A.colptr, A.p,
                       (int64_t)SPW_LONG_PER_LANE * A.plan.col_L, col_list, cnt + 2);
    OEM_HIP(hipGetLastError());
    return 0;
}

// X'y / n, the column scales and the scaled lambda_zero vector from the compressed columns in one pass; stats[0 .. 3] from y
int launch_spw_stats(hipStream_t s, const SpwArgs &A, const double *y, int standardize, double *xy, double *stats, double *xy_std)
{
    SpwStats S;
    S.xy = xy; S.stats = stats; S.xy_std = xy_std; S.standardize = standardize; S.p = A.p; S.n = (double)(A.foldid ? A.nk : A.n);
    const SpwMask M{A.foldid, A.leave_out};
    int rc;
    if (A.foldid) {
        hipLaunchKernelGGL(spw_y_kernel<true>, dim3(1), dim3(1024), 0, s, y, A.n, A.p, stats, M, A.nk);
        rc = spw_launch<true, true>(s, A.colptr, A.rowidx, A.val, A.p, A.plan.col_L, A.long_col_list, A.n_long_cols, y, (double *)nullptr, 1.0,
                                    (const int *)nullptr, S, M);
    } else {
        hipLaunchKernelGGL(spw_y_kernel<false>, dim3(1), dim3(1024), 0, s, y, A.n, A.p, stats, M, A.n);
        rc = spw_launch<true, false>(s, A.colptr, A.rowidx, A.val, A.p, A.plan.col_L, A.long_col_list, A.n_long_cols, y, (double *)nullptr, 1.0,
                                     (const int *)nullptr, S);
    }
    if (rc) return rc;
    OEM_HIP(hipGetLastError());
    return 0;
}

// compute.loss (ref src/oem_sparse.h:932-941): sum (y - X b)^2 of the RETURNED coefficients b [nk][rows] (slot 0 the intercept: none
// here), one row pass per (penalty, lambda) into t, its squares by chunks of 2048 rows into part [nk][chunks], added in chunk order
int launch_spw_loss(hipStream_t s, const SpwArgs &A, const double *y, const double *b, int rows, int nk, double *t, double *part, double *loss)
{
    const int nchunk = (int)(((int64_t)A.n + 2047) / 2048);
    for (int k = 0; k < nk; ++k) {
        const int rc = launch_spw_rows(s, A, b + (size_t)k * rows + 1, t, 1.0, nullptr);
        if (rc) return rc;
        if (A.foldid) hipLaunchKernelGGL(spw_resid_sq_kernel<true>, dim3(nchunk), dim3(256), 0, s, y, t, A.n, part + (size_t)k * nchunk, SpwMask{A.foldid, A.leave_out});
        else hipLaunchKernelGGL(spw_resid_sq_kernel<false>, dim3(nchunk), dim3(256), 0, s, y, t, A.n, part + (size_t)k * nchunk, SpwMask{nullptr, 0});
    }
    hipLaunchKernelGGL(spw_loss_sum_kernel, dim3((nk + 255) / 256), dim3(256), 0, s, part, nchunk, nk, loss);
    OEM_HIP(hipGetLastError());
    return 0;
}

}  // namespace oemgpu

extern "C" {
#pragma GCC visibility push(default)

// out[0] route (sparse_wide_route), [1] rows per wave, [2] columns per wave, [3] long-row form used, [4] long-column form used,
// [5] workgroups of the row pass, [6] of the column pass (short forms), [7] bytes of the engine's own workspace
int oemgpu_selftest_sparse_wide_plan(int64_t n, int32_t p, int64_t nnz, int64_t longest_row, int64_t longest_col, int32_t num_cu, int64_t *out)
{
    using namespace oemgpu;
    if (n < 1 || p < 1 || nnz < 0 || longest_row < 0 || longest_col < 0 || num_cu < 1 || !out) { set_error("selftest_sparse_wide_plan: bad argument"); return OEMGPU_ERR_ARG; }
    const SpwPlan P = spw_plan(n, p, nnz, longest_row, longest_col, num_cu);
    out[0] = P.route; out[1] = 64 / P.row_L; out[2] = 64 / P.col_L; out[3] = P.long_rows; out[4] = P.long_cols;
    out[5] = P.row_wgs; out[6] = P.col_wgs; out[7] = (int64_t)P.ws_bytes;
    return 0;
}

#pragma GCC visibility pop
}
