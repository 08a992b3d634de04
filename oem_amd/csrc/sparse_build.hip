// sparse_build.hip -- the resident sparse x (oemgpu_sparse_x) from compressed columns OR compressed rows that are already on the device
// (oemgpu_sparse_x_create_dev): what sparse_x_build makes of a host matrix, array for array, without the matrix leaving HBM.
//
//   check   sb_ptr_kernel (a thread per pointer) widens the pointers into the handle and flags ptr[0] != 0, ptr[last] != nnz and a
//           decreasing pointer; sb_entry_kernel (a thread per non-zero) finds the entry's line by one binary search over the checked
//           pointers, widens index and value into the handle, and takes an integer minimum of 2 k + class over the entries k that are
//           out of range (class 0) or not above their predecessor in the line (class 1): the first offending entry in csc_check's
//           walk.  The host reads the flags after each of the two kernels; nothing indexes with an index before it has passed.
//   sort    the input lines are sorted, so a STABLE sort of the non-zeros by their index gives the other orientation in its final
//           order: least-significant-digit counting sort on the index, digits of at most 11 bits.  A pass is
//             sb_hist_kernel     workgroup w counts the digits of its `per` consecutive non-zeros in LDS (integer atomics) -> tab[d][w];
//             sb_scan_wg_kernel  a wave per digit: tab[d][.] -> the exclusive sums over the workgroups, tot[d];
//             sb_scan_bins_kernel one workgroup: tot -> the exclusive sums over the digits;
//             sb_scatter_kernel  workgroup w walks its non-zeros in tiles of 256 (thread = non-zero): the lanes of a wave with the same
//                                digit find each other by `digit_bits` ballots, rank = the lower lanes among them, the waves of a tile
//                                are added in wave order, the tiles in tile order: equal digits keep their order.
//           The first pass reads the handle's own orientation (index, value) and the line numbers, the last one writes line numbers and
//           values straight into the handle's other orientation and the sorted indices into the workspace.
//   ptr     the other orientation's pointers: one lower bound per line over the sorted indices (no atomics).
// Values move as 64-bit patterns (float32 is widened once, in the register it was loaded into); there is no floating-point arithmetic
// and no floating-point atomic: two calls give the same arrays.  The cost follows nnz and the pass count (1 pass up to 2048 target
// lines, 2 up to 2^22, 3 beyond), not the aspect ratio, and a full line is 'per'-sized pieces like any other run of non-zeros.
#include "ctx.hpp"
#include "logistic.hpp"

#include <vector>

namespace oemgpu {

namespace {

constexpr int SB_NT = 256, SB_NW = SB_NT / 64;          // threads / waves of a workgroup; a tile is SB_NT non-zeros
constexpr int SB_MAX_DIGIT_BITS = 11, SB_MAX_BINS = 1 << SB_MAX_DIGIT_BITS;
constexpr int64_t SB_PER_MIN = 8 * SB_NT;               // a workgroup's share is a multiple of 8 tiles
enum { SB_E_PTR0 = 0, SB_E_PTRLAST = 1, SB_E_DECR = 2, SB_E_ENTRY = 3, SB_E_MAXLEN = 4, SB_E_WORDS = 8 };

struct SbPlan {
    int64_t T;          // target lines: the range of the indices
    int key_bits, passes, digit_bits, nwg;
    int64_t per;        // non-zeros per workgroup
    size_t a_err, a_line, a_skey, a_key[2], a_ln[2], a_val[2], a_tab, a_tot, ws_bytes;
    size_t h_cp, h_ri, h_v, h_rp, h_cc, h_cv, h_ch, handle_bytes;
};

SbPlan sb_plan(int64_t n, int p, int64_t nnz, int layout, int num_cu)
{
    SbPlan P;
    P.T = layout == OEMGPU_SPARSE_CSC ? n : (int64_t)p;
    P.key_bits = 0;
    while (P.key_bits < 63 && ((int64_t)1 << P.key_bits) < P.T) ++P.key_bits;       // bits of T - 1
    P.passes = (P.key_bits + SB_MAX_DIGIT_BITS - 1) / SB_MAX_DIGIT_BITS;
    if (P.passes < 1) P.passes = 1;
    P.digit_bits = (P.key_bits + P.passes - 1) / P.passes;
    if (P.digit_bits < 1) P.digit_bits = 1;
    const int64_t want = 4 * (int64_t)num_cu;                                        // four workgroups of 40 KB LDS to a CU
    int64_t per = (nnz + want - 1) / want;
    per = (per + SB_PER_MIN - 1) / SB_PER_MIN * SB_PER_MIN;
    if (per < SB_PER_MIN) per = SB_PER_MIN;
    P.per = per;
    P.nwg = (int)((nnz + per - 1) / per);
    if (P.nwg < 1) P.nwg = 1;
    const size_t ne = (size_t)nnz + 1, nbins = (size_t)1 << P.digit_bits;
    Bump W;
    P.a_err = W.take(8 * SB_E_WORDS);
    P.a_line = W.take(4 * ne);
    P.a_skey = W.take(4 * ne);
    for (int b = 0; b < 2; ++b) {                        // ping (two passes or more), pong (three)
        const bool have = P.passes >= b + 2;
        P.a_key[b] = W.take(have ? 4 * ne : 0); P.a_ln[b] = W.take(have ? 4 * ne : 0); P.a_val[b] = W.take(have ? 8 * ne : 0);
    }
    P.a_tab = W.take(4 * nbins * (size_t)P.nwg);
    P.a_tot = W.take(4 * nbins);
    P.ws_bytes = W.off;
    Bump B;                                              // the handle: sparse_x_build's regions, in its order
    P.h_cp = B.take(8 * (size_t)(p + 1)); P.h_ri = B.take(4 * ne); P.h_v = B.take(8 * ne);
    P.h_rp = B.take(8 * (size_t)(n + 1)); P.h_cc = B.take(4 * ne); P.h_cv = B.take(8 * ne);
    P.h_ch = B.take(4 * (size_t)(csc_chunks(n) + 1) * p);
    P.handle_bytes = B.off;
    return P;
}

// ---------------------------------------------------------------------------------------------------- check and widen
template <typename PT>
__global__ __launch_bounds__(256) void sb_ptr_kernel(const PT *__restrict__ ptr, int64_t nline, int64_t nnz, int64_t *__restrict__ out,
                                                     unsigned long long *__restrict__ err)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j > nline) return;
    const int64_t v = (int64_t)ptr[j];
    out[j] = v;
    if (j == 0 && v != 0) err[SB_E_PTR0] = 1ull;
    if (j == nline && v != nnz) err[SB_E_PTRLAST] = 1ull;
    if (j < nline && (int64_t)ptr[j + 1] < v) atomicMin(&err[SB_E_DECR], (unsigned long long)j);
}

// ptr: the handle's checked pointers (ptr[0] = 0, non-decreasing, ptr[nline] = nnz), so every search ends inside [1, nline]
template <typename IT, typename VT>
__global__ __launch_bounds__(256) void sb_entry_kernel(const int64_t *__restrict__ ptr, int64_t nline, const IT *__restrict__ idx,
                                                       const VT *__restrict__ val, int64_t nnz, int64_t T, int32_t *__restrict__ oidx,
                                                       unsigned long long *__restrict__ oval, int32_t *__restrict__ line,
                                                       unsigned long long *__restrict__ err)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nnz) return;
    int64_t lo = 0, hi = nline;                          // the first pointer beyond k; the line is the one before it
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (ptr[mid] <= k) lo = mid + 1; else hi = mid; }
    const int64_t j = lo > 0 ? lo - 1 : 0;
    const int64_t i = (int64_t)idx[k];
    const bool outside = i < 0 || i >= T;
    if (outside) atomicMin(&err[SB_E_ENTRY], 2ull * (unsigned long long)k);
    else if (k > ptr[j] && (int64_t)idx[k - 1] >= i) atomicMin(&err[SB_E_ENTRY], 2ull * (unsigned long long)k + 1ull);
    oidx[k] = outside ? 0 : (int32_t)i;
    if constexpr (sizeof(VT) == 8) oval[k] = reinterpret_cast<const unsigned long long *>(val)[k];
    else oval[k] = (unsigned long long)__double_as_longlong((double)val[k]);
    line[k] = (int32_t)j;
}

// ---------------------------------------------------------------------------------------------------- a pass of the sort
__global__ __launch_bounds__(SB_NT) void sb_hist_kernel(const int32_t *__restrict__ key, int64_t nnz, int64_t per, int shift, int nbins, int nwg,
                                                        uint32_t *__restrict__ tab)
{
    __shared__ uint32_t h[SB_MAX_BINS];
    const int tid = threadIdx.x;
    for (int d = tid; d < nbins; d += SB_NT) h[d] = 0u;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < nnz ? lo + per : nnz;
    for (int64_t k = lo + tid; k < hi; k += SB_NT) atomicAdd(&h[((uint32_t)key[k] >> shift) & (uint32_t)(nbins - 1)], 1u);
    __syncthreads();
    for (int d = tid; d < nbins; d += SB_NT) tab[(size_t)d * nwg + blockIdx.x] = h[d];
}

// a wave per digit: tab[d][w] -> the non-zeros of digit d in the workgroups before w; tot[d] = all of them
__global__ __launch_bounds__(SB_NT) void sb_scan_wg_kernel(uint32_t *__restrict__ tab, int nbins, int nwg, uint32_t *__restrict__ tot)
{
    const int lane = threadIdx.x & 63, d = blockIdx.x * SB_NW + (threadIdx.x >> 6);
    if (d >= nbins) return;                              // (the whole wave)
    uint32_t *row = tab + (size_t)d * nwg;
    uint32_t run = 0u;
    for (int base = 0; base < nwg; base += 64) {
        const int w = base + lane;
        const uint32_t v = w < nwg ? row[w] : 0u;
        uint32_t inc = v;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
        if (w < nwg) row[w] = run + inc - v;
        run += __shfl(inc, 63, 64);
    }
    if (lane == 0) tot[d] = run;
}

// one workgroup: tot[d] -> the non-zeros of the digits before d
__global__ __launch_bounds__(SB_NT) void sb_scan_bins_kernel(uint32_t *__restrict__ tot, int nbins)
{
    __shared__ uint32_t part[SB_NT];
    const int tid = threadIdx.x, per = (nbins + SB_NT - 1) / SB_NT;
    const int lo = tid * per < nbins ? tid * per : nbins, hi = lo + per < nbins ? lo + per : nbins;
    uint32_t s = 0u;
    for (int d = lo; d < hi; ++d) s += tot[d];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0u;
        for (int t = 0; t < SB_NT; ++t) { const uint32_t v = part[t]; part[t] = run; run += v; }
    }
    __syncthreads();
    uint32_t run = part[tid];
    for (int d = lo; d < hi; ++d) { const uint32_t v = tot[d]; tot[d] = run; run += v; }
}

__global__ __launch_bounds__(SB_NT) void sb_scatter_kernel(const int32_t *__restrict__ skey, const int32_t *__restrict__ sline,
                                                           const unsigned long long *__restrict__ sval, int64_t nnz, int64_t per, int shift,
                                                           int digit_bits, int nwg, const uint32_t *__restrict__ tab,
                                                           const uint32_t *__restrict__ dbase, int32_t *__restrict__ dkey,
                                                           int32_t *__restrict__ dline, unsigned long long *__restrict__ dval)
{
    __shared__ uint32_t base[SB_MAX_BINS];               // where the next non-zero of a digit goes
    __shared__ uint32_t cnt[SB_NW][SB_MAX_BINS];         // a tile's non-zeros per (wave, digit); zero between tiles
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, nbins = 1 << digit_bits;
    for (int d = tid; d < nbins; d += SB_NT) {
        base[d] = dbase[d] + tab[(size_t)d * nwg + blockIdx.x];
        for (int v = 0; v < SB_NW; ++v) cnt[v][d] = 0u;
    }
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < nnz ? lo + per : nnz;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int64_t t0 = lo; t0 < hi; t0 += SB_NT) {        // (uniform: every thread of the workgroup meets every barrier)
        const int64_t k = t0 + tid;
        const bool valid = k < hi;
        const int32_t key = valid ? skey[k] : 0;
        const int d = (int)(((uint32_t)key >> shift) & (uint32_t)(nbins - 1));
        unsigned long long m = __ballot(valid);
        for (int b = 0; b < digit_bits; ++b) {
            const bool bit = (d >> b) & 1;
            const unsigned long long bb = __ballot(valid && bit);
            m &= bit ? bb : ~bb;
        }
        const uint32_t rank = (uint32_t)__popcll(m & lt), c = (uint32_t)__popcll(m);
        const bool leader = valid && rank == 0u;
        if (leader) cnt[w][d] = c;
        __syncthreads();
        uint32_t pos = 0u;
        if (valid) {
            pos = base[d] + rank;
            for (int v = 0; v < w; ++v) pos += cnt[v][d];
        }
        __syncthreads();                                 // every place is read before the bases move on
        if (leader) { atomicAdd(&base[d], c); cnt[w][d] = 0u; }
        if (valid && (int64_t)pos < nnz) { dkey[pos] = key; dline[pos] = sline[k]; dval[pos] = sval[k]; }
    }
}

// the pointers of the sorted orientation: tptr[t] = the first sorted index >= t, t = 0 .. T
__global__ __launch_bounds__(256) void sb_lower_bound_kernel(const int32_t *__restrict__ skey, int64_t nnz, int64_t T, int64_t *__restrict__ tptr)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > T) return;
    int64_t lo = 0, hi = nnz;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if ((int64_t)skey[mid] < t) lo = mid + 1; else hi = mid; }
    tptr[t] = lo;
}

// the longest column (an integer maximum: a wave's own first, then one atomic a wave)
__global__ __launch_bounds__(256) void sb_maxlen_kernel(const int64_t *__restrict__ colptr, int p, unsigned long long *__restrict__ err)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long len = j < p ? (unsigned long long)(colptr[j + 1] - colptr[j]) : 0ull;
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(len, o, 64); if (t > len) len = t; }
    if ((threadIdx.x & 63) == 0 && len > 0ull) atomicMax(&err[SB_E_MAXLEN], len);
}

// HIP-event times of the last oemgpu_sparse_x_create_dev of this thread: check and widen, the sort passes, pointers / chunk pointers / maxcol
thread_local double g_sb_ms[3] = {0.0, 0.0, 0.0};

unsigned blocks_of(int64_t items) { return (unsigned)((items + 255) / 256); }

template <typename IT>
int sb_launch_entry(hipStream_t s, const int64_t *ptr, int64_t nline, const IT *idx, const void *val, int val_dtype, int64_t nnz, int64_t T,
                    int32_t *oidx, double *oval, int32_t *line, unsigned long long *err)
{
    unsigned long long *ov = reinterpret_cast<unsigned long long *>(oval);
    if (val_dtype == OEMGPU_F32)
        hipLaunchKernelGGL((sb_entry_kernel<IT, float>), dim3(blocks_of(nnz)), dim3(256), 0, s, ptr, nline, idx, (const float *)val, nnz, T, oidx, ov, line, err);
    else
        hipLaunchKernelGGL((sb_entry_kernel<IT, double>), dim3(blocks_of(nnz)), dim3(256), 0, s, ptr, nline, idx, (const double *)val, nnz, T, oidx, ov, line, err);
    OEM_HIP(hipGetLastError());
    return 0;
}

}  // namespace

}  // namespace oemgpu

using namespace oemgpu;

extern "C" {
#pragma GCC visibility push(default)

int oemgpu_selftest_sparse_build_plan(int64_t n, int32_t p, int64_t nnz, int32_t layout, int32_t num_cu, int64_t *out)
{
    static const char *who = "selftest_sparse_build_plan";
    if (n < 1 || p < 1 || nnz < 0 || num_cu < 1 || !out) { set_error("%s: bad argument", who); return OEMGPU_ERR_ARG; }
    if (layout != OEMGPU_SPARSE_CSC && layout != OEMGPU_SPARSE_CSR) { set_error("%s: layout must be OEMGPU_SPARSE_CSC or OEMGPU_SPARSE_CSR", who); return OEMGPU_ERR_ARG; }
    if (n >= (int64_t)1 << 31 || nnz >= (int64_t)1 << 31) { set_error("%s: n >= 2^31 or nnz >= 2^31 is not supported", who); return OEMGPU_ERR_UNSUPPORTED; }
    const SbPlan P = sb_plan(n, p, nnz, layout, num_cu);
    out[0] = P.passes; out[1] = P.digit_bits; out[2] = P.nwg; out[3] = (int64_t)P.ws_bytes; out[4] = (int64_t)P.handle_bytes; out[5] = P.per;
    out[6] = P.key_bits; out[7] = P.T;
    return 0;
}

int oemgpu_sparse_x_create_dev(oemgpu_ctx *c, int64_t n, int32_t p, int32_t layout, const void *ptr_dev, int32_t ptr_dtype, const void *idx_dev,
                               int32_t idx_dtype, const void *val_dev, int32_t val_dtype, int64_t nnz, oemgpu_sparse_x **out)
{
    static const char *who = "sparse_x_create_dev";
    if (out) *out = nullptr;
    if (!c || !ptr_dev || !out) { set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG; }
    if (layout != OEMGPU_SPARSE_CSC && layout != OEMGPU_SPARSE_CSR) { set_error("%s: layout must be OEMGPU_SPARSE_CSC or OEMGPU_SPARSE_CSR", who); return OEMGPU_ERR_ARG; }
    if ((ptr_dtype != OEMGPU_I32 && ptr_dtype != OEMGPU_I64) || (idx_dtype != OEMGPU_I32 && idx_dtype != OEMGPU_I64)) {
        set_error("%s: pointer and index dtypes must be OEMGPU_I32 or OEMGPU_I64", who); return OEMGPU_ERR_ARG;
    }
    if (val_dtype != OEMGPU_F64 && val_dtype != OEMGPU_F32) { set_error("%s: the value dtype must be OEMGPU_F64 or OEMGPU_F32", who); return OEMGPU_ERR_ARG; }
    if (n < 1 || p < 1 || nnz < 0) { set_error("%s: bad dimensions", who); return OEMGPU_ERR_ARG; }
    const bool csc = layout == OEMGPU_SPARSE_CSC;
    if (nnz > 0 && (!idx_dev || !val_dev)) { set_error("%s: NULL %s indices or values", who, csc ? "row" : "column"); return OEMGPU_ERR_ARG; }
    if (n >= (int64_t)1 << 31) { set_error("%s: n >= 2^31 is not supported (32-bit row indices)", who); return OEMGPU_ERR_UNSUPPORTED; }
    if (nnz >= (int64_t)1 << 31) { set_error("%s: nnz >= 2^31 is not supported (32-bit positions)", who); return OEMGPU_ERR_UNSUPPORTED; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const SbPlan P = sb_plan(n, p, nnz, layout, c->num_cu);
    if (ctx_reserve(c, P.ws_bytes)) return OEMGPU_ERR_HIP;
    oemgpu_sparse_x *x = new oemgpu_sparse_x;
    x->device = c->device; x->n = n; x->p = p; x->nnz = nnz; x->maxcol = 0; x->bytes = P.handle_bytes;
    if (hipMalloc((void **)&x->base, P.handle_bytes) != hipSuccess) {
        set_error("%s: cannot allocate %zu bytes of device memory", who, P.handle_bytes);
        delete x;
        return OEMGPU_ERR_HIP;
    }
    g_alloc_count += 1;
    x->colptr = (int64_t *)(x->base + P.h_cp); x->rowidx = (int32_t *)(x->base + P.h_ri); x->val = (double *)(x->base + P.h_v);
    x->rowptr = (int64_t *)(x->base + P.h_rp); x->ccol = (int32_t *)(x->base + P.h_cc); x->cval = (double *)(x->base + P.h_cv);
    x->cptr = (int32_t *)(x->base + P.h_ch);
    hipStream_t s = c->stream;
    char *ws = c->ws;
    unsigned long long *err = (unsigned long long *)(ws + P.a_err);
    int32_t *line0 = (int32_t *)(ws + P.a_line), *skey = (int32_t *)(ws + P.a_skey);
    uint32_t *tab = (uint32_t *)(ws + P.a_tab), *tot = (uint32_t *)(ws + P.a_tot);
    // the input's own orientation and the other one
    const int64_t nline = csc ? (int64_t)p : n, T = P.T;
    int64_t *optr = csc ? x->colptr : x->rowptr, *tptr = csc ? x->rowptr : x->colptr;
    int32_t *oidx = csc ? x->rowidx : x->ccol, *tidx = csc ? x->ccol : x->rowidx;
    double *oval = csc ? x->val : x->cval, *tval = csc ? x->cval : x->val;
    const char *pname = csc ? "colptr" : "rowptr", *lname = csc ? "column" : "row", *iname = csc ? "row" : "column";

    if (!c->xvs_ev_made) {
        for (int i = 0; i <= OEMGPU_XVS_NPHASES; ++i) OEM_HIP(hipEventCreate(&c->xvs_ev[i]));
        c->xvs_ev_made = true;
    }
    for (double &v : g_sb_ms) v = 0.0;
    auto build = [&]() -> int {
        unsigned long long h[SB_E_WORDS] = {0ull, 0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull, 0ull};
        (void)hipEventRecord(c->xvs_ev[0], s);
        OEM_HIP(hipMemcpyAsync(err, h, sizeof(h), hipMemcpyHostToDevice, s));
        if (ptr_dtype == OEMGPU_I32)
            hipLaunchKernelGGL(sb_ptr_kernel<int32_t>, dim3(blocks_of(nline + 1)), dim3(256), 0, s, (const int32_t *)ptr_dev, nline, nnz, optr, err);
        else
            hipLaunchKernelGGL(sb_ptr_kernel<int64_t>, dim3(blocks_of(nline + 1)), dim3(256), 0, s, (const int64_t *)ptr_dev, nline, nnz, optr, err);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipMemcpyAsync(h, err, sizeof(h), hipMemcpyDeviceToHost, s));
        OEM_HIP(hipStreamSynchronize(s));
        if (h[SB_E_PTR0]) { set_error("%s: %s[0] must be 0", who, pname); return OEMGPU_ERR_ARG; }
        if (h[SB_E_PTRLAST]) { set_error("%s: %s[%s] must be nnz", who, pname, csc ? "p" : "n"); return OEMGPU_ERR_ARG; }
        if (h[SB_E_DECR] != ~0ull) { set_error("%s: %s must be non-decreasing", who, pname); return OEMGPU_ERR_ARG; }
        if (nnz == 0) {
            OEM_HIP(hipMemsetAsync(tptr, 0, 8 * (size_t)(T + 1), s));
        } else {
            int rc = idx_dtype == OEMGPU_I32
                ? sb_launch_entry<int32_t>(s, optr, nline, (const int32_t *)idx_dev, val_dev, val_dtype, nnz, T, oidx, oval, line0, err)
                : sb_launch_entry<int64_t>(s, optr, nline, (const int64_t *)idx_dev, val_dev, val_dtype, nnz, T, oidx, oval, line0, err);
            if (rc) return rc;
            OEM_HIP(hipMemcpyAsync(h, err, sizeof(h), hipMemcpyDeviceToHost, s));
            OEM_HIP(hipStreamSynchronize(s));
            if (h[SB_E_ENTRY] != ~0ull) {
                const int64_t k = (int64_t)(h[SB_E_ENTRY] >> 1);
                int32_t j = 0;
                long long i = 0;
                OEM_HIP(hipMemcpy(&j, line0 + k, sizeof(j), hipMemcpyDeviceToHost));
                if (idx_dtype == OEMGPU_I32) { int32_t v = 0; OEM_HIP(hipMemcpy(&v, (const int32_t *)idx_dev + k, sizeof(v), hipMemcpyDeviceToHost)); i = v; }
                else { int64_t v = 0; OEM_HIP(hipMemcpy(&v, (const int64_t *)idx_dev + k, sizeof(v), hipMemcpyDeviceToHost)); i = v; }
                if (h[SB_E_ENTRY] & 1ull) set_error("%s: %s indices of %s %d are not strictly increasing", who, iname, lname, (int)j);
                else set_error("%s: %s index %lld of %s %d outside [0, %s)", who, iname, i, lname, (int)j, csc ? "n" : "p");
                return OEMGPU_ERR_ARG;
            }
            // ---- the stable sort by index: (oidx, line0, oval) -> ... -> (skey, tidx, tval)
            (void)hipEventRecord(c->xvs_ev[1], s);
            const int nbins = 1 << P.digit_bits;
            const int32_t *sk = oidx, *sl = line0;
            const unsigned long long *sv = reinterpret_cast<const unsigned long long *>(oval);
            for (int pass = 0; pass < P.passes; ++pass) {
                const bool last = pass + 1 == P.passes;
                const int b = pass & 1;
                int32_t *dk = last ? skey : (int32_t *)(ws + P.a_key[b]), *dl = last ? tidx : (int32_t *)(ws + P.a_ln[b]);
                unsigned long long *dv = last ? reinterpret_cast<unsigned long long *>(tval) : (unsigned long long *)(ws + P.a_val[b]);
                const int shift = pass * P.digit_bits;
                hipLaunchKernelGGL(sb_hist_kernel, dim3(P.nwg), dim3(SB_NT), 0, s, sk, nnz, P.per, shift, nbins, P.nwg, tab);
                hipLaunchKernelGGL(sb_scan_wg_kernel, dim3((nbins + SB_NW - 1) / SB_NW), dim3(SB_NT), 0, s, tab, nbins, P.nwg, tot);
                hipLaunchKernelGGL(sb_scan_bins_kernel, dim3(1), dim3(SB_NT), 0, s, tot, nbins);
                hipLaunchKernelGGL(sb_scatter_kernel, dim3(P.nwg), dim3(SB_NT), 0, s, sk, sl, sv, nnz, P.per, shift, P.digit_bits, P.nwg, tab, tot, dk, dl, dv);
                OEM_HIP(hipGetLastError());
                sk = dk; sl = dl; sv = dv;
            }
            (void)hipEventRecord(c->xvs_ev[2], s);
            hipLaunchKernelGGL(sb_lower_bound_kernel, dim3(blocks_of(T + 1)), dim3(256), 0, s, skey, nnz, T, tptr);
            OEM_HIP(hipGetLastError());
        }
        int rc = launch_csc_chunk_ptr(s, x->colptr, x->rowidx, n, p, x->cptr);
        if (rc) return rc;
        hipLaunchKernelGGL(sb_maxlen_kernel, dim3(blocks_of(p)), dim3(256), 0, s, x->colptr, (int)p, err);
        OEM_HIP(hipGetLastError());
        (void)hipEventRecord(c->xvs_ev[3], s);
        OEM_HIP(hipMemcpyAsync(h, err, sizeof(h), hipMemcpyDeviceToHost, s));
        OEM_HIP(hipStreamSynchronize(s));                    // the caller's arrays may go once this returns
        x->maxcol = (int64_t)h[SB_E_MAXLEN];
        if (nnz > 0)
            for (int i = 0; i < 3; ++i) {
                float f = 0.f;
                if (hipEventElapsedTime(&f, c->xvs_ev[i], c->xvs_ev[i + 1]) == hipSuccess) g_sb_ms[i] = f;
            }
        return 0;
    };
    const int rc = build();
    if (rc) { (void)hipStreamSynchronize(s); (void)hipFree(x->base); delete x; return rc; }
    *out = x;
    return 0;
}

int oemgpu_last_sparse_build_timings(double *ms)
{
    if (!ms) { set_error("NULL argument"); return OEMGPU_ERR_ARG; }
    for (int i = 0; i < 3; ++i) ms[i] = g_sb_ms[i];
    return 0;
}

int oemgpu_sparse_x_dims(const oemgpu_sparse_x *x, int64_t *out)
{
    if (!x || !out) { set_error("sparse_x_dims: NULL argument"); return OEMGPU_ERR_ARG; }
    out[0] = x->n; out[1] = x->p; out[2] = x->nnz; out[3] = x->maxcol;
    return 0;
}

int oemgpu_sparse_x_export(const oemgpu_sparse_x *x, int64_t *colptr, int32_t *rowidx, double *val, int64_t *rowptr, int32_t *ccol, double *cval,
                           int32_t *cptr)
{
    if (!x) { set_error("sparse_x_export: NULL argument"); return OEMGPU_ERR_ARG; }
    int cur = 0;
    OEM_HIP(hipGetDevice(&cur));
    if (cur != x->device) OEM_HIP(hipSetDevice(x->device));
    auto copy = [&]() -> int {
        const size_t nz = (size_t)x->nnz;
        if (colptr) OEM_HIP(hipMemcpy(colptr, x->colptr, 8 * (size_t)(x->p + 1), hipMemcpyDeviceToHost));
        if (rowptr) OEM_HIP(hipMemcpy(rowptr, x->rowptr, 8 * (size_t)(x->n + 1), hipMemcpyDeviceToHost));
        if (cptr) OEM_HIP(hipMemcpy(cptr, x->cptr, 4 * (size_t)(csc_chunks(x->n) + 1) * (size_t)x->p, hipMemcpyDeviceToHost));
        if (nz > 0) {
            if (rowidx) OEM_HIP(hipMemcpy(rowidx, x->rowidx, 4 * nz, hipMemcpyDeviceToHost));
            if (val) OEM_HIP(hipMemcpy(val, x->val, 8 * nz, hipMemcpyDeviceToHost));
            if (ccol) OEM_HIP(hipMemcpy(ccol, x->ccol, 4 * nz, hipMemcpyDeviceToHost));
            if (cval) OEM_HIP(hipMemcpy(cval, x->cval, 8 * nz, hipMemcpyDeviceToHost));
        }
        return 0;
    };
    const int rc = copy();
    if (cur != x->device) (void)hipSetDevice(cur);
    return rc;
}

#pragma GCC visibility pop
}
