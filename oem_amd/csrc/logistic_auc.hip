// logistic_auc.hip -- the AUC of cv.oem for binomial fits on the device: what cv.oemfit_binomial (ref R/cv_oem.R:288-307) asks of auc.mat
// (R/utils.R:90-125) for every fold and column, without predmat leaving the device.  For fold f (its rows in row order) and column c:
// order the rows by prob ascending, TIES IN ROW ORDER (numpy's stable argsort: NaN behind every number, NaNs among themselves in row
// order; the reference draws runif for ties, so any order is one of its draws), y2 = (y == y_hi), and
//     n1[f] = rows with y2 = 1,  n0[f] = the rest,  u[f, c] = sum over the rows with y2 = 1 of the rows with y2 = 0 in front of it.
// Three integers per (fold, column): the device returns them exactly, the host keeps exp(log u - log n1 - log n0).
//
// perm, once per call: the rows of fold 1 in row order, then fold 2, ... -- a stable counting sort of the row numbers by foldid.  One
// wave per chunk of rows counts its folds in LDS (auc_fold_count_kernel), one workgroup scans the fold-major count table in chunk order
// (auc_fold_scan_kernel: off[K + 1] falls out of it), and the wave of a chunk scatters its rows, 64 at a time in row order, each
// distinct fold of the 64 by a ballot (auc_fold_scatter_kernel).  A fold id outside 1 .. K raises a flag that the host reads with off.
//
// One workgroup of 1024 per (fold, column) segment (auc_segment_kernel); no workgroup talks to another.
//   key     bits(prob) with the sign cleared (-0.0 is +0.0; a probability has none) and every NaN the one quiet NaN 0x7FF8 << 48: on
//           bits 0 .. 62 the unsigned order is numpy's.  Bit 63 carries y2 and is never sorted on, so there is no payload array.
//   gather  key[i] = key(predmat[c n + perm[off[f] + i]]); the histograms of all eight digits are taken in the same read (LDS integer
//           atomics; a wave whose 64 keys share a digit adds once).
//   sort    least-significant digit first, 8 bits a pass (the last pass 7).  A pass whose keys all share the digit is skipped (the
//           exponent bytes of probabilities usually do).  A pass: exclusive scan of its 256 bins, then tiles of 1024 keys (thread = key,
//           so lane and wave order are key order): the lanes of a wave with the same digit find each other by eight ballots, rank =
//           popcount of the lower lanes, the first of them writes the wave's count; thread d adds the 16 waves' counts of digit d in
//           wave order onto the bin's running base; key -> base of (wave, digit) + rank.  Equal digits keep their order: stable.
//   count   one pass over the sorted keys with the running number of y2 = 0 keys: u += zeros in front, for every y2 = 1 key.
// Two forms of the same kernel: a segment whose two key buffers fit in LDS beside the bins (AucPlan::lmax keys) never touches HBM
// after the gather; a longer one ping-pongs between two workspace buffers.  Columns go in batches that keep the workspace under
// AUC_WS_BYTES.  Plain stores, integer atomics in LDS only: two calls give the same integers.
#include "logistic.hpp"

#include <algorithm>
#include <vector>

namespace oemgpu {

static const size_t AUC_LDS_BYTES = (size_t)160 << 10;   // LDS of a gfx950 CU
static const size_t AUC_WS_BYTES = (size_t)256 << 20;    // key buffers of a batch of columns + perm (the bound of the binomial fit's Z blocks)
static const int AUC_NT = 1024, AUC_NW = AUC_NT / 64;    // threads / waves of a segment's workgroup; a tile is AUC_NT keys
static const int AUC_MAX_FOLDS = 4096;                   // a chunk's fold counters sit in LDS
static const int64_t AUC_MAX_CHUNKS = 1024;
// LDS beside the key buffers, in 4-byte words: hist 8 x 256, cnt and offs AUC_NW x 256 each, binbase 256, wz 2 x AUC_NW, skip 8 (+ 8 pad),
// then AUC_NW x 2 64-bit words of the closing sums
static const size_t AUC_AUX_BYTES = 4 * (size_t)(8 * 256 + 2 * AUC_NW * 256 + 256 + 2 * AUC_NW + 16) + 8 * 2 * (size_t)AUC_NW;

struct AucPlan {
    int64_t tile;      // keys per tile of a pass
    int64_t lmax;      // the longest segment sorted in LDS
    int cb;            // columns per batch
    int nbatch;
    size_t ws;         // workspace bytes: perm, the chunk counts, off, n1, and of a batch of columns u and (if a segment is longer than lmax) the key buffers
    size_t lds;        // dynamic LDS bytes of the largest launch
    bool hbm;          // the longest fold takes the HBM form
    int64_t chunk;     // rows per chunk of the counting sort (a multiple of 64)
    int64_t nchunk;
};

static AucPlan auc_plan(int64_t n, int nfolds, int ncol, int num_cu, int64_t longest_fold)
{
    (void)num_cu;      // a segment is one workgroup whatever the chip: K ncol of them fill it (kept in the signature for the next form)
    AucPlan P;
    P.tile = AUC_NT;
    P.lmax = (int64_t)((AUC_LDS_BYTES - AUC_AUX_BYTES) / 16);
    P.hbm = longest_fold > P.lmax;
    int64_t ch = (n + AUC_MAX_CHUNKS - 1) / AUC_MAX_CHUNKS;
    P.chunk = std::max<int64_t>(1024, (ch + 63) / 64 * 64);
    P.nchunk = (n + P.chunk - 1) / P.chunk;
    // what does not grow with the columns: perm, the chunk counts, off, n1, the granules.  A column of a batch adds its nfolds results
    // and, in the HBM form, its two key buffers -- so the columns the bound admits depend on n and nfolds alone, not on ncol
    const size_t fixed = 4 * (size_t)n + 4 * (size_t)nfolds * P.nchunk + 8 * ((size_t)nfolds + 2) + 8 * (size_t)nfolds + 5 * 256;
    const size_t per_col = 8 * (size_t)nfolds + (P.hbm ? 16 * (size_t)n : 0);
    if (P.hbm) {
        const size_t room = AUC_WS_BYTES > fixed ? AUC_WS_BYTES - fixed : 0;
        P.cb = (int)std::min<size_t>(std::max<size_t>(1, room / per_col), (size_t)std::min(ncol, 65535));
    } else {
        P.cb = std::min(ncol, 65535);
    }
    P.ws = fixed + per_col * P.cb;
    P.nbatch = (ncol + P.cb - 1) / P.cb;
    // the LDS form asks for the buffers of the longest segment it serves; the HBM form for the bins alone
    const int64_t lds_keys = std::min(std::max<int64_t>(longest_fold, 0), P.lmax);
    P.lds = AUC_AUX_BYTES + (P.hbm ? 16 * (size_t)P.lmax : 16 * (size_t)lds_keys);
    return P;
}

namespace {

// ---------------------------------------------------------------------------------------------------- perm: rows in fold order
// cnt: fold-major, cnt[k nchunk + c] = rows of fold k + 1 in chunk c
__global__ __launch_bounds__(64) void auc_fold_count_kernel(const int32_t *__restrict__ foldid, int64_t n, int K, int64_t chunk, int64_t nchunk,
                                                            uint32_t *__restrict__ cnt, int32_t *__restrict__ bad)
{
    extern __shared__ uint32_t fh[];
    const int lane = threadIdx.x;
    for (int k = lane; k < K; k += 64) fh[k] = 0u;
    __syncthreads();
    const int64_t r_lo = (int64_t)blockIdx.x * chunk, r_hi = (r_lo + chunk < n) ? r_lo + chunk : n;
    bool b = false;
    for (int64_t r = r_lo + lane; r < r_hi; r += 64) {
        const int32_t f = foldid[r];
        if (f < 1 || f > K) b = true;
        else atomicAdd(&fh[f - 1], 1u);
    }
    __syncthreads();
    for (int k = lane; k < K; k += 64) cnt[(size_t)k * nchunk + blockIdx.x] = fh[k];
    if (b) *bad = 1;
}

// in place: cnt[i] -> the sum of the entries in front of it; off[k] = where fold k + 1 starts, off[K] = the rows with a fold
__global__ __launch_bounds__(1024) void auc_fold_scan_kernel(uint32_t *__restrict__ cnt, int64_t total, int64_t nchunk, int K, int64_t *__restrict__ off)
{
    __shared__ unsigned long long part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (total + 1023) / 1024, lo = std::min<int64_t>(total, tid * per), hi = std::min<int64_t>(total, lo + per);
    unsigned long long s = 0;
    for (int64_t i = lo; i < hi; ++i) s += cnt[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < 1024; ++t) { const unsigned long long v = part[t]; part[t] = run; run += v; }
        off[K] = (int64_t)run;
    }
    __syncthreads();
    unsigned long long run = part[tid];
    for (int64_t i = lo; i < hi; ++i) {
        const uint32_t v = cnt[i];
        cnt[i] = (uint32_t)run;
        if (i % nchunk == 0) off[i / nchunk] = (int64_t)run;
        run += v;
    }
}

// the wave of chunk c walks its rows 64 at a time; the rows of one fold among the 64 take consecutive places in row (= lane) order
__global__ __launch_bounds__(64) void auc_fold_scatter_kernel(const int32_t *__restrict__ foldid, int64_t n, int K, int64_t chunk, int64_t nchunk,
                                                              const uint32_t *__restrict__ cnt, int32_t *__restrict__ perm)
{
    extern __shared__ uint32_t fbase[];                  // (another lane moves a base between two reads of this one: the barriers below)
    const int lane = threadIdx.x;
    for (int k = lane; k < K; k += 64) fbase[k] = cnt[(size_t)k * nchunk + blockIdx.x];
    __syncthreads();
    const int64_t r_lo = (int64_t)blockIdx.x * chunk, r_hi = (r_lo + chunk < n) ? r_lo + chunk : n;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int64_t r0 = r_lo; r0 < r_hi; r0 += 64) {
        const int64_t r = r0 + lane;
        int32_t f = (r < r_hi) ? foldid[r] : 0;
        if (f < 1 || f > K) f = 0;                       // (a bad id: the call fails on the flag of the count kernel)
        unsigned long long todo = __ballot(f != 0);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            const int32_t v = __shfl(f, src, 64);
            const unsigned long long m = __ballot(f == v);
            if (f == v) perm[fbase[v - 1] + (uint32_t)__popcll(m & lt)] = (int32_t)r;
            __syncthreads();                             // (one wave: orders the group's reads before the base moves on)
            if (lane == src) fbase[v - 1] = fbase[v - 1] + (uint32_t)__popcll(m);
            __syncthreads();
            todo &= ~m;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- a segment: key, sort, count
__device__ __forceinline__ unsigned long long auc_key(double prob, bool one)
{
    unsigned long long b = (unsigned long long)__double_as_longlong(prob) & 0x7FFFFFFFFFFFFFFFull;   // -0.0 -> +0.0
    if (prob != prob) b = 0x7FF8000000000000ull;                                                      // every NaN the one quiet NaN
    return b | (one ? 0x8000000000000000ull : 0ull);
}

__device__ __forceinline__ int auc_digit(unsigned long long key, int pass)
{
    return (int)(key >> (8 * pass)) & (pass == 7 ? 0x7F : 0xFF);
}

// grid (K, columns of the batch).  pred: column 0 of the batch; ws: 2 x cb x n keys (HBM form); u: the batch's
// nfolds x ncol table (ncol = columns of the batch); n1: written by the workgroups of the call's first column only (n1 != null)
template <bool INLDS>
__global__ __launch_bounds__(AUC_NT) void auc_segment_kernel(const double *__restrict__ pred, int64_t n, const double *__restrict__ y, double y_hi,
                                                             const int32_t *__restrict__ perm, const int64_t *__restrict__ off, int64_t lmax,
                                                             int64_t cap, unsigned long long *__restrict__ ws, int cb, int64_t *__restrict__ u,
                                                             int ncol, int64_t *__restrict__ n1)
{
    extern __shared__ unsigned long long lsh[];
    const int f = blockIdx.x, j = blockIdx.y;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int64_t o = off[f];
    const int64_t len64 = off[f + 1] - o;
    if (INLDS ? len64 > lmax : len64 <= lmax) return;    // the other form's segment (the same for the whole workgroup)
    const uint32_t len = (uint32_t)len64;
    uint32_t *hist = reinterpret_cast<uint32_t *>(lsh);  // 8 x 256: bin counts of every digit
    uint32_t *cnt = hist + 8 * 256;                      // AUC_NW x 256: a tile's keys per (wave, digit); zero between tiles
    uint32_t *offs = cnt + AUC_NW * 256;                 // AUC_NW x 256: where the keys of (wave, digit) of this tile go
    uint32_t *binbase = offs + AUC_NW * 256;             // 256: where the next key of a digit goes
    uint32_t *wz = binbase + 256;                        // 2 x AUC_NW: y2 = 0 keys per wave of a tile of the closing pass
    uint32_t *skip = wz + 2 * AUC_NW;                    // 8 (+ 8 pad): the pass would move nothing
    unsigned long long *red = reinterpret_cast<unsigned long long *>(skip + 16);   // 2 x AUC_NW
    unsigned long long *src, *dst;
    if (INLDS) {
        src = red + 2 * AUC_NW;
        dst = src + cap;
    } else {
        src = ws + (size_t)j * n + o;
        dst = ws + ((size_t)cb + j) * n + o;
    }
    for (int k = tid; k < 8 * 256 + AUC_NW * 256; k += AUC_NT) hist[k] = 0u;   // hist and cnt
    if (tid < 16) skip[tid] = 0u;
    __syncthreads();
    // ---- gather, key, histograms
    const double *pc = pred + (size_t)j * n;
    for (uint32_t i0 = 0; i0 < len; i0 += AUC_NT) {
        const uint32_t i = i0 + tid;
        const bool in = i < len;
        unsigned long long key = 0ull;
        if (in) {
            const int32_t row = perm[o + i];
            key = auc_key(pc[row], y[row] == y_hi);
            src[i] = key;
        }
        const unsigned long long act = __ballot(in);
        if (act == 0ull) continue;
        const int first = __ffsll((long long)act) - 1;
#pragma unroll
        for (int ps = 0; ps < 8; ++ps) {
            const int d = auc_digit(key, ps);
            const int d0 = __shfl(d, first, 64);
            if (__ballot(in && d == d0) == act) {        // the wave's keys share the digit: one add
                if (lane == first) atomicAdd(&hist[ps * 256 + d0], (uint32_t)__popcll(act));
            } else if (in) {
                atomicAdd(&hist[ps * 256 + d], 1u);
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < 8 * 256; k += AUC_NT)
        if (hist[k] == len) skip[k >> 8] = 1u;           // (len >= 1 here or the bins are all 0 == len: an empty segment skips every pass)
    __syncthreads();
    // ---- the passes
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int ps = 0; ps < 8; ++ps) {
        if (skip[ps]) continue;
        if (tid < 256) {
            uint32_t run = 0u;
            for (int k = 0; k < tid; ++k) run += hist[ps * 256 + k];
            binbase[tid] = run;
        }
        __syncthreads();
        for (uint32_t i0 = 0; i0 < len; i0 += AUC_NT) {
            const uint32_t i = i0 + tid;
            const bool in = i < len;
            const unsigned long long key = in ? src[i] : 0ull;
            const int d = in ? auc_digit(key, ps) : 0;
            unsigned long long m = __ballot(in);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (d >> b) & 1;
                const unsigned long long bb = __ballot(bit);
                m &= bit ? bb : ~bb;
            }
            const uint32_t rank = (uint32_t)__popcll(m & lt);
            if (in && rank == 0u) cnt[w * 256 + d] = (uint32_t)__popcll(m);
            __syncthreads();
            if (tid < 256) {
                uint32_t run = binbase[tid];
#pragma unroll
                for (int ww = 0; ww < AUC_NW; ++ww) {
                    const uint32_t c = cnt[ww * 256 + tid];
                    offs[ww * 256 + tid] = run;
                    cnt[ww * 256 + tid] = 0u;
                    run += c;
                }
                binbase[tid] = run;
            }
            __syncthreads();
            if (in) dst[offs[w * 256 + d] + rank] = key;
        }
        __syncthreads();
        unsigned long long *t = src; src = dst; dst = t;
    }
    // ---- u from the sorted keys
    unsigned long long uacc = 0ull, ones = 0ull;
    uint32_t zbase = 0u;
    int buf = 0;
    for (uint32_t i0 = 0; i0 < len; i0 += AUC_NT, buf ^= 1) {
        const uint32_t i = i0 + tid;
        const bool in = i < len;
        const unsigned long long key = in ? src[i] : 0ull;
        const bool one = in && (key >> 63) != 0ull;
        const unsigned long long mz = __ballot(in && !one);
        if (lane == 0) wz[buf * AUC_NW + w] = (uint32_t)__popcll(mz);
        __syncthreads();
        uint32_t before = zbase, all = 0u;
#pragma unroll
        for (int ww = 0; ww < AUC_NW; ++ww) {
            const uint32_t c = wz[buf * AUC_NW + ww];
            if (ww < w) before += c;
            all += c;
        }
        if (one) { uacc += (unsigned long long)(before + (uint32_t)__popcll(mz & lt)); ones += 1ull; }
        zbase += all;
    }
    for (int sh = 32; sh > 0; sh >>= 1) {
        uacc += __shfl_xor(uacc, sh, 64);
        ones += __shfl_xor(ones, sh, 64);
    }
    if (lane == 0) { red[2 * w] = uacc; red[2 * w + 1] = ones; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long a = 0ull, b = 0ull;
        for (int ww = 0; ww < AUC_NW; ++ww) { a += red[2 * ww]; b += red[2 * ww + 1]; }
        u[(size_t)f * ncol + j] = (int64_t)a;
        if (n1 && j == 0) n1[f] = (int64_t)b;
    }
}

}  // namespace

static int logistic_cv_auc_run(oemgpu_ctx *c, const double *pred, int64_t n, int32_t ncol, const double *y, double y_hi, const int32_t *foldid,
                               int32_t nfolds, int64_t *u, int64_t *n1, int64_t *n0)
{
    hipStream_t s = c->stream;
    const int K = nfolds;
    // the counting sort does not depend on the longest fold; the plan is made again once the folds are known
    AucPlan P = auc_plan(n, K, ncol, c->num_cu, 0);
    const int64_t chunk = P.chunk, nchunk = P.nchunk;
    Bump B;
    const size_t a_perm = B.take(4 * (size_t)n), a_cnt = B.take(4 * (size_t)K * nchunk), a_off = B.take(8 * ((size_t)K + 2));
    ctx_void_cv(c);
    if (ctx_grow(c, &c->aux, &c->aux_bytes, B.off)) return OEMGPU_ERR_HIP;
    {
        int32_t *perm = (int32_t *)(c->aux + a_perm);
        uint32_t *cnt = (uint32_t *)(c->aux + a_cnt);
        int64_t *off = (int64_t *)(c->aux + a_off);
        int32_t *bad = (int32_t *)(off + K + 1);
        OEM_HIP(hipMemsetAsync(bad, 0, 8, s));
        hipLaunchKernelGGL(auc_fold_count_kernel, dim3((unsigned)nchunk), dim3(64), 4 * (size_t)K, s, foldid, n, K, chunk, nchunk, cnt, bad);
        hipLaunchKernelGGL(auc_fold_scan_kernel, dim3(1), dim3(1024), 0, s, cnt, (int64_t)K * nchunk, nchunk, K, off);
        hipLaunchKernelGGL(auc_fold_scatter_kernel, dim3((unsigned)nchunk), dim3(64), 4 * (size_t)K, s, foldid, n, K, chunk, nchunk, cnt, perm);
        OEM_HIP(hipGetLastError());
    }
    std::vector<int64_t> hoff((size_t)K + 2);
    OEM_HIP(hipMemcpyAsync(hoff.data(), c->aux + a_off, 8 * hoff.size(), hipMemcpyDeviceToHost, s));
    OEM_HIP(hipStreamSynchronize(s));
    if ((int32_t)hoff[(size_t)K + 1] != 0 || hoff[K] != n) { set_error("logistic_cv_auc: a fold id is outside [1, nfolds]"); return OEMGPU_ERR_ARG; }
    int64_t longest = 0, shortest = n;
    for (int f = 0; f < K; ++f) {
        longest = std::max(longest, hoff[f + 1] - hoff[f]);
        shortest = std::min(shortest, hoff[f + 1] - hoff[f]);
    }
    if (longest >= ((int64_t)1 << 31)) { set_error("logistic_cv_auc: a fold of 2^31 rows or more is not supported"); return OEMGPU_ERR_UNSUPPORTED; }
    P = auc_plan(n, K, ncol, c->num_cu, longest);
    // perm, the counts and off stay where they were built (c->aux); the results and a batch's key buffers go to c->ws
    Bump W;
    const size_t a_u = W.take(8 * (size_t)K * P.cb), a_n1 = W.take(8 * (size_t)K), a_keys = W.take(P.hbm ? 16 * (size_t)n * P.cb : 0);
    if (ctx_reserve(c, W.off)) return OEMGPU_ERR_HIP;
    const int32_t *perm = (const int32_t *)(c->aux + a_perm);
    const int64_t *off = (const int64_t *)(c->aux + a_off);
    int64_t *ud = (int64_t *)(c->ws + a_u), *n1d = (int64_t *)(c->ws + a_n1);
    unsigned long long *keys = (unsigned long long *)(c->ws + a_keys);
    const bool any_lds = shortest <= P.lmax, any_hbm = P.hbm;
    const int64_t cap = std::min(longest, P.lmax);
    const size_t lds_in = AUC_AUX_BYTES + 16 * (size_t)cap;
    if (any_lds && lds_limit_once(reinterpret_cast<const void *>(&auc_segment_kernel<true>), lds_in)) return OEMGPU_ERR_HIP;
    if (any_hbm && lds_limit_once(reinterpret_cast<const void *>(&auc_segment_kernel<false>), AUC_AUX_BYTES)) return OEMGPU_ERR_HIP;
    std::vector<int64_t> hu(P.nbatch > 1 ? (size_t)K * P.cb : 0);
    for (int c0 = 0; c0 < ncol; c0 += P.cb) {
        const int nc = std::min(P.cb, ncol - c0);
        const double *pb = pred + (size_t)c0 * n;
        int64_t *n1b = c0 == 0 ? n1d : nullptr;
        if (any_lds)
            hipLaunchKernelGGL(auc_segment_kernel<true>, dim3((unsigned)K, (unsigned)nc), dim3(AUC_NT), lds_in, s, pb, n, y, y_hi, perm, off, P.lmax, cap,
                               (unsigned long long *)nullptr, P.cb, ud, nc, n1b);
        if (any_hbm)
            hipLaunchKernelGGL(auc_segment_kernel<false>, dim3((unsigned)K, (unsigned)nc), dim3(AUC_NT), AUC_AUX_BYTES, s, pb, n, y, y_hi, perm, off, P.lmax,
                               cap, keys, P.cb, ud, nc, n1b);
        OEM_HIP(hipGetLastError());
        // the batch's K x nc results: straight into u when the batch is the call, else through hu into columns c0 .. c0 + nc of each fold
        if (P.nbatch == 1) {
            OEM_HIP(hipMemcpyAsync(u, ud, 8 * (size_t)K * nc, hipMemcpyDeviceToHost, s));
        } else {
            OEM_HIP(hipMemcpyAsync(hu.data(), ud, 8 * (size_t)K * nc, hipMemcpyDeviceToHost, s));
            OEM_HIP(hipStreamSynchronize(s));
            for (int f = 0; f < K; ++f) std::copy(hu.begin() + (size_t)f * nc, hu.begin() + (size_t)(f + 1) * nc, u + (size_t)f * ncol + c0);
        }
    }
    OEM_HIP(hipMemcpyAsync(n1, n1d, 8 * (size_t)K, hipMemcpyDeviceToHost, s));
    OEM_HIP(hipStreamSynchronize(s));
    for (int f = 0; f < K; ++f) n0[f] = (hoff[f + 1] - hoff[f]) - n1[f];
    return 0;
}

}  // namespace oemgpu

using namespace oemgpu;

extern "C" {
#pragma GCC visibility push(default)

int oemgpu_logistic_cv_auc_dev(oemgpu_ctx *c, const double *predmat_dev, int64_t n, int32_t ncol, const double *y_dev, double y_hi,
                               const int32_t *foldid_dev, int32_t nfolds, int64_t *u, int64_t *n1, int64_t *n0)
{
    if (!c || !predmat_dev || !y_dev || !foldid_dev || !u || !n1 || !n0) { set_error("logistic_cv_auc: NULL argument"); return OEMGPU_ERR_ARG; }
    if (n < 1 || ncol < 1 || nfolds < 1) { set_error("logistic_cv_auc: bad n, ncol or nfolds"); return OEMGPU_ERR_ARG; }
    if (nfolds > AUC_MAX_FOLDS) { set_error("logistic_cv_auc: nfolds > %d is not supported", AUC_MAX_FOLDS); return OEMGPU_ERR_UNSUPPORTED; }
    if (n >= ((int64_t)1 << 31)) { set_error("logistic_cv_auc: n >= 2^31 is not supported"); return OEMGPU_ERR_UNSUPPORTED; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    return logistic_cv_auc_run(c, predmat_dev, n, ncol, y_dev, y_hi, foldid_dev, nfolds, u, n1, n0);
}

int oemgpu_selftest_cv_auc_plan(int64_t n, int32_t nfolds, int32_t ncol, int32_t num_cu, int64_t longest_fold, int64_t *out)
{
    if (n < 1 || nfolds < 1 || nfolds > AUC_MAX_FOLDS || ncol < 1 || num_cu < 1 || longest_fold < 0 || longest_fold > n || !out) {
        set_error("selftest_cv_auc_plan: bad argument");
        return OEMGPU_ERR_ARG;
    }
    const AucPlan P = auc_plan(n, nfolds, ncol, num_cu, longest_fold);
    out[0] = P.tile; out[1] = P.lmax; out[2] = P.cb; out[3] = P.nbatch; out[4] = (int64_t)P.ws; out[5] = (int64_t)P.lds; out[6] = P.hbm ? 1 : 0;
    out[7] = P.chunk; out[8] = P.nchunk;
    return 0;
}

#pragma GCC visibility pop
}
