// api.hip -- C ABI of liboemgpu: contexts, workspace, argument checks, and the entry points of the host-side driver that the
// reference keeps in src/oem_dense.cpp:30-309, src/oem_xtx.cpp:29-219 and src/oem_big.cpp:30-258; what they all end in
// (engine choice, lambda bookkeeping, result packing, DataStd::recover) is paths.hip.  All arithmetic of the hot path runs in the HIP
// kernels of gram.hip / path_small.hip / path_large.hip; there is no CPU fallback.
#include "paths.hpp"
#include "dense_src.hpp"
#include "multi.hpp"
#include "logistic.hpp"     // oemgpu_sparse_x

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace oemgpu {

// ---------------------------------------------------------------- the environment switches (switches.hpp), parsed once
static std::mutex g_sw_mu;
static std::atomic<const Switches *> g_sw{nullptr};
static unsigned g_sw_generation = 0;
static const Switches *sw_parse()
{
    Switches *t = new Switches();                     // (a reload leaks the old table -- a few hundred bytes, tests only: readers may still hold it)
    auto read = [](const char *name, Switch &v) {
        const char *e = getenv(name);
        v.set = e != nullptr;
        if (e) { v.num = atoll(e); strncpy(v.str, e, sizeof v.str - 1); v.str[sizeof v.str - 1] = 0; }
    };
#define OEM_SW_READ(name) read(#name, t->name);
    OEM_SWITCH_TABLE(OEM_SW_READ)
#undef OEM_SW_READ
    t->generation = ++g_sw_generation;
    return t;
}
const Switches &sw()
{
    const Switches *t = g_sw.load(std::memory_order_acquire);
    if (__builtin_expect(t != nullptr, 1)) return *t;
    std::lock_guard<std::mutex> lk(g_sw_mu);
    t = g_sw.load(std::memory_order_acquire);
    if (!t) { t = sw_parse(); g_sw.store(t, std::memory_order_release); }
    return *t;
}
void sw_reload()
{
    std::lock_guard<std::mutex> lk(g_sw_mu);
    g_sw.store(sw_parse(), std::memory_order_release);
}

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

// (kernel, device) -> largest dynamic-LDS limit set so far
int lds_limit_once(const void *fn, size_t bytes)
{
    struct Key { const void *fn; int dev; size_t bytes; };
    static std::mutex mu;
    static std::vector<Key> seen;
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> lk(mu);
        for (const Key &k : seen) if (k.fn == fn && k.dev == dev && k.bytes >= bytes) return 0;
    }
    OEM_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    std::lock_guard<std::mutex> lk(mu);
    for (Key &k : seen) if (k.fn == fn && k.dev == dev) { if (k.bytes < bytes) k.bytes = bytes; return 0; }
    seen.push_back(Key{fn, dev, bytes});
    return 0;
}

}  // namespace oemgpu

using namespace oemgpu;

namespace oemgpu {

int ctx_reserve(oemgpu_ctx *c, size_t bytes)
{
    if (bytes <= c->ws_bytes) return 0;
    if (c->ws) { OEM_HIP(hipStreamSynchronize(c->stream)); OEM_HIP(hipFree(c->ws)); c->ws = nullptr; c->ws_bytes = 0; }
    bytes = bytes + bytes / 8 + (1 << 20);
    OEM_HIP(hipMalloc((void **)&c->ws, bytes)); ++g_alloc_count;
    c->ws_bytes = bytes;
    return 0;
}

int ctx_grow(oemgpu_ctx *c, char **buf, size_t *have, size_t bytes)
{
    if (bytes <= *have) return 0;
    if (*buf) { OEM_HIP(hipStreamSynchronize(c->stream)); OEM_HIP(hipFree(*buf)); *buf = nullptr; *have = 0; }
    OEM_HIP(hipMalloc((void **)buf, bytes)); ++g_alloc_count;
    *have = bytes;
    return 0;
}

int set_device(const oemgpu_ctx *c) { OEM_HIP(hipSetDevice(c->device)); return 0; }

// ---------------------------------------------------------------- process-wide context cache
static std::mutex g_cache_mu;
static std::vector<oemgpu_ctx *> g_cache;

oemgpu_ctx *ctx_acquire(int device)
{
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        for (oemgpu_ctx *c : g_cache)
            if (c->device == device && !c->busy) { c->busy = true; (void)hipSetDevice(device); return c; }
    }
    oemgpu_ctx *c = oemgpu_create(device, nullptr);
    if (!c) return nullptr;
    c->cached = true; c->busy = true;
    std::lock_guard<std::mutex> lk(g_cache_mu);
    g_cache.push_back(c);
    return c;
}

// A cached context keeps its grow-only buffers between calls (no allocation in the steady state) -- up to a bound: the copy of the
// host rows (c->xres: up to half of HBM for one large fit) xval.oem's fold-ordered copy (c->aux) and the packed triangle of a q > 1024 Gram on the launch engines (c->pack_buf) are freed on release when they
// exceed OEMGPU_CACHE_KEEP_BYTES (default: an eighth of the device's memory, 36 GB on MI355X), so that one large oem() / big.oem()
// call does not starve torch or other users of the GPU for the rest of the session.  Streams, pinned staging lanes
// and the workspace stay.  The caller has synchronised the context's stream.
void ctx_release(oemgpu_ctx *c)
{
    if (!c) return;
    size_t keep = c->hbm_total / 8;
    if (sw().OEMGPU_CACHE_KEEP_BYTES.set && sw().OEMGPU_CACHE_KEEP_BYTES.num >= 0) keep = (size_t)sw().OEMGPU_CACHE_KEEP_BYTES.num;
    if (c->xres_bytes > keep || c->aux_bytes > keep || c->pack_bytes > keep) {
        (void)hipSetDevice(c->device);
        if (c->xres_bytes > keep) { (void)hipFree(c->xres); c->xres = nullptr; c->xres_bytes = 0; }
        if (c->aux_bytes > keep) { (void)hipFree(c->aux); c->aux = nullptr; c->aux_bytes = 0; }
        if (c->pack_bytes > keep) { (void)hipFree(c->pack_buf); c->pack_buf = nullptr; c->pack_bytes = 0; }
    }
    std::lock_guard<std::mutex> lk(g_cache_mu);
    c->busy = false;
}

int ctx_pinned(oemgpu_ctx *c, size_t bytes)
{
    if (bytes <= c->pinned_bytes) return 0;
    if (c->pinned) { OEM_HIP(hipStreamSynchronize(c->stream)); OEM_HIP(hipHostFree(c->pinned)); c->pinned = nullptr; c->pinned_bytes = 0; }
    bytes = bytes + bytes / 8 + 4096;
    OEM_HIP(hipHostMalloc((void **)&c->pinned, bytes, hipHostMallocDefault)); ++g_alloc_count;
    c->pinned_bytes = bytes;
    return 0;
}

}  // namespace oemgpu

namespace {

// ---------------------------------------------------------------- argument checks (the R front ends stop() on these)
int check_opts(const oemgpu_opts *o, int p, int ngroupvars_expected)
{
    if (!o) { set_error("opts is NULL"); return OEMGPU_ERR_ARG; }
    if (o->npen < 1 || !o->penalty) { set_error("at least one penalty is required"); return OEMGPU_ERR_ARG; }
    bool any_grp = false;
    for (int k = 0; k < o->npen; ++k) {
        if (o->penalty[k] < 0 || o->penalty[k] >= OEMGPU_NPENALTIES) { set_error("unknown penalty code %d", o->penalty[k]); return OEMGPU_ERR_ARG; }
        any_grp |= pen_is_grp(o->penalty[k]);
    }
    if (p < 2) { set_error("x must have at least two columns"); return OEMGPU_ERR_ARG; }                 // ref R/oem.R:226-229
    if (nl_of(o) < 1) { set_error("nlambda must be a positive integer"); return OEMGPU_ERR_ARG; }       // ref R/oem.R:361-364
    if (!(o->lambda_user && o->nlambda_user > 0) && !(o->lambda_min_ratio > 0.0 && o->lambda_min_ratio < 1.0)) {
        set_error("lambda.min.ratio must be between 0 and 1"); return OEMGPU_ERR_ARG;                    // ref R/oem.R:356-359
    }
    if (o->maxit <= 0) { set_error("maxit and irls.maxit should be positive"); return OEMGPU_ERR_ARG; }  // ref R/oem.R:427-430
    if (o->tol < 0) { set_error("tol and irls.tol should be nonnegative"); return OEMGPU_ERR_ARG; }
    if (!o->penalty_factor) { set_error("penalty.factor must have same length as number of columns in x"); return OEMGPU_ERR_ARG; }
    if (any_grp) {
        if (!o->groups || o->ngroupvars != ngroupvars_expected) {
            set_error("If any group penalty is used groups must have same length as number of columns in x");   // ref R/oem.R:288-290
            return OEMGPU_ERR_ARG;
        }
        if (!o->unique_groups || o->ngroups < 1) { set_error("unique_groups is empty"); return OEMGPU_ERR_ARG; }
        if (o->n_group_weights > 0 && o->n_group_weights != o->ngroups) {
            set_error("group.weights must have same length as the number of groups"); return OEMGPU_ERR_ARG;   // ref R/oem.R:313-315
        }
    }
    return 0;
}

}  // namespace

// the same checks for the entry points of other translation units (logistic.hip)
int oemgpu::check_opts_export(const oemgpu_opts *o, int p, int ngroupvars_expected) { return check_opts(o, p, ngroupvars_expected); }

#ifdef OEM_HOST_TIMING
namespace { struct HostT { double acc[8] = {0}; long n = 0; ~HostT() { if (n) fprintf(stderr, "host timing over %ld calls (us): entry->moments enqueued %.2f | ->path enqueued %.2f | ->copy enqueued %.2f | ->synced %.2f | ->unpacked/returned %.2f\n", n, acc[0] / n, acc[1] / n, acc[2] / n, acc[3] / n, acc[4] / n); } } g_ht; }
double oemgpu::g_tp[6];
#endif
namespace oemgpu {
// out[i] = ((parts[0][i] + parts[1][i]) + parts[2][i]) + ...: the shards' moment buffers added in shard (= rank = device) order -- the order
// hoststream.hip adds them in, so the one-process-per-GPU form (all-gather + this kernel) and the in-library form return the same bits
__global__ __launch_bounds__(256) void sum_in_order_kernel(const double *__restrict__ parts, int nparts, size_t len, double *__restrict__ out)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x) {
        double s = parts[i];
        for (int r = 1; r < nparts; ++r) s += parts[(size_t)r * len + i];
        out[i] = s;
    }
}

// moments of one device-resident shard into `moments` (overwrite) ; tpart/vpart scratch from the workspace
int shard_moments(oemgpu_ctx *c, const GramPlan &pl, const double *x, int64_t n, int64_t ld, const double *y,
                  const double *sums, double *tpart, double *vpart, double *moments)
{
    {                       // no clear: moments_reduce_kernel writes all (p+2)^2 entries
        Timer t(c, OEMGPU_T_GRAMK);
        int rc = launch_gram(c->stream, pl, x, n, ld, y, sums, tpart, vpart);
        if (rc) return rc;
    }
    return launch_moments_reduce(c->stream, pl, tpart, vpart, moments);
}

// ---------------------------------------------------------------- where a dense x lies (dense_src.hpp)
static_assert(GRAM_RM_P_MAX == OEMGPU_RM_P_MAX, "the header's limit is the kernel's");

int dense_src_check(const char *who, const DenseSrc &X, int64_t n, int32_t p)
{
    if (X.colmajor()) {
        if (X.ld < n) { set_error("%s: ld < n", who); return OEMGPU_ERR_ARG; }
        return 0;
    }
    if (X.dtype != OEMGPU_F64 && X.dtype != OEMGPU_F32) { set_error("%s: dtype is neither OEMGPU_F64 nor OEMGPU_F32", who); return OEMGPU_ERR_ARG; }
    if (X.ld < p) { set_error("%s: ldr < p", who); return OEMGPU_ERR_ARG; }
    const int el = X.dtype == OEMGPU_F32 ? 4 : 8;              // (every row-major kernel loads one element per lane)
    if ((uintptr_t)X.x % el) { set_error("%s: x_dev is not aligned to its %d-byte elements", who, el); return OEMGPU_ERR_ARG; }
    return 0;
}

int dense_src_shift_sums(hipStream_t s, const DenseSrc &X, int64_t n, int p, const double *y, double *sums)
{
    if (X.colmajor()) return launch_shift_sums(s, X.cm(), n, X.ld, p, y, sums);
    return launch_shift_sums_rm(s, X.x, X.dtype, n, X.ld, p, y, sums);
}

int dense_src_gather(hipStream_t s, const DenseSrc &X, int64_t n, int p, const double *y, const int32_t *foldid, int K, const int *pos,
                     double *xo, int64_t ldo, double *yo)
{
    if (X.colmajor()) return launch_gather_rows(s, X.cm(), n, X.ld, p, y, pos, xo, ldo, yo);
    return launch_gather_rows_rm(s, X.x, X.dtype, n, X.ld, p, y, foldid, K, pos, xo, ldo, yo);
}

static int rm_p_refusal(const char *who, int32_t p)
{
    if (p <= GRAM_RM_P_MAX) return 0;
    set_error("%s: the row-major pass takes p <= %d; larger p takes the column-major entry (oemgpu_fit_dense_dev / oemgpu_moments_dev)", who, GRAM_RM_P_MAX);
    return OEMGPU_ERR_UNSUPPORTED;
}

// (by the CU count alone: the host-only plans have no context)
static int moment_plan_cus(const char *who, int num_cu, bool colmajor, int64_t n, int32_t p, MomentPlan *pl)
{
    Bump B;
    if (colmajor) {
        pl->cm = gram_plan(n, p, num_cu);
        B.take(pl->cm.tpart_doubles * 8); B.take(pl->cm.vpart_doubles * 8);
    } else {
        if (int rc = rm_p_refusal(who, p)) return rc;
        pl->rm = gram_rm_plan(n, p, num_cu);
        B.take(pl->rm.tpart_doubles * 8);
    }
    pl->scratch_bytes = B.off;
    return 0;
}

int dense_src_moment_plan(const char *who, const oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, MomentPlan *pl)
{
    if (!X.colmajor()) if (int rc = rm_p_refusal(who, p)) return rc;      // (before the context is looked at)
    return moment_plan_cus(who, c->num_cu, X.colmajor(), n, p, pl);
}

int dense_src_moments(oemgpu_ctx *c, const MomentPlan &pl, const DenseSrc &X, int64_t n, const double *y, const double *sums, char *scratch,
                      double *moments)
{
    double *tpart = (double *)scratch;
    if (X.colmajor()) {
        Bump B; B.take(pl.cm.tpart_doubles * 8);
        return shard_moments(c, pl.cm, X.cm(), n, X.ld, y, sums, tpart, (double *)(scratch + B.off), moments);
    }
    {
        Timer t(c, OEMGPU_T_GRAMK);
        int rc = launch_gram_rm(c->stream, pl.rm, X.x, X.dtype, n, X.ld, y, sums, tpart);
        if (rc) return rc;
    }
    return launch_gram_rm_reduce(c->stream, pl.rm, tpart, moments);
}

// self-test aid: `blocks` workgroups that each take a whole CU (150 KB of LDS) and spin for `ms` milliseconds of device time
__global__ __launch_bounds__(256) void hold_cus_kernel(unsigned long long ticks, int *sink)
{
    extern __shared__ int hold_lds[];
    hold_lds[threadIdx.x] = (int)threadIdx.x;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
    if (hold_lds[threadIdx.x] == -1 && sink) *sink = 1;
}
}  // namespace

// =====================================================================================================
#pragma GCC visibility push(default)
extern "C" {

void oemgpu_reload_switches(void) { sw_reload(); }

const char *oemgpu_switch_names(void)
{
#define OEM_SW_NAME(name) #name " "
    return OEM_SWITCH_TABLE(OEM_SW_NAME);
#undef OEM_SW_NAME
}

const char *oemgpu_last_error(void) { return g_err; }
const char *oemgpu_version(void) { return "oemgpu 0.1 (gfx950)"; }

int oemgpu_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

oemgpu_ctx *oemgpu_create(int32_t device, void *stream)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) { set_error("no HIP device available (liboemgpu has no CPU fallback)"); return nullptr; }
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    if (device >= n) { set_error("device %d out of range (%d devices)", device, n); return nullptr; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { set_error("hipGetDeviceProperties failed"); return nullptr; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; liboemgpu is built for gfx950 only", device, prop.gcnArchName);
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) { set_error("hipSetDevice(%d) failed", device); return nullptr; }
    oemgpu_ctx *c = new oemgpu_ctx();
    c->device = device;
    c->num_cu = prop.multiProcessorCount;
    c->hbm_total = prop.totalGlobalMem;
    if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
    else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); delete c; return nullptr; }
        c->own_stream = true; ++g_alloc_count;
    }
    for (int i = 0; i < OEMGPU_NTIMERS; ++i) { c->ev_used[i] = false; c->ms[i] = 0.0; }
    return c;
}

void oemgpu_destroy(oemgpu_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->ws) (void)hipFree(c->ws);
    if (c->pinned) (void)hipHostFree(c->pinned);
    if (c->pinned_in) (void)hipHostFree(c->pinned_in);
    if (c->aux) (void)hipFree(c->aux);
    if (c->xres) (void)hipFree(c->xres);
    if (c->blob_buf) (void)hipFree(c->blob_buf);
    if (c->pack_buf) (void)hipFree(c->pack_buf);
    if (c->perm_buf) (void)hipFree(c->perm_buf);
    if (c->abort_host) (void)hipHostFree(c->abort_host);
    if (c->acc) (void)hipFree(c->acc);
    for (oemgpu_lane &l : c->lanes) {
        for (int k = 0; k < 2; ++k) {
            if (l.slot[k]) (void)hipHostFree(l.slot[k]);
            if (l.slot_ev[k]) (void)hipEventDestroy(l.slot_ev[k]);
            if (l.blk_ev[k]) (void)hipEventDestroy(l.blk_ev[k]);
        }
        if (l.s) (void)hipStreamDestroy(l.s);
    }
    for (int k = 0; k < 2; ++k) if (c->done_ev[k]) (void)hipEventDestroy(c->done_ev[k]);
    if (c->xfer_ev) (void)hipEventDestroy(c->xfer_ev);
    if (c->xfer_host) (void)hipHostFree(c->xfer_host);
    for (oemgpu_ctx *k : c->kids) oemgpu_destroy(k);
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->ev_made) for (int i = 0; i < 2 * OEMGPU_NTIMERS; ++i) (void)hipEventDestroy(c->ev[i]);
    if (c->xvs_ev_made) for (int i = 0; i <= OEMGPU_XVS_NPHASES; ++i) (void)hipEventDestroy(c->xvs_ev[i]);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

void oemgpu_release_cache(void)
{
    std::vector<oemgpu_ctx *> drop;
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        std::vector<oemgpu_ctx *> keep;
        for (oemgpu_ctx *c : g_cache) (c->busy ? keep : drop).push_back(c);
        g_cache.swap(keep);
    }
    for (oemgpu_ctx *c : drop) oemgpu_destroy(c);
}

int oemgpu_synchronize(oemgpu_ctx *c)
{
    if (!c) { set_error("ctx is NULL"); return OEMGPU_ERR_ARG; }
    OEM_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int oemgpu_selftest_gram_plan(int64_t n, int32_t p, int32_t num_cu, int64_t *out)
{
    if (n < 1 || p < 1 || num_cu < 1 || !out) { set_error("selftest_gram_plan: bad argument"); return OEMGPU_ERR_ARG; }
    const GramPlan pl = gram_plan(n, p, num_cu);
    const int64_t n8 = pl.n8, n6 = pl.n6, n4 = pl.n4;
    out[0] = pl.ntc; out[1] = n8; out[2] = n6; out[3] = pl.nchunk; out[4] = pl.steps;
    out[5] = 64 * (n8 * (n8 - 1) / 2) + 48 * n8 * n6 + 32 * n8 * n4 + 24 * n6 * n4 + 36 * n8 + 24 * n6 + 12 * n4;
    out[7] = n4;
    if (pl.wd) { out[1] = out[2] = out[7] = -1; out[5] = pl.wd == 4 ? 136 * pl.wd_units + 128 * pl.wd_units * (pl.wd_units - 1) : 80; }      // (one eight-wave workgroup per row chunk, the triangle of 16 tile columns: gram_wd.hip)
    out[6] = (int64_t)pl.ntc * (pl.ntc + 1) / 2;
    // the scratch sized for "any row count up to n" holds the plans of smaller row counts (folds, row tiles)
    const GramPlan bd = gram_plan_bound(n, p, num_cu);
    for (int64_t d = 1; d <= 4096 && n / d >= 1; d = d < 16 ? d + 1 : d * 2) {
        for (int64_t m : {n / d, n / d + 1, n - n / (d + 1)}) {
            if (m < 1 || m > n) continue;
            const GramPlan q = gram_plan(m, p, num_cu);
            if (q.tpart_doubles > bd.tpart_doubles || q.vpart_doubles > bd.vpart_doubles) {
                set_error("selftest_gram_plan: the plan of %lld rows (%d chunks) does not fit the bound for %lld (%d chunks)", (long long)m, q.nchunk, (long long)n, bd.nchunk);
                return OEMGPU_ERR_INTERNAL;
            }
        }
    }
    return 0;
}

int oemgpu_selftest_gram_form(int64_t n, int64_t ld, int32_t p, int32_t aligned, int32_t num_cu, int64_t *out)
{
    if (n < 1 || ld < 1 || p < 1 || num_cu < 1 || !out) { set_error("selftest_gram_form: bad argument"); return OEMGPU_ERR_ARG; }
    const GramForm f = gram_form(gram_plan(n, p, num_cu), n, ld, aligned != 0);
    out[0] = f.form; out[1] = f.strips;
    return 0;
}

int oemgpu_selftest_hold_cus(oemgpu_ctx *c, int32_t blocks, double ms)
{
    if (!c || blocks < 1 || blocks > 4096 || !(ms > 0.0) || ms > 30000.0) { set_error("hold_cus: bad argument"); return OEMGPU_ERR_ARG; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const int lds = 150 * 1024;
    OEM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&hold_cus_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(hold_cus_kernel, dim3(blocks), dim3(256), lds, c->stream, (unsigned long long)(ms * 1e5), (int *)nullptr);      // s_memrealtime: 100 MHz
    OEM_HIP(hipGetLastError());
    return 0;
}

int oemgpu_sum_in_order_dev(oemgpu_ctx *c, const double *parts_dev, int32_t nparts, int64_t len, double *out_dev)
{
    if (!c || !parts_dev || !out_dev || nparts < 1 || len < 1) { set_error("sum_in_order: bad argument"); return OEMGPU_ERR_ARG; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const int blocks = (int)std::min<int64_t>((len + 255) / 256, 2048);
    hipLaunchKernelGGL(sum_in_order_kernel, dim3(blocks), dim3(256), 0, c->stream, parts_dev, (int)nparts, (size_t)len, out_dev);
    OEM_HIP(hipGetLastError());
    return 0;
}

int oemgpu_selftest_sympk_gemv(oemgpu_ctx *c, const double *xx_dev, int32_t q, const double *vec_dev, double *out_dev, int32_t reps, double *us_per_product)
{
    if (!c || !xx_dev || !vec_dev || !out_dev || q <= 4096 || reps < 0 || reps > 100000) { set_error("selftest_sympk_gemv: bad argument (q > 4096)"); return OEMGPU_ERR_ARG; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    if (ctx_grow(c, &c->pack_buf, &c->pack_bytes, sympk_doubles(q) * sizeof(double))) return OEMGPU_ERR_HIP;
    return sympk_gemv_probe(c->stream, xx_dev, q, (double *)c->pack_buf, vec_dev, out_dev, reps, us_per_product);
}

int oemgpu_set_timing(oemgpu_ctx *c, int32_t on)
{
    if (!c) { set_error("ctx is NULL"); return OEMGPU_ERR_ARG; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    if (on && !c->ev_made) {
        for (int i = 0; i < 2 * OEMGPU_NTIMERS; ++i) OEM_HIP(hipEventCreate(&c->ev[i]));
        c->ev_made = true;
    }
    c->timing = on != 0;
    return 0;
}

int oemgpu_last_timings(oemgpu_ctx *c, double *ms)
{
    if (!c || !ms) { set_error("NULL argument"); return OEMGPU_ERR_ARG; }
    OEM_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < OEMGPU_NTIMERS; ++i) {
        ms[i] = 0.0;
        if (c->ev_made && c->ev_used[i]) {
            float f = 0.f;
            if (hipEventElapsedTime(&f, c->ev[2 * i], c->ev[2 * i + 1]) == hipSuccess) ms[i] = f;
        }
    }
    ms[OEMGPU_T_PATHCYC] = c->diag[0];
    ms[OEMGPU_T_PATHTICKS] = c->diag[1];
    return 0;
}

// ---------------------------------------------------------------------------------------------- staged interface
// what every entry below asks of (c, x, y, n, p) and of where x lies, in the called entry's name; no device work
static int src_args_check(const char *who, const oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const void *y_dev, bool outputs)
{
    if (!c || !X.x || !y_dev || !outputs) { set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG; }
    if (n < 1 || p < 1) { set_error("%s: bad n / p (n >= 1, p >= 1)", who); return OEMGPU_ERR_ARG; }
    return dense_src_check(who, X, n, p);
}

static int shift_sums_src(const char *who, oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const double *y_dev, double *sums_dev)
{
    if (int rc = src_args_check(who, c, X, n, p, y_dev, sums_dev != nullptr)) return rc;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    Timer t(c, OEMGPU_T_SHIFT);
    return dense_src_shift_sums(c->stream, X, n, p, y_dev, sums_dev);
}

int oemgpu_shift_sums_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                          double *sums_dev)
{
    return shift_sums_src("shift_sums", c, dense_src_cm(x_dev, ld), n, p, y_dev, sums_dev);
}

int oemgpu_shift_sums_rm_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                             double *sums_dev)
{
    return shift_sums_src("shift_sums_rm", c, dense_src_rm(x_dev, dtype, ldr), n, p, y_dev, sums_dev);
}

static int moments_src(const char *who, oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const double *y_dev, const double *sums_dev,
                       double *moments_dev)
{
    if (int rc = src_args_check(who, c, X, n, p, y_dev, moments_dev != nullptr)) return rc;
    MomentPlan pl;
    if (int rc = dense_src_moment_plan(who, c, X, n, p, &pl)) return rc;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    if (ctx_reserve(c, pl.scratch_bytes)) return OEMGPU_ERR_HIP;
    Timer t(c, OEMGPU_T_MOMENTS);
    return dense_src_moments(c, pl, X, n, y_dev, sums_dev, c->ws, moments_dev);
}

int oemgpu_moments_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                       const double *sums_dev, double *moments_dev)
{
    return moments_src("moments", c, dense_src_cm(x_dev, ld), n, p, y_dev, sums_dev, moments_dev);
}

int oemgpu_moments_rm_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                          const double *sums_dev, double *moments_dev)
{
    return moments_src("moments_rm", c, dense_src_rm(x_dev, dtype, ldr), n, p, y_dev, sums_dev, moments_dev);
}

static int run_paths_parts(oemgpu_ctx *c, Bump B, const double *xx, const double *xy, const double *st, int p, int q, int sem, int standardize, int intercept,
                           const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d,
                           const WideArgs *wd, const double *lmax_xy);

// wpatch (device, or NULL): the constants of DataStd's WEIGHTED standardisation (weighted.hip).  The moments are then those of the
// standardised, sqrt(w)-scaled copy: finalize takes them as they are (flag 0) and the constants go into `stats` for the lambda
// grid (scaleY) and for recover(), which run under the caller's flags.
static int solve_moments_impl(oemgpu_ctx *c, const double *moments_dev, const double *sums_dev, int32_t p,
                              int32_t semantics, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                              double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, const double *wpatch,
                              const PathExtras *ex = nullptr, const double *lmax_xy = nullptr, size_t extra_ws = 0, double *big_xy_std = nullptr);

int oemgpu_solve_moments_dev(oemgpu_ctx *c, const double *moments_dev, const double *sums_dev, int32_t p,
                             int32_t semantics, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                             double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    return solve_moments_impl(c, moments_dev, sums_dev, p, semantics, standardize, intercept, o, beta, lambda_out, niter, loss, d, nullptr);
}

static int solve_moments_impl(oemgpu_ctx *c, const double *moments_dev, const double *sums_dev, int32_t p,
                              int32_t semantics, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                              double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, const double *wpatch,
                              const PathExtras *ex, const double *lmax_xy, size_t extra_ws, double *big_xy_std)
{
    if (!c || !moments_dev || !beta || !lambda_out || !niter || !loss || !d) { set_error("solve_moments: NULL argument"); return OEMGPU_ERR_ARG; }
    if (semantics != OEMGPU_SEM_DENSE && semantics != OEMGPU_SEM_BIG && semantics != OEMGPU_SEM_XVAL) { set_error("unknown semantics %d", semantics); return OEMGPU_ERR_ARG; }
    const int q = p + ((semantics != OEMGPU_SEM_DENSE && intercept) ? 1 : 0);
    int rc = check_opts(o, p, q);
    if (rc) return rc;
    if (semantics == OEMGPU_SEM_BIG && o->compute_loss) {
        set_error("compute.loss is not available for big.oem: the reference expression is ill-formed (src/oem_big.h:899-921)");
        return OEMGPU_ERR_UNSUPPORTED;
    }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    Bump B;
    const size_t a_xx = B.take((size_t)q * q * 8), a_xy = B.take((size_t)q * 8), a_st = B.take((size_t)stats_len(p) * 8);
    // moments/sums may live in the workspace (fit_dense_dev): keep them below this frame
    size_t base = 0;
    if ((const char *)moments_dev >= c->ws && (const char *)moments_dev < c->ws + c->ws_bytes)
        base = ((const char *)moments_dev - c->ws) + (size_t)oemgpu_moments_len(p) * 8;
    if (sums_dev && (const char *)sums_dev >= c->ws && (const char *)sums_dev < c->ws + c->ws_bytes) {
        size_t e = ((const char *)sums_dev - c->ws) + (size_t)oemgpu_sums_len(p) * 8;
        if (e > base) base = e;
    }
    base = (base + 255) / 256 * 256;
    const size_t need = base + B.off + paths_ws_bytes(p, q, o) + extra_ws + 4096;
    if (need > c->ws_bytes) {
        if (base != 0) { set_error("internal: workspace frame too small"); return OEMGPU_ERR_INTERNAL; }
        if (ctx_reserve(c, need)) return OEMGPU_ERR_HIP;
    }
    Bump B2; B2.off = base + B.off;
    double *xx = (double *)(c->ws + base + a_xx), *xy = (double *)(c->ws + base + a_xy), *st = (double *)(c->ws + base + a_st);
    {
        Timer t(c, OEMGPU_T_FINAL);
        // big_xy_std (big.oem / sparse x with nobs <= nvars on the Gram, fit_big_gram_dev): X'X / n and X'y / n of the data as they are,
        // the column scales only in `stats` (returned coefficients) and in big_xy_std = xy colsq_inv (lambda_zero)
        const bool plain = wpatch || big_xy_std;
        rc = launch_finalize(c->stream, moments_dev, sums_dev, p, semantics, plain ? 0 : standardize, plain ? 0 : intercept, xx, xy, st);
        if (!rc && wpatch) rc = launch_weighted_patch_stats(c->stream, wpatch, p, st);
        if (!rc && big_xy_std) { rc = launch_big_gram_scales(c->stream, xx, xy, p, standardize, st, big_xy_std); lmax_xy = big_xy_std; }
        if (rc) return rc;
    }
    if (!ex) return run_paths_parts(c, B2, xx, xy, st, p, q, semantics, standardize, intercept, o, beta, lambda_out, niter, loss, d, nullptr, lmax_xy);
    PathExtras x = *ex;
    x.lmax_xy_dev = lmax_xy;
    return run_paths(c, B2, xx, xy, st, p, q, semantics, standardize, intercept, o, nullptr, beta, lambda_out, niter, loss, d, x);
}

// p >= n.  The reference switches to its two-GEMV iteration when nobs <= nvars (ref src/oem_dense.h:476-482); here that form is
// taken where it pays: the Gram form (same iteration, p^2 doubles read per iteration and held in memory) wins while p fits the
// register / cooperating engines (p <= 1024: ~1 us per iteration, no launch per iteration) and while 2 n p >= p^2; beyond, the
// wide engine reads 8 n p bytes per iteration and needs no p x p matrix (p = 20,000: 80 MB of Xs instead of 3.2 GB).
// OEM_WIDE=1 forces it wherever it can run (tests), OEM_NO_WIDE=1 switches it off.
static bool wide_pays(int64_t n, int32_t p, const oemgpu_opts *o)
{
    if (n > p || n > WIDE_MAX_N) return false;
    if (sw().OEM_NO_WIDE.set) return false;
    if (sw().OEM_WIDE.set) return true;
    // round 4: one element-wise penalty at 1024 < p <= 2048 -- the Gram form on the row-split engine (path_rowcoop_kernel: ONE exchange
    // per iteration, ~3.4 us) beats the persistent wide engine's two (500 x 2,000: 4.0 us).  Several penalties stay here: the wide
    // engine runs them side by side in workgroup sets of their own.
    if (p > 1024 && p <= 2048 && o && o->npen == 1 && !pen_is_grp(o->penalty[0]) && !o->accelerate && !o->compute_loss &&
        !sw().OEM_NO_ROWCOOP.set && !sw().OEM_NO_SYMCOOP.set && !sw().OEM_NO_COOP.set) return false;
    if (p <= 1024) return false;                  // (the register engines run the Gram form at 1-3 us per iteration)
    // where Xs fits the registers of the cooperating engine (path_wcoop.hip) that one launch beats everything else at these sizes
    // (n = 900, p = 1500: 5.6 against 11.6 us per iteration on the launch-per-iteration Gram engines)
    const int g = path_wcoop_workgroups((int)n, p);
    const bool wc = n <= 1024 && g >= 1 && g <= WCOOP_GMAX && !sw().OEM_NO_WCOOP.set;
    // round 4: up to p = 4096 the Gram lives in the register files of the chip (path_symcoop.hip: 5-7 us per iteration, no launch per
    // iteration) -- that beats the wide engine's launches (1,000 x 4,000: ~20 us per iteration) wherever the persistent wide engine
    // does not take the call
    if (p <= 4096 && !sw().OEM_NO_SYMCOOP.set && !sw().OEM_NO_COOP.set) return wc;
    if (2 * n < p) return true;
    // n <= p < 2n: the Gram is the smaller matrix
    return wc;
}

// p >= n, several penalties, some of them group penalties: one group penalty sends the WHOLE call to the engines that know group
// operators, and where the standardised X only fits the chip's registers WITH the accumulator file (path_wres_kernel: element-wise
// operators only) that is the launch-per-iteration engine re-reading Xs every iteration (500 x 20,000: 26-33 us per iteration
// against 7).  Penalties are independent cold starts (ref src/oem_dense.cpp:206-246), so the call is made in two parts there --
// the element-wise penalties, then the group penalties -- and the results go back into the caller's order.  (The eigenvalue step
// runs twice; both engines hold d to 1e-10 and the first part's is reported.)  OEM_NO_PENALTY_SPLIT=1: one call.
// The same for n > p with 1024 < p <= 2048: the element-wise penalties take the one-exchange row-split engine (path_rowcoop_kernel, ~3 us
// per iteration), the group penalties the symmetric engine's general form (~5).
static int run_paths_parts(oemgpu_ctx *c, Bump B, const double *xx, const double *xy, const double *st, int p, int q, int sem, int standardize, int intercept,
                           const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d,
                           const WideArgs *wd, const double *lmax_xy)
{
    std::vector<int> ie, ig;
    for (int k = 0; k < o->npen; ++k) (pen_is_grp(o->penalty[k]) ? ig : ie).push_back(k);
    bool split = !ie.empty() && !ig.empty() && !o->accelerate && !sw().OEM_NO_PENALTY_SPLIT.set;
    if (split && wd && wd->sparse) split = false;              // (one engine there: the launches over the non-zeros take every penalty)
    else if (split && wd) {
        const int gw = path_wres_workgroups(wd->n, p);
        const bool wcoop_fits = path_wcoop_workgroups(wd->n, p) >= 1 && path_wcoop_workgroups(wd->n, p) <= (c->num_cu * 3 / 4 < WCOOP_GMAX ? c->num_cu * 3 / 4 : WCOOP_GMAX);
        split = !wcoop_fits && gw >= 1 && gw <= c->num_cu - 8 && path_wres_xchg_doubles(wd->n, p) > 0 && !sw().OEM_NO_WRES.set && !sw().OEM_NO_WCOOP.set;
    } else if (split)
        split = q > 1024 && q <= 2048 && sem == OEMGPU_SEM_DENSE && path_rowcoop_workgroups(q) <= c->num_cu * 3 / 4 &&
                !sw().OEM_NO_ROWCOOP.set && !sw().OEM_NO_SYMCOOP.set && !sw().OEM_NO_COOP.set;
    PathExtras x;
    x.wide = wd; x.lmax_xy_dev = lmax_xy;
    if (!split) return run_paths(c, B, xx, xy, st, p, q, sem, standardize, intercept, o, nullptr, beta, lambda_out, niter, loss, d, x);
    const int nl = nl_of(o), rows = p + 1;
    const bool user = o->lambda_user && o->nlambda_user > 0;
    bool first = true;
    for (const std::vector<int> *part : {&ie, &ig}) {
        const int m = (int)part->size();
        std::vector<int32_t> pen(m);
        std::vector<double> lam(user ? (size_t)m * nl : 0);
        for (int k = 0; k < m; ++k) {
            pen[k] = o->penalty[(*part)[k]];
            if (user) memcpy(&lam[(size_t)k * nl], o->lambda_user + (size_t)(*part)[k] * nl, sizeof(double) * nl);
        }
        oemgpu_opts os = *o;
        os.npen = m; os.penalty = pen.data(); os.lambda_user = user ? lam.data() : nullptr;
        std::vector<double> b((size_t)m * nl * rows), lo((size_t)m * nl), ls((size_t)m * nl);
        std::vector<int32_t> ni((size_t)m * nl);
        double dd = 0.0;
        Bump Bp = B;                                             // (each part takes the same frame behind xy / stats)
        const int rc = run_paths(c, Bp, xx, xy, st, p, q, sem, standardize, intercept, &os, nullptr, b.data(), lo.data(), ni.data(), ls.data(), &dd, x);
        if (rc) return rc;
        for (int k = 0; k < m; ++k) {
            const size_t dst = (size_t)(*part)[k] * nl, src = (size_t)k * nl;
            memcpy(beta + dst * rows, &b[src * rows], sizeof(double) * (size_t)nl * rows);
            memcpy(lambda_out + dst, &lo[src], sizeof(double) * nl);
            memcpy(loss + dst, &ls[src], sizeof(double) * nl);
            memcpy(niter + dst, &ni[src], sizeof(int32_t) * nl);
        }
        if (first) *d = dd;
        first = false;
    }
    return 0;
}

// The workspace of "moments, then solve": behind the `frame` bytes the solve must find intact (sums, moments) lies the moment pass's
// scratch (up to pass_end), and later, over it, solve_moments_impl's own frame -- the q x q matrix, xy, stats, the engines' -- plus `extra`
static size_t moments_solve_ws(size_t frame, size_t pass_end, int32_t p, const oemgpu_opts *o, size_t extra = 0)
{
    const size_t solve = frame + ((size_t)p * p + p + stats_len(p)) * 8 + 1024 + paths_ws_bytes(p, p, o) + extra + 4096;
    return solve > pass_end ? solve : pass_end;
}

// The wide engine's staging in aux (whatever cv.oem's layout stamp vouched for is void): the blocked standardised copy xs, ys and the
// engine's scratch, and the WideArgs that name them.  The caller fills xs / ys (launch_wide_standardize) through the writable
// pointers handed back: WideArgs holds them const, as the engines read them.
static int wide_stage(oemgpu_ctx *c, int64_t n, int32_t p, WideArgs *wd, double **xs, double **ys)
{
    const WideLayout lay = wide_layout(n);
    Bump X;
    const size_t a_xs = X.take(sizeof(double) * (size_t)lay.rows() * p), a_ys = X.take(sizeof(double) * (size_t)lay.rows()),
                 a_sc = X.take(sizeof(double) * wide_scratch_doubles((int)n, p));
    ctx_void_cv(c);
    if (ctx_grow(c, &c->aux, &c->aux_bytes, X.off)) return OEMGPU_ERR_HIP;
    *xs = (double *)(c->aux + a_xs); *ys = (double *)(c->aux + a_ys);
    wd->xs = *xs; wd->ys = *ys; wd->lay = lay; wd->n = (int)n; wd->scratch = (double *)(c->aux + a_sc);
    return 0;
}

static int fit_dense_wide_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                              int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                              double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    if (set_device(c)) return OEMGPU_ERR_HIP;
    WideArgs wd;
    double *xs, *ys;
    int rc = wide_stage(c, n, p, &wd, &xs, &ys);
    if (rc) return rc;
    Bump B;
    const size_t a_xy = B.take((size_t)p * 8), a_st = B.take((size_t)stats_len(p) * 8);       // stats last: run_paths returns it with the outputs
    if (ctx_reserve(c, B.off + paths_ws_bytes(p, p, o) + 4096)) return OEMGPU_ERR_HIP;
    double *xy = (double *)(c->ws + a_xy), *st = (double *)(c->ws + a_st);
    {
        Timer t(c, OEMGPU_T_MOMENTS);             // the stage that reads X: DataStd on the data (the standardised copy, X'Y / n)
        rc = launch_wide_standardize(c->stream, x_dev, n, ld, p, y_dev, standardize, intercept, wd.lay, xs, ys, xy, st);
        if (rc) return rc;
    }
    return run_paths_parts(c, B, nullptr, xy, st, p, p, OEMGPU_SEM_DENSE, standardize, intercept, o, beta, lambda_out, niter, loss, d, &wd, nullptr);
}

// oemSparse::get_loss with nobs <= nvars (ref src/oem_sparse.h:932-941): the residual of the RETURNED coefficients on the data as they are
static int big_wide_sparse_loss(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev, const oemgpu_opts *o,
                                const double *beta, const int32_t *niter, double *loss)
{
    const size_t nk = (size_t)o->npen * nl_of(o), nchunk = (size_t)((n + 2047) / 2048);
    Bump L;
    const size_t a_b = L.take(nk * (size_t)(p + 1) * 8), a_p = L.take(nk * nchunk * 8), a_l = L.take(nk * 8);
    if (ctx_reserve(c, L.off + 4096)) return OEMGPU_ERR_HIP;          // (the paths are done: their frame may be overlaid)
    double *bd = (double *)(c->ws + a_b), *ld_ = (double *)(c->ws + a_l);
    OEM_HIP(hipMemcpyAsync(bd, beta, nk * (size_t)(p + 1) * 8, hipMemcpyHostToDevice, c->stream));
    int rc;
    if ((rc = launch_resid_loss(c->stream, x_dev, n, ld, p, y_dev, bd, p + 1, (int)nk, (double *)(c->ws + a_p), ld_))) return rc;
    OEM_HIP(hipMemcpyAsync(loss, ld_, nk * 8, hipMemcpyDeviceToHost, c->stream));
    OEM_HIP(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < nk; ++k) if (niter[k] == 0) loss[k] = 1e99;
    return 0;
}

// big.oem / oem() on a sparse x with nobs <= nvars and NO intercept (ref src/oem_big.h:537-541, 568-584, 743-764, 880-897;
// src/oem_sparse.h:607-612, 638-647): the iteration u = X'(Y - X beta)/n + d beta on the data AS THEY ARE, d from X X'/n, no y scaling;
// with standardize only lambda_zero (max |x_j'y| colsq_inv_j / n) and the returned coefficients (beta colsq_inv) carry the column
// scales -- what the reference does.  The wide engine on the DataStd-flag-0 copy is exactly that iteration.  (With an intercept the
// reference multiplies the n x nvars map by a vector of nvars + 1 entries: refused by the callers.)
static int fit_big_wide_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev, int32_t standardize,
                            const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, bool sparse_loss = false)
{
    if (set_device(c)) return OEMGPU_ERR_HIP;
    if (n < 2) { set_error("big.oem / sparse x with p >= n: at least two rows"); return OEMGPU_ERR_UNSUPPORTED; }
    int rc;
    if (!wide_pays(n, p, o)) {
        // ... on the Gram where the two-product form does not pay (p <= 1024: the register engines; n <= p < 2 n beyond the persistent
        // engines; more than WIDE_MAX_N rows, where the wide engine ends) -- as oemgpu_fit_dense_dev does for oemDense: the iteration
        // u = X'(Y - X b)/n + d b is (dI - X'X/n) b + X'Y/n, and X X'/n and X'X/n share their non-zero spectrum
        const GramPlan pl = gram_plan(n, p, c->num_cu);
        Bump B;
        const size_t a_xs2 = B.take((size_t)p * 8), a_mom = B.take((size_t)oemgpu_moments_len(p) * 8);
        const size_t frame = B.off;
        const size_t a_t = B.take(pl.tpart_doubles * 8), a_v = B.take(pl.vpart_doubles * 8);
        if (ctx_reserve(c, moments_solve_ws(frame, B.off, p, o))) return OEMGPU_ERR_HIP;
        double *mom = (double *)(c->ws + a_mom);
        {
            Timer t(c, OEMGPU_T_MOMENTS);
            rc = shard_moments(c, pl, x_dev, n, ld, y_dev, nullptr, (double *)(c->ws + a_t), (double *)(c->ws + a_v), mom);
            if (rc) return rc;
        }
        oemgpu_opts og = *o;
        og.compute_loss = 0;                          // (a sparse x: the loss is a pass of its own below; big.oem never has one)
        rc = solve_moments_impl(c, mom, nullptr, p, OEMGPU_SEM_BIG, standardize, 0, &og, beta, lambda_out, niter, loss, d, nullptr, nullptr, nullptr, 0,
                                (double *)(c->ws + a_xs2));
        return (rc || !sparse_loss) ? rc : big_wide_sparse_loss(c, x_dev, n, ld, p, y_dev, o, beta, niter, loss);
    }
    WideArgs wd;
    double *xs, *ys;
    if ((rc = wide_stage(c, n, p, &wd, &xs, &ys))) return rc;
    Bump B;
    const size_t a_xs2 = B.take((size_t)p * 8), a_xy = B.take((size_t)p * 8), a_st = B.take((size_t)stats_len(p) * 8);       // stats last (run_paths)
    if (ctx_reserve(c, B.off + paths_ws_bytes(p, p, o) + 4096)) return OEMGPU_ERR_HIP;
    double *xy = (double *)(c->ws + a_xy), *st = (double *)(c->ws + a_st), *xy_std = (double *)(c->ws + a_xs2);
    {
        Timer t(c, OEMGPU_T_MOMENTS);
        rc = launch_wide_standardize(c->stream, x_dev, n, ld, p, y_dev, 0, 0, wd.lay, xs, ys, xy, st);
        if (!rc && standardize) rc = launch_big_wide_scales(c->stream, x_dev, n, ld, p, xy, st, xy_std);
        if (rc) return rc;
    }
    rc = run_paths_parts(c, B, nullptr, xy, st, p, p, OEMGPU_SEM_BIG, standardize, 0, o, beta, lambda_out, niter, loss, d, &wd, standardize ? xy_std : nullptr);
    return (rc || !sparse_loss) ? rc : big_wide_sparse_loss(c, x_dev, n, ld, p, y_dev, o, beta, niter, loss);
}

// the same from one contiguous host matrix (n rows, column-major, ld = n)
static int fit_big_wide_host(const double *x, int64_t n, int32_t p, const double *y, int32_t standardize, const oemgpu_opts *o,
                             double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, bool sparse_loss = false)
{
    oemgpu_ctx *c = ctx_acquire(o->device);
    if (!c) return OEMGPU_ERR_NO_DEVICE;
    double *xd = nullptr, *yd = nullptr;
    int64_t ld = 0;
    int rc = host_upload_resident(c, x, n, p, y, o, &xd, &ld, &yd, 0, true);
    if (!rc) rc = fit_big_wide_dev(c, xd, n, ld, p, yd, standardize, o, beta, lambda_out, niter, loss, d, sparse_loss);
    (void)hipStreamSynchronize(c->stream);
    ctx_release(c);
    return rc;
}

// oem() on a dense x wherever it lies: moments about 0, the solve, and -- only when finalize advises a shift -- the sample sums, the
// moments about them and the solve again
static int fit_dense_src(const char *who, oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const double *y_dev,
                         int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                         double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    HT(0);
    int rc = src_args_check(who, c, X, n, p, y_dev, beta && lambda_out && niter && loss && d);
    if (!rc) rc = check_opts(o, p, p);
    if (rc) return rc;
    // p >= n (ref src/oem_dense.h:476-482,513-521: d from XXt / n, u = X'(Y - X b)/n + d b): the reference's own form where it
    // pays (wide_pays), else the same iteration on the Gram: the non-zero spectra of XXt and XtX coincide and
    // X'(Y - X b)/n + d b = (dI - X'X/n) b + X'Y/n.
    if (wide_pays(n, p, o)) {
        if (X.colmajor()) return fit_dense_wide_dev(c, X.cm(), n, X.ld, p, y_dev, standardize, intercept, o, beta, lambda_out, niter, loss, d);
        set_error("%s: %lld x %d is a shape of the p >= n engines, which read a column-major x: it takes the column-major entry "
                  "(oemgpu_fit_dense_dev)", who, (long long)n, p);
        return OEMGPU_ERR_UNSUPPORTED;
    }
    MomentPlan pl;
    if ((rc = dense_src_moment_plan(who, c, X, n, p, &pl))) return rc;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    Bump B;
    const size_t a_sums = B.take((size_t)oemgpu_sums_len(p) * 8), a_mom = B.take((size_t)oemgpu_moments_len(p) * 8);
    const size_t frame = B.off;
    const size_t a_scr = B.take(pl.scratch_bytes);
    if (ctx_reserve(c, moments_solve_ws(frame, B.off, p, o))) return OEMGPU_ERR_HIP;
    double *sums = (double *)(c->ws + a_sums), *mom = (double *)(c->ws + a_mom);
    // Moments about 0 first: that is what the shift predicate yields unless some column has |mean| > 16 sd, and finalize tells
    // (from the full-data moments) when it was the wrong guess.  The sample pass and the shifted pass then run only for such data.
    {
        Timer t(c, OEMGPU_T_MOMENTS);
        rc = dense_src_moments(c, pl, X, n, y_dev, nullptr, c->ws + a_scr, mom);
        if (rc) return rc;
    }
    HT(1);
    rc = oemgpu_solve_moments_dev(c, mom, nullptr, p, OEMGPU_SEM_DENSE, standardize, intercept, o, beta, lambda_out, niter, loss, d);
#ifdef OEM_HOST_TIMING
    HT(5); g_ht.acc[0] += g_tp[1] - g_tp[0]; g_ht.acc[1] += g_tp[2] - g_tp[1]; g_ht.acc[2] += g_tp[3] - g_tp[2]; g_ht.acc[3] += g_tp[4] - g_tp[3]; g_ht.acc[4] += g_tp[5] - g_tp[4]; ++g_ht.n;
#endif
    if (rc || !c->shift_advised) return rc;
    {
        Timer t(c, OEMGPU_T_SHIFT);
        rc = dense_src_shift_sums(c->stream, X, n, p, y_dev, sums);
        if (rc) return rc;
    }
    {
        Timer t(c, OEMGPU_T_MOMENTS);
        rc = dense_src_moments(c, pl, X, n, y_dev, sums, c->ws + a_scr, mom);
        if (rc) return rc;
    }
    return oemgpu_solve_moments_dev(c, mom, sums, p, OEMGPU_SEM_DENSE, standardize, intercept, o, beta, lambda_out, niter, loss, d);
}

int oemgpu_fit_dense_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                         int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                         double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    return fit_dense_src("fit_dense", c, dense_src_cm(x_dev, ld), n, p, y_dev, standardize, intercept, o, beta, lambda_out, niter, loss, d);
}

int oemgpu_fit_dense_rm_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                            int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                            double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    return fit_dense_src("fit_dense_rm", c, dense_src_rm(x_dev, dtype, ldr), n, p, y_dev, standardize, intercept, o, beta, lambda_out, niter, loss, d);
}

int oemgpu_selftest_gram_rm_plan(int64_t n, int32_t p, int32_t num_cu, int64_t *out)
{
    if (n < 1 || p < 1 || num_cu < 1 || !out) { set_error("selftest_gram_rm_plan: bad argument"); return OEMGPU_ERR_ARG; }
    if (int rc = rm_p_refusal("selftest_gram_rm_plan", p)) return rc;
    const GramRmPlan pl = gram_rm_plan(n, p, num_cu);
    out[0] = pl.ntc; out[1] = pl.nblk; out[2] = pl.nchunk; out[3] = pl.steps; out[4] = (int64_t)pl.nchunk * pl.nblk;
    out[5] = (int64_t)pl.tpart_doubles; out[6] = (int64_t)(pl.nchunk - 1) * pl.steps * 16; out[7] = GRAM_RM_P_MAX;
    return 0;
}

// oemDense with observation weights (weighted.hip has the algebra and the reference lines).  n > p.
static int fit_dense_weighted_impl(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev, const double *w_dev,
                                   const double *w_host, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                                   double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    if (!c || !x_dev || !y_dev || (!w_dev && !w_host)) { set_error("fit_dense_weighted: NULL argument"); return OEMGPU_ERR_ARG; }
    int rc = check_opts(o, p, p);
    if (rc) return rc;
    if (n < 1 || ld < n) { set_error("fit_dense_weighted: bad n / ld"); return OEMGPU_ERR_ARG; }
    const bool wide = n <= p;                             // the XWXt branch (ref src/oem_dense.h:466-471, 513-517)
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const int flag = (standardize ? 1 : 0) + 2 * (intercept ? 1 : 0);
    const int64_t ldz = (n + 63) / 64 * 64;
    Bump Z;
    const size_t a_z = Z.take(sizeof(double) * (size_t)ldz * p), a_yz = Z.take(sizeof(double) * (size_t)ldz), a_ws = Z.take(sizeof(double) * (size_t)(2 + 2 * p)),
                 a_w = Z.take(sizeof(double) * (size_t)n);
    // nobs <= nvars: the first pass's X'WX / n, X'(Yw) / n and constants are kept -- d, lambda_zero and the loss belong to them
    const size_t a_xx1 = wide ? Z.take(sizeof(double) * (size_t)p * p) : 0, a_xy1 = wide ? Z.take(sizeof(double) * (size_t)p) : 0,
                 a_st1 = wide ? Z.take(sizeof(double) * (size_t)stats_len(p)) : 0;
    ctx_void_cv(c);
    if (ctx_grow(c, &c->aux, &c->aux_bytes, Z.off)) return OEMGPU_ERR_HIP;
    double *z = (double *)(c->aux + a_z), *yz = (double *)(c->aux + a_yz), *wsd = (double *)(c->aux + a_ws);
    if (w_host) {
        for (int64_t i = 0; i < n; ++i)
            if (!(w_host[i] >= 0.0) || !std::isfinite(w_host[i])) { set_error("fit_dense_weighted: weights must be finite and >= 0"); return OEMGPU_ERR_ARG; }
        OEM_HIP(hipMemcpyAsync(c->aux + a_w, w_host, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        w_dev = (const double *)(c->aux + a_w);
    }
    const GramPlan pl = gram_plan(n, p, c->num_cu);
    Bump B;
    const size_t a_mom = B.take((size_t)oemgpu_moments_len(p) * 8);
    const size_t frame = B.off;
    const size_t a_t = B.take(pl.tpart_doubles * 8), a_v = B.take(pl.vpart_doubles * 8);
    const size_t large_ws = wide ? path_large_work_doubles(p, 128) * 8 + 4096 : 0;      // (the launch-per-iteration engine at any p)
    const size_t need = moments_solve_ws(frame, B.off, p, o, large_ws);
    if (ctx_reserve(c, need)) return OEMGPU_ERR_HIP;
    double *mom = (double *)(c->ws + a_mom);
    {
        Timer t(c, OEMGPU_T_MOMENTS);
        rc = launch_weighted_stats(c->stream, x_dev, n, ld, p, y_dev, w_dev, flag, wsd);
        if (!rc) rc = launch_weighted_apply(c->stream, x_dev, n, ld, p, y_dev, w_dev, flag, wsd, 0, z, ldz, yz);
        if (!rc) rc = shard_moments(c, pl, z, n, ldz, yz, nullptr, (double *)(c->ws + a_t), (double *)(c->ws + a_v), mom);
        if (rc) return rc;
    }
    if (!wide) return solve_moments_impl(c, mom, nullptr, p, OEMGPU_SEM_DENSE, standardize, intercept, o, beta, lambda_out, niter, loss, d, wsd);
    // ---- nobs <= nvars.  The reference takes d from (sqrt(w) Xs)(sqrt(w) Xs)'/n -- the non-zero spectrum of the Z'Z / n just formed --
    // and lambda_zero from XY = Xs'(Ys w)/n, but iterates u = Xs'((Ys - Xs beta) w^2)/n + d beta: the Gram form on Z2 = diag(w) Xs.
    double *xx1 = (double *)(c->aux + a_xx1), *xy1 = (double *)(c->aux + a_xy1), *st1 = (double *)(c->aux + a_st1);
    rc = launch_finalize(c->stream, mom, nullptr, p, OEMGPU_SEM_DENSE, 0, 0, xx1, xy1, st1);
    if (!rc) rc = launch_weighted_patch_stats(c->stream, wsd, p, st1);
    double lam1 = 0.0;
    if (!rc) rc = oemgpu_eig_max_dev(c, xx1, p, &lam1);              // (uses the workspace from its start: nothing of this call lives there now)
    if (rc) return rc;
    if (ctx_reserve(c, need)) return OEMGPU_ERR_HIP;
    mom = (double *)(c->ws + a_mom);
    {
        Timer t(c, OEMGPU_T_MOMENTS);
        rc = launch_weighted_apply(c->stream, x_dev, n, ld, p, y_dev, w_dev, flag, wsd, 1, z, ldz, yz);
        if (!rc) rc = shard_moments(c, pl, z, n, ldz, yz, nullptr, (double *)(c->ws + a_t), (double *)(c->ws + a_v), mom);
        if (rc) return rc;
    }
    PathExtras ex;
    ex.d_fixed = lam1 * 1.005;                                        // ref src/oem_dense.h:498
    ex.loss_xx = xx1; ex.loss_xy = xy1; ex.loss_stats = st1;          // get_loss = sum w (Ys - Xs beta)^2 (ref :759-770): the FIRST Gram's identity
    return solve_moments_impl(c, mom, nullptr, p, OEMGPU_SEM_DENSE, standardize, intercept, o, beta, lambda_out, niter, loss, d, wsd, &ex, xy1, large_ws);
}

int oemgpu_fit_dense_weighted_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev, const double *w_dev,
                                  int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                                  double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    return fit_dense_weighted_impl(c, x_dev, n, ld, p, y_dev, w_dev, nullptr, standardize, intercept, o, beta, lambda_out, niter, loss, d);
}

// host buffers in, as `.Call("oem_fit_dense", x, y, family, penalty, weights, ...)` hands them over (ref src/oem_dense.cpp:30-75)
int oemgpu_fit_dense_weighted(const double *x, int64_t n, int32_t p, const double *y, const double *weights, int32_t standardize, int32_t intercept,
                              const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    if (!x || !y || !weights || !o || !beta || !lambda_out || !niter || !loss || !d) { set_error("fit_dense_weighted: NULL argument"); return OEMGPU_ERR_ARG; }
    int rc = check_opts(o, p, p);
    if (rc) return rc;
    if (n < 1) { set_error("fit_dense_weighted: bad n"); return OEMGPU_ERR_ARG; }
    oemgpu_ctx *c = ctx_acquire(o->device);
    if (!c) return OEMGPU_ERR_NO_DEVICE;
    double *xd = nullptr, *yd = nullptr;
    int64_t ld = 0;
    rc = host_upload_resident(c, x, n, p, y, o, &xd, &ld, &yd, 0, true);
    if (!rc) rc = fit_dense_weighted_impl(c, xd, n, ld, p, yd, nullptr, weights, standardize, intercept, o, beta, lambda_out, niter, loss, d);
    (void)hipStreamSynchronize(c->stream);
    ctx_release(c);
    return rc;
}

int oemgpu_fit_xtx_dev(oemgpu_ctx *c, const double *xtx_dev, const double *xty_dev, int32_t p, const double *scale_factor,
                       const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    if (!c || !xtx_dev || !xty_dev || !beta || !lambda_out || !niter || !loss || !d) { set_error("fit_xtx: NULL argument"); return OEMGPU_ERR_ARG; }
    int rc = check_opts(o, p, p);
    if (rc) return rc;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    Bump B;
    const size_t a_xx = B.take((size_t)p * p * 8), a_xy = B.take((size_t)p * 8), a_sf = B.take((size_t)p * 8),
                 a_st = B.take((size_t)stats_len(p) * 8);      // stats last: run_paths returns it with the outputs
    if (ctx_reserve(c, B.off + paths_ws_bytes(p, p, o) + 4096)) return OEMGPU_ERR_HIP;
    double *xx = (double *)(c->ws + a_xx), *xy = (double *)(c->ws + a_xy), *st = (double *)(c->ws + a_st), *sf = (double *)(c->ws + a_sf);
    std::vector<double> sinv;
    if (scale_factor) {
        sinv.resize(p);
        for (int j = 0; j < p; ++j) sinv[j] = 1 / scale_factor[j];                // ref src/oem_xtx.h:527-529
        OEM_HIP(hipMemcpyAsync(sf, sinv.data(), sizeof(double) * p, hipMemcpyHostToDevice, c->stream));
        OEM_HIP(hipStreamSynchronize(c->stream));
    }
    {
        Timer t(c, OEMGPU_T_FINAL);
        rc = launch_xtx_prepare(c->stream, xtx_dev, xty_dev, scale_factor ? sf : nullptr, p, xx, xy, st);
        if (rc) return rc;
    }
    return run_paths(c, B, xx, xy, st, p, p, SEM_XTX, 0, 0, o, scale_factor, beta, lambda_out, niter, loss, d);
}

int oemgpu_last_shift_in_effect(oemgpu_ctx *c) { return c ? c->shifted : -1; }
int oemgpu_last_shift_advised(oemgpu_ctx *c) { return c ? c->shift_advised : -1; }

int oemgpu_eig_max_dev(oemgpu_ctx *c, const double *a_dev, int32_t p, double *lambda_max)
{
    if (!c || !a_dev || !lambda_max || p < 1) { set_error("eig_max: bad argument"); return OEMGPU_ERR_ARG; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    // run the engines with zero penalties: they stop after the eigenvalue step
    Bump B;
    const size_t a_z = B.take((size_t)(p + 8) * 8), a_o = B.take(256);
    const int lan = 2 * p < 32 ? 32 : (2 * p < 288 ? 2 * p : 288);
    size_t work_d = p <= SMALL_P_MAX ? path_small_xchg_bytes() / 8 : path_large_work_doubles(p, lan);
    const bool coop = path_coop_eligible(p, false, false, 0, 1);
    if (coop && work_d < path_coop_xchg_bytes() / 8) work_d = path_coop_xchg_bytes() / 8;
    const size_t a_w = B.take(work_d * 8);
    if (ctx_reserve(c, B.off)) return OEMGPU_ERR_HIP;
    if (ctx_pinned(c, 16384)) return OEMGPU_ERR_HIP;
    OEM_HIP(hipMemsetAsync(c->ws + a_z, 0, (size_t)(p + 8) * 8, c->stream));
    PathArgs a;
    memset(&a, 0, sizeof a);
    a.p = p; a.npen = 0; a.nl = 1; a.maxit = 1; a.lanczos_steps = lan; a.lambda_min_ratio = 0.5;
    a.xx = a_dev; a.xy = (const double *)(c->ws + a_z); a.pf = a.xy; a.stats = a.xy;
    a.d_out = (double *)(c->ws + a_o);
    a.work = (double *)(c->ws + a_w);
    a.pen_lo = 0; a.pen_hi = 0;
    CoopSlots slots;
    if (coop) slots.take(c->device, path_coop_workgroups(p), c->num_cu * 3 / 4);
    int rc = p <= SMALL_P_MAX ? launch_path_small(c->stream, a) : (coop ? launch_path_coop(c->stream, a) : run_path_large(c->stream, a, (double *)c->pinned));
    if (rc) return rc;
    double h[D_OUT_LEN];
    OEM_HIP(hipMemcpyAsync(h, a.d_out, sizeof h, hipMemcpyDeviceToHost, c->stream));
    OEM_HIP(hipStreamSynchronize(c->stream));
    if (h[6] != 0.0) { set_error("cooperating workgroups lost each other (exchange timeout)"); return OEMGPU_ERR_INTERNAL; }
    *lambda_max = h[1];
    c->eig_steps = (int)h[4]; c->eig_capped = h[5] != 0.0;
    return 0;
}

int oemgpu_last_path_engine(oemgpu_ctx *c, int32_t *engine, int32_t *persistent_fallbacks)
{
    if (!c) return -1;
    if (engine) *engine = c->last_engine;
    if (persistent_fallbacks) *persistent_fallbacks = c->persistent_fallbacks;
    return 0;
}

int oemgpu_last_placement(oemgpu_ctx *c) { return c ? c->last_placement : -1; }

int oemgpu_last_path_rounds(oemgpu_ctx *c, int64_t *short_rounds, int64_t *rounds)
{
    if (!c) return -1;
    if (short_rounds) *short_rounds = c->path_rounds_short;
    if (rounds) *rounds = c->path_rounds;
    return 0;
}

int oemgpu_last_eigen_info(oemgpu_ctx *c, int32_t *steps, int32_t *capped)
{
    if (!c) return -1;
    if (steps) *steps = c->eig_steps;
    if (capped) *capped = c->eig_capped ? 1 : 0;
    return 0;
}

// ---------------------------------------------------------------------------------------------- drop-in entry points
// Host buffers in, host buffers out.  Contexts come from the process-wide cache and own every device / pinned buffer the
// calls need (grow-only), so a repeated call creates no stream, allocates nothing and frees nothing.
int oemgpu_fit_dense(const double *x, int64_t n, int32_t p, const double *y, int32_t standardize, int32_t intercept,
                     const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    if (!x || !y || !o || !beta || !lambda_out || !niter || !loss || !d) { set_error("fit_dense: NULL argument"); return OEMGPU_ERR_ARG; }
    int rc = check_opts(o, p, p);
    if (rc) return rc;
    if (n < 1) { set_error("fit_dense: bad n"); return OEMGPU_ERR_ARG; }
    // p >= n (ref src/oem_dense.h:476-482,513-521): where the reference's two-GEMV form pays (wide_pays) the rows go up once and the
    // wide engine iterates through the standardised copy -- no (p+2)^2 moment buffer; otherwise the same iteration on the Gram.
    if (wide_pays(n, p, o) && o->ngpus <= 1) {
        oemgpu_ctx *c = ctx_acquire(o->device);
        if (!c) return OEMGPU_ERR_NO_DEVICE;
        double *xd = nullptr, *yd = nullptr;
        int64_t ld = 0;
        rc = host_upload_resident(c, x, n, p, y, o, &xd, &ld, &yd, 0, true);      // ld = n: whole columns go up as linear copies
        if (!rc) rc = fit_dense_wide_dev(c, xd, n, ld, p, yd, standardize, intercept, o, beta, lambda_out, niter, loss, d);
        (void)hipStreamSynchronize(c->stream);
        ctx_release(c);
        return rc;
    }
    return host_fit_dense(x, n, p, y, standardize, intercept, o, beta, lambda_out, niter, loss, d);
}

int oemgpu_fit_xtx(const double *xtx, const double *xty, int32_t p, const double *scale_factor, const oemgpu_opts *o,
                   double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    if (!xtx || !xty || !o) { set_error("fit_xtx: NULL argument"); return OEMGPU_ERR_ARG; }
    int rc = check_opts(o, p, p);
    if (rc) return rc;
    oemgpu_ctx *c = ctx_acquire(o->device);
    if (!c) return OEMGPU_ERR_NO_DEVICE;
    const size_t nb = sizeof(double) * (size_t)p * p;
    rc = ctx_grow(c, &c->xres, &c->xres_bytes, nb + sizeof(double) * (size_t)p + 256);
    double *ad = (double *)c->xres, *bd = (double *)(c->xres + (nb + 255) / 256 * 256);
    if (!rc) {
        hipError_t e = hipMemcpyAsync(ad, xtx, nb, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(bd, xty, sizeof(double) * (size_t)p, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) { set_error("upload of xtx failed: %s", hipGetErrorString(e)); rc = OEMGPU_ERR_HIP; }
    }
    if (!rc) rc = oemgpu_fit_xtx_dev(c, ad, bd, p, scale_factor, o, beta, lambda_out, niter, loss, d);
    (void)hipStreamSynchronize(c->stream);
    ctx_release(c);
    return rc;
}

int oemgpu_fit_big(const double *const *x_shards, const int64_t *n_shard, int32_t nshards, int32_t p,
                   const double *const *y_shards, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                   double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    if (!x_shards || !n_shard || !y_shards || !o || nshards < 1 || !beta || !lambda_out || !niter || !loss || !d) {
        set_error("fit_big: bad argument"); return OEMGPU_ERR_ARG;
    }
    const int q = p + (intercept ? 1 : 0);
    int rc = check_opts(o, p, q);
    if (rc) return rc;
    if (o->compute_loss) {
        set_error("compute.loss is not available for big.oem: the reference expression is ill-formed (src/oem_big.h:899-921)");
        return OEMGPU_ERR_UNSUPPORTED;
    }
    int64_t n = 0;
    for (int s = 0; s < nshards; ++s) {
        if (n_shard[s] < 0 || (n_shard[s] > 0 && (!x_shards[s] || !y_shards[s]))) { set_error("fit_big: bad shard %d", s); return OEMGPU_ERR_ARG; }
        n += n_shard[s];
    }
    if (n <= q) {
        // nobs <= nvars + intercept: the XXt branch (ref src/oem_big.h:537-541, 568-584)
        if (intercept) {
            set_error("big.oem with p >= n and an intercept: the reference multiplies the n x p map by a vector of p + 1 entries (src/oem_big.h:568-584) -- "
                      "nothing well-formed to reproduce; intercept = FALSE is served");
            return OEMGPU_ERR_UNSUPPORTED;
        }
        std::vector<double> xc, yc;                                     // the shards as one matrix (n <= p rows)
        try { xc.resize((size_t)n * p); yc.resize((size_t)n); }
        catch (const std::bad_alloc &) { set_error("big.oem with p >= n: no host memory for the %lld x %d matrix", (long long)n, p); return OEMGPU_ERR_ARG; }
        int64_t r0 = 0;
        for (int s = 0; s < nshards; ++s) {
            const int64_t ns = n_shard[s];
            for (int j = 0; j < p && ns > 0; ++j) memcpy(xc.data() + (size_t)j * n + r0, x_shards[s] + (size_t)j * ns, sizeof(double) * (size_t)ns);
            if (ns > 0) memcpy(yc.data() + r0, y_shards[s], sizeof(double) * (size_t)ns);
            r0 += ns;
        }
        return fit_big_wide_host(xc.data(), n, p, yc.data(), standardize, o, beta, lambda_out, niter, loss, d);
    }
    return host_fit_big(x_shards, n_shard, nshards, p, y_shards, standardize, intercept, o, beta, lambda_out, niter, loss, d);
}

// ---------------------------------------------------------------------------------------------- oem() on a sparse X
// oemSparse's Gram is oemBig's with the intercept column holding `intval` instead of 1 (ref src/oem_sparse.h:577-593):
// XX_sparse = D XX_big D, XY_sparse = D XY_big, D = diag(intval, 1, ..., 1).
static __global__ void scale_intercept_kernel(double *__restrict__ xx, double *__restrict__ xy, int q, double intval)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= q) return;
    if (j == 0) { xx[0] *= intval * intval; xy[0] *= intval; }
    else { xx[(size_t)j * q] *= intval; xx[j] *= intval; }
}

// The oemSparse solve on one moment buffer (both triangles, about 0; its [p + 1][p + 1] entry the number of rows, which stands wherever n
// enters: the column scales' n - 1, the / n): oemBig's XX and XY (launch_finalize), the intercept's row and column times intval, the
// paths with get_beta's in-place intercept scale (ref src/oem_sparse.h:493-508, 577-593, 897-900).  oemgpu_fit_sparse and
// oemgpu_cv_sparse_fold_fits_res both end here.  The workspace: whatever the caller has carved (B), then xx, xy, stats and the paths'
// frame -- reserved (`need` bytes of c->ws) BEFORE the moments are computed if they live in c->ws themselves.
struct SparseSolveWs { Bump B; size_t a_xx, a_xy, a_st, need; };
static SparseSolveWs sparse_solve_ws(Bump B, int p, int q, const oemgpu_opts *o)
{
    SparseSolveWs W;
    W.a_xx = B.take((size_t)q * q * 8); W.a_xy = B.take((size_t)q * 8); W.a_st = B.take((size_t)stats_len(p) * 8);
    W.B = B;
    W.need = B.off + paths_ws_bytes(p, q, o) + 4096;
    return W;
}
static int sparse_solve(oemgpu_ctx *c, const SparseSolveWs &W, const double *mom, int p, int q, int standardize, int intercept, const oemgpu_opts *o,
                        double intval, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    double *xx = (double *)(c->ws + W.a_xx), *xy = (double *)(c->ws + W.a_xy), *st = (double *)(c->ws + W.a_st);
    int rc = launch_finalize(c->stream, mom, nullptr, p, OEMGPU_SEM_BIG, standardize, intercept, xx, xy, st);
    if (rc) return rc;
    std::vector<double> sf;
    if (intercept) {
        hipLaunchKernelGGL(scale_intercept_kernel, dim3((q + 255) / 256), dim3(256), 0, c->stream, xx, xy, q, intval);
        sf.assign(q, 1.0); sf[0] = 1.0 / intval;              // get_beta multiplies the intercept slot by intval, in place (ref :897-900)
    }
    Bump B = W.B;
    return run_paths(c, B, xx, xy, st, p, q, SEM_SPARSE, standardize, intercept, o, intercept ? sf.data() : nullptr, beta, lambda_out, niter, loss, d);
}

// diag[j] = sum x_j^2 of a moment buffer ((p + 2)^2), j < p
static __global__ void moment_diag_kernel(const double *__restrict__ M, int p, double *__restrict__ diag)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < p) diag[j] = M[(size_t)j * (p + 2) + j];
}

// the frame of one instance of solve_moments_batch (xx | xy | stats), and the workspace a batch of `nbatch` reserves
static size_t batch_instance_bytes(int p, int q)
{
    return ((size_t)q * q * 8 + 255) / 256 * 256 + ((size_t)q * 8 + 255) / 256 * 256 + ((size_t)stats_len(p) * 8 + 255) / 256 * 256;
}
static size_t batch_ws_bytes(int p, int q, const oemgpu_opts *o, int nbatch)
{
    Bump B;
    B.take(batch_instance_bytes(p, q) * nbatch);
    return B.off + paths_ws_bytes(p, q, o, nbatch) + 4096;
}

// nbatch moment buffers (instance b at moments + b * mstride, all OUTSIDE the context workspace), one finalize each, then ONE
// launch that walks all their paths side by side (q <= SMALL_P_MAX).  Outputs as in run_paths.
// cs != nullptr: observation weights -- the moments are those of the p + 1 data columns [sqrt(w) | sqrt(w) X] ((p + 3)^2 each) and
// cs holds the unweighted column sums of squares and the row count of every instance (launch_finalize_weighted).
// shared_lmax: every lambda grid from instance 0's X'Y -- or, with 0 < lmax_group < nbatch, instance b's from the first instance of its
// group of lmax_group (xval_oem_multi: the K + 1 fits of every response on that response's full-data grid).
static int solve_moments_batch(oemgpu_ctx *c, const double *moments, size_t mstride, int nbatch, int32_t p, int32_t semantics,
                               int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                               double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, bool shared_lmax,
                               const double *cs = nullptr, size_t cstride = 0, int32_t *shift_advised = nullptr, int lmax_group = 0)
{
    const int q = p + ((semantics != OEMGPU_SEM_DENSE && intercept) ? 1 : 0);
    Bump B;
    const size_t per = batch_instance_bytes(p, q);
    const size_t a_0 = B.take(per * nbatch);
    if (ctx_reserve(c, batch_ws_bytes(p, q, o, nbatch))) return OEMGPU_ERR_HIP;
    const size_t o_xy = ((size_t)q * q * 8 + 255) / 256 * 256, o_st = o_xy + ((size_t)q * 8 + 255) / 256 * 256;
    for (int b = 0; b < nbatch; ++b) {
        char *f = c->ws + a_0 + per * b;
        int rc = cs ? launch_finalize_weighted(c->stream, moments + mstride * b, cs + cstride * b, p, standardize, intercept, (double *)f,
                                               (double *)(f + o_xy), (double *)(f + o_st))
                    : launch_finalize(c->stream, moments + mstride * b, nullptr, p, semantics, standardize, intercept, (double *)f,
                                      (double *)(f + o_xy), (double *)(f + o_st));
        if (rc) return rc;
    }
    char *f0 = c->ws + a_0;
    PathExtras x;
    x.nbatch = nbatch; x.bstride = per / 8; x.shared_lmax = shared_lmax; x.lmax_group = lmax_group; x.shift_advised_out = shift_advised;
    return run_paths(c, B, (const double *)f0, (const double *)(f0 + o_xy), (const double *)(f0 + o_st), p, q, semantics, standardize,
                     intercept, o, nullptr, beta, lambda_out, niter, loss, d, x);
}

// ---------------------------------------------------------------------------------------------- xval.oem
static int any_grp_count(const oemgpu_opts *o)
{
    for (int k = 0; k < o->npen; ++k) if (pen_is_grp(o->penalty[k])) return o->ngroups;
    return 0;
}

static int ctx_aux(oemgpu_ctx *c, size_t bytes)
{
    if (bytes <= c->aux_bytes) return 0;
    ctx_void_cv(c);                                              // (a new allocation may come back at the old address)
    if (c->aux) { OEM_HIP(hipStreamSynchronize(c->stream)); OEM_HIP(hipFree(c->aux)); c->aux = nullptr; c->aux_bytes = 0; }
    OEM_HIP(hipMalloc((void **)&c->aux, bytes)); ++g_alloc_count;
    c->aux_bytes = bytes;
    return 0;
}

// ---------------------------------------------------------------------------------------------- many responses on one x (multi.hip)
// How many responses one batched launch takes, and on which engine: plan_paths' rules for nbatch > 1, read from the side of the caller
// who chooses nbatch.  Never more than 513 instances (the most the batch launch has been run at: xval.oem with 512 folds); and wherever
// an instance is more than one workgroup -- the cooperating engine's set, the four workgroups per penalty of path_small.hip at
// 208 < q <= 288 -- those workgroups wait for each other, so all of a launch together stay within 3/4 of the CUs.  (The cooperating
// engine splits the penalties over sets of their own only while instances x penalties x workgroups <= half the CUs, plan_paths'
// pen_split rule, so the factor npen never breaks the bound there; path_small.hip always splits.)  Engine 0: no batch engine takes
// the shape -- q > 1024, the cooperating engine switched off beyond 288, or fewer CUs than one set needs -- and the responses are
// solved one after another.
struct MultiSolve { int cap = 1, engine = OEMGPU_ENGINE_NONE; };
static MultiSolve multi_solve_plan(int num_cu, int q, int npen, int ngroups)
{
    MultiSolve S;
    const int cus = num_cu * 3 / 4;
    int cap = 0, engine = OEMGPU_ENGINE_NONE;
    if (path_coop_eligible(q, false, false, ngroups, 2)) { cap = cus / path_coop_workgroups(q); engine = OEMGPU_ENGINE_COOP; }
    else if (q <= 208) { cap = 513; engine = OEMGPU_ENGINE_ROWS; }                     // (path_small_takes_rows: one workgroup per instance and penalty, which waits for nobody)
    else if (q <= SMALL_P_MAX) { cap = cus / (4 * (npen > 1 ? npen : 1)); engine = OEMGPU_ENGINE_ROWS; }
    if (cap >= 1) { S.cap = cap < 513 ? cap : 513; S.engine = engine; }
    return S;
}

// The buffers of the call in oemgpu_ctx::aux -- the one moment buffer, one response as a contiguous vector, the chunk partials of the
// X'Y pass, the composed buffers of ONE batched launch -- and the workspace reserved once for the passes and the largest launch.
struct MultiLay {
    MultiPlan xp;
    MultiSolve sv;
    MomentPlan mp;
    bool one_order = false;
    int nsolve = 0;
    size_t a_base = 0, a_col = 0, a_part = 0, a_comp = 0, total = 0, ws = 0;
};
static int multi_layout(const char *who, int num_cu, bool colmajor, int64_t n, int32_t p, int32_t m, const oemgpu_opts *o, bool solve, MultiLay *L)
{
    // The Gram block of every layout from ONE summation order wherever there is one: gram_rm.hip's pass, which reads a column-major x
    // too (its CM form), up to its p; beyond, a column-major x keeps gram.hip's pass (a row-major one is refused there)
    L->one_order = !colmajor || p <= GRAM_RM_P_MAX;
    if (int rc = moment_plan_cus(who, num_cu, !L->one_order, n, p, &L->mp)) return rc;
    L->xp = multi_plan(n, p, m, num_cu);
    const size_t mlen = (size_t)oemgpu_moments_len(p) * 8;
    Bump A;
    L->a_base = A.take(mlen); L->a_col = A.take((size_t)n * 8); L->a_part = A.take(L->xp.part_doubles * 8);
    L->ws = L->mp.scratch_bytes + 4096;
    if (solve) {
        L->sv = multi_solve_plan(num_cu, p, o->npen, any_grp_count(o));
        L->nsolve = (m + L->sv.cap - 1) / L->sv.cap;
        const int nb = m < L->sv.cap ? m : L->sv.cap;
        L->a_comp = A.take(mlen * nb);
        const size_t w = L->sv.engine != OEMGPU_ENGINE_NONE ? batch_ws_bytes(p, p, o, nb) : moments_solve_ws(0, 0, p, o);
        if (w > L->ws) L->ws = w;
    }
    L->total = A.off;
    return 0;
}

// the one moment pass about 0 (response 0 riding as y) into `base`, the X'Y pass into `part`
static int multi_passes(oemgpu_ctx *c, const MultiLay &L, const DenseSrc &X, const MultiY &Y)
{
    char *ax = c->aux;
    double *col = (double *)(ax + L.a_col);
    const double *y0 = Y.y;
    int rc = 0;
    if (Y.rs != 1) { if ((rc = launch_multi_column(c->stream, Y, L.xp.n, 0, col))) return rc; y0 = col; }
    Timer t(c, OEMGPU_T_MOMENTS);                                    // (both passes over x: the moment build of this call)
    if (L.one_order) {
        {
            Timer tk(c, OEMGPU_T_GRAMK);
            if ((rc = launch_gram_rm(c->stream, L.mp.rm, X.x, X.colmajor() ? -1 : X.dtype, L.xp.n, X.ld, y0, nullptr, (double *)c->ws))) return rc;
        }
        if ((rc = launch_gram_rm_reduce(c->stream, L.mp.rm, (const double *)c->ws, (double *)(ax + L.a_base)))) return rc;
    } else if ((rc = dense_src_moments(c, L.mp, X, L.xp.n, y0, nullptr, c->ws, (double *)(ax + L.a_base)))) return rc;
    return launch_multi_xty(c->stream, L.xp, X, Y, (double *)(ax + L.a_part));
}

// oem() for every column of Y on one dense x, wherever it lies: one moment pass about 0, one X'Y pass, the paths in batched launches
// (route 0) or one by one (1); a response whose solve advises a shift is fitted again by fit_dense_src (2)
static int fit_dense_multi_src(const char *who, oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const double *y_dev, int64_t rs, int64_t cs,
                               int32_t m, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                               double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, int32_t *route)
{
    int rc = src_args_check(who, c, X, n, p, y_dev, beta && lambda_out && niter && loss && d && route);
    if (!rc) rc = multi_y_check(who, n, rs, cs, m);
    if (!rc) rc = check_opts(o, p, p);
    if (rc) return rc;
    if (n <= p) {
        set_error("%s: %lld x %d has n <= p, a shape of the p >= n engines, which this call does not serve: such responses are fitted one at a "
                  "time (oemgpu_fit_dense_dev)", who, (long long)n, p);
        return OEMGPU_ERR_UNSUPPORTED;
    }
    if (!X.colmajor()) if ((rc = rm_p_refusal(who, p))) return rc;      // (before the context is looked at)
    MultiLay L;
    if ((rc = multi_layout(who, c->num_cu, X.colmajor(), n, p, m, o, true, &L))) return rc;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    ctx_void_cv(c);
    if (ctx_aux(c, L.total)) return OEMGPU_ERR_HIP;
    if (ctx_reserve(c, L.ws)) return OEMGPU_ERR_HIP;                 // once, for the passes and the largest launch
    const MultiY Y{y_dev, rs, cs};
    if ((rc = multi_passes(c, L, X, Y))) return rc;
    const double *base = (const double *)(c->aux + L.a_base), *part = (const double *)(c->aux + L.a_part);
    double *comp = (double *)(c->aux + L.a_comp), *col = (double *)(c->aux + L.a_col);
    const size_t nk = (size_t)o->npen * nl_of(o), blen = nk * (size_t)(p + 1), mlen = (size_t)oemgpu_moments_len(p);
    auto interrupted = [&]() {
        if (!(o->interrupt && o->interrupt(o->interrupt_arg))) return false;
        set_error("interrupted by the caller");
        return true;
    };
    std::vector<int32_t> adv(m, 0);
    for (int r0 = 0; r0 < m; r0 += L.sv.cap) {
        const int nb = m - r0 < L.sv.cap ? m - r0 : L.sv.cap;
        if (r0 > 0 && interrupted()) return OEMGPU_ERR_INTERRUPTED;
        if ((rc = launch_multi_compose(c->stream, L.xp, base, part, r0, nb, comp))) return rc;
        if (L.sv.engine != OEMGPU_ENGINE_NONE) {
            rc = solve_moments_batch(c, comp, mlen, nb, p, OEMGPU_SEM_DENSE, standardize, intercept, o, beta + blen * r0, lambda_out + nk * r0,
                                     niter + nk * r0, loss + nk * r0, d + r0, false, nullptr, 0, adv.data() + r0);
            for (int b = 0; b < nb; ++b) route[r0 + b] = 0;
        } else {
            rc = solve_moments_impl(c, comp, nullptr, p, OEMGPU_SEM_DENSE, standardize, intercept, o, beta + blen * r0, lambda_out + nk * r0,
                                    niter + nk * r0, loss + nk * r0, d + r0, nullptr);
            adv[r0] = c->shift_advised ? 1 : 0;
            route[r0] = 1;
        }
        if (rc) return rc;
    }
    // the shift predicate looks at x AND y (finalize_kernel): if x advises, every response does; else only those whose own y does
    for (int r = 0; r < m; ++r) {
        if (!adv[r]) continue;
        if (interrupted()) return OEMGPU_ERR_INTERRUPTED;
        const double *yr = y_dev + (int64_t)r * cs;
        if (rs != 1) { if ((rc = launch_multi_column(c->stream, Y, n, r, col))) return rc; yr = col; }
        if ((rc = fit_dense_src(who, c, X, n, p, yr, standardize, intercept, o, beta + blen * r, lambda_out + nk * r, niter + nk * r, loss + nk * r, d + r)))
            return rc;
        route[r] = 2;
    }
    return 0;
}

int oemgpu_fit_dense_multi_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev, int64_t y_rs, int64_t y_cs,
                               int32_t m, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                               double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, int32_t *route)
{
    return fit_dense_multi_src("fit_dense_multi", c, dense_src_cm(x_dev, ld), n, p, y_dev, y_rs, y_cs, m, standardize, intercept, o, beta, lambda_out,
                               niter, loss, d, route);
}

int oemgpu_fit_dense_multi_rm_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev, int64_t y_rs,
                                  int64_t y_cs, int32_t m, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                                  double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, int32_t *route)
{
    return fit_dense_multi_src("fit_dense_multi_rm", c, dense_src_rm(x_dev, dtype, ldr), n, p, y_dev, y_rs, y_cs, m, standardize, intercept, o, beta,
                               lambda_out, niter, loss, d, route);
}

int oemgpu_selftest_multi_plan(int64_t n, int32_t p, int32_t m, int32_t npen, int32_t layout, int32_t num_cu, int64_t *out)
{
    if (n < 1 || p < 1 || m < 1 || npen < 1 || num_cu < 1 || (layout != 0 && layout != 1) || !out) { set_error("selftest_multi_plan: bad argument"); return OEMGPU_ERR_ARG; }
    if (n <= p) { set_error("selftest_multi_plan: n <= p, a shape of the p >= n engines, which the call does not serve"); return OEMGPU_ERR_UNSUPPORTED; }
    // (the workspace of the paths grows with the penalties and lambdas: npen element-wise penalties of 100 lambdas stand for the call's)
    std::vector<int32_t> pen(npen, OEMGPU_LASSO);
    oemgpu_opts o;
    memset(&o, 0, sizeof o);
    o.npen = npen; o.penalty = pen.data(); o.nlambda = 100;
    MultiLay L;
    if (int rc = multi_layout("selftest_multi_plan", num_cu, layout == 0, n, p, m, &o, true, &L)) return rc;
    out[0] = L.xp.rows; out[1] = L.xp.nchunk; out[2] = L.xp.mb; out[3] = L.xp.npass; out[4] = L.sv.cap; out[5] = L.nsolve; out[6] = L.sv.engine;
    out[7] = (int64_t)(L.total + L.ws);
    return 0;
}

int oemgpu_selftest_multi_moments_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                                      int64_t y_rs, int64_t y_cs, int32_t m, double *moments_out_dev)
{
    const char *who = "selftest_multi_moments";
    const DenseSrc X = dtype < 0 ? dense_src_cm((const double *)x_dev, ld) : dense_src_rm(x_dev, dtype, ld);
    int rc = src_args_check(who, c, X, n, p, y_dev, moments_out_dev != nullptr);
    if (!rc) rc = multi_y_check(who, n, y_rs, y_cs, m);
    if (rc) return rc;
    if (!X.colmajor()) if ((rc = rm_p_refusal(who, p))) return rc;
    MultiLay L;
    if ((rc = multi_layout(who, c->num_cu, X.colmajor(), n, p, m, nullptr, false, &L))) return rc;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    ctx_void_cv(c);
    if (ctx_aux(c, L.total)) return OEMGPU_ERR_HIP;
    if (ctx_reserve(c, L.ws)) return OEMGPU_ERR_HIP;
    if ((rc = multi_passes(c, L, X, MultiY{y_dev, y_rs, y_cs}))) return rc;
    const size_t mlen = (size_t)oemgpu_moments_len(p);
    for (int r0 = 0; r0 < m; r0 += 4096) {
        const int nb = m - r0 < 4096 ? m - r0 : 4096;
        if ((rc = launch_multi_compose(c->stream, L.xp, (const double *)(c->aux + L.a_base), (const double *)(c->aux + L.a_part), r0, nb,
                                       moments_out_dev + mlen * r0))) return rc;
    }
    OEM_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// The call in three phases over one buffer layout in oemgpu_ctx::aux (a pure function of n, p, K, npen, nl and "weighted", so
// the phases may also be separate C-ABI calls with a collective between them: row shards on several GPUs, oemgpu_xval_*_dev):
//   prepare  rows into fold order, per-fold moments of the LOCAL rows           (additive over row shards)
//   solve    fold sums, the full-data fit and the K left-out-fold fits           (replicated; needs the moments of ALL rows)
//   cverr    per-observation error of the LOCAL rows, merged to (count, mean, M2) per (penalty, lambda)
struct XvalLay {
    int64_t n, ldp;
    int p, pm, K, npen, nl;
    CvErrPlan cv;                                                 // the CV-error launch of phase 3 (xval.hip: cv_error_plan)
    bool weighted;
    size_t mlen, cslen;
    GramPlan plmax;
    size_t a_cs, a_cnt, a_fn, a_bad, a_pos, a_xp, a_yp, a_mf, a_mc, a_ms, a_t, a_v, a_b, a_part, a_out, a_peer, total;
};
// sp (xval.oem on a sparse x): the fold segments start on multiples of CSC_CHUNK rows, there is no dense copy (a_xp and the peer
// staging are empty, the Gram scratch is that of one tile on the tile route and empty on the compressed-column route), the CV-error
// partials are one per wave of csr_cv_error_kernel; the sparse call's own regions follow at `total` (XvalSparsePlan's offsets)
static XvalLay xval_layout(int num_cu, int64_t n, int p, int K, int npen, int nl, bool weighted, const XvalSparsePlan *sp = nullptr)
{
    XvalLay L;
    L.n = n; L.p = p; L.K = K; L.npen = npen; L.nl = nl; L.weighted = weighted;
    L.ldp = sp ? sp->npad_max : (n + 16 * (int64_t)K + 15) / 16 * 16;
    // observation weights: the fold-ordered copy gets a leading column sqrt(w) and everything is scaled by sqrt(w), so the moment
    // kernels see pm = p + 1 data columns and their Gram IS X'WX with its intercept border (ref src/oem_xval_dense.h:486-623)
    L.pm = p + (weighted ? 1 : 0);
    L.mlen = (size_t)oemgpu_moments_len(L.pm); L.cslen = (size_t)p + 1;
    L.cv = cv_error_plan(n, p, K, npen, nl, num_cu);
    L.plmax = sp ? sp->plmax : gram_plan_bound(n, L.pm, num_cu);   // holds the moment plan of every fold
    Bump A;
    L.a_cs = A.take(sizeof(double) * L.cslen * (2 * (size_t)K + 1));      // per fold, then all folds / all but fold ff
    L.a_cnt = A.take(fold_layout_ints(n, K) * sizeof(int)); L.a_fn = A.take(sizeof(int64_t) * 2 * K); L.a_bad = A.take(256);
    L.a_pos = A.take(sizeof(int) * (size_t)n); L.a_xp = A.take(sp ? 0 : sizeof(double) * (size_t)L.ldp * L.pm);
    L.a_yp = A.take(sizeof(double) * (size_t)L.ldp); L.a_mf = A.take(sizeof(double) * L.mlen * K);
    L.a_mc = A.take(sizeof(double) * L.mlen); L.a_ms = A.take(sizeof(double) * L.mlen * (K + 1));
    L.a_t = A.take(L.plmax.tpart_doubles * 8); L.a_v = A.take(L.plmax.vpart_doubles * 8);
    L.a_b = A.take(sizeof(double) * (size_t)K * npen * nl * (p + 1));
    L.a_part = A.take(sizeof(double) * (sp ? (size_t)sp->cv_waves * npen * sp->nl16 * 4 : cv_part_doubles(L.cv.nwg, K, npen, nl))); L.a_out = A.take(sizeof(double) * 3 * (size_t)npen * nl);
    L.a_peer = A.take(sp ? 0 : sizeof(double) * (L.mlen + L.cslen) * K);   // another device's fold moments on their way into the sum
    L.total = A.off;
    return L;
}
static XvalLay xval_layout(oemgpu_ctx *c, int64_t n, int p, int K, int npen, int nl, bool weighted)
{
    return xval_layout(c->num_cu, n, p, K, npen, nl, weighted);
}

// what every phase needs of the rows and folds, whether or not it fits anything
static int xval_check_rows(int64_t n, int64_t ld, int K, int type_measure)
{
    if (K < 2 || K > 512) { set_error("xval_dense: nfolds must be in 2..512"); return OEMGPU_ERR_ARG; }
    if (type_measure != 0 && type_measure != 1) { set_error("xval_dense: type_measure must be 0 (mse) or 1 (mae)"); return OEMGPU_ERR_ARG; }
    if (n < 1 || ld < n) { set_error("xval_dense: bad n / ld"); return OEMGPU_ERR_ARG; }
    if (n + 16 * (int64_t)K >= (int64_t)1 << 31) { set_error("xval_dense: n too large for 32-bit row positions"); return OEMGPU_ERR_UNSUPPORTED; }
    return 0;
}

static int xval_check(oemgpu_ctx *c, const void *x_dev, const void *y_dev, const void *foldid_dev, int64_t n, int64_t ld, int p, int K,
                      int intercept, int type_measure, bool weighted, const oemgpu_opts *o)
{
    if (!o) { set_error("xval_dense: NULL argument"); return OEMGPU_ERR_ARG; }
    (void)c; (void)x_dev; (void)y_dev; (void)foldid_dev;
    if (intercept >= 0) {                                          // (< 0: a phase that does not solve; the options were checked by the one that does)
        int rc = check_opts(o, p, p + (intercept ? 1 : 0));
        if (rc) return rc;
    } else if (!o->penalty || o->npen < 1) { set_error("xval_dense: no penalty"); return OEMGPU_ERR_ARG; }
    int rc = xval_check_rows(n, ld, K, type_measure);
    if (rc) return rc;
    if (weighted && o->compute_loss) {
        set_error("compute.loss with observation weights: the reference's loss is the unweighted residual sum (src/oem_xval_dense.h:1122-1145), "
                  "which the weighted Gram does not hold");
        return OEMGPU_ERR_UNSUPPORTED;
    }
    return 0;
}

// phase 1: hf <- the local fold sizes [K] and fold starts [K]; mfold (and csq) in aux <- the local rows' per-fold moments
static int xval_fold_moments(oemgpu_ctx *c, const XvalLay &L, const std::vector<int64_t> &hf, const double *sums);
static int xval_prepare(oemgpu_ctx *c, const XvalLay &L, const DenseSrc &X, const double *y_dev, const double *w_dev,
                        const int32_t *foldid_dev, std::vector<int64_t> &hf, bool moments = true)
{
    const int64_t n = L.n;
    const int K = L.K, p = L.p;
    char *ax = c->aux;
    int *blockcnt = (int *)(ax + L.a_cnt), *bad = (int *)(ax + L.a_bad), *pos = (int *)(ax + L.a_pos);
    int64_t *fold_n = (int64_t *)(ax + L.a_fn), *fold_start = fold_n + K;
    double *xp = (double *)(ax + L.a_xp), *yp = (double *)(ax + L.a_yp);
    // ---- rows into fold order (whatever cv.oem's layout stamp vouched for is overwritten from here on: cv_lay_out stamps again)
    ctx_void_cv(c);
    hf.assign(2 * K, 0);
    int hbad = 0, rc;
    {
        Timer t(c, OEMGPU_T_FOLDORDER);
        rc = launch_fold_layout(c->stream, foldid_dev, n, K, blockcnt, fold_n, fold_start, pos, bad);
        if (rc) return rc;
        OEM_HIP(hipMemcpyAsync(hf.data(), fold_n, sizeof(int64_t) * 2 * K, hipMemcpyDeviceToHost, c->stream));
        OEM_HIP(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        double *csq = (double *)(ax + L.a_cs);
        if (w_dev) {
            rc = launch_gather_rows(c->stream, w_dev, n, n, 1, y_dev, pos, xp, L.ldp, yp);               // column 0 <- w
            if (!rc) rc = dense_src_gather(c->stream, X, n, p, y_dev, foldid_dev, K, pos, xp + L.ldp, L.ldp, yp);
            if (!rc) rc = launch_weight_scale(c->stream, xp, L.ldp, yp, p, K, fold_start, fold_n, csq);
        } else rc = dense_src_gather(c->stream, X, n, p, y_dev, foldid_dev, K, pos, xp, L.ldp, yp);
        if (rc) return rc;
    }
    OEM_HIP(hipStreamSynchronize(c->stream));
    if (hbad) { set_error("xval_dense: foldid must hold values in 1..nfolds"); return OEMGPU_ERR_ARG; }
    // ---- per-fold moments about 0 (ref src/oem_xval_dense.h:358-484)
    return moments ? xval_fold_moments(c, L, hf, nullptr) : 0;
}

// mfold in aux <- the moments of every fold segment of the fold-ordered rows, one MFMA pass each, about 0 or about the shift that
// `sums` (device: oemgpu_shift_sums_dev's layout) yields -- the same sums for every fold, so that the buffers stay additive
static int xval_fold_moments(oemgpu_ctx *c, const XvalLay &L, const std::vector<int64_t> &hf, const double *sums)
{
    const int K = L.K;
    char *ax = c->aux;
    const double *xp = (const double *)(ax + L.a_xp), *yp = (const double *)(ax + L.a_yp);
    double *mfold = (double *)(ax + L.a_mf);
    for (int k = 0; k < K; ++k) {
        const int64_t nk = hf[k], st = hf[K + k];
        if (nk == 0) { OEM_HIP(hipMemsetAsync(mfold + L.mlen * k, 0, sizeof(double) * L.mlen, c->stream)); continue; }
        const GramPlan pl = gram_plan(nk, L.pm, c->num_cu);
        if (pl.tpart_doubles > L.plmax.tpart_doubles || pl.vpart_doubles > L.plmax.vpart_doubles) {
            set_error("internal: fold plan larger than its scratch"); return OEMGPU_ERR_INTERNAL;
        }
        int rc = shard_moments(c, pl, xp + st, nk, L.ldp, yp + st, sums, (double *)(ax + L.a_t), (double *)(ax + L.a_v), mfold + L.mlen * k);
        if (rc) return rc;
    }
    return 0;
}

// phase 2: mfold (and csq) in aux hold the per-fold moments of ALL rows; fold_tot[K] their fold sizes, n_tot the row count.
// The full-data fit (ff = 0) and one fit per left-out fold on the lambdas of the first (ref src/oem_xval_dense.cpp:213-340);
// the fold coefficients end in aux (bdev) for phase 3.
static int xval_fold_sizes_check(int K, int p, const int64_t *fold_tot, int64_t n_tot)
{
    if (n_tot <= p) { set_error("dimension of x larger than number of observations"); return OEMGPU_ERR_UNSUPPORTED; }   // ref src/oem_xval_dense.h:690-731
    for (int k = 0; k < K; ++k)
        if (n_tot - fold_tot[k] <= p) { set_error("dimension of x larger than number of observations"); return OEMGPU_ERR_UNSUPPORTED; }  // ref :849-852
    return 0;
}

static int xval_solve_sums(oemgpu_ctx *c, const XvalLay &L, double *msum, const double *cssum, double *bdev, int32_t standardize, int32_t intercept,
                           const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d);
static int xval_solve(oemgpu_ctx *c, const XvalLay &L, const int64_t *fold_tot, int64_t n_tot, int32_t standardize, int32_t intercept,
                      const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    const int K = L.K;
    const size_t mlen = L.mlen, cslen = L.cslen;
    const bool weighted = L.weighted;
    char *ax = c->aux;
    double *mfold = (double *)(ax + L.a_mf);
    double *csq = (double *)(ax + L.a_cs), *cssum = csq + cslen * K;
    int rc = xval_fold_sizes_check(K, L.p, fold_tot, n_tot);
    if (rc) return rc;
    double *msum = (double *)(ax + L.a_ms);                      // [K + 1]: all folds, then all but fold ff
    for (int ff = 0; ff <= K; ++ff) {
        rc = launch_fold_sum(c->stream, mfold, K, mlen, ff, msum + mlen * ff);
        if (!rc && weighted) rc = launch_fold_sum(c->stream, csq, K, cslen, ff, cssum + cslen * ff);
        if (rc) return rc;
    }
    return xval_solve_sums(c, L, msum, cssum, (double *)(ax + L.a_b), standardize, intercept, o, beta, lambda_out, niter, loss, d);
}

// The K + 1 fits of ONE response from its sums msum[K + 1] (all folds, then all but fold ff; device, outside the workspace; weighted: cssum
// alike): the full-data fit into the outputs, the K fold fits on its lambdas into bdev[K][npen][nl][p + 1] (device) for phase 3.
// xval_solve ends here, and so does every response of oemgpu_xval_dense_multi_dev that no batched launch takes (route 1).
static int xval_solve_sums(oemgpu_ctx *c, const XvalLay &L, double *msum, const double *cssum, double *bdev, int32_t standardize, int32_t intercept,
                           const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    const int K = L.K, p = L.p, npen = L.npen, nl = L.nl, q = p + (intercept ? 1 : 0);
    const size_t mlen = L.mlen, cslen = L.cslen;
    const bool weighted = L.weighted;
    int rc = 0;
    const size_t blen = (size_t)npen * nl * (p + 1), nk2 = (size_t)npen * nl;
    std::vector<double> hb(blen * K);
    const bool coop_batch = q > SMALL_P_MAX && path_coop_eligible(q, false, o->compute_loss != 0, any_grp_count(o), K + 1) &&
                            path_coop_workgroups(q) * (K + 1) <= c->num_cu * 3 / 4;
    if (q <= SMALL_P_MAX || coop_batch) {
        // The K + 1 fits are independent chains of tiny dependent steps: ONE launch, one workgroup (set) per fit.  (K streams
        // would run four at a time: the hardware queues are few.)  The folds' lambda grid is the full fit's, which a fold's
        // kernel derives from the full-data X'Y itself (PathArgs::lmax_xy) instead of waiting for the full fit to end.
        std::vector<double> ab(blen * (K + 1)), al(nk2 * (K + 1)), aloss(nk2 * (K + 1)), ad(K + 1);
        std::vector<int32_t> an(nk2 * (K + 1));
        rc = solve_moments_batch(c, msum, mlen, K + 1, p, OEMGPU_SEM_XVAL, standardize, intercept, o, ab.data(), al.data(), an.data(),
                                 aloss.data(), ad.data(), true, weighted ? cssum : nullptr, cslen);
        if (rc) return rc;
        memcpy(beta, ab.data(), sizeof(double) * blen);
        memcpy(lambda_out, al.data(), sizeof(double) * nk2);
        memcpy(niter, an.data(), sizeof(int32_t) * nk2);
        memcpy(loss, aloss.data(), sizeof(double) * nk2);       // the reference reports the loss of the full fit only (ref :296-301)
        *d = ad[0];
        memcpy(hb.data(), ab.data() + blen, sizeof(double) * blen * K);
    } else if (weighted) {
        // weighted and beyond one launch's size: the K + 1 fits one after the other on this context (each a cooperating-workgroup
        // or launch-per-iteration solve of its own), the folds on the full fit's lambdas
        rc = solve_moments_batch(c, msum, mlen, 1, p, OEMGPU_SEM_XVAL, standardize, intercept, o, beta, lambda_out, niter, loss, d, false,
                                 cssum, cslen);
        if (rc) return rc;
        oemgpu_opts of = *o;
        of.lambda_user = lambda_out; of.nlambda_user = nl; of.compute_loss = 0;
        std::vector<double> hl(nk2), hloss(nk2);
        std::vector<int32_t> hn(nk2);
        double hd = 0.0;
        for (int ff = 1; ff <= K; ++ff) {
            rc = solve_moments_batch(c, msum + mlen * ff, mlen, 1, p, OEMGPU_SEM_XVAL, standardize, intercept, &of, hb.data() + blen * (ff - 1),
                                     hl.data(), hn.data(), hloss.data(), &hd, false, cssum + cslen * ff, cslen);
            if (rc) return rc;
        }
    } else {
        rc = oemgpu_solve_moments_dev(c, msum, nullptr, p, OEMGPU_SEM_XVAL, standardize, intercept, o, beta, lambda_out, niter, loss, d);
        if (rc) return rc;
        oemgpu_opts of = *o;
        of.lambda_user = lambda_out; of.nlambda_user = nl; of.compute_loss = 0;
        // The fold fits run on K worker threads: they must never call back into the caller (R's API is single-threaded, and
        // R_CheckStack on a foreign stack raises a spurious interrupt -- ADVICE r2).  The caller is polled on THIS thread only:
        // by the full-data fit above, before the fold threads start and after they have joined.
        of.interrupt = nullptr; of.interrupt_arg = nullptr;
        if (o->interrupt && o->interrupt(o->interrupt_arg)) { set_error("interrupted by the caller"); return OEMGPU_ERR_INTERRUPTED; }
        std::vector<double> hl(nk2 * K), hloss(nk2 * K), hd(K);
        std::vector<int32_t> hn(nk2 * K);
        msum += mlen;                                            // the folds' sums
        while ((int)c->kids.size() < K) {
            oemgpu_ctx *kid = oemgpu_create(c->device, nullptr);
            if (!kid) return OEMGPU_ERR_HIP;
            c->kids.push_back(kid);
        }
        if (!c->fork_ev) OEM_HIP(hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));
        OEM_HIP(hipEventRecord(c->fork_ev, c->stream));
        for (int ff = 1; ff <= K; ++ff) OEM_HIP(hipStreamWaitEvent(c->kids[ff - 1]->stream, c->fork_ev, 0));
        {
            std::vector<int> rcs(K, 0);
            std::vector<std::string> errs(K);
            std::vector<std::thread> th;
            th.reserve(K);
            for (int ff = 1; ff <= K; ++ff)
                th.emplace_back([&, ff]() {
                    const int i = ff - 1;
                    rcs[i] = oemgpu_solve_moments_dev(c->kids[i], msum + mlen * i, nullptr, p, OEMGPU_SEM_XVAL, standardize, intercept, &of,
                                                      hb.data() + blen * i, hl.data() + nk2 * i, hn.data() + nk2 * i, hloss.data() + nk2 * i,
                                                      &hd[i]);
                    if (rcs[i]) errs[i] = oemgpu_last_error();          // the message lives in this thread
                });
            for (auto &t : th) t.join();
            for (int i = 0; i < K; ++i)
                if (rcs[i]) { set_error("fold %d: %s", i + 1, errs[i].c_str()); return rcs[i]; }
            if (o->interrupt && o->interrupt(o->interrupt_arg)) { set_error("interrupted by the caller"); return OEMGPU_ERR_INTERRUPTED; }
        }
    }
    OEM_HIP(hipMemcpyAsync(bdev, hb.data(), sizeof(double) * blen * K, hipMemcpyHostToDevice, c->stream));
    OEM_HIP(hipStreamSynchronize(c->stream));                   // hb is a local
    return 0;
}

// phase 3: per-observation error of every LOCAL row under the fit that left its fold out (ref src/oem_xval_dense.cpp:343-461).
// triples == nullptr: cvm / cvsd of these rows (they are all rows); else triples[npen][nl][3] <- (count, mean, M2 = sum (v - mean)^2),
// which the caller merges over the row shards (oemgpu_xval_merge).
static int xval_cverr(oemgpu_ctx *c, const XvalLay &L, int32_t type_measure, const oemgpu_opts *o, double *cvm, double *cvsd, double *triples)
{
    const int K = L.K, p = L.p, npen = L.npen, nl = L.nl;
    char *ax = c->aux;
    int64_t *fold_n = (int64_t *)(ax + L.a_fn), *fold_start = fold_n + K;
    double *xp = (double *)(ax + L.a_xp), *yp = (double *)(ax + L.a_yp), *bdev = (double *)(ax + L.a_b);
    double *part = (double *)(ax + L.a_part), *cvout = (double *)(ax + L.a_out);
    int rc = launch_cv_error(c->stream, xp, L.ldp, yp, fold_start, fold_n, K, p, bdev, npen, nl, type_measure, L.weighted ? 1 : 0, L.cv, (double)L.n,
                             part, cvout, triples != nullptr);
    if (rc) return rc;
    const int per = triples ? 3 : 2;
    std::vector<double> hc((size_t)per * npen * nl);
    OEM_HIP(hipMemcpyAsync(hc.data(), cvout, sizeof(double) * hc.size(), hipMemcpyDeviceToHost, c->stream));
    OEM_HIP(hipStreamSynchronize(c->stream));
    if (triples) { memcpy(triples, hc.data(), sizeof(double) * hc.size()); return 0; }
    for (int k = 0; k < npen; ++k) {
        const int nlam = (o->penalty[k] == OEMGPU_OLS) ? 1 : nl;
        for (int i = 0; i < nl; ++i) {
            const size_t ki = (size_t)k * nl + i;
            cvm[ki] = i < nlam ? hc[2 * ki] : 0.0;
            cvsd[ki] = i < nlam ? hc[2 * ki + 1] : 0.0;
        }
    }
    return 0;
}

// xval.oem on a dense x wherever it lies: everything behind the fold-ordered copy is the same, and so are the results, bit for bit
static int xval_dense_src(const char *who, oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const double *y_dev,
                          const double *w_dev, const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept,
                          int32_t type_measure, const oemgpu_opts *o,
                          double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, double *cvm, double *cvsd)
{
    if (!c || !X.x || !y_dev || !foldid_dev || !beta || !lambda_out || !niter || !loss || !d || !cvm || !cvsd) {
        set_error("xval_dense: NULL argument"); return OEMGPU_ERR_ARG;
    }
    const int K = nfolds;
    int rc = dense_src_check(who, X, n, p);
    if (!rc) rc = xval_check(c, X.x, y_dev, foldid_dev, n, n, p, K, intercept, type_measure, w_dev != nullptr, o);
    if (rc) return rc;
    if (n <= p) { set_error("dimension of x larger than number of observations"); return OEMGPU_ERR_UNSUPPORTED; }   // ref src/oem_xval_dense.h:690-731
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const XvalLay L = xval_layout(c, n, p, K, o->npen, nl_of(o), w_dev != nullptr);
    if (ctx_aux(c, L.total)) return OEMGPU_ERR_HIP;
    std::vector<int64_t> hf;
    rc = xval_prepare(c, L, X, y_dev, w_dev, foldid_dev, hf);
    if (!rc) rc = xval_solve(c, L, hf.data(), n, standardize, intercept, o, beta, lambda_out, niter, loss, d);
    if (!rc) rc = xval_cverr(c, L, type_measure, o, cvm, cvsd, nullptr);
    return rc;
}

int oemgpu_xval_dense_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                          const double *w_dev, const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept,
                          int32_t type_measure, const oemgpu_opts *o,
                          double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, double *cvm, double *cvsd)
{
    return xval_dense_src("xval_dense", c, dense_src_cm(x_dev, ld), n, p, y_dev, w_dev, foldid_dev, nfolds, standardize, intercept, type_measure, o, beta,
                          lambda_out, niter, loss, d, cvm, cvsd);
}

// oemgpu_xval_dense_dev with the rows gathered from a row-major x where it lies (xval.hip: fold_gather_rm_kernel)
int oemgpu_xval_dense_rm_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                             const double *w_dev, const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept,
                             int32_t type_measure, const oemgpu_opts *o,
                             double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, double *cvm, double *cvsd)
{
    return xval_dense_src("xval_dense_rm", c, dense_src_rm(x_dev, dtype, ldr), n, p, y_dev, w_dev, foldid_dev, nfolds, standardize, intercept,
                          type_measure, o, beta, lambda_out, niter, loss, d, cvm, cvsd);
}

// ---------------------------------------------------------------------------------------------- xval.oem for many responses on one x
//   What depends on x alone is made once -- the fold layout, the fold-ordered copy xp, the K fold Gram passes (response 0
// riding as y) -- and so is one X'Y pass over the fold-ordered rows for all m responses (multi.hip, fold-segmented).  Per solve chunk of nb
// responses: the nb (K + 1) composed sums in one launch, their paths in one batched launch (instance r (K + 1) + ff, every response's
// fits on ITS full-data lambda grid: PathArgs::lmax_group), the CV error of the nb responses in one launch and one finish launch.
// The buffers: XvalLay's for the shared part, then the regions below, in oemgpu_ctx::aux.
struct XvalMultiLay {
    XvalLay L;
    MultiPlan xp;                                                 // the X'Y pass: blocks, groups, rows per chunk
    MultiSolve sv;
    CvErrPlan cv;                                                 // the CV-error launch of nb responses
    int nb = 1, nsolve = 0, route = 1;
    size_t b_col = 0, b_yp = 0, b_cf = 0, b_part = 0, b_comp = 0, b_tab = 0, b_cvpart = 0, b_cvout = 0;       // bytes
    size_t a_col = 0, a_yp = 0, a_cf = 0, a_part = 0, a_comp = 0, a_tab = 0, a_cvpart = 0, a_cvout = 0, total = 0;
};
// nb_limit > 0: no more responses per chunk than that (the device's free memory)
// dense_sem (cv_oem_multi): the solves are oem()'s (OEMGPU_SEM_DENSE: the intercept is centred out, q = p)
// nb_exact > 0 (a call that solves nothing: the scoring self-test): that many responses per chunk, whatever the solve plan holds
static XvalMultiLay xval_multi_layout(int num_cu, int64_t n, int p, int K, int m, int intercept, const oemgpu_opts *o, int nb_limit,
                                      bool dense_sem = false, int nb_exact = 0)
{
    XvalMultiLay V;
    const int npen = o->npen, nl = nl_of(o), q = p + ((intercept && !dense_sem) ? 1 : 0);
    V.L = xval_layout(num_cu, n, p, K, npen, nl, false);
    V.xp = multi_plan(n, p, m, num_cu);
    V.sv = multi_solve_plan(num_cu, q, npen, any_grp_count(o));
    // route 0: nb = floor(cap / (K + 1)) responses per batched launch; route 1: no batch engine takes the shape, or not even one
    // response's K + 1 instances fit a launch -- every response's sums then go through xval_solve_sums, as xval.oem's do
    V.route = (V.sv.engine != OEMGPU_ENGINE_NONE && V.sv.cap >= K + 1) ? 0 : 1;
    int nb = V.route == 0 ? V.sv.cap / (K + 1) : 1;
    if (nb_exact > 0) nb = nb_exact;
    if (nb > m) nb = m;
    if (nb_limit > 0 && nb > nb_limit) nb = nb_limit;
    V.nb = nb; V.nsolve = (m + nb - 1) / nb;
    V.cv = cv_error_plan_many(n, p, K, npen, nl, nb, num_cu);
    V.b_col = (size_t)n * 8;                                                       // response 0 as a contiguous vector (a row-major Y)
    V.b_yp = (size_t)V.L.ldp * m * 8;                                              // Yp: the responses in fold order, column-major
    V.b_cf = (size_t)(K + 1) * sizeof(int);                                        // first chunk of every fold
    V.b_part = multi_fold_part_doubles(V.xp, K) * 8;                               // the X'Y panels of every (fold) chunk
    V.b_comp = (size_t)nb * (K + 1) * V.L.mlen * 8;                                // one chunk's composed sums
    V.b_tab = (size_t)nb * K * npen * nl * (p + 1) * 8;                            // its fold tables
    V.b_cvpart = (size_t)nb * cv_part_doubles(V.cv.nwg, K, npen, nl) * 8;          // its CV-error partials
    V.b_cvout = (size_t)nb * 2 * npen * nl * 8;                                    // (cvm, cvsd)
    Bump A;
    A.off = V.L.total;
    V.a_col = A.take(V.b_col); V.a_yp = A.take(V.b_yp); V.a_cf = A.take(V.b_cf); V.a_part = A.take(V.b_part);
    V.a_comp = A.take(V.b_comp); V.a_tab = A.take(V.b_tab); V.a_cvpart = A.take(V.b_cvpart); V.a_cvout = A.take(V.b_cvout);
    V.total = A.off;
    return V;
}

// HIP-event times of the last call's phases on this thread (oemgpu_set_timing on; added over the solve chunks; the clock waits for
// every phase's end, so the timed call is not the fast one): fold order and gathers, fold Gram passes, fold X'Y, composition, paths, CV error
static thread_local double g_xvm_ms[OEMGPU_XVM_NPHASES] = {0, 0, 0, 0, 0, 0};
struct XvmClock {
    oemgpu_ctx *c;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool on;
    double *ms;                                                   // the phase sums: xval_oem_multi's, or cv_oem_multi's (their first three phases are the same)
    explicit XvmClock(oemgpu_ctx *c_, double *ms_ = g_xvm_ms) : c(c_), on(c_->timing), ms(ms_)
    {
        if (on && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) on = false;
    }
    ~XvmClock() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    void begin() { if (on) (void)hipEventRecord(e0, c->stream); }
    void end(int phase)
    {
        if (!on) return;
        float f = 0.f;
        (void)hipEventRecord(e1, c->stream);
        if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&f, e0, e1) == hipSuccess) ms[phase] += f;
    }
};

// phases 1-3: the rows of x and Y into fold order, the K fold Gram passes, the fold X'Y pass.  hf <- fold sizes [K] and starts [K].
static int xval_multi_passes(oemgpu_ctx *c, const XvalMultiLay &V, const DenseSrc &X, const MultiY &Y, const int32_t *foldid_dev, int m,
                             std::vector<int64_t> &hf, XvmClock &clk)
{
    const XvalLay &L = V.L;
    const int K = L.K;
    char *ax = c->aux;
    double *col = (double *)(ax + V.a_col), *Yp = (double *)(ax + V.a_yp), *part = (double *)(ax + V.a_part);
    int *cfirst = (int *)(ax + V.a_cf);
    const int64_t *fold_n = (const int64_t *)(ax + L.a_fn), *fold_start = fold_n + K;
    const double *y0 = Y.y;                                          // response 0 rides along as y
    int rc = 0;
    clk.begin();
    if (Y.rs != 1) { if ((rc = launch_multi_column(c->stream, Y, L.n, 0, col))) return rc; y0 = col; }
    if ((rc = xval_prepare(c, L, X, y0, nullptr, foldid_dev, hf, false))) return rc;         // (waits: the fold ids are valid from here on)
    if ((rc = launch_gather_responses(c->stream, Y.y, Y.rs, Y.cs, L.n, m, (const int *)(ax + L.a_pos), Yp, L.ldp))) return rc;
    clk.end(0);
    clk.begin();
    if ((rc = xval_fold_moments(c, L, hf, nullptr))) return rc;
    clk.end(1);
    // the chunks of the X'Y pass from the fold sizes: none straddles a fold, an empty fold has none
    std::vector<int> cf(K + 1, 0);
    for (int k = 0; k < K; ++k) {
        const int64_t nc = (hf[k] + V.xp.rows - 1) / V.xp.rows;
        if (cf[k] + nc > multi_fold_chunks_max(V.xp, K)) { set_error("internal: fold chunks beyond their scratch"); return OEMGPU_ERR_INTERNAL; }
        cf[k + 1] = cf[k] + (int)nc;
    }
    OEM_HIP(hipMemcpyAsync(cfirst, cf.data(), sizeof(int) * (K + 1), hipMemcpyHostToDevice, c->stream));
    OEM_HIP(hipStreamSynchronize(c->stream));                        // cf is a local
    clk.begin();
    rc = launch_multi_fold_xty(c->stream, V.xp, K, cf[K], (const double *)(ax + L.a_xp), L.ldp, Yp, fold_start, fold_n, cfirst, part);
    clk.end(2);
    return rc;
}

static int xval_dense_multi_src(const char *who, oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const double *y_dev, int64_t rs, int64_t cs,
                                int32_t m, const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept, int32_t type_measure,
                                const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, double *cvm,
                                double *cvsd, int32_t *route)
{
    if (!c || !X.x || !y_dev || !foldid_dev || !beta || !lambda_out || !niter || !loss || !d || !cvm || !cvsd || !route) {
        set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG;
    }
    const int K = nfolds;
    int rc = dense_src_check(who, X, n, p);
    if (!rc) rc = xval_check(c, X.x, y_dev, foldid_dev, n, n, p, K, intercept, type_measure, false, o);
    if (!rc) rc = multi_y_check(who, n, rs, cs, m);
    if (rc) return rc;
    // the largest fold holds at least ceil(n / K) rows: its fit would keep n - that <= p of them (ref src/oem_xval_dense.h:690-731, 849-852)
    if (n <= p || n - (n + K - 1) / K <= p) { set_error("dimension of x larger than number of observations"); return OEMGPU_ERR_UNSUPPORTED; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    XvalMultiLay V = xval_multi_layout(c->num_cu, n, p, K, m, intercept, o, 0);
    {   // one chunk's sums, tables and partials grow with nb: fewer responses per chunk rather than an allocation that fails
        size_t fre = 0, tot = 0;
        if (hipMemGetInfo(&fre, &tot) == hipSuccess)
            while (V.nb > 1 && V.total > fre + c->aux_bytes) V = xval_multi_layout(c->num_cu, n, p, K, m, intercept, o, V.nb / 2);
    }
    if (ctx_aux(c, V.total)) return OEMGPU_ERR_HIP;
    for (double &v : g_xvm_ms) v = 0.0;
    XvmClock clk(c);
    const XvalLay &L = V.L;
    std::vector<int64_t> hf;
    if ((rc = xval_multi_passes(c, V, X, MultiY{y_dev, rs, cs}, foldid_dev, m, hf, clk))) return rc;
    if ((rc = xval_fold_sizes_check(K, p, hf.data(), n))) return rc;
    char *ax = c->aux;
    const int npen = L.npen, nl = L.nl;
    const size_t mlen = L.mlen, blen = (size_t)npen * nl * (p + 1), nk2 = (size_t)npen * nl;
    const double *mfold = (const double *)(ax + L.a_mf), *part = (const double *)(ax + V.a_part), *Yp = (const double *)(ax + V.a_yp);
    const int *cfirst = (const int *)(ax + V.a_cf);
    const int64_t *fold_n = (const int64_t *)(ax + L.a_fn), *fold_start = fold_n + K;
    double *comp = (double *)(ax + V.a_comp), *tab = (double *)(ax + V.a_tab), *cvpart = (double *)(ax + V.a_cvpart), *cvout = (double *)(ax + V.a_cvout);
    auto interrupted = [&]() {
        if (!(o->interrupt && o->interrupt(o->interrupt_arg))) return false;
        set_error("interrupted by the caller");
        return true;
    };
    std::vector<double> ab, al, aloss, ad, hb, hc;
    std::vector<int32_t> an;
    for (int r0 = 0; r0 < m; r0 += V.nb) {
        const int nb = m - r0 < V.nb ? m - r0 : V.nb, ninst = nb * (K + 1);
        if (r0 > 0 && interrupted()) return OEMGPU_ERR_INTERRUPTED;
        clk.begin();
        if ((rc = launch_multi_fold_compose(c->stream, V.xp, K, mfold, part, cfirst, r0, nb, false, comp))) return rc;
        clk.end(3);
        clk.begin();
        if (V.route == 0) {
            // instance b (K + 1) + ff: response r0 + b, all folds (ff = 0) or all but fold ff, on the lambda grid of instance b (K + 1)
            ab.resize(blen * ninst); al.resize(nk2 * ninst); an.resize(nk2 * ninst); aloss.resize(nk2 * ninst); ad.resize(ninst); hb.resize(blen * K * nb);
            rc = solve_moments_batch(c, comp, mlen, ninst, p, OEMGPU_SEM_XVAL, standardize, intercept, o, ab.data(), al.data(), an.data(), aloss.data(),
                                     ad.data(), true, nullptr, 0, nullptr, K + 1);
            if (rc) return rc;
            for (int b = 0; b < nb; ++b) {
                const size_t i0 = (size_t)b * (K + 1), r = (size_t)r0 + b;
                memcpy(beta + blen * r, ab.data() + blen * i0, sizeof(double) * blen);
                memcpy(lambda_out + nk2 * r, al.data() + nk2 * i0, sizeof(double) * nk2);
                memcpy(niter + nk2 * r, an.data() + nk2 * i0, sizeof(int32_t) * nk2);
                memcpy(loss + nk2 * r, aloss.data() + nk2 * i0, sizeof(double) * nk2);          // the full fit's (ref src/oem_xval_dense.cpp:296-301)
                d[r] = ad[i0];
                memcpy(hb.data() + blen * K * b, ab.data() + blen * (i0 + 1), sizeof(double) * blen * K);
                route[r] = 0;
            }
            OEM_HIP(hipMemcpyAsync(tab, hb.data(), sizeof(double) * blen * K * nb, hipMemcpyHostToDevice, c->stream));
        } else {
            rc = xval_solve_sums(c, L, comp, nullptr, tab, standardize, intercept, o, beta + blen * r0, lambda_out + nk2 * r0, niter + nk2 * r0,
                                 loss + nk2 * r0, d + r0);
            if (rc) return rc;
            route[r0] = 1;
        }
        clk.end(4);
        clk.begin();
        rc = launch_cv_error_many(c->stream, (const double *)(ax + L.a_xp), L.ldp, Yp + (size_t)L.ldp * r0, fold_start, fold_n, K, p, tab, npen, nl,
                                  type_measure, V.cv, (double)n, nb, cvpart, cvout);
        if (rc) return rc;
        hc.resize(2 * nk2 * nb);
        OEM_HIP(hipMemcpyAsync(hc.data(), cvout, sizeof(double) * hc.size(), hipMemcpyDeviceToHost, c->stream));
        OEM_HIP(hipStreamSynchronize(c->stream));                    // hb and hc are read and written by the copies above
        clk.end(5);
        for (int b = 0; b < nb; ++b)
            for (int k = 0; k < npen; ++k) {
                const int nlam = (o->penalty[k] == OEMGPU_OLS) ? 1 : nl;
                for (int i = 0; i < nl; ++i) {
                    const size_t ki = (size_t)k * nl + i, src = 2 * (nk2 * b + ki), dst = nk2 * ((size_t)r0 + b) + ki;
                    cvm[dst] = i < nlam ? hc[src] : 0.0;
                    cvsd[dst] = i < nlam ? hc[src + 1] : 0.0;
                }
            }
    }
    return 0;
}

int oemgpu_xval_dense_multi_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev, int64_t y_rs, int64_t y_cs,
                                int32_t m, const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept, int32_t type_measure,
                                const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, double *cvm,
                                double *cvsd, int32_t *route)
{
    return xval_dense_multi_src("xval_dense_multi", c, dense_src_cm(x_dev, ld), n, p, y_dev, y_rs, y_cs, m, foldid_dev, nfolds, standardize, intercept,
                                type_measure, o, beta, lambda_out, niter, loss, d, cvm, cvsd, route);
}

int oemgpu_xval_dense_multi_rm_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev, int64_t y_rs,
                                   int64_t y_cs, int32_t m, const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept,
                                   int32_t type_measure, const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss,
                                   double *d, double *cvm, double *cvsd, int32_t *route)
{
    return xval_dense_multi_src("xval_dense_multi_rm", c, dense_src_rm(x_dev, dtype, ldr), n, p, y_dev, y_rs, y_cs, m, foldid_dev, nfolds, standardize,
                                intercept, type_measure, o, beta, lambda_out, niter, loss, d, cvm, cvsd, route);
}

int oemgpu_last_xval_multi_timings(double *ms)
{
    if (!ms) { set_error("last_xval_multi_timings: NULL argument"); return OEMGPU_ERR_ARG; }
    for (int i = 0; i < OEMGPU_XVM_NPHASES; ++i) ms[i] = g_xvm_ms[i];
    return 0;
}

int oemgpu_selftest_xval_multi_plan(int64_t n, int32_t p, int32_t nfolds, int32_t m, int32_t npen, int32_t nl, int32_t num_cu, int64_t *out)
{
    if (n < 1 || p < 1 || m < 1 || npen < 1 || nl < 1 || num_cu < 1 || !out) { set_error("selftest_xval_multi_plan: bad argument"); return OEMGPU_ERR_ARG; }
    if (int rc = xval_check_rows(n, n, nfolds, 0)) return rc;
    if (n <= p) { set_error("selftest_xval_multi_plan: n <= p, which the call does not serve"); return OEMGPU_ERR_UNSUPPORTED; }
    std::vector<int32_t> pen(npen, OEMGPU_LASSO);
    oemgpu_opts o;
    memset(&o, 0, sizeof o);
    o.npen = npen; o.penalty = pen.data(); o.nlambda = nl;
    const XvalMultiLay V = xval_multi_layout(num_cu, n, p, nfolds, m, 1, &o, 0);
    const int64_t v[OEMGPU_XVM_PLAN_LEN] = {V.nb, V.nsolve, V.sv.engine, V.route, V.xp.rows, multi_fold_chunks_max(V.xp, nfolds), V.xp.npass, V.xp.mb, V.cv.nwg,
                                            (int64_t)V.L.total, (int64_t)V.b_col, (int64_t)V.b_yp, (int64_t)V.b_cf, (int64_t)V.b_part, (int64_t)V.b_comp,
                                            (int64_t)V.b_tab, (int64_t)V.b_cvpart, (int64_t)V.b_cvout, (int64_t)V.total, V.sv.cap};
    for (int i = 0; i < OEMGPU_XVM_PLAN_LEN; ++i) out[i] = v[i];
    return 0;
}

int oemgpu_selftest_xval_multi_fold_moments_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                                                int64_t y_rs, int64_t y_cs, int32_t m, const int32_t *foldid_dev, int32_t nfolds, double *moments_out_dev)
{
    const char *who = "selftest_xval_multi_fold_moments";
    if (!c || !x_dev || !y_dev || !foldid_dev || !moments_out_dev) { set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG; }
    const DenseSrc X = dtype < 0 ? dense_src_cm((const double *)x_dev, ld) : dense_src_rm(x_dev, dtype, ld);
    const int K = nfolds;
    int rc = dense_src_check(who, X, n, p);
    if (!rc) rc = xval_check_rows(n, n, K, 0);
    if (!rc) rc = multi_y_check(who, n, y_rs, y_cs, m);
    if (rc) return rc;
    std::vector<int32_t> pen(1, OEMGPU_LASSO);
    oemgpu_opts o;
    memset(&o, 0, sizeof o);
    o.npen = 1; o.penalty = pen.data(); o.nlambda = 1;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const XvalMultiLay V = xval_multi_layout(c->num_cu, n, p, K, m, 1, &o, 1);
    if (ctx_aux(c, V.total)) return OEMGPU_ERR_HIP;
    XvmClock clk(c);
    std::vector<int64_t> hf;
    if ((rc = xval_multi_passes(c, V, X, MultiY{y_dev, y_rs, y_cs}, foldid_dev, m, hf, clk))) return rc;
    const int step = 65535 / K;
    for (int r0 = 0; r0 < m; r0 += step) {
        const int nb = m - r0 < step ? m - r0 : step;
        if ((rc = launch_multi_fold_compose(c->stream, V.xp, K, (const double *)(c->aux + V.L.a_mf), (const double *)(c->aux + V.a_part),
                                            (const int *)(c->aux + V.a_cf), r0, nb, true, moments_out_dev + V.L.mlen * K * r0))) return rc;
    }
    OEM_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- the same three phases as separate calls, for row shards on several GPUs (one process per GPU; the caller sums the fold
// moments and the fold sizes over the ranks between phases 1 and 2 and merges the error triples after phase 3).  All three calls
// of one fit take the same (n_local, p, nfolds, weighted, o): the buffer layout in the context is a function of those.
int64_t oemgpu_xval_moments_len(int32_t p, int32_t nfolds, int32_t weighted)
{
    return (int64_t)nfolds * (oemgpu_moments_len(p + (weighted ? 1 : 0)) + (weighted ? p + 1 : 0));
}

int oemgpu_xval_fold_moments_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                                 const double *w_dev, const int32_t *foldid_dev, int32_t nfolds, const oemgpu_opts *o,
                                 double *fold_moments_dev, int64_t *fold_n)
{
    if (!c || !x_dev || !y_dev || !foldid_dev || !fold_moments_dev || !fold_n) { set_error("xval_fold_moments: NULL argument"); return OEMGPU_ERR_ARG; }
    const int K = nfolds;
    int rc = xval_check(c, x_dev, y_dev, foldid_dev, n, ld, p, K, -1, 0, w_dev != nullptr, o);
    if (rc) return rc;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const XvalLay L = xval_layout(c, n, p, K, o->npen, nl_of(o), w_dev != nullptr);
    if (ctx_aux(c, L.total)) return OEMGPU_ERR_HIP;
    std::vector<int64_t> hf;
    rc = xval_prepare(c, L, dense_src_cm(x_dev, ld), y_dev, w_dev, foldid_dev, hf);
    if (rc) return rc;
    for (int k = 0; k < K; ++k) fold_n[k] = hf[k];
    OEM_HIP(hipMemcpyAsync(fold_moments_dev, c->aux + L.a_mf, sizeof(double) * L.mlen * K, hipMemcpyDeviceToDevice, c->stream));
    if (w_dev) OEM_HIP(hipMemcpyAsync(fold_moments_dev + L.mlen * K, c->aux + L.a_cs, sizeof(double) * L.cslen * K, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

int oemgpu_xval_solve_folds_dev(oemgpu_ctx *c, const double *fold_moments_dev, const int64_t *fold_n_total, int64_t n_local, int32_t p,
                                int32_t nfolds, int32_t weighted, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                                double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    if (!c || !fold_moments_dev || !fold_n_total || !beta || !lambda_out || !niter || !loss || !d) { set_error("xval_solve_folds: NULL argument"); return OEMGPU_ERR_ARG; }
    const int K = nfolds;
    int rc = xval_check(c, fold_moments_dev, fold_moments_dev, fold_moments_dev, n_local, n_local, p, K, intercept, 0, weighted != 0, o);
    if (rc) return rc;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const XvalLay L = xval_layout(c, n_local, p, K, o->npen, nl_of(o), weighted != 0);
    if (c->aux_bytes < L.total) { set_error("xval_solve_folds: call oemgpu_xval_fold_moments_dev with the same arguments first"); return OEMGPU_ERR_ARG; }
    ctx_void_cv(c);                                              // the moments, sums and coefficients below land at THIS layout's offsets
    OEM_HIP(hipMemcpyAsync(c->aux + L.a_mf, fold_moments_dev, sizeof(double) * L.mlen * K, hipMemcpyDeviceToDevice, c->stream));
    if (weighted) OEM_HIP(hipMemcpyAsync(c->aux + L.a_cs, fold_moments_dev + L.mlen * K, sizeof(double) * L.cslen * K, hipMemcpyDeviceToDevice, c->stream));
    int64_t n_tot = 0;
    for (int k = 0; k < K; ++k) n_tot += fold_n_total[k];
    return xval_solve(c, L, fold_n_total, n_tot, standardize, intercept, o, beta, lambda_out, niter, loss, d);
}

int oemgpu_xval_cv_triples_dev(oemgpu_ctx *c, int64_t n_local, int32_t p, int32_t nfolds, int32_t weighted, int32_t type_measure,
                               const oemgpu_opts *o, double *triples)
{
    if (!c || !o || !triples) { set_error("xval_cv_triples: NULL argument"); return OEMGPU_ERR_ARG; }
    int rc = xval_check(c, triples, triples, triples, n_local, n_local, p, nfolds, -1, type_measure, weighted != 0, o);
    if (rc) return rc;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const XvalLay L = xval_layout(c, n_local, p, nfolds, o->npen, nl_of(o), weighted != 0);
    if (c->aux_bytes < L.total) { set_error("xval_cv_triples: call the first two phases with the same arguments first"); return OEMGPU_ERR_ARG; }
    ctx_void_cv(c);                                              // the partials land at THIS layout's offsets
    return xval_cverr(c, L, type_measure, o, nullptr, nullptr, triples);
}

// Test infrastructure: phase 3 alone on a coefficient table of the caller's -- the layout, the fold-ordered (and weight-scaled) copy
// and the launch are those of oemgpu_xval_dense_dev (xval_layout, xval_prepare, launch_cv_error); nothing is fitted, so n <= p is fine.
int oemgpu_selftest_xval_cv_error_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                                      const double *w_dev, const int32_t *foldid_dev, int32_t nfolds, const double *coef, int32_t npen,
                                      int32_t nl, int32_t type_measure, double *cvm, double *cvsd, double *triples)
{
    if (!c || !x_dev || !y_dev || !foldid_dev || !coef || (!triples && (!cvm || !cvsd))) {
        set_error("selftest_xval_cv_error: NULL argument"); return OEMGPU_ERR_ARG;
    }
    if (p < 1 || npen < 1 || nl < 1) { set_error("selftest_xval_cv_error: bad p, npen or nl"); return OEMGPU_ERR_ARG; }
    const int K = nfolds;
    int rc = xval_check_rows(n, ld, K, type_measure);
    if (rc) return rc;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const XvalLay L = xval_layout(c, n, p, K, npen, nl, w_dev != nullptr);
    if (ctx_aux(c, L.total)) return OEMGPU_ERR_HIP;
    std::vector<int64_t> hf;
    rc = xval_prepare(c, L, dense_src_cm(x_dev, ld), y_dev, w_dev, foldid_dev, hf);
    if (rc) return rc;
    char *ax = c->aux;
    int64_t *fold_n = (int64_t *)(ax + L.a_fn), *fold_start = fold_n + K;
    double *cvout = (double *)(ax + L.a_out);
    OEM_HIP(hipMemcpyAsync(ax + L.a_b, coef, sizeof(double) * (size_t)K * npen * nl * (p + 1), hipMemcpyHostToDevice, c->stream));
    rc = launch_cv_error(c->stream, (const double *)(ax + L.a_xp), L.ldp, (const double *)(ax + L.a_yp), fold_start, fold_n, K, p,
                         (const double *)(ax + L.a_b), npen, nl, type_measure, L.weighted ? 1 : 0, L.cv, (double)L.n, (double *)(ax + L.a_part),
                         cvout, triples != nullptr);
    if (rc) return rc;
    const size_t nk = (size_t)npen * nl;
    std::vector<double> hc((triples ? 3 : 2) * nk);
    OEM_HIP(hipMemcpyAsync(hc.data(), cvout, sizeof(double) * hc.size(), hipMemcpyDeviceToHost, c->stream));
    OEM_HIP(hipStreamSynchronize(c->stream));                   // coef and hc are the caller's and a local
    if (triples) { memcpy(triples, hc.data(), sizeof(double) * hc.size()); return 0; }
    for (size_t ki = 0; ki < nk; ++ki) { cvm[ki] = hc[2 * ki]; cvsd[ki] = hc[2 * ki + 1]; }
    return 0;
}

// (count, mean, M2) of the union of `nsets` row sets per (penalty, lambda) by Chan, Golub & LeVeque's update, in set order; then
// cvm = mean, cvsd = sqrt(M2 / (n - 1)) / sqrt(n)  (ref src/oem_xval_dense.cpp:452-461).  Pure host arithmetic.
int oemgpu_xval_merge(const double *triples, int32_t nsets, const oemgpu_opts *o, double *cvm, double *cvsd)
{
    if (!triples || !o || !cvm || !cvsd || nsets < 1) { set_error("xval_merge: bad argument"); return OEMGPU_ERR_ARG; }
    const int npen = o->npen, nl = nl_of(o);
    const size_t nk = (size_t)npen * nl;
    for (int k = 0; k < npen; ++k) {
        const int nlam = (o->penalty[k] == OEMGPU_OLS) ? 1 : nl;
        for (int i = 0; i < nl; ++i) {
            const size_t ki = (size_t)k * nl + i;
            double na = 0.0, ma = 0.0, qa = 0.0;
            for (int s = 0; s < nsets; ++s) {
                const double *t = triples + ((size_t)s * nk + ki) * 3;
                const double nb = t[0], mb = t[1], qb = t[2];
                if (!(nb > 0.0)) continue;
                if (na > 0.0) {
                    const double nn = na + nb, dl = mb - ma;
                    ma += dl * (nb / nn);
                    qa += qb + dl * dl * (na * nb / nn);
                    na = nn;
                } else { na = nb; ma = mb; qa = qb; }
            }
            cvm[ki] = i < nlam ? ma : 0.0;
            cvsd[ki] = (i < nlam && na > 1.0) ? std::sqrt((qa < 0.0 ? 0.0 : qa) / (na - 1.0)) / std::sqrt(na) : 0.0;
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- cv.oem, family = "gaussian"
// The layout is xval.oem's (unweighted) with this route's own regions behind it at L.total: the per-fold triples, the valid columns
// per penalty, the sample sums of a shifted pass, and the inverse of the fold permutation for the prediction store.
struct CvLay {
    XvalLay L;
    size_t a_tri, a_ncol, a_sums, a_inv, total;
};
static CvLay cv_layout(oemgpu_ctx *c, int64_t n, int p, int K, int npen, int nl)
{
    CvLay V;
    V.L = xval_layout(c, n, p, K, npen, nl, false);
    Bump A; A.off = V.L.total;
    V.a_tri = A.take(sizeof(double) * 3 * (size_t)K * npen * nl); V.a_ncol = A.take(sizeof(int) * (size_t)npen);
    V.a_sums = A.take(sizeof(double) * (size_t)oemgpu_sums_len(p)); V.a_inv = A.take(sizeof(int) * (size_t)V.L.ldp);
    V.total = A.off;
    return V;
}

static int cv_check_rows(const char *who, int64_t n, int64_t ld, int p, int K)
{
    int rc = xval_check_rows(n, ld, K, 0);
    if (rc) return rc;
    if (p < 1) { set_error("%s: bad p", who); return OEMGPU_ERR_ARG; }
    return 0;
}

// rows into fold order (and the fold moments about 0), and the stamp oemgpu_cv_score_dev looks for
static int cv_lay_out(oemgpu_ctx *c, const CvLay &V, const DenseSrc &X, const double *y_dev, const int32_t *foldid_dev,
                      bool moments, std::vector<int64_t> &hf)
{
    if (ctx_aux(c, V.total)) return OEMGPU_ERR_HIP;
    int rc = xval_prepare(c, V.L, X, y_dev, nullptr, foldid_dev, hf, moments);
    if (rc) return rc;
    c->cv_n = V.L.n; c->cv_p = V.L.p; c->cv_K = V.L.K; c->cv_aux = c->aux; c->cv_hf = hf; c->cv_kind = CV_KIND_DENSE;
    return 0;
}

static int cv_fold_fits_src(const char *who, oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const double *y_dev,
                            const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                            double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, int64_t *fold_n)
{
    if (!c || !X.x || !y_dev || !foldid_dev || !o || !beta || !lambda_out || !niter || !loss || !d || !fold_n) {
        set_error("cv_fold_fits: NULL argument"); return OEMGPU_ERR_ARG;
    }
    const int K = nfolds;
    int rc = dense_src_check(who, X, n, p);
    if (!rc) rc = check_opts(o, p, p);
    if (!rc) rc = cv_check_rows("cv_fold_fits", n, n, p, K);
    if (rc) return rc;
    // the largest fold holds at least ceil(n / K) rows: some fold fit is then not the Gram form whatever the ids are
    if (n - (n + K - 1) / K <= p) {
        set_error("cv_fold_fits: %lld rows in %d folds leave some fold no more rows than the %d columns", (long long)n, K, p);
        return OEMGPU_ERR_UNSUPPORTED;
    }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const int npen = o->npen, nl = nl_of(o);
    const CvLay V = cv_layout(c, n, p, K, npen, nl);
    const XvalLay &L = V.L;
    std::vector<int64_t> hf;
    rc = cv_lay_out(c, V, X, y_dev, foldid_dev, true, hf);
    if (rc) return rc;
    for (int k = 0; k < K; ++k) {
        fold_n[k] = hf[k];
        if (n - hf[k] <= p) {
            set_error("cv_fold_fits: fold %d leaves %lld rows for %d columns (the fit of p >= n is not this route's)", k + 1, (long long)(n - hf[k]), p);
            return OEMGPU_ERR_UNSUPPORTED;
        }
    }
    char *ax = c->aux;
    const double *mfold = (const double *)(ax + L.a_mf);
    double *msum = (double *)(ax + L.a_ms), *sums = (double *)(ax + V.a_sums);
    const size_t blen = (size_t)npen * nl * (p + 1), nk2 = (size_t)npen * nl;
    // fold ff: the sum of the other folds' moments in fold order, then oem()'s solve on it (R/cv_oem.R:155-175)
    auto solve_all = [&](const double *sm, bool *advised) -> int {
        for (int ff = 1; ff <= K; ++ff) {
            double *ms = msum + L.mlen * ff;
            int r = launch_fold_sum(c->stream, mfold, K, L.mlen, ff, ms);
            if (!r) r = oemgpu_solve_moments_dev(c, ms, sm, p, OEMGPU_SEM_DENSE, standardize, intercept, o, beta + blen * (ff - 1),
                                                 lambda_out + nk2 * (ff - 1), niter + nk2 * (ff - 1), loss + nk2 * (ff - 1), d + (ff - 1));
            if (r) return r;
            if (advised && c->shift_advised) *advised = true;
        }
        return 0;
    };
    bool advised = false;
    rc = solve_all(nullptr, &advised);
    if (rc || !advised) return rc;
    // oemgpu_fit_dense_dev's rule, for all folds at once: sample sums of all rows, the segment passes about them, the solves again
    // (a row-major source's sums are the column-major float64 copy's, bit for bit)
    rc = dense_src_shift_sums(c->stream, X, n, p, y_dev, sums);
    if (!rc) rc = xval_fold_moments(c, L, hf, sums);
    if (!rc) rc = solve_all(sums, nullptr);
    return rc;
}

int oemgpu_cv_fold_fits_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                            const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                            double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, int64_t *fold_n)
{
    return cv_fold_fits_src("cv_fold_fits", c, dense_src_cm(x_dev, ld), n, p, y_dev, foldid_dev, nfolds, standardize, intercept, o, beta, lambda_out, niter, loss,
                            d, fold_n);
}

// oemgpu_cv_fold_fits_dev with the rows gathered from a row-major x where it lies; the layout stamp is the same CV_KIND_DENSE, so
// oemgpu_cv_score_dev scores it as it is
int oemgpu_cv_fold_fits_rm_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                               const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                               double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, int64_t *fold_n)
{
    return cv_fold_fits_src("cv_fold_fits_rm", c, dense_src_rm(x_dev, dtype, ldr), n, p, y_dev, foldid_dev, nfolds, standardize, intercept, o, beta, lambda_out, niter,
                            loss, d, fold_n);
}

// Test infrastructure: the fold layout and the row-major gather alone, into buffers of the caller's -- xo_dev: p columns of ldo >=
// 16 * ceil((n + 16 nfolds) / 16) doubles, yo_dev: ldo doubles; fold_n / fold_start (host, [nfolds]) <- the fold sizes and where each
// fold's segment starts.  Nothing is fitted: any n >= 1, p >= 1.
int oemgpu_selftest_fold_gather_rm_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev,
                                       const int32_t *foldid_dev, int32_t nfolds, double *xo_dev, int64_t ldo, double *yo_dev,
                                       int64_t *fold_n, int64_t *fold_start)
{
    if (!c || !x_dev || !y_dev || !foldid_dev || !xo_dev || !yo_dev || !fold_n || !fold_start) {
        set_error("selftest_fold_gather_rm: NULL argument"); return OEMGPU_ERR_ARG;
    }
    const DenseSrc X = dense_src_rm(x_dev, dtype, ldr);
    int rc = dense_src_check("selftest_fold_gather_rm", X, n, p);
    if (!rc) rc = cv_check_rows("selftest_fold_gather_rm", n, n, p, nfolds);
    if (rc) return rc;
    const int K = nfolds;
    if (ldo < (n + 16 * (int64_t)K + 15) / 16 * 16) { set_error("selftest_fold_gather_rm: ldo is shorter than the fold-ordered rows"); return OEMGPU_ERR_ARG; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    Bump B;
    const size_t a_cnt = B.take(fold_layout_ints(n, K) * sizeof(int)), a_fn = B.take(sizeof(int64_t) * 2 * K), a_bad = B.take(256),
                 a_pos = B.take(sizeof(int) * (size_t)n);
    if (ctx_reserve(c, B.off)) return OEMGPU_ERR_HIP;
    int *blockcnt = (int *)(c->ws + a_cnt), *bad = (int *)(c->ws + a_bad), *pos = (int *)(c->ws + a_pos);
    int64_t *fn = (int64_t *)(c->ws + a_fn);
    rc = launch_fold_layout(c->stream, foldid_dev, n, K, blockcnt, fn, fn + K, pos, bad);
    if (!rc) rc = dense_src_gather(c->stream, X, n, p, y_dev, foldid_dev, K, pos, xo_dev, ldo, yo_dev);
    if (rc) return rc;
    int hbad = 0;
    std::vector<int64_t> hf(2 * K);
    OEM_HIP(hipMemcpyAsync(hf.data(), fn, sizeof(int64_t) * 2 * K, hipMemcpyDeviceToHost, c->stream));
    OEM_HIP(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    OEM_HIP(hipStreamSynchronize(c->stream));
    if (hbad) { set_error("xval_dense: foldid must hold values in 1..nfolds"); return OEMGPU_ERR_ARG; }
    for (int k = 0; k < K; ++k) { fold_n[k] = hf[k]; fold_start[k] = hf[K + k]; }
    return 0;
}

int oemgpu_cv_score_dev(oemgpu_ctx *c, int64_t n, int32_t p, int32_t nfolds, const double *coef, int32_t npen, int32_t nl,
                        const int32_t *ncol, int32_t type_measure, double *triples, double *predmat_dev)
{
    if (!c || !coef || !ncol || !triples) { set_error("cv_score: NULL argument"); return OEMGPU_ERR_ARG; }
    if (p < 1 || npen < 1 || nl < 1) { set_error("cv_score: bad p, npen or nl"); return OEMGPU_ERR_ARG; }
    const int K = nfolds;
    int rc = xval_check_rows(n, n, K, type_measure);
    if (rc) return rc;
    for (int k = 0; k < npen; ++k)
        if (ncol[k] < 0 || ncol[k] > nl) { set_error("cv_score: ncol[%d] = %d is outside 0..%d", k, ncol[k], nl); return OEMGPU_ERR_ARG; }
    if (c->cv_kind != CV_KIND_DENSE || c->cv_n != n || c->cv_p != p || c->cv_K != K || !c->aux || c->cv_aux != c->aux || (int)c->cv_hf.size() != 2 * K) {
        set_error("cv_score: call oemgpu_cv_fold_fits_dev with the same n, p and nfolds on this context first"); return OEMGPU_ERR_ARG;
    }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const CvLay V = cv_layout(c, n, p, K, npen, nl);
    const XvalLay &L = V.L;
    if (c->aux_bytes < V.total) { set_error("cv_score: npen and nl must be those of the call that laid the rows out"); return OEMGPU_ERR_ARG; }
    char *ax = c->aux;
    int64_t *fold_n = (int64_t *)(ax + L.a_fn), *fold_start = fold_n + K;
    const int *pos = (const int *)(ax + L.a_pos);
    int *ncol_dev = (int *)(ax + V.a_ncol), *inv = (int *)(ax + V.a_inv);
    double *bdev = (double *)(ax + L.a_b), *tri = (double *)(ax + V.a_tri);
    const size_t blen = (size_t)K * npen * nl * (p + 1), tlen = (size_t)3 * K * npen * nl;
    // the fold sizes and starts go up again from the host copy of phase 1: what the kernels index the rows by is this call's own
    OEM_HIP(hipMemcpyAsync(fold_n, c->cv_hf.data(), sizeof(int64_t) * 2 * K, hipMemcpyHostToDevice, c->stream));
    OEM_HIP(hipMemcpyAsync(bdev, coef, sizeof(double) * blen, hipMemcpyHostToDevice, c->stream));
    OEM_HIP(hipMemcpyAsync(ncol_dev, ncol, sizeof(int) * (size_t)npen, hipMemcpyHostToDevice, c->stream));
    if (predmat_dev) { rc = launch_fold_inverse(c->stream, pos, n, L.ldp, inv); if (rc) return rc; }
    rc = launch_cv_fold_error(c->stream, (const double *)(ax + L.a_xp), L.ldp, (const double *)(ax + L.a_yp), fold_start, fold_n, K, p, bdev,
                              npen, nl, type_measure, L.cv, (double *)(ax + L.a_part), ncol_dev, tri, predmat_dev, inv, n);
    if (rc) return rc;
    OEM_HIP(hipMemcpyAsync(triples, tri, sizeof(double) * tlen, hipMemcpyDeviceToHost, c->stream));
    OEM_HIP(hipStreamSynchronize(c->stream));                   // coef, ncol and triples are the caller's
    return 0;
}

// Test infrastructure: phase 2 alone on a table of the caller's -- the rows are laid out as phase 1 lays them out (no moments, nothing
// fitted, so a fold may leave fewer rows than columns), then oemgpu_cv_score_dev as it is.
int oemgpu_selftest_cv_score_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev,
                                 const int32_t *foldid_dev, int32_t nfolds, const double *coef, int32_t npen, int32_t nl,
                                 const int32_t *ncol, int32_t type_measure, double *triples, double *predmat_dev)
{
    if (!c || !x_dev || !y_dev || !foldid_dev || !coef || !ncol || !triples) { set_error("selftest_cv_score: NULL argument"); return OEMGPU_ERR_ARG; }
    if (npen < 1 || nl < 1) { set_error("selftest_cv_score: bad npen or nl"); return OEMGPU_ERR_ARG; }
    int rc = cv_check_rows("selftest_cv_score", n, ld, p, nfolds);
    if (rc) return rc;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const CvLay V = cv_layout(c, n, p, nfolds, npen, nl);
    std::vector<int64_t> hf;
    rc = cv_lay_out(c, V, dense_src_cm(x_dev, ld), y_dev, foldid_dev, false, hf);
    if (rc) return rc;
    return oemgpu_cv_score_dev(c, n, p, nfolds, coef, npen, nl, ncol, type_measure, triples, predmat_dev);
}

// ---------------------------------------------------------------------------------------------- cv.oem for many Gaussian responses on one x
//   cv.oem's K + 1 calls of oem() per response (R/cv_oem.R:105, 129-175) and cv.oemfit_gaussian's prediction loop
// (:349-423) for all m responses from xval_multi_passes' ONE fold layout, gather, K fold Gram passes and fold X'Y pass.  Per chunk of nb
// responses: the nb (K + 1) composed sums, their paths in one batched launch under oem()'s own semantics (every instance its own
// standardisation, y scale and lambda grid: OEMGPU_SEM_DENSE, no shared lmax), the index table of lambda.interp (R/utils.R:64-144) on the
// host, the interpolation and the per-fold scoring on the device.  The buffers: XvalMultiLay's, then the regions below, in oemgpu_ctx::aux.
struct CvMultiLay {
    XvalMultiLay V;
    size_t b_raw = 0, b_idx = 0, b_ncol = 0, b_inv = 0, b_pred = 0, b_tri = 0;                                       // bytes
    size_t a_raw = 0, a_idx = 0, a_ncol = 0, a_inv = 0, a_pred = 0, a_tri = 0, total = 0;
};
static CvMultiLay cv_multi_layout(int num_cu, int64_t n, int p, int K, int m, const oemgpu_opts *o, int nb_limit, bool keep, int nb_exact = 0)
{
    CvMultiLay W;
    W.V = xval_multi_layout(num_cu, n, p, K, m, 1, o, nb_limit, true, nb_exact);
    const size_t nb = (size_t)W.V.nb, npen = (size_t)o->npen, nl = (size_t)nl_of(o);
    W.b_raw = W.V.b_tab;                                                            // the chunk's fold tables as they were fitted
    W.b_idx = nb * K * npen * nl * sizeof(CvInterpIdx);                             // the index table
    W.b_ncol = nb * npen * sizeof(int);
    W.b_inv = (size_t)W.V.L.ldp * sizeof(int);                                      // fold position -> caller's row
    W.b_pred = keep ? nb * npen * nl * (size_t)n * 8 : 0;                           // one chunk's yhat, in the caller's row order
    W.b_tri = nb * K * npen * nl * 3 * 8;                                           // its per-fold triples
    Bump A;
    A.off = W.V.total;
    W.a_raw = A.take(W.b_raw); W.a_idx = A.take(W.b_idx); W.a_ncol = A.take(W.b_ncol); W.a_inv = A.take(W.b_inv);
    W.a_pred = A.take(W.b_pred); W.a_tri = A.take(W.b_tri);
    W.total = A.off;
    return W;
}

static thread_local double g_cvm_ms[OEMGPU_CVM_NPHASES] = {0, 0, 0, 0, 0, 0, 0};
// Test infrastructure (oemgpu_selftest_cv_multi_nb_limit): at most that many responses per chunk in this thread's calls, as if the
// device's free memory had asked for it; 0: no limit
static thread_local int g_cvm_nb_limit = 0;

// np.interp(x, xp, 0..k-1) for an ascending xp: the operations of numpy's compiled loop, in its order
static double cv_np_interp(double x, const double *xp, int k)
{
    if (x <= xp[0]) return 0.0;
    if (x >= xp[k - 1]) return (double)(k - 1);
    int lo = 0, hi = k - 1;                                          // xp[lo] <= x < xp[hi]
    while (hi - lo > 1) { const int mid = (lo + hi) / 2; if (x >= xp[mid]) lo = mid; else hi = mid; }
    if (xp[lo] == x) return (double)lo;
    const double slope = 1.0 / (xp[lo + 1] - xp[lo]);
    return slope * (x - xp[lo]) + (double)lo;
}
// lambda.interp (R/utils.R:64-87, glmnet's) of the k lambdas `lam` at the ns values s: api._lambda_interp's operations in its order
static void cv_lambda_interp(const double *lam, int k, const double *s, int ns, CvInterpIdx *out, std::vector<double> &lamn)
{
    if (k == 1) { for (int j = 0; j < ns; ++j) out[j] = CvInterpIdx{0, 0, 1.0}; return; }
    double lo = lam[0], hi = lam[0];
    for (int i = 1; i < k; ++i) { if (lam[i] < lo) lo = lam[i]; if (lam[i] > hi) hi = lam[i]; }
    const double span = lam[0] - lam[k - 1];
    lamn.resize(k);
    for (int i = 0; i < k; ++i) lamn[i] = (lam[0] - lam[i]) / span;
    for (int j = 0; j < ns; ++j) {
        double sj = s[j];
        if (sj < lo) sj = lo;
        if (sj > hi) sj = hi;
        const double sfrac = (lam[0] - sj) / span;
        const double coord = cv_np_interp(sfrac, lamn.data(), k);
        int left = (int)std::floor(coord), right = (int)std::ceil(coord);
        if (!(left >= 0)) left = 0;                                  // (a NaN grid: the indices stay inside the table, the values are NaN)
        if (left > k - 1) left = k - 1;
        if (!(right >= 0)) right = 0;
        if (right > k - 1) right = k - 1;
        out[j] = CvInterpIdx{left, right, left == right ? 1.0 : (sfrac - lamn[right]) / (lamn[left] - lamn[right])};
    }
}
// One response: the index table idx[K][npen][nl] and ncol[npen] from the full fit's grid lam0[npen][nl] and the fold grids
// lamf[K][npen][nl] -- ncol = the count of lam0 >= max over folds of the fold grid's minimum (R/cv_oem.R:364-375: no extrapolation)
static void cv_interp_table(const oemgpu_opts *o, int K, const double *lam0, const double *lamf, CvInterpIdx *idx, int32_t *ncol)
{
    const int npen = o->npen, nl = nl_of(o);
    std::vector<double> lamn;
    for (int k = 0; k < npen; ++k) {
        const int nlam = nl;                                         // ("ols", a grid of one, is refused by the entries)
        double floor_ = 0.0;
        for (int ff = 0; ff < K; ++ff) {
            const double *g = lamf + ((size_t)ff * npen + k) * nl;
            double mn = g[0];
            for (int i = 1; i < nlam; ++i) if (g[i] < mn) mn = g[i];
            if (ff == 0 || mn > floor_) floor_ = mn;
        }
        const double *s = lam0 + (size_t)k * nl;
        int nc = 0;
        while (nc < nlam && s[nc] >= floor_) ++nc;                   // (the grids descend: the valid columns lead)
        ncol[k] = nc;
        for (int ff = 0; ff < K; ++ff) {
            CvInterpIdx *row = idx + ((size_t)ff * npen + k) * nl;
            cv_lambda_interp(lamf + ((size_t)ff * npen + k) * nl, nlam, s, nc, row, lamn);
            for (int j = nc; j < nl; ++j) row[j] = CvInterpIdx{0, 0, 1.0};
        }
    }
}

static int cv_dense_multi_src(const char *who, oemgpu_ctx *c, const DenseSrc &X, int64_t n, int32_t p, const double *y_dev, int64_t rs, int64_t cs,
                              int32_t m, const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept, int32_t type_measure,
                              const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, int32_t *ncol,
                              double *triples, int64_t *fold_n_out, int32_t *route, double *fold_beta, double *fold_lambda, int32_t *fold_niter,
                              double *predmat)
{
    if (!c || !X.x || !y_dev || !foldid_dev || !beta || !lambda_out || !niter || !loss || !d || !ncol || !triples || !fold_n_out || !route) {
        set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG;
    }
    const int K = nfolds;
    int rc = dense_src_check(who, X, n, p);
    if (!rc) rc = xval_check(c, X.x, y_dev, foldid_dev, n, n, p, K, 0, type_measure, false, o);       // (oem()'s semantics: q = p)
    if (!rc) rc = multi_y_check(who, n, rs, cs, m);
    if (rc) return rc;
    // the largest fold holds at least ceil(n / K) rows: some fold fit is then not the Gram form whatever the ids are
    if (n <= p || n - (n + K - 1) / K <= p) {
        set_error("%s: %lld rows in %d folds leave some fit no more rows than the %d columns (the fit of p >= n is not this call's: "
                  "oemgpu_fit_dense_dev fold by fold)", who, (long long)n, K, p);
        return OEMGPU_ERR_UNSUPPORTED;
    }
    for (int k = 0; k < o->npen; ++k)
        if (o->penalty[k] == OEMGPU_OLS) {
            set_error("%s: the \"ols\" penalty is not served (its one-lambda grid is oemgpu_fit_dense_dev's, fold by fold)", who);
            return OEMGPU_ERR_UNSUPPORTED;
        }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const bool keep = predmat != nullptr;
    CvMultiLay W = cv_multi_layout(c->num_cu, n, p, K, m, o, g_cvm_nb_limit, keep);
    {   // one chunk's sums, tables, predictions and partials grow with nb: fewer responses per chunk rather than an allocation that fails
        size_t fre = 0, tot = 0;
        if (hipMemGetInfo(&fre, &tot) == hipSuccess)
            while (W.V.nb > 1 && W.total > fre + c->aux_bytes) W = cv_multi_layout(c->num_cu, n, p, K, m, o, W.V.nb / 2, keep);
    }
    if (ctx_aux(c, W.total)) return OEMGPU_ERR_HIP;
    for (double &v : g_cvm_ms) v = 0.0;
    XvmClock clk(c, g_cvm_ms);
    const XvalMultiLay &V = W.V;
    const XvalLay &L = V.L;
    std::vector<int64_t> hf;
    if ((rc = xval_multi_passes(c, V, X, MultiY{y_dev, rs, cs}, foldid_dev, m, hf, clk))) return rc;
    for (int k = 0; k < K; ++k) {
        fold_n_out[k] = hf[k];
        if (n - hf[k] <= p) {
            set_error("%s: fold %d leaves %lld rows for %d columns (the fit of p >= n is not this call's)", who, k + 1, (long long)(n - hf[k]), p);
            return OEMGPU_ERR_UNSUPPORTED;
        }
    }
    char *ax = c->aux;
    const int npen = L.npen, nl = L.nl;
    const size_t mlen = L.mlen, blen = (size_t)npen * nl * (p + 1), nk2 = (size_t)npen * nl;
    const double *mfold = (const double *)(ax + L.a_mf), *part = (const double *)(ax + V.a_part), *Yp = (const double *)(ax + V.a_yp);
    const int *cfirst = (const int *)(ax + V.a_cf);
    const int64_t *fold_n = (const int64_t *)(ax + L.a_fn), *fold_start = fold_n + K;
    double *comp = (double *)(ax + V.a_comp), *tab = (double *)(ax + V.a_tab), *cvpart = (double *)(ax + V.a_cvpart);
    double *raw = (double *)(ax + W.a_raw), *pred = keep ? (double *)(ax + W.a_pred) : nullptr, *tri = (double *)(ax + W.a_tri);
    CvInterpIdx *idx_dev = (CvInterpIdx *)(ax + W.a_idx);
    int *ncol_dev = (int *)(ax + W.a_ncol), *inv = (int *)(ax + W.a_inv);
    if (keep) if ((rc = launch_fold_inverse(c->stream, (const int *)(ax + L.a_pos), n, L.ldp, inv))) return rc;
    auto interrupted = [&]() {
        if (!(o->interrupt && o->interrupt(o->interrupt_arg))) return false;
        set_error("interrupted by the caller");
        return true;
    };
    std::vector<double> ab, al, aloss, ad, hb;
    std::vector<int32_t> an, adv, hn;
    std::vector<CvInterpIdx> hidx;
    for (int r0 = 0; r0 < m; r0 += V.nb) {
        const int nb = m - r0 < V.nb ? m - r0 : V.nb, ninst = nb * (K + 1);
        if (r0 > 0 && interrupted()) return OEMGPU_ERR_INTERRUPTED;
        clk.begin();
        if ((rc = launch_multi_fold_compose(c->stream, V.xp, K, mfold, part, cfirst, r0, nb, false, comp))) return rc;
        clk.end(3);
        // ---- the paths: instance b (K + 1) + ff is response r0 + b on all folds (ff = 0) or on all but fold ff, each as oem() fits it
        clk.begin();
        ab.resize(blen * ninst); al.resize(nk2 * ninst); an.resize(nk2 * ninst); aloss.resize(nk2 * ninst); ad.resize(ninst); adv.assign(ninst, 0);
        if (V.route == 0) {
            rc = solve_moments_batch(c, comp, mlen, ninst, p, OEMGPU_SEM_DENSE, standardize, intercept, o, ab.data(), al.data(), an.data(), aloss.data(),
                                     ad.data(), false, nullptr, 0, adv.data());
            if (rc) return rc;
        } else {
            for (int i = 0; i < ninst; ++i) {
                rc = solve_moments_impl(c, comp + mlen * i, nullptr, p, OEMGPU_SEM_DENSE, standardize, intercept, o, ab.data() + blen * i, al.data() + nk2 * i,
                                        an.data() + nk2 * i, aloss.data() + nk2 * i, ad.data() + i, nullptr);
                if (rc) return rc;
                adv[i] = c->shift_advised ? 1 : 0;
            }
        }
        clk.end(4);
        // ---- the full fits out, the index tables of lambda.interp (host: O(nb K npen nl) scalars)
        hb.resize(blen * K * nb); hidx.resize(nk2 * K * nb); hn.assign((size_t)npen * nb, 0);
        for (int b = 0; b < nb; ++b) {
            const size_t i0 = (size_t)b * (K + 1), r = (size_t)r0 + b;
            bool shifted = false;
            for (int ff = 0; ff <= K; ++ff) shifted = shifted || adv[i0 + ff] != 0;
            memcpy(hb.data() + blen * K * b, ab.data() + blen * (i0 + 1), sizeof(double) * blen * K);
            if (shifted) {                                           // oem()'s shifted pass is the single route's: reported, nothing scored
                route[r] = 2;
                for (size_t t = 0; t < nk2 * K; ++t) hidx[nk2 * K * b + t] = CvInterpIdx{0, 0, 1.0};
                for (int k = 0; k < npen; ++k) ncol[(size_t)npen * r + k] = 0;
                continue;
            }
            route[r] = V.route;
            memcpy(beta + blen * r, ab.data() + blen * i0, sizeof(double) * blen);
            memcpy(lambda_out + nk2 * r, al.data() + nk2 * i0, sizeof(double) * nk2);
            memcpy(niter + nk2 * r, an.data() + nk2 * i0, sizeof(int32_t) * nk2);
            memcpy(loss + nk2 * r, aloss.data() + nk2 * i0, sizeof(double) * nk2);
            d[r] = ad[i0];
            if (fold_beta) memcpy(fold_beta + blen * K * r, ab.data() + blen * (i0 + 1), sizeof(double) * blen * K);
            if (fold_lambda) memcpy(fold_lambda + nk2 * K * r, al.data() + nk2 * (i0 + 1), sizeof(double) * nk2 * K);
            if (fold_niter) memcpy(fold_niter + nk2 * K * r, an.data() + nk2 * (i0 + 1), sizeof(int32_t) * nk2 * K);
            cv_interp_table(o, K, al.data() + nk2 * i0, al.data() + nk2 * (i0 + 1), hidx.data() + nk2 * K * b, hn.data() + (size_t)npen * b);
            for (int k = 0; k < npen; ++k) ncol[(size_t)npen * r + k] = hn[(size_t)npen * b + k];
        }
        // ---- the interpolation on the device: raw fold tables, index table and ncol up, tab <- beta[left] frac + beta[right] (1 - frac)
        clk.begin();
        OEM_HIP(hipMemcpyAsync(raw, hb.data(), sizeof(double) * blen * K * nb, hipMemcpyHostToDevice, c->stream));
        OEM_HIP(hipMemcpyAsync(idx_dev, hidx.data(), sizeof(CvInterpIdx) * nk2 * K * nb, hipMemcpyHostToDevice, c->stream));
        OEM_HIP(hipMemcpyAsync(ncol_dev, hn.data(), sizeof(int) * (size_t)npen * nb, hipMemcpyHostToDevice, c->stream));
        if ((rc = launch_cv_interp(c->stream, raw, idx_dev, ncol_dev, nb, K, npen, nl, p, tab))) return rc;
        clk.end(5);
        // ---- the held-out rows of the nb responses scored where they lie: per-fold (count, mean, M2), yhat with predmat
        clk.begin();
        rc = launch_cv_fold_error_many(c->stream, (const double *)(ax + L.a_xp), L.ldp, Yp + (size_t)L.ldp * r0, fold_start, fold_n, K, p, tab, npen, nl,
                                       type_measure, V.cv, nb, cvpart, ncol_dev, tri, pred, inv, n);
        if (rc) return rc;
        OEM_HIP(hipMemcpyAsync(triples + 3 * nk2 * K * r0, tri, sizeof(double) * 3 * nk2 * K * nb, hipMemcpyDeviceToHost, c->stream));
        if (keep) OEM_HIP(hipMemcpyAsync(predmat + nk2 * (size_t)n * r0, pred, sizeof(double) * nk2 * (size_t)n * nb, hipMemcpyDeviceToHost, c->stream));
        OEM_HIP(hipStreamSynchronize(c->stream));                    // hb, hidx and hn are read by the copies above
        clk.end(6);
    }
    return 0;
}

int oemgpu_cv_dense_multi_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev, int64_t y_rs, int64_t y_cs,
                              int32_t m, const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept, int32_t type_measure,
                              const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, int32_t *ncol,
                              double *triples, int64_t *fold_n, int32_t *route, double *fold_beta, double *fold_lambda, int32_t *fold_niter,
                              double *predmat)
{
    return cv_dense_multi_src("cv_dense_multi", c, dense_src_cm(x_dev, ld), n, p, y_dev, y_rs, y_cs, m, foldid_dev, nfolds, standardize, intercept,
                              type_measure, o, beta, lambda_out, niter, loss, d, ncol, triples, fold_n, route, fold_beta, fold_lambda, fold_niter, predmat);
}

int oemgpu_cv_dense_multi_rm_dev(oemgpu_ctx *c, const void *x_dev, int32_t dtype, int64_t n, int64_t ldr, int32_t p, const double *y_dev, int64_t y_rs,
                                 int64_t y_cs, int32_t m, const int32_t *foldid_dev, int32_t nfolds, int32_t standardize, int32_t intercept,
                                 int32_t type_measure, const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d,
                                 int32_t *ncol, double *triples, int64_t *fold_n, int32_t *route, double *fold_beta, double *fold_lambda,
                                 int32_t *fold_niter, double *predmat)
{
    return cv_dense_multi_src("cv_dense_multi_rm", c, dense_src_rm(x_dev, dtype, ldr), n, p, y_dev, y_rs, y_cs, m, foldid_dev, nfolds, standardize,
                              intercept, type_measure, o, beta, lambda_out, niter, loss, d, ncol, triples, fold_n, route, fold_beta, fold_lambda, fold_niter,
                              predmat);
}

int oemgpu_last_cv_multi_timings(double *ms)
{
    if (!ms) { set_error("last_cv_multi_timings: NULL argument"); return OEMGPU_ERR_ARG; }
    for (int i = 0; i < OEMGPU_CVM_NPHASES; ++i) ms[i] = g_cvm_ms[i];
    return 0;
}

int oemgpu_selftest_cv_multi_plan(int64_t n, int32_t p, int32_t nfolds, int32_t m, int32_t npen, int32_t nl, int32_t num_cu, int32_t keep,
                                  int32_t nb_limit, int64_t *out)
{
    if (n < 1 || p < 1 || m < 1 || npen < 1 || nl < 1 || num_cu < 1 || nb_limit < 0 || !out) { set_error("selftest_cv_multi_plan: bad argument"); return OEMGPU_ERR_ARG; }
    if (int rc = xval_check_rows(n, n, nfolds, 0)) return rc;
    if (n <= p) { set_error("selftest_cv_multi_plan: n <= p, which the call does not serve"); return OEMGPU_ERR_UNSUPPORTED; }
    std::vector<int32_t> pen(npen, OEMGPU_LASSO);
    oemgpu_opts o;
    memset(&o, 0, sizeof o);
    o.npen = npen; o.penalty = pen.data(); o.nlambda = nl;
    const CvMultiLay W = cv_multi_layout(num_cu, n, p, nfolds, m, &o, nb_limit, keep != 0);
    const XvalMultiLay &V = W.V;
    const int64_t v[OEMGPU_CVM_PLAN_LEN] = {V.nb, V.nsolve, V.sv.engine, V.route, V.xp.rows, multi_fold_chunks_max(V.xp, nfolds), V.xp.npass, V.xp.mb, V.cv.nwg,
                                            (int64_t)V.L.total, (int64_t)V.b_col, (int64_t)V.b_yp, (int64_t)V.b_cf, (int64_t)V.b_part, (int64_t)V.b_comp,
                                            (int64_t)V.b_tab, (int64_t)V.b_cvpart, (int64_t)V.b_cvout, (int64_t)V.total, V.sv.cap,
                                            (int64_t)W.b_raw, (int64_t)W.b_idx, (int64_t)W.b_ncol, (int64_t)W.b_inv, (int64_t)W.b_pred, (int64_t)W.b_tri,
                                            (int64_t)W.total};
    for (int i = 0; i < OEMGPU_CVM_PLAN_LEN; ++i) out[i] = v[i];
    return 0;
}

int oemgpu_selftest_cv_multi_nb_limit(int32_t nb_limit)
{
    if (nb_limit < 0) { set_error("selftest_cv_multi_nb_limit: a negative limit"); return OEMGPU_ERR_ARG; }
    g_cvm_nb_limit = nb_limit;
    return 0;
}

int oemgpu_selftest_cv_interp(int32_t nfolds, int32_t npen, int32_t nl, const double *lam_full, const double *lam_fold, int32_t *left, int32_t *right,
                              double *frac, int32_t *ncol)
{
    if (nfolds < 1 || npen < 1 || nl < 1 || !lam_full || !lam_fold || !left || !right || !frac || !ncol) { set_error("selftest_cv_interp: bad argument"); return OEMGPU_ERR_ARG; }
    std::vector<int32_t> pen(npen, OEMGPU_LASSO);
    oemgpu_opts o;
    memset(&o, 0, sizeof o);
    o.npen = npen; o.penalty = pen.data(); o.nlambda = nl;
    std::vector<CvInterpIdx> idx((size_t)nfolds * npen * nl);
    cv_interp_table(&o, nfolds, lam_full, lam_fold, idx.data(), ncol);
    for (size_t t = 0; t < idx.size(); ++t) { left[t] = idx[t].left; right[t] = idx[t].right; frac[t] = idx[t].frac; }
    return 0;
}

// Test infrastructure: the fold layout, the gathers and the many-response scoring alone on tables of the caller's (nothing is fitted, so
// a fold may leave fewer rows than columns); with raw_dev == 0 the tables are scored as they are, else they go through cv_interp_kernel first
int oemgpu_selftest_cv_score_multi_dev(oemgpu_ctx *c, const double *x_dev, int64_t n, int64_t ld, int32_t p, const double *y_dev, int64_t y_rs,
                                       int64_t y_cs, int32_t m, const int32_t *foldid_dev, int32_t nfolds, const double *coef, int32_t npen, int32_t nl,
                                       const int32_t *ncol, int32_t type_measure, int32_t nb, const int32_t *left, const int32_t *right,
                                       const double *frac, double *table_out, double *triples, double *predmat_dev)
{
    const char *who = "selftest_cv_score_multi";
    if (!c || !x_dev || !y_dev || !foldid_dev || !coef || !ncol || !triples) { set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG; }
    if (p < 1 || npen < 1 || nl < 1 || nb < 1) { set_error("%s: bad p, npen, nl or nb", who); return OEMGPU_ERR_ARG; }
    if ((left || right || frac) && !(left && right && frac)) { set_error("%s: left, right and frac go together", who); return OEMGPU_ERR_ARG; }
    const int K = nfolds;
    int rc = xval_check_rows(n, ld, K, type_measure);
    if (!rc) rc = multi_y_check(who, n, y_rs, y_cs, m);
    if (rc) return rc;
    const size_t nk2 = (size_t)npen * nl, blen = nk2 * (p + 1);
    for (size_t t = 0; t < (size_t)m * npen; ++t)
        if (ncol[t] < 0 || ncol[t] > nl) { set_error("%s: ncol[%d] = %d is outside 0..%d", who, (int)t, ncol[t], nl); return OEMGPU_ERR_ARG; }
    if (left)
        for (size_t t = 0; t < (size_t)m * K * nk2; ++t)
            if (left[t] < 0 || left[t] >= nl || right[t] < 0 || right[t] >= nl) { set_error("%s: an index outside 0..nl-1", who); return OEMGPU_ERR_ARG; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    std::vector<int32_t> pen(npen, OEMGPU_LASSO);
    oemgpu_opts o;
    memset(&o, 0, sizeof o);
    o.npen = npen; o.penalty = pen.data(); o.nlambda = nl;
    if (nb > m) nb = m;
    const CvMultiLay W = cv_multi_layout(c->num_cu, n, p, K, m, &o, 0, false, nb);       // (nothing is solved: the chunk is the caller's nb)
    if (ctx_aux(c, W.total)) return OEMGPU_ERR_HIP;
    const XvalLay &L = W.V.L;
    char *ax = c->aux;
    std::vector<int64_t> hf;
    double *Yp = (double *)(ax + W.V.a_yp), *tab = (double *)(ax + W.V.a_tab), *raw = (double *)(ax + W.a_raw), *tri = (double *)(ax + W.a_tri);
    const MultiY Y{y_dev, y_rs, y_cs};
    const double *y0 = y_dev;                                        // response 0 rides along as y
    if (y_rs != 1) { if ((rc = launch_multi_column(c->stream, Y, n, 0, (double *)(ax + W.V.a_col)))) return rc; y0 = (const double *)(ax + W.V.a_col); }
    if ((rc = xval_prepare(c, L, dense_src_cm(x_dev, ld), y0, nullptr, foldid_dev, hf, false))) return rc;
    if ((rc = launch_gather_responses(c->stream, y_dev, y_rs, y_cs, n, m, (const int *)(ax + L.a_pos), Yp, L.ldp))) return rc;
    const int64_t *fold_n = (const int64_t *)(ax + L.a_fn), *fold_start = fold_n + K;
    CvInterpIdx *idx_dev = (CvInterpIdx *)(ax + W.a_idx);
    int *ncol_dev = (int *)(ax + W.a_ncol), *inv = (int *)(ax + W.a_inv);
    if (predmat_dev) if ((rc = launch_fold_inverse(c->stream, (const int *)(ax + L.a_pos), n, L.ldp, inv))) return rc;
    std::vector<CvInterpIdx> hidx;
    for (int r0 = 0; r0 < m; r0 += nb) {
        const int cb = m - r0 < nb ? m - r0 : nb;
        OEM_HIP(hipMemcpyAsync(ncol_dev, ncol + (size_t)npen * r0, sizeof(int) * (size_t)npen * cb, hipMemcpyHostToDevice, c->stream));
        if (left) {
            hidx.resize((size_t)cb * K * nk2);
            for (size_t t = 0; t < hidx.size(); ++t) { const size_t g = (size_t)r0 * K * nk2 + t; hidx[t] = CvInterpIdx{left[g], right[g], frac[g]}; }
            OEM_HIP(hipMemcpyAsync(raw, coef + blen * K * r0, sizeof(double) * blen * K * cb, hipMemcpyHostToDevice, c->stream));
            OEM_HIP(hipMemcpyAsync(idx_dev, hidx.data(), sizeof(CvInterpIdx) * hidx.size(), hipMemcpyHostToDevice, c->stream));
            if ((rc = launch_cv_interp(c->stream, raw, idx_dev, ncol_dev, cb, K, npen, nl, p, tab))) return rc;
            if (table_out) OEM_HIP(hipMemcpyAsync(table_out + blen * K * r0, tab, sizeof(double) * blen * K * cb, hipMemcpyDeviceToHost, c->stream));
        } else OEM_HIP(hipMemcpyAsync(tab, coef + blen * K * r0, sizeof(double) * blen * K * cb, hipMemcpyHostToDevice, c->stream));
        rc = launch_cv_fold_error_many(c->stream, (const double *)(ax + L.a_xp), L.ldp, Yp + (size_t)L.ldp * r0, fold_start, fold_n, K, p, tab, npen, nl,
                                       type_measure, W.V.cv, cb, (double *)(ax + W.V.a_cvpart), ncol_dev, tri,
                                       predmat_dev ? predmat_dev + nk2 * (size_t)n * r0 : nullptr, inv, n);
        if (rc) return rc;
        OEM_HIP(hipMemcpyAsync(triples + 3 * nk2 * K * r0, tri, sizeof(double) * 3 * nk2 * K * cb, hipMemcpyDeviceToHost, c->stream));
        OEM_HIP(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// rows [r0, r1) of the host data resident on the context's device: x (leading dimension *ld), y, foldid and the weights
static int xval_upload_rows(oemgpu_ctx *c, const double *x, int64_t n, int32_t p, const double *y, const double *weights, const int32_t *foldid,
                            int64_t r0, int64_t r1, const oemgpu_opts *o, double **xd, int64_t *ld, double **yd, double **wd, int32_t **fd)
{
    const int64_t nr = r1 - r0;
    int rc = host_upload_resident(c, x + r0, nr, p, y + r0, o, xd, ld, yd, n);   // staged through the pinned lanes, leaves room for foldid behind y
    if (rc) return rc;
    *fd = (int32_t *)(*yd + ((nr + 2 + 31) / 32 * 32));
    *wd = nullptr;
    hipError_t e = hipMemcpyAsync(*fd, foldid + r0, sizeof(int32_t) * (size_t)nr, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { set_error("upload of foldid failed: %s", hipGetErrorString(e)); return OEMGPU_ERR_HIP; }
    if (weights) {                                               // the rows' weights in the accumulator buffer of the host path (grow-only)
        rc = ctx_grow(c, &c->acc, &c->acc_bytes, sizeof(double) * (size_t)(nr + 2));
        if (rc) return rc;
        *wd = (double *)c->acc;
        if (hipMemcpyAsync(*wd, weights + r0, sizeof(double) * (size_t)nr, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
            set_error("upload of the weights failed"); return OEMGPU_ERR_HIP;
        }
    }
    return 0;
}

// opts.ngpus > 1: the three phases of the call (xval_prepare / xval_solve / xval_cverr) with the rows split over the devices like
// oemgpu_fit_dense does (floor(n / G) each, the remainder on the last), one host thread per device for the two row-bound phases:
// the fold moments are handed to the first device by peer copies and added in device order, the K + 1 fits run there, the fold
// coefficients go back to every device, and the error triples of the devices' rows merge on the host (oemgpu_xval_merge).
static int xval_dense_devices(const std::vector<int> &dev, const double *x, int64_t n, int32_t p, const double *y, const double *weights,
                              const int32_t *foldid, int32_t K, int32_t standardize, int32_t intercept, int32_t type_measure,
                              const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d,
                              double *cvm, double *cvsd)
{
    const int G = (int)dev.size(), npen = o->npen, nl = nl_of(o);
    struct Part {
        oemgpu_ctx *c = nullptr;
        int64_t r0 = 0, r1 = 0, ld = 0;
        double *xd = nullptr, *yd = nullptr, *wd = nullptr;
        int32_t *fd = nullptr;
        XvalLay L;
        std::vector<int64_t> hf;
        std::vector<double> tri;
        int rc = 0;
        std::string err;
    };
    std::vector<Part> P(G);
    auto release_all = [&]() { for (Part &q : P) if (q.c) { (void)hipSetDevice(q.c->device); (void)hipStreamSynchronize(q.c->stream); ctx_release(q.c); q.c = nullptr; } };
    for (int g = 0; g < G; ++g) {
        oemgpu_row_split(n, G, g, &P[g].r0, &P[g].r1);
        if (P[g].r1 - P[g].r0 < 1) { release_all(); set_error("xval_dense: fewer rows than devices"); return OEMGPU_ERR_ARG; }
        P[g].c = ctx_acquire(dev[g]);
        if (!P[g].c) { release_all(); return OEMGPU_ERR_NO_DEVICE; }
    }
    auto each = [&](auto &&work) -> int {                           // work(g) on one host thread per device; the first failure, in device order
        std::vector<std::thread> th;
        auto run = [&](int g) {
            P[g].rc = set_device(P[g].c) ? OEMGPU_ERR_HIP : work(g);
            if (P[g].rc) P[g].err = oemgpu_last_error();                // the message lives in the worker's thread
        };
        for (int g = 1; g < G; ++g) th.emplace_back(run, g);
        run(0);
        for (auto &t : th) t.join();
        for (int g = 0; g < G; ++g) if (P[g].rc) { set_error("device %d: %s", dev[g], P[g].err.c_str()); return P[g].rc; }
        return 0;
    };
    // ---- phase 1: rows up, into fold order, per-fold moments
    int rc = each([&](int g) -> int {
        Part &q = P[g];
        int r = xval_upload_rows(q.c, x, n, p, y, weights, foldid, q.r0, q.r1, o, &q.xd, &q.ld, &q.yd, &q.wd, &q.fd);
        if (r) return r;
        q.L = xval_layout(q.c, q.r1 - q.r0, p, K, npen, nl, weights != nullptr);
        if (ctx_aux(q.c, q.L.total)) return OEMGPU_ERR_HIP;
        return xval_prepare(q.c, q.L, dense_src_cm(q.xd, q.ld), q.yd, q.wd, q.fd, q.hf);
    });
    if (rc) { release_all(); return rc; }
    // ---- the fold moments of devices 1 .. G-1 into device 0's, in device order (bitwise reproducible); fold sizes on the host
    std::vector<int64_t> fold_tot(K, 0);
    for (int g = 0; g < G; ++g) for (int k = 0; k < K; ++k) fold_tot[k] += P[g].hf[k];
    Part &Z = P[0];
    const size_t mlenK = Z.L.mlen * K, cslenK = Z.L.cslen * K;
    double *peer = (double *)(Z.c->aux + Z.L.a_peer);
    for (int g = 1; g < G && !rc; ++g) {
        Part &q = P[g];
        // the staging area is reused for every peer: the add of peer g-1 must have read it before peer g overwrites it
        if (set_device(Z.c) || hipEventRecord(Z.c->xfer_ev, Z.c->stream) != hipSuccess || set_device(q.c) ||
            hipStreamWaitEvent(q.c->stream, Z.c->xfer_ev, 0) != hipSuccess) { set_error("xval_dense: event ordering failed"); rc = OEMGPU_ERR_HIP; break; }
        rc = host_hand_over(Z.c, peer, q.c, (const double *)(q.c->aux + q.L.a_mf), mlenK);
        if (!rc && weights) rc = host_hand_over(Z.c, peer + mlenK, q.c, (const double *)(q.c->aux + q.L.a_cs), cslenK);
        if (!rc) rc = set_device(Z.c) ? OEMGPU_ERR_HIP : host_add_into(Z.c, (double *)(Z.c->aux + Z.L.a_mf), peer, mlenK);
        if (!rc && weights) rc = host_add_into(Z.c, (double *)(Z.c->aux + Z.L.a_cs), peer + mlenK, cslenK);
    }
    // ---- phase 2 on the first device: the K + 1 fits; the fold coefficients back to every device
    if (!rc) rc = set_device(Z.c) ? OEMGPU_ERR_HIP : xval_solve(Z.c, Z.L, fold_tot.data(), n, standardize, intercept, o, beta, lambda_out, niter, loss, d);
    const size_t blenK = (size_t)K * npen * nl * (p + 1);
    for (int g = 1; g < G && !rc; ++g)
        rc = host_hand_over(P[g].c, (double *)(P[g].c->aux + P[g].L.a_b), Z.c, (const double *)(Z.c->aux + Z.L.a_b), blenK);
    // ---- phase 3: the error triples of every device's rows, merged in device order
    if (!rc) rc = each([&](int g) -> int {
        P[g].tri.assign((size_t)3 * npen * nl, 0.0);
        return xval_cverr(P[g].c, P[g].L, type_measure, o, nullptr, nullptr, P[g].tri.data());
    });
    if (!rc) {
        std::vector<double> all;
        for (int g = 0; g < G; ++g) all.insert(all.end(), P[g].tri.begin(), P[g].tri.end());
        rc = oemgpu_xval_merge(all.data(), G, o, cvm, cvsd);
    }
    release_all();
    return rc;
}

int oemgpu_xval_dense(const double *x, int64_t n, int32_t p, const double *y, const double *weights, const int32_t *foldid, int32_t nfolds,
                      int32_t standardize, int32_t intercept, int32_t type_measure, const oemgpu_opts *o,
                      double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, double *cvm, double *cvsd)
{
    if (!x || !y || !foldid || !o) { set_error("xval_dense: NULL argument"); return OEMGPU_ERR_ARG; }
    int rc = check_opts(o, p, p + (intercept ? 1 : 0));
    if (rc) return rc;
    if (n < 1) { set_error("xval_dense: bad n"); return OEMGPU_ERR_ARG; }
    if (o->ngpus > 1) {
        if (!beta || !lambda_out || !niter || !loss || !d || !cvm || !cvsd) { set_error("xval_dense: NULL argument"); return OEMGPU_ERR_ARG; }
        std::vector<int> dev;
        if ((rc = host_device_list(o, dev)) != 0) return rc;
        rc = xval_check(nullptr, x, y, foldid, n, n, p, nfolds, intercept, type_measure, weights != nullptr, o);
        if (rc) return rc;
        if (n <= p) { set_error("dimension of x larger than number of observations"); return OEMGPU_ERR_UNSUPPORTED; }
        return xval_dense_devices(dev, x, n, p, y, weights, foldid, nfolds, standardize, intercept, type_measure, o, beta, lambda_out,
                                  niter, loss, d, cvm, cvsd);
    }
    oemgpu_ctx *c = ctx_acquire(o->device);
    if (!c) return OEMGPU_ERR_NO_DEVICE;
    double *xd = nullptr, *yd = nullptr, *wd = nullptr;
    int32_t *fd = nullptr;
    int64_t ld = 0;
    rc = xval_upload_rows(c, x, n, p, y, weights, foldid, 0, n, o, &xd, &ld, &yd, &wd, &fd);
    if (!rc) rc = oemgpu_xval_dense_dev(c, xd, n, ld, p, yd, wd, fd, nfolds, standardize, intercept, type_measure, o, beta, lambda_out,
                                        niter, loss, d, cvm, cvsd);
    (void)hipStreamSynchronize(c->stream);
    ctx_release(c);
    return rc;
}

// ---------------------------------------------------------------------------------------------- xval.oem on a sparse x
// Thread-local phase times of the last oemgpu_xval_sparse call (HIP events on the call's stream): upload, fold order (layout, permuted
// columns, chunk pointers), fold moments, compressed rows, the K + 1 fits, CV error
static thread_local double g_xvs_ms[OEMGPU_XVS_NPHASES] = {0, 0, 0, 0, 0, 0};

enum { XVS_FULL = 0, XVS_MOMENTS = 1, XVS_CVERR = 2 };

// Phases 1 - 3 of the fold routes on a sparse x, over compressed columns (cd, rd, vd), y and foldid that are on the device -- xval.oem's
// upload, or an oemgpu_sparse_x and the caller's vectors (cv.oem):
//   1  fold order: launch_fold_layout with every fold segment on a multiple of CSC_CHUNK rows, hf <- the fold sizes [K] and starts [K],
//      the chunk ranges, the columns rewritten in that row order, their chunk pointers;
//   2  (moments) the K fold moment buffers about 0 from ONE pass over the non-zeros, on the route of sparse_route;
//   3  (rows) the fold-ordered compressed rows.
// mark() after every phase that ran.  From the device: OEMGPU_ERR_ARG, in `who`'s name, for a fold id outside 1..K.
struct XvsHost { std::vector<int64_t> hf; std::vector<int32_t> rtab, frange; };   // the caller's: copies enqueued here read them
static int xvs_fold_phases(oemgpu_ctx *c, const XvalSparsePlan &SP, const XvalLay &L, const int64_t *cd, const int32_t *rd, const double *vd,
                           const double *yd, const int32_t *fd, int64_t maxcol, bool moments, bool rows, XvsHost &H, const std::function<void()> &mark,
                           const char *who)
{
    std::vector<int64_t> &hf = H.hf;
    std::vector<int32_t> &rtab = H.rtab, &frange = H.frange;
    const int64_t n = L.n;
    const int K = L.K, p = L.p;
    hipStream_t s = c->stream;
    char *ax = c->aux, *sx = c->aux + L.total;
    int64_t *rowptr = (int64_t *)(sx + SP.a_rowptr);
    int32_t *prow = (int32_t *)(sx + SP.a_prow), *cfo = (int32_t *)(sx + SP.a_cfo), *cptr = (int32_t *)(sx + SP.a_cptr), *ccol = (int32_t *)(sx + SP.a_ccol),
            *rtab_d = (int32_t *)(sx + SP.a_rtab);
    double *pval = (double *)(sx + SP.a_pval), *cval = (double *)(sx + SP.a_cval);
    int *blockcnt = (int *)(ax + L.a_cnt), *bad = (int *)(ax + L.a_bad), *pos = (int *)(ax + L.a_pos);
    int64_t *fold_n = (int64_t *)(ax + L.a_fn), *fold_start = fold_n + K;
    double *yp = (double *)(ax + L.a_yp), *mfold = (double *)(ax + L.a_mf);
    // ---- phase 1: fold order
    int rc = launch_fold_layout(s, fd, n, K, blockcnt, fold_n, fold_start, pos, bad, CSC_CHUNK);
    if (rc) return rc;
    hf.assign(2 * (size_t)K, 0);
    int hbad = 0;
    OEM_HIP(hipMemcpyAsync(hf.data(), fold_n, sizeof(int64_t) * 2 * K, hipMemcpyDeviceToHost, s));
    OEM_HIP(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, s));
    OEM_HIP(hipStreamSynchronize(s));
    if (hbad) { set_error("%s: foldid must hold values in 1..nfolds", who); return OEMGPU_ERR_ARG; }
    int64_t npad = 0;
    rc = xval_sparse_ranges(SP, hf.data(), rtab, frange, &npad);
    if (rc) return rc;
    const int nrange = (int)rtab.size() - 1, nchunk = (int)(npad / CSC_CHUNK);
    int32_t *frange_d = rtab_d + SP.nrange_max + 1;
    OEM_HIP(hipMemcpyAsync(rtab_d, rtab.data(), sizeof(int32_t) * rtab.size(), hipMemcpyHostToDevice, s));
    OEM_HIP(hipMemcpyAsync(frange_d, frange.data(), sizeof(int32_t) * frange.size(), hipMemcpyHostToDevice, s));
    rc = launch_csc_fold_permute(s, cd, rd, vd, yd, fd, pos, n, p, K, npad, cfo, prow, pval, yp);
    if (!rc) rc = launch_csc_chunk_ptr(s, cd, prow, npad, p, cptr);
    if (rc) return rc;
    mark();
    // ---- phase 2: the K fold moment buffers from one pass over the non-zeros
    if (moments) {
        if (SP.R.csc) {
            rc = launch_csc_fold_moments(s, cd, prow, pval, yp, cptr, cfo, fold_start, fold_n, p, K, nchunk, nrange, rtab_d, frange_d,
                                         (double *)(sx + SP.a_gpart), (double *)(sx + SP.a_ypart), mfold);
            if (rc) return rc;
        } else {
            for (int k = 0; k < K; ++k) {
                double *Mk = mfold + L.mlen * k;
                if (hf[k] == 0) { OEM_HIP(hipMemsetAsync(Mk, 0, sizeof(double) * L.mlen, s)); continue; }
                rc = csc_tile_moments(c, SP.R, cd, prow, pval, nullptr, yp, npad, p, maxcol, (double *)(sx + SP.a_tile), (double *)(ax + L.a_t),
                                      (double *)(ax + L.a_v), (double *)(sx + SP.a_mtile), Mk, hf[K + k], hf[k]);
                if (rc) return rc;
            }
        }
        mark();
    }
    // ---- phase 3: the compressed-row copy of the fold-ordered matrix
    if (rows) {
        rc = launch_csr_rowptr(s, cd, prow, cptr, p, nchunk, rowptr);
        if (!rc) rc = launch_csc_to_csr(s, cd, prow, pval, cptr, npad, p, rowptr, ccol, cval);
        if (rc) return rc;
        mark();
    }
    return 0;
}

// The call in one place; the two selftests stop early (XVS_MOMENTS: after the K moment buffers) or skip the fits (XVS_CVERR: coefficients
// of the caller's).  mode != XVS_FULL: o is NULL, npen / nl are the caller's.
static int xval_sparse_impl(int mode, int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values, const double *y,
                            const int32_t *foldid, int32_t K, int32_t standardize, int32_t intercept, int32_t type_measure, const oemgpu_opts *o,
                            int npen, int nl, const double *coef, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d,
                            double *cvm, double *cvsd, double *triples, double *moments_out, oemgpu_ctx *cres = nullptr,
                            const oemgpu_sparse_x *xres = nullptr)
{
    // xres (oemgpu_xval_sparse_res): the columns are the handle's, y and foldid the caller's device vectors, cres the caller's context
    const char *who = mode == XVS_FULL ? "xval_sparse" : (mode == XVS_MOMENTS ? "selftest_xval_sparse_fold_moments" : "selftest_xval_sparse_cv_error");
    int rc = 0;
    if (mode == XVS_FULL) {
        rc = check_opts(o, p, p + (intercept ? 1 : 0));
        if (rc) return rc;
        npen = o->npen; nl = nl_of(o);
    } else if (p < 1 || npen < 1 || nl < 1) { set_error("%s: bad p, npen or nl", who); return OEMGPU_ERR_ARG; }
    if (n < 1) { set_error("xval_sparse: bad n"); return OEMGPU_ERR_ARG; }
    const int64_t maxcol = xres ? xres->maxcol : csc_check(who, n, p, colptr, rowidx, values, nullptr);     // first, as in oemgpu_fit_sparse (it reads rows against n: n >= 1 comes before it)
    if (maxcol < 0) return (int)maxcol;
    if (K < 2 || K > 512) { set_error("xval_dense: nfolds must be in 2..512"); return OEMGPU_ERR_ARG; }
    if (type_measure != 0 && type_measure != 1) { set_error("xval_dense: type_measure must be 0 (mse) or 1 (mae)"); return OEMGPU_ERR_ARG; }
    if (n + (int64_t)CSC_CHUNK * K >= (int64_t)1 << 31) { set_error("xval_sparse: n too large for 32-bit row positions"); return OEMGPU_ERR_UNSUPPORTED; }
    if (mode == XVS_FULL && n <= p) { set_error("dimension of x larger than number of observations"); return OEMGPU_ERR_UNSUPPORTED; }   // ref src/oem_xval_dense.h:690-731
    const int64_t nnz = xres ? xres->nnz : colptr[p];
    if (xres && set_device(cres)) return OEMGPU_ERR_HIP;
    oemgpu_ctx *c = xres ? cres : ctx_acquire(o ? o->device : -1);
    if (!c) return OEMGPU_ERR_NO_DEVICE;
    struct Release { oemgpu_ctx *c; bool own; ~Release() { (void)hipStreamSynchronize(c->stream); if (own) ctx_release(c); } } release{c, xres == nullptr};
    hipStream_t s = c->stream;
    if (!c->xvs_ev_made) {
        for (int i = 0; i <= OEMGPU_XVS_NPHASES; ++i) OEM_HIP(hipEventCreate(&c->xvs_ev[i]));
        c->xvs_ev_made = true;
    }
    int nmark = 0;
    auto mark = [&]() { if (nmark <= OEMGPU_XVS_NPHASES) (void)hipEventRecord(c->xvs_ev[nmark++], s); };
    for (double &v : g_xvs_ms) v = 0.0;

    const XvalSparsePlan SP = xval_sparse_plan(n, p, nnz, K, npen, nl, c->num_cu, xres != nullptr);     // (resident: no slots for the uploaded copies)
    const XvalLay L = xval_layout(c->num_cu, n, p, K, npen, nl, false, &SP);
    ctx_void_cv(c);
    if (ctx_aux(c, L.total + SP.bytes)) return OEMGPU_ERR_HIP;
    char *ax = c->aux, *sx = c->aux + L.total;
    const int64_t *cd = xres ? xres->colptr : (int64_t *)(sx + SP.a_col);
    int64_t *rowptr = (int64_t *)(sx + SP.a_rowptr);
    const int32_t *rd = xres ? xres->rowidx : (int32_t *)(sx + SP.a_row), *fd = xres ? foldid : (int32_t *)(sx + SP.a_fid);
    int32_t *ccol = (int32_t *)(sx + SP.a_ccol);
    const double *vd = xres ? xres->val : (double *)(sx + SP.a_val), *yd = xres ? y : (double *)(sx + SP.a_y);
    double *cval = (double *)(sx + SP.a_cval);
    int64_t *fold_n = (int64_t *)(ax + L.a_fn), *fold_start = fold_n + K;
    double *yp = (double *)(ax + L.a_yp), *mfold = (double *)(ax + L.a_mf), *bdev = (double *)(ax + L.a_b);

    // ---- phase 0: the compressed columns, y and foldid up, once
    mark();
    if (!xres) {
        OEM_HIP(hipMemcpyAsync((void *)cd, colptr, sizeof(int64_t) * (size_t)(p + 1), hipMemcpyHostToDevice, s));
        if (nnz > 0) {
            OEM_HIP(hipMemcpyAsync((void *)rd, rowidx, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, s));
            OEM_HIP(hipMemcpyAsync((void *)vd, values, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, s));
        }
        OEM_HIP(hipMemcpyAsync((void *)yd, y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
        OEM_HIP(hipMemcpyAsync((void *)fd, foldid, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    }
    // ---- phases 1 - 3: fold order, the K fold moment buffers, the fold-ordered compressed rows
    mark();
    XvsHost H;
    rc = xvs_fold_phases(c, SP, L, cd, rd, vd, yd, fd, maxcol, true, mode != XVS_MOMENTS, H, mark, "xval_dense");   // (the message xval.oem has always given)
    if (rc) return rc;
    const std::vector<int64_t> &hf = H.hf;
    if (mode == XVS_MOMENTS) {
        OEM_HIP(hipMemcpyAsync(moments_out, mfold, sizeof(double) * L.mlen * K, hipMemcpyDeviceToHost, s));
        OEM_HIP(hipStreamSynchronize(s));
        return 0;
    }
    // ---- phase 4: the K + 1 fits (xval_solve as it is: the moment buffers carry the column sums and n)
    if (mode == XVS_FULL) rc = xval_solve(c, L, hf.data(), n, standardize, intercept, o, beta, lambda_out, niter, loss, d);
    else OEM_HIP(hipMemcpyAsync(bdev, coef, sizeof(double) * (size_t)K * npen * nl * (p + 1), hipMemcpyHostToDevice, s));
    if (rc) return rc;
    mark();
    // ---- phase 5: CV error over the compressed rows
    double *cvout = (double *)(ax + L.a_out);
    rc = launch_csr_cv_error(s, SP, rowptr, ccol, cval, yp, fold_start, fold_n, bdev, (double *)(sx + SP.a_bt), type_measure, (double *)(ax + L.a_part),
                             cvout, triples != nullptr);
    if (rc) return rc;
    mark();
    const size_t nk = (size_t)npen * nl;
    std::vector<double> hc((triples ? 3 : 2) * nk);
    OEM_HIP(hipMemcpyAsync(hc.data(), cvout, sizeof(double) * hc.size(), hipMemcpyDeviceToHost, s));
    OEM_HIP(hipStreamSynchronize(s));                           // coef and hc are the caller's and a local
    for (int i = 0; i + 1 < nmark && i < OEMGPU_XVS_NPHASES; ++i) {
        float f = 0.f;
        if (hipEventElapsedTime(&f, c->xvs_ev[i], c->xvs_ev[i + 1]) == hipSuccess) g_xvs_ms[i] = f;
    }
    if (triples) { memcpy(triples, hc.data(), sizeof(double) * hc.size()); return 0; }
    for (int k = 0; k < npen; ++k) {
        const int nlam = (o && o->penalty[k] == OEMGPU_OLS) ? 1 : nl;      // (the selftest masks nothing)
        for (int i = 0; i < nl; ++i) {
            const size_t ki = (size_t)k * nl + i;
            cvm[ki] = i < nlam ? hc[2 * ki] : 0.0;
            cvsd[ki] = i < nlam ? hc[2 * ki + 1] : 0.0;
        }
    }
    return 0;
}

int oemgpu_xval_sparse(int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values, const double *y,
                       const int32_t *foldid, int32_t nfolds, int32_t standardize, int32_t intercept, int32_t type_measure, const oemgpu_opts *o,
                       double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, double *cvm, double *cvsd)
{
    if (!colptr || !y || !foldid || !o || !beta || !lambda_out || !niter || !loss || !d || !cvm || !cvsd) {
        set_error("xval_sparse: NULL argument"); return OEMGPU_ERR_ARG;
    }
    if (o->ngpus > 1) { set_error("xval_sparse: the rows of a sparse x are not split over devices"); return OEMGPU_ERR_UNSUPPORTED; }
    return xval_sparse_impl(XVS_FULL, n, p, colptr, rowidx, values, y, foldid, nfolds, standardize, intercept, type_measure, o, 0, 0, nullptr,
                            beta, lambda_out, niter, loss, d, cvm, cvsd, nullptr, nullptr);
}

int oemgpu_last_xval_sparse_timings(double *ms)
{
    if (!ms) { set_error("NULL argument"); return OEMGPU_ERR_ARG; }
    for (int i = 0; i < OEMGPU_XVS_NPHASES; ++i) ms[i] = g_xvs_ms[i];
    return 0;
}

int oemgpu_selftest_xval_sparse_plan(int64_t n, int32_t p, int64_t nnz, int32_t nfolds, int32_t npen, int32_t nl, int32_t num_cu, int64_t *out)
{
    if (n < 1 || p < 1 || nnz < 0 || npen < 1 || nl < 1 || num_cu < 1 || !out) { set_error("selftest_xval_sparse_plan: bad argument"); return OEMGPU_ERR_ARG; }
    if (nfolds < 2 || nfolds > 512) { set_error("selftest_xval_sparse_plan: nfolds must be in 2..512"); return OEMGPU_ERR_ARG; }
    if (n + (int64_t)CSC_CHUNK * nfolds >= (int64_t)1 << 31) { set_error("xval_sparse: n too large for 32-bit row positions"); return OEMGPU_ERR_UNSUPPORTED; }
    const XvalSparsePlan SP = xval_sparse_plan(n, p, nnz, nfolds, npen, nl, num_cu);
    const XvalLay L = xval_layout(num_cu, n, p, nfolds, npen, nl, false, &SP);
    // the ranges of the worst case for one fold: n - K + 1 rows in the first fold, one row in every other (n >= K), through the function the call uses
    std::vector<int64_t> fn((size_t)nfolds, n >= nfolds ? 1 : 0);
    fn[0] = n >= nfolds ? n - nfolds + 1 : n;
    std::vector<int32_t> rtab, frange;
    int64_t npad = 0;
    int rc = xval_sparse_ranges(SP, fn.data(), rtab, frange, &npad);
    if (rc) return rc;
    out[0] = SP.R.csc ? 1 : 0; out[1] = SP.nchunk_max; out[2] = SP.per; out[3] = SP.rpf_max; out[4] = SP.nrange_max; out[5] = SP.R.rows;
    out[6] = SP.cv_nwg; out[7] = SP.cv_waves; out[8] = SP.cv_lblk; out[9] = (int64_t)(L.total + SP.bytes); out[10] = CSC_CHUNK;
    out[11] = SP.R.csc ? (int64_t)csc_gram_lds_bytes(p) : 0; out[12] = frange[1] - frange[0]; out[13] = (int64_t)rtab.size() - 1;
    out[14] = npad; out[15] = rtab[frange[1]];
    const int64_t ntile = csc_tiles(SP.R, fn[0]);
    int64_t t0 = 0, t1 = 0;
    csc_tile_rows(SP.R, 0, fn[0], ntile - 1, &t0, &t1);
    out[16] = ntile; out[17] = t1;
    return 0;
}

int oemgpu_selftest_xval_sparse_fold_moments(int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values,
                                             const double *y, const int32_t *foldid, int32_t nfolds, double *moments_out)
{
    if (!colptr || !y || !foldid || !moments_out) { set_error("selftest_xval_sparse_fold_moments: NULL argument"); return OEMGPU_ERR_ARG; }
    return xval_sparse_impl(XVS_MOMENTS, n, p, colptr, rowidx, values, y, foldid, nfolds, 0, 0, 0, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr, nullptr, nullptr, moments_out);
}

int oemgpu_selftest_xval_sparse_cv_error(int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values, const double *y,
                                         const int32_t *foldid, int32_t nfolds, const double *coef, int32_t npen, int32_t nl, int32_t type_measure,
                                         double *cvm, double *cvsd, double *triples)
{
    if (!colptr || !y || !foldid || !coef || (!triples && (!cvm || !cvsd))) { set_error("selftest_xval_sparse_cv_error: NULL argument"); return OEMGPU_ERR_ARG; }
    return xval_sparse_impl(XVS_CVERR, n, p, colptr, rowidx, values, y, foldid, nfolds, 0, 0, type_measure, nullptr, npen, nl, coef, nullptr, nullptr,
                            nullptr, nullptr, nullptr, cvm, cvsd, triples, nullptr);
}

// ---------------------------------------------------------------------------------------------- cv.oem, family = "gaussian", sparse x
// One layout function for the whole call (the entries and oemgpu_selftest_cv_sparse_plan read it): xval.oem's sparse plan without the
// upload regions (the handle holds the columns), the xval layout in front of it, and behind both this route's own regions -- the
// per-fold wave partials of the scoring launch, the per-fold triples, the valid columns per penalty, the inverse of the fold
// permutation for the prediction store, the diagonal of a summed moment buffer on its way to the host (intval).
struct CvSparseLay {
    XvalSparsePlan SP;
    XvalLay L;
    CvSparseScorePlan S;
    size_t a_part, a_tri, a_ncol, a_inv, a_diag, own, total;
};
static CvSparseLay cv_sparse_layout(int num_cu, int64_t n, int p, int64_t nnz, int K, int npen, int nl)
{
    CvSparseLay V;
    V.SP = xval_sparse_plan(n, p, nnz, K, npen, nl, num_cu, true);
    V.L = xval_layout(num_cu, n, p, K, npen, nl, false, &V.SP);
    V.S = cv_sparse_score_plan(n, K, npen, nl, num_cu);
    Bump A; A.off = V.L.total + V.SP.bytes;
    V.a_part = A.take(V.S.part_bytes); V.a_tri = A.take(sizeof(double) * 3 * (size_t)K * npen * nl); V.a_ncol = A.take(sizeof(int) * (size_t)npen);
    V.a_inv = A.take(sizeof(int) * (size_t)V.SP.npad_max); V.a_diag = A.take(sizeof(double) * (size_t)p);
    V.total = A.off;
    V.own = V.total - V.L.total - V.SP.bytes;
    return V;
}

static int cv_sparse_check_rows(const char *who, int64_t n, int p, int K)
{
    if (K < 2 || K > 512) { set_error("%s: nfolds must be in 2..512", who); return OEMGPU_ERR_ARG; }
    if (n < 1 || p < 1) { set_error("%s: bad n or p", who); return OEMGPU_ERR_ARG; }
    if (n + (int64_t)CSC_CHUNK * K >= (int64_t)1 << 31) { set_error("%s: n too large for 32-bit row positions", who); return OEMGPU_ERR_UNSUPPORTED; }
    return 0;
}

// phases 1 - 3 on the handle's arrays, and the stamp oemgpu_cv_sparse_score_res looks for; ms != nullptr: the phase times
static int cv_sparse_lay_out(oemgpu_ctx *c, const CvSparseLay &V, const oemgpu_sparse_x *x, const double *y_dev, const int32_t *foldid_dev,
                             bool moments, XvsHost &H, bool timed, const char *who)
{
    ctx_void_cv(c);
    if (ctx_aux(c, V.total)) return OEMGPU_ERR_HIP;
    if (timed && !c->xvs_ev_made) {
        for (int i = 0; i <= OEMGPU_XVS_NPHASES; ++i) OEM_HIP(hipEventCreate(&c->xvs_ev[i]));
        c->xvs_ev_made = true;
    }
    int nmark = 0;
    auto mark = [&]() { if (timed && nmark <= OEMGPU_XVS_NPHASES) (void)hipEventRecord(c->xvs_ev[nmark++], c->stream); };
    mark(); mark();                                              // (no upload phase: the handle holds the columns)
    int rc = xvs_fold_phases(c, V.SP, V.L, x->colptr, x->rowidx, x->val, y_dev, foldid_dev, x->maxcol, moments, true, H, mark, who);
    if (rc) return rc;
    c->cv_n = V.L.n; c->cv_p = V.L.p; c->cv_K = V.L.K; c->cv_aux = c->aux; c->cv_hf = H.hf; c->cv_kind = CV_KIND_SPARSE;
    c->cv_nnz = x->nnz; c->cv_npen = V.L.npen; c->cv_nl = V.L.nl;
    return 0;
}

int oemgpu_cv_sparse_fold_fits_res(oemgpu_ctx *c, const oemgpu_sparse_x *x, const double *y_dev, const int32_t *foldid_dev, int32_t nfolds,
                                   int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                                   double *beta, double *lambda_out, int32_t *niter, double *loss, double *d, int64_t *fold_n)
{
    static const char *who = "cv_sparse_fold_fits";
    if (!c || !x || !y_dev || !foldid_dev || !o || !beta || !lambda_out || !niter || !loss || !d || !fold_n) {
        set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG;
    }
    const int64_t n = x->n;
    const int p = x->p, K = nfolds, q = p + (intercept ? 1 : 0);
    int rc = check_opts(o, p, q);                               // the intercept's group comes first, as in oemgpu_fit_sparse
    if (!rc) rc = cv_sparse_check_rows(who, n, p, K);
    if (rc) return rc;
    // the largest fold holds at least ceil(n / K) rows: some fold fit is then not the Gram form whatever the ids are
    if (n - (n + K - 1) / K <= p) {
        set_error("%s: %lld rows in %d folds leave some fold no more rows than the %d columns", who, (long long)n, K, p);
        return OEMGPU_ERR_UNSUPPORTED;
    }
    if (c->device != x->device) { set_error("%s: the context and the sparse x are on different devices", who); return OEMGPU_ERR_ARG; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const int npen = o->npen, nl = nl_of(o);
    const CvSparseLay V = cv_sparse_layout(c->num_cu, n, p, x->nnz, K, npen, nl);
    const XvalLay &L = V.L;
    for (double &v : g_xvs_ms) v = 0.0;
    XvsHost H;
    rc = cv_sparse_lay_out(c, V, x, y_dev, foldid_dev, true, H, true, who);
    if (rc) return rc;
    const std::vector<int64_t> &hf = H.hf;
    for (int k = 0; k < K; ++k) {
        fold_n[k] = hf[k];
        if (n - hf[k] <= p) {
            set_error("%s: fold %d leaves %lld rows for %d columns (the fit of p >= n is not this route's)", who, k + 1, (long long)(n - hf[k]), p);
            return OEMGPU_ERR_UNSUPPORTED;
        }
    }
    char *ax = c->aux;
    const double *mfold = (const double *)(ax + L.a_mf);
    double *msum = (double *)(ax + L.a_ms), *diag = (double *)(ax + V.a_diag);
    const SparseSolveWs W = sparse_solve_ws(Bump{}, p, q, o);   // the moment buffers live in aux: the workspace holds the solve alone
    if (ctx_reserve(c, W.need)) return OEMGPU_ERR_HIP;
    const size_t blen = (size_t)npen * nl * (p + 1), nk2 = (size_t)npen * nl;
    std::vector<double> hdiag((size_t)p);
    // slot 0: all rows (the sum of ALL fold buffers); slot ff: the rows outside fold ff (R/cv_oem.R:105, 155-175 -> oem_fit_sparse)
    for (int ff = 0; ff <= K; ++ff) {
        double *ms = msum + L.mlen * ff;
        rc = launch_fold_sum(c->stream, mfold, K, L.mlen, ff, ms);
        if (rc) return rc;
        // intval = sqrt(mean(diag(XX)) / n) from the summed buffer's diagonal, the expression of oemgpu_fit_sparse with the kept rows' n
        const double nkept = (double)(n - (ff ? hf[ff - 1] : 0));
        double intval = 1.0;
        if (intercept) {
            hipLaunchKernelGGL(moment_diag_kernel, dim3((p + 255) / 256), dim3(256), 0, c->stream, ms, p, diag);
            OEM_HIP(hipGetLastError());
            OEM_HIP(hipMemcpyAsync(hdiag.data(), diag, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, c->stream));
            OEM_HIP(hipStreamSynchronize(c->stream));
            double xxdiag = 0.0;
            for (int j = 0; j < p; ++j) {
                const double ss = hdiag[j];
                double cs = ss / (nkept - 1.0);
                if (cs == 0.0) cs = 1.0;                          // a column that is empty among the kept rows
                xxdiag += standardize ? ss / cs : ss;
            }
            xxdiag /= (double)p;
            intval = std::sqrt(xxdiag / nkept);
        }
        rc = sparse_solve(c, W, ms, p, q, standardize, intercept, o, intval, beta + blen * ff, lambda_out + nk2 * ff, niter + nk2 * ff,
                          loss + nk2 * ff, d + ff);
        if (rc) { if (ff) { const std::string e = oemgpu_last_error(); set_error("fold %d: %s", ff, e.c_str()); } return rc; }
    }
    (void)hipEventRecord(c->xvs_ev[5], c->stream);
    OEM_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 5; ++i) {
        float f = 0.f;
        if (hipEventElapsedTime(&f, c->xvs_ev[i], c->xvs_ev[i + 1]) == hipSuccess) g_xvs_ms[i] = f;
    }
    return 0;
}

int oemgpu_cv_sparse_score_res(oemgpu_ctx *c, int64_t n, int32_t p, int32_t nfolds, const double *coef, int32_t npen, int32_t nl,
                               const int32_t *ncol, int32_t type_measure, double *triples, double *predmat_dev)
{
    static const char *who = "cv_sparse_score";
    if (!c || !coef || !ncol || !triples) { set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG; }
    if (p < 1 || npen < 1 || nl < 1) { set_error("%s: bad p, npen or nl", who); return OEMGPU_ERR_ARG; }
    const int K = nfolds;
    int rc = cv_sparse_check_rows(who, n, p, K);
    if (rc) return rc;
    if (type_measure != 0 && type_measure != 1) { set_error("%s: type_measure must be 0 (mse) or 1 (mae)", who); return OEMGPU_ERR_ARG; }
    for (int k = 0; k < npen; ++k)
        if (ncol[k] < 0 || ncol[k] > nl) { set_error("%s: ncol[%d] = %d is outside 0..%d", who, k, ncol[k], nl); return OEMGPU_ERR_ARG; }
    if (c->cv_kind != CV_KIND_SPARSE || c->cv_n != n || c->cv_p != p || c->cv_K != K || c->cv_npen != npen || c->cv_nl != nl || !c->aux ||
        c->cv_aux != c->aux || (int)c->cv_hf.size() != 2 * K) {
        set_error("%s: call oemgpu_cv_sparse_fold_fits_res with the same n, p, nfolds, npen and nl on this context first", who); return OEMGPU_ERR_ARG;
    }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const CvSparseLay V = cv_sparse_layout(c->num_cu, n, p, c->cv_nnz, K, npen, nl);
    const XvalLay &L = V.L;
    if (c->aux_bytes < V.total) { set_error("internal: the sparse cv layout is larger than the buffer that holds it"); return OEMGPU_ERR_INTERNAL; }
    char *ax = c->aux, *sx = c->aux + L.total;
    int64_t *fold_n = (int64_t *)(ax + L.a_fn), *fold_start = fold_n + K;
    const int *pos = (const int *)(ax + L.a_pos);
    int *ncol_dev = (int *)(ax + V.a_ncol), *inv = (int *)(ax + V.a_inv);
    double *bdev = (double *)(ax + L.a_b), *tri = (double *)(ax + V.a_tri);
    const size_t blen = (size_t)K * npen * nl * (p + 1), tlen = (size_t)3 * K * npen * nl;
    // the fold sizes and starts go up again from the host copy of phase 1: what the kernels index the rows by is this call's own
    OEM_HIP(hipMemcpyAsync(fold_n, c->cv_hf.data(), sizeof(int64_t) * 2 * K, hipMemcpyHostToDevice, c->stream));
    OEM_HIP(hipMemcpyAsync(bdev, coef, sizeof(double) * blen, hipMemcpyHostToDevice, c->stream));
    OEM_HIP(hipMemcpyAsync(ncol_dev, ncol, sizeof(int) * (size_t)npen, hipMemcpyHostToDevice, c->stream));
    if (predmat_dev) { rc = launch_fold_inverse(c->stream, pos, n, V.SP.npad_max, inv); if (rc) return rc; }
    rc = launch_csr_cv_fold_score(c->stream, V.S, p, (const int64_t *)(sx + V.SP.a_rowptr), (const int32_t *)(sx + V.SP.a_ccol),
                                  (const double *)(sx + V.SP.a_cval), (const double *)(ax + L.a_yp), fold_start, fold_n, bdev,
                                  (double *)(sx + V.SP.a_bt), type_measure, (double *)(ax + V.a_part), ncol_dev, tri, predmat_dev, inv, n);
    if (rc) return rc;
    OEM_HIP(hipMemcpyAsync(triples, tri, sizeof(double) * tlen, hipMemcpyDeviceToHost, c->stream));
    OEM_HIP(hipStreamSynchronize(c->stream));                   // coef, ncol and triples are the caller's
    return 0;
}

// Test infrastructure: the layout and the compressed rows alone -- no moments, nothing fitted, so a fold may leave fewer rows than
// columns -- then oemgpu_cv_sparse_score_res as it is, on a table of the caller's.
int oemgpu_selftest_cv_sparse_score(oemgpu_ctx *c, const oemgpu_sparse_x *x, const double *y_dev, const int32_t *foldid_dev, int32_t nfolds,
                                    const double *coef, int32_t npen, int32_t nl, const int32_t *ncol, int32_t type_measure, double *triples,
                                    double *predmat_dev)
{
    static const char *who = "selftest_cv_sparse_score";
    if (!c || !x || !y_dev || !foldid_dev || !coef || !ncol || !triples) { set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG; }
    if (npen < 1 || nl < 1) { set_error("%s: bad npen or nl", who); return OEMGPU_ERR_ARG; }
    int rc = cv_sparse_check_rows(who, x->n, x->p, nfolds);
    if (rc) return rc;
    if (type_measure != 0 && type_measure != 1) { set_error("%s: type_measure must be 0 (mse) or 1 (mae)", who); return OEMGPU_ERR_ARG; }
    for (int k = 0; k < npen; ++k)
        if (ncol[k] < 0 || ncol[k] > nl) { set_error("%s: ncol[%d] = %d is outside 0..%d", who, k, ncol[k], nl); return OEMGPU_ERR_ARG; }
    if (c->device != x->device) { set_error("%s: the context and the sparse x are on different devices", who); return OEMGPU_ERR_ARG; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const CvSparseLay V = cv_sparse_layout(c->num_cu, x->n, x->p, x->nnz, nfolds, npen, nl);
    XvsHost H;
    rc = cv_sparse_lay_out(c, V, x, y_dev, foldid_dev, false, H, false, who);
    if (rc) return rc;
    return oemgpu_cv_sparse_score_res(c, x->n, x->p, nfolds, coef, npen, nl, ncol, type_measure, triples, predmat_dev);
}

int oemgpu_selftest_cv_sparse_plan(int64_t n, int32_t p, int64_t nnz, int32_t nfolds, int32_t npen, int32_t nl, int32_t num_cu, int64_t *out)
{
    if (nnz < 0 || npen < 1 || nl < 1 || num_cu < 1 || !out) { set_error("selftest_cv_sparse_plan: bad argument"); return OEMGPU_ERR_ARG; }
    int rc = cv_sparse_check_rows("selftest_cv_sparse_plan", n, p, nfolds);
    if (rc) return rc;
    const CvSparseLay V = cv_sparse_layout(num_cu, n, p, nnz, nfolds, npen, nl);
    out[0] = V.SP.R.csc ? 1 : 0; out[1] = V.S.nwg; out[2] = V.S.waves; out[3] = V.S.lblk; out[4] = (int64_t)V.S.part_bytes;
    out[5] = (int64_t)V.total; out[6] = (int64_t)V.L.total; out[7] = (int64_t)V.SP.bytes; out[8] = (int64_t)V.own; out[9] = V.SP.npad_max;
    out[10] = V.S.nl16; out[11] = CSC_CHUNK;
    return 0;
}

// cv.oem's scoring on a resident sparse x with n <= p (ref R/cv_oem.R:376-391; R/utils.R:128-144): the handle's compressed rows in the
// caller's order, the folds' rows from foldid, one fold's table on the device at a time (xval_sparse.hip: csr_cv_wide_score_kernel).
// Everything lives in the context's workspace: the fold buffer (aux) and its cv stamp are neither read nor touched.
static int cv_wide_score_checks(const char *who, int64_t n, int32_t p, int32_t nfolds, int32_t npen, int32_t nl)
{
    if (n < 1 || p < 1 || npen < 1 || nl < 1) { set_error("%s: bad n, p, npen or nl", who); return OEMGPU_ERR_ARG; }
    if (nfolds < 3 || nfolds > 512) { set_error("%s: nfolds must be in 3..512", who); return OEMGPU_ERR_ARG; }
    if (n >= 2147483647LL) { set_error("%s: n must be below 2^31", who); return OEMGPU_ERR_UNSUPPORTED; }
    return 0;
}

int oemgpu_cv_sparse_wide_score_res(oemgpu_ctx *c, const oemgpu_sparse_x *x, const double *y_dev, const int32_t *foldid_dev, int32_t nfolds,
                                    const double *coef, int32_t npen, int32_t nl, const int32_t *ncol, int32_t type_measure, double *triples,
                                    double *predmat_dev)
{
    static const char *who = "cv_sparse_wide_score_res";
    if (!c || !x || !y_dev || !foldid_dev || !coef || !ncol || !triples) { set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG; }
    int rc = cv_wide_score_checks(who, x->n, x->p, nfolds, npen, nl);
    if (rc) return rc;
    if (type_measure != 0 && type_measure != 1) { set_error("%s: type_measure must be 0 (mse) or 1 (mae)", who); return OEMGPU_ERR_ARG; }
    for (int k = 0; k < npen; ++k)
        if (ncol[k] < 0 || ncol[k] > nl) { set_error("%s: ncol[%d] = %d is outside 0..%d", who, k, ncol[k], nl); return OEMGPU_ERR_ARG; }
    if (c->device != x->device) { set_error("%s: the context and the sparse x are on different devices", who); return OEMGPU_ERR_ARG; }
    if (set_device(c)) return OEMGPU_ERR_HIP;
    const int n = (int)x->n, p = x->p, K = nfolds;
    hipStream_t s = c->stream;
    // the per-fold row lists, ascending rows, once per call: n ids down, n rows up (n <= p is small next to the non-zeros)
    std::vector<int32_t> fid((size_t)n), list((size_t)n);
    std::vector<int> start((size_t)K + 1, 0);
    OEM_HIP(hipMemcpyAsync(fid.data(), foldid_dev, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    OEM_HIP(hipStreamSynchronize(s));
    long long bad = 0;
    for (int i = 0; i < n; ++i) { if (fid[i] < 1 || fid[i] > K) ++bad; else ++start[fid[i]]; }
    if (bad) { set_error("%s: %lld fold ids are outside [1, %d]", who, bad, K); return OEMGPU_ERR_ARG; }
    for (int k = 0; k < K; ++k) start[k + 1] += start[k];
    {
        std::vector<int> cur(start.begin(), start.end() - 1);
        for (int i = 0; i < n; ++i) list[(size_t)cur[fid[i] - 1]++] = i;
    }
    const CvWideScorePlan P = cv_wide_score_plan(n, p, K, npen, nl, c->num_cu);
    if (ctx_reserve(c, P.bytes + 4096)) return OEMGPU_ERR_HIP;
    int32_t *list_dev = (int32_t *)(c->ws + P.a_list);
    double *raw = (double *)(c->ws + P.a_raw), *bt = (double *)(c->ws + P.a_bt), *part = (double *)(c->ws + P.a_part), *tri = (double *)(c->ws + P.a_tri);
    int *ncol_dev = (int *)(c->ws + P.a_ncol);
    const size_t flen = (size_t)npen * nl * (p + 1), tlen = (size_t)3 * K * npen * nl, pk = P.part_bytes / sizeof(double) / K;
    OEM_HIP(hipMemcpyAsync(list_dev, list.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    OEM_HIP(hipMemcpyAsync(ncol_dev, ncol, sizeof(int) * (size_t)npen, hipMemcpyHostToDevice, s));
    for (int k = 0; k < K; ++k) {                             // fold by fold: its table up, its rows scored (one stream: the order is the stream's)
        const int nk = start[k + 1] - start[k];
        if (nk > 0) OEM_HIP(hipMemcpyAsync(raw, coef + (size_t)k * flen, sizeof(double) * flen, hipMemcpyHostToDevice, s));
        rc = launch_csr_cv_wide_score_fold(s, P, p, x->rowptr, x->ccol, x->cval, y_dev, list_dev + start[k], nk, raw, bt, type_measure, ncol_dev,
                                           part + (size_t)k * pk, predmat_dev, n);
        if (rc) return rc;
    }
    if ((rc = launch_cv_fold_finish(s, part, P.waves, K, npen, nl, ncol_dev, tri))) return rc;
    OEM_HIP(hipMemcpyAsync(triples, tri, sizeof(double) * tlen, hipMemcpyDeviceToHost, s));
    OEM_HIP(hipStreamSynchronize(s));                           // coef, ncol and triples are the caller's
    return 0;
}

// out[0] waves per fold, [1] workgroups per fold (x npen x out[2]), [2] blocks of 64 lambdas, [3] bytes of ONE staged table
// (p + 1) nl16 8 (npen of them are staged per fold), [4] bytes of the wave partials of all folds, [5] nl16, [6] workspace bytes of the call
int oemgpu_selftest_cv_sparse_wide_score_plan(int64_t n, int32_t p, int32_t nfolds, int32_t npen, int32_t nl, int32_t num_cu, int64_t *out)
{
    static const char *who = "selftest_cv_sparse_wide_score_plan";
    if (num_cu < 1 || !out) { set_error("%s: bad argument", who); return OEMGPU_ERR_ARG; }
    int rc = cv_wide_score_checks(who, n, p, nfolds, npen, nl);
    if (rc) return rc;
    const CvWideScorePlan P = cv_wide_score_plan(n, p, nfolds, npen, nl, num_cu);
    out[0] = P.waves; out[1] = P.nwg; out[2] = P.lblk; out[3] = (int64_t)P.table_bytes; out[4] = (int64_t)P.part_bytes; out[5] = P.nl16;
    out[6] = (int64_t)P.bytes;
    return 0;
}

// What the sparse wide engine's entries check after their NULL arguments, before any device work (the sentences of the fold fit)
static int spw_entry_checks(const char *who, const oemgpu_ctx *c, const oemgpu_sparse_x *x, const int32_t *foldid_dev, int32_t nfolds, int32_t leave_out)
{
    if (nfolds < 3 || nfolds > 512) { set_error("%s: nfolds must be in 3..512", who); return OEMGPU_ERR_ARG; }
    if (leave_out < 0 || leave_out > nfolds) { set_error("%s: leave_out must be in [0, nfolds]", who); return OEMGPU_ERR_ARG; }
    if (leave_out > 0 && !foldid_dev) { set_error("%s: NULL foldid with leave_out > 0", who); return OEMGPU_ERR_ARG; }
    if (c->device != x->device) { set_error("%s: the context and the sparse x are on different devices", who); return OEMGPU_ERR_ARG; }
    if (x->n < 2) { set_error("%s: at least two rows", who); return OEMGPU_ERR_ARG; }
    if (x->n > x->p) {
        set_error("%s: n > p (%lld x %d) is the Gram form's: oemgpu_fit_sparse serves it", who, (long long)x->n, (int)x->p);
        return OEMGPU_ERR_UNSUPPORTED;
    }
    return 0;
}

// The kept rows of a fold (the ids' range whatever is left out); nk = n without fold ids
static int spw_kept_rows(oemgpu_ctx *c, const char *who, const int32_t *foldid_dev, int n, int32_t nfolds, int32_t leave_out, int64_t *nk)
{
    *nk = n;
    if (!foldid_dev) return 0;
    std::vector<int64_t> none;
    const int rc = logit_fold_scan(c, who, foldid_dev, n, nfolds, leave_out, 0, nk, &none);
    if (rc) return rc;
    if (*nk < 2) {
        set_error("%s: fold %d keeps %lld of the %d rows: a fit needs at least two", who, (int)leave_out, (long long)*nk, n);
        return OEMGPU_ERR_ARG;
    }
    return 0;
}

// The engine's setup before its first pass, once for the fit and for oemgpu_selftest_sparse_wide_pass: the mask (only when the fold has
// rows), the lanes -- spw_plan's for the context's CUs, or row_lanes / col_lanes where not 0 --, the engine's workspace in c->aux, the
// lists of the lines longer than 32 x the lanes in force, and the check of the plan's long forms against the lists.  longest: NULL, or
// <- the longest row and column.
static int spw_setup(oemgpu_ctx *c, const oemgpu_sparse_x *x, const int32_t *foldid_dev, int32_t leave_out, int64_t nk, int row_lanes,
                     int col_lanes, SpwArgs &A, int64_t *longest)
{
    const int p = x->p, n = (int)x->n;                       // (n <= p: an int)
    hipStream_t s = c->stream;
    int rc;
    if (leave_out > 0 && nk < n) { A.foldid = foldid_dev; A.leave_out = leave_out; }      // (a fold without rows: the fit of all rows, unmasked)
    A.nk = (int)nk;
    A.colptr = x->colptr; A.rowptr = x->rowptr; A.rowidx = x->rowidx; A.ccol = x->ccol; A.val = x->val; A.cval = x->cval;
    A.n = n; A.p = p;
    A.plan = spw_plan(n, p, x->nnz, 0, 0, c->num_cu, row_lanes, col_lanes);       // (the lanes; the long forms once the lines have been looked at)
    A.long_row_list = A.long_col_list = nullptr; A.n_long_rows = A.n_long_cols = 0;
    Bump X;
    const size_t a_vec = X.take(sizeof(double) * spw_vec_doubles(n)), a_lr = X.take(sizeof(int32_t) * ((size_t)n + 1)),
                 a_lc = X.take(sizeof(int32_t) * ((size_t)p + 1)), a_cnt = X.take(64);
    if (X.off != A.plan.ws_bytes) { set_error("internal: the sparse wide plan and its workspace disagree"); return OEMGPU_ERR_INTERNAL; }
    ctx_void_cv(c);
    if (ctx_grow(c, &c->aux, &c->aux_bytes, X.off)) return OEMGPU_ERR_HIP;
    A.vec = (double *)(c->aux + a_vec);
    int32_t *lrow = (int32_t *)(c->aux + a_lr), *lcol = (int32_t *)(c->aux + a_lc);
    int *cnt = (int *)(c->aux + a_cnt);
    if (ctx_pinned(c, 16384)) return OEMGPU_ERR_HIP;
    if ((rc = launch_spw_scan(s, A, lrow, lcol, cnt))) return rc;
    OEM_HIP(hipMemcpyAsync(c->pinned, cnt, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    OEM_HIP(hipStreamSynchronize(s));
    const int *h = (const int *)c->pinned;
    const int nlr = h[0], nlc = h[2];
    A.plan = spw_plan(n, p, x->nnz, h[1], h[3], c->num_cu, row_lanes, col_lanes);
    if (nlr < 0 || nlr > n || nlc < 0 || nlc > p || (nlr > 0) != (A.plan.long_rows != 0) || (nlc > 0) != (A.plan.long_cols != 0)) {
        set_error("internal: the sparse wide plan and the lists of long lines disagree"); return OEMGPU_ERR_INTERNAL;
    }
    A.long_row_list = lrow; A.long_col_list = lcol; A.n_long_rows = nlr; A.n_long_cols = nlc;
    if (longest) { longest[0] = h[1]; longest[1] = h[3]; }
    return 0;
}

// oem() on a resident sparse x with nobs <= nvars and no intercept: fit_big_wide_dev's iteration (the comment there) with both products
// over the non-zeros of the handle (sparse_wide.hip; path_large.hip: run_path_sparse_wide).  Nothing of n p entries is allocated.
// The ONE body is the fold entry's: leave_out = 0 (or a fold without rows) sets no mask and launches what this entry always launched.
int oemgpu_fit_sparse_wide_res(oemgpu_ctx *c, const oemgpu_sparse_x *x, const double *y_dev, int32_t standardize, const oemgpu_opts *o,
                               double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    int64_t kept = 0;
    return oemgpu_fit_sparse_wide_fold_res(c, x, y_dev, nullptr, 3, 0, standardize, o, beta, lambda_out, niter, loss, d, &kept);
}

// cv.oem's fold fit on the same engine (ref R/cv_oem.R:155-175 -> src/oem_sparse.h:607-612, 638-647, 932-941 on x[keep, ], y[keep]):
// the rows with foldid == leave_out are left out by the masked passes of sparse_wide.hip, the kept-row count stands for n.
int oemgpu_fit_sparse_wide_fold_res(oemgpu_ctx *c, const oemgpu_sparse_x *x, const double *y_dev, const int32_t *foldid_dev, int32_t nfolds,
                                    int32_t leave_out, int32_t standardize, const oemgpu_opts *o, double *beta, double *lambda_out,
                                    int32_t *niter, double *loss, double *d, int64_t *kept)
{
    static const char *who = "fit_sparse_wide";
    if (!c || !x || !y_dev || !o || !beta || !lambda_out || !niter || !loss || !d || !kept) { set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG; }
    int rc = spw_entry_checks(who, c, x, foldid_dev, nfolds, leave_out);
    if (rc) return rc;
    const int p = x->p, n = (int)x->n;                       // (n <= p: an int)
    if ((rc = check_opts(o, p, p))) return rc;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    hipStream_t s = c->stream;
    int64_t nk = n;
    if ((rc = spw_kept_rows(c, who, foldid_dev, n, nfolds, leave_out, &nk))) return rc;
    *kept = nk;
    SpwArgs A;
    if ((rc = spw_setup(c, x, foldid_dev, leave_out, nk, 0, 0, A, nullptr))) return rc;
    Bump B;
    const size_t a_xs2 = B.take((size_t)p * 8), a_xy = B.take((size_t)p * 8), a_st = B.take((size_t)stats_len(p) * 8);       // stats last (run_paths)
    if (ctx_reserve(c, B.off + paths_ws_bytes(p, p, o) + 4096)) return OEMGPU_ERR_HIP;
    double *xy = (double *)(c->ws + a_xy), *st = (double *)(c->ws + a_st), *xy_std = (double *)(c->ws + a_xs2);
    {
        Timer t(c, OEMGPU_T_MOMENTS);
        if ((rc = launch_spw_stats(s, A, y_dev, standardize, xy, st, xy_std))) return rc;
    }
    WideArgs wd;
    wd.xs = nullptr; wd.ys = nullptr; wd.lay = WideLayout{0, 0, 0}; wd.n = n; wd.scratch = nullptr; wd.sparse = &A;
    PathExtras px;
    px.wide = &wd; px.lmax_xy_dev = standardize ? xy_std : nullptr;
    rc = run_paths(c, B, nullptr, xy, st, p, p, OEMGPU_SEM_BIG, standardize, 0, o, nullptr, beta, lambda_out, niter, loss, d, px);
    if (rc || !o->compute_loss) return rc;
    // oemSparse::get_loss with nobs <= nvars (ref src/oem_sparse.h:932-941): the residual of the RETURNED coefficients
    const size_t nfit = (size_t)o->npen * nl_of(o), nchunk = (size_t)((n + 2047) / 2048);
    Bump L;
    const size_t a_b = L.take(nfit * (size_t)(p + 1) * 8), a_p = L.take(nfit * nchunk * 8), a_l = L.take(nfit * 8);
    if (ctx_reserve(c, L.off + 4096)) return OEMGPU_ERR_HIP;          // (the paths are done: their frame may be overlaid)
    double *bd = (double *)(c->ws + a_b), *ld_ = (double *)(c->ws + a_l);
    OEM_HIP(hipMemcpyAsync(bd, beta, nfit * (size_t)(p + 1) * 8, hipMemcpyHostToDevice, s));
    if ((rc = launch_spw_loss(s, A, y_dev, bd, p + 1, (int)nfit, A.vec, (double *)(c->ws + a_p), ld_))) return rc;
    OEM_HIP(hipMemcpyAsync(loss, ld_, nfit * 8, hipMemcpyDeviceToHost, s));
    OEM_HIP(hipStreamSynchronize(s));
    for (size_t k = 0; k < nfit; ++k) if (niter[k] == 0) loss[k] = 1e99;
    return 0;
}

// ONE pass of the engine above after the fit's own setup (spw_setup), with the lanes of either orientation forced where not 0: what
// the tests hold every instantiation of sparse_wide.hip's kernels to (include/oemgpu.h)
int oemgpu_selftest_sparse_wide_pass(oemgpu_ctx *c, const oemgpu_sparse_x *x, int32_t pass, int32_t row_lanes, int32_t col_lanes,
                                     const int32_t *foldid_dev, int32_t nfolds, int32_t leave_out, int32_t standardize, double scale,
                                     const double *in_dev, const double *coef_dev, int32_t ncoef, double *out_dev, double *out2_dev,
                                     double *stats_dev, int64_t *info, int32_t *long_rows, int32_t *long_cols)
{
    static const char *who = "selftest_sparse_wide_pass";
    if (!c || !x || !in_dev || !out_dev || !info) { set_error("%s: NULL argument", who); return OEMGPU_ERR_ARG; }
    if (pass < OEMGPU_SPW_PASS_ROWS || pass > OEMGPU_SPW_PASS_LOSS) { set_error("%s: pass must be 0 (rows), 1 (columns), 2 (stats) or 3 (loss)", who); return OEMGPU_ERR_ARG; }
    if (pass == OEMGPU_SPW_PASS_STATS && (!out2_dev || !stats_dev)) { set_error("%s: NULL argument (the stats pass writes out2_dev and stats_dev)", who); return OEMGPU_ERR_ARG; }
    if (pass == OEMGPU_SPW_PASS_LOSS && (!coef_dev || ncoef < 1)) { set_error("%s: NULL argument or ncoef < 1 (the loss pass reads coef_dev)", who); return OEMGPU_ERR_ARG; }
    for (const int32_t L : {row_lanes, col_lanes})
        if (L != 0 && (L < 1 || L > 64 || (L & (L - 1)))) { set_error("%s: lanes must be 0 (the plan's) or one of 1, 2, 4, 8, 16, 32, 64", who); return OEMGPU_ERR_ARG; }
    int rc = spw_entry_checks(who, c, x, foldid_dev, nfolds, leave_out);
    if (rc) return rc;
    const int p = x->p, n = (int)x->n;
    if (set_device(c)) return OEMGPU_ERR_HIP;
    hipStream_t s = c->stream;
    int64_t nk = n, longest[2] = {0, 0};
    if ((rc = spw_kept_rows(c, who, foldid_dev, n, nfolds, leave_out, &nk))) return rc;
    SpwArgs A;
    if ((rc = spw_setup(c, x, foldid_dev, leave_out, nk, row_lanes, col_lanes, A, longest))) return rc;
    info[0] = A.plan.row_L; info[1] = A.plan.col_L; info[2] = A.n_long_rows; info[3] = A.n_long_cols; info[4] = longest[0]; info[5] = longest[1];
    info[6] = nk; info[7] = A.foldid ? 1 : 0;
    if (long_rows && A.n_long_rows > 0) OEM_HIP(hipMemcpyAsync(long_rows, A.long_row_list, sizeof(int32_t) * (size_t)A.n_long_rows, hipMemcpyDeviceToHost, s));
    if (long_cols && A.n_long_cols > 0) OEM_HIP(hipMemcpyAsync(long_cols, A.long_col_list, sizeof(int32_t) * (size_t)A.n_long_cols, hipMemcpyDeviceToHost, s));
    if (pass == OEMGPU_SPW_PASS_ROWS) rc = launch_spw_rows(s, A, in_dev, out_dev, scale, nullptr);
    else if (pass == OEMGPU_SPW_PASS_COLS) rc = launch_spw_cols(s, A, in_dev, out_dev, scale, nullptr);
    else if (pass == OEMGPU_SPW_PASS_STATS) rc = launch_spw_stats(s, A, in_dev, standardize, out_dev, stats_dev, out2_dev);
    else {
        const size_t nchunk = (size_t)((n + 2047) / 2048);
        if (ctx_reserve(c, (size_t)ncoef * nchunk * 8 + 4096)) return OEMGPU_ERR_HIP;
        rc = launch_spw_loss(s, A, in_dev, coef_dev, p + 1, ncoef, A.vec, (double *)c->ws, out_dev);
    }
    if (rc) return rc;
    OEM_HIP(hipGetLastError());
    OEM_HIP(hipStreamSynchronize(s));
    return 0;
}

int oemgpu_fit_sparse(int64_t n, int32_t p, const int64_t *colptr, const int32_t *rowidx, const double *values, const double *y,
                      int32_t standardize, int32_t intercept, const oemgpu_opts *o,
                      double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    if (!colptr || !y || !o || !beta || !lambda_out || !niter || !loss || !d) { set_error("fit_sparse: NULL argument"); return OEMGPU_ERR_ARG; }
    const int q = p + (intercept ? 1 : 0);
    int rc = check_opts(o, p, q);             // R prepends the unpenalised group 0 for the intercept slot (ref R/oem.R:296-338); oemSparse scans all groups.size() = q slots (ref src/oem_sparse.h:465)
    if (rc) return rc;
    if (n <= p && intercept) {
        set_error("a sparse x with p >= n and an intercept: the reference multiplies the n x p map by a vector of p + 1 entries (src/oem_sparse.h:638-647) -- "
                  "nothing well-formed to reproduce; intercept = FALSE is served");
        return OEMGPU_ERR_UNSUPPORTED;
    }
    // nobs <= nvars, sparse by sparse_wide_route's rule: from the non-zeros (sparse_wide.hip) -- the handle of oemgpu_sparse_x_create
    // built once, y uploaded, oemgpu_fit_sparse_wide_res, the handle freed; nothing of n p entries on either side
    const bool from_nnz = n >= 2 && n <= p && sparse_wide_route(n, p, colptr[p]);
    std::vector<int64_t> rowptr;
    const int64_t maxcol = csc_check("fit_sparse", n, p, colptr, rowidx, values, from_nnz ? &rowptr : nullptr);
    if (maxcol < 0) return (int)maxcol;
    if (from_nnz) {
        const int64_t nnz = colptr[p];
        for (int64_t i = 0; i < n; ++i) rowptr[(size_t)i + 1] += rowptr[(size_t)i];
        // the row copy on the host, every row's entries in column order (the columns are walked in order)
        std::vector<int32_t> ccol;
        std::vector<double> cval;
        std::vector<int64_t> cur;
        try { ccol.resize((size_t)nnz + 1); cval.resize((size_t)nnz + 1); cur.assign(rowptr.begin(), rowptr.end() - 1); }
        catch (const std::bad_alloc &) { set_error("sparse x with p >= n: no host memory for the row copy of %lld non-zeros", (long long)nnz); return OEMGPU_ERR_ARG; }
        for (int j = 0; j < p; ++j)
            for (int64_t k = colptr[j]; k < colptr[j + 1]; ++k) { const int64_t pos = cur[(size_t)rowidx[k]]++; ccol[(size_t)pos] = j; cval[(size_t)pos] = values[k]; }
        oemgpu_ctx *c = ctx_acquire(o->device);
        if (!c) return OEMGPU_ERR_NO_DEVICE;
        oemgpu_sparse_x *xh = nullptr;
        rc = sparse_x_build(c, n, p, colptr, rowidx, values, rowptr, maxcol, &xh, ccol.data(), cval.data());
        if (!rc && ctx_grow(c, &c->xres, &c->xres_bytes, sizeof(double) * (size_t)(n + 2))) rc = OEMGPU_ERR_HIP;
        if (!rc && hipMemcpyAsync(c->xres, y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
            set_error("fit_sparse: device staging failed"); rc = OEMGPU_ERR_HIP;
        }
        if (!rc) rc = oemgpu_fit_sparse_wide_res(c, xh, (const double *)c->xres, standardize, o, beta, lambda_out, niter, loss, d);
        (void)hipStreamSynchronize(c->stream);
        oemgpu_sparse_x_destroy(xh);
        ctx_release(c);
        return rc;
    }
    if (n <= p) {
        // nobs <= nvars: the XXt branch (ref src/oem_sparse.h:607-612, 638-647) is oemBig's, line for line
        std::vector<double> xc;                                         // n <= p rows: the dense copy the wide engine reads
        try { xc.assign((size_t)n * p, 0.0); }
        catch (const std::bad_alloc &) { set_error("sparse x with p >= n: no host memory for the dense %lld x %d copy", (long long)n, p); return OEMGPU_ERR_ARG; }
        for (int j = 0; j < p; ++j)
            for (int64_t k = colptr[j]; k < colptr[j + 1]; ++k) xc[(size_t)j * n + rowidx[k]] = values[k];
        return fit_big_wide_host(xc.data(), n, p, y, standardize, o, beta, lambda_out, niter, loss, d, o->compute_loss != 0);
    }
    const int64_t nnz = colptr[p];
    // intval = sqrt(mean(diag(XX)) / n) with XX the (standardised) Gram before the division by n (ref src/oem_sparse.h:493-508, 577-578)
    double intval = 1.0;
    {
        double xxdiag = 0.0;
        for (int j = 0; j < p; ++j) {
            double ss = 0.0;
            for (int64_t k = colptr[j]; k < colptr[j + 1]; ++k) ss += values[k] * values[k];
            double cs = ss / ((double)n - 1.0);
            if (cs == 0.0) cs = 1.0;
            xxdiag += standardize ? ss / cs : ss;
        }
        xxdiag /= (double)p;
        if (intercept) intval = std::sqrt(xxdiag / (double)n);
    }
    oemgpu_ctx *c = ctx_acquire(o->device);
    if (!c) return OEMGPU_ERR_NO_DEVICE;
    const SparseRoute R = sparse_route(n, p, nnz);
    double *xd = nullptr, *yd = nullptr, *vd = nullptr;
    int64_t *cd = nullptr;
    int32_t *rd = nullptr;
    void *cwork = nullptr;
    hipError_t e = hipSuccess;
    {                                                       // every staging buffer out of the context's grow-only input buffer
        Bump S;
        const size_t a_x = S.take(R.csc ? csc_moments_work_bytes(n, p) : sizeof(double) * (size_t)R.ld * p),
                     a_y = S.take(sizeof(double) * (size_t)(n + 2)),
                     a_c = S.take(sizeof(int64_t) * (size_t)(p + 1)), a_r = S.take(sizeof(int32_t) * (size_t)(nnz + 1)),
                     a_v = S.take(sizeof(double) * (size_t)(nnz + 1));
        if (ctx_grow(c, &c->xres, &c->xres_bytes, S.off)) { ctx_release(c); return OEMGPU_ERR_HIP; }
        xd = (double *)(c->xres + a_x); cwork = c->xres + a_x; yd = (double *)(c->xres + a_y); cd = (int64_t *)(c->xres + a_c);
        rd = (int32_t *)(c->xres + a_r); vd = (double *)(c->xres + a_v);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(yd, y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(cd, colptr, sizeof(int64_t) * (size_t)(p + 1), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && nnz > 0) e = hipMemcpyAsync(rd, rowidx, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && nnz > 0) e = hipMemcpyAsync(vd, values, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { set_error("fit_sparse: device staging failed: %s", hipGetErrorString(e)); rc = OEMGPU_ERR_HIP; }
    // The moment buffer by the route of sparse_route (sparse.hip): at the densities of the reference's examples (1 %) the compressed
    // columns; denser, the tiles of csc_tile_moments -- with one tile of a few hundred MB and a fraction of a millisecond there.
    if (!rc) {
        const GramPlan plmax = gram_plan_bound(R.rows, p, c->num_cu);
        Bump B;
        const size_t mlen = (size_t)oemgpu_moments_len(p);
        const size_t a_mom = B.take(mlen * 8), a_tmp = B.take(mlen * 8), a_t = B.take(plmax.tpart_doubles * 8), a_v = B.take(plmax.vpart_doubles * 8);
        const SparseSolveWs W = sparse_solve_ws(B, p, q, o);
        rc = ctx_reserve(c, W.need) ? OEMGPU_ERR_HIP : 0;
        double *mom = (double *)(c->ws + a_mom);
        if (!rc) rc = R.csc ? launch_csc_moments(c->stream, cd, rd, vd, yd, n, p, cwork, mom)
                            : csc_tile_moments(c, R, cd, rd, vd, nullptr, yd, n, p, maxcol, xd, (double *)(c->ws + a_t), (double *)(c->ws + a_v),
                                               (double *)(c->ws + a_tmp), mom);
        if (!rc) rc = sparse_solve(c, W, mom, p, q, standardize, intercept, o, intval, beta, lambda_out, niter, loss, d);
    }
    (void)hipStreamSynchronize(c->stream);
    ctx_release(c);
    return rc;
}

int oemgpu_xval_sparse_res(oemgpu_ctx *c, const oemgpu_sparse_x *x, const double *y_dev, const int32_t *foldid_dev, int32_t nfolds,
                           int32_t standardize, int32_t intercept, int32_t type_measure, const oemgpu_opts *o, double *beta,
                           double *lambda_out, int32_t *niter, double *loss, double *d, double *cvm, double *cvsd)
{
    if (!c || !x || !y_dev || !foldid_dev || !o || !beta || !lambda_out || !niter || !loss || !d || !cvm || !cvsd) {
        set_error("xval_sparse: NULL argument"); return OEMGPU_ERR_ARG;
    }
    if (o->ngpus > 1) { set_error("xval_sparse: the rows of a sparse x are not split over devices"); return OEMGPU_ERR_UNSUPPORTED; }
    if (c->device != x->device) { set_error("xval_sparse: the context and the sparse x are on different devices"); return OEMGPU_ERR_ARG; }
    return xval_sparse_impl(XVS_FULL, x->n, x->p, nullptr, nullptr, nullptr, y_dev, foldid_dev, nfolds, standardize, intercept, type_measure, o,
                            0, 0, nullptr, beta, lambda_out, niter, loss, d, cvm, cvsd, nullptr, nullptr, c, x);
}

// oemgpu_fit_sparse on a resident x: the same route, kernels and solve, nothing uploaded; intval from the moment buffer's diagonal
int oemgpu_fit_sparse_res(oemgpu_ctx *c, const oemgpu_sparse_x *x, const double *y_dev, int32_t standardize, int32_t intercept,
                          const oemgpu_opts *o, double *beta, double *lambda_out, int32_t *niter, double *loss, double *d)
{
    if (!c || !x || !y_dev || !o || !beta || !lambda_out || !niter || !loss || !d) { set_error("fit_sparse: NULL argument"); return OEMGPU_ERR_ARG; }
    const int64_t n = x->n, nnz = x->nnz;
    const int p = x->p, q = p + (intercept ? 1 : 0);
    int rc = check_opts(o, p, q);
    if (rc) return rc;
    if (n <= p && intercept) {
        set_error("a sparse x with p >= n and an intercept: the reference multiplies the n x p map by a vector of p + 1 entries (src/oem_sparse.h:638-647) -- "
                  "nothing well-formed to reproduce; intercept = FALSE is served");
        return OEMGPU_ERR_UNSUPPORTED;
    }
    if (c->device != x->device) { set_error("fit_sparse: the context and the sparse x are on different devices"); return OEMGPU_ERR_ARG; }
    if (n <= p) return oemgpu_fit_sparse_wide_res(c, x, y_dev, standardize, o, beta, lambda_out, niter, loss, d);
    if (set_device(c)) return OEMGPU_ERR_HIP;
    hipStream_t s = c->stream;
    const SparseRoute R = sparse_route(n, p, nnz);
    if (ctx_grow(c, &c->xres, &c->xres_bytes, R.csc ? csc_moments_work_bytes(n, p) : sizeof(double) * (size_t)R.ld * p)) return OEMGPU_ERR_HIP;
    const GramPlan plmax = gram_plan_bound(R.rows, p, c->num_cu);
    Bump B;
    const size_t mlen = (size_t)oemgpu_moments_len(p);
    const size_t a_mom = B.take(mlen * 8), a_tmp = B.take(mlen * 8), a_t = B.take(plmax.tpart_doubles * 8), a_v = B.take(plmax.vpart_doubles * 8),
                 a_diag = B.take(sizeof(double) * (size_t)p);
    const SparseSolveWs W = sparse_solve_ws(B, p, q, o);
    if (ctx_reserve(c, W.need)) return OEMGPU_ERR_HIP;
    double *mom = (double *)(c->ws + a_mom), *diag = (double *)(c->ws + a_diag);
    rc = R.csc ? launch_csc_moments(s, x->colptr, x->rowidx, x->val, y_dev, n, p, c->xres, mom)
               : csc_tile_moments(c, R, x->colptr, x->rowidx, x->val, nullptr, y_dev, n, p, x->maxcol, (double *)c->xres, (double *)(c->ws + a_t),
                                  (double *)(c->ws + a_v), (double *)(c->ws + a_tmp), mom);
    double intval = 1.0;
    if (!rc && intercept) {                                  // sqrt(mean(diag(XX)) / n), the expression of oemgpu_fit_sparse
        std::vector<double> hdiag((size_t)p);
        hipLaunchKernelGGL(moment_diag_kernel, dim3((p + 255) / 256), dim3(256), 0, s, mom, p, diag);
        OEM_HIP(hipGetLastError());
        OEM_HIP(hipMemcpyAsync(hdiag.data(), diag, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, s));
        OEM_HIP(hipStreamSynchronize(s));
        double xxdiag = 0.0;
        for (int j = 0; j < p; ++j) {
            const double ss = hdiag[j];
            double cs = ss / ((double)n - 1.0);
            if (cs == 0.0) cs = 1.0;
            xxdiag += standardize ? ss / cs : ss;
        }
        xxdiag /= (double)p;
        intval = std::sqrt(xxdiag / (double)n);
    }
    if (!rc) rc = sparse_solve(c, W, mom, p, q, standardize, intercept, o, intval, beta, lambda_out, niter, loss, d);
    (void)hipStreamSynchronize(s);
    return rc;
}

}  // extern "C"
#pragma GCC visibility pop
