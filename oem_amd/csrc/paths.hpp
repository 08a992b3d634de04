// paths.hpp -- what api.hip needs of the driver every Gaussian fit ends in (paths.hip: plan_paths / run_paths).
#pragma once

#include "ctx.hpp"

namespace oemgpu {

// sem of run_paths: OEMGPU_SEM_*, or 2 for oem.xtx.
enum { SEM_XTX = 2, SEM_SPARSE = 4 };        // OEMGPU_SEM_XVAL = 3 (oemgpu.h): oemBig's algebra with xval.oem's lambda_zero, groups and loss;
                                              // SEM_SPARSE: oemSparse (the intercept slot rescaled in place through `scale_factor`, groups = q entries, slot 0 the intercept's group 0)
inline int nl_of(const oemgpu_opts *o) { return (o->lambda_user && o->nlambda_user > 0) ? o->nlambda_user : o->nlambda; }

// What a caller of run_paths may set beyond the problem itself (every default: not used).
// nbatch > 1: that many independent problems (instance b at xx + b * bstride, ... ; outputs of instance b at beta + b * npen * nl *
// rows, lambda_out / niter / loss + b * npen * nl, d_out[b]) solved by ONE launch, one workgroup (set) each; q <= SMALL_P_MAX only.
// Weighted oemDense with nobs <= nvars (weighted.hip): d comes from one matrix, the iteration runs on another and the loss belongs to
// the first again -- d handed over (launch-per-iteration Gram engine only), the loss as a pass of its own over (loss_xx, loss_xy, loss_stats).
struct PathExtras {
    int nbatch = 1;
    size_t bstride = 0;
    bool shared_lmax = false;                // nbatch > 1: every lambda grid from instance 0's X'Y
    int lmax_group = 0;                      // ... with shared_lmax, 0 < lmax_group < nbatch: instance b's from instance (b / lmax_group) * lmax_group (PathArgs::lmax_group)
    const WideArgs *wide = nullptr;          // the p >= n iteration through the standardised X itself (no Gram matrix: xx is NULL)
    const double *lmax_xy_dev = nullptr;     // the lambda grid from the caller's vector (big.oem with p >= n: the scaled X'y)
    double d_fixed = 0.0;
    const double *loss_xx = nullptr, *loss_xy = nullptr, *loss_stats = nullptr;
    int32_t *shift_advised_out = nullptr;    // [nbatch] (host) <- what finalize advised for every instance (oemgpu_ctx::shift_advised keeps the last one's)
};

// xx (q x q), xy (q), stats already on the device (in the workspace, B the frame behind them).
int run_paths(oemgpu_ctx *c, Bump &B, const double *xx, const double *xy, const double *stats, int p, int q, int sem,
              int standardize, int intercept, const oemgpu_opts *o, const double *scale_factor,
              double *beta, double *lambda_out, int32_t *niter, double *loss, double *d_out, const PathExtras &x = PathExtras());
size_t paths_ws_bytes(int p, int q, const oemgpu_opts *o, int nbatch = 1);      // a bound on what run_paths carves behind B

// CU slots of the persistent engines: all workgroups of all such kernels in flight must be resident at once, so concurrent callers queue.
// Booked per device AND per XCD: a device-scope launch of `want` workgroups is dealt round the XCDs by the dispatcher
// (ceil(want / 8) CUs of each); a one-XCD launch (path_coop.hip, q <= 512) puts the W workgroups of instance y on XCD (base + y) mod 8
// and gets the base for which the fullest XCD it touches stays emptiest -- and waits while no base leaves every XCD within its CUs.
struct CoopSlots {
    int n = 0, dev = 0;
    int add[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    void take(int device, int want, int capacity);
    int take_local(int device, int W, int ninst, int num_cu, int capacity);      // `ninst` instances of W workgroups, each on ONE XCD; returns the XCD of instance 0
    void release();
    ~CoopSlots() { release(); }
};

}  // namespace oemgpu
#ifdef OEM_HOST_TIMING      // (a variant library, never the product: five stages of a fit, stamped in api.hip -- 0, 1, 5 -- and in run_paths)
#include <chrono>
namespace oemgpu { extern double g_tp[6]; }
#define HT(i) oemgpu::g_tp[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count()
#else
#define HT(i) do { } while (0)
#endif
