"""Wall time of cv_oem(family="gaussian") on a device-resident x on one MI355X: the resident route against the host loop it replaces, in
one process, alternated on the same tensor.

    python tools/cv_gaussian_time.py [--n 1000000] [--p 100] [--nfolds 10] [--nlambda 100] [--reps 5] [--seed 11] [--json out.json]

  resident  oem_amd.cv_oem(xd, yd, penalty="lasso", foldid=..., tol=1e-10): the full fit, rows into fold order once, K solves from sums
            of fold moments (oemgpu_cv_fold_fits_dev), the scoring of the fold-ordered rows (oemgpu_cv_score_dev);
  host      the same call with the eligibility test switched off: x.cpu(), K gathers of the kept rows, K host-resident oem() calls,
            predictions and errors in numpy -- what cv_oem did with a device tensor before the resident route existed.
Both see the same folds and options; the first run of each is a warm-up and every run ends in a synchronise.  Printed as one JSON line:
the median and the range of either route over the repeated runs, their ratio, the largest relative difference between the two routes'
cvm, and the phases of one more resident run: the full fit, the fold order (the layout kernels and the gather, device time between
events: OEMGPU_T_FOLDORDER), the K fold moment passes (oemgpu_xval_fold_moments_dev on the same rows, wall time, less the fold order),
the K solves (the fold-fit call, wall time, less order and moments) and the scoring call (wall time, table upload included), without and
with the prediction store of keep=True (the n x nlambda matrix stays on the device in that figure)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=100)
    ap.add_argument("--nfolds", type=int, default=10)
    ap.add_argument("--nlambda", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import oem_amd
    from oem_amd import _lib as B
    from oem_amd import api
    rng = np.random.default_rng(a.seed)
    x = rng.normal(size=(a.n, a.p)) * 3.0
    b = np.concatenate([rng.uniform(size=a.p // 4), np.zeros(a.p - a.p // 4)])
    y = x @ b + rng.normal(size=a.n)
    fid = rng.permutation(np.resize(np.arange(1, a.nfolds + 1), a.n))
    xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda:0").t()         # (n, p) column-major
    yd = torch.as_tensor(y, device="cuda:0")
    del x
    kw = dict(penalty="lasso", nlambda=a.nlambda, tol=1e-10, foldid=fid)
    eligible = api._cv_gaussian_resident

    def route(resident):
        api._cv_gaussian_resident = eligible if resident else (lambda *args: False)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cvm = oem_amd.cv_oem(xd, yd, **kw)["cvm"][0]
            torch.cuda.synchronize()
            return time.perf_counter() - t0, cvm
        finally:
            api._cv_gaussian_resident = eligible

    times, res = {"resident": [], "host": []}, {}
    for rep in range(a.reps + 1):                                                # run 0 warms both routes up
        for name in ("resident", "host"):
            dt, res[name] = route(name == "resident")
            if rep > 0:
                times[name].append(dt)

    # ---- the phases of one more resident run
    lib, ctx = oem_amd.lib(), api.context(0)
    fd = torch.as_tensor(fid.astype(np.int32), device="cuda:0")

    def wall(fn):
        torch.cuda.synchronize(); lib.oemgpu_synchronize(ctx)
        t0 = time.perf_counter()
        out = fn()
        lib.oemgpu_synchronize(ctx)
        return (time.perf_counter() - t0) * 1e3, out
    fit_ms, fit0 = wall(lambda: oem_amd.oem(xd, yd, penalty="lasso", nlambda=a.nlambda, tol=1e-10))
    lib.oemgpu_set_timing(ctx, 1)
    fits_ms, (outlist, dev) = wall(lambda: api._cv_gaussian_fold_fits(xd, yd, fid, a.nfolds, ["lasso"], (), dict(nlambda=a.nlambda, tol=1e-10)))
    ms = (C.c_double * B.NTIMERS)()
    lib.oemgpu_last_timings(ctx, ms)
    order_ms = ms[5]                                                             # OEMGPU_T_FOLDORDER
    lib.oemgpu_set_timing(ctx, 0)
    lam = [np.asarray(fit0["lambda"][0])]
    which = [lam[0] >= max(np.min(o["lambda"][0]) for o in outlist)]
    score_ms, _ = wall(lambda: api._cv_gaussian_score(dev, outlist, lam, which, "mse", False))
    pm = torch.empty((1, len(lam[0]), a.n), dtype=torch.float64, device="cuda:0")      # keep = TRUE: the same call with the prediction store
    tri = np.zeros((a.nfolds, 1, len(lam[0]), 3))
    coef, ncol = api._cv_gaussian_table(outlist, lam, which, a.p)
    dp = C.POINTER(C.c_double)
    keep_ms, rc = wall(lambda: lib.oemgpu_cv_score_dev(ctx, a.n, a.p, a.nfolds, coef.ctypes.data_as(dp), 1, len(lam[0]),
                                                       ncol.ctypes.data_as(C.POINTER(C.c_int32)), 0, tri.ctypes.data_as(dp), pm.data_ptr()))
    B.check(rc)
    del pm
    mom = torch.empty(int(lib.oemgpu_xval_moments_len(a.p, a.nfolds, 0)), dtype=torch.float64, device="cuda:0")
    fn = (C.c_int64 * a.nfolds)()
    xp, n, p, ld, keepalive = api._device_matrix(xd)
    prep_ms, rc = wall(lambda: lib.oemgpu_xval_fold_moments_dev(ctx, xp, n, ld, p, yd.data_ptr(), None, fd.data_ptr(), a.nfolds,
                                                                C.byref(dev["args"].c), mom.data_ptr(), fn))
    B.check(rc)

    k = min(len(res["resident"]), len(res["host"]))
    med = {name: float(np.median(t)) for name, t in times.items()}
    out = dict(n=a.n, p=a.p, nfolds=a.nfolds, nlambda=a.nlambda, reps=a.reps, resident_median_s=med["resident"], host_median_s=med["host"],
               resident_range_s=[min(times["resident"]), max(times["resident"])], host_range_s=[min(times["host"]), max(times["host"])],
               host_over_resident=med["host"] / med["resident"],
               cvm_max_rel_diff=float(np.max(np.abs(res["resident"][:k] - res["host"][:k]) / np.abs(res["host"][:k]))),
               phases_ms=dict(full_fit=fit_ms, fold_order=order_ms, fold_moments=prep_ms - order_ms, solves=fits_ms - prep_ms, scoring=score_ms,
                              scoring_with_prediction_store=keep_ms))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
