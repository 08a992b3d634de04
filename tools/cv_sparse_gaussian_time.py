"""Wall time and device memory of cv_oem(family="gaussian") on a resident sparse x on one MI355X, against the only route there was for
this input before: the same matrix densified, as a device tensor.  One process, the two routes alternated.

    python tools/cv_sparse_gaussian_time.py [--n 250000] [--p 200] [--density 0.01] [--nfolds 10] [--nlambda 100] [--reps 5] [--json out.json]

  sparse  oem_amd.cv_oem(SparseX(x), yd, penalty="lasso", foldid=..., tol=1e-10): the columns into fold order, K fold moment buffers from
          one pass over the non-zeros, K + 1 oemSparse solves (oemgpu_cv_sparse_fold_fits_res), the scoring of the fold-ordered
          compressed rows (oemgpu_cv_sparse_score_res);
  dense   oem_amd.cv_oem(xd, yd, ...) with xd = x.toarray() on the device: DataStd's semantics, not oemSparse's -- the two routes
          answer different questions (centred columns against raw ones), so only time and memory are compared, never cvm.
Both see the same folds and options; the first run of each is a warm-up and every run ends in a synchronise.  Printed as one JSON line:
the median and the range of either route over the repeated runs, their ratio, the device bytes either route holds (the handle's
allocation as the library reports it and the call's buffer from the plan; the dense matrix and its fold-ordered copy, 8 n p and
8 ldp p by the layout rule of section 3.5), and the phases of one more sparse run: fold order, fold moments, compressed rows and the
K + 1 solves (HIP events on the call's stream: oemgpu_last_xval_sparse_timings), and the scoring call
(wall time, table upload included) without and with the prediction store of keep=True."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=250_000)
    ap.add_argument("--p", type=int, default=200)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--nfolds", type=int, default=10)
    ap.add_argument("--nlambda", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import numpy as np
    import scipy.sparse as sp
    import torch

    import oem_amd
    from oem_amd import _lib as B
    from oem_amd import api
    rng = np.random.default_rng(a.seed)
    x = sp.random(a.n, a.p, density=a.density, random_state=a.seed, format="csc", data_rvs=lambda k: rng.normal(size=k) * 3.0)
    b = np.concatenate([rng.uniform(size=a.p // 4), np.zeros(a.p - a.p // 4)])
    y = x @ b + rng.normal(size=a.n)
    fid = rng.permutation(np.resize(np.arange(1, a.nfolds + 1), a.n))
    sx = api.SparseX(x)
    xd = torch.as_tensor(np.ascontiguousarray(x.toarray().T), device="cuda:0").t()      # (n, p) column-major
    yd = torch.as_tensor(y, device="cuda:0")
    kw = dict(penalty="lasso", nlambda=a.nlambda, tol=1e-10, foldid=fid)

    def route(xx):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        oem_amd.cv_oem(xx, yd, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    times = {"sparse": [], "dense": []}
    for rep in range(a.reps + 1):                                                # run 0 warms both routes up
        for name, xx in (("sparse", sx), ("dense", xd)):
            dt = route(xx)
            if rep > 0:
                times[name].append(dt)

    # ---- the phases of one more sparse run
    lib, ctx = oem_amd.lib(), api.context(0)

    def wall(fn):
        torch.cuda.synchronize(); lib.oemgpu_synchronize(ctx)
        t0 = time.perf_counter()
        out = fn()
        lib.oemgpu_synchronize(ctx)
        return (time.perf_counter() - t0) * 1e3, out
    fits_ms, (fit0, outlist, dev) = wall(lambda: api._cv_gaussian_sparse_fold_fits(sx, yd, fid, a.nfolds, ["lasso"], (),
                                                                                    dict(nlambda=a.nlambda, tol=1e-10)))
    ph = api.xval_sparse_timings()
    lam = [np.asarray(fit0["lambda"][0])]
    which = [lam[0] >= max(np.min(o["lambda"][0]) for o in outlist)]
    score_ms, _ = wall(lambda: api._cv_gaussian_score(dev, outlist, lam, which, "mse", False))
    pm = torch.empty((1, len(lam[0]), a.n), dtype=torch.float64, device="cuda:0")      # keep = TRUE: the same call with the prediction store
    tri = np.zeros((a.nfolds, 1, len(lam[0]), 3))
    coef, ncol = api._cv_gaussian_table(outlist, lam, which, a.p)
    dp = C.POINTER(C.c_double)
    keep_ms, rc = wall(lambda: lib.oemgpu_cv_sparse_score_res(ctx, a.n, a.p, a.nfolds, coef.ctypes.data_as(dp), 1, len(lam[0]),
                                                              ncol.ctypes.data_as(C.POINTER(C.c_int32)), 0, tri.ctypes.data_as(dp), pm.data_ptr()))
    B.check(rc)
    del pm

    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    plan = api.cv_sparse_plan(a.n, a.p, sx.nnz, a.nfolds, 1, a.nlambda, num_cu)
    handle_bytes = sx.device_bytes                                               # the handle's one allocation, as the library sized it
    ldp = (a.n + 16 * a.nfolds + 15) // 16 * 16
    med = {name: float(np.median(t)) for name, t in times.items()}
    out = dict(n=a.n, p=a.p, nnz=sx.nnz, nfolds=a.nfolds, nlambda=a.nlambda, reps=a.reps, sparse_median_s=med["sparse"], dense_median_s=med["dense"],
               sparse_range_s=[min(times["sparse"]), max(times["sparse"])], dense_range_s=[min(times["dense"]), max(times["dense"])],
               dense_over_sparse=med["dense"] / med["sparse"], route="csc" if plan["csc"] else "tiles",
               sparse_device_bytes=dict(handle=handle_bytes, call=plan["bytes"]),
               dense_device_bytes=dict(x=8 * a.n * a.p, fold_ordered_copy=8 * ldp * a.p),
               phases_ms=dict(fold_order=ph["fold_order"], fold_moments=ph["fold_moments"], compressed_rows=ph["compressed_rows"],
                              solves=ph["fits"], fold_fits_call_wall=fits_ms, scoring=score_ms, scoring_with_prediction_store=keep_ms))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:                                             # one record: a second run replaces the first
            f.write(json.dumps(out) + "\n")
    sx.close()


if __name__ == "__main__":
    main()
