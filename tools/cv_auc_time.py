"""Wall time of cv_oem(family="binomial", type_measure="auc") on one MI355X, and of the AUC entry alone.

    python tools/cv_auc_time.py [--n 1000000] [--p 100] [--nfolds 10] [--nlambda 100] [--reps 5] [--pkg DIR] [--json out.json]

The whole call is timed on seeded data with a seeded foldid: one warm-up, then --reps repeats (wall clock around the call, the device
synchronised on both sides).  --pkg DIR imports oem_amd from another checkout (built there), so the same script times the commit
before the device AUC -- whose AUC is a host argsort per fold and column on a host copy of predmat -- and this one, on the same box.

Where the package has the device entry (api.logistic_cv_auc), the arguments cv_oem hands it are kept and the entry is timed alone on
them, --reps times after a warm-up, between two HIP events (torch.cuda.Event on the stream the caller waits on; the entry is
synchronous, so the pair brackets its launches, its two small copies to the host and its waits).  Its algorithmic traffic is counted
from the data: per key 20 B of gather reads (prob, perm, y) and an 8 B write, 16 B for every sorting pass that is not skipped -- a
pass is skipped when the whole segment shares the digit, counted here on the host for the first, middle and last column of every fold --
and an 8 B read of the closing count.  Printed: that traffic over the measured time, beside the time of the same bytes at the HBM
rate (8 TB/s), for segments that take the workspace form; `lds` segments move the gather's bytes only."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=100)
    ap.add_argument("--nfolds", type=int, default=10)
    ap.add_argument("--nlambda", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pkg", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg) if a.pkg else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch

    import oem_amd
    from oem_amd import api
    rng = np.random.default_rng(11)
    x = rng.normal(size=(a.n, a.p))
    b = np.zeros(a.p)
    b[:5] = [0.8, -0.6, 0.4, 0.3, -0.2]
    y = (rng.uniform(size=a.n) < 1.0 / (1.0 + np.exp(-(x @ b + 0.2)))).astype(np.float64)
    fid = rng.permutation(np.resize(np.arange(1, a.nfolds + 1), a.n))
    xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda:0").t()       # (n, p) column-major
    del x
    kept = {}
    inner = getattr(api, "logistic_cv_auc", None)
    if inner is not None:
        def keeping(pm, yd, fd, nfolds, y_hi=None):
            kept.update(pm=pm, yd=yd, fd=fd, nfolds=nfolds, y_hi=y_hi)
            return inner(pm, yd, fd, nfolds, y_hi=y_hi)
        api.logistic_cv_auc = keeping

    def call():
        return oem_amd.cv_oem(xd, y, family="binomial", penalty="lasso", nlambda=a.nlambda, type_measure="auc", foldid=fid)

    times, res = [], None
    for rep in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    out = dict(n=a.n, p=a.p, nfolds=a.nfolds, nlambda=a.nlambda, device_auc=inner is not None, cv_s=times, cv_median_s=float(np.median(times)),
               cv_min_s=min(times), cv_spread_s=max(times) - min(times), cvm_head=[float(v) for v in res["cvm"][0][:3]],
               cvm_sum=float(np.sum(res["cvm"][0])), lambdas=len(res["cvm"][0]))
    if inner is not None:
        api.logistic_cv_auc = inner
        pm, yd, fd = kept["pm"], kept["yd"], kept["fd"]
        ncol, n = pm.shape
        ev, wall, first = [], [], None
        for rep in range(a.reps + 1):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            got = inner(pm, yd, fd, kept["nfolds"], y_hi=kept["y_hi"])
            e1.record()
            torch.cuda.synchronize()
            if rep:
                ev.append(e0.elapsed_time(e1) * 1e-3)
                wall.append(time.perf_counter() - t0)
            first = got if first is None else first
            assert all(np.array_equal(g, h) for g, h in zip(got, first))
        sizes = np.bincount(fid, minlength=a.nfolds + 1)[1:]
        P = api.cv_auc_plan(n, a.nfolds, ncol, torch.cuda.get_device_properties(0).multi_processor_count, int(sizes.max()))
        cols = sorted({0, ncol // 2, ncol - 1})
        host = pm[cols].cpu().numpy()
        passes = []
        for f in range(1, a.nfolds + 1):
            for v in host[:, fid == f]:
                k = np.where(np.isnan(v), np.uint64(0x7FF8000000000000), np.abs(v).view(np.uint64))
                passes.append(sum(int(len(np.unique((k >> np.uint64(8 * d)) & np.uint64(0x7F if d == 7 else 0xFF))) > 1) for d in range(8)))
        mean_passes = float(np.mean(passes))
        keys = float(n) * ncol
        hbm_keys = float(sizes[sizes > P["lmax"]].sum()) * ncol
        bytes_moved = keys * 20.0 + hbm_keys * (8.0 + 16.0 * mean_passes + 8.0)
        t = float(np.median(ev))
        out.update(auc_event_s=ev, auc_wall_s=wall, auc_median_s=t, auc_ncol=ncol, auc_form=P["form"], auc_cb=P["cb"], auc_batches=P["batches"],
                   auc_mean_passes=mean_passes, auc_bytes=bytes_moved, auc_bytes_per_s=bytes_moved / t, auc_time_at_8TBs=bytes_moved / 8e12)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
