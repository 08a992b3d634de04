"""Wall time of cv_oem(family="binomial") on one MI355X against what the library could do before it had a fold entry, in one process,
alternating the two routes on the same resident x.

    python tools/logistic_cv_time.py [--n 1000000] [--p 100] [--nfolds 10] [--nlambda 100] [--reps 2] [--json out.json]

  cv     oem_amd.cv_oem(xd, y, family="binomial", penalty="lasso", foldid=...): K + 1 fits on the one x (the fold fits are masked row
         passes) and one scoring call on the device;
  loop   K + 1 calls of oem_fit_logistic_dense, the fold fits on torch-gathered device copies of the kept rows, then the held-out
         deviance in numpy from a host copy of x.
Both see the same folds and options and the first round of each is a warm-up.  Printed: the best wall time of either route, their
ratio (the masked pass reads the left-out rows too, so K / (K - 1) is its floor), the scoring call's share of cv, the largest
difference between the two routes' cvm, and the device memory either route needs beyond x and y (torch's peak, which holds foldid and
the gathered copy; the library's grow-only workspace is the same single-fit workspace in both and is reported as the drop in free
device memory over the first call)."""
import argparse
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
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
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
    xt = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda:0")           # (p, n) row-major = (n, p) column-major
    xd = xt.t()
    fd = torch.as_tensor(fid.astype(np.int64), device="cuda:0")
    kw = dict(penalty="lasso", nlambda=a.nlambda)
    score_s = [0.0]
    inner = api.logistic_cv_score

    def timed_score(*args, **kwargs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = inner(*args, **kwargs)
        score_s[0] += time.perf_counter() - t0
        return out
    api.logistic_cv_score = timed_score

    def route_cv():
        return oem_amd.cv_oem(xd, y, family="binomial", foldid=fid, **kw)["cvm"][0]

    def route_loop():
        fit0 = oem_amd.oem_fit_logistic_dense(xd, y, **kw)
        lam = np.asarray(fit0["lambda"][0])
        outlist = []
        for i in range(1, a.nfolds + 1):
            keep = torch.nonzero(fd != i).reshape(-1)
            xg = xt.index_select(1, keep).t()                                   # the gathered copy: n_eff x p, column-major
            outlist.append(oem_amd.oem_fit_logistic_dense(xg, y[fid != i], **kw))
            del xg
        ok = lam >= max(np.min(o["lambda"][0]) for o in outlist)
        dev = np.full((a.nfolds, len(lam)), np.nan)
        cnt = np.zeros(a.nfolds)
        for i, o in enumerate(outlist):
            rows = fid == i + 1
            pr = oem_amd.predict(o, x[rows], s=lam[ok], type="response")
            pm = np.clip(pr, 1e-5, 1 - 1e-5)
            y2 = y[rows][:, None]
            dev[i, :ok.sum()] = (-2 * (y2 * np.log(pm) + (1 - y2) * np.log(1 - pm))).mean(axis=0)
            cnt[i] = rows.sum()
        return (dev * cnt[:, None]).sum(axis=0) / cnt.sum()

    times = {"cv": [], "loop": []}
    mem = {}
    res = {}
    for rep in range(a.reps + 1):                                               # round 0 warms both routes up
        for name, fn in (("cv", route_cv), ("loop", route_loop)):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            free0 = torch.cuda.mem_get_info()[0]
            score_s[0] = 0.0
            t0 = time.perf_counter()
            res[name] = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep == 0:
                mem[name + "_torch_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
                mem[name + "_free_drop_bytes"] = int(free0 - torch.cuda.mem_get_info()[0])
            else:
                times[name].append(dt)
                if name == "cv":
                    times.setdefault("score", []).append(score_s[0])
    k = len(res["cv"])                                                         # cv_oem has trimmed the lambdas no fold reaches
    best = int(np.argmin(times["cv"]))
    out = dict(n=a.n, p=a.p, nfolds=a.nfolds, nlambda=a.nlambda, cv_s=min(times["cv"]), loop_s=min(times["loop"]), cv_all=times["cv"],
               loop_all=times["loop"], score_s=times["score"][best], **mem)
    out["ratio"] = out["cv_s"] / out["loop_s"]
    out["expected_at_most"] = a.nfolds / (a.nfolds - 1) * 1.05
    out["score_share"] = out["score_s"] / out["cv_s"]
    out["cvm_max_abs_diff"] = float(np.nanmax(np.abs(res["cv"][:k] - res["loop"][:k])))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
