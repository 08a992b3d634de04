"""Wall time of cv_oem(family="binomial") on a scipy.sparse x on one MI355X against what the library could do before it had a resident
sparse x, in one process, alternating the two routes.

    python tools/logistic_sparse_cv_time.py [--shape big|tile] [--nfolds 10] [--nlambda 100] [--reps 2] [--json out.json]

Shapes (those of tools/logistic_sparse_time.py): "big" is 1e6 x 1000 at 0.5 % (the compressed-column Gram route), "tile" 2e5 x 200 at
5 % (the row-tile route); lasso, K random folds, default settings.
  cv     oem_amd.cv_oem(x, y, family="binomial", penalty="lasso", foldid=...): one SparseX (one upload, one compressed-row build), the
         full fit and the K fold fits as masked passes over it, one scoring call on the device;
  loop   K + 1 calls of oem_fit_logistic_sparse, the fold fits on host-sliced matrices (rows of a csr copy made once, outside the
         clock), each of which uploads its arrays and builds its row copy again; then the held-out deviance in numpy.
Both see the same folds and options and the first round of each is a warm-up.  Printed: the best wall time of either route, their
ratio with the bound one expects (the masked passes touch K / (K - 1) of the rows a sliced fit does; the loop pays K more uploads and
row-copy builds and the host slicing), the scoring call's share of cv, the largest difference between the two routes' cvm, the handle's
bytes, and the device memory either route takes beyond them: torch's peak (y, foldid, a mask) and the drop in free device memory over
the first call (the library's grow-only workspace; in cv it contains the handle while the call runs)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"big": dict(n=1_000_000, p=1000, density=0.005), "tile": dict(n=200_000, p=200, density=0.05)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="tile", choices=sorted(SHAPES))
    ap.add_argument("--nfolds", type=int, default=10)
    ap.add_argument("--nlambda", type=int, default=100)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import numpy as np
    import scipy.sparse as sp
    import torch

    import oem_amd
    from oem_amd import api
    cfg = SHAPES[a.shape]
    n, p = cfg["n"], cfg["p"]
    rng = np.random.default_rng(11)
    x = sp.random(n, p, density=cfg["density"], format="csc", random_state=rng, data_rvs=lambda m: rng.normal(size=m))
    b = np.zeros(p)
    b[:5] = [0.8, -0.6, 0.4, 0.3, -0.2]
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-(x @ b + 0.2)))).astype(np.float64)
    fid = rng.permutation(np.resize(np.arange(1, a.nfolds + 1), n))
    xr = x.tocsr()                                                              # for the loop's row slices
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
        return oem_amd.cv_oem(x, y, family="binomial", foldid=fid, **kw)["cvm"][0]

    def route_loop():
        fit0 = oem_amd.oem_fit_logistic_sparse(x, y, **kw)
        lam = np.asarray(fit0["lambda"][0])
        outlist = []
        for i in range(1, a.nfolds + 1):
            keep = fid != i
            outlist.append(oem_amd.oem_fit_logistic_sparse(xr[keep], y[keep], **kw))
        ok = lam >= max(np.min(o["lambda"][0]) for o in outlist)
        dev = np.full((a.nfolds, len(lam)), np.nan)
        cnt = np.zeros(a.nfolds)
        for i, o in enumerate(outlist):
            rows = fid == i + 1
            pr = oem_amd.predict(o, xr[rows], s=lam[ok], type="response")
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
    nnz = int(x.nnz)
    out = dict(shape=a.shape, n=n, p=p, nnz=nnz, nfolds=a.nfolds, nlambda=a.nlambda, cv_s=min(times["cv"]), loop_s=min(times["loop"]),
               cv_all=times["cv"], loop_all=times["loop"], score_s=times["score"][best],
               handle_bytes=24 * (nnz + 1) + 8 * (n + 1) + 8 * (p + 1) + 4 * (-(-n // 8192) + 1) * p, **mem)
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
