"""Call times of the sparse binomial fit (oem_amd.oem_fit_logistic_sparse) on one MI355X.

    python tools/logistic_sparse_time.py [--shape manpage|big|tile] [--reps 2] [--cpu] [--ab K] [--json out.json]

Shapes: "manpage" is the sparse example of R/oem.R:141-158 (2e4 x 50 at 1 %, grp.lasso, 10 lambdas, no intercept, irls.tol 1e-3,
tol 1e-8); "big" is 1e6 x 1000 at 0.5 %, lasso, 100 lambdas, default settings (the compressed-column route); "tile" is 2e5 x 200 at
5 %, the same settings (the row-tile route).  Prints the host-clock time of the synchronous call (the first call warms up), the
IRLS steps, row passes, Hessian builds and inner iterations, and with --cpu the time of the CPU restatement
(tests/logistic_sparse_restatement.py, BLAS on one thread) on the same problem.  --ab K alternates K times the Gaussian sparse fit
(oem(), whose compressed-column route runs the unweighted csc_gram_kernel) and the binomial fit on the same matrix, so that one
`rocprofv3 --kernel-trace --stats` run of this tool gives both Gram kernels' times side by side; the per-kernel split of an IRLS step
(row pass, column pass, Gram, Lanczos, inner loop) comes from that kernel trace, not from this script."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    "manpage": dict(n=20000, p=50, density=0.01, penalty=["grp.lasso"], nlambda=10, intercept=False, irls_tol=1e-3, tol=1e-8),
    "big": dict(n=1_000_000, p=1000, density=0.005, penalty=["lasso"], nlambda=100, intercept=True, irls_tol=1e-3, tol=1e-7),
    "tile": dict(n=200_000, p=200, density=0.05, penalty=["lasso"], nlambda=100, intercept=True, irls_tol=1e-3, tol=1e-7),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="manpage", choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--ab", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import numpy as np
    import scipy.sparse as sp

    import oem_amd
    cfg = SHAPES[a.shape]
    n, p = cfg["n"], cfg["p"]
    rng = np.random.default_rng(11)
    x = sp.random(n, p, density=cfg["density"], format="csc", random_state=rng, data_rvs=lambda m: rng.normal(size=m))
    b = np.zeros(p)
    b[:5] = [0.8, -0.6, 0.4, 0.3, -0.2]
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-(x @ b + 0.2)))).astype(np.float64)
    groups = np.repeat(np.arange(1, p // 10 + 2), 10)[:p]
    kw = dict(penalty=cfg["penalty"], nlambda=cfg["nlambda"], intercept=cfg["intercept"], irls_tol=cfg["irls_tol"], tol=cfg["tol"],
              groups=groups if any("grp" in q for q in cfg["penalty"]) else ())
    walls = []
    for rep in range(a.reps):                     # the first call warms up (code objects, workspace)
        t0 = time.perf_counter()
        fit = oem_amd.oem_fit_logistic_sparse(x, y, **kw)
        walls.append(time.perf_counter() - t0)
    st = oem_amd.logistic_stats()
    out = dict(shape=a.shape, n=n, p=p, nnz=int(x.nnz), nlambda=cfg["nlambda"], penalty=cfg["penalty"], call_s=walls[-1],
               call_s_all=walls, irls_steps=st["irls_steps"], row_passes=st["row_passes"], grams=st["grams"], inner_iters=st["inner_iters"])
    out["ms_per_irls_step"] = 1e3 * walls[-1] / max(1.0, st["irls_steps"])
    for _ in range(a.ab):                         # unweighted (Gaussian, compressed columns) and weighted Gram on one matrix, alternating
        oem_amd.oem(x, y, penalty="lasso", nlambda=2, intercept=False, standardize=False)
        oem_amd.oem_fit_logistic_sparse(x, y, penalty="lasso", nlambda=1, irls_maxit=2, intercept=False, standardize=False)
    if a.cpu:
        os.environ.setdefault("OMP_NUM_THREADS", "1")
        try:
            from threadpoolctl import threadpool_limits
        except ImportError:
            threadpool_limits = None
        from tests import logistic_sparse_restatement as RS
        g = groups if any("grp" in q for q in cfg["penalty"]) else None
        if g is not None and cfg["intercept"]:
            g = np.concatenate([[0], g])
        rkw = dict(penalty=cfg["penalty"], nlambda=cfg["nlambda"], intercept=cfg["intercept"], irls_tol=cfg["irls_tol"], tol=cfg["tol"],
                   groups=g, unique_groups=None if g is None else np.unique(g))
        t0 = time.perf_counter()
        if threadpool_limits is not None:
            with threadpool_limits(1):
                ref = RS.fit(x, y, **rkw)
        else:
            ref = RS.fit(x, y, **rkw)
        out["cpu_restatement_s"] = time.perf_counter() - t0
        out["max_abs_beta_diff"] = float(max(np.abs(np.asarray(fit["beta"][k]) - ref["beta"][k]).max() for k in range(len(cfg["penalty"]))))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
