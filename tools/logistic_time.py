"""Per-stage times of the dense binomial fit (oem_amd.oem_fit_logistic_dense) on one MI355X.

    python tools/logistic_time.py [--n 1000000] [--p 100] [--nlambda 100] [--hessian upper.bound|full] [--penalty lasso ...]
                                  [--cpu] [--json out.json]

Prints the row pass, the Z + Gram + Lanczos and the inner-solve times (HIP events, oemgpu_set_timing), the IRLS steps and inner
iterations, the wall time of the call, and with --cpu the time of the one-core CPU restatement (tests/logistic_restatement.py, with
the BLAS limited to one thread) on the same problem.  For the row pass's bytes run it under `rocprofv3 --pmc FETCH_SIZE` in a run of
its own (counters only)."""
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
    ap.add_argument("--nlambda", type=int, default=100)
    ap.add_argument("--hessian", default="upper.bound")
    ap.add_argument("--penalty", nargs="+", default=["lasso"])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import ctypes as C

    import numpy as np
    import torch

    import oem_amd
    from oem_amd import api
    rng = np.random.default_rng(11)
    x = rng.normal(size=(a.n, a.p))
    b = np.zeros(a.p)
    b[:5] = [0.8, -0.6, 0.4, 0.3, -0.2]
    y = (rng.uniform(size=a.n) < 1.0 / (1.0 + np.exp(-(x @ b + 0.2)))).astype(np.float64)
    xd = torch.as_tensor(np.asfortranarray(x).T.copy(), device="cuda:0").t()
    yd = torch.as_tensor(y, device="cuda:0")
    groups = np.repeat(np.arange(1, a.p // 5 + 2), 5)[:a.p]
    ctx = api.context(0)
    oem_amd.lib().oemgpu_set_timing(ctx, 1)
    rows = []
    for rep in range(a.reps):                     # the first call warms up (code objects, workspace)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = oem_amd.oem_fit_logistic_dense(xd, yd, penalty=a.penalty, groups=groups, nlambda=a.nlambda, hessian_type=a.hessian,
                                             compute_loss=True)
        wall = time.perf_counter() - t0
        st = api.logistic_stats()
        st["wall_s"] = wall
        rows.append(st)
    st = rows[-1]
    out = dict(n=a.n, p=a.p, nlambda=a.nlambda, hessian=a.hessian, penalty=a.penalty, **st)
    out["inner_us_per_iter"] = 1e3 * st["inner_ms"] / max(1.0, st["inner_iters"])
    out["row_pass_us"] = 1e3 * st["rows_ms"] / max(1.0, st["row_passes"] - st["grams"])
    out["row_pass_TBps"] = 8.0 * a.n * a.p / (out["row_pass_us"] * 1e-6) / 1e12 if st["row_passes"] > st["grams"] else None
    if a.cpu:
        os.environ.setdefault("OMP_NUM_THREADS", "1")
        try:
            from threadpoolctl import threadpool_limits
        except ImportError:
            threadpool_limits = None
        from tests import logistic_restatement as R
        g = np.concatenate([[0], groups])
        t0 = time.perf_counter()
        if threadpool_limits is not None:
            with threadpool_limits(1):
                ref = R.fit(x, y, penalty=a.penalty, groups=g, unique_groups=np.unique(g), nlambda=a.nlambda,
                            hessian_full=a.hessian == "full", compute_loss=True)
        else:
            ref = R.fit(x, y, penalty=a.penalty, groups=g, unique_groups=np.unique(g), nlambda=a.nlambda,
                        hessian_full=a.hessian == "full", compute_loss=True)
        out["cpu_restatement_s"] = time.perf_counter() - t0
        out["max_abs_beta_diff"] = float(max(np.abs(np.asarray(fit["beta"][k]) - ref["beta"][k]).max() for k in range(len(a.penalty))))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
