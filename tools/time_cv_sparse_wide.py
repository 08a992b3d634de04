#!/usr/bin/env python3
"""Times cv.oem on a sparse x with n <= p (10 folds, lasso, 100 lambdas, tol 1e-7, no intercept):

  this commit   cv_oem(SparseX(x), y, intercept=False) -- the full fit and the K fold fits as masked passes over the resident
                non-zeros (oemgpu_fit_sparse_wide_fold_res), the scoring from the handle's compressed rows
                (oemgpu_cv_sparse_wide_score_res); the handle is made inside every timed call, as a user's first call would;
  the parent    the only thing it can do: K + 1 calls of oem() on sliced scipy matrices (each rebuilds the compressed-row copy on
                the host and uploads 24 bytes per non-zero again), the held-out rows scored in numpy.

    python tools/time_cv_sparse_wide.py [--parent-tree /path/to/a/checkout/of/the/parent] [--out profiles/cv_sparse_wide_time.json]
                                        [--shapes 2000x200000x0.01,5000x50000x0.02] [--batches 5]

Every (tree, shape) runs in a process of its own (this script again with --child, the tree's own oem_amd first on sys.path): seeded
data, one warm-up call during which a thread samples the device's free memory (the peak of the call), then `batches` timed batches of
`calls` calls each, a host clock around calls that end synchronised.  Reported per (tree, shape): the median batch in ms per call
with the spread of the five, the peak of host memory (ru_maxrss) and of device memory, and the bytes the handle saves as arithmetic:
24 nnz K of upload, 1 / K of every row pass.  Where both trees ran a shape, their cvm and lambda.min are compared.  Without
--parent-tree only this commit is timed (and the sliced loop on this commit's library, as `loop`, for a same-library comparison)."""
import argparse
import ctypes as C
import json
import resource
import subprocess
import sys
import threading
import time
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
DEFAULT_SHAPES = "2000x200000x0.01,5000x50000x0.02"
NFOLDS, NLAMBDA, TOL = 10, 100, 1e-7


def make_data(n, p, dens, seed=7):
    """a CSC matrix of about dens n p normal entries, y from six well-filled columns plus noise, fold ids 1..NFOLDS"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    per_col = rng.binomial(n, dens, size=p).astype(np.int64)
    colptr = np.zeros(p + 1, dtype=np.int64)
    np.cumsum(per_col, out=colptr[1:])
    nnz = int(colptr[-1])
    col_of = np.repeat(np.arange(p, dtype=np.int64), per_col)
    pos = np.arange(nnz, dtype=np.int64) - colptr[col_of]
    c = per_col[col_of].astype(np.float64)                          # stratified rows: distinct and increasing inside a column
    lo = np.floor(pos * n / c); hi = np.maximum(np.floor((pos + 1) * n / c), lo + 1)
    rows = (lo + np.floor(rng.random(nnz) * (hi - lo))).astype(np.int32)
    vals = rng.normal(size=nnz) * 1.5
    x = sp.csc_matrix((vals, rows, colptr), shape=(n, p))
    b = np.zeros(p); b[np.argsort(-per_col, kind="stable")[:6]] = rng.uniform(1, 2, 6)
    y = x @ b + 0.5 * rng.normal(size=n)
    fid = rng.permutation(np.resize(np.arange(1, NFOLDS + 1), n))
    return x, y, fid


def cv_on_the_handle(oa, x, y, fid):
    with oa.SparseX(x) as sx:
        f = oa.cv_oem(sx, y, intercept=False, penalty="lasso", foldid=fid, nlambda=NLAMBDA, tol=TOL)
    return np.asarray(f["cvm"][0]), float(f["lambda.min"])


def cv_by_the_sliced_loop(oa, x, y, fid):
    """K + 1 calls of oem() on sliced scipy matrices, predict's interpolation, the errors and cvcompute's fold means in numpy"""
    kw = dict(intercept=False, penalty="lasso", nlambda=NLAMBDA, tol=TOL)
    xr = x.tocsr()
    fit0 = oa.oem(x, y, **kw)
    outs = [oa.oem(xr[fid != k].tocsc(), y[fid != k], **kw) for k in range(1, NFOLDS + 1)]
    lam = np.asarray(fit0["lambda"][0])
    which = lam >= max(np.min(o["lambda"][0]) for o in outs)
    means = np.full((NFOLDS, int(which.sum())), np.nan)
    for k in range(1, NFOLDS + 1):
        rows = fid == k
        pred = np.asarray(oa.predict(outs[k - 1], xr[rows], s=lam[which], which_model=0))
        means[k - 1] = ((y[rows][:, None] - pred) ** 2).mean(axis=0)
    w = np.bincount(fid, minlength=NFOLDS + 1)[1:].astype(np.float64)
    cvm = (means * w[:, None]).sum(axis=0) / w.sum()
    return cvm, float(lam[which][np.argmin(cvm)])


def child(a):
    sys.path.insert(0, a.tree)
    import oem_amd as oa
    assert Path(oa.__file__).resolve().parent.parent == Path(a.tree).resolve(), oa.__file__
    oa.lib()
    x, y, fid = make_data(a.n, a.p, a.dens)
    run = cv_on_the_handle if a.mode == "handle" else cv_by_the_sliced_loop
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0      # (no device: this fails, nothing is timed)
    free0, low = free.value, [free.value]
    stop = threading.Event()

    def sample():
        f, t = C.c_size_t(0), C.c_size_t(0)
        while not stop.is_set():
            if hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0 and f.value < low[0]:
                low[0] = f.value
            time.sleep(0.002)
    warnings.simplefilter("ignore")
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    th = threading.Thread(target=sample); th.start()
    t0 = time.perf_counter(); cvm, lam_min = run(oa, x, y, fid); warm = time.perf_counter() - t0
    stop.set(); th.join()
    rss1 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    calls = a.calls if a.calls > 0 else max(1, min(20, int(1.0 / max(warm, 1e-3))))
    batch_ms = []
    for _ in range(a.batches):
        t0 = time.perf_counter()
        for _ in range(calls):
            run(oa, x, y, fid)
        batch_ms.append((time.perf_counter() - t0) * 1e3 / calls)
        print(f"  {a.mode} {a.n}x{a.p}: batch {len(batch_ms)} of {a.batches}, {batch_ms[-1]:.0f} ms per call", file=sys.stderr, flush=True)
    nnz = int(x.nnz)
    res = dict(mode=a.mode, n=a.n, p=a.p, density=a.dens, nnz=nnz, folds=NFOLDS, lambdas=NLAMBDA, tol=TOL, calls_per_batch=calls,
               warmup_ms=warm * 1e3, batch_ms_per_call=batch_ms, ms_per_call=float(np.median(batch_ms)),
               spread_ms=float(max(batch_ms) - min(batch_ms)), host_peak_bytes_over_data=int((rss1 - rss0) * 1024),
               host_peak_bytes=int(rss1 * 1024), device_peak_bytes=int(free0 - low[0]), lambda_min=lam_min, cvm=[float(v) for v in cvm],
               upload_bytes_saved_by_the_handle=24 * nnz * NFOLDS, row_pass_share_saved=1.0 / NFOLDS)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=str(ROOT))
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--mode", default="handle", choices=["handle", "loop"])
    ap.add_argument("--n", type=int); ap.add_argument("--p", type=int); ap.add_argument("--dens", type=float)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--calls", type=int, default=0, help="calls per batch (0: about a second's worth, at most 20)")
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cv_sparse_wide_time.json"))
    ap.add_argument("--timeout", type=int, default=900, help="seconds a (tree, shape) process may take (six cv runs; the first shape needs minutes)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = dict(method="median of %d batches; host clock around synchronised calls; one process per (tree, shape)" % a.batches, runs=[])
    trees = [("this", str(ROOT), "handle"), ("parent", a.parent_tree, "loop") if a.parent_tree else ("this-loop", str(ROOT), "loop")]
    for shape in a.shapes.split(","):
        n, p, dens = shape.split("x")
        got = {}
        for tree, path, mode in trees:
            cmd = [sys.executable, __file__, "--child", "--tree", path, "--mode", mode, "--n", n, "--p", p, "--dens", dens,
                   "--batches", str(a.batches), "--calls", str(a.calls)]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)    # (stderr passes through: a line per batch)
            except subprocess.TimeoutExpired:
                out["runs"].append(dict(tree=tree, n=int(n), p=int(p), density=float(dens), error="timed out after %d s" % a.timeout))
                print(f"{tree} {n}x{p}: timed out", flush=True)
                return finish(a, out, 1)                            # (nothing more is started on the device after a run that did not end)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                out["runs"].append(dict(tree=tree, n=int(n), p=int(p), density=float(dens), error=r.stdout[-400:], rc=r.returncode))
                print(f"{tree} {n}x{p}: rc={r.returncode} {r.stdout[-300:]}", flush=True)
                if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
                    return finish(a, out, 1)
                continue
            res = json.loads(line[0][7:]); res["tree"] = tree
            out["runs"].append(res); got[tree] = res
            print(f"{tree} {n}x{p}@{dens}: {res['ms_per_call']:.1f} ms/cv (spread {res['spread_ms']:.1f}), host {res['host_peak_bytes_over_data'] / 1e6:.0f} MB, "
                  f"device {res['device_peak_bytes'] / 1e6:.0f} MB", flush=True)
        if len(got) == 2:
            (ta, ra), (tb, rb) = got.items()
            m = min(len(ra["cvm"]), len(rb["cvm"]))
            gap = float(np.max(np.abs(np.array(ra["cvm"][:m]) - np.array(rb["cvm"][:m])) / np.array(rb["cvm"][:m])))
            out["runs"].append(dict(compare=f"{n}x{p}", trees=[ta, tb], cvm_max_rel_diff=gap, lambda_min=[ra["lambda_min"], rb["lambda_min"]]))
            print(f"{ta} vs {tb} {n}x{p}: cvm max rel diff {gap:.2e}, lambda.min {ra['lambda_min']:.6g} / {rb['lambda_min']:.6g}", flush=True)
    return finish(a, out, 0)


def finish(a, out, rc):
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
