#!/usr/bin/env python3
"""Times oem() on a sparse x with p >= n (oemgpu_fit_sparse, lasso, 100 lambdas, tol 1e-7) on the route through the non-zeros
(oem_amd/csrc/sparse_wide.hip) and, given the library of the parent commit, on the dense-copy route it replaces.

    python tools/time_sparse_wide.py [--parent-lib /path/to/parent/liboemgpu.so] [--out profiles/sparse_wide_time.json]
                                     [--shapes 2000x200000x0.01,5000x50000x0.02,20000x1000000x0.001] [--batches 5]

Every (tree, shape) runs in a process of its own (this script again with --child): seeded data, one warm-up call during which a thread
samples the device's free memory (the peak of the call) -- then `batches` timed batches of `calls` calls each, a host clock around
calls that end synchronised.  Reported per (tree, shape): the median batch in ms per call with the spread of the five, that time over
the iterations the call made (all of the call -- handle, eigen step, copies -- not kernel time), the peak of host memory (ru_maxrss)
and of device memory, and for this commit the bytes the two passes of an iteration must move (12 bytes per non-zero per pass plus
their vectors and line pointers) over that time as a share of the HBM peak: a lower bound of the passes' own share, since the time
also holds the update kernel, the eigen step and the set-up.  Where both trees ran a shape, their coefficients are compared.
The C ABI is called through ctypes alone, so the same script drives a library that lacks this commit's symbols.
The last shape is this commit's only by default: the parent needs a 160 GB dense copy there."""
import argparse
import ctypes as C
import json
import os
import resource
import subprocess
import sys
import tempfile
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
HBM_PEAK = 8.0e12            # bytes / s, MI355X
DEFAULT_SHAPES = "2000x200000x0.01,5000x50000x0.02,20000x1000000x0.001"


def make_data(n, p, dens, seed=7):
    """compressed columns with about dens n p normal entries, y from six columns plus noise"""
    rng = np.random.default_rng(seed)
    per_col = rng.binomial(n, dens, size=p).astype(np.int64)
    colptr = np.zeros(p + 1, dtype=np.int64)
    np.cumsum(per_col, out=colptr[1:])
    nnz = int(colptr[-1])
    # distinct sorted rows per column: a random key per entry, ranked inside the column, spread over [0, n)
    col_of = np.repeat(np.arange(p, dtype=np.int64), per_col)
    rows = np.empty(nnz, dtype=np.int32)
    pos = np.arange(nnz, dtype=np.int64) - colptr[col_of]
    # stratified: entry k of a column with c entries falls in [k n / c, (k + 1) n / c): distinct and increasing
    c = per_col[col_of].astype(np.float64)
    lo = np.floor(pos * n / c); hi = np.maximum(np.floor((pos + 1) * n / c), lo + 1)
    rows[:] = (lo + np.floor(rng.random(nnz) * (hi - lo))).astype(np.int32)
    vals = rng.normal(size=nnz) * 1.5
    b = rng.uniform(1, 2, 6)
    y = 0.5 * rng.normal(size=n)
    for j, bj in zip(np.argsort(-per_col, kind="stable")[:6], b):
        k0, k1 = colptr[j], colptr[j + 1]
        y[rows[k0:k1]] += bj * vals[k0:k1]
    return colptr, rows, vals, y


def child(a):
    from oem_amd._lib import OemgpuOpts, _dp, _ip
    n, p, dens = a.n, a.p, a.dens
    colptr, rows, vals, y = make_data(n, p, dens)
    nnz = int(colptr[-1])
    if a.route is not None:
        os.environ["OEM_SPARSE_GRAM"] = a.route
    hip = C.CDLL("libamdhip64.so")
    lib = C.CDLL(a.lib)
    nl = 100
    pen = np.array([1], dtype=np.int32)                             # lasso
    pf = np.ones(p)
    o = OemgpuOpts()
    o.npen = 1; o.penalty = pen.ctypes.data_as(_ip); o.nlambda = nl; o.lambda_min_ratio = 0.01
    o.alpha, o.gamma, o.tau, o.tol = 1.0, 3.0, 0.5, 1e-7
    o.maxit = 500; o.penalty_factor = pf.ctypes.data_as(_dp); o.device = -1
    beta = np.zeros((nl, p + 1)); lam = np.zeros(nl); niter = np.zeros(nl, dtype=np.int32); loss = np.zeros(nl); d = C.c_double(0)
    lib.oemgpu_last_error.restype = C.c_char_p

    def call():
        rc = lib.oemgpu_fit_sparse(C.c_int64(n), C.c_int32(p), C.c_void_p(colptr.ctypes.data), C.c_void_p(rows.ctypes.data), C.c_void_p(vals.ctypes.data),
                                   C.c_void_p(y.ctypes.data), C.c_int32(1), C.c_int32(0), C.byref(o), beta.ctypes.data_as(_dp), lam.ctypes.data_as(_dp),
                                   niter.ctypes.data_as(_ip), loss.ctypes.data_as(_dp), C.byref(d))
        if rc != 0:
            raise RuntimeError(lib.oemgpu_last_error().decode())

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
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    th = threading.Thread(target=sample); th.start()
    t0 = time.perf_counter(); call(); warm = time.perf_counter() - t0
    stop.set(); th.join()
    rss1 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    calls = a.calls if a.calls > 0 else max(1, min(20, int(1.0 / max(warm, 1e-3))))
    batch_ms = []
    for _ in range(a.batches):
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        batch_ms.append((time.perf_counter() - t0) * 1e3 / calls)
    its = int(niter.sum())
    med = float(np.median(batch_ms))
    eng = C.c_int32(-1)
    if hasattr(lib, "oemgpu_last_host_path_engine"):
        lib.oemgpu_last_host_path_engine(C.byref(eng))
    res = dict(n=n, p=p, density=dens, nnz=nnz, lambdas=nl, tol=1e-7, iterations=its, engine=int(eng.value), calls_per_batch=calls,
               warmup_ms=warm * 1e3, batch_ms_per_call=batch_ms, ms_per_call=med, spread_ms=float(max(batch_ms) - min(batch_ms)),
               us_per_iteration_whole_call=med * 1e3 / max(its, 1), host_peak_bytes_over_data=int((rss1 - rss0) * 1024),
               host_peak_bytes=int(rss1 * 1024), device_peak_bytes=int(free0 - low[0]), d=float(d.value))
    if eng.value == 10:
        per_it = 2 * 12 * nnz + 8 * (p + n) * 2 + 8 * (n + 1) + 8 * (p + 1)   # both passes: values + indices, vector in and out, line pointers
        res["pass_bytes_per_iteration"] = int(per_it)
        res["pass_bytes_over_call_time_share_of_hbm_peak"] = per_it / (res["us_per_iteration_whole_call"] * 1e-6) / HBM_PEAK
    if a.dump:
        np.save(a.dump, beta)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=str(ROOT / "oem_amd" / "liboemgpu.so"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--route", default=None, help="child: OEM_SPARSE_GRAM for the run (wide | nowide)")
    ap.add_argument("--n", type=int); ap.add_argument("--p", type=int); ap.add_argument("--dens", type=float)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--calls", type=int, default=0, help="calls per batch (0: about a second's worth, at most 20)")
    ap.add_argument("--dump", default=None)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--parent-shapes", type=int, default=2, help="the first so many shapes also run on the parent library")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sparse_wide_time.json"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds a (tree, shape) process may take")
    a = ap.parse_args()
    if a.child:
        return child(a)
    shapes = [tuple(s.split("x")) for s in a.shapes.split(",")]
    out = dict(method="median of %d batches; host clock around synchronised calls; one process per (tree, shape)" % a.batches,
               hbm_peak_bytes_per_s=HBM_PEAK, runs=[])
    with tempfile.TemporaryDirectory() as tmp:
        for si, (n, p, dens) in enumerate(shapes):
            dumps = {}
            trees = [("this", a.lib)] + ([("parent", a.parent_lib)] if a.parent_lib and si < a.parent_shapes else [])
            for tree, lib in trees:
                dump = os.path.join(tmp, f"{tree}_{si}.npy")
                cmd = [sys.executable, __file__, "--child", "--lib", lib, "--n", n, "--p", p, "--dens", dens, "--batches", str(a.batches),
                       "--calls", str(a.calls), "--dump", dump]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                except subprocess.TimeoutExpired:
                    out["runs"].append(dict(tree=tree, n=int(n), p=int(p), density=float(dens), error="timed out after %d s" % a.timeout))
                    print(f"{tree} {n}x{p}: timed out", flush=True)
                    return finish(a, out, 1)                        # (nothing more is started on the device after a run that did not end)
                line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    out["runs"].append(dict(tree=tree, n=int(n), p=int(p), density=float(dens), error=(r.stderr or r.stdout)[-400:], rc=r.returncode))
                    print(f"{tree} {n}x{p}: rc={r.returncode} {(r.stderr or '')[-300:]}", flush=True)
                    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
                        return finish(a, out, 1)
                    continue
                res = json.loads(line[0][7:]); res["tree"] = tree
                out["runs"].append(res); dumps[tree] = dump
                print(f"{tree} {n}x{p}@{dens}: {res['ms_per_call']:.1f} ms/call (spread {res['spread_ms']:.1f}), {res['us_per_iteration_whole_call']:.1f} us/iteration, "
                      f"host {res['host_peak_bytes_over_data'] / 1e6:.0f} MB, device {res['device_peak_bytes'] / 1e6:.0f} MB, engine {res['engine']}", flush=True)
            if len(dumps) == 2:
                b0, b1 = np.load(dumps["this"]), np.load(dumps["parent"])
                out["runs"].append(dict(compare=f"{n}x{p}", max_abs_diff=float(np.abs(b0 - b1).max()), scale=float(np.abs(b1).max())))
                print(f"this vs parent {n}x{p}: max |diff| {np.abs(b0 - b1).max():.3e} of scale {np.abs(b1).max():.3e}", flush=True)
            for f in dumps.values():
                os.remove(f)
    return finish(a, out, 0)


def finish(a, out, rc):
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
