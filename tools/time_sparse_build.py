#!/usr/bin/env python3
"""Times the two ways from a torch sparse tensor that lies on the device to a resident oem_amd.SparseX:

    (a) host    the only way before SparseX took tensors: the tensor's components to the host, a scipy matrix of them, SparseX(scipy)
                (scipy's canonicalisation, csc_check on one host thread, the upload, the row copy by csc_to_csr_kernel);
    (b) device  SparseX(tensor): checked, copied and transposed where it lies (oem_amd/csrc/sparse_build.hip).

    python tools/time_sparse_build.py [--out profiles/sparse_build_time.json] [--shapes 250000x200x0.01,1000000x512x0.01,2000x200000x0.01]
                                      [--batches 5]

Every (shape, route) runs in a process of its own (this script again with --child): seeded data, a torch.sparse_csr_tensor of it on the
device (torch's default compressed layout; int64 indices, float64 values), one warm-up build during which a thread samples the
device's free memory (the peak of the call, over what the tensor itself holds), then `batches` timed batches of `calls` builds each:
a host clock around builds that end synchronised, every handle closed inside the clock.  Reported per (shape, route): the median batch
in ms per build with the spread of the batches, the peak of host memory over the data (ru_maxrss) and of device memory; for (b) also
the HIP-event times of the build's three phases (oemgpu_last_sparse_build_timings, the median over the timed builds) and the bytes the
sort passes must move, 36 bytes per non-zero per pass, over the passes' event time as a share of the HBM peak."""
import argparse
import ctypes as C
import json
import resource
import subprocess
import sys
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
HBM_PEAK = 8.0e12            # bytes / s, MI355X
DEFAULT_SHAPES = "250000x200x0.01,1000000x512x0.01,2000x200000x0.01"


def make_rows(n, p, dens, seed=7):
    """compressed rows with about dens n p normal entries: distinct, ascending columns in every row (stratified draws)"""
    rng = np.random.default_rng(seed)
    per_row = rng.binomial(p, dens, size=n).astype(np.int64)
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(per_row, out=ptr[1:])
    nnz = int(ptr[-1])
    row_of = np.repeat(np.arange(n, dtype=np.int64), per_row)
    pos = np.arange(nnz, dtype=np.int64) - ptr[row_of]
    c = per_row[row_of].astype(np.float64)
    lo = np.floor(pos * p / c); hi = np.maximum(np.floor((pos + 1) * p / c), lo + 1)
    cols = (lo + np.floor(rng.random(nnz) * (hi - lo))).astype(np.int64)
    return ptr, cols, rng.normal(size=nnz)


def child(a):
    import scipy.sparse as sp
    import torch
    import oem_amd
    n, p = a.n, a.p
    ptr, cols, vals = make_rows(n, p, a.dens)
    nnz = int(ptr[-1])
    t = torch.sparse_csr_tensor(torch.as_tensor(ptr, device="cuda"), torch.as_tensor(cols, device="cuda"), torch.as_tensor(vals, device="cuda"),
                                size=(n, p))
    del ptr, cols, vals
    torch.cuda.synchronize()
    L = oem_amd.lib()
    phases = []

    def build():
        if a.route == "host":
            m = sp.csr_matrix((t.values().cpu().numpy(), t.col_indices().cpu().numpy(), t.crow_indices().cpu().numpy()), shape=(n, p))
            sx = oem_amd.SparseX(m)
        else:
            sx = oem_amd.SparseX(t)
            ms = (C.c_double * 3)()
            L.oemgpu_last_sparse_build_timings(ms)
            phases.append(list(ms))
        assert sx.nnz == nnz
        sx.close()

    free0 = torch.cuda.mem_get_info()[0]
    low, stop = [free0], threading.Event()

    def sample():
        while not stop.is_set():
            f = torch.cuda.mem_get_info()[0]
            if f < low[0]:
                low[0] = f
            time.sleep(0.002)
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    th = threading.Thread(target=sample); th.start()
    t0 = time.perf_counter(); build(); warm = time.perf_counter() - t0
    stop.set(); th.join()
    rss1 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    calls = a.calls if a.calls > 0 else max(1, min(50, int(1.0 / max(warm, 1e-3))))
    del phases[:]
    batch_ms = []
    for _ in range(a.batches):
        t0 = time.perf_counter()
        for _ in range(calls):
            build()
        batch_ms.append((time.perf_counter() - t0) * 1e3 / calls)
    res = dict(n=n, p=p, density=a.dens, nnz=nnz, route=a.route, calls_per_batch=calls, warmup_ms=warm * 1e3, batch_ms_per_build=batch_ms,
               ms_per_build=float(np.median(batch_ms)), spread_ms=float(max(batch_ms) - min(batch_ms)),
               host_peak_bytes_over_data=int((rss1 - rss0) * 1024), device_peak_bytes_over_tensor=int(free0 - low[0]))
    if phases:
        out = (C.c_int64 * 8)()
        assert L.oemgpu_selftest_sparse_build_plan(n, p, nnz, 1, torch.cuda.get_device_properties(0).multi_processor_count, out) == 0
        med = np.median(np.array(phases), axis=0)
        sort_bytes = 36 * nnz * int(out[0])
        res.update(passes=int(out[0]), digit_bits=int(out[1]), workgroups=int(out[2]), check_ms=float(med[0]), sort_ms=float(med[1]),
                   pointers_ms=float(med[2]), sort_bytes=sort_bytes,
                   sort_share_of_hbm_peak=(sort_bytes / (med[1] * 1e-3) / HBM_PEAK) if med[1] > 0 else None)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--route", default=None)
    ap.add_argument("--n", type=int); ap.add_argument("--p", type=int); ap.add_argument("--dens", type=float)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--calls", type=int, default=0, help="builds per batch (0: about a second's worth, at most 50)")
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sparse_build_time.json"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds a (shape, route) process may take")
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = dict(method="median of %d batches; host clock around synchronised builds, the handle closed inside; one process per (shape, route); "
                      "phase times by HIP events" % a.batches, hbm_peak_bytes_per_s=HBM_PEAK, runs=[])
    rc = 0
    for n, p, dens in [tuple(s.split("x")) for s in a.shapes.split(",")]:
        for route in ("host", "device"):
            cmd = [sys.executable, __file__, "--child", "--route", route, "--n", n, "--p", p, "--dens", dens, "--batches", str(a.batches),
                   "--calls", str(a.calls)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                out["runs"].append(dict(route=route, n=int(n), p=int(p), density=float(dens), error="timed out after %d s" % a.timeout))
                print(f"{route} {n}x{p}: timed out", flush=True)
                return finish(a, out, 1)                            # (nothing more is started on the device after a run that did not end)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                out["runs"].append(dict(route=route, n=int(n), p=int(p), density=float(dens), error=(r.stderr or r.stdout)[-400:], rc=r.returncode))
                print(f"{route} {n}x{p}: rc={r.returncode} {(r.stderr or '')[-300:]}", flush=True)
                return finish(a, out, 1)
            res = json.loads(line[0][7:])
            out["runs"].append(res)
            extra = "" if route == "host" else (f", passes {res['passes']}, sort {res['sort_ms']:.3f} ms = {100 * (res['sort_share_of_hbm_peak'] or 0):.1f} % "
                                                f"of the HBM peak, check {res['check_ms']:.3f} ms, pointers {res['pointers_ms']:.3f} ms")
            print(f"{route} {n}x{p}@{dens}: {res['ms_per_build']:.2f} ms/build (spread {res['spread_ms']:.2f}), host {res['host_peak_bytes_over_data'] / 1e6:.0f} MB, "
                  f"device {res['device_peak_bytes_over_tensor'] / 1e6:.0f} MB{extra}", flush=True)
    return finish(a, out, rc)


def finish(a, out, rc):
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
