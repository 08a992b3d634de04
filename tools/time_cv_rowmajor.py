#!/usr/bin/env python3
"""Times cv_oem (10 folds, 100 lambdas, lasso) and xval_oem on the same data handed over as a row-major float64 tensor, a row-major
float32 tensor and a column-major float64 tensor, on this tree and on a checkout of the parent commit, each tree x shape x layout in a
child process of its own, one after the other on one device.

    python tools/time_cv_rowmajor.py --parent-root DIR [--out profiles/cv_rowmajor_time.json] [--shapes 1000000x100,1000000x512]

--parent-root: a checkout of the parent commit with its library built (python -m oem_amd.build there).  Without it only this tree is
timed.  The data is that of tools/time_rowmajor.py (float32-representable, generated on the device from one seed), so both trees see
the same tensors.

Per call kind a child makes two untimed calls, then B batches of k calls back to back (both front ends return host arrays, so a call
ends synchronised); ms per call is the median batch, `spread` is (slowest - fastest batch) / median: the run-to-run spread a
difference between two rows has to exceed to mean anything.  Besides the time a child reports the peak of torch's allocated bytes
across one call (the float64 and transposed copies show there; the library's own buffers, the fold-ordered copy among them, do not)
and the HIP-event time of the fold-order phase of the last call -- the fold layout plus the gather of the rows into fold order, which
is gather_rows_kernel on a column-major tensor (and on every tensor of the parent tree, behind torch's copies) and
fold_gather_rm_kernel on a row-major one."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SHAPES = [(1_000_000, 100), (1_000_000, 512)]
LAYOUTS = ["rm64", "rm32", "cm64"]
FAULTS = (134, 139, 124, 137)
T_FOLDORDER = 5                          # include/oemgpu.h: OEMGPU_T_FOLDORDER
NFOLDS, NLAMBDA, BATCHES = 10, 100, 5


def child(a):
    sys.path.insert(0, str(Path(a.package_root).resolve()))
    sys.path.insert(1, str(ROOT / "tools"))
    import ctypes as C
    import numpy as np
    import torch
    import oem_amd
    from oem_amd import api
    from oem_amd import _lib as L
    from time_rowmajor import make_data
    assert Path(oem_amd.__file__).resolve().parent.parent == Path(a.package_root).resolve()
    n, p = a.n, a.p
    x, y = make_data(torch, n, p, a.layout)
    fid = np.random.default_rng(20240501).permutation(np.resize(np.arange(1, NFOLDS + 1), n))
    calls = {"cv_oem": lambda: oem_amd.cv_oem(x, y, penalty="lasso", foldid=fid, nlambda=NLAMBDA),
             "xval_oem": lambda: oem_amd.xval_oem(x, y, penalty="lasso", foldid=fid, nlambda=NLAMBDA)}
    ctx = api.context()
    lib = L.lib()
    for name, call in calls.items():
        call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = call()
        est = time.perf_counter() - t0
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.max_memory_allocated()
        call()
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base
        k = max(3, min(20, int(1.0 / max(est, 1e-3))))
        batches = []
        for _ in range(BATCHES):
            t0 = time.perf_counter()
            for _ in range(k):
                call()
            batches.append(1e3 * (time.perf_counter() - t0) / k)
        lib.oemgpu_set_timing(ctx, 1)
        call()
        tm = (C.c_double * 16)()
        lib.oemgpu_last_timings(ctx, tm)
        lib.oemgpu_set_timing(ctx, 0)
        med = statistics.median(batches)
        print(json.dumps({"tree": a.label, "call": name, "n": n, "p": p, "layout": a.layout, "ms_per_call": med,
                          "batches_ms": batches, "calls_per_batch": k, "spread": (max(batches) - min(batches)) / med,
                          "peak_extra_bytes": int(extra), "x_bytes": int(x.numel() * x.element_size()), "np4_bytes": 4 * n * p,
                          "foldorder_ms": tm[T_FOLDORDER], "lambda_min": float(fit["lambda.min"])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--n", type=int); ap.add_argument("--p", type=int); ap.add_argument("--layout", choices=LAYOUTS)
    ap.add_argument("--package-root", default=str(ROOT)); ap.add_argument("--label", default="this tree")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--shapes", default=",".join(f"{n}x{p}" for n, p in SHAPES))
    ap.add_argument("--out", default=None, help="write the table as JSON here")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a)
    trees = [("this tree", str(ROOT))] + ([("parent commit", a.parent_root)] if a.parent_root else [])
    rows = []
    for shape in a.shapes.split(","):
        n, p = (int(v) for v in shape.split("x"))
        for layout in LAYOUTS:
            for label, root in trees:
                cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--n", str(n), "--p", str(p), "--layout", layout,
                       "--package-root", root, "--label", label]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                except subprocess.TimeoutExpired:
                    print(f"{label} {n} x {p} {layout}: no answer in {a.timeout} s; nothing more is started", flush=True)
                    return 1
                if r.returncode != 0:
                    print(f"{label} {n} x {p} {layout}: exit {r.returncode}\n{r.stderr[-2000:]}", flush=True)
                    return 1                                       # whatever it was: nothing more is started on that device
                for line in r.stdout.strip().splitlines():
                    if not line.startswith("{"):
                        continue
                    row = json.loads(line)
                    rows.append(row)
                    print(f"{label:>13} {row['call']:>8} {n:>9} x {p:<4} {layout}: {row['ms_per_call']:9.2f} ms/call (spread {100 * row['spread']:4.1f} %)  "
                          f"fold order {row['foldorder_ms']:7.3f} ms  torch peak {row['peak_extra_bytes'] / 1e9:6.3f} GB  (4 n p = {row['np4_bytes'] / 1e9:.3f} GB)",
                          flush=True)
                if a.out:                                          # (after every child: a later fault keeps what was measured)
                    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                    Path(a.out).write_text(json.dumps({"nfolds": NFOLDS, "nlambda": NLAMBDA, "penalty": "lasso", "batches": BATCHES, "rows": rows},
                                                      indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
