#!/usr/bin/env python3
"""Times predict() on a device tensor -- row-major float64, row-major float32, column-major float64 -- and on a resident SparseX of
the same shape at 1 % density, for one coefficient column and for 100, next to what a user can write on the device without it:
torch.addmm(b0, x, B) in float64 on the same tensors in the same process (for a float32 x with the .double() copy it needs).  Each
shape x layout runs in a child process of its own, one after the other on one device.

    python tools/time_predict.py [--out profiles/predict_time.json] [--shapes 1000000x100,1000000x512]

The data is that of tools/time_rowmajor.py.  Per call kind a child makes two untimed calls, then B batches of k calls back to back (a
call of predict ends synchronised; the torch product is followed by torch.cuda.synchronize() once per call, as a user who wants the
values would); ms per call is the median batch, `spread` is (slowest - fastest batch) / median.  Rates: `hbm_fraction` counts the
bytes that have to move once -- x as it lies (a sparse x: 12 bytes per stored entry and 8 per row pointer) and the n x ncol output --
against 8 TB/s; `mfma_fraction` counts the flops the kernel issues, 2 n K4 16 ceil(ncol / 16) with K4 = p + 1 rounded up to 4, against
the 78.6 TF of the FP64 MFMA pipe."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SHAPES = [(1_000_000, 100), (1_000_000, 512)]
LAYOUTS = ["rm64", "rm32", "cm64", "sparse"]
NCOLS = [1, 100]
BATCHES = 5
DENSITY = 0.01
HBM_PEAK, MFMA_PEAK = 8e12, 78.6e12


def child(a):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(1, str(ROOT / "tools"))
    import numpy as np
    import torch
    import oem_amd
    from oem_amd import api
    n, p = a.n, a.p
    rng = np.random.default_rng(20240501)
    if a.layout == "sparse":
        import scipy.sparse as sp
        xs = sp.random(n, p, density=DENSITY, format="csc", random_state=rng, dtype=np.float64)
        x = oem_amd.SparseX(xs)
        x_bytes = 12 * xs.nnz + 8 * (n + 1)
        del xs
    else:
        from time_rowmajor import make_data
        x, _ = make_data(torch, n, p, a.layout)
        x_bytes = x.numel() * x.element_size()
    for ncol in NCOLS:
        nbeta = rng.standard_normal((p + 1, ncol))
        fit = api.OemFit(beta=[nbeta], penalty=["lasso"], family="gaussian")
        fit["lambda"] = [np.geomspace(1.0, 0.01, ncol)]
        calls = {"predict": lambda: oem_amd.predict(fit, x)}
        if a.layout != "sparse":
            b0 = torch.as_tensor(nbeta[0], device=x.device)
            B = torch.as_tensor(nbeta[1:], device=x.device)

            def addmm():
                r = torch.addmm(b0, x if x.dtype == torch.float64 else x.double(), B)
                torch.cuda.synchronize()
                return r
            calls["torch.addmm"] = addmm
        K4 = (p + 1 + 3) // 4 * 4
        for name, call in calls.items():
            call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            est = time.perf_counter() - t0
            k = max(3, min(50, int(0.5 / max(est, 1e-4))))
            batches = []
            for _ in range(BATCHES):
                t0 = time.perf_counter()
                for _ in range(k):
                    call()
                batches.append(1e3 * (time.perf_counter() - t0) / k)
            med = statistics.median(batches)
            moved = x_bytes + 8 * n * ncol
            row = {"call": name, "n": n, "p": p, "layout": a.layout, "ncol": ncol, "ms_per_call": med, "batches_ms": batches,
                   "calls_per_batch": k, "spread": (max(batches) - min(batches)) / med, "bytes_moved_once": int(moved),
                   "hbm_fraction": moved / (med * 1e-3) / HBM_PEAK}
            if a.layout != "sparse" and name == "predict":
                row["mfma_fraction"] = 2.0 * n * K4 * 16 * ((ncol + 15) // 16) / (med * 1e-3) / MFMA_PEAK
            print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--n", type=int); ap.add_argument("--p", type=int); ap.add_argument("--layout", choices=LAYOUTS)
    ap.add_argument("--shapes", default=",".join(f"{n}x{p}" for n, p in SHAPES))
    ap.add_argument("--layouts", default=",".join(LAYOUTS))
    ap.add_argument("--out", default=None, help="write the table as JSON here")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for shape in a.shapes.split(","):
        n, p = (int(v) for v in shape.split("x"))
        for layout in a.layouts.split(","):
            cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--n", str(n), "--p", str(p), "--layout", layout]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(f"{n} x {p} {layout}: no answer in {a.timeout} s; nothing more is started", flush=True)
                return 1
            if r.returncode != 0:
                print(f"{n} x {p} {layout}: exit {r.returncode}\n{r.stderr[-2000:]}", flush=True)
                return 1                                           # whatever it was: nothing more is started on that device
            for line in r.stdout.strip().splitlines():
                if not line.startswith("{"):
                    continue
                row = json.loads(line)
                rows.append(row)
                mf = f"  MFMA {row['mfma_fraction']:.3f}" if "mfma_fraction" in row else ""
                print(f"{row['call']:>12} {n:>9} x {p:<4} {layout:>6} ncol {row['ncol']:>3}: {row['ms_per_call']:8.3f} ms/call (spread "
                      f"{100 * row['spread']:4.1f} %)  HBM {row['hbm_fraction']:.3f}{mf}", flush=True)
            if a.out:                                              # (after every child: a later fault keeps what was measured)
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                Path(a.out).write_text(json.dumps({"batches": BATCHES, "density": DENSITY, "hbm_peak": HBM_PEAK, "mfma_peak": MFMA_PEAK,
                                                   "rows": rows}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
