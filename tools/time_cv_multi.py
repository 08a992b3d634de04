#!/usr/bin/env python3
"""Times cv.oem for m Gaussian responses on one resident x: cv_oem_multi(x, Y, foldid) on this tree against the only way the parent
commit has, a loop of m cv_oem() calls, each tree x shape x layout in a child process of its own.

    python tools/time_cv_multi.py [--out profiles/cv_multi_time.json] [--baseline-root DIR] [--shapes 1000000x100x16,...] [--box NAME]

A call is cv_oem_multi(x, Y, foldid=f, **kw) (this tree) or [cv_oem(x, y_r, foldid=f, **kw) for the m contiguous columns y_r] (the
baseline tree -- never this tree's own loop; without --baseline-root the baseline is not measured and the table says so), kw = lasso,
100 lambdas of each fit's own grid, 10 folds, tol 1e-7.  Data and clock as in tools/time_multi.py: one untimed call, 0.2 s of untimed
calls, then five batches of K synchronised calls; ms per call = batch time / K, the median of the five with the smallest and the largest.

The phases come from the library's own HIP events (oemgpu_set_timing; oemgpu_last_cv_multi_timings), the median of five timed calls
(a timed call waits for every phase's end, so it is not the fast one).  Two of them are set against their bounds: the
interpolation against 3 x 8 bytes per table entry (m nfolds nl (p + 1) entries) at the 8.0 TB/s of the HBM's specification, and the
scoring against 2 n (p + 1) nl m flops at the 78.6 TFLOP/s of the FP64 matrix specification."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
from time_multi import FAULTS, FP64_MATRIX_FLOPS, HBM_BYTES_PER_S, LAYOUTS, make_data  # noqa: E402

SHAPES = [(1_000_000, 100, 1), (1_000_000, 100, 16), (1_000_000, 100, 256), (1_000_000, 512, 16)]
NFOLDS, NLAMBDA = 10, 100
PHASES = ["fold_order", "fold_gram", "fold_xty", "compose", "paths", "interp", "score"]


def child(a):
    sys.path.insert(0, str(Path(a.package_root).resolve()))
    import numpy as np
    import torch
    import oem_amd
    from oem_amd import api
    from oem_amd import _lib as L
    assert Path(oem_amd.__file__).resolve().parent.parent == Path(a.package_root).resolve()
    n, p, m = a.n, a.p, a.m
    x, Y = make_data(torch, n, p, m, a.layout)
    fid = np.random.default_rng(7).permutation(np.resize(np.arange(1, NFOLDS + 1), n))
    kw = dict(penalty="lasso", nlambda=NLAMBDA, tol=1e-7, foldid=fid)
    if a.mode == "multi":
        def call():
            return oem_amd.cv_oem_multi(x, Y, **kw)
    else:
        cols = Y.t().contiguous()                                          # the m responses as contiguous vectors: nothing is copied per call

        def call():
            return [oem_amd.cv_oem(x, cols[r], **kw) for r in range(m)]
    torch.cuda.synchronize()
    call(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    fits = call(); torch.cuda.synchronize()
    est = time.perf_counter() - t0
    tend = time.perf_counter() + 0.2
    while time.perf_counter() < tend:
        call()
    K = max(1, min(100, int(0.3 / max(est, 1e-4))))
    batches = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            call()
        torch.cuda.synchronize()
        batches.append(1e3 * (time.perf_counter() - t0) / K)
    row = {"n": n, "p": p, "m": m, "layout": a.layout, "mode": a.mode, "nfolds": NFOLDS, "nlambda": NLAMBDA, "calls_per_batch": K,
           "ms_per_call": statistics.median(batches), "ms_min": min(batches), "ms_max": max(batches),
           "cvm_sum": float(sum(np.nansum(f["cvm"][0]) for f in fits))}
    if a.mode == "multi":
        row["routes"] = sorted({int(f["route"]) for f in fits})
        plan = api.cv_multi_plan(n, p, NFOLDS, m, npen=1, nl=NLAMBDA, num_cu=torch.cuda.get_device_properties(0).multi_processor_count)
        ctx, lib = api.context(), L.lib()
        lib.oemgpu_set_timing(ctx, 1)
        seen = {k: [] for k in PHASES}
        for _ in range(5):
            call()
            for k, v in api.cv_multi_timings().items():
                seen[k].append(v)
        lib.oemgpu_set_timing(ctx, 0)
        interp_bytes, score_flops = 3 * 8 * m * NFOLDS * NLAMBDA * (p + 1), 2 * n * (p + 1) * NLAMBDA * m
        interp_bound, score_bound = 1e3 * interp_bytes / HBM_BYTES_PER_S, 1e3 * score_flops / FP64_MATRIX_FLOPS
        row.update({k + "_ms": statistics.median(v) for k, v in seen.items()})
        row.update({k + "_ms_min": min(v) for k, v in seen.items()})
        row.update({k + "_ms_max": max(v) for k, v in seen.items()})
        row.update(responses_per_chunk=plan["nb"], solve_chunks=plan["solve_chunks"], xty_passes=plan["passes"], aux_bytes=plan["bytes"],
                   interp_bound_bytes=interp_bytes, interp_bound_ms=interp_bound, interp_share_of_bound=interp_bound / row["interp_ms"],
                   score_bound_flops=score_flops, score_bound_ms=score_bound, score_share_of_bound=score_bound / row["score_ms"])
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--n", type=int); ap.add_argument("--p", type=int); ap.add_argument("--m", type=int)
    ap.add_argument("--layout", choices=LAYOUTS); ap.add_argument("--mode", choices=["multi", "loop"])
    ap.add_argument("--package-root", default=str(ROOT))
    ap.add_argument("--baseline-root", default=None, help="a checkout of the parent commit, built: its loop of m cv_oem() calls is the baseline")
    ap.add_argument("--shapes", default=",".join(f"{n}x{p}x{m}" for n, p, m in SHAPES))
    ap.add_argument("--out", default=None, help="write the table as JSON here")
    ap.add_argument("--box", default="not stated", help="which machine and visit the numbers are from (goes into the JSON)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for shape in a.shapes.split(","):
        n, p, m = (int(v) for v in shape.split("x"))
        for layout in LAYOUTS:
            got = {}
            for mode, root in (("multi", a.package_root), ("loop", a.baseline_root)):
                if root is None:
                    continue
                cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--n", str(n), "--p", str(p), "--m", str(m), "--layout", layout,
                       "--mode", mode, "--package-root", root]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                except subprocess.TimeoutExpired:
                    print(f"{n} x {p} x {m} {layout} {mode}: no answer in {a.timeout} s; nothing more is started", flush=True)
                    return 1
                if r.returncode != 0:
                    print(f"{n} x {p} x {m} {layout} {mode}: exit {r.returncode}\n{r.stderr[-2000:]}", flush=True)
                    if r.returncode < 0 or r.returncode in FAULTS:
                        return 1                               # a fault or a hang: nothing more is started on that device
                    continue
                got[mode] = json.loads(r.stdout.strip().splitlines()[-1])
            if "multi" not in got:
                continue
            row = got["multi"]
            base = got.get("loop")
            row["baseline_ms_per_call"] = base["ms_per_call"] if base else None
            row["baseline_ms_min"], row["baseline_ms_max"] = (base["ms_min"], base["ms_max"]) if base else (None, None)
            row["baseline"] = "a loop of m cv_oem() calls on the parent commit's tree" if base else "not measured"
            rows.append(row)
            speed = f"{base['ms_per_call'] / row['ms_per_call']:6.2f} x" if base else "baseline not measured"
            print(f"{n:>9} x {p:<4} m = {m:<4} {layout}: {row['ms_per_call']:9.3f} ms [{row['ms_min']:.3f}, {row['ms_max']:.3f}]  "
                  f"loop {base['ms_per_call'] if base else float('nan'):9.3f} ms  {speed}  phases " +
                  " ".join(f"{k} {row[k + '_ms']:.3f}" for k in PHASES) +
                  f"  interpolation {100 * row['interp_share_of_bound']:.0f} % of {row['interp_bound_ms']:.4f} ms, scoring "
                  f"{100 * row['score_share_of_bound']:.0f} % of {row['score_bound_ms']:.3f} ms", flush=True)
            if a.out:                                          # (after every row: a later child that hangs loses nothing)
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                Path(a.out).write_text(json.dumps({"box": a.box, "rows": rows}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
