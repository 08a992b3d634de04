#!/usr/bin/env python3
"""Times m responses on one resident x: oem_multi(x, Y) on this tree against the only way the parent commit has, a loop of m oem() calls,
each tree x shape x layout in a child process of its own.

    python tools/time_multi.py [--out profiles/multi_time.json] [--baseline-root DIR] [--shapes 1000000x100x16,...] [--box NAME]

A call is oem_multi(x, Y, **kw) (this tree) or [oem(x, y_r, **kw) for the m contiguous columns y_r] (the baseline tree; without
--baseline-root the baseline is not measured and the table says so), kw = lasso, 100 lambdas of each response's own grid, tol 1e-7.
After one untimed call and 0.2 s of untimed calls (the clocks settle) come five batches of K calls, one synchronisation behind each
batch; ms per call = batch time / K, reported as the median of the five with the smallest and the largest.  K is whatever makes a batch
about 0.3 s, at least 1.

The X'Y pass alone comes from the library's own HIP events (oemgpu_set_timing) of an oem_multi call: OEMGPU_T_MOMENTS spans the one
moment pass and the X'Y pass, OEMGPU_T_GRAMK the moment pass's MFMA kernel; the X'Y pass is their difference (it carries the moment
pass's reduce kernel, some microseconds), the median of five calls.  It is set against the bound of DESIGN.md 3.18: e n p passes +
8 n m bytes (e the bytes of an element of x) at the 8.0 TB/s of the HBM's specification and 2 n (p + 2) m flops at the 78.6 TFLOP/s of
the FP64 matrix specification, whichever takes longer."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SHAPES = [(1_000_000, 100, 1), (1_000_000, 100, 16), (1_000_000, 100, 256), (1_000_000, 512, 64)]
LAYOUTS = ["cm64", "rm32"]
FAULTS = (134, 139, 124, 137)
HBM_BYTES_PER_S, FP64_MATRIX_FLOPS = 8.0e12, 78.6e12


def make_data(torch, n, p, m, layout):
    """float32-representable x, the same in both layouts, and Y = x B + noise, generated on the device in row chunks"""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(20240501)
    B = torch.zeros((p, m), dtype=torch.float64, device=dev)
    B[:25] = torch.rand((min(25, p), m), generator=g, device=dev, dtype=torch.float64) - 0.5
    if layout == "cm64":
        store = torch.empty((p, n), dtype=torch.float64, device=dev)       # (p, n) row-major == (n, p) column-major
        x = store.t()
    else:
        x = torch.empty((n, p), dtype=torch.float32, device=dev)
    Y = torch.empty((n, m), dtype=torch.float64, device=dev)
    step = 250_000
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        c = torch.randn((r1 - r0, p), generator=g, device=dev, dtype=torch.float32)
        x[r0:r1] = c.to(x.dtype)
        Y[r0:r1] = c.double() @ B + torch.randn((r1 - r0, m), generator=g, device=dev, dtype=torch.float64)
    torch.cuda.synchronize()
    return x, Y


def child(a):
    sys.path.insert(0, str(Path(a.package_root).resolve()))
    import ctypes as C
    import torch
    import oem_amd
    from oem_amd import api
    from oem_amd import _lib as L
    assert Path(oem_amd.__file__).resolve().parent.parent == Path(a.package_root).resolve()
    n, p, m = a.n, a.p, a.m
    x, Y = make_data(torch, n, p, m, a.layout)
    kw = dict(penalty="lasso", nlambda=100, tol=1e-7)
    if a.mode == "multi":
        def call():
            return oem_amd.oem_multi(x, Y, **kw)
    else:
        cols = Y.t().contiguous()                                          # the m responses as contiguous vectors: nothing is copied per call

        def call():
            return [oem_amd.oem(x, cols[r], **kw) for r in range(m)]
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
    row = {"n": n, "p": p, "m": m, "layout": a.layout, "mode": a.mode, "calls_per_batch": K, "ms_per_call": statistics.median(batches),
           "ms_min": min(batches), "ms_max": max(batches), "beta_abs_sum": float(sum(abs(f["beta"][0]).sum() for f in fits))}
    if a.mode == "multi":
        row["routes"] = sorted({int(f["route"]) for f in fits})
        plan = api.multi_plan(n, p, m, layout=0 if a.layout == "cm64" else 1, num_cu=torch.cuda.get_device_properties(0).multi_processor_count)
        ctx, lib = api.context(), L.lib()
        lib.oemgpu_set_timing(ctx, 1)
        xty, mom = [], []
        for _ in range(5):
            call()
            tm = (C.c_double * L.NTIMERS)()
            lib.oemgpu_last_timings(ctx, tm)
            xty.append(tm[L.T_MOMENTS] - tm[L.T_GRAMK]); mom.append(tm[L.T_GRAMK])
        lib.oemgpu_set_timing(ctx, 0)
        nbytes = x.element_size() * n * p * plan["passes"] + 8 * n * m
        flops = 2 * n * (p + 2) * m
        t_bytes, t_flops = 1e3 * nbytes / HBM_BYTES_PER_S, 1e3 * flops / FP64_MATRIX_FLOPS
        row.update(xty_ms=statistics.median(xty), xty_ms_min=min(xty), xty_ms_max=max(xty), moment_pass_ms=statistics.median(mom),
                   xty_passes=plan["passes"], solve_chunks=plan["solve_chunks"], responses_per_launch=plan["cap"],
                   bound_bytes=nbytes, bound_flops=flops, bound_ms=max(t_bytes, t_flops), bound_binds="bytes" if t_bytes >= t_flops else "flops",
                   xty_share_of_bound=max(t_bytes, t_flops) / statistics.median(xty))
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--n", type=int); ap.add_argument("--p", type=int); ap.add_argument("--m", type=int)
    ap.add_argument("--layout", choices=LAYOUTS); ap.add_argument("--mode", choices=["multi", "loop"])
    ap.add_argument("--package-root", default=str(ROOT))
    ap.add_argument("--baseline-root", default=None, help="a checkout of the parent commit, built: its loop of m oem() calls is the baseline")
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
            row["baseline"] = "a loop of m oem() calls on the parent commit's tree" if base else "not measured"
            rows.append(row)
            speed = f"{base['ms_per_call'] / row['ms_per_call']:6.2f} x" if base else "baseline not measured"
            print(f"{n:>9} x {p:<4} m = {m:<4} {layout}: {row['ms_per_call']:9.3f} ms [{row['ms_min']:.3f}, {row['ms_max']:.3f}]  "
                  f"loop {base['ms_per_call'] if base else float('nan'):9.3f} ms  {speed}  X'Y {row['xty_ms']:.3f} ms = "
                  f"{100 * row['xty_share_of_bound']:.0f} % of the {row['bound_binds']} bound ({row['bound_ms']:.3f} ms), moment pass {row['moment_pass_ms']:.3f} ms",
                  flush=True)
            if a.out:                                          # (after every row: a later child that hangs loses nothing)
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                Path(a.out).write_text(json.dumps({"box": a.box, "rows": rows}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
