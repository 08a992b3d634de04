#!/usr/bin/env python3
"""Times m binomial responses on one resident x: oem_fit_logistic_dense_multi(x, Y) on this tree against the only way the parent commit
has, a loop of m oem_fit_logistic_dense calls, each tree x shape x layout in a child process of its own under its own time limit.

    python tools/time_logistic_multi.py [--out profiles/logistic_multi_time.json] [--baseline-root DIR] [--shapes 1000000x100x16,...]
                                        [--layouts cm64,rm32] [--append] [--box NAME] [--timeout S] [--baseline-timeout S]

A call is oem_fit_logistic_dense_multi(x, Y, **kw) (this tree) or [oem_fit_logistic_dense(x, y_r, **kw) for the m columns y_r] (the
baseline tree; without --baseline-root the baseline is not measured and the table says so), kw = lasso, 100 lambdas of each
response's own grid, hessian "upper.bound", the default tolerances.  After one untimed call (and 0.2 s of untimed calls when a call is
shorter than that) come five batches of K calls, one synchronisation behind each batch; ms per call = batch time / K, reported as the
median of the five with the smallest and the largest.  K is whatever makes a batch about 0.3 s, at least 1.  The tool stops at the
first child that fails or runs out of time: nothing more is started on that device.

The row pass alone comes from the library's own HIP events (oemgpu_set_timing) of one more call: ms of all row passes over their
number (the X'Y pass of every response chunk counted in).  It is set against the bound of DESIGN.md 3.20: e n p blocks + 8 n m bytes
(e the bytes of an element of x) at the 8.0 TB/s of the HBM's specification and 4 n (p + 1) m flops at the 78.6 TFLOP/s of the FP64
matrix specification, whichever takes longer.  The lock-step overhead is sum over lambda of max_r niter (the steps all responses
wait for) against mean_r sum over lambda of niter (the steps a response needs)."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SHAPES = [(1_000_000, p, m) for p in (100, 512) for m in (1, 16, 64)]
LAYOUTS = ["cm64", "rm32"]
HBM_BYTES_PER_S, FP64_MATRIX_FLOPS = 8.0e12, 78.6e12


def make_data(torch, n, p, m, layout):
    """float32-representable x, the same in both layouts, and 0/1 responses drawn from their own sparse beta and intercept,
    generated on the device in row chunks"""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(20240601)
    B = torch.zeros((p, m), dtype=torch.float64, device=dev)
    B[:10] = (torch.rand((min(10, p), m), generator=g, device=dev, dtype=torch.float64) - 0.5) * torch.linspace(0.3, 1.5, m, device=dev, dtype=torch.float64)
    off = torch.linspace(-1.0, 1.0, m, device=dev, dtype=torch.float64)
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
        prob = torch.sigmoid(c.double() @ B + off)
        Y[r0:r1] = (torch.rand((r1 - r0, m), generator=g, device=dev, dtype=torch.float64) < prob).to(torch.float64)
    torch.cuda.synchronize()
    return x, Y


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
    kw = dict(penalty="lasso", nlambda=100)
    if a.mode == "multi":
        def call():
            return oem_amd.oem_fit_logistic_dense_multi(x, Y, **kw)
    else:
        cols = Y.t().contiguous()                                          # the m responses as contiguous device vectors

        def call():
            return [oem_amd.oem_fit_logistic_dense(x, cols[r], **kw) for r in range(m)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fits = call(); torch.cuda.synchronize()                               # untimed: the context's buffers exist from here on
    est = time.perf_counter() - t0
    if est < 0.2:
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
    ni = np.array([np.minimum(np.asarray(f["niter"][0]), 100) for f in fits])                     # [m, nl]
    row = {"n": n, "p": p, "m": m, "layout": a.layout, "mode": a.mode, "calls_per_batch": K, "ms_per_call": statistics.median(batches),
           "ms_min": min(batches), "ms_max": max(batches), "beta_abs_sum": float(sum(abs(f["beta"][0]).sum() for f in fits)),
           "steps_lockstep": int(ni.max(axis=0).sum()), "steps_mean_response": float(ni.sum(axis=1).mean())}
    if a.mode == "multi":
        plan = api.logistic_multi_plan(n, p, m, layout=0 if a.layout == "cm64" else 1, num_cu=torch.cuda.get_device_properties(0).multi_processor_count)
        ctx, lib = api.context(), L.lib()
        lib.oemgpu_set_timing(ctx, 1)
        call()
        lib.oemgpu_set_timing(ctx, 0)
        st = api.logistic_multi_stats()
        passes = st["row_passes"] + plan["response_chunks"]
        blocks = plan["blocks"] * plan["response_chunks"]
        nbytes = x.element_size() * n * p * blocks + 8 * n * m
        flops = 4 * n * (p + 1) * m
        t_bytes, t_flops = 1e3 * nbytes / HBM_BYTES_PER_S, 1e3 * flops / FP64_MATRIX_FLOPS
        row.update(row_pass_ms=st["rows_ms"] / passes, row_passes=passes, gram_ms=st["gram_ms"], inner_ms=st["inner_ms"], steps=st["steps"],
                   blocks_skipped=st["blocks_skipped"], response_blocks=blocks, bound_bytes=nbytes, bound_flops=flops,
                   bound_ms=max(t_bytes, t_flops), bound_binds="bytes" if t_bytes >= t_flops else "flops",
                   row_pass_share_of_bound=max(t_bytes, t_flops) / (st["rows_ms"] / passes))
    print(json.dumps(row))


def run_child(cmd, limit):
    """the child under its time limit, a line every minute while it runs; (exit code or None for a timeout, stdout, stderr)"""
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    t0 = time.monotonic()
    while True:
        try:
            out, err = proc.communicate(timeout=60)
            return proc.returncode, out, err
        except subprocess.TimeoutExpired:
            waited = time.monotonic() - t0
            if waited > limit:
                proc.kill()
                proc.communicate()
                return None, "", ""
            print(f"  ... {waited:.0f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--n", type=int); ap.add_argument("--p", type=int); ap.add_argument("--m", type=int)
    ap.add_argument("--layout", choices=LAYOUTS); ap.add_argument("--mode", choices=["multi", "loop"])
    ap.add_argument("--package-root", default=str(ROOT))
    ap.add_argument("--baseline-root", default=None, help="a checkout of the parent commit, built: its loop of m oem_fit_logistic_dense calls is the baseline")
    ap.add_argument("--shapes", default=",".join(f"{n}x{p}x{m}" for n, p, m in SHAPES))
    ap.add_argument("--layouts", default=",".join(LAYOUTS))
    ap.add_argument("--out", default=None, help="write the table as JSON here")
    ap.add_argument("--append", action="store_true", help="keep the rows --out already holds (a visit split into several runs)")
    ap.add_argument("--box", default="not stated", help="which machine and visit the numbers are from (goes into the JSON)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child of this tree")
    ap.add_argument("--baseline-timeout", type=int, default=900, help="seconds per child of the baseline tree (m single fits per call)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = json.loads(Path(a.out).read_text())["rows"] if a.append and a.out and Path(a.out).exists() else []
    for shape in a.shapes.split(","):
        n, p, m = (int(v) for v in shape.split("x"))
        for layout in a.layouts.split(","):
            got = {}
            for mode, root, limit in (("multi", a.package_root, a.timeout), ("loop", a.baseline_root, a.baseline_timeout)):
                if root is None:
                    continue
                cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--n", str(n), "--p", str(p), "--m", str(m), "--layout", layout,
                       "--mode", mode, "--package-root", root]
                code, out, err = run_child(cmd, limit)
                if code is None:
                    print(f"{n} x {p} x {m} {layout} {mode}: no answer in {limit} s; nothing more is started", flush=True)
                    return 1
                if code != 0:
                    print(f"{n} x {p} x {m} {layout} {mode}: exit {code}; nothing more is started\n{err[-2000:]}", flush=True)
                    return 1
                got[mode] = json.loads(out.strip().splitlines()[-1])
            row = got["multi"]
            base = got.get("loop")
            row["baseline_ms_per_call"] = base["ms_per_call"] if base else None
            row["baseline_ms_min"], row["baseline_ms_max"] = (base["ms_min"], base["ms_max"]) if base else (None, None)
            row["baseline"] = "a loop of m oem_fit_logistic_dense calls on the parent commit's tree" if base else "not measured"
            rows.append(row)
            speed = f"{base['ms_per_call'] / row['ms_per_call']:6.2f} x" if base else "baseline not measured"
            print(f"{n:>9} x {p:<4} m = {m:<3} {layout}: {row['ms_per_call']:10.2f} ms [{row['ms_min']:.2f}, {row['ms_max']:.2f}]  "
                  f"loop {base['ms_per_call'] if base else float('nan'):10.2f} ms  {speed}  row pass {row['row_pass_ms']:.3f} ms, "
                  f"{100 * row['row_pass_share_of_bound']:.0f} % of the {row['bound_binds']} bound ({row['bound_ms']:.3f} ms); "
                  f"steps {row['steps_lockstep']} lock-step / {row['steps_mean_response']:.0f} a response", flush=True)
            if a.out:                                          # (after every row: a later child that hangs loses nothing)
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                Path(a.out).write_text(json.dumps({"box": a.box, "rows": rows}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
