#!/usr/bin/env python3
"""Times oem_fit_logistic_dense() on the same data handed over as a row-major float64 tensor, a row-major float32 tensor and a
column-major float64 tensor, each shape x layout in a child process of its own (the scheme of tools/time_rowmajor.py).

    python tools/time_logistic_rowmajor.py [--out profiles/logistic_rowmajor_time.json] [--package-root DIR --label "parent commit"]
                                           [--shapes 1000000x100,1000000x512]

The timed step is the Python call oem_fit_logistic_dense(x, y, penalty="lasso", nlambda=100, hessian_type=h) itself, for h =
"upper.bound" and "full", because what is compared is what the call does with the tensor it is given: reads it in place, or converts
and transposes it first.  Untimed calls for 0.2 s (the clocks settle) and W warm-up calls, then K timed calls back to back with one
synchronisation behind them; ms per call = wall time / K (K: what fits --budget seconds, 2 to 50).  Besides the time a child reports
the peak of torch's allocated bytes during one call (the copies show there; the library's own workspace does not) and, from one more
call with the library's stage timers on (oemgpu_last_logistic_stats), the row pass alone: HIP-event milliseconds over the row passes
that build no Hessian, and their number.

--package-root: the checkout whose oem_amd is timed (default: this one).  The same script on the parent commit's tree gives the
"before" table: there every row-major tensor goes through the float64 conversion and the transposed copy."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SHAPES = [(1_000_000, 100), (1_000_000, 512)]
LAYOUTS = ["rm64", "rm32", "cm64"]
HESSIANS = ["upper.bound", "full"]
FAULTS = (134, 139, 124, 137)


def make_data(torch, n, p, layout):
    """float32-representable data, the same in every layout, generated on the device in row chunks (no n x p temporary besides x)"""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(20240601)
    b = torch.zeros(p, dtype=torch.float64, device=dev)
    b[:25] = torch.rand(25, generator=g, device=dev, dtype=torch.float64) - 0.5
    if layout == "cm64":
        store = torch.empty((p, n), dtype=torch.float64, device=dev)       # (p, n) row-major == (n, p) column-major
        x = store.t()
    else:
        x = torch.empty((n, p), dtype=torch.float64 if layout == "rm64" else torch.float32, device=dev)
    y = torch.empty(n, dtype=torch.float64, device=dev)
    step = 500_000
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        c = torch.randn((r1 - r0, p), generator=g, device=dev, dtype=torch.float32)
        x[r0:r1] = c.to(x.dtype)
        u = torch.rand(r1 - r0, generator=g, device=dev, dtype=torch.float64)
        y[r0:r1] = (u < torch.sigmoid(c.double() @ b + 0.3)).double()
    torch.cuda.synchronize()
    return x, y


def child(a):
    sys.path.insert(0, str(Path(a.package_root).resolve()))
    import ctypes as C
    import torch
    import oem_amd
    from oem_amd import api
    from oem_amd import _lib as L
    assert Path(oem_amd.__file__).resolve().parent.parent == Path(a.package_root).resolve()
    n, p = a.n, a.p
    x, y = make_data(torch, n, p, a.layout)
    yh = y.cpu().numpy()
    out = {"n": n, "p": p, "layout": a.layout, "x_bytes": int(x.numel() * x.element_size())}
    for h in HESSIANS:
        def solve():
            return oem_amd.oem_fit_logistic_dense(x, yh, penalty="lasso", nlambda=100, hessian_type=h)
        solve(); torch.cuda.synchronize()                                  # (the context and its workspace exist from here on)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.max_memory_allocated()
        t0 = time.perf_counter()
        solve(); torch.cuda.synchronize()
        est = time.perf_counter() - t0
        extra = torch.cuda.max_memory_allocated() - base
        tend = time.perf_counter() + 0.2
        while time.perf_counter() < tend:
            solve()
        steps = max(2, min(50, int(a.budget / max(est, 1e-4))))
        warm = 1 if est > 0.5 else min(3, steps)
        for _ in range(warm):
            solve()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fit = solve()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ctx = api.context()
        lib = L.lib()
        lib.oemgpu_set_timing(ctx, 1)
        solve()
        st = (C.c_double * 8)()
        lib.oemgpu_last_logistic_stats(st)
        lib.oemgpu_set_timing(ctx, 0)
        ms_rows, ms_gram, ms_inner, irls, _, passes, grams, _ = list(st)
        plain = passes - grams                                             # row passes that build no Hessian: what ms_rows times
        out[h] = {"ms_per_call": 1e3 * dt / steps, "steps": steps, "warmup": warm, "peak_extra_bytes": int(extra),
                  "ms_rows": ms_rows, "plain_row_passes": plain, "ms_per_row_pass": ms_rows / plain if plain else None,
                  "ms_gram": ms_gram, "grams": grams, "ms_inner": ms_inner, "irls_steps": irls,
                  "beta_abs_sum": float(abs(fit["beta"][0]).sum())}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--n", type=int); ap.add_argument("--p", type=int); ap.add_argument("--layout", choices=LAYOUTS)
    ap.add_argument("--package-root", default=str(ROOT))
    ap.add_argument("--shapes", default=",".join(f"{n}x{p}" for n, p in SHAPES))
    ap.add_argument("--out", default=None, help="write the table as JSON here")
    ap.add_argument("--label", default="this commit", help="what the table is of (goes into the JSON)")
    ap.add_argument("--budget", type=float, default=2.0, help="seconds of timed calls per child and Hessian type (at least 2 calls)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for shape in a.shapes.split(","):
        n, p = (int(v) for v in shape.split("x"))
        for layout in LAYOUTS:
            cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--n", str(n), "--p", str(p), "--layout", layout,
                   "--package-root", a.package_root, "--budget", str(a.budget)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(f"{n} x {p} {layout}: no answer in {a.timeout} s; nothing more is started", flush=True)
                return 1
            if r.returncode != 0:
                print(f"{n} x {p} {layout}: exit {r.returncode}\n{r.stderr[-2000:]}", flush=True)
                if r.returncode < 0 or r.returncode in FAULTS:
                    return 1                                   # a fault or a hang: nothing more is started on that device
                continue
            row = json.loads(r.stdout.strip().splitlines()[-1])
            rows.append(row)
            if a.out:                                          # (after every row: a run cut short keeps what it has)
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                Path(a.out).write_text(json.dumps({"tree": a.label, "rows": rows}, indent=1) + "\n")
            for h in HESSIANS:
                v = row[h]
                rp = v["ms_per_row_pass"]
                print(f"{n:>9} x {p:<4} {layout} {h:<11}: {v['ms_per_call']:10.2f} ms/call  row pass {rp if rp is None else round(rp, 4)} ms "
                      f"x {v['plain_row_passes']:.0f}  gram {v['ms_gram']:9.2f} ms x {v['grams']:.0f}  peak extra "
                      f"{v['peak_extra_bytes'] / 1e9:7.3f} GB of x {row['x_bytes'] / 1e9:6.3f} GB  (K = {v['steps']})", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
