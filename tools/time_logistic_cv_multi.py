#!/usr/bin/env python3
"""Times the cross-validation of m binomial responses on one resident x: cv_oem_logistic_multi(x, Y) on this tree against the only way
the parent commit has, a loop of m cv_oem(x, y_r, family="binomial") calls with the same foldid, each tree x shape x layout in a child
process of its own under its own time limit.

    python tools/time_logistic_cv_multi.py [--out profiles/logistic_cv_multi_time.json] [--baseline-root DIR] [--shapes 1000000x100x16,...]
                                           [--layouts cm64,rm32] [--append] [--box NAME] [--timeout S] [--baseline-timeout S] [--single-above S]

kw = lasso, 100 lambdas of each fit's own grid, 10 folds, type_measure "deviance", hessian "upper.bound", the default tolerances.  After
one untimed call come five batches of one call each, a synchronisation behind each; ms per call is the median of the five, reported
with the smallest and the largest.  A baseline whose untimed call takes longer than --single-above seconds is not repeated five times:
that one call (made after a warm-up cv_oem of one response, so that the context's buffers exist) is the number, marked "single_run".
The tool stops at the first child that fails or runs out of time: nothing more is started on that device.

From one more call of this tree with the library's HIP events on (oemgpu_set_timing; the events synchronise every stage, so this call is
slower than the timed ones and only its SHARES are reported): the ms of the row passes, of the Gram builds with their Lanczos runs and
of the inner solves inside the one fold-fit call, and what the call spends outside it -- the scoring of the held-out rows and the cv
layer on the host.  The lock-step overhead: the lock-step IRLS steps of the call (summed over its chunks of 64 instances) against
the steps an instance needs alone (sum over lambda of its niter), as the mean and the largest over the instances."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
from time_logistic_multi import make_data, run_child  # noqa: E402

SHAPES = [(1_000_000, 100, m) for m in (1, 4, 16)]
LAYOUTS = ["cm64", "rm32"]
NFOLDS = 10


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
    foldid = np.random.default_rng(20240602).permutation(np.resize(np.arange(1, NFOLDS + 1), n))
    kw = dict(penalty="lasso", nlambda=100, foldid=foldid)
    if a.mode == "multi":
        def call():
            return oem_amd.cv_oem_logistic_multi(x, Y, **kw)
    else:
        cols = Y.t().contiguous()                                          # the m responses as contiguous device vectors

        def call():
            return [oem_amd.cv_oem(x, cols[r], family="binomial", **kw) for r in range(m)]
    if a.mode == "loop" and m > 1:
        oem_amd.cv_oem(x, Y[:, 0].contiguous(), family="binomial", **kw)   # untimed: the context's buffers exist from here on
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = call(); torch.cuda.synchronize()
    est = time.perf_counter() - t0
    single = a.mode == "loop" and est > a.single_above
    batches = [1e3 * est]
    if not single:
        batches = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            batches.append(1e3 * (time.perf_counter() - t0))
    row = {"n": n, "p": p, "m": m, "layout": a.layout, "mode": a.mode, "nfolds": NFOLDS, "single_run": single, "ms_per_call": statistics.median(batches),
           "ms_min": min(batches), "ms_max": max(batches), "cvm_sum": float(sum(np.nansum(r["cvm"][0]) for r in res)),
           "lambda_min": [float(r["lambda.min"]) for r in res]}
    if a.mode == "multi":
        ctx, lib = api.context(), L.lib()
        lib.oemgpu_set_timing(ctx, 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(); torch.cuda.synchronize()
        total = 1e3 * (time.perf_counter() - t0)
        lib.oemgpu_set_timing(ctx, 0)
        st = api.logistic_multi_stats()
        fits = oem_amd.oem_fit_logistic_dense_multi_folds(x, Y, foldid, penalty="lasso", nlambda=100)
        alone = np.array([np.minimum(np.asarray(f["niter"][0]), 100).sum() for per in fits for f in per])
        row.update(timed_call_ms=total, fits_ms=st["wall_ms"], rows_ms=st["rows_ms"], gram_lanczos_ms=st["gram_ms"], inner_ms=st["inner_ms"],
                   scoring_and_cv_layer_ms=total - st["wall_ms"], share_rows=st["rows_ms"] / total, share_gram_lanczos=st["gram_ms"] / total,
                   share_inner=st["inner_ms"] / total, share_scoring_and_cv_layer=(total - st["wall_ms"]) / total, instances=int(m * (NFOLDS + 1)),
                   steps_lockstep=int(st["steps"]), row_passes=int(st["row_passes"]), grams=int(st["grams"]), lanczos=int(st["lanczos"]),
                   steps_alone_mean=float(alone.mean()), steps_alone_max=int(alone.max()))
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--n", type=int); ap.add_argument("--p", type=int); ap.add_argument("--m", type=int)
    ap.add_argument("--layout", choices=LAYOUTS); ap.add_argument("--mode", choices=["multi", "loop"])
    ap.add_argument("--package-root", default=str(ROOT))
    ap.add_argument("--baseline-root", default=None, help="a checkout of the parent commit, built: its loop of m cv_oem(family='binomial') calls is the baseline")
    ap.add_argument("--shapes", default=",".join(f"{n}x{p}x{m}" for n, p, m in SHAPES))
    ap.add_argument("--layouts", default=",".join(LAYOUTS))
    ap.add_argument("--out", default=None, help="write the table as JSON here")
    ap.add_argument("--append", action="store_true", help="keep the rows --out already holds (a visit split into several runs)")
    ap.add_argument("--box", default="not stated", help="which machine and visit the numbers are from (goes into the JSON)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child of this tree")
    ap.add_argument("--baseline-timeout", type=int, default=600, help="seconds per child of the baseline tree")
    ap.add_argument("--single-above", type=float, default=30.0, help="a baseline call longer than this many seconds is timed once")
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
                       "--mode", mode, "--package-root", root, "--single-above", str(a.single_above)]
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
            row["baseline_single_run"] = base["single_run"] if base else None
            row["baseline"] = "a loop of m cv_oem(family='binomial') calls on the parent commit's tree" if base else "not measured"
            row["same_lambda_min_as_baseline"] = (row["lambda_min"] == base["lambda_min"]) if base else None
            rows.append(row)
            speed = f"{base['ms_per_call'] / row['ms_per_call']:6.2f} x" if base else "baseline not measured"
            print(f"{n:>9} x {p:<4} m = {m:<3} {layout}: {row['ms_per_call']:10.1f} ms [{row['ms_min']:.1f}, {row['ms_max']:.1f}]  "
                  f"loop {base['ms_per_call'] if base else float('nan'):10.1f} ms{' (one run)' if base and base['single_run'] else ''}  {speed}  "
                  f"shares: rows {100 * row['share_rows']:.0f} %, Gram + Lanczos {100 * row['share_gram_lanczos']:.0f} %, inner {100 * row['share_inner']:.0f} %, "
                  f"scoring + cv layer {100 * row['share_scoring_and_cv_layer']:.0f} %; steps {row['steps_lockstep']} lock-step / "
                  f"{row['steps_alone_mean']:.0f} an instance alone (max {row['steps_alone_max']})", flush=True)
            if a.out:                                          # (after every row: a later child that hangs loses nothing)
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                Path(a.out).write_text(json.dumps({"box": a.box, "rows": rows}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
