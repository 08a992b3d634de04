#!/usr/bin/env python3
"""The row-split path kernel outside its OEM rounds, by stamped segment: prologue, Lanczos steps, Ritz looks, lambda set-up,
lambda advance, tail.  For the problem of tools/path_cost.py (n = 20,000, elastic.net, 100 lambdas, tol 1e-10) at p = 100 and 200.

    tools/build_variant.sh diag path_small.hip -DOEM_PATH_DIAG
    OEMGPU_LIB=oem_amd/liboemgpu_diag.so python tools/path_fixed_part.py [p ...]

Stamps forbid overlaps the product kernel has and cost cycles themselves (about 1.5 x on a Lanczos step): read the shares and the
differences between two builds, never the totals.  The second call of each shape is the one reported (warm instruction cache); the
first call's launch -> ranking and prologue figures are printed beside it, since that is what a fresh process pays."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import oem_amd as oa  # noqa: E402
from oem_amd import _lib as L  # noqa: E402
import torch  # noqa: E402

lib = L.lib()
lib.oemgpu_diag_read_all.argtypes = [C.POINTER(C.c_ulonglong)]


def stamps():
    out = (C.c_ulonglong * 48)()
    assert lib.oemgpu_diag_read_all(out) == 0
    return np.array(list(out), dtype=np.float64)


def report(p, n=20000):
    rng = np.random.default_rng(123)
    b = np.concatenate([rng.uniform(size=p // 4), np.zeros(p - p // 4)])
    x = rng.normal(size=(n, p)) * 3.0
    y = x @ b + rng.normal(size=n)
    xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t()
    yd = torch.as_tensor(y, device="cuda")
    kw = dict(penalty="elastic.net", intercept=True, standardize=False, tol=1e-10)
    oa.oem(xd, yd, **kw)
    cold = stamps()
    fit = oa.oem(xd, yd, **kw)
    d = stamps()
    short, rounds = oa.api.last_path_rounds()
    nl = len(np.ravel(fit["niter"][0]))
    nst, looks = int(d[6]), int(d[29])
    rnd = d[0:5].sum() + d[[18, 20, 21, 22, 23]].sum()
    lan = {"product + reduce-scatter + alpha share": d[15], "stores + barrier": d[13], "reads + alpha sum": d[14],
           "orthogonalise copy + norm + rsqrt": d[17], "T stores, tests, next vector": d[19]}
    total = d[30]
    fixed = [("launch -> ranking done", d[24]), ("matrix and vectors in registers", d[25]), ("start vector normalised", d[5]),
             (f"Lanczos steps ({nst})", sum(lan.values())), ("T stores + tests of the steps with a look", d[10] - d[12:17].sum()),
             (f"Ritz looks ({looks})", d[9]),
             ("A = dI - XX + lambda-grid constants", d[26]), ("operator constants + lambda values into LDS", d[27]),
             (f"lambda advance ({nl} lambdas)", d[8]), ("last lambda's stores", d[28])]
    print(f"p={p} n={n}: {rounds} OEM rounds ({short} short), {nl} lambdas, {nst} Lanczos steps, {looks} looks; "
          f"stamped kernel {total:.0f} cycles, of which rounds {rnd:.0f}")
    print(f"  first call of the process: launch -> ranking {cold[24]:.0f}, matrix and vectors {cold[25]:.0f}, start vector {cold[5]:.0f}, "
          f"stamped kernel {cold[30]:.0f}")
    acc = rnd
    for name, v in fixed:
        print(f"  {name:46s} {v:10.0f}")
        acc += v
    print(f"  {'last stamp -> kernel end (remainder)':46s} {total - acc:10.0f}")
    print(f"  per Lanczos step ({nst} steps):")
    for name, v in lan.items():
        print(f"    {name:44s} {v / max(nst, 1):8.1f}")
    print(f"    {'total':44s} {sum(lan.values()) / max(nst, 1):8.1f}")
    for k in range(min(looks, 8)):
        print(f"  look {k + 1}: {d[32 + k]:8.0f} cycles, {int(d[40 + k])} sweeps")
    print(f"  per lambda advance: {d[8] / nl:.1f} cycles; per round (stamped): {rnd / max(rounds, 1):.1f}")


for arg in (sys.argv[1:] or ["100", "200"]):
    report(int(arg))
