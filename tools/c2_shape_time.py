#!/usr/bin/env python3
"""A config-2-shaped problem on the row-split path kernel's eight-wave form: n = 5,000, p = 200, 200 lambdas, tol 1e-10, MCP (gamma 2)
and SCAD (gamma 4); path-kernel cycles (best of five), rounds and the share of short ones.

    [OEMGPU_LIB=oem_amd/liboemgpu_<variant>.so] python tools/c2_shape_time.py
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oem_amd import _lib as L  # noqa: E402
import torch  # noqa: E402
from oem_amd.distributed import HipBackend, oem_sharded  # noqa: E402

lib = L.lib()
backend = HipBackend(0)
n, p = 5000, 200
rng = np.random.default_rng(2)
b = np.concatenate([rng.uniform(-1.0, 1.0, 20), np.zeros(p - 20)])
x = rng.normal(size=(n, p))
y = x @ b + rng.normal(size=n)
xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t()
yd = torch.as_tensor(y, device="cuda")
L.check(lib.oemgpu_set_timing(backend.ctx, 1))
for pen, gamma in (("mcp", 2.0), ("scad", 4.0)):
    best = None
    for _ in range(5):
        fit = oem_sharded(xd, yd, backend=backend, penalty=pen, gamma=gamma, nlambda=200, tol=1e-10)
        ms = (C.c_double * L.NTIMERS)()
        L.check(lib.oemgpu_last_timings(backend.ctx, ms))
        best = ms[6] if best is None else min(best, ms[6])
    s, r = C.c_int64(0), C.c_int64(0)
    L.check(lib.oemgpu_last_path_rounds(backend.ctx, C.byref(s), C.byref(r)))
    print(f"{pen} gamma {gamma}: path kernel {best:.0f} cycles, {r.value} rounds ({s.value} short), "
          f"niter sum {int(np.minimum(fit['niter'][0], 500).sum())}, d {fit['d']:.17g}")
