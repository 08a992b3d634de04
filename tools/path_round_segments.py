#!/usr/bin/env python3
"""The five stamped segments of the row-split path kernel's OEM round, full and short form side by side.

    tools/build_variant.sh diag path_small.hip -DOEM_PATH_DIAG
    OEMGPU_LIB=oem_amd/liboemgpu_diag.so python tools/path_round_segments.py [p]

Stamps forbid overlaps the product kernel has and cost cycles themselves: read the shares and the differences, never the totals.
Segments: threshold + stop rule + loop | stores + barrier | reads | FMAs | adds + reduce-scatter."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import oem_amd as oa  # noqa: E402
from oem_amd import _lib as L  # noqa: E402
import torch  # noqa: E402

p = int(sys.argv[1]) if len(sys.argv) > 1 else 100
n = 20000
rng = np.random.default_rng(123)
b = np.concatenate([rng.uniform(size=p // 4), np.zeros(p - p // 4)])
x = rng.normal(size=(n, p)) * 3.0
y = x @ b + rng.normal(size=n)
xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t()
yd = torch.as_tensor(y, device="cuda")
kw = dict(penalty="elastic.net", intercept=True, standardize=False, tol=1e-10)
oa.oem(xd, yd, **kw)
oa.oem(xd, yd, **kw)
short, rounds = oa.api.last_path_rounds()
lib = L.lib()
lib.oemgpu_diag_read.argtypes = [C.POINTER(C.c_ulonglong)]
out = (C.c_ulonglong * 24)()
assert lib.oemgpu_diag_read(out) == 0
d = np.array(list(out), dtype=np.float64)
full = rounds - short
print(f"p={p}: {rounds} OEM rounds, {short} short, {full} full; cycles per round by segment [threshold+stop+loop | stores+barrier | reads | FMAs | adds+reduce]")
if full:
    print("    full :", np.round(d[0:5] / full, 1), "sum", round(d[0:5].sum() / full, 1))
if short:
    s = d[[18, 20, 21, 22, 23]]
    print("    short:", np.round(s / short, 1), "sum", round(s.sum() / short, 1))
