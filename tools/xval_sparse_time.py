#!/usr/bin/env python3
"""Time xval.oem on a sparse x (oemgpu_xval_sparse) at man/oem.Rd's sparse shape -- 2.5e5 x 200 at 1 %, 10 folds, 100 lambdas, lasso --
against the only route there was before it: xval_oem on the densified host copy.  The two calls ALTERNATE on one device (devices of
a pool differ by a few per cent; the alternation removes that); medians over `reps` runs each, from host memory, the whole call.
Per phase of the sparse call: HIP events through oemgpu_last_xval_sparse_timings, next to the counted work and its bound.

    python tools/xval_sparse_time.py [n] [reps]
"""
import json
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import oem_amd as oa  # noqa: E402
from oem_amd import api  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(float(args[0])) if args else 250_000
reps = int(args[1]) if len(args) > 1 else 5
p, K, nl, dens = 200, 10, 100, 0.01
rng = np.random.default_rng(123)
x = sp.random(n, p, density=dens, format="csc", random_state=np.random.RandomState(123), data_rvs=rng.standard_normal)
x.sort_indices()
b = np.concatenate([rng.uniform(0.5, 1.5, 25), np.zeros(p - 25)])
y = x @ b + rng.normal(size=n)
foldid = rng.permutation(np.resize(np.arange(1, K + 1), n))
xdense = np.asfortranarray(x.toarray())
kw = dict(foldid=foldid, penalty="lasso", nlambda=nl, tol=1e-7)
num_cu = torch.cuda.get_device_properties(0).multi_processor_count


def once(xx):
    t0 = time.perf_counter()
    f = oa.xval_oem(xx, y, **kw)
    return 1e3 * (time.perf_counter() - t0), f


once(x); once(xdense)                                            # allocations, code objects
t_sparse, t_dense, phases = [], [], []
for _ in range(reps):
    ms, fs = once(x)
    t_sparse.append(ms); phases.append(api.xval_sparse_timings())
    ms, fd = once(xdense)
    t_dense.append(ms)
assert np.allclose(fs["cvm"][0], fd["cvm"][0], rtol=1e-9)
med = {k: float(np.median([ph[k] for ph in phases])) for k in phases[0]}
nnz = int(x.nnz)
colnnz = np.diff(x.indptr)
gathers = int(np.sum(colnnz * (np.arange(p) + 1)))                # column b meets the dense copy of every column a <= b
plan = api.xval_sparse_plan(n, p, nnz, K, 1, nl, num_cu)
csr_bytes = plan["cv_lblk"] * (12 * nnz + 8 * n)                 # one read of the compressed rows (and y) per block of 64 lambdas
# The two rates are nominal peaks, not what a gather or a row walk can reach: 150 TB/s is every CU of an MI355X streaming conflict-free
# ds_read_b64 at 2.4 GHz (256 CUs x 256 B/clk), one double per gather; 6.3 TB/s is the HBM3E rate a streaming float4 copy measures
# (8.0 TB/s on paper).  The fractions below say how far a phase is from those ceilings, nothing more.
lds_rate = 150e12 / 8
hbm_rate = 6.3e12
out = {"n": n, "p": p, "nnz": nnz, "nfolds": K, "nlambda": nl, "reps": reps, "num_cu": num_cu,
       "sparse_ms_median": float(np.median(t_sparse)), "densified_ms_median": float(np.median(t_dense)),
       "sparse_ms": t_sparse, "densified_ms": t_dense, "phase_ms_median": med, "csc_route": plan["csc"], "device_bytes": plan["bytes"],
       "upload_bytes_sparse": 12 * nnz + 8 * (p + 1) + 12 * n, "upload_bytes_densified": 8 * n * p + 12 * n,
       "gram_gathers": gathers, "gram_fraction_of_lds_bound": gathers / lds_rate / (1e-3 * med["fold_moments"]) if med["fold_moments"] > 0 else None,
       "cv_error_bytes": csr_bytes, "cv_error_fraction_of_hbm_bound": csr_bytes / hbm_rate / (1e-3 * med["cv_error"]) if med["cv_error"] > 0 else None,
       "iters_full_fit": int(np.sum(fs["niter"][0])), "lambda_min": float(fs["lambda.min"])}
out["sparse_not_slower"] = bool(out["sparse_ms_median"] <= out["densified_ms_median"])
print(json.dumps(out))
if not out["sparse_not_slower"]:
    print("SLOWER: the sparse call's median exceeds the densified call's at this shape", file=sys.stderr)
    sys.exit(1)
