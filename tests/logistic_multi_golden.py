"""The three seeded oem_fit_logistic_dense_multi calls behind tests/golden/logistic_multi_bytes.json.  The file holds SHA-256 hashes of
the bytes the plain call returned BEFORE its lock-step driver learned fold instances and its row pass a fold mask;
tests/test_gpu_logistic_multi_bytes.py holds today's call to them.  The three cover the row pass's forms (LT 1, 4 and 2; 2, 4 and 8
column tiles per wave), a chunk of more than 16 responses, all three layouts of x, both layouts of Y and a group penalty.

    python -m tests.logistic_multi_golden OUT.json      (on a GPU; writes what this tree returns)
"""
import hashlib
import json
import sys

import numpy as np

from tests.logistic_multi_restatement import data

PROBLEMS = {
    "p12_m3_cm": dict(n=1500, p=12, m=3, seed=9101, layout="cm", ylayout="rm", kw=dict(penalty=["lasso", "mcp"], nlambda=12, compute_loss=True)),
    "p30_m20_f32": dict(n=1800, p=30, m=20, seed=9102, layout="f32", ylayout="cm",
                        kw=dict(penalty=["lasso", "grp.lasso"], groups=np.repeat(np.arange(1, 7), 5), nlambda=6, compute_loss=True)),
    "p300_m18_rm": dict(n=2100, p=300, m=18, seed=9103, layout="rm", ylayout="rm",
                        kw=dict(penalty=["lasso"], nlambda=4, compute_loss=True, lambda_min_ratio=0.05, intercept=False)),
}


def run(oa, name):
    """the call on the problem's device tensors -> {"beta", "lambda", "niter", "loss", "d"}: SHA-256 over the m responses' bytes"""
    import torch
    s = PROBLEMS[name]
    x, Y = data(s["n"], s["p"], s["m"], s["seed"])
    x = x.astype(np.float32).astype(np.float64)
    if s["layout"] == "cm":
        xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t()
    else:
        xd = torch.as_tensor(np.ascontiguousarray(x), device="cuda").to(torch.float32 if s["layout"] == "f32" else torch.float64)
    Yd = torch.as_tensor(np.ascontiguousarray(Y), device="cuda") if s["ylayout"] == "rm" else torch.as_tensor(np.ascontiguousarray(Y.T), device="cuda").t()
    fits = oa.oem_fit_logistic_dense_multi(xd, Yd, **s["kw"])
    out = {}
    for key, dt in (("beta", np.float64), ("lambda", np.float64), ("niter", np.int32), ("loss", np.float64)):
        h = hashlib.sha256()
        for f in fits:
            for a in f[key]:
                h.update(np.ascontiguousarray(np.asarray(a, dtype=dt)).tobytes())
        out[key] = h.hexdigest()
    out["d"] = hashlib.sha256(b"".join(np.float64(f["d"]).tobytes() for f in fits)).hexdigest()
    return out


if __name__ == "__main__":
    import oem_amd
    with open(sys.argv[1], "w") as f:
        json.dump({name: run(oem_amd, name) for name in PROBLEMS}, f, indent=0, sort_keys=True)
