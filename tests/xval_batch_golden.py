"""The two seeded xval_oem problems behind tests/golden/xval_batch_bytes.json: the batched launch of K + 1 instances that share
instance 0's lambda grid, on the row-split engine (p = 41) and on the cooperating engine (p = 300).  The file holds the bytes xval_oem
returned BEFORE the batch learned lambda groups (PathArgs::lmax_group); tests/test_gpu_xval_multi.py holds today's xval_oem to them.

    python -m tests.xval_batch_golden OUT.json      (on a GPU; writes what this tree returns)
"""
import json
import sys

import numpy as np

PROBLEMS = {
    "p41_lasso": dict(n=600, p=41, seed=4101, penalty="lasso", nlambda=12, compute_loss=False),
    "p300_mcp": dict(n=900, p=300, seed=30001, penalty="mcp", nlambda=10, compute_loss=True),
}
NFOLDS = 4


def problem(name):
    s = PROBLEMS[name]
    rng = np.random.default_rng(s["seed"])
    n, p = s["n"], s["p"]
    x = (rng.normal(size=(n, p)) * (1.0 + rng.uniform(size=p)) + 0.3).astype(np.float32).astype(np.float64)
    b = np.zeros(p)
    b[rng.choice(p, 8, replace=False)] = rng.uniform(-1, 1, 8)
    y = x @ b + rng.normal(size=n) + 1.0
    foldid = rng.permutation(np.resize(np.arange(1, NFOLDS + 1), n))
    return x, y, foldid


def run(oa, name):
    """xval_oem on the problem's column-major device tensor -> {"beta", "lambda", "cvm"} as hex of their float64 bytes"""
    import torch
    s = PROBLEMS[name]
    x, y, foldid = problem(name)
    xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t()
    fit = oa.xval_oem(xd, y, foldid=foldid, penalty=s["penalty"], nlambda=s["nlambda"], tol=1e-9, compute_loss=s["compute_loss"])
    return {k: np.ascontiguousarray(np.asarray(fit[k][0], dtype=np.float64)).tobytes().hex() for k in ("beta", "lambda", "cvm")}


if __name__ == "__main__":
    import oem_amd
    with open(sys.argv[1], "w") as f:
        json.dump({name: run(oem_amd, name) for name in PROBLEMS}, f, indent=0, sort_keys=True)
