"""The seeded problems behind tests/golden/launch_drivers_bytes.json: one per branch of the launch-per-iteration host drivers of
oem_amd/csrc/path_large.hip (run_path_large, run_path_wide_nr, run_path_wide_blocks, run_path_sparse_wide).  The file holds what the
tree returned BEFORE those drivers took their pointers from path_large_layout.hpp and their batch loop from replay_batches;
tests/test_gpu_launch_drivers_bytes.py holds today's tree to the same bytes.

    python -m tests.launch_drivers_golden OUT.json      (on a GPU; writes what this tree returns)

A result is recorded as the bytes of lambda, niter, d (and loss where the case asks for it) in hex, and beta as the SHA-256 of its
float64 bytes with its count of non-zeros (beta at q = 4097 would be a quarter of a megabyte of hex; equal digests are equal bytes).
"""
import hashlib
import json
import os
import sys
import warnings

import numpy as np

_NO_WIDE_PERSISTENT = ("OEM_WIDE", "OEM_NO_WCOOP", "OEM_NO_WSTREAM")      # (OEM_NO_WCOOP also switches path_wres_kernel off)


def _runs(k):
    return lambda q: np.arange(q) // k + 1


def _scattered(q):
    return np.random.default_rng(q).permutation(np.repeat(np.arange(1, q // 20 + 1), 20))


# kind "xtx": oem_xtx on a q x q Gram; "dense": oem on an n x p device tensor; "sparse": oem / sparse_wide_fold_fit on a SparseX.
# env: the switches that keep the persistent engines away at that size (paths.hip: plan_paths), so that the launches take the call.
CASES = {
    # fused Lanczos in its ragged form, replicated update <8, false> (group operators make the whole call non-element-wise)
    "xtx300_lasso_grp": dict(kind="xtx", q=300, seed=300, env=("OEM_NO_COOP",), engine="launches",
                             kw=dict(penalty=["lasso", "grp.lasso"], groups=_runs(8), nlambda=5, maxit=200)),
    # fused Lanczos full form, oem_fused_kernel<8>
    "xtx512_lasso": dict(kind="xtx", q=512, seed=512, env=("OEM_NO_COOP",), engine="launches", kw=dict(penalty=["lasso"], nlambda=5, maxit=200)),
    # packed triangle: pack, Lanczos through the packed product + lanczos_update_reg_kernel<8>, (head, product) pairs
    "xtx1025_lasso_mcp": dict(kind="xtx", q=1025, seed=1025, env=("OEM_NO_SYMCOOP",), engine="launches",
                              kw=dict(penalty=["lasso", "mcp"], nlambda=5, maxit=100)),
    # the pairs with head_gen (the `gen` region).  Only oem() accelerates or computes a loss (oem_xtx passes neither on), so this row is
    # the dense entry at p = 1025: same Gram engine, same switch.
    "dense1025_lasso_accel_loss": dict(kind="dense", n=1300, p=1025, seed=10250, env=("OEM_NO_SYMCOOP",), engine="launches", loss=True,
                                       kw=dict(penalty=["lasso"], nlambda=4, maxit=100, accelerate=True, compute_loss=True)),
    # replicated update with the packed buffer present (q <= 2048): scattered groups are no head's
    "xtx1200_grp_scattered": dict(kind="xtx", q=1200, seed=1200, env=("OEM_NO_SYMCOOP",), engine="launches",
                                  kw=dict(penalty=["grp.lasso"], groups=_scattered, nlambda=4, maxit=100)),
    # (packed product, update) pairs with the non-zero flags, update_lds: runs of 120 are longer than a head takes (96)
    "xtx2100_grp_runs120": dict(kind="xtx", q=2100, seed=2100, env=("OEM_NO_SYMCOOP",), engine="launches",
                                kw=dict(penalty=["grp.lasso"], groups=_runs(120), nlambda=4, maxit=60)),
    # symgemv Lanczos, oem_symfused_kernel, the SState behind the partial vectors
    "xtx4096_lasso": dict(kind="xtx", q=4096, seed=4096, env=("OEM_NO_SYMCOOP",), engine="launches", kw=dict(penalty=["lasso"], nlambda=4, maxit=60)),
    # row-streaming launch_gemv + path_update_kernel<8> pairs
    "xtx4097_lasso_nosym": dict(kind="xtx", q=4097, seed=4097, env=("OEM_NO_SYM",), engine="launches", kw=dict(penalty=["lasso"], nlambda=4, maxit=60)),
    # p >= n, one row block: fused form (batch 64), group-fused form, general form (batch 32) for groups and for Nesterov's step
    "wide50_lasso": dict(kind="dense", n=50, p=200, seed=50200, env=_NO_WIDE_PERSISTENT, engine="wlaunches",
                         kw=dict(penalty=["lasso"], nlambda=5, maxit=200)),
    "wide50_grp_fused": dict(kind="dense", n=50, p=200, seed=50200, env=_NO_WIDE_PERSISTENT, engine="wlaunches",
                             kw=dict(penalty=["grp.lasso"], groups=_runs(4), nlambda=5, maxit=200)),
    "wide50_grp_general": dict(kind="dense", n=50, p=200, seed=50200, env=_NO_WIDE_PERSISTENT + ("OEM_WIDE_NO_GROUP_FUSED",), engine="wlaunches",
                               kw=dict(penalty=["grp.lasso"], groups=_runs(4), nlambda=5, maxit=200)),
    "wide50_lasso_accel": dict(kind="dense", n=50, p=200, seed=50200, env=_NO_WIDE_PERSISTENT, engine="wlaunches",
                               kw=dict(penalty=["lasso"], nlambda=5, maxit=200, accelerate=True)),
    # two row blocks (n > 2048): run_path_wide_blocks, batch 16
    "wide2100_lasso_grp": dict(kind="dense", n=2100, p=2200, seed=21002200, env=_NO_WIDE_PERSISTENT, engine="wlaunches",
                               kw=dict(penalty=["lasso", "grp.lasso"], groups=_runs(4), nlambda=4, maxit=30)),
    # the resident sparse x, no intercept: the full fit, and a fold fit (masked start vector, nk rows)
    "sparse40_full": dict(kind="sparse", n=40, p=120, seed=40120, env=(), engine="sparse-wide", kw=dict(penalty=["lasso", "grp.lasso"], groups=_runs(4), nlambda=5, maxit=200)),
    "sparse40_fold": dict(kind="sparse", n=40, p=120, seed=40120, env=(), engine="sparse-wide", fold=1,
                          kw=dict(penalty=["lasso", "grp.lasso"], groups=_runs(4), nlambda=5, maxit=200)),
}
NFOLDS = 4
SWITCHES = sorted({s for c in CASES.values() for s in c["env"]})


def problem(name):
    """the case's inputs on the host: (xtx, xty) | (x, y) | (scipy csc x, y, foldid)"""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    if c["kind"] == "xtx":                                           # a low-rank part plus a diagonal: positive definite, made in O(64 q^2)
        q = c["q"]
        f = rng.normal(size=(q, 64)) * rng.uniform(0.5, 1.5, size=(q, 1))
        xtx = f @ f.T / 64.0 + np.diag(rng.uniform(0.5, 1.5, q))
        xtx = np.asfortranarray(0.5 * (xtx + xtx.T))
        b = np.zeros(q)
        b[rng.choice(q, 12, replace=False)] = rng.uniform(-1, 1, 12)
        return xtx, xtx @ b + 0.05 * rng.normal(size=q)
    n, p = c["n"], c["p"]
    x = (rng.normal(size=(n, p)) * (1.0 + rng.uniform(size=p)) + 0.3).astype(np.float32).astype(np.float64)
    if c["kind"] == "sparse":
        import scipy.sparse as sp
        x = sp.csc_matrix(x * (rng.uniform(size=(n, p)) < 0.2))
    b = np.zeros(p)
    b[rng.choice(p, 8, replace=False)] = rng.uniform(-1, 1, 8)
    y = x @ b + rng.normal(size=n) + 1.0
    if c["kind"] == "sparse":
        return x, y, rng.permutation(np.resize(np.arange(1, NFOLDS + 1), n)).astype(np.int32)
    return x, y


def run(oa, name):
    """the case on this tree, the switches already as CASES[name]["env"] says -> (record, engine name)"""
    import torch
    from oem_amd import api
    c = CASES[name]
    kw = dict(c["kw"], tol=1e-9)
    if "groups" in kw:
        kw["groups"] = kw["groups"](c.get("q", c.get("p")))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if c["kind"] == "xtx":
            xtx, xty = problem(name)
            fit = oa.oem_xtx(torch.as_tensor(xtx, device="cuda"), xty, **kw)
            engine = api.last_path_engine()[0]
        elif c["kind"] == "dense":
            x, y = problem(name)
            fit = oa.oem(torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t(), y, **kw)
            engine = api.last_path_engine()[0]
        else:
            x, y, foldid = problem(name)
            with api.SparseX(x) as sx:
                if c.get("fold"):
                    fit = api.sparse_wide_fold_fit(sx, torch.as_tensor(y, device="cuda"), torch.as_tensor(foldid, device="cuda"), NFOLDS, c["fold"], **kw)
                else:
                    fit = oa.oem(sx, y, intercept=False, **kw)
            engine = api.last_host_path_engine()
    rec = {}
    for k in range(len(kw["penalty"])):
        beta = np.ascontiguousarray(np.asarray(fit["beta"][k], dtype=np.float64))
        rec["beta%d" % k] = hashlib.sha256(beta.tobytes()).hexdigest()
        rec["nonzero%d" % k] = int(np.count_nonzero(beta))
        rec["lambda%d" % k] = np.ascontiguousarray(np.asarray(fit["lambda"][k], dtype=np.float64)).tobytes().hex()
        rec["niter%d" % k] = np.ascontiguousarray(np.ravel(fit["niter"][k]).astype(np.int64)).tobytes().hex()
        if c.get("loss"):
            rec["loss%d" % k] = np.ascontiguousarray(np.asarray(fit["loss"][k], dtype=np.float64)).tobytes().hex()
    rec["d"] = np.float64(fit["d"]).tobytes().hex()
    return rec, engine


if __name__ == "__main__":
    import oem_amd
    from oem_amd import _lib
    out = {}
    for name, c in CASES.items():
        for s in SWITCHES:
            os.environ.pop(s, None)
        for s in c["env"]:
            os.environ[s] = "1"
        _lib.reload_switches()
        out[name], engine = run(oem_amd, name)
        assert engine == c["engine"], (name, engine)
        print(name, engine, {k: v for k, v in out[name].items() if k.startswith("nonzero")}, flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
