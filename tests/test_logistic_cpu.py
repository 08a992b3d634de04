"""The dense binomial fit without a GPU: the C ABI (declared, exported, its refusals before any device is looked for), the plan
self-test, the CPU restatement (tests/logistic_restatement.py) held to independent solutions, the R binding
(r/oem_shim_logistic.c) run over the stand-in R runtime, and the binomial branches of predict / logLik."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import logistic_restatement as R

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("oemgpu_fit_logistic_dense", "oemgpu_fit_logistic_dense_dev", "oemgpu_selftest_logistic_plan", "oemgpu_last_logistic_stats")


def test_entries_declared_and_exported():
    import oem_amd
    h = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "oemgpu.h").read_text(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", h), name
        assert name in oem_amd.EXPORTS, name
        assert hasattr(oem_amd.lib(), name), name
    assert "oem_fit_logistic_dense" in oem_amd.__all__


def _opts(penalty=("lasso",), p=5, groups=None, ug=None, **kw):
    from oem_amd import api
    g = np.zeros(0, np.int32) if groups is None else np.asarray(groups, np.int32)
    u = np.zeros(0, np.int32) if ug is None else np.asarray(ug, np.int32)
    return api._Args(list(penalty), [], 10, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(p), g, u, np.zeros(0))


def _call(n=50, p=5, intercept=1, hessian_full=0, irls_maxit=10, irls_tol=1e-3, **kw):
    import oem_amd
    from oem_amd import api
    a = _opts(p=p, **kw)
    x = np.asfortranarray(np.random.default_rng(0).normal(size=(n, p)))
    y = (np.arange(n) % 2).astype(np.float64)
    return oem_amd.lib().oemgpu_fit_logistic_dense(api._dptr(x), n, p, api._dptr(y), 1, intercept, hessian_full, irls_maxit, irls_tol,
                                                  C.byref(a.c), *a.outputs(p + 1))


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK), reason="a GPU is present: valid arguments would compute")
def test_valid_arguments_without_gpu_give_no_device():
    assert _call() == -2
    assert _call(hessian_full=1) == -2


def test_argument_errors_before_device():
    assert _call(hessian_full=2) == -1
    assert _call(hessian_full=-1) == -1
    assert _call(irls_maxit=0) == -1
    assert _call(irls_maxit=-3) == -1
    assert _call(irls_tol=-1.0) == -1
    # a group penalty whose groups do not cover q = p + 1 coordinates (the intercept's group first)
    assert _call(penalty=("grp.lasso",), groups=[1, 1, 2, 2, 3], ug=[1, 2, 3]) == -1


def test_refusals_before_device():
    import oem_amd
    assert _call(n=6, p=5, intercept=1) == -4           # p + intercept >= n: the reference's XWXt branch
    assert _call(n=5, p=5, intercept=0) == -4
    assert "XWXt" in oem_amd.lib().oemgpu_last_error().decode()
    x = np.random.default_rng(1).normal(size=(40, 3))
    y = (x[:, 0] > 0).astype(float)
    with pytest.raises(oem_amd.OemgpuError) as ei:
        oem_amd.oem_fit_logistic_dense(x, y, weights=np.ones(40))
    assert ei.value.code == -4 and "weights not implemented" in str(ei.value)
    with pytest.raises(ValueError, match="binary outcome"):
        oem_amd.oem_fit_logistic_dense(x, np.arange(40.0) % 3)


def test_oem_binomial_still_not_implemented():
    import oem_amd
    x = np.random.default_rng(2).normal(size=(30, 3))
    with pytest.raises(NotImplementedError):
        oem_amd.oem(x, (x[:, 0] > 0).astype(float), family="binomial")


@pytest.mark.parametrize("hessian_full", [0, 1])
@pytest.mark.parametrize("intercept", [0, 1])
def test_plan_covers_rows_and_bounds_workspace(intercept, hessian_full):
    import oem_amd
    L = oem_amd.lib()
    out = (C.c_int64 * 8)()
    for n in (2, 63, 64, 65, 1000, 4097, 50000, 1_000_000, 3_000_017):
        for p in (1, 2, 50, 100, 192, 193, 1023, 1024, 1500, 8191):
            if p + intercept >= n:
                continue
            for num_cu in (1, 80, 256):
                assert L.oemgpu_selftest_logistic_plan(n, p, intercept, hessian_full, num_cu, out) == 0
                ch, nchunk, rbz, nzblk, inner_wg, staged, ws, bound = list(out)
                assert ch % 64 == 0 and ch >= 64
                # chunk c = rows [c ch, min(n, (c + 1) ch)): every row exactly once, no empty chunk
                assert (nchunk - 1) * ch < n <= nchunk * ch
                # Z blocks: whole chunks, covering all of them
                assert rbz % ch == 0 and rbz >= ch
                assert (nzblk - 1) * (rbz // ch) < nchunk <= nzblk * (rbz // ch)
                assert rbz * (p + intercept) * 8 <= max(256 << 20, ch * (p + intercept) * 8)
                assert inner_wg == (1 if p + intercept <= 1024 else 0)
                assert staged == (1 if p <= 192 else 0)
                assert 0 < ws <= bound
    assert L.oemgpu_selftest_logistic_plan(0, 5, 1, 0, 80, out) == -1
    assert L.oemgpu_selftest_logistic_plan(100, 5, 1, 2, 80, out) == -1


def _problem(n, p, seed, b0=0.4):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, p)) * rng.uniform(0.5, 2.0, size=p)
    b = np.zeros(p)
    b[:3] = [1.2, -0.8, 0.5]
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-(x @ b + b0)))).astype(float)
    return x, y


@pytest.mark.parametrize("hessian_full", [False, True])
def test_restatement_meets_lasso_kkt(hessian_full):
    """at tight tolerances the OEM-IRLS fixed point is the minimiser of (1/n) sum logloss + lambda |b|_1 on the scaled columns"""
    x, y = _problem(400, 8, 3)
    n = x.shape[0]
    ref = R.fit(x, y, penalty=["lasso"], nlambda=6, lambda_min_ratio=0.05, tol=1e-13, irls_tol=1e-11, maxit=100000, irls_maxit=200,
                hessian_full=hessian_full)
    s = 1.0 / np.sqrt(np.sum(x * x, axis=0) / (n - 1.0))
    xs = x * s
    for i, lam in enumerate(ref["lambda"][0]):
        beta = ref["beta"][0][:, i]
        b = beta[1:] / s
        prob = 1.0 / (1.0 + np.exp(-(xs @ b + beta[0])))
        g = xs.T @ (y - prob) / n
        assert abs(np.sum(y - prob) / n) < 1e-8
        act = np.abs(b) > 0
        assert np.all(np.abs(g[act] - lam * np.sign(b[act])) < 1e-7 * max(1.0, lam)), (i, g[act], lam)
        assert np.all(np.abs(g[~act]) <= lam * (1 + 1e-8) + 1e-10)


@pytest.mark.parametrize("intercept,standardize", [(False, True), (True, False), (False, False)])
def test_restatement_meets_lasso_kkt_without_intercept_or_scaling(intercept, standardize):
    """the same fixed point with the intercept dropped (row 0 of beta stays 0) or the columns left unscaled (s = 1)"""
    x, y = _problem(400, 8, 6)
    n = x.shape[0]
    ref = R.fit(x, y, penalty=["lasso"], nlambda=6, lambda_min_ratio=0.05, tol=1e-13, irls_tol=1e-11, maxit=100000, irls_maxit=200,
                intercept=intercept, standardize=standardize)
    s = 1.0 / np.sqrt(np.sum(x * x, axis=0) / (n - 1.0)) if standardize else np.ones(x.shape[1])
    xs = x * s
    for i, lam in enumerate(ref["lambda"][0]):
        beta = ref["beta"][0][:, i]
        if not intercept:
            assert beta[0] == 0.0
        b = beta[1:] / s
        prob = 1.0 / (1.0 + np.exp(-(xs @ b + beta[0])))
        g = xs.T @ (y - prob) / n
        if intercept:
            assert abs(np.sum(y - prob) / n) < 1e-8
        act = np.abs(b) > 0
        assert np.all(np.abs(g[act] - lam * np.sign(b[act])) < 1e-7 * max(1.0, lam)), (i, g[act], lam)
        assert np.all(np.abs(g[~act]) <= lam * (1 + 1e-8) + 1e-10)


@pytest.mark.parametrize("hessian_full", [False, True])
def test_restatement_counters(hessian_full):
    """stats: the W floor and the loss clamps fire on near-separable data; a Hessian per penalty for upper.bound, per row pass for full;
    a row pass per IRLS step except the skipped first step of each later lambda"""
    x, y = R.near_separable(3000, 20, 1)
    pens = ["lasso", "mcp", "ols"]
    st = {}
    ref = R.fit(x, y, penalty=pens, nlambda=8, lambda_min_ratio=1e-3, compute_loss=True, hessian_full=hessian_full, stats=st)
    assert st["floored"] > 0 and st["clamped"] > 0, st
    assert st["grams"] == (st["rows"] if hessian_full else len(pens)), st
    later = sum(len(np.atleast_1d(ref["niter"][k])) - 1 for k in range(len(pens)))          # first steps skipped: one per later lambda
    assert st["rows"] == st["irls"] - later, st
    assert st["irls"] == sum(int(np.sum(ref["niter"][k])) for k in range(len(pens))), st     # no cap hit: niter = the steps taken
    assert st["inner"] >= st["irls"]
    st0 = {}
    R.fit(x, y, penalty=pens, nlambda=8, lambda_min_ratio=1e-3, compute_loss=False, hessian_full=hessian_full, stats=st0)
    assert st0["clamped"] == 0 and st0["floored"] == st["floored"]                           # clamps count the reported losses only
    xs, ys = _problem(400, 5, 7)                                                             # mild data: nothing floored or clamped
    st1 = {}
    R.fit(xs, ys, penalty=["lasso"], nlambda=5, compute_loss=True, stats=st1)
    assert st1["floored"] == 0 and st1["clamped"] == 0, st1


def test_restatement_agrees_with_scikit_learn():
    pytest.importorskip("sklearn")
    from sklearn.linear_model import LogisticRegression
    x, y = _problem(300, 6, 4)
    n = x.shape[0]
    ref = R.fit(x, y, penalty=["lasso"], nlambda=5, lambda_min_ratio=0.1, tol=1e-13, irls_tol=1e-11, maxit=100000, irls_maxit=200)
    s = 1.0 / np.sqrt(np.sum(x * x, axis=0) / (n - 1.0))
    xs = x * s
    for i in (1, 2, 4):
        lam = ref["lambda"][0][i]
        m = LogisticRegression(penalty="l1", C=1.0 / (n * lam), solver="saga", tol=1e-12, max_iter=200000, fit_intercept=True)
        m.fit(xs, y)
        beta = ref["beta"][0][:, i]
        assert abs(m.intercept_[0] - beta[0]) < 2e-5
        assert np.abs(m.coef_[0] - beta[1:] / s).max() < 2e-5


def test_restatement_quirks():
    """niter = irls_maxit + 1 at the cap; d = 1.0005 lambda_max of the first Gram (W = 1/4 at beta = 0)"""
    x, y = _problem(200, 4, 5)
    ref2 = R.fit(x, y, penalty=["lasso"], nlambda=3, irls_maxit=2, irls_tol=0.0, compute_loss=True)
    assert list(ref2["niter"][0]) == [3, 3, 3]                  # the cap: irls_maxit + 1
    n = x.shape[0]
    s = 1.0 / np.sqrt(np.sum(x * x, axis=0) / (n - 1.0))
    z = np.column_stack([np.full(n, 0.5), 0.5 * x * s])
    assert abs(ref2["d"] - 1.0005 * np.linalg.eigvalsh(z.T @ z / n)[-1]) < 1e-12 * ref2["d"]   # upper bound: W = 1/4 at beta = 0


def test_r_binding_compiles_and_marshals(tmp_path):
    stub, here = ROOT / "tests" / "r_api_stub", ROOT / "tests" / "r_shim_logistic"
    flags = ["-Wall", "-Wextra", "-Werror", "-I", str(stub), "-I", str(here), "-I", str(ROOT / "include")]
    objs = []
    for src in (ROOT / "r" / "oem_shim_logistic.c", stub / "r_stub_runtime.c", here / "fake_logistic.c", here / "driver.c"):
        obj = tmp_path / (src.name + ".o")
        r = subprocess.run(["gcc", "-std=c99", "-g", "-O0", *flags, "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        objs.append(str(obj))
    exe = tmp_path / "drv"
    subprocess.run(["gcc", "-o", str(exe), *objs], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "checks passed" in r.stdout and int(r.stdout.split()[3]) > 100


def test_predict_and_loglik_binomial():
    from oem_amd import api
    fit = api.OemFitBinomial(beta=[np.array([[0.5, -1.0], [1.0, 2.0], [0.0, -0.5]])], **{"lambda": [np.array([0.2, 0.1])]},
                             loss=[np.array([30.0, 25.5])], family="binomial", penalty=["lasso"], nobs=50, nvars=2)
    newx = np.array([[1.0, 2.0], [-1.0, 0.0], [0.0, 3.0]])
    eta = np.column_stack([np.ones(3), newx]) @ fit["beta"][0]
    np.testing.assert_allclose(api.predict(fit, newx), eta)
    np.testing.assert_allclose(api.predict(fit, newx, type="response"), 1.0 / (1.0 + np.exp(-eta)))
    assert np.array_equal(api.predict(fit, newx, type="class"), (eta > 0).astype(int))
    np.testing.assert_allclose(api.logLik(fit), [-30.0, -25.5])
    gauss = dict(fit, family="gaussian")
    np.testing.assert_allclose(api.predict(gauss, newx, type="response"), eta)       # the Gaussian branch is unchanged
