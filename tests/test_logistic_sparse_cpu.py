"""The sparse binomial fit without a GPU: the C ABI (declared, exported, its refusals and argument errors before any device is looked
for), the plan self-test, the CPU restatement (tests/logistic_sparse_restatement.py) held to the dense restatement and to the KKT
conditions, the R binding (r/oem_shim_logistic_sparse.c) run over the stand-in R runtime, and predict() on a sparse newx."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from tests import logistic_restatement as RD
from tests import logistic_sparse_restatement as RS
from tests.test_gpu_logistic_sparse_bounds import _edge_matrix

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("oemgpu_fit_logistic_sparse", "oemgpu_selftest_logistic_sparse_plan", "oemgpu_selftest_csc_plan")


def _problem(n, p, density, seed, intercept_shift=0.0):
    rng = np.random.default_rng(seed)
    x = sp.random(n, p, density=density, format="csc", random_state=rng, data_rvs=lambda k: rng.uniform(-1.0, 1.0, k) * 2.0)
    b = np.zeros(p)
    b[: max(1, p // 3)] = rng.uniform(-1.5, 1.5, max(1, p // 3))
    eta = x @ b + intercept_shift
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    return x, y


def test_entries_declared_and_exported():
    import oem_amd
    h = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "oemgpu.h").read_text(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", h), name
        assert name in oem_amd.EXPORTS, name
        assert hasattr(oem_amd.lib(), name), name
    assert "oem_fit_logistic_sparse" in oem_amd.__all__
    src = (ROOT / "oem_amd" / "build.py").read_text()
    assert '"logistic_sparse.hip"' in src


# the edge matrix of the GPU bounds file ((n, p, seed)): empty columns and rows, stored zeros, a one-entry column, rows 8191 / 8192 / n - 1
EDGE = [(8291, 9, 2), (641, 33, 62)]


def _is_the_dense_full_hessian(standardize, shape):
    x, y = _problem(300, 7, 0.3, 1) if shape is None else _edge_matrix(*shape, k=3)
    kw = dict(penalty=["lasso", "mcp"], nlambda=6, lambda_min_ratio=0.05, intercept=False, standardize=standardize, compute_loss=True,
              irls_tol=1e-6, tol=1e-9)
    if shape is not None:
        kw["irls_maxit"] = 20                                    # mcp runs away along the edge matrix's few-entry columns: a few steps of it do
    st_s, st_d = {}, {}
    a = RS.fit(x, y, stats=st_s, **kw)
    b = RD.fit(x.toarray(), y, hessian_full=True, stats=st_d, **kw)
    for k in range(2):
        # the two sum in different orders (a sparse product, a dense one): on the edge matrix, where |beta| grows to ~100, the 1e-12 is
        # taken relative to it
        atol = 1e-12 if shape is None else 1e-12 * max(1.0, float(np.abs(b["beta"][k]).max()))
        np.testing.assert_allclose(a["beta"][k], b["beta"][k], rtol=0, atol=atol)
        assert np.array_equal(a["niter"][k], b["niter"][k])
        np.testing.assert_allclose(a["loss"][k], b["loss"][k], rtol=1e-12)
        np.testing.assert_allclose(a["lambda"][k], b["lambda"][k], rtol=1e-13)
    assert a["d"] == pytest.approx(b["d"], rel=1e-13)
    assert {k: st_s[k] for k in ("irls", "inner", "rows", "grams")} == {k: st_d[k] for k in ("irls", "inner", "rows", "grams")}
    assert st_s["grams"] == st_s["rows"] and a["intval"] == 0.0


@pytest.mark.parametrize("standardize", [True, False])
def test_restatement_without_intercept_is_the_dense_full_hessian(standardize):
    _is_the_dense_full_hessian(standardize, None)


@pytest.mark.parametrize("shape", EDGE)
@pytest.mark.parametrize("standardize", [True, False])
def test_restatement_without_intercept_is_the_dense_full_hessian_on_the_edge_matrix(standardize, shape):
    _is_the_dense_full_hessian(standardize, shape)


def test_restatement_kkt_with_intercept():
    """intercept + standardize: at every lambda (B[0] / intval, B[1:]) is a lasso-logistic KKT point -- this pins eta with beta_0 as it
    is (quirk 3), the intercept's XX row only steering the iteration (6), and the in-place rescale that the next lambda starts from (9)"""
    _kkt_with_intercept(None)


@pytest.mark.parametrize("shape", EDGE)
def test_restatement_kkt_with_intercept_on_the_edge_matrix(shape):
    _kkt_with_intercept(shape)


def _kkt_with_intercept(shape):
    rng = np.random.default_rng(3)
    if shape is None:
        n, p = 400, 8
        x = sp.random(n, p, density=0.35, format="csc", random_state=rng,
                      data_rvs=lambda k: rng.choice([-1.0, 1.0], k) * rng.uniform(0.5, 1.5, k))
        eta = x @ np.array([1.2, -0.8, 0.6, 0, 0, 0, 0, 0]) + 0.4
        y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    else:
        n, p = shape[:2]
        x, y = _edge_matrix(*shape, k=3, intercept=0.4)
    st = {}
    res = RS.fit(x, y, penalty=["lasso"], nlambda=6, lambda_min_ratio=0.02, tol=1e-12, irls_tol=1e-12, maxit=200000, irls_maxit=400, stats=st)
    intval = res["intval"]
    assert intval > 0 and st["intval"] == intval
    assert np.all(res["niter"][0] <= 400)                       # every lambda converged
    xd = x.toarray()
    colsq = np.sum(xd * xd, axis=0) / (n - 1.0)
    colsq[colsq == 0.0] = 1.0                                    # an empty column (quirk 2)
    s = 1.0 / np.sqrt(colsq)
    for li, lam in enumerate(res["lambda"][0]):
        B = res["beta"][0][:, li]
        b0 = B[0] / intval
        prob = 1.0 / (1.0 + np.exp(-(xd @ B[1:] + b0)))
        r = y - prob
        assert abs(r.sum() / n) <= 1e-7
        g = s * (xd.T @ r) / n                                   # the gradient in the standardized coordinates
        nz = B[1:] != 0
        assert np.all(np.abs(g[~nz]) <= lam + 1e-7)
        assert np.all(np.abs(g[nz] - lam * np.sign(B[1:][nz])) <= 1e-7)


def test_restatement_hessian_every_step_and_intval_fixed():
    x, y = _problem(250, 5, 0.4, 4, intercept_shift=0.3)
    st = {}
    res = RS.fit(x, y, penalty=["lasso", "grp.lasso"], groups=[0, 1, 1, 2, 2, 3], unique_groups=[0, 1, 2, 3], nlambda=4, stats=st)
    assert st["grams"] == st["rows"] and st["rows"] < st["irls"]     # every row pass builds the Hessian; later lambdas skip a step
    xd = x.toarray()
    n = xd.shape[0]
    s = 1.0 / np.sqrt(np.sum(xd * xd, axis=0) / (n - 1.0))
    xs = xd * s                                                   # the first build is at beta = 0: W = 1/4
    xxdiag = np.mean(np.diag(xs.T @ (0.25 * xs)))
    assert res["intval"] == pytest.approx(np.sqrt((xxdiag / (0.25 * n)) / n), rel=1e-12)
    with pytest.raises(RS.Unsupported):
        RS.fit(x, y, intercept=True, standardize=False)
    with pytest.raises(RS.Unsupported):
        RS.fit(x[:5], y[:5], intercept=True)


# ------------------------------------------------------------------------------------------ the C entry before any device
def _opts(penalty=("lasso",), p=5, groups=None, ug=None):
    from oem_amd import api
    g = np.zeros(0, np.int32) if groups is None else np.asarray(groups, np.int32)
    u = np.zeros(0, np.int32) if ug is None else np.asarray(ug, np.int32)
    return api._Args(list(penalty), [], 10, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(p), g, u, np.zeros(0))


def _csc(n=50, p=5, seed=0, density=0.3):
    x = sp.random(n, p, density=density, format="csc", random_state=np.random.default_rng(seed))
    return (np.ascontiguousarray(x.indptr, np.int64), np.ascontiguousarray(x.indices, np.int32), np.ascontiguousarray(x.data, np.float64))


def _call(n=50, p=5, arrays=None, standardize=1, intercept=1, irls_maxit=10, irls_tol=1e-3, **kw):
    import oem_amd
    from oem_amd import api
    a = _opts(p=p, **kw)
    cp, ri, va = arrays if arrays is not None else _csc(n, p)
    y = (np.arange(n) % 2).astype(np.float64)
    return oem_amd.lib().oemgpu_fit_logistic_sparse(n, p, cp.ctypes.data, api._iptr(ri), api._dptr(va), api._dptr(y), standardize, intercept,
                                                    irls_maxit, irls_tol, C.byref(a.c), *a.outputs(p + 1))


def test_refusals_before_device_c_entry():
    assert _call(intercept=1, standardize=0) == -4              # the reference reads colsq_inv it never wrote
    assert _call(n=6, p=5, intercept=1) == -4                    # p + intercept >= n: the XWXt branch
    assert _call(n=5, p=5, intercept=0) == -4
    assert _call(n=9000, p=8192, arrays=(np.zeros(8193, np.int64), np.zeros(1, np.int32), np.zeros(1)), intercept=0) == -4   # p > 8191
    assert _call(irls_maxit=0) == -1                             # the dense fit's own checks
    assert _call(irls_tol=-1.0) == -1
    assert _call(penalty=("grp.lasso",), groups=[1, 1, 2, 2, 3], ug=[1, 2, 3]) == -1


def _call_gaussian(n, p, arrays, intercept):
    import oem_amd
    from oem_amd import api
    a = _opts(p=p)
    cp, ri, va = arrays
    y = (np.arange(n) % 2).astype(np.float64)
    return oem_amd.lib().oemgpu_fit_sparse(n, p, cp.ctypes.data, api._iptr(ri), api._dptr(va), api._dptr(y), 1, intercept, C.byref(a.c),
                                           *a.outputs(p + 1))


# (entry, n, p, intercept): the binomial entry, the Gaussian entry on both of its branches (n > p: the moments; n <= p: the dense copy
# of the wide engine, served without an intercept)
@pytest.mark.parametrize("entry,n,p,intercept", [("logistic", 50, 5, 1), ("gaussian", 50, 5, 1), ("gaussian", 50, 5, 0),
                                                 ("gaussian", 6, 10, 0)])
def test_csc_arrays_refused_before_device(entry, n, p, intercept):
    import oem_amd
    call = (lambda arr: _call(n=n, p=p, arrays=arr, intercept=intercept)) if entry == "logistic" else \
        (lambda arr: _call_gaussian(n, p, arr, intercept))
    cp, ri, va = _csc(n, p, density=0.3 if n > p else 0.5)
    assert np.any(np.diff(cp) >= 2)
    bad = cp.copy(); bad[0] = 1
    assert call((bad, ri, va)) == -1                             # colptr[0] != 0
    bad = cp.copy(); bad[2] = bad[3] + 1
    assert call((bad, ri, va)) == -1                             # colptr decreasing
    for v in (-1, n, 2 ** 31 - 1):                               # a row index outside [0, n)
        r2 = ri.copy(); r2[3] = v
        assert call((cp, r2, va)) == -1
    c0 = int(np.argmax(np.diff(cp) >= 2))                        # a column with two entries
    r2 = ri.copy(); r2[cp[c0] + 1] = r2[cp[c0]]                  # repeated row
    assert call((cp, r2, va)) == -1
    assert "strictly increasing" in oem_amd.lib().oemgpu_last_error().decode()
    r2 = ri.copy(); r2[cp[c0]], r2[cp[c0] + 1] = r2[cp[c0] + 1], r2[cp[c0]]   # decreasing rows
    assert call((cp, r2, va)) == -1
    assert "strictly increasing" in oem_amd.lib().oemgpu_last_error().decode()


def test_refusals_through_python():
    import oem_amd
    x, y = _problem(60, 4, 0.4, 2)
    with pytest.raises(oem_amd.OemgpuError) as e:
        oem_amd.oem_fit_logistic_sparse(x, y, intercept=True, standardize=False)
    assert e.value.code == -4 and "colsq_inv" in str(e.value)
    with pytest.raises(oem_amd.OemgpuError) as e:
        oem_amd.oem_fit_logistic_sparse(x[:4], y[:4])
    assert e.value.code == -4
    with pytest.raises(ValueError):
        oem_amd.oem_fit_logistic_sparse(x, y, irls_maxit=0)
    with pytest.raises(oem_amd.OemgpuError) as e:
        oem_amd.oem_fit_logistic_sparse(x, y, weights=np.ones(60))
    assert e.value.code == -4
    with pytest.raises(ValueError):
        oem_amd.oem_fit_logistic_sparse(x, y, hessian_type="newton")
    with pytest.raises(TypeError):
        oem_amd.oem_fit_logistic_sparse(x.toarray(), y)
    with pytest.raises(ValueError):
        oem_amd.oem_fit_logistic_sparse(x, np.arange(60.0) % 3)
    with pytest.raises(NotImplementedError):                     # oem(family = "binomial") is unchanged
        oem_amd.oem(x.toarray(), y, family="binomial")


def test_csc_arrays_sums_duplicates_and_leaves_the_input():
    from oem_amd import api
    # column 0: rows 3, 1, 3 (a duplicate, out of order); column 1 empty; column 2: rows 2, 0
    x = sp.csc_matrix((np.array([1.0, 2.0, 4.0, 5.0, 6.0]), np.array([3, 1, 3, 2, 0], np.int32), np.array([0, 3, 3, 5], np.int32)), shape=(4, 3))
    kept = [a.copy() for a in (x.indptr, x.indices, x.data)]
    cp, ri, va = api._csc_arrays(x)
    assert (cp.dtype, ri.dtype, va.dtype) == (np.int64, np.int32, np.float64)
    assert all(a.flags.c_contiguous for a in (cp, ri, va))
    assert cp.tolist() == [0, 2, 2, 4] and ri.tolist() == [1, 3, 0, 2] and va.tolist() == [2.0, 5.0, 6.0, 5.0]
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip((x.indptr, x.indices, x.data), kept))
    cp2, ri2, va2 = api._csc_arrays(x.tocoo().astype(np.float32))        # any format and dtype: the same arrays
    assert cp2.tolist() == cp.tolist() and ri2.tolist() == ri.tolist() and va2.tolist() == va.tolist()


def test_plan_sweep():
    import oem_amd
    lib = oem_amd.lib()
    out = (C.c_int64 * 8)()
    for n in (100, 9000, 2 * 10 ** 4, 2 * 10 ** 5, 10 ** 6, 3 * 10 ** 9):
        for p in (3, 50, 200, 1000, 1023, 1024, 4000, 6200, 8191):
            if p + 1 >= n:
                continue
            for dens in (0.001, 0.01, 0.02, 0.05, 0.3):
                nnz = int(dens * n * p)
                for icpt in (0, 1):
                    assert lib.oemgpu_selftest_logistic_sparse_plan(n, p, nnz, icpt, 256, out) == 0
                    route, inner, ws, bound, rc, nch, ch, _ = list(out)
                    rule = (8192 * 8 + 16 * p + 64 <= 160 * 1024) and nnz <= 0.02 * n * p and n < 2 ** 31
                    assert route == int(rule), (n, p, nnz)
                    assert inner == int(p + icpt <= 1024)
                    assert 0 < ws <= bound, (n, p, nnz, ws, bound)
                    assert nch * ch >= n and (nch - 1) * ch < n and ch % 64 == 0
                    assert (rc == 0) == bool(route) and (route or 64 <= rc <= n)
                    if not route:
                        assert rc * p * 8 <= 2 ** 31 or rc == 64
    assert lib.oemgpu_selftest_logistic_sparse_plan(0, 5, 10, 0, 256, out) == -1
    assert lib.oemgpu_selftest_logistic_sparse_plan(100, 5, -1, 0, 256, out) == -1


def test_csc_plan_sweep():
    """the compressed-column Gram's own plan over the grid of test_plan_sweep: every chunk lies in a range, the range sums stay under
    256 MB, and the route is open exactly while the kernel's LDS fits a CU"""
    import oem_amd
    lib = oem_amd.lib()
    out, lsp = (C.c_int64 * 4)(), (C.c_int64 * 8)()
    for n in (100, 9000, 2 * 10 ** 4, 2 * 10 ** 5, 10 ** 6, 3 * 10 ** 9):
        for p in (3, 50, 200, 1000, 1023, 1024, 4000, 6200, 8191):
            if p + 1 >= n:
                continue
            assert lib.oemgpu_selftest_csc_plan(n, p, out) == 0
            chunks, ranges, cper, lds = list(out)
            assert chunks == -(-n // 8192) and lds == 8192 * 8 + 16 * p + 64
            assert ranges >= 1, (n, p)
            assert ranges <= chunks, (n, p)
            assert cper * ranges >= chunks and (cper - 1) * ranges < chunks, (n, p)
            assert ranges * p * p * 8 <= 256e6 or ranges == 1, (n, p)
            assert lib.oemgpu_selftest_logistic_sparse_plan(n, p, 0, 0, 256, lsp) == 0
            assert lsp[0] == int(lds <= 160 * 1024 and n < 2 ** 31), (n, p)      # nnz = 0: only the LDS and the 32-bit rows decide
    for n, p, want in ((24577, 101, (4, 4, 1)), (32769, 411, (5, 4, 2)), (8193, 6140, (2, 1, 2)), (8192, 33, (1, 1, 1))):
        assert lib.oemgpu_selftest_csc_plan(n, p, out) == 0
        assert tuple(out)[:3] == want, (n, p, list(out))
    assert lib.oemgpu_selftest_csc_plan(8193, 6140, out) == 0 and out[3] == 160 * 1024
    assert lib.oemgpu_selftest_csc_plan(8193, 6141, out) == 0 and out[3] > 160 * 1024
    assert lib.oemgpu_selftest_csc_plan(0, 5, out) == -1
    assert lib.oemgpu_selftest_csc_plan(100, 0, out) == -1


def test_r_binding_compiles_and_marshals(tmp_path):
    stub, here = ROOT / "tests" / "r_api_stub", ROOT / "tests" / "r_shim_logistic_sparse"
    flags = ["-Wall", "-Wextra", "-Werror", "-I", str(stub), "-I", str(here), "-I", str(ROOT / "include")]
    objs = []
    for src in (ROOT / "r" / "oem_shim_logistic_sparse.c", stub / "r_stub_runtime.c", here / "fake_logistic_sparse.c", here / "driver.c"):
        obj = tmp_path / (src.name + ".o")
        r = subprocess.run(["gcc", "-std=c99", "-g", "-O0", *flags, "-c", str(src), "-o", str(obj)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        objs.append(str(obj))
    exe = tmp_path / "drv"
    subprocess.run(["gcc", "-o", str(exe), *objs], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "checks passed" in r.stdout and int(r.stdout.split()[4]) > 100


def test_integration_lists_the_sparse_binding():
    txt = (ROOT / "INTEGRATION.md").read_text()
    assert "oem_shim_logistic_sparse.c" in txt and "src/oem_logistic_sparse.cpp" in txt


def test_predict_sparse_newx():
    from oem_amd import api
    fit = api.OemFitBinomial(beta=[np.array([[0.5, -1.0], [1.0, 2.0], [0.0, -0.5]])], **{"lambda": [np.array([0.2, 0.1])]},
                             loss=[np.array([30.0, 25.5])], family="binomial", penalty=["lasso"], nobs=50, nvars=2)
    newx = np.array([[1.0, 2.0], [-1.0, 0.0], [0.0, 3.0]])
    for m in (sp.csc_matrix(newx), sp.csr_matrix(newx), sp.coo_matrix(newx)):
        np.testing.assert_allclose(api.predict(fit, m), api.predict(fit, newx), rtol=0, atol=1e-15)
        np.testing.assert_allclose(api.predict(fit, m, type="response"), api.predict(fit, newx, type="response"), rtol=0, atol=1e-15)
        assert np.array_equal(api.predict(fit, m, type="class"), api.predict(fit, newx, type="class"))
        assert np.array_equal(api.predict(fit, m, s=0.15), api.predict(fit, newx, s=0.15))
