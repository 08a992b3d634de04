"""cv.oem for binomial fits on a sparse x, the part that needs no GPU: the resident-x entries are declared, exported and bound; their
argument errors come back before a device is looked for (the context, the handle and the device pointers point at zeroed host scratch
here and are never followed by the checks under test); the workspace of a fit on a resident x is the plain sparse fit's less exactly the
pieces the handle and the caller hold; and cv_oem makes its checks of a sparse x without a device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = Path(__file__).resolve().parent.parent
NEW = ("oemgpu_fit_logistic_sparse_fold_res", "oemgpu_logistic_cv_score_sparse_res", "oemgpu_selftest_logistic_sparse_res_plan",
       "oemgpu_sparse_x_create", "oemgpu_sparse_x_destroy")


def test_new_symbols_are_declared_exported_and_bound():
    import oem_amd
    h = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "oemgpu.h").read_text(), flags=re.S)
    L = oem_amd.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, h), name
        assert hasattr(L, name), name
        assert name in oem_amd.EXPORTS, name
    assert re.search(r"typedef\s+struct\s+oemgpu_sparse_x\s+oemgpu_sparse_x\s*;", h)
    assert oem_amd.SparseX.__name__ in oem_amd.__all__


def _opts(p, nlambda=5):
    from oem_amd import api
    return api._Args(["lasso"], [], nlambda, 1e-4, 1.0, 3.0, 0.5, 1e-7, 500, False, False, np.ones(p), np.zeros(0, np.int32),
                     np.zeros(0, np.int32), np.zeros(0))


def _csc(n=50, p=5, seed=0, density=0.3):
    x = sp.random(n, p, density=density, format="csc", random_state=np.random.default_rng(seed))
    return (np.ascontiguousarray(x.indptr, np.int64), np.ascontiguousarray(x.indices, np.int32), np.ascontiguousarray(x.data, np.float64))


def test_create_refuses_before_any_device_with_the_fits_sentences():
    """the compressed-column checks are csc_check's, in create's name; the context is host scratch and is never followed"""
    import oem_amd
    from oem_amd import api
    L = oem_amd.lib()
    scratch = (C.c_double * 64)()
    ctx = C.addressof(scratch)
    n, p = 50, 5
    cp, ri, va = _csc(n, p)
    assert np.any(np.diff(cp) >= 2)

    def call(ctx_, n_, p_, cp_, ri_, va_):
        h = C.c_void_p(12345)
        rc = L.oemgpu_sparse_x_create(ctx_, n_, p_, None if cp_ is None else cp_.ctypes.data, api._iptr(ri_), api._dptr(va_), C.byref(h))
        assert rc != 0 and not h.value                          # a refused create leaves a NULL handle behind
        return rc, L.oemgpu_last_error().decode()
    assert call(None, n, p, cp, ri, va)[0] == -1
    assert call(ctx, n, p, None, ri, va)[0] == -1
    assert L.oemgpu_sparse_x_create(ctx, n, p, cp.ctypes.data, api._iptr(ri), api._dptr(va), None) == -1
    assert call(ctx, 0, p, cp, ri, va)[0] == -1
    assert call(ctx, n, 0, cp, ri, va)[0] == -1
    bad = cp.copy(); bad[0] = 1
    assert call(ctx, n, p, bad, ri, va) == (-1, "sparse_x_create: colptr[0] must be 0")
    bad = cp.copy(); bad[2] = bad[3] + 1
    assert call(ctx, n, p, bad, ri, va) == (-1, "sparse_x_create: colptr must be non-decreasing")
    for v in (-1, n, 2 ** 31 - 1):
        r2 = ri.copy(); r2[3] = v
        rc, msg = call(ctx, n, p, cp, r2, va)
        assert rc == -1 and "outside [0, n)" in msg
    c0 = int(np.argmax(np.diff(cp) >= 2))
    r2 = ri.copy(); r2[cp[c0] + 1] = r2[cp[c0]]
    rc, msg = call(ctx, n, p, cp, r2, va)
    assert rc == -1 and msg == "sparse_x_create: row indices of column %d are not strictly increasing" % c0
    rc, msg = call(ctx, n, p, cp, None, None)
    assert rc == -1 and msg == "sparse_x_create: NULL row indices or values"
    L.oemgpu_sparse_x_destroy(None)                             # destroy accepts NULL


def test_fold_entry_argument_errors_before_any_device():
    import oem_amd
    L = oem_amd.lib()
    p = 4
    a = _opts(p)
    out = a.outputs(p + 1)
    scratch = (C.c_double * 64)()
    ptr = C.addressof(scratch)

    def call(ctx=ptr, x=ptr, y=ptr, foldid=ptr, nfolds=5, leave_out=1, standardize=1, intercept=1):
        return L.oemgpu_fit_logistic_sparse_fold_res(ctx, x, y, foldid, nfolds, leave_out, standardize, intercept, 100, 1e-3, C.byref(a.c), *out)
    for kw in (dict(ctx=None), dict(x=None), dict(y=None)):
        assert call(**kw) == -1
        assert b"NULL" in L.oemgpu_last_error()
    assert call(nfolds=2) == -1
    assert b"nfolds" in L.oemgpu_last_error()
    assert call(leave_out=-1) == -1
    assert call(leave_out=6) == -1
    assert b"leave_out" in L.oemgpu_last_error()
    assert call(foldid=None, leave_out=1) == -1                 # (leave_out = 0 may come without fold ids)
    assert b"foldid" in L.oemgpu_last_error()


def test_score_entry_argument_errors_before_any_device():
    import oem_amd
    L = oem_amd.lib()
    scratch = (C.c_double * 64)()
    ptr = C.addressof(scratch)
    dp = C.cast(scratch, C.POINTER(C.c_double))
    cnt = (C.c_int64 * 8)()
    assert L.oemgpu_logistic_cv_score_sparse_res(ptr, None, ptr, 1.0, ptr, 5, dp, 3, dp, cnt, None) == -1
    assert L.oemgpu_logistic_cv_score_sparse_res(None, ptr, ptr, 1.0, ptr, 5, dp, 3, dp, cnt, None) == -1
    assert L.oemgpu_logistic_cv_score_sparse_res(ptr, ptr, ptr, 1.0, None, 5, dp, 3, dp, cnt, None) == -1
    assert L.oemgpu_logistic_cv_score_sparse_res(ptr, ptr, ptr, 1.0, ptr, 2, dp, 3, dp, cnt, None) == -1
    assert L.oemgpu_logistic_cv_score_sparse_res(ptr, ptr, ptr, 1.0, ptr, 5, dp, 0, dp, cnt, None) == -1


def _r256(b):
    return (b + 255) // 256 * 256


def test_resident_workspace_is_the_fits_less_the_resident_pieces():
    """both routes, one and several row-pass workgroups, nnz = 0: out[2] drops by the 256-byte granules of colptr, rowidx, values, y,
    the row pointers, the row copy's columns and values and the chunk pointers; nothing else of the plan moves"""
    import oem_amd
    L = oem_amd.lib()
    a, b = (C.c_int64 * 8)(), (C.c_int64 * 8)()
    routes = set()
    for n in (64, 100, 9000, 2 * 10 ** 5, 10 ** 6, 3 * 10 ** 9):
        for p in (3, 40, 200, 1000, 6200, 8191):
            if p + 1 >= n:
                continue
            for dens in (0.0, 0.005, 0.05, 0.3):
                nnz = int(dens * n * p)
                for icpt in (0, 1):
                    for num_cu in (64, 256):
                        assert L.oemgpu_selftest_logistic_sparse_plan(n, p, nnz, icpt, num_cu, a) == 0
                        assert L.oemgpu_selftest_logistic_sparse_res_plan(n, p, nnz, icpt, num_cu, b) == 0
                        A, B = list(a), list(b)
                        chunks = A[7]
                        resident = (_r256(8 * (p + 1)) + 2 * _r256(4 * (nnz + 1)) + 2 * _r256(8 * (nnz + 1)) + _r256(8 * n) + _r256(8 * (n + 1)) +
                                    _r256(4 * (chunks + 1) * p))
                        assert A[2] - B[2] == resident, (n, p, nnz, A, B)
                        assert A[:2] + A[3:] == B[:2] + B[3:]
                        assert 0 < B[2] <= B[3]
                        routes.add(A[0])
    assert routes == {0, 1}
    assert L.oemgpu_selftest_logistic_sparse_res_plan(0, 5, 10, 0, 256, b) == -1
    assert L.oemgpu_selftest_logistic_sparse_res_plan(100, 5, 10, 0, 256, None) == -1


def test_cv_oem_checks_a_sparse_x_without_a_device():
    import oem_amd
    rng = np.random.default_rng(3)
    x = sp.random(60, 4, density=0.5, format="csr", random_state=rng)
    y = (rng.uniform(size=60) < 0.5).astype(np.float64)
    with pytest.raises(ValueError, match="sparse x is served for family = \"binomial\" only"):
        oem_amd.cv_oem(x, y, family="gaussian", nfolds=5)
    with pytest.raises(ValueError, match="sparse x is served for family = \"binomial\" only"):
        oem_amd.cv_oem(x.tocsc(), y, nfolds=5)
    with pytest.raises(oem_amd.OemgpuError, match="weights not implemented yet."):
        oem_amd.cv_oem(x, y, family="binomial", weights=np.ones(60))
    with pytest.raises(ValueError, match="y must be a binary outcome"):
        oem_amd.cv_oem(x, rng.integers(0, 3, size=60).astype(np.float64), family="binomial", nfolds=5)
    with pytest.raises(TypeError):
        oem_amd.SparseX(x.toarray())
