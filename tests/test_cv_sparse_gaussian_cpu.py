"""cv.oem(family = "gaussian") on a resident sparse x, the part that needs no GPU: the exports, the host plan
(oemgpu_selftest_cv_sparse_plan -- the function the entries take their layout from) over a sweep of shapes, and the refusals of
oemgpu_cv_sparse_fold_fits_res / oemgpu_cv_sparse_score_res / oemgpu_selftest_cv_sparse_score that come back before a device is
looked for.

The plan is checked for what the scoring kernel and the buffers rely on:
  * the per-fold wave partials [K][waves][npen][nl16][4] are K waves npen nl16 32 bytes and stay under 64 MB, with at least one
    workgroup of four waves, and the lambda blocks cover nl;
  * the device bytes are the xval layout + the sparse fold plan + this route's own regions, the last written out term by term, and
    the fold plan is xval.oem's sparse plan less the five upload regions (the handle holds the columns, the caller y and foldid);
  * the route is the rule of oemgpu_fit_sparse, and both routes occur.
"""
import ctypes as C

import numpy as np
import pytest

CH = 8192
PART_MAX = 64 * 10 ** 6


@pytest.fixture(scope="module")
def api():
    from oem_amd import api
    return api


def _lib():
    import oem_amd
    return oem_amd.lib()


def _r256(b):
    return -(-b // 256) * 256


def test_exports(api):
    from oem_amd import _lib as B
    L = _lib()
    for name in ("oemgpu_cv_sparse_fold_fits_res", "oemgpu_cv_sparse_score_res", "oemgpu_selftest_cv_sparse_score",
                 "oemgpu_selftest_cv_sparse_plan"):
        assert name in B.EXPORTS and hasattr(L, name)
    header = open(__file__.rsplit("/tests/", 1)[0] + "/include/oemgpu.h").read()
    for name in ("oemgpu_cv_sparse_fold_fits_res", "oemgpu_cv_sparse_score_res", "oemgpu_selftest_cv_sparse_score",
                 "oemgpu_selftest_cv_sparse_plan"):
        assert ("int " + name + "(") in header
    assert callable(api.cv_sparse_gaussian_score) and callable(api.cv_sparse_plan)
    assert "oemgpu_sparse_x_bytes" in B.EXPORTS and L.oemgpu_sparse_x_bytes(None) == 0


def _route_rule(n, p, nnz):
    return (CH * 8 + 16 * p + 64 <= 160 * 1024) and nnz <= 0.02 * n * p and n < 2 ** 31


def test_plan_sweep(api):
    seen, capped = set(), 0
    for n in (600, 8192, 24577, 250_000, 3_000_000):
        for p in (2, 41, 200, 2000):
            if p >= n:
                continue
            for dens in (0.001, 0.01, 0.1):
                nnz = int(dens * n * p)
                for K in (2, 3, 10, 130, 512):
                    for nl in (1, 64, 65, 100):
                        for cu, npen in ((64, 1), (256, 2), (304, 1)):
                            d = api.cv_sparse_plan(n, p, nnz, K, npen, nl, cu)
                            tag = (n, p, nnz, K, nl, cu, npen)
                            nl16 = -(-nl // 16) * 16
                            assert d["csc"] == _route_rule(n, p, nnz), tag
                            seen.add(d["csc"])
                            # ---- the scoring launch and its partials
                            assert d["nl16"] == nl16 and d["lblk"] == -(-nl // 64) and d["lblk"] * 64 >= nl16, tag
                            assert d["nwg"] >= 1 and d["waves"] == 4 * d["nwg"], tag
                            assert d["part_bytes"] == K * d["waves"] * npen * nl16 * 32, tag
                            assert d["part_bytes"] <= PART_MAX, tag
                            # what the launch would be without the bound on the partials: four workgroups per CU over (penalty, lambda
                            # block), a wave no fewer than 16 rows, at most 1024
                            free = max(1, min(cu * 4 // (npen * d["lblk"]), -(-n // 64), 1024))
                            assert d["nwg"] <= free, tag
                            if d["nwg"] < free:                     # lowered by the bound alone, and not further than it asks
                                capped += 1
                                assert K * 4 * (d["nwg"] + 1) * npen * nl16 * 32 > PART_MAX, tag
                            # ---- the device bytes, term by term
                            assert d["align"] == CH and d["rows_max"] == (n // CH + K) * CH, tag
                            own = (_r256(d["part_bytes"]) + _r256(24 * K * npen * nl) + _r256(4 * npen) + _r256(4 * d["rows_max"])
                                   + _r256(8 * p))
                            assert d["own_bytes"] == own, tag
                            assert d["bytes"] == d["xval_bytes"] + d["fold_bytes"] + d["own_bytes"], tag
                            x = api.xval_sparse_plan(n, p, nnz, K, npen, nl, cu)
                            upload = _r256(8 * (p + 1)) + _r256(4 * (nnz + 1)) + _r256(8 * (nnz + 1)) + _r256(8 * n) + _r256(4 * n)
                            assert x["bytes"] - upload == d["xval_bytes"] + d["fold_bytes"], tag
    assert seen == {True, False}
    assert capped > 0
    # K = 512 at 100 lambdas: the bound leaves 8 workgroups (32 waves) to one penalty, 4 to two
    assert api.cv_sparse_plan(3_000_000, 200, 6_000_000, 512, 1, 100, 256)["nwg"] == 8
    assert api.cv_sparse_plan(3_000_000, 200, 6_000_000, 512, 2, 100, 256)["nwg"] == 4
    # never less than one workgroup: eight penalties still fit the bound with it, nine (512 x 9 x 112 > 500,000) are the one case beyond
    d8, d9 = (api.cv_sparse_plan(3_000_000, 200, 6_000_000, 512, m, 100, 256) for m in (8, 9))
    assert d8["nwg"] == 1 and d8["part_bytes"] <= PART_MAX
    assert d9["nwg"] == 1 and d9["waves"] == 4 and d9["part_bytes"] == 512 * 4 * 9 * 112 * 32


def test_plan_refusals():
    L = _lib()
    out = (C.c_int64 * 12)()
    assert L.oemgpu_selftest_cv_sparse_plan(1000, 5, 50, 5, 1, 10, 256, out) == 0
    for args in ((0, 5, 50, 5, 1, 10, 256), (1000, 0, 50, 5, 1, 10, 256), (1000, 5, -1, 5, 1, 10, 256), (1000, 5, 50, 5, 0, 10, 256),
                 (1000, 5, 50, 5, 1, 0, 256), (1000, 5, 50, 5, 1, 10, 0), (1000, 5, 50, 1, 1, 10, 256), (1000, 5, 50, 513, 1, 10, 256)):
        assert L.oemgpu_selftest_cv_sparse_plan(*args, out) == -1, args
    assert L.oemgpu_selftest_cv_sparse_plan(1000, 5, 50, 5, 1, 10, 256, None) == -1
    # 32-bit row positions: n + 8192 K must stay below 2^31
    assert L.oemgpu_selftest_cv_sparse_plan(2 ** 31 - CH * 5, 5, 50, 5, 1, 10, 256, out) == -4
    assert b"32-bit" in L.oemgpu_last_error()
    assert L.oemgpu_selftest_cv_sparse_plan(2 ** 31 - CH * 5 - 1, 5, 50, 5, 1, 10, 256, out) == 0


# ---------------------------------------------------------------------------------------- refusals before any device
class _Handle(C.Structure):
    """the leading fields of struct oemgpu_sparse_x (oem_amd/csrc/logistic.hpp), all that the checks in front of the device read"""
    _fields_ = [("device", C.c_int), ("n", C.c_int64), ("nnz", C.c_int64), ("maxcol", C.c_int64), ("p", C.c_int32), ("rest", C.c_void_p * 9)]


def _opts(p, npen=1, nlambda=5):
    from oem_amd import api
    return api._Args(["lasso"] * npen, [], nlambda, 1e-4, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(p), np.zeros(0, np.int32),
                     np.zeros(0, np.int32), np.zeros(0))


def test_fold_fits_refusals_before_any_device():
    """NULL pointers and nfolds outside 2..512: -1; 32-bit row positions and n - ceil(n / K) <= p: -4 -- the context and the device
    pointers are never looked at (they point at host scratch here), the handle's arrays neither"""
    L = _lib()
    scratch = (C.c_double * 64)()
    ptr = C.addressof(scratch)
    dp = C.cast(scratch, C.POINTER(C.c_double))
    ip = C.cast(scratch, C.POINTER(C.c_int32))
    lp = C.cast(scratch, C.POINTER(C.c_int64))
    a = _opts(4)
    h = _Handle(device=0, n=50, nnz=20, maxcol=5, p=4)
    hp = C.addressof(h)

    def call(ctx=ptr, x=hp, y=ptr, fid=ptr, K=5, o=C.byref(a.c), beta=dp, lam=dp, niter=ip, loss=dp, d=dp, fn=lp):
        return L.oemgpu_cv_sparse_fold_fits_res(ctx, x, y, fid, K, 1, 1, o, beta, lam, niter, loss, d, fn)
    for kw in (dict(ctx=None), dict(x=None), dict(y=None), dict(fid=None), dict(o=None), dict(beta=None), dict(lam=None), dict(niter=None),
               dict(loss=None), dict(d=None), dict(fn=None)):
        assert call(**kw) == -1, kw
        assert b"NULL" in L.oemgpu_last_error()
    for K in (1, 513, 0, -2):
        assert call(K=K) == -1
        assert b"nfolds" in L.oemgpu_last_error()
    big = _Handle(device=0, n=2 ** 31 - CH * 5, nnz=20, maxcol=5, p=4)
    assert call(x=C.addressof(big)) == -4
    assert b"32-bit" in L.oemgpu_last_error()
    # 50 rows in 5 folds: the largest fold holds >= 10, so at most 40 are kept -- p = 40 is refused before the device
    a40 = _opts(40)
    h40 = _Handle(device=0, n=50, nnz=20, maxcol=5, p=40)
    assert call(x=C.addressof(h40), o=C.byref(a40.c)) == -4
    assert b"no more rows than" in L.oemgpu_last_error()
    # the options: q = p + intercept coordinates -- a group vector of p entries with an intercept is refused
    g = _opts(4)
    g.groups = np.arange(1, 5, dtype=np.int32); g.c.groups = g.groups.ctypes.data_as(C.POINTER(C.c_int32)); g.c.ngroupvars = 4
    g.ug = np.arange(1, 5, dtype=np.int32); g.c.unique_groups = g.ug.ctypes.data_as(C.POINTER(C.c_int32)); g.c.ngroups = 4
    from oem_amd import api
    g.pen[0] = api.PENALTIES.index("grp.lasso")
    assert call(o=C.byref(g.c)) == -1
    assert b"groups must have same length" in L.oemgpu_last_error()


def test_score_refusals_before_any_device():
    L = _lib()
    scratch = (C.c_double * 64)()
    ptr = C.addressof(scratch)
    dp = C.cast(scratch, C.POINTER(C.c_double))
    ncol = (C.c_int32 * 2)(3, 3)

    def call(ctx=ptr, n=50, p=4, K=5, coef=dp, npen=2, nl=3, nc=ncol, tm=0, tri=dp, pm=None):
        return L.oemgpu_cv_sparse_score_res(ctx, n, p, K, coef, npen, nl, nc, tm, tri, pm)
    for kw in (dict(ctx=None), dict(coef=None), dict(nc=None), dict(tri=None)):
        assert call(**kw) == -1, kw
        assert b"NULL" in L.oemgpu_last_error()
    for kw in (dict(p=0), dict(npen=0), dict(nl=0), dict(n=0), dict(tm=2), dict(tm=-1)):
        assert call(**kw) == -1, kw
    for K in (1, 513):
        assert call(K=K) == -1
        assert b"nfolds" in L.oemgpu_last_error()
    for bad in ((4, 3), (3, -1)):
        assert call(nc=(C.c_int32 * 2)(*bad)) == -1
        assert b"ncol" in L.oemgpu_last_error()
    assert call(n=2 ** 31 - CH * 5) == -4
    # the selftest: the same checks, on the handle's shape
    h = _Handle(device=0, n=50, nnz=20, maxcol=5, p=4)
    hp = C.addressof(h)

    def st(ctx=ptr, x=hp, y=ptr, fid=ptr, K=5, coef=dp, npen=2, nl=3, nc=ncol, tm=0, tri=dp):
        return L.oemgpu_selftest_cv_sparse_score(ctx, x, y, fid, K, coef, npen, nl, nc, tm, tri, None)
    for kw in (dict(ctx=None), dict(x=None), dict(y=None), dict(fid=None), dict(coef=None), dict(nc=None), dict(tri=None)):
        assert st(**kw) == -1, kw
        assert b"NULL" in L.oemgpu_last_error()
    for kw in (dict(K=1), dict(K=513), dict(npen=0), dict(nl=0), dict(tm=2), dict(nc=(C.c_int32 * 2)(4, 3))):
        assert st(**kw) == -1, kw
