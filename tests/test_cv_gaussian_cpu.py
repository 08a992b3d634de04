"""cv.oem(family = "gaussian") on a resident x, the part that needs no GPU: the restatement (tests/cv_gaussian_restatement.py) against
hand-computed figures, the host-side packing of the coefficient table against predict(..., s = ...), the refusals of
oemgpu_cv_fold_fits_dev / oemgpu_cv_score_dev that come back before a device is looked for, and the exports."""
import ctypes as C

import numpy as np

from tests import cv_gaussian_restatement as R


def _lib():
    import oem_amd
    return oem_amd.lib()


# ---------------------------------------------------------------------------------------- the restatement
# 12 rows in 3 folds of 5, 4 and 3; two columns, the second one not valid for fold 3 (nlams = 2, 2, 1) and NaN there
Y = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0])
FOLD = np.array([1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3])
PRED = np.column_stack([Y - np.array([1, -1, 2, -2, 0, 1, 1, -1, -1, 3, 0, -3.0]),
                        Y - np.array([2, 2, -2, -2, 0, 1, -1, 0, 0, 0, 0, 0.0])])
PRED[9:, 1] = np.nan


def test_restatement_grouped_by_hand():
    """mse.  Column 0: fold means 10/5, 4/4, 18/3 = 2, 1, 6; cvm = (5*2 + 4*1 + 3*6)/12 = 32/12; cvsd^2 = (5*(2/3)^2 + 4*(5/3)^2 + 3*(10/3)^2)
    / 12 / (3 - 1).  Column 1: fold means 16/5, 2/4 over folds 1 and 2 only, N = 2: cvm = 18/9 = 2, cvsd^2 = (5*1.2^2 + 4*1.5^2)/9/1."""
    cvm, cvsd = R.cv_statistics([PRED], Y, FOLD, np.array([2, 2, 1]), "mse", True)
    assert np.allclose(cvm[0], [32.0 / 12.0, 2.0], rtol=1e-14)
    v0 = (5 * (2.0 / 3.0) ** 2 + 4 * (5.0 / 3.0) ** 2 + 3 * (10.0 / 3.0) ** 2) / 12.0 / 2.0
    v1 = (5 * 1.2 ** 2 + 4 * 1.5 ** 2) / 9.0 / 1.0
    assert np.allclose(cvsd[0], np.sqrt([v0, v1]), rtol=1e-14)
    # mae, column 0: fold means 6/5, 1, 2; cvm = 16/12
    cvm, cvsd = R.cv_statistics([PRED], Y, FOLD, np.array([2, 2, 1]), "mae", True)
    assert np.isclose(cvm[0][0], 16.0 / 12.0, rtol=1e-14)
    m = 16.0 / 12.0
    assert np.isclose(cvsd[0][0], np.sqrt((5 * (1.2 - m) ** 2 + 4 * (1 - m) ** 2 + 3 * (2 - m) ** 2) / 12.0 / 2.0), rtol=1e-14)


def test_restatement_ungrouped_by_hand():
    """mse, rows as they are.  Column 0: errors 1,1,4,4,0,1,1,1,1,9,0,9: mean 32/12, N = 12; column 1: 4,4,4,4,0,1,1,0,0 over the nine
    rows that have a prediction: mean 2, N = 9."""
    cvm, cvsd = R.cv_statistics([PRED], Y, FOLD, np.array([2, 2, 1]), "mse", False)
    e0 = np.array([1, 1, 4, 4, 0, 1, 1, 1, 1, 9, 0, 9.0]); e1 = np.array([4, 4, 4, 4, 0, 1, 1, 0, 0.0])
    assert np.allclose(cvm[0], [32.0 / 12.0, 2.0], rtol=1e-14)
    assert np.allclose(cvsd[0], [np.sqrt(np.mean((e0 - e0.mean()) ** 2) / 11.0), np.sqrt(np.mean((e1 - 2.0) ** 2) / 8.0)], rtol=1e-14)


def test_restatement_interpolation_by_hand():
    """lambda 4, 2, 1 and s = 3, 1.5, 2, 9, 0.5: halfway between the first two, halfway between the last two, on a knot, clamped at both ends"""
    left, right, frac = R.lambda_interp(np.array([4.0, 2.0, 1.0]), np.array([3.0, 1.5, 2.0, 9.0, 0.5]))
    assert left.tolist() == [0, 1, 1, 0, 2] and right.tolist() == [1, 2, 1, 0, 2]
    assert np.allclose(frac, [0.5, 0.5, 1.0, 1.0, 1.0], rtol=1e-15)
    fit = {"lambda": [np.array([4.0, 2.0, 1.0])], "beta": [np.array([[1.0, 2.0, 4.0], [0.0, 1.0, 3.0]])]}
    assert np.allclose(R.predict_at(fit, 0, np.array([[2.0]]), np.array([3.0, 1.5])), [1.5 + 2 * 0.5, 3.0 + 2 * 2.0])


# ---------------------------------------------------------------------------------------- the coefficient table
def test_table_packing_matches_predict():
    """_cv_gaussian_table on made-up fold fits: fold k's leading ncol columns are predict(fold k, s = the kept lambdas, "coefficients"),
    the rest stays zero, ncol counts which_lam -- and the interpolation agrees with the restatement's"""
    import oem_amd
    from oem_amd import api
    rng = np.random.default_rng(5)
    p, nl, K = 4, 6, 3
    lam_full = [np.geomspace(2.0, 0.02, nl), np.geomspace(3.0, 0.05, nl)]
    outlist = []
    for k in range(K):
        o = api.OemFit()
        o["lambda"] = [np.geomspace(2.0 + 0.1 * k, 0.02 * (1 + 0.7 * k), nl), np.geomspace(3.0, 0.05 * (1 + k), nl)]
        o["beta"] = [rng.normal(size=(p + 1, nl)), rng.normal(size=(p + 1, nl))]
        o["penalty"] = ["lasso", "mcp"]
        outlist.append(o)
    which_lam = [lam_full[m] >= max(np.min(o["lambda"][m]) for o in outlist) for m in range(2)]
    coef, ncol = api._cv_gaussian_table(outlist, lam_full, which_lam, p)
    assert coef.shape == (K, 2, nl, p + 1) and ncol.dtype == np.int32
    assert ncol.tolist() == [int(w.sum()) for w in which_lam] and 0 < ncol[0] < nl and 0 < ncol[1] < nl
    for k, o in enumerate(outlist):
        for m in range(2):
            want = oem_amd.predict(o, type="coefficients", s=lam_full[m][which_lam[m]], which_model=m)
            assert np.array_equal(coef[k, m, :ncol[m]], want.T)
            assert not coef[k, m, ncol[m]:].any()
            left, right, frac = R.lambda_interp(o["lambda"][m], lam_full[m][which_lam[m]])
            assert np.allclose(coef[k, m, :ncol[m]].T, o["beta"][m][:, left] * frac + o["beta"][m][:, right] * (1 - frac), rtol=1e-13, atol=1e-15)


def test_eligibility_needs_a_device_tensor():
    """a numpy x, whatever the folds, is the host loop's"""
    from oem_amd import api
    x = np.zeros((40, 3))
    fid = np.resize(np.arange(1, 5), 40)
    assert api._cv_gaussian_resident(x, ["lasso"], {}, fid, 4) is False


# ---------------------------------------------------------------------------------------- refusals before any device
def _opts(npen=1, nlambda=5):
    from oem_amd import api
    a = api._Args(["lasso"] * npen, [], nlambda, 1e-4, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(4), np.zeros(0, np.int32),
                  np.zeros(0, np.int32), np.zeros(0))
    return a


def test_fold_fits_refusals_before_any_device():
    """NULL pointers, nfolds outside 2..512, n < 1, ld < n: -1; 32-bit row positions and n - ceil(n / K) <= p: -4 -- the context and the
    device pointers are never looked at (they point at host scratch here)"""
    L = _lib()
    scratch = (C.c_double * 64)()
    ptr = C.addressof(scratch)
    dp = C.cast(scratch, C.POINTER(C.c_double))
    ip = C.cast(scratch, C.POINTER(C.c_int32))
    lp = C.cast(scratch, C.POINTER(C.c_int64))
    a = _opts()

    def call(ctx=ptr, x=ptr, n=50, ld=50, p=4, y=ptr, fid=ptr, K=5, o=C.byref(a.c), beta=dp, lam=dp, niter=ip, loss=dp, d=dp, fn=lp):
        return L.oemgpu_cv_fold_fits_dev(ctx, x, n, ld, p, y, fid, K, 1, 1, o, beta, lam, niter, loss, d, fn)
    for kw in (dict(ctx=None), dict(x=None), dict(y=None), dict(fid=None), dict(o=None), dict(beta=None), dict(lam=None), dict(niter=None),
               dict(loss=None), dict(d=None), dict(fn=None)):
        assert call(**kw) == -1, kw
        assert b"NULL" in L.oemgpu_last_error()
    for kw in (dict(n=0), dict(ld=49), dict(p=1)):
        assert call(**kw) == -1, kw
    for K in (1, 513, 0, -2):
        assert call(K=K) == -1
        assert b"nfolds" in L.oemgpu_last_error()
    assert call(n=2 ** 31 - 80, ld=2 ** 31 - 80) == -4
    # 50 rows in 5 folds: the largest fold holds >= 10, so at most 40 are kept -- p = 40 is refused, p = 39 is not refused HERE
    a40 = _opts()
    a40.pf = np.ones(40); a40.c.penalty_factor = a40.pf.ctypes.data_as(C.POINTER(C.c_double))
    assert L.oemgpu_cv_fold_fits_dev(ptr, ptr, 50, 50, 40, ptr, ptr, 5, 1, 1, C.byref(a40.c), dp, dp, ip, dp, dp, lp) == -4
    assert b"no more rows than" in L.oemgpu_last_error()
    assert L.oemgpu_cv_fold_fits_dev(ptr, ptr, 7, 7, 5, ptr, ptr, 3, 1, 1, C.byref(a40.c), dp, dp, ip, dp, dp, lp) == -4      # 7 - 3 = 4 <= 5


def test_score_refusals_before_any_device():
    L = _lib()
    scratch = (C.c_double * 64)()
    ptr = C.addressof(scratch)
    dp = C.cast(scratch, C.POINTER(C.c_double))
    ncol = (C.c_int32 * 2)(3, 3)

    def call(ctx=ptr, n=50, p=4, K=5, coef=dp, npen=2, nl=3, nc=ncol, tm=0, tri=dp, pm=None):
        return L.oemgpu_cv_score_dev(ctx, n, p, K, coef, npen, nl, nc, tm, tri, pm)
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
    assert L.oemgpu_selftest_cv_score_dev(None, ptr, 50, 50, 4, ptr, ptr, 5, dp, 2, 3, ncol, 0, dp, None) == -1
    assert L.oemgpu_selftest_cv_score_dev(ptr, ptr, 50, 49, 4, ptr, ptr, 5, dp, 2, 3, ncol, 0, dp, None) == -1


def test_exports():
    from oem_amd import _lib as B
    from oem_amd import api
    L = _lib()
    for name in ("oemgpu_cv_fold_fits_dev", "oemgpu_cv_score_dev", "oemgpu_selftest_cv_score_dev"):
        assert name in B.EXPORTS and hasattr(L, name)
    assert callable(api.cv_gaussian_score)
