"""cv.oem(family = "gaussian") on a resident x.

A. oemgpu_cv_score_dev alone (through oemgpu_selftest_cv_score_dev: the fold layout, then the entry as it is) against numpy in long
   double on DENSE RANDOM tables -- fitted tables are mostly zeros and nearly equal across folds, which hides dropped chunks and
   swapped indices -- in every form of the launch plan, with folds of 1, 17 and 2822 rows and an absent one, the fewest and many
   folds, ld > n, two penalties with different numbers of valid columns, one valid column and none, mse and mae.  Counts are exact;
   the per-fold mean is held to rtol 1e-12 and M2 to 1e-11, the figures tests/test_gpu_xval_bounds.py holds the same product to (the
   per-fold finish changes only the order of the merge); a prediction to the bound of a dot product of p + 1 terms in float64,
   4 (p + 2) eps sum |x_j b_j|.
B. oemgpu_cv_fold_fits_dev against oracle.fit_dense on the gathered kept rows: lambda rtol 1e-11, d 1e-11, beta 1e-8 max(1, |beta|_inf)
   (the figures of tests/test_gpu_xval.py::_compare), also on columns offset by 1e5, where moments about 0 lose 2e-5.
C. cv_oem on a device tensor against tests/cv_gaussian_restatement.py: cvm rtol 1e-9, cvsd 1e-8, fit.preval 1e-8 scale, the same
   lambda.min and best.model; the calls that are not eligible still take the host loop."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import cv_gaussian_restatement as R

pytestmark = pytest.mark.gpu

LD = np.longdouble
RTOL_M, RTOL_S = 1e-12, 1e-11
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def api():
    from oem_amd import api
    return api


@pytest.fixture(scope="module")
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(x, y, fid, pad=0):
    """x, y, foldid on the device; pad > 0: x is a view of a taller column-major buffer (ld = n + pad) whose spare rows are NaN"""
    import torch
    n, p = x.shape
    buf = torch.full((p, n + pad), float("nan"), dtype=torch.float64, device="cuda:0")
    xd = buf.t()[:n]
    xd.copy_(torch.as_tensor(np.ascontiguousarray(x)))
    assert xd.stride() == (1, n + pad)
    return (xd, torch.as_tensor(np.asarray(y, dtype=np.float64), device="cuda:0"),
            torch.as_tensor(np.ascontiguousarray(fid, dtype=np.int32), device="cuda:0"))


# ------------------------------------------------------------------------------------------------------------- A: the scoring entry
def _score_reference(x, y, fid, coef, ncol, measure):
    """triples[K][npen][nl][3] in long double ((0, NaN, NaN) where the entry must say so), yhat[npen][nl][n] and its bound in float64"""
    K, npen, nl, _ = coef.shape
    n = len(y)
    tri = np.full((K, npen, nl, 3), np.nan, dtype=LD)
    tri[..., 0] = 0
    pred = np.full((npen, nl, n), np.nan)
    bound = np.zeros((npen, nl, n))
    xx, yy = x.astype(LD), y.astype(LD)
    for k in range(K):
        rows = np.nonzero(fid == k + 1)[0]
        if len(rows) == 0:
            continue
        b = coef[k].astype(LD)
        yh = b[..., :1] + b[..., 1:] @ xx[rows].T                                      # [npen, nl, rows]
        res = yy[rows] - yh
        v = res * res if measure == "mse" else np.abs(res)
        m = v.mean(axis=-1)
        m2 = ((v - m[..., None]) ** 2).sum(axis=-1)
        mag = np.abs(coef[k][..., :1]) + np.abs(coef[k][..., 1:]) @ np.abs(x[rows]).T
        for pen in range(npen):
            c = ncol[pen]
            tri[k, pen, :c, 0] = len(rows); tri[k, pen, :c, 1] = m[pen, :c]; tri[k, pen, :c, 2] = m2[pen, :c]
            pred[pen, :c, rows] = yh[pen, :c].astype(np.float64).T
            bound[pen, :c, rows] = mag[pen, :c].T
    return tri, pred, 4.0 * (x.shape[1] + 2) * EPS * bound


def _check_score(api, x, y, fid, K, coef, ncol, measure, label, pad=0):
    xd, yd, fd = _dev(x, y, fid, pad)
    tri, pm = api.cv_gaussian_score(xd, yd, fd, K, coef, ncol, type_measure=measure, predmat=True)
    ref, pref, pbound = _score_reference(x, y, fid, coef, ncol, measure)
    some = ref[..., 0] > 0
    assert np.array_equal(tri[..., 0], ref[..., 0].astype(np.float64)), label                       # counts, zero where masked or empty
    assert np.all(np.isnan(tri[..., 1][~some])) and np.all(np.isnan(tri[..., 2][~some])), label
    gm = float(np.max(np.abs(tri[..., 1][some].astype(LD) - ref[..., 1][some]) / np.abs(ref[..., 1][some]))) if some.any() else 0.0
    many = ref[..., 0] > 1
    gs = float(np.max(np.abs(tri[..., 2][many].astype(LD) - ref[..., 2][many]) / ref[..., 2][many])) if many.any() else 0.0
    print(f"GAP {label}: fold mean {gm:.1e} fold M2 {gs:.1e}")
    assert np.all(tri[..., 2][some & ~many] == 0.0), label                                           # one row: no spread
    assert gm <= RTOL_M, (label, gm)
    assert gs <= RTOL_S, (label, gs)
    assert np.array_equal(np.isnan(pm), np.isnan(pref)), label                                       # NaN exactly in the masked columns
    ok = ~np.isnan(pref)
    gp = float(np.max(np.abs(pm[ok] - pref[ok]) / np.maximum(pbound[ok], 1e-300))) if ok.any() else 0.0
    print(f"GAP {label}: yhat {gp:.2f} of its bound")
    assert gp <= 1.0, (label, gp)
    tri2, pm2 = api.cv_gaussian_score(xd, yd, fd, K, coef, ncol, type_measure=measure, predmat=True)     # the same call: the same bits
    assert np.array_equal(tri, tri2, equal_nan=True) and np.array_equal(pm, pm2, equal_nan=True), label
    tri3, none = api.cv_gaussian_score(xd, yd, fd, K, coef, ncol, type_measure=measure)                # and without the prediction store
    assert none is None and np.array_equal(tri, tri3, equal_nan=True), label


def _table(seed, K, npen, nl, p):
    return np.random.default_rng(seed).normal(size=(K, npen, nl, p + 1)) / np.sqrt(p + 1.0)


FORMS = [(23, 21, "single", 2, 1), (60, 20, "multi", 2, 1), (170, 112, "chunk", 7, 1), (10, 250, "single", 6, 3)]


@pytest.mark.parametrize("measure", ["mse", "mae"])
@pytest.mark.parametrize("p,nl,form,lt,passes", FORMS, ids=[f"p{f[0]}-nl{f[1]}" for f in FORMS])
def test_score_forms(api, num_cu, p, nl, form, lt, passes, measure):
    """one case per form of cv_error_plan (p = 170 at 112 lambdas: two coefficient chunks; 250 lambdas: three passes), three random folds
    of 235 / 234 / 234 rows -- no multiple of 16 -- two penalties, the second with three columns fewer"""
    n, K = 703, 3
    P = api.xval_cv_plan(n, p, K, 2, nl, num_cu)
    assert (P["form"], P["lt"], P["passes"]) == (form, lt, passes), P
    if form == "chunk":
        assert P["chunks"] == 2
    rng = np.random.default_rng(1000 * p + nl)
    x = np.asfortranarray(rng.normal(size=(n, p)) + 0.1)
    y = rng.normal(size=n) + 0.3
    fid = rng.permutation(np.resize(np.arange(1, K + 1), n))
    _check_score(api, x, y, fid, K, _table(7 * p + nl, K, 2, nl, p), [nl, nl - 3], measure, f"{form} p={p} nl={nl} {measure}")


@pytest.mark.parametrize("p,nl", [(23, 21), (170, 112)], ids=["single", "chunk"])
def test_score_fold_sizes_and_leading_dimension(api, p, nl):
    """folds of 1, 17 and 2822 rows and an id that never occurs; the long fold takes several rounds of row tiles with a partial last one
    (in CHUNK form its idle waves still meet the staging barriers); x is a view with ld = n + 37 whose spare rows are NaN"""
    K = 4
    fid = np.random.default_rng(31).permutation(np.concatenate([np.full(1, 1), np.full(17, 2), np.full(2822, 4)]))
    n = len(fid)
    rng = np.random.default_rng(77 + p)
    x = np.asfortranarray(rng.normal(size=(n, p)) + 0.1)
    y = rng.normal(size=n) + 0.3
    for measure in ("mse", "mae"):
        _check_score(api, x, y, fid, K, _table(5 * p + nl, K, 1, nl, p), [nl], measure, f"fold sizes p={p} {measure}", pad=37)


@pytest.mark.parametrize("K,n", [(2, 703), (130, 1500)])
def test_score_fewest_and_many_folds(api, K, n):
    """K = 2; K = 130 with two penalties: more (fold, penalty) pairs than CUs, one workgroup each, folds of 11 or 12 rows"""
    p, nl = 23, 21
    rng = np.random.default_rng(600 + K)
    x = np.asfortranarray(rng.normal(size=(n, p)) + 0.1)
    y = rng.normal(size=n) + 0.3
    fid = rng.permutation(np.resize(np.arange(1, K + 1), n))
    _check_score(api, x, y, fid, K, _table(K, K, 2, nl, p), [nl, nl - 3], "mse", f"K={K}")


def test_score_one_valid_column_and_none(api):
    p, nl, n, K = 23, 21, 703, 3
    rng = np.random.default_rng(9)
    x = np.asfortranarray(rng.normal(size=(n, p)) + 0.1)
    y = rng.normal(size=n) + 0.3
    fid = rng.permutation(np.resize(np.arange(1, K + 1), n))
    _check_score(api, x, y, fid, K, _table(3, K, 2, nl, p), [1, 0], "mae", "ncol = (1, 0)")


def test_score_needs_the_layout(api):
    """the scoring entry on a context whose fold layout is another shape's, or another call's: refused, nothing read"""
    import ctypes as C
    import oem_amd
    rng = np.random.default_rng(2)
    x = np.asfortranarray(rng.normal(size=(200, 5))); y = rng.normal(size=200)
    fid = np.resize(np.arange(1, 4), 200)
    xd, yd, fd = _dev(x, y, fid)
    coef = _table(1, 3, 1, 4, 5)
    api.cv_gaussian_score(xd, yd, fd, 3, coef, [4])
    tri = np.zeros((3, 1, 4, 3))
    ncol = np.array([4], dtype=np.int32)
    dp = C.POINTER(C.c_double)
    rc = oem_amd.lib().oemgpu_cv_score_dev(api.context(0), 201, 5, 3, coef.ctypes.data_as(dp), 1, 4, ncol.ctypes.data_as(C.POINTER(C.c_int32)), 0,
                                           tri.ctypes.data_as(dp), None)
    assert rc == -1 and b"oemgpu_cv_fold_fits_dev" in oem_amd.lib().oemgpu_last_error()
    # the right shape, but xval.oem's phase 3 has laid ITS rows out on the context since (same buffer, no reallocation): refused as well
    ip = C.POINTER(C.c_int32)

    def score():
        return oem_amd.lib().oemgpu_cv_score_dev(api.context(0), 200, 5, 3, coef.ctypes.data_as(dp), 1, 4, ncol.ctypes.data_as(ip), 0, tri.ctypes.data_as(dp), None)
    assert score() == 0
    api.xval_cv_error(xd, yd, fd, 3, coef)
    assert score() == -1 and b"oemgpu_cv_fold_fits_dev" in oem_amd.lib().oemgpu_last_error()


# ------------------------------------------------------------------------------------------------------------- B: the fold fits
N, P_, NF = 3001, 23, 5
GROUPS = np.arange(P_) // 4 + 1
PENS = ["lasso", "mcp", "grp.lasso"]
SEED = 11
USER_LAMBDA = [np.geomspace(1.5, 2e-3, 17), np.geomspace(1.0, 1e-3, 17), np.geomspace(2.0, 5e-3, 17)]


@functools.lru_cache(maxsize=None)
def _data(offset=False):
    rng = np.random.default_rng(SEED)
    x = np.asfortranarray(rng.normal(size=(N, P_)) * 2 + 0.3)
    y = x[:, :4] @ np.array([1.0, -1.5, 0.5, 2.0]) + rng.normal(size=N) + 0.4
    fid = rng.permutation(np.resize(np.arange(1, NF + 1), N))
    if offset:
        x = x.copy(order="F")
        x[:, [1, 7, 22]] += 1e5
    return x, y, fid


def _kw(user):
    return dict(tol=1e-10, maxit=2000, **({} if user else {"nlambda": 21}))


@functools.lru_cache(maxsize=None)
def _oracle_fits(std, icpt, user=False, offset=False):
    """(full fit, fold fits on the gathered rows), computed once per configuration and shared"""
    x, y, fid = _data(offset)
    opts = dict(penalty=PENS, standardize=std, intercept=icpt, lambda_=USER_LAMBDA if user else None, groups=GROUPS,
                unique_groups=np.unique(GROUPS), lambda_min_ratio=1e-4, **_kw(user))
    return orc.fit_dense(x, y, **opts), [orc.fit_dense(x[fid != i], y[fid != i], **opts) for i in range(1, NF + 1)]


def _fold_fits(api, std, icpt, user=False, offset=False):
    x, y, fid = _data(offset)
    xd, yd, _ = _dev(x, y, fid)
    kw = dict(standardize=std, intercept=icpt, groups=GROUPS, **_kw(user))
    return api._cv_gaussian_fold_fits(xd, yd, fid, NF, PENS, USER_LAMBDA if user else (), kw)


def _compare_fits(outlist, ref, label):
    worst = 0.0
    for i, (f, r) in enumerate(zip(outlist, ref)):
        assert abs(f["d"] - r["d"]) < 1e-11 * r["d"], (label, i)
        for k in range(len(PENS)):
            assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-11), (label, i, k)
            scale = max(1.0, float(np.abs(r["beta"][k]).max()))
            gap = float(np.abs(f["beta"][k] - r["beta"][k]).max()) / scale
            worst = max(worst, gap)
            assert gap < 1e-8, (label, i, k, gap)
    print(f"GAP {label}: beta {worst:.1e} of max(1, |beta|_inf)")


@pytest.mark.parametrize("std,icpt", [(True, True), (False, True), (True, False), (False, False)])
def test_fold_fits(api, std, icpt):
    outlist, dev = _fold_fits(api, std, icpt)
    x, y, fid = _data()
    assert dev["fold_n"].tolist() == [int((fid == i).sum()) for i in range(1, NF + 1)]
    assert [o["nobs"] for o in outlist] == [N - int((fid == i).sum()) for i in range(1, NF + 1)]
    _compare_fits(outlist, _oracle_fits(std, icpt)[1], f"standardize={std} intercept={icpt}")


def test_fold_fits_user_lambda(api):
    outlist, _ = _fold_fits(api, True, True, user=True)
    for o in outlist:
        for k in range(len(PENS)):
            assert np.array_equal(o["lambda"][k], USER_LAMBDA[k])
    _compare_fits(outlist, _oracle_fits(True, True, user=True)[1], "user lambda")


def test_fold_fits_offset_columns(api):
    """three columns + 1e5: moments about 0 lose (mean / sd)^2 eps ~ 2e-5 of the centred Gram; the shifted pass keeps the bound"""
    import oem_amd
    outlist, dev = _fold_fits(api, True, True, offset=True)
    assert oem_amd.lib().oemgpu_last_shift_in_effect(dev["ctx"]) == 1
    _compare_fits(outlist, _oracle_fits(True, True, offset=True)[1], "offset columns")


def test_fold_fits_refusals(api):
    import oem_amd
    rng = np.random.default_rng(4)
    n, p = 100, 20
    x = np.asfortranarray(rng.normal(size=(n, p))); y = rng.normal(size=n)
    fid = np.concatenate([np.full(80, 1), np.full(10, 2), np.full(10, 3)])                            # fold 1 leaves 20 rows for 20 columns
    xd, yd, _ = _dev(x, y, fid)
    with pytest.raises(oem_amd.OemgpuError, match="fold 1 leaves 20 rows") as e:
        api._cv_gaussian_fold_fits(xd, yd, fid, 3, ["lasso"], (), dict(nlambda=5))
    assert e.value.code == -4
    bad = np.resize(np.arange(1, 4), n); bad[7] = 0
    with pytest.raises(oem_amd.OemgpuError, match="foldid must hold values") as e:
        api._cv_gaussian_fold_fits(xd, yd, bad, 3, ["lasso"], (), dict(nlambda=5))
    assert e.value.code == -1


def test_fold_fits_absent_fold_is_the_full_fit(api):
    """an id in 1..K that never occurs: that fold's fit is the fit of all rows"""
    import oem_amd
    x, y, fid = _data()
    xd, yd, _ = _dev(x, y, fid)
    fid6 = np.where(fid == 5, 6, fid)                                                               # ids 1, 2, 3, 4, 6 of 6
    outlist, dev = api._cv_gaussian_fold_fits(xd, yd, fid6, 6, ["lasso"], (), dict(nlambda=21, tol=1e-10, maxit=2000))
    assert dev["fold_n"][4] == 0
    full = oem_amd.oem(xd, yd, penalty="lasso", nlambda=21, tol=1e-10, maxit=2000)
    assert np.allclose(outlist[4]["lambda"][0], full["lambda"][0], rtol=1e-13)
    assert np.abs(outlist[4]["beta"][0] - full["beta"][0]).max() < 1e-8 * max(1.0, float(np.abs(full["beta"][0]).max()))


# ------------------------------------------------------------------------------------------------------------- C: cv_oem end to end
# lasso and grp.lasso of the fits above (penalties are independent cold starts).  Not mcp: below some lambda its solution is least squares
# on the support whatever lambda is, so its cvm has a plateau at the minimum -- ties to rounding, which no route can be held to.
E2E = [0, 2]
E2E_PENS = [PENS[k] for k in E2E]


def _sub(fit):
    return {key: ([val[k] for k in E2E] if isinstance(val, list) else val) for key, val in fit.items()}


@pytest.mark.parametrize("user", [False, True], ids=["auto lambda", "user lambda"])
@pytest.mark.parametrize("measure", ["mse", "mae"])
@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "rows"])
def test_cv_oem_against_the_restatement(api, monkeypatch, grouped, measure, user):
    """cv_oem on a device tensor with keep=True; x never comes to the host.  (Auto lambda at this seed: the last of the 21 columns lies
    below the smallest lambda of some fold, so the masked column is exercised -- asserted.)"""
    import oem_amd
    import torch
    x, y, fid = _data()
    xd, yd, _ = _dev(x, y, fid)
    full, folds = _oracle_fits(True, True, user=user)
    ref = R.cv_oem(x, y, fid, E2E_PENS, type_measure=measure, grouped=grouped, fits=(_sub(full), [_sub(o) for o in folds]))
    if not user:
        assert all(int(w.sum()) == 20 for w in ref["which_lam"])
    mins = []
    for c in ref["cvm"]:                                                                            # no near-tie at the minimum
        s = np.sort(c)
        assert s[1] - s[0] > 1e-6 * s[0]
        mins.append(s[0])
    assert abs(mins[0] - mins[1]) > 1e-6 * min(mins)
    cpu = torch.Tensor.cpu

    def guarded(self, *a, **k):
        assert tuple(self.shape) != tuple(xd.shape), "x was copied to the host"
        return cpu(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", guarded)
    f = oem_amd.cv_oem(xd, yd, penalty=E2E_PENS, foldid=fid, type_measure=measure, grouped=grouped, keep=True, groups=GROUPS,
                       lambda_=[USER_LAMBDA[k] for k in E2E] if user else None, **_kw(user))
    monkeypatch.undo()
    for k in range(len(E2E)):
        assert np.allclose(f["lambda"][k], ref["lambda"][k], rtol=1e-11)
        gm = float(np.max(np.abs(f["cvm"][k] - ref["cvm"][k]) / ref["cvm"][k]))
        gs = float(np.max(np.abs(f["cvsd"][k] - ref["cvsd"][k]) / ref["cvsd"][k]))
        print(f"GAP {E2E_PENS[k]} {measure} grouped={grouped} user={user}: cvm {gm:.1e} cvsd {gs:.1e}")
        assert gm <= 1e-9 and gs <= 1e-8, (k, gm, gs)
        pv, pr = f["fit.preval"][k], ref["predmat"][k]
        assert pv.shape == pr.shape and np.array_equal(np.isnan(pv), np.isnan(pr))
        ok = ~np.isnan(pr)
        assert np.abs(pv[ok] - pr[ok]).max() < 1e-8 * max(1.0, float(np.abs(pr[ok]).max()))
    assert f["model.min"] - 1 == ref["model_min"] and f["best.model"] == E2E_PENS[ref["model_min"]]
    assert np.isclose(f["lambda.min"], ref["lambda_min"], rtol=1e-11)
    assert np.array_equal(f["foldid"], fid)
    assert set(f) == set(oem_amd.cv_oem(x[:400], y[:400], penalty=E2E_PENS, foldid=np.resize(np.arange(1, 4), 400), keep=True, groups=GROUPS, nlambda=5))


def test_ineligible_calls_take_the_host_loop(api, monkeypatch):
    """a numpy x, "ols" among the penalties, ngpus and p > n never reach the device route (its fold-fit helper is patched to raise), and a
    device tensor then gives what the host loop gives on a numpy copy of the same data; weights stay refused.  With "ols" the host loop
    itself ends in predict(), which cannot interpolate the one-column "ols" table (an IndexError, before and after this route): what is
    held is that the device tensor and the numpy copy end the same way, message included."""
    import oem_amd
    import torch

    def never(*a, **k):
        raise AssertionError("the device route was taken")
    monkeypatch.setattr(api, "_cv_gaussian_fold_fits", never)
    x, y, fid = _data()
    x, y, fid = x[:1200], y[:1200], np.resize(np.arange(1, 5), 1200)
    xd, yd, _ = _dev(x, y, fid)
    kw = dict(foldid=fid, nlambda=8, tol=1e-9)
    a = oem_amd.cv_oem(x, y, penalty="lasso", **kw)                                                  # numpy x: the host loop (its figures are pinned in tests/test_gpu_host.py and test_gpu_xval.py)

    def outcome(xx, yy):                                                                            # the result, or what the call raises
        try:
            return oem_amd.cv_oem(xx, yy, penalty=["lasso", "ols"], **kw)
        except Exception as e:                                                                      # noqa: BLE001
            return type(e), str(e)
    o1, o2 = outcome(xd, yd), outcome(x, y)                                                         # "ols" on a device tensor: the host loop on x.cpu()
    assert type(o1) is type(o2)
    if isinstance(o1, dict):
        assert np.allclose(o1["cvm"][0], o2["cvm"][0], rtol=1e-10) and np.allclose(o1["cvm"][0], a["cvm"][0], rtol=1e-10)
    else:
        assert o1 == o2
    d1 = oem_amd.cv_oem(xd, yd, penalty="lasso", ngpus=1, **kw)                                     # row shards are the host entries' option
    assert np.allclose(d1["cvm"][0], a["cvm"][0], rtol=1e-10)
    with pytest.raises(ValueError, match="weights not implemented"):
        oem_amd.cv_oem(xd, yd, penalty="lasso", weights=np.ones(len(y)), **kw)
    rng = np.random.default_rng(8)
    xw = np.asfortranarray(rng.normal(size=(300, 1500)))
    yw = xw[:, :5] @ np.ones(5) + rng.normal(size=300)
    fw = np.resize(np.arange(1, 4), 300)
    xwd = torch.as_tensor(np.ascontiguousarray(xw.T), device="cuda:0").t()
    with pytest.warns(UserWarning, match="optimized for n >> p"):
        w1 = oem_amd.cv_oem(xwd, yw, penalty="lasso", foldid=fw, nlambda=5, tol=1e-6)
    with pytest.warns(UserWarning, match="optimized for n >> p"):
        w2 = oem_amd.cv_oem(xw, yw, penalty="lasso", foldid=fw, nlambda=5, tol=1e-6)
    assert np.allclose(w1["cvm"][0], w2["cvm"][0], rtol=1e-8)
