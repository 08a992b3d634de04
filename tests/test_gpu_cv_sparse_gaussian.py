"""cv.oem(family = "gaussian") on a resident sparse x.

A. oemgpu_cv_sparse_score_res alone (through oemgpu_selftest_cv_sparse_score: the fold layout and the compressed rows, then the entry as
   it is) against numpy in long double on DENSE RANDOM tables: folds of 1, 17 and 8,200 rows (the long one crosses the 8192-row chunk),
   the rest, and an absent one; rows without a stored entry and an empty column; p = 23 and 170; 5, 64, 65 and 100 lambdas (one block of
   64, exactly one, two); one and two penalties with all, nl - 3, one and no valid column; mse and mae; 130 folds of 7 or 8 rows.
   Tolerances are section 3.14's: counts exact, fold means rtol 1e-12, M2 1e-11, (0, NaN, NaN) where due, yhat within
   4 (nnz_i + 2) eps (|b_0| + sum |x_ij b_j|) in the caller's row order with NaN in the invalid columns, the same bits from two calls.
B. oemgpu_cv_sparse_fold_fits_res against oracle.fit_sparse on the gathered rows x.tocsr()[foldid != i]: the figures of the sparse
   parity tests (tests/test_gpu_parity.py) -- beta 1e-8 max(1, |beta|_inf), d 1e-10, lambda rtol 1e-11, niter +- 1 -- for standardize x
   intercept, lasso / mcp / grp.lasso, a user lambda list, both Gram routes; one column lies wholly in fold 4 (the fit that leaves
   fold 4 out sees an empty column) and one wholly in fold 2.  Slot 0 against oem_amd.oem on the scipy matrix: 1e-9.
C. cv_oem(SparseX(x), y) against tests/cv_gaussian_restatement.py on x.toarray() with the oracle's sparse fits: cvm rtol 1e-9, cvsd
   1e-8, the same lambda.min and best.model, fit.preval, predict_cv on a sparse newx.
D. refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

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


def _vec(y, fid):
    import torch
    return (torch.as_tensor(np.asarray(y, dtype=np.float64), device="cuda:0"),
            torch.as_tensor(np.ascontiguousarray(fid, dtype=np.int32), device="cuda:0"))


# ------------------------------------------------------------------------------------------------------------- A: the scoring entry
_YHAT = {}                                                  # the long-double products, shared by the mse and the mae case of a table


def _score_reference(x, y, fid, coef, ncol, measure, key=None):
    """triples[K][npen][nl][3] in long double ((0, NaN, NaN) where the entry must say so), yhat[npen][nl][n] and its bound in float64"""
    K, npen, nl, _ = coef.shape
    n = len(y)
    xd = x.toarray()
    yhat = _YHAT.setdefault(key, {}) if key is not None else {}
    nnz_row = np.diff(x.tocsr().indptr)
    tri = np.full((K, npen, nl, 3), np.nan, dtype=LD)
    tri[..., 0] = 0
    pred = np.full((npen, nl, n), np.nan)
    bound = np.zeros((npen, nl, n))
    xx, yy = xd.astype(LD), y.astype(LD)
    for k in range(K):
        rows = np.nonzero(fid == k + 1)[0]
        if len(rows) == 0:
            continue
        b = coef[k].astype(LD)
        if k not in yhat:
            yhat[k] = b[..., :1] + b[..., 1:] @ xx[rows].T                             # [npen, nl, rows]
        yh = yhat[k]
        res = yy[rows] - yh
        v = res * res if measure == "mse" else np.abs(res)
        m = v.mean(axis=-1)
        m2 = ((v - m[..., None]) ** 2).sum(axis=-1)
        mag = (np.abs(coef[k][..., :1]) + np.abs(coef[k][..., 1:]) @ np.abs(xd[rows]).T) * (4.0 * (nnz_row[rows] + 2) * EPS)
        for pen in range(npen):
            c = ncol[pen]
            tri[k, pen, :c, 0] = len(rows); tri[k, pen, :c, 1] = m[pen, :c]; tri[k, pen, :c, 2] = m2[pen, :c]
            pred[pen, :c, rows] = yh[pen, :c].astype(np.float64).T
            bound[pen, :c, rows] = mag[pen, :c].T
    return tri, pred, bound


def _check_score(api, sx, x, y, fid, K, coef, ncol, measure, label, key=None):
    yd, fd = _vec(y, fid)
    tri, pm = api.cv_sparse_gaussian_score(sx, yd, fd, K, coef, ncol, type_measure=measure, predmat=True)
    ref, pref, pbound = _score_reference(x, y, fid, coef, ncol, measure, key)
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
    tri2, pm2 = api.cv_sparse_gaussian_score(sx, yd, fd, K, coef, ncol, type_measure=measure, predmat=True)   # the same call: the same bits
    assert np.array_equal(tri, tri2, equal_nan=True) and np.array_equal(pm, pm2, equal_nan=True), label
    tri3, none = api.cv_sparse_gaussian_score(sx, yd, fd, K, coef, ncol, type_measure=measure)              # and without the prediction store
    assert none is None and np.array_equal(tri, tri3, equal_nan=True), label


def _table(seed, K, npen, nl, p):
    return np.random.default_rng(seed).normal(size=(K, npen, nl, p + 1)) / np.sqrt(p + 1.0)


def _sparse(seed, n, p, density):
    """n x p at `density` with values N(0.1, 1), column 3 emptied and every 97th row left without a stored entry"""
    rng = np.random.default_rng(seed)
    x = sp.random(n, p, density=density, random_state=seed, format="csr", data_rvs=lambda k: rng.normal(size=k) + 0.1).tolil()
    x[:, 3] = 0.0
    x[::97] = 0.0
    x = sp.csc_matrix(x); x.eliminate_zeros()
    assert x[:, 3].nnz == 0 and (np.diff(x.tocsr().indptr) == 0).sum() >= n // 97
    return x


S_K = 5
S_FID = np.random.default_rng(31).permutation(np.concatenate([np.full(1, 1), np.full(17, 2), np.full(8200, 3), np.full(2793, 5)]))   # 11,011 rows, fold 4 absent


@functools.lru_cache(maxsize=None)
def _score_data(p):
    x = _sparse(77 + p, len(S_FID), p, 0.2 if p == 23 else 0.05)
    y = np.random.default_rng(78 + p).normal(size=len(S_FID)) + 0.3
    return x, y


@pytest.fixture(scope="module")
def score_x(api):
    made = {}

    def get(p):
        if p not in made:
            made[p] = api.SparseX(_score_data(p)[0])
        return made[p]
    yield get
    for h in made.values():
        h.close()


@pytest.mark.parametrize("measure", ["mse", "mae"])
@pytest.mark.parametrize("nl", [5, 64, 65, 100])
@pytest.mark.parametrize("p", [23, 170])
def test_score_fold_sizes(api, score_x, p, nl, measure):
    """folds of 1, 17, 8,200 and 2,793 rows and an id that never occurs: the wave stride runs over folds of very unequal size, most
    waves see no row of the short ones (their partials are zeros), the long one spans two 8192-row chunks; two penalties, the second
    with three columns fewer"""
    x, y = _score_data(p)
    _check_score(api, score_x(p), x, y, S_FID, S_K, _table(5 * p + nl, S_K, 2, nl, p), [nl, nl - 3], measure, f"p={p} nl={nl} {measure}",
                 key=(p, nl))


@pytest.mark.parametrize("ncol", [[65], [1, 0]], ids=["one penalty", "ncol = (1, 0)"])
def test_score_one_penalty_one_valid_column_and_none(api, score_x, ncol):
    x, y = _score_data(23)
    _check_score(api, score_x(23), x, y, S_FID, S_K, _table(3 + len(ncol), S_K, len(ncol), 65, 23), ncol, "mae", f"ncol={ncol}")


def test_score_many_folds(api):
    """K = 130 at n = 1,000: folds of 7 or 8 rows, more flushes than rows per wave"""
    n, p, K, nl = 1000, 23, 130, 21
    x = _sparse(600, n, p, 0.2)
    rng = np.random.default_rng(601)
    y = rng.normal(size=n) + 0.3
    fid = rng.permutation(np.resize(np.arange(1, K + 1), n))
    with api.SparseX(x) as sx:
        _check_score(api, sx, x, y, fid, K, _table(K, K, 2, nl, p), [nl, nl - 3], "mse", f"K={K}")


# ------------------------------------------------------------------------------------------------------------- B: the fold fits
N, P_, NF, NL = 3001, 23, 5, 30
GROUPS = np.arange(P_) // 4 + 1
PENS = ["lasso", "mcp", "grp.lasso"]
USER_LAMBDA = [np.geomspace(1.5, 2e-3, 17), np.geomspace(1.0, 1e-3, 17), np.geomspace(2.0, 5e-3, 17)]
COL_F4, COL_F2 = 20, 9                                      # columns whose non-zeros all lie in fold 4 / in fold 2


@functools.lru_cache(maxsize=None)
def _data():
    rng = np.random.default_rng(11)
    fid = rng.permutation(np.resize(np.arange(1, NF + 1), N))
    x = sp.random(N, P_, density=0.05, random_state=12, format="csc", data_rvs=lambda k: rng.normal(size=k) * 2 + 0.3).tolil()
    for col, fold in ((COL_F4, 4), (COL_F2, 2)):
        x[np.nonzero(fid != fold)[0], col] = 0.0
    x = sp.csc_matrix(x); x.eliminate_zeros()
    assert x[:, COL_F4].nnz > 5 and x[:, COL_F2].nnz > 5 and x.tocsr()[fid != 4][:, COL_F4].nnz == 0
    b = np.zeros(P_); b[:4] = [1.0, -1.5, 0.5, 2.0]; b[COL_F2] = 1.0
    y = x @ b + rng.normal(size=N) * 0.5 + 0.4
    return x, y, fid


def _kw(user):
    return dict(tol=1e-10, maxit=2000, **({} if user else {"nlambda": NL}))


@functools.lru_cache(maxsize=None)
def _oracle_fits(std, icpt, user=False):
    """(full fit, fold fits on the gathered rows), computed once per configuration and shared"""
    x, y, fid = _data()
    rg, rug = orc.r_sparse_groups(GROUPS, icpt)
    opts = dict(penalty=PENS, standardize=std, intercept=icpt, lambda_=USER_LAMBDA if user else None, groups=rg, unique_groups=rug,
                lambda_min_ratio=1e-4, **_kw(user))
    xr = x.tocsr()
    return orc.fit_sparse(x, y, **opts), [orc.fit_sparse(xr[fid != i], y[fid != i], **opts) for i in range(1, NF + 1)]


@pytest.fixture(scope="module")
def fit_x(api):
    with api.SparseX(_data()[0]) as sx:
        yield sx


def _fold_fits(api, sx, std, icpt, user=False, pens=PENS):
    x, y, fid = _data()
    kw = dict(standardize=std, intercept=icpt, groups=GROUPS, **_kw(user))
    lam = [USER_LAMBDA[PENS.index(q)] for q in pens] if user else ()
    return api._cv_gaussian_sparse_fold_fits(sx, y, fid, NF, pens, lam, kw)


def _compare_fits(fits, ref, label, pens=PENS):
    worst = 0.0
    for i, (f, r) in enumerate(zip(fits, ref)):
        assert abs(f["d"] - r["d"]) < 1e-10 * r["d"], (label, i)
        for k, q in enumerate(pens):
            kr = PENS.index(q)
            assert np.allclose(f["lambda"][k], r["lambda"][kr], rtol=1e-11), (label, i, k)
            scale = max(1.0, float(np.abs(r["beta"][kr]).max()))
            gap = float(np.abs(f["beta"][k] - r["beta"][kr]).max()) / scale
            worst = max(worst, gap)
            assert gap < 1e-8, (label, i, k, gap)
            dn = np.abs(np.ravel(f["niter"][k]).astype(int) - np.ravel(r["niter"][kr]))
            assert dn.max() <= 1, (label, i, k, dn)
    print(f"GAP {label}: beta {worst:.1e} of max(1, |beta|_inf)")


@pytest.mark.parametrize("std,icpt", [(True, True), (False, True), (True, False), (False, False)])
def test_fold_fits(api, fit_x, std, icpt):
    import oem_amd
    fit0, outlist, dev = _fold_fits(api, fit_x, std, icpt)
    x, y, fid = _data()
    assert dev["fold_n"].tolist() == [int((fid == i).sum()) for i in range(1, NF + 1)]
    assert fit0["nobs"] == N and [o["nobs"] for o in outlist] == [N - int((fid == i).sum()) for i in range(1, NF + 1)]
    full, folds = _oracle_fits(std, icpt)
    _compare_fits([fit0] + outlist, [full] + folds, f"standardize={std} intercept={icpt}")
    for k in range(len(PENS)):                                                                      # the column that is empty among the kept rows
        assert not np.asarray(outlist[3]["beta"][k])[1 + COL_F4].any() and not np.asarray(folds[3]["beta"][k])[1 + COL_F4].any()
    # slot 0 is what oem() on the scipy matrix returns, decorated the same way
    g = oem_amd.oem(x, y, penalty=PENS, standardize=std, intercept=icpt, groups=GROUPS, **_kw(False))
    for k in range(len(PENS)):
        assert np.allclose(fit0["lambda"][k], g["lambda"][k], rtol=1e-11)
        assert np.abs(fit0["beta"][k] - g["beta"][k]).max() < 1e-9
    assert fit0["rownames"] == g["rownames"] and fit0["varnames"] == g["varnames"] and set(fit0) == set(g)


def test_fold_fits_user_lambda(api, fit_x):
    fit0, outlist, _ = _fold_fits(api, fit_x, True, True, user=True)
    for o in [fit0] + outlist:
        for k in range(len(PENS)):
            assert np.array_equal(o["lambda"][k], USER_LAMBDA[k])
    full, folds = _oracle_fits(True, True, user=True)
    _compare_fits([fit0] + outlist, [full] + folds, "user lambda")


@pytest.mark.parametrize("route", ["csc", "dense"])
def test_fold_fits_both_gram_routes(api, fit_x, monkeypatch, route):
    monkeypatch.setenv("OEM_SPARSE_GRAM", route)
    fit0, outlist, _ = _fold_fits(api, fit_x, True, True, pens=["lasso", "mcp"])
    full, folds = _oracle_fits(True, True)
    _compare_fits([fit0] + outlist, [full] + folds, f"OEM_SPARSE_GRAM={route}", pens=["lasso", "mcp"])


def test_fold_fits_absent_fold_is_the_full_fit(api, fit_x):
    """an id in 1..K that never occurs: that fold's fit is the fit of all rows -- the same moment sums, the same bits"""
    x, y, fid = _data()
    fid6 = np.where(fid == 5, 6, fid)                                                               # ids 1, 2, 3, 4, 6 of 6
    fit0, outlist, dev = api._cv_gaussian_sparse_fold_fits(fit_x, y, fid6, 6, ["lasso"], (), dict(nlambda=21, tol=1e-10, maxit=2000))
    assert dev["fold_n"][4] == 0
    assert np.array_equal(outlist[4]["lambda"][0], fit0["lambda"][0]) and np.array_equal(outlist[4]["beta"][0], fit0["beta"][0])


# ------------------------------------------------------------------------------------------------------------- C: cv_oem end to end
# lasso and grp.lasso of the fits above (penalties are independent cold starts).  Not mcp: below some lambda its solution is least squares
# on the support whatever lambda is, so its cvm has a plateau at the minimum -- ties to rounding, which no route can be held to.
E2E = [0, 2]
E2E_PENS = [PENS[k] for k in E2E]


def _sub(fit):
    return {key: ([val[k] for k in E2E] if isinstance(val, list) else val) for key, val in fit.items()}


@pytest.mark.parametrize("measure", ["mse", "mae"])
@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "rows"])
def test_cv_oem_against_the_restatement(api, fit_x, grouped, measure):
    """cv_oem on the SparseX with keep=True; y comes as a device tensor in one of the four cases.  At this seed the last of the 30
    columns lies below the smallest lambda of some fold, so a masked column is exercised -- asserted."""
    import oem_amd
    x, y, fid = _data()
    full, folds = _oracle_fits(True, True)
    ref = R.cv_oem(x.toarray(), y, fid, E2E_PENS, type_measure=measure, grouped=grouped, fits=(_sub(full), [_sub(o) for o in folds]))
    assert all(int(w.sum()) == NL - 1 for w in ref["which_lam"])
    mins = []
    for c in ref["cvm"]:                                                                            # no near-tie at the minimum
        s = np.sort(c)
        assert s[1] - s[0] > 1e-6 * s[0]
        mins.append(s[0])
    assert abs(mins[0] - mins[1]) > 1e-6 * min(mins)
    yy = _vec(y, fid)[0] if (grouped and measure == "mae") else y
    f = oem_amd.cv_oem(fit_x, yy, penalty=E2E_PENS, foldid=fid, type_measure=measure, grouped=grouped, keep=True, groups=GROUPS,
                       parallel=True, **_kw(False))
    for k in range(len(E2E)):
        assert np.allclose(f["lambda"][k], ref["lambda"][k], rtol=1e-11)
        gm = float(np.max(np.abs(f["cvm"][k] - ref["cvm"][k]) / ref["cvm"][k]))
        gs = float(np.max(np.abs(f["cvsd"][k] - ref["cvsd"][k]) / ref["cvsd"][k]))
        print(f"GAP {E2E_PENS[k]} {measure} grouped={grouped}: cvm {gm:.1e} cvsd {gs:.1e}")
        assert gm <= 1e-9 and gs <= 1e-8, (k, gm, gs)
        pv, pr = f["fit.preval"][k], ref["predmat"][k]
        assert pv.shape == pr.shape and np.array_equal(np.isnan(pv), np.isnan(pr))
        ok = ~np.isnan(pr)
        assert np.abs(pv[ok] - pr[ok]).max() < 1e-8 * max(1.0, float(np.abs(pr[ok]).max()))
    assert f["model.min"] - 1 == ref["model_min"] and f["best.model"] == E2E_PENS[ref["model_min"]]
    assert np.isclose(f["lambda.min"], ref["lambda_min"], rtol=1e-11)
    assert np.array_equal(f["foldid"], fid)
    assert set(f) == set(oem_amd.cv_oem(x.toarray()[:400], y[:400], penalty=E2E_PENS, foldid=np.resize(np.arange(1, 4), 400), keep=True,
                                        groups=GROUPS, nlambda=5))
    # predict_cv on a sparse newx: the full fit's coefficients at lambda.min
    newx = x[:50]
    want = R.predict_at(_sub(full), ref["model_min"], newx.toarray(), np.array([ref["lambda_min"]]))
    got = oem_amd.predict_cv(f, newx)
    assert np.abs(np.ravel(got) - np.ravel(want)).max() < 1e-8 * max(1.0, float(np.abs(want).max()))


# ------------------------------------------------------------------------------------------------------------- D: refusals
def test_python_refusals(api, fit_x):
    import oem_amd
    x, y, fid = _data()
    kw = dict(foldid=fid, nlambda=5)
    with pytest.raises(ValueError, match="ols"):
        oem_amd.cv_oem(fit_x, y, penalty=["lasso", "ols"], **kw)
    with pytest.raises(ValueError, match="weights not implemented"):
        oem_amd.cv_oem(fit_x, y, penalty="lasso", weights=np.ones(N), **kw)
    with pytest.raises(ValueError, match="not split over devices"):
        oem_amd.cv_oem(fit_x, y, penalty="lasso", ngpus=2, **kw)
    with pytest.raises(ValueError, match="not split over devices"):
        oem_amd.cv_oem(fit_x, y, penalty="lasso", devices=[0], **kw)
    with pytest.raises(ValueError, match="lengths do not match"):
        oem_amd.cv_oem(fit_x, y[:-1], penalty="lasso", **kw)
    with pytest.raises(ValueError, match="nfolds must be bigger than 3"):
        oem_amd.cv_oem(fit_x, y, penalty="lasso", foldid=np.resize(np.arange(1, 3), N), nlambda=5)
    stray = fid.copy(); stray[7] = 0
    with pytest.raises(ValueError, match="foldid must hold one integer in 1..nfolds"):
        oem_amd.cv_oem(fit_x, y, penalty="lasso", foldid=stray, nlambda=5)
    closed = api.SparseX(x[:100])
    closed.close()
    with pytest.raises(ValueError, match="closed"):
        oem_amd.cv_oem(closed, y[:100], penalty="lasso", foldid=np.resize(np.arange(1, 4), 100), nlambda=5)
    with pytest.raises(ValueError, match="oem\\(\\) on a SparseX is not built"):                  # out of scope, and said so
        oem_amd.oem(fit_x, y, penalty="lasso", nlambda=5)
    assert fit_x.device_bytes >= 24 * x.nnz + 8 * N
    # a scipy matrix keeps its refusal, and says where the route is
    with pytest.raises(ValueError, match='sparse x is served for family = "binomial" only') as e:
        oem_amd.cv_oem(x, y, penalty="lasso", **kw)
    assert "SparseX" in str(e.value)


def test_a_fold_that_keeps_too_few_rows_is_named(api):
    import oem_amd
    rng = np.random.default_rng(4)
    n, p = 100, 20
    x = sp.random(n, p, density=0.3, random_state=4, format="csc")
    y = rng.normal(size=n)
    fid = np.concatenate([np.full(10, 1), np.full(80, 2), np.full(10, 3)])                            # fold 2 leaves 20 rows for 20 columns
    with api.SparseX(x) as sx:
        with pytest.raises(ValueError, match="fold 2 leaves 20 rows for 20 columns"):
            oem_amd.cv_oem(sx, y, penalty="lasso", foldid=fid, nlambda=5)
        # the entry itself, behind the Python check: the same fold from the device, and a stray id
        a, _, _, _ = oem_amd.oem(sx, y, penalty="lasso", nlambda=5, _args_only=True)
        yd, fd = _vec(y, fid)
        out = [np.zeros((4, 1, 5, p + 1)), np.zeros((4, 1, 5)), np.zeros((4, 1, 5), dtype=np.int32), np.zeros((4, 1, 5)), np.zeros(4)]
        fn = np.zeros(3, dtype=np.int64)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)

        def call(f):
            return oem_amd.lib().oemgpu_cv_sparse_fold_fits_res(api.context(0), sx.handle, yd.data_ptr(), f.data_ptr(), 3, 1, 1, C.byref(a.c),
                                                                out[0].ctypes.data_as(dp), out[1].ctypes.data_as(dp), out[2].ctypes.data_as(ip),
                                                                out[3].ctypes.data_as(dp), out[4].ctypes.data_as(dp),
                                                                fn.ctypes.data_as(C.POINTER(C.c_int64)))
        assert call(fd) == -4 and b"fold 2 leaves 20 rows" in oem_amd.lib().oemgpu_last_error()
        bad = np.resize(np.arange(1, 4), n); bad[7] = 4
        assert call(_vec(y, bad)[1]) == -1 and b"cv_sparse_fold_fits: foldid must hold values" in oem_amd.lib().oemgpu_last_error()


def test_a_layout_is_scored_by_its_own_entry_only(api):
    """the dense scoring entry after a sparse layout, and the sparse one after a dense layout and after xval.oem's, on the same context
    and the same (n, p, K, npen, nl): OEMGPU_ERR_ARG, nothing read"""
    import oem_amd
    import torch
    L = oem_amd.lib()
    rng = np.random.default_rng(2)
    n, p, K, nl = 200, 5, 3, 4
    x = sp.random(n, p, density=0.4, random_state=2, format="csc")
    y = rng.normal(size=n)
    fid = np.resize(np.arange(1, K + 1), n)
    yd, fd = _vec(y, fid)
    xd = torch.as_tensor(np.ascontiguousarray(x.toarray().T), device="cuda:0").t()
    coef = _table(1, K, 1, nl, p)
    tri = np.zeros((K, 1, nl, 3))
    ncol = np.array([nl], dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    args = (api.context(0), n, p, K, coef.ctypes.data_as(dp), 1, nl, ncol.ctypes.data_as(ip), 0, tri.ctypes.data_as(dp), None)
    with api.SparseX(x) as sx:
        want, _ = api.cv_sparse_gaussian_score(sx, yd, fd, K, coef, [nl])
        assert L.oemgpu_cv_sparse_score_res(*args) == 0 and np.array_equal(tri, want)
        assert L.oemgpu_cv_score_dev(*args) == -1 and b"oemgpu_cv_fold_fits_dev" in L.oemgpu_last_error()
        assert L.oemgpu_cv_sparse_score_res(api.context(0), n, p, K, coef.ctypes.data_as(dp), 1, nl - 1, ncol.ctypes.data_as(ip), 0,
                                            tri.ctypes.data_as(dp), None) == -1                       # another nl: another layout
        api.cv_gaussian_score(xd, yd, fd, K, coef, [nl])                                              # a dense layout of the same shape
        assert L.oemgpu_cv_score_dev(*args) == 0
        assert L.oemgpu_cv_sparse_score_res(*args) == -1 and b"oemgpu_cv_sparse_fold_fits_res" in L.oemgpu_last_error()
        api.cv_sparse_gaussian_score(sx, yd, fd, K, coef, [nl])
        assert L.oemgpu_cv_sparse_score_res(*args) == 0
        api.xval_cv_error(xd, yd, fd, K, coef)                                                        # xval.oem lays ITS rows out
        assert L.oemgpu_cv_sparse_score_res(*args) == -1 and L.oemgpu_cv_score_dev(*args) == -1
