"""cv.oem on a resident sparse x with n <= p on the GPU.

A. oemgpu_fit_sparse_wide_fold_res: the bits of oemgpu_fit_sparse_wide_res with leave_out = 0 and with a fold id no row carries, the
   same bits from two calls; every fold of every parity input against oracle.fit_sparse on the SLICED data by the _agree rule and
   DTOL of tests/test_gpu_sparse_wide.py (tests/test_cv_sparse_wide_cpu.py shows on the CPU that these inputs stay inside the rule
   on the reference side alone), lambda to 1e-12, kept exact, the loss to 1e-7; the structures a fold can make (a column it empties,
   an all-ones column, empty rows kept and left out, folds of 1, n - 3 and 2 rows; a full row left out and kept, a full column);
   exact exclusion (y = NaN in the left-out rows, the other folds' ids permuted: the same bits); the refusals from the device.
B. oemgpu_cv_sparse_wide_score_res against numpy in long double on a table of the caller's: counts exact, fold means and M2 to 1e-12
   of their scale (the mean error; the sum of squared errors M2 is what is left of after cancellation), (0, NaN, NaN) where due, eta
   in the caller's row order within 4 (nnz_i + 2) eps (|b_0| + sum |x_ij b_j|) with NaN in the invalid columns, the same bits from
   two calls, and after another cv call has left its layout on the context -- which stays valid.
C. cv_oem(SparseX, intercept=False) against tests/cv_gaussian_restatement.py with the oracle's fits on the sliced data; oem(SparseX)
   against oem(scipy x) bit for bit; predict_cv; the refusals in Python, the two pinned n > p sentences among them."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as orc
from tests import cv_gaussian_restatement as CR
from tests import cv_sparse_wide_restatement as M
from tests.test_gpu_sparse_wide import DTOL, _agree, _same_bits

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = np.finfo(np.float64).eps
ERR_ARG = -1
PENS = ["lasso", "mcp", "elastic.net", "grp.lasso", "sparse.grp.lasso"]
LOSS_PENS = ["lasso", "mcp"]


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available()
    from oem_amd import api
    return api


def _vec(y, fid):
    import torch
    return (torch.as_tensor(np.asarray(y, dtype=np.float64), device="cuda:0"),
            None if fid is None else torch.as_tensor(np.ascontiguousarray(fid, dtype=np.int32), device="cuda:0"))


def _groups(p):
    return np.arange(p) // 4 + 1


def _fold_fit(api, sx, y, fid, K, k, **kw):
    yd, fd = _vec(y, fid)
    return api.sparse_wide_fold_fit(sx, yd, fd, K, k, **kw)


def _sliced_oracle(x, y, fid, k, **kw):
    keep = fid != k
    return orc.fit_sparse(sp.csr_matrix(x)[keep].tocsc(), y[keep], native=True, intercept=False, **kw)


def _compare(f, r, pens, tol, label, loss=False):
    assert abs(f["d"] - r["d"]) <= DTOL * r["d"], (label, f["d"], r["d"])
    for i, pen in enumerate(pens):
        assert np.allclose(f["lambda"][i], r["lambda"][i], rtol=1e-12, atol=0), (label, pen)
        _agree(f, r, i, tol, (label, pen))
        assert np.all(np.asarray(f["beta"][i])[0] == 0.0)
        if loss:
            assert np.allclose(np.ravel(f["loss"][i]), np.ravel(r["loss"][i]), rtol=1e-7, atol=0), (label, pen)
        else:
            assert np.all(np.ravel(f["loss"][i]) == 1e99)


# ------------------------------------------------------------------------------------------------------------- A: the fold fit
def test_bits_of_the_unmasked_entry_and_of_two_calls(api):
    n, p, dens, K = M.PARITY_CASES[3]
    x, y, fid = M.parity_input(n, p, dens, K)
    kw = dict(M.PARITY_KW, penalty=PENS, groups=_groups(p), alpha=0.7, standardize=True, compute_loss=True)
    with api.SparseX(x) as sx:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            f = api.oem(sx, y, intercept=False, **kw)               # oemgpu_fit_sparse_wide_res
        assert api.last_host_path_engine() == "sparse-wide"
        g = _fold_fit(api, sx, y, fid, K, 0, **kw)
        _same_bits(f, g)
        g = _fold_fit(api, sx, y, None, K, 0, **kw)                 # a NULL foldid with leave_out = 0
        _same_bits(f, g)
        assert g["nobs"] == n
        g = _fold_fit(api, sx, y, fid, K + 1, K + 1, **kw)          # an id that never occurs: the fit of all rows
        _same_bits(f, g)
        assert g["nobs"] == n
        a = _fold_fit(api, sx, y, fid, K, 2, **kw)
        b = _fold_fit(api, sx, y, fid, K, 2, **kw)
        _same_bits(a, b)
        assert a["nobs"] == int((fid != 2).sum()) and a["d"] != f["d"]


@pytest.mark.parametrize("n,p,dens,K", M.PARITY_CASES)
@pytest.mark.parametrize("standardize", [False, True])
def test_every_fold_against_the_oracle_on_the_sliced_data(api, n, p, dens, K, standardize):
    x, y, fid = M.parity_input(n, p, dens, K)
    g = _groups(p)
    kw = dict(M.PARITY_KW, penalty=PENS, groups=g, alpha=0.7, standardize=standardize)
    lkw = dict(M.PARITY_KW, penalty=LOSS_PENS, standardize=standardize, compute_loss=True)
    with api.SparseX(x) as sx:
        for k in range(1, K + 1):
            f = _fold_fit(api, sx, y, fid, K, k, **kw)
            assert f["nobs"] == int((fid != k).sum())               # kept, exact
            _compare(f, _sliced_oracle(x, y, fid, k, unique_groups=np.unique(g), **kw), PENS, kw["tol"], (n, p, k))
            f = _fold_fit(api, sx, y, fid, K, k, **lkw)
            _compare(f, _sliced_oracle(x, y, fid, k, **lkw), LOSS_PENS, lkw["tol"], (n, p, k, "loss"), loss=True)


def _structure(name):
    """(x, y, foldid, K) at 50 x 300 (6 %), or 200 x 20,000 (1 %) for the long forms"""
    if name == "long":
        n, p, K = 200, 20000, 3
        rng = np.random.default_rng(11)
        x = sp.random(n, p, density=0.01, format="lil", random_state=rng, data_rvs=lambda k: rng.normal(size=k) * 1.5)
        x[7, :] = 0.1 * rng.normal(size=p)                          # one row stores all p entries
        x[:, 123] = 1.0                                             # one column stores all n: all ones
        fid = rng.permutation(np.resize(np.arange(1, K + 1), n))
        fid[7] = 1                                                  # the full row: left out by fold 1, kept by the others
    else:
        n, p, K = 50, 300, 3
        rng = np.random.default_rng(50 + len(name))
        x = sp.random(n, p, density=0.06, format="lil", random_state=rng, data_rvs=lambda k: rng.normal(size=k) * 1.5)
        if name == "fold sizes":                                    # folds of 1, n - 3 and 2 rows; an empty row in fold 2 and one in fold 3
            fid = rng.permutation(np.concatenate([np.full(1, 1), np.full(n - 3, 2), np.full(2, 3)]))
            x[np.nonzero(fid == 2)[0][4], :] = 0.0
            x[np.nonzero(fid == 3)[0][0], :] = 0.0
        else:                                                       # "columns": column 17 lies wholly in fold 1, column 40 is all ones
            fid = rng.permutation(np.resize(np.arange(1, K + 1), n))
            x[np.nonzero(fid != 1)[0], 17] = 0.0
            x[np.nonzero(fid == 1)[0], 17] = rng.normal(size=int((fid == 1).sum())) + 2.0
            x[:, 40] = 1.0
            x[np.nonzero(fid == 2)[0][0], :] = 0.0                  # an empty row: left out by fold 2, kept by 1 and 3
            x[np.nonzero(fid == 2)[0][0], 40] = 0.0
    x = sp.csc_matrix(x); x.sum_duplicates(); x.sort_indices()
    b = np.zeros(p); b[np.argsort(-np.diff(x.indptr), kind="stable")[:5]] = rng.uniform(1, 2, 5)
    y = x @ b + 0.3 * rng.normal(size=n)
    return x, y, fid, K


@pytest.mark.parametrize("name,folds", [("columns", (1, 2, 3)), ("fold sizes", (1, 2, 3)), ("long", (1, 2))])
def test_structures(api, name, folds):
    x, y, fid, K = _structure(name)
    n, p = x.shape
    g = _groups(p)
    big = name == "long"
    kw = dict(penalty=["lasso", "grp.lasso"] if big else ["lasso", "mcp", "grp.lasso"], groups=g, standardize=True, nlambda=3 if big else 5,
              lambda_min_ratio=0.05, tol=1e-9, maxit=400)
    if big:
        assert np.diff(x.indptr).max() == n and np.diff(sp.csr_matrix(x).indptr).max() == p and fid[7] == 1
    if name == "fold sizes":
        assert [int((fid == k).sum()) for k in (1, 2, 3)] == [1, n - 3, 2]
    with api.SparseX(x) as sx:
        for k in folds:
            f = _fold_fit(api, sx, y, fid, K, k, **kw)
            assert f["nobs"] == int((fid != k).sum())
            _compare(f, _sliced_oracle(x, y, fid, k, unique_groups=np.unique(g), **kw), kw["penalty"], kw["tol"], (name, k))
            if name == "columns" and k == 1:                        # the column the fold empties: colsq -> 1, never selected
                assert sp.csr_matrix(x)[fid != 1][:, 17].nnz == 0 and x[:, 17].nnz > 5
                assert all(not np.asarray(b)[1 + 17].any() for b in f["beta"])


def test_exclusion_is_exact(api):
    n, p, dens, K = M.PARITY_CASES[2]
    x, y, fid = M.parity_input(n, p, dens, K)
    kw = dict(M.PARITY_KW, penalty=["lasso", "grp.lasso"], groups=_groups(p), standardize=True, compute_loss=True)
    with api.SparseX(x) as sx:
        f = _fold_fit(api, sx, y, fid, K, 2, **kw)
        g = _fold_fit(api, sx, np.where(fid == 2, np.nan, y), fid, K, 2, **kw)        # y of a left-out row is never read
        _same_bits(f, g)
        assert np.all(np.isfinite(np.asarray(g["beta"][0]))) and np.all(np.isfinite(np.ravel(g["loss"][0])))
        other = fid.copy()
        rows = np.nonzero(fid != 2)[0]
        other[rows] = np.random.default_rng(3).permutation(fid[rows])                 # the ids of the other folds change hands
        assert np.array_equal(other == 2, fid == 2) and not np.array_equal(other, fid)
        g = _fold_fit(api, sx, y, other, K, 2, **kw)
        _same_bits(f, g)


def test_refusals_from_the_device(api):
    from oem_amd import _lib as L
    n, p, dens, K = M.PARITY_CASES[0]
    x, y, fid = M.parity_input(n, p, dens, K)
    kw = dict(M.PARITY_KW, penalty=["lasso"])
    with api.SparseX(x) as sx:
        for bad in (0, K + 1, -3):
            stray = fid.copy(); stray[5] = bad
            for k in (0, 1):                                        # the ids' range whatever is left out
                with pytest.raises(L.OemgpuError, match="fold ids are outside") as e:
                    _fold_fit(api, sx, y, stray, K, k, **kw)
                assert e.value.code == ERR_ARG
        one = np.full(n, 2); one[9] = 1; one[10] = 3
        assert _fold_fit(api, sx, y, one, K, 2, **kw)["nobs"] == 2                     # two kept rows are served
        one[10] = 2
        with pytest.raises(L.OemgpuError, match="fold 2 keeps 1 of the %d rows" % n) as e:
            _fold_fit(api, sx, y, one, K, 2, **kw)
        assert e.value.code == ERR_ARG
        f = _fold_fit(api, sx, y, fid, K, 1, **kw)                  # the context serves the next call
        assert f["nobs"] == int((fid != 1).sum())


# ------------------------------------------------------------------------------------------------------------- B: the scoring entry
S_N, S_P, S_K = 60, 400, 4
_YHAT = {}


@functools.lru_cache(maxsize=None)
def _score_data():
    rng = np.random.default_rng(91)
    x = sp.random(S_N, S_P, density=0.05, format="lil", random_state=rng, data_rvs=lambda k: rng.normal(size=k) + 0.1)
    x[:, 3] = 0.0
    x[11, :] = 0.0                                                  # a row without a stored entry
    x = sp.csc_matrix(x); x.eliminate_zeros(); x.sort_indices()
    y = rng.normal(size=S_N) + 0.3
    fid = rng.permutation(np.concatenate([np.full(1, 1), np.full(17, 2), np.full(S_N - 18, 4)]))      # fold 3 has no rows
    return x, y, fid


def _score_reference(x, y, fid, coef, ncol, measure, key):
    """triples[K][npen][nl][3] in long double ((0, NaN, NaN) where the entry must say so), their scales, eta[npen][nl][n] and its bound"""
    K, npen, nl, _ = coef.shape
    n = len(y)
    xd = x.toarray()
    nnz_row = np.diff(x.tocsr().indptr)
    tri = np.full((K, npen, nl, 3), np.nan, dtype=LD); tri[..., 0] = 0
    scale = np.ones((K, npen, nl, 3), dtype=LD)
    pred = np.full((npen, nl, n), np.nan); bound = np.zeros((npen, nl, n))
    xx, yy = xd.astype(LD), y.astype(LD)
    yhat = _YHAT.setdefault(key, {})
    for k in range(K):
        rows = np.nonzero(fid == k + 1)[0]
        if len(rows) == 0:
            continue
        b = coef[k].astype(LD)
        if k not in yhat:
            yhat[k] = b[..., :1] + b[..., 1:] @ xx[rows].T
        yh = yhat[k]
        res = yy[rows] - yh
        v = res * res if measure == "mse" else np.abs(res)
        m = v.mean(axis=-1)
        m2 = ((v - m[..., None]) ** 2).sum(axis=-1)
        mag = (np.abs(coef[k][..., :1]) + np.abs(coef[k][..., 1:]) @ np.abs(xd[rows]).T) * (4.0 * (nnz_row[rows] + 2) * EPS)
        for pen in range(npen):
            c = ncol[pen]
            tri[k, pen, :c, 0] = len(rows); tri[k, pen, :c, 1] = m[pen, :c]; tri[k, pen, :c, 2] = m2[pen, :c]
            scale[k, pen, :c, 1] = m[pen, :c]; scale[k, pen, :c, 2] = (v * v).sum(axis=-1)[pen, :c]
            pred[pen, :c, rows] = yh[pen, :c].astype(np.float64).T
            bound[pen, :c, rows] = mag[pen, :c].T
    return tri, scale, pred, bound


@pytest.fixture(scope="module")
def score_x(api):
    with api.SparseX(_score_data()[0]) as sx:
        yield sx


@pytest.mark.parametrize("measure", ["mse", "mae"])
@pytest.mark.parametrize("npen", [1, 3])
@pytest.mark.parametrize("nl", [1, 16, 17, 64, 65])
def test_score_against_numpy(api, score_x, nl, npen, measure):
    x, y, fid = _score_data()
    coef = np.random.default_rng(7 * nl + npen).normal(size=(S_K, npen, nl, S_P + 1)) / np.sqrt(S_P + 1.0)
    ncol = [nl] if npen == 1 else [nl, max(nl - 3, 1), 0]           # a penalty cut short, and one without a valid column
    yd, fd = _vec(y, fid)
    tri, pm = api.cv_sparse_wide_score(score_x, yd, fd, S_K, coef, ncol, type_measure=measure, predmat=True)
    ref, scale, pref, pbound = _score_reference(x, y, fid, coef, ncol, measure, (nl, npen))
    label = (nl, npen, measure)
    assert np.array_equal(tri[..., 0], ref[..., 0].astype(np.float64)), label       # counts; zero where masked and for the empty fold
    some = ref[..., 0] > 0
    assert not some[2].any() and some[0, 0].all()
    assert np.all(np.isnan(tri[..., 1:][~some])), label
    for j in (1, 2):
        gap = float(np.max(np.abs(tri[..., j][some].astype(LD) - ref[..., j][some]) / scale[..., j][some]))
        print(f"GAP {label}: triple[{j}] {gap:.1e} of its scale")
        assert gap <= 1e-12, (label, j, gap)
    assert np.all(tri[0, ..., 2][some[0]] == 0.0)                   # one row: no spread
    assert np.array_equal(np.isnan(pm), np.isnan(pref)), label
    ok = ~np.isnan(pref)
    gp = float(np.max(np.abs(pm[ok] - pref[ok]) / np.maximum(pbound[ok], 1e-300)))
    assert gp <= 1.0, (label, gp)
    tri2, pm2 = api.cv_sparse_wide_score(score_x, yd, fd, S_K, coef, ncol, type_measure=measure, predmat=True)
    assert np.array_equal(tri, tri2, equal_nan=True) and np.array_equal(pm, pm2, equal_nan=True), label
    tri3, none = api.cv_sparse_wide_score(score_x, yd, fd, S_K, coef, ncol, type_measure=measure)
    assert none is None and np.array_equal(tri, tri3, equal_nan=True), label


def test_score_leaves_another_calls_layout_alone(api, score_x):
    """a sparse and a dense cv layout on the same context: the wide scoring returns the same bits, and the layout it found is still
    the one oemgpu_cv_sparse_score_res / oemgpu_cv_score_dev accept afterwards"""
    import torch
    from oem_amd import _lib as L
    x, y, fid = _score_data()
    nl, npen = 17, 2
    coef = np.random.default_rng(5).normal(size=(S_K, npen, nl, S_P + 1)) / np.sqrt(S_P + 1.0)
    ncol = np.array([nl, nl - 3], dtype=np.int32)
    yd, fd = _vec(y, fid)
    ctx = api.context(0)
    base = api.cv_sparse_wide_score(score_x, yd, fd, S_K, coef, ncol, predmat=True, ctx=ctx)
    other = api.cv_sparse_gaussian_score(score_x, yd, fd, S_K, coef, ncol, ctx=ctx)[0]              # leaves a sparse layout in the fold buffer
    again = api.cv_sparse_wide_score(score_x, yd, fd, S_K, coef, ncol, predmat=True, ctx=ctx)
    assert np.array_equal(base[0], again[0], equal_nan=True) and np.array_equal(base[1], again[1], equal_nan=True)
    tri = np.zeros((S_K, npen, nl, 3))
    L.check(L.lib().oemgpu_cv_sparse_score_res(ctx, S_N, S_P, S_K, api._dptr(coef), npen, nl, api._iptr(ncol), 0, api._dptr(tri), None))
    assert np.array_equal(tri, other, equal_nan=True)              # not voided, not overwritten
    assert np.allclose(tri[..., 1], base[0][..., 1], rtol=1e-12, equal_nan=True)     # (the two scoring entries agree)
    xd = torch.as_tensor(np.asfortranarray(x.toarray()).T.copy(), device="cuda:0").T               # column-major n x p
    dense = api.cv_gaussian_score(xd, yd, fd, S_K, coef, ncol, ctx=ctx)[0]                          # now a dense layout
    again = api.cv_sparse_wide_score(score_x, yd, fd, S_K, coef, ncol, predmat=True, ctx=ctx)
    assert np.array_equal(base[0], again[0], equal_nan=True) and np.array_equal(base[1], again[1], equal_nan=True)
    L.check(L.lib().oemgpu_cv_score_dev(ctx, S_N, S_P, S_K, api._dptr(coef), npen, nl, api._iptr(ncol), 0, api._dptr(tri), None))
    assert np.array_equal(tri, dense, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------- C: cv_oem, oem, predict_cv
E2E_PENS = ["lasso", "grp.lasso"]
E2E_KW = dict(nlambda=12, lambda_min_ratio=0.05, tol=1e-11, maxit=4000)


@functools.lru_cache(maxsize=None)
def _e2e(n, p, K):
    """(x, y, foldid, groups, the oracle's full fit, its fold fits on the sliced data), computed once and left unchanged"""
    rng = np.random.default_rng(n + p + K)
    x = sp.random(n, p, density=0.05 if p < 1000 else 0.02, format="csc", random_state=rng, data_rvs=lambda k: rng.normal(size=k) * 1.5)
    x.sort_indices()
    b = np.zeros(p); b[np.argsort(-np.diff(x.indptr), kind="stable")[:5]] = rng.uniform(1, 2, 5)
    y = x @ b + 0.5 * rng.normal(size=n)
    fid = rng.permutation(np.resize(np.arange(1, K + 1), n))
    g = _groups(p)
    opts = dict(penalty=E2E_PENS, standardize=True, intercept=False, groups=g, unique_groups=np.unique(g), native=True, **E2E_KW)
    xr = x.tocsr()
    full = orc.fit_sparse(x, y, **opts)
    folds = [orc.fit_sparse(xr[fid != i].tocsc(), y[fid != i], **opts) for i in range(1, K + 1)]
    return x, y, fid, g, full, folds


@pytest.mark.parametrize("n,p,K", [(60, 400, 3), (65, 1100, 5)])
@pytest.mark.parametrize("measure,grouped", [("mse", True), ("mae", True), ("mse", False)])
def test_cv_oem_against_the_restatement(api, n, p, K, measure, grouped):
    import oem_amd
    x, y, fid, g, full, folds = _e2e(n, p, K)
    ref = CR.cv_oem(x.toarray(), y, fid, E2E_PENS, type_measure=measure, grouped=grouped, intercept=False, fits=(full, folds))
    for c in ref["cvm"]:                                            # no near-tie at the minimum
        s = np.sort(c)
        assert s[1] - s[0] > 1e-6 * s[0]
    yy = _vec(y, None)[0] if measure == "mae" else y                # y as a device tensor in one case
    with api.SparseX(x) as sx, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = oem_amd.cv_oem(sx, yy, intercept=False, penalty=E2E_PENS, foldid=fid, type_measure=measure, grouped=grouped, keep=True,
                           groups=g, **E2E_KW)
        assert api.last_host_path_engine() == "sparse-wide"
        for k in range(len(E2E_PENS)):
            assert f["lambda"][k].shape == ref["lambda"][k].shape and np.allclose(f["lambda"][k], ref["lambda"][k], rtol=1e-11)
            gm = float(np.max(np.abs(f["cvm"][k] - ref["cvm"][k]) / ref["cvm"][k]))
            gs = float(np.max(np.abs(f["cvsd"][k] - ref["cvsd"][k]) / ref["cvsd"][k]))
            print(f"GAP {n}x{p} {E2E_PENS[k]} {measure} grouped={grouped}: cvm {gm:.1e} cvsd {gs:.1e}")
            assert gm <= 1e-9 and gs <= 1e-8, (k, gm, gs)
            pv, pr = f["fit.preval"][k], ref["predmat"][k]
            assert pv.shape == pr.shape and np.array_equal(np.isnan(pv), np.isnan(pr))
            ok = ~np.isnan(pr)
            assert np.abs(pv[ok] - pr[ok]).max() < 1e-8 * max(1.0, float(np.abs(pr[ok]).max()))
        assert f["model.min"] - 1 == ref["model_min"] and f["best.model"] == E2E_PENS[ref["model_min"]]
        assert np.isclose(f["lambda.min"], ref["lambda_min"], rtol=1e-11)
        assert np.array_equal(f["foldid"], fid) and f["oem.fit"]["nobs"] == n
        # predict_cv: the full fit's coefficients at lambda.min, on a scipy newx and on the resident x itself
        want = CR.predict_at(full, ref["model_min"], x[:20].toarray(), np.array([ref["lambda_min"]]))
        got = oem_amd.predict_cv(f, x[:20])
        assert np.abs(np.ravel(got) - np.ravel(want)).max() < 1e-8 * max(1.0, float(np.abs(want).max()))
        got = oem_amd.predict_cv(f, sx)
        got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
        assert np.abs(np.ravel(got)[:20] - np.ravel(want)).max() < 1e-8 * max(1.0, float(np.abs(want).max()))


def test_oem_on_a_sparse_x_handle_is_oem_on_the_scipy_matrix(api, monkeypatch):
    import oem_amd
    monkeypatch.delenv("OEM_SPARSE_GRAM", raising=False)
    n, p, dens, K = M.PARITY_CASES[3]                               # 40 x 1100 at 2 %: sparse_wide_route takes it
    x, y, fid = M.parity_input(n, p, dens, K)
    kw = dict(M.PARITY_KW, penalty=PENS, groups=_groups(p), alpha=0.7, standardize=True, compute_loss=True, intercept=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = oem_amd.oem(x, y, **kw)
        assert api.last_host_path_engine() == "sparse-wide"
        with api.SparseX(x) as sx:
            g = oem_amd.oem(sx, _vec(y, None)[0], **kw)             # y on the device
            assert api.last_host_path_engine() == "sparse-wide"
            h = oem_amd.oem(sx, y, **kw)
    _same_bits(f, g)
    _same_bits(f, h)
    assert set(f) == set(g) and f["rownames"] == g["rownames"] and f["nobs"] == g["nobs"] == n


def test_python_refusals(api):
    import oem_amd
    from oem_amd import _lib as L
    n, p, dens, K = M.PARITY_CASES[0]
    x, y, fid = M.parity_input(n, p, dens, K)
    kw = dict(foldid=fid, nlambda=5, intercept=False)
    with api.SparseX(x) as sx, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for call in (lambda: oem_amd.cv_oem(sx, y, penalty="lasso", foldid=fid, nlambda=5),                 # intercept=True, the default
                     lambda: oem_amd.oem(sx, y, penalty="lasso", nlambda=5)):
            with pytest.raises(L.OemgpuError, match="p >= n and an intercept") as e:
                call()
            assert "intercept = FALSE is served" in str(e.value) and e.value.code == -4
        with pytest.raises(ValueError, match="ols"):
            oem_amd.cv_oem(sx, y, penalty=["lasso", "ols"], **kw)
        with pytest.raises(ValueError, match="weights not implemented"):
            oem_amd.cv_oem(sx, y, penalty="lasso", weights=np.ones(n), **kw)
        with pytest.raises(ValueError, match="not split over devices"):
            oem_amd.cv_oem(sx, y, penalty="lasso", ngpus=2, **kw)
        with pytest.raises(ValueError, match="not split over devices"):
            oem_amd.cv_oem(sx, y, penalty="lasso", devices=[0], **kw)
        with pytest.raises(ValueError, match="lengths do not match"):
            oem_amd.cv_oem(sx, y[:-1], penalty="lasso", **kw)
        with pytest.raises(ValueError, match="nfolds must be bigger than 3"):
            oem_amd.cv_oem(sx, y, penalty="lasso", foldid=np.resize(np.arange(1, 3), n), nlambda=5, intercept=False)
        stray = fid.copy(); stray[7] = 0
        with pytest.raises(ValueError, match="foldid must hold one integer in 1..nfolds"):
            oem_amd.cv_oem(sx, y, penalty="lasso", foldid=stray, nlambda=5, intercept=False)
    with pytest.raises(ValueError, match="closed"):
        oem_amd.cv_oem(sx, y, penalty="lasso", **kw)
    with pytest.raises(ValueError, match="closed"):
        oem_amd.oem(sx, y, penalty="lasso", nlambda=5, intercept=False)


def test_the_two_pinned_sentences_of_a_tall_handle_are_unchanged(api):
    import oem_amd
    rng = np.random.default_rng(4)
    n, p = 100, 20
    x = sp.random(n, p, density=0.3, format="csc", random_state=rng)
    y = rng.normal(size=n)
    with api.SparseX(x) as sx:
        with pytest.raises(ValueError, match="oem\\(\\) on a SparseX is not built"):
            oem_amd.oem(sx, y, penalty="lasso", nlambda=5)
        fid = np.concatenate([np.full(85, 1), np.full(8, 2), np.full(7, 3)])
        with pytest.raises(ValueError, match="fold 1 leaves 15 rows for 20 columns \\(a fit of p >= n is not served here\\)"):
            oem_amd.cv_oem(sx, y, penalty="lasso", foldid=fid, nlambda=5)
