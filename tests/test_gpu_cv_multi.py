"""cv.oem for many Gaussian responses on one resident x (cv_oem_multi; oemgpu_cv_dense_multi_dev / _rm_dev): every element
against cv_oem on its column and against tests/cv_gaussian_restatement.py fed the oracle's fits, the fold fits against cv_oem's own, the
interpolation kernel against numpy, the many-response scoring against long-double sums, route 2, the edges of the solve chunks, bytes,
fit.preval, and the call's plumbing.

Bounds (none of them this file's own): _hold (TIGHT / DTOL) of tests/test_gpu_multi.py for beta, lambda, niter, loss and d; cvm to rtol
1e-9 and cvsd to rtol 1e-8, fit.preval to 1e-8 of its scale, per-fold mean to 1e-12 and M2 to 1e-11 against long double, the fold fits to
tests/test_gpu_cv_gaussian.py's section B (d 1e-11, lambda 1e-11, beta 1e-8 of max(1, |beta|_inf)); lambda.min by _hold_min of
tests/test_gpu_xval_multi.py (the same grid position, the value to 1e-12).  The interpolation kernel: 4 eps max(|beta_left|,
|beta_right|) per entry -- two products and one sum, one product possibly fused."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests import cv_gaussian_restatement as R
from tests.test_gpu_cv_gaussian import RTOL_M, RTOL_S, _score_reference
from tests.test_gpu_multi import _hold, _same_bytes
from tests.test_gpu_rowmajor import _colmajor, _rowmajor
from tests.test_gpu_xval_multi import NF, PARITY, _PIDS, _folds, _hold_cv, _hold_min, _responses

ERR_ARG, ERR_UNSUPPORTED, ERR_INTERRUPTED = -1, -4, -6
EPS = np.finfo(np.float64).eps
KEYS = {"lambda", "cvm", "cvsd", "cvup", "cvlo", "nzero", "name", "oem.fit", "lambda.min", "lambda.1se", "model.min", "best.model", "penalty"}


@pytest.fixture(scope="module")
def oa():
    import torch
    assert torch.cuda.is_available()
    import oem_amd
    oem_amd.lib()
    return oem_amd


@pytest.fixture(scope="module")
def api(oa):
    from oem_amd import api
    return api


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _hold_cv_fit(fit, ref, loss=False):
    """an element against cv_oem's result on its column"""
    _hold(fit["oem.fit"], ref["oem.fit"], loss=loss)
    assert len(fit["lambda"]) == len(ref["lambda"])
    for k in range(len(ref["lambda"])):
        assert np.allclose(fit["lambda"][k], ref["lambda"][k], rtol=1e-12, atol=0) and fit["nzero"][k].shape == ref["nzero"][k].shape
    _hold_cv(fit, ref)
    _hold_min(fit, ref)
    assert fit["name"] == ref["name"] and fit["penalty"] == ref["penalty"]


# ------------------------------------------------------------------------------------------------ 1. parity
def _cv_case(case):
    p, pen, std, icpt, closs, groups, n, m, tm, route = case
    x, Y = _responses(n, p, m, p + len(pen))
    kw = dict(penalty=pen, nlambda=10 if p > 1000 else 12, tol=1e-9, standardize=std, intercept=icpt, compute_loss=closs, type_measure=tm)
    okw = dict(nlambda=kw["nlambda"], tol=1e-9, compute_loss=closs, lambda_min_ratio=1e-4)
    if groups is not None:
        kw["groups"] = groups
        okw.update(groups=np.asarray(groups), unique_groups=np.unique(groups))
    return x, Y, _folds(n, NF, p), kw, okw


@pytest.mark.parametrize("case", PARITY, ids=_PIDS)
def test_parity_with_cv_oem_and_the_restatement(oa, case):
    import torch
    p, pen, std, icpt, closs, groups, n, m, tm, route = case
    x, Y, fid, kw, okw = _cv_case(case)
    pens = [pen] if isinstance(pen, str) else list(pen)
    grouped = PARITY.index(case) % 2 == 0                                 # both forms of cvcompute over the cases
    xc = _colmajor(x)
    fits = oa.cv_oem_multi(xc, torch.as_tensor(Y, device="cuda"), foldid=fid, grouped=grouped, **kw)
    assert len(fits) == m and [f["route"] for f in fits] == [route] * m
    assert not np.allclose(fits[0]["lambda"][0], fits[1]["lambda"][0], rtol=1e-3)          # every response on its own grid
    for r in range(m):
        one = oa.cv_oem(xc, Y[:, r], foldid=fid, grouped=grouped, **kw)
        assert KEYS <= set(one) and set(fits[r]) == set(one) | {"route"}
        _hold_cv_fit(fits[r], one, loss=closs)
        ref = R.cv_oem(x, Y[:, r], fid, pens, type_measure=tm, grouped=grouped, standardize=std, intercept=icpt, **okw)
        _hold(fits[r]["oem.fit"], ref["fits"][0], loss=closs, niter=False)
        for k in range(len(pens)):
            assert np.allclose(fits[r]["lambda"][k], ref["lambda"][k], rtol=1e-12, atol=0)
            gm = float(np.max(np.abs(fits[r]["cvm"][k] - ref["cvm"][k]) / ref["cvm"][k]))
            gs = float(np.max(np.abs(fits[r]["cvsd"][k] - ref["cvsd"][k]) / ref["cvsd"][k]))
            print(f"GAP cv_multi p = {p} {pens[k]} {tm} grouped={grouped} response {r}: cvm {gm:.1e} cvsd {gs:.1e} to the restatement")
            assert gm <= 1e-9 and gs <= 1e-8, (r, k, gm, gs)
    assert np.asarray(oa.predict_cv(fits[0], x[:7])).shape[0] == 7
    assert oa.summary_cv(fits[0]) is not None


def test_parity_user_lambda_and_the_other_grouping(oa):
    """a user lambda is shared by the responses and by every fold: nothing is interpolated, no column is masked"""
    import torch
    n, p, m = 3000, 41, 5
    x, Y = _responses(n, p, m, 17)
    fid, xc = _folds(n, NF, 18), _colmajor(x)
    lam = [np.geomspace(2.0, 2e-3, 11), np.geomspace(1.0, 5e-3, 11)]
    for grouped, tm in [(True, "mae"), (False, "mse")]:
        kw = dict(penalty=["lasso", "mcp"], lambda_=lam, tol=1e-9, type_measure=tm, grouped=grouped)
        fits = oa.cv_oem_multi(xc, torch.as_tensor(Y, device="cuda"), foldid=fid, **kw)
        for r in range(m):
            assert [len(c) for c in fits[r]["cvm"]] == [11, 11]
            assert all(np.array_equal(fits[r]["lambda"][k], lam[k]) for k in range(2))
            _hold_cv_fit(fits[r], oa.cv_oem(xc, Y[:, r], foldid=fid, **kw))


# ------------------------------------------------------------------------------------------------ 2. fold fits
N2, P2, K2, M2 = 1201, 23, 5, 3
GROUPS2 = np.arange(P2) // 4 + 1
PENS2 = ["lasso", "mcp", "grp.lasso"]


def _fold_case(api, std, icpt, lam=()):
    x, Y = _responses(N2, P2, M2, 31)
    fid = _folds(N2, K2, 32)
    kw = dict(standardize=std, intercept=icpt, groups=GROUPS2, tol=1e-10, maxit=2000, **({} if len(lam) else {"nlambda": 21}))
    xc = _colmajor(x)
    a, varnames, s_, i_ = api.oem(xc, Y, penalty=PENS2, lambda_=lam, _args_only=True, **kw)
    out = api._cv_multi_call(xc, Y, np.ascontiguousarray(fid, dtype=np.int32), K2, a, s_, i_, "mse", False, fold_fits=True)
    return x, Y, fid, xc, kw, out


@pytest.mark.parametrize("std,icpt", [(True, True), (False, True), (True, False), (False, False)])
def test_fold_fits_are_those_of_cv_oem(api, std, icpt):
    x, Y, fid, xc, kw, out = _fold_case(api, std, icpt)
    assert out["route"].tolist() == [0] * M2
    assert out["fold_n"].tolist() == [int((fid == i).sum()) for i in range(1, K2 + 1)]
    worst = 0.0
    for r in range(M2):
        outlist, dev = api._cv_gaussian_fold_fits(xc, Y[:, r], fid, K2, PENS2, (), kw)
        for i, ref in enumerate(outlist):
            for k in range(len(PENS2)):
                assert np.allclose(out["fold_lambda"][r, i, k], ref["lambda"][k], rtol=1e-11, atol=0), (r, i, k)
                b = np.asarray(ref["beta"][k])                                           # (p + 1) x nl
                scale = max(1.0, float(np.abs(b).max()))
                gap = float(np.abs(out["fold_beta"][r, i, k].T - b).max()) / scale
                worst = max(worst, gap)
                assert gap < 1e-8, (r, i, k, gap)
                assert np.abs(out["fold_niter"][r, i, k].astype(int) - np.ravel(ref["niter"][k]).astype(int)).max() <= 1
    print(f"GAP cv_multi fold fits standardize={std} intercept={icpt}: beta {worst:.1e} of max(1, |beta|_inf)")


def test_an_absent_fold_is_the_full_fit_and_scores_nothing(oa, api):
    n, p, m = 600, 7, 2
    x, Y = _responses(n, p, m, 33)
    fid = np.resize(np.array([1, 2, 4, 5]), n)                            # nfolds = 5, no row in fold 3
    xc = _colmajor(x)
    a, _, s_, i_ = api.oem(xc, Y, penalty=["lasso"], nlambda=9, tol=1e-10, _args_only=True)
    out = api._cv_multi_call(xc, Y, np.ascontiguousarray(fid, dtype=np.int32), 5, a, s_, i_, "mse", False, fold_fits=True)
    assert out["fold_n"].tolist() == [150, 150, 0, 150, 150]
    for r in range(m):
        assert np.array_equal(out["fold_lambda"][r, 2], out["lambda"][r]) and np.array_equal(out["fold_beta"][r, 2], out["beta"][r])
        t = out["triples"][r, 2]
        assert np.all(t[..., 0] == 0) and np.all(np.isnan(t[..., 1:]))
    fits = oa.cv_oem_multi(xc, Y, foldid=fid, penalty="lasso", nlambda=9, tol=1e-10)
    for r in range(m):
        _hold_cv_fit(fits[r], oa.cv_oem(xc, Y[:, r], foldid=fid, penalty="lasso", nlambda=9, tol=1e-10))


def test_fold_refusals_from_the_device(oa, api):
    n, p, m = 60, 5, 2
    x, Y = _responses(n, p, m, 25)
    xc = _colmajor(x)
    fid = np.ones(n, dtype=np.int32)
    fid[:3], fid[3:5] = 2, 3                                              # fold 1 holds 55 rows: its fit would keep 5 <= p
    a, _, s_, i_ = api.oem(xc, Y, penalty=["lasso"], nlambda=5, _args_only=True)
    with pytest.raises(oa.OemgpuError) as e:
        api._cv_multi_call(xc, Y, fid, 3, a, s_, i_, "mse", False)
    assert e.value.code == ERR_UNSUPPORTED and "fold 1 leaves 5 rows for 5 columns" in str(e.value)
    bad = np.ascontiguousarray(_folds(n, 3, 26), dtype=np.int32)
    bad[7] = 0
    with pytest.raises(oa.OemgpuError) as e:
        api._cv_multi_call(xc, Y, bad, 3, a, s_, i_, "mse", False)
    assert e.value.code == ERR_ARG and "foldid" in str(e.value)
    assert len(oa.cv_oem_multi(xc, Y, foldid=_folds(n, 3, 26), penalty="lasso", nlambda=5)) == m       # the same context serves the next call


# ------------------------------------------------------------------------------------------------ 3. the interpolation kernel
def _interp_case(api, p, nl, seed):
    from tests.test_cv_multi_cpu import _fits_of, _grids
    n, K, m, npen = 400, 3, 3, 2
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, p)); Y = rng.normal(size=(n, m))
    fid = _folds(n, K, seed + 1)
    raw = rng.normal(size=(m, K, npen, nl, p + 1))
    full, fold, idx = [], [], []
    for r in range(m):
        f0, fk = _grids(rng, K, npen, nl)
        full.append(f0); fold.append(fk); idx.append(api.cv_multi_interp_table(f0, fk))
    left, right, frac = (np.stack([i[j] for i in idx]) for j in range(3))
    ncol = np.stack([i[3] for i in idx])
    return x, Y, fid, raw, full, fold, left, right, frac, ncol, _fits_of


@pytest.mark.parametrize("nl", [7, 16, 17, 100])
@pytest.mark.parametrize("p", [5, 57])
def test_interpolation_kernel(api, p, nl):
    x, Y, fid, raw, full, fold, left, right, frac, ncol, fits_of = _interp_case(api, p, nl, 1000 * p + nl)
    m, K, npen = raw.shape[:3]
    tri, tab = api.cv_multi_score(_colmajor(x), Y, fid, K, raw, ncol, nb=2, interp=(left, right, frac))
    assert tab.shape == raw.shape and not np.isnan(tab).any()
    worst = worst_ref = 0.0
    for r in range(m):
        which = [np.arange(nl) < ncol[r, k] for k in range(npen)]
        ref, ncol_ref = api._cv_gaussian_table(fits_of(fold[r], raw[r], p), list(full[r]), which, p)
        assert np.array_equal(ncol_ref, ncol[r])
        for i in range(K):
            for k in range(npen):
                c = ncol[r, k]
                assert np.all(tab[r, i, k, c:] == 0.0)                                   # rows from ncol on are zero
                bl, br = raw[r, i, k, left[r, i, k, :c]], raw[r, i, k, right[r, i, k, :c]]
                f = frac[r, i, k, :c, None]
                bound = 4 * EPS * np.maximum(np.abs(bl), np.abs(br))
                gap = np.abs(tab[r, i, k, :c] - (bl * f + br * (1 - f)))
                worst = max(worst, float(np.max(gap / np.maximum(bound, 1e-300))) if c else 0.0)
                assert np.all(gap <= bound), (r, i, k)
                # and against predict()'s own interpolation of the same fold fits (_cv_gaussian_table), to the same bound
                gref = np.abs(tab[r, i, k, :c] - ref[i, k, :c])
                worst_ref = max(worst_ref, float(np.max(gref / np.maximum(bound, 1e-300))) if c else 0.0)
                assert np.all(gref <= bound) and np.all(ref[i, k, c:] == 0.0), (r, i, k)
    print(f"GAP cv_interp p = {p} nl = {nl}: {worst:.2f} of 4 eps max(|b_left|, |b_right|) to numpy on the table's indices, {worst_ref:.2f} of it to _cv_gaussian_table")


def test_interpolation_on_a_shared_grid_passes_the_tables_through(api):
    n, p, K, m, npen, nl = 400, 9, 3, 2, 2, 17
    rng = np.random.default_rng(5)
    x, Y, fid = rng.normal(size=(n, p)), rng.normal(size=(n, m)), _folds(n, K, 6)
    raw = rng.normal(size=(m, K, npen, nl, p + 1))
    full = np.stack([np.geomspace(1.5, 2e-3, nl), np.geomspace(1.0, 1e-3, nl)])
    left, right, frac, ncol = api.cv_multi_interp_table(full, np.broadcast_to(full, (K, npen, nl)).copy())
    rep = lambda a: np.stack([a] * m)
    tri, tab = api.cv_multi_score(_colmajor(x), Y, fid, K, raw, rep(ncol), nb=2, interp=(rep(left), rep(right), rep(frac)))
    assert np.array_equal(tab, raw)
    tri2, none = api.cv_multi_score(_colmajor(x), Y, fid, K, raw, rep(ncol), nb=2)          # the same tables, not interpolated
    assert none is None and np.array_equal(tri, tri2, equal_nan=True)


# ------------------------------------------------------------------------------------------------ 4. scoring with a response dimension
# (p, nl, nb, form, measure)
SCORE = [(20, 5, 1, "single", "mse"), (20, 16, 3, "single", "mae"), (20, 17, 17, "single", "mse"), (20, 100, 3, "single", "mae"),
         (80, 17, 3, "multi", "mse"), (80, 100, 1, "multi", "mae"), (80, 5, 17, "multi", "mse"), (80, 16, 1, "multi", "mse"),
         (170, 100, 1, "chunk", "mse"), (170, 100, 3, "chunk", "mae"), (170, 100, 17, "chunk", "mse")]


@pytest.mark.parametrize("p,nl,nb,form,measure", SCORE, ids=[f"p{c[0]}-nl{c[1]}-nb{c[2]}-{c[4]}" for c in SCORE])
def test_scoring_with_a_response_dimension(api, p, nl, nb, form, measure):
    import torch
    K, npen = 5, 2
    m = nb + 1 if nb == 3 else nb                                         # (nb = 3: a second launch of one response)
    sizes = [37, 1, 50, 0, 23]                                            # off every 16-row tile; a fold of one row; an empty fold
    n = sum(sizes)
    assert api.xval_cv_plan(n, p, K, npen, nl, _cus())["form"] == form
    rng = np.random.default_rng(100 * p + nl + nb)
    fid = rng.permutation(np.repeat(np.arange(1, K + 1), sizes))
    x, Y = rng.normal(size=(n, p)), rng.normal(size=(n, m))
    # The fold of one row: its mean IS one residual, and the bound is relative to it.  Among m npen nl residuals of size ~1 some lie
    # within 1e-3 of zero, where the rounding of yhat alone ((p + 2) eps |b||x|) is 1e-12 of the residual in any float64 evaluation
    # (numpy's included).  That row's y is moved 6 away, so that every residual of it keeps its size; the other folds keep both signs.
    Y[fid == 2] += 6.0
    coef = rng.normal(size=(m, K, npen, nl, p + 1)) / np.sqrt(p + 1.0)
    ncol = rng.integers(1, nl + 1, size=(m, npen)).astype(np.int32)
    ncol[0] = (0, nl)                                                     # nothing valid for one penalty, everything for the other
    ncol[-1] = (nl, 0) if m > 1 else ncol[-1]
    guard = 3 * nl + 5
    buf = torch.full((m * npen * nl * n + 2 * guard,), float("nan"), dtype=torch.float64, device="cuda")
    block = buf[guard:guard + m * npen * nl * n]
    block.fill_(12345.0)
    tri, none = api.cv_multi_score(_colmajor(x), Y, fid, K, coef, ncol, type_measure=measure, nb=nb, predmat=block)
    assert none is None
    host = buf.cpu().numpy()
    assert np.all(np.isnan(host[:guard])) and np.all(np.isnan(host[-guard:]))              # nothing outside the block
    pm = host[guard:-guard].reshape(m, npen, nl, n)
    assert not np.any(pm == 12345.0)                                      # every caller's row of every column written
    gm = gs = gp = 0.0
    for r in range(m):
        ref, pref, pbound = _score_reference(x, Y[:, r], fid, coef[r], ncol[r], measure)
        some, many = ref[..., 0] > 0, ref[..., 0] > 1
        assert np.array_equal(tri[r, ..., 0], ref[..., 0].astype(np.float64)), r
        assert np.all(np.isnan(tri[r, ..., 1][~some])) and np.all(np.isnan(tri[r, ..., 2][~some])), r
        gm = max(gm, float(np.max(np.abs(tri[r, ..., 1][some].astype(np.longdouble) - ref[..., 1][some]) / np.abs(ref[..., 1][some]))))
        if many.any():
            gs = max(gs, float(np.max(np.abs(tri[r, ..., 2][many].astype(np.longdouble) - ref[..., 2][many]) / ref[..., 2][many])))
        assert np.all(tri[r, ..., 2][some & ~many] == 0.0), r
        assert np.array_equal(np.isnan(pm[r]), np.isnan(pref)), r         # NaN exactly in the columns >= that response's ncol
        ok = ~np.isnan(pref)
        gp = max(gp, float(np.max(np.abs(pm[r][ok] - pref[ok]) / np.maximum(pbound[ok], 1e-300))))
    print(f"GAP cv_multi score p = {p} nl = {nl} nb = {nb} {measure}: fold mean {gm:.1e} fold M2 {gs:.1e} yhat {gp:.2f} of its bound")
    assert gm <= RTOL_M and gs <= RTOL_S and gp <= 1.0, (gm, gs, gp)
    tri2, _ = api.cv_multi_score(_colmajor(x), Y, fid, K, coef, ncol, type_measure=measure, nb=nb)      # without the store: the same bits
    assert np.array_equal(tri, tri2, equal_nan=True)


def test_single_response_scoring_is_what_it_was(api):
    """nresp = 1: the many-response launch of one response writes the bytes of oemgpu_selftest_cv_score_dev"""
    import torch
    n, p, K, npen, nl = 333, 23, 4, 2, 21
    rng = np.random.default_rng(44)
    x, y, fid = rng.normal(size=(n, p)), rng.normal(size=n), _folds(n, K, 45)
    coef = rng.normal(size=(K, npen, nl, p + 1)) / 5.0
    ncol = np.array([nl, 7], dtype=np.int32)
    xc = _colmajor(x)
    for measure in ("mse", "mae"):
        t1, pm1 = api.cv_gaussian_score(xc, torch.as_tensor(y, device="cuda"), torch.as_tensor(fid.astype(np.int32), device="cuda"), K, coef, ncol,
                                        type_measure=measure, predmat=True)
        block = torch.zeros(npen * nl * n, dtype=torch.float64, device="cuda")
        tm, _ = api.cv_multi_score(xc, y[:, None], fid, K, coef[None], ncol[None], type_measure=measure, nb=1, predmat=block)
        assert np.array_equal(tm[0], t1, equal_nan=True)
        assert np.array_equal(block.cpu().numpy().reshape(npen, nl, n), pm1, equal_nan=True)


# ------------------------------------------------------------------------------------------------ 5. route 2
def test_one_response_that_advises_a_shift(oa):
    n, p, m = 2000, 20, 3
    x, Y = _responses(n, p, m, 61)
    Y[:, 1] += 100.0 * Y[:, 1].std()                                      # mean^2 > 256 var: finalize_kernel's predicate
    assert Y[:, 1].mean() ** 2 > 256 * Y[:, 1].var()
    xc, fid = _colmajor(x), _folds(n, NF, 62)
    kw = dict(foldid=fid, penalty=["lasso", "mcp"], nlambda=12, tol=1e-9, keep=True)
    fits = oa.cv_oem_multi(xc, Y, **kw)
    assert [f["route"] for f in fits] == [0, 2, 0]
    one = oa.cv_oem(xc, Y[:, 1], **kw)
    assert set(fits[1]) == set(one) | {"route"}
    _same_bytes(dict(fits[1]["oem.fit"], route=0), dict(one["oem.fit"], route=0))
    for key in ("cvm", "cvsd", "lambda", "fit.preval"):
        for k in range(2):
            assert np.asarray(fits[1][key][k]).tobytes() == np.asarray(one[key][k]).tobytes(), key
    assert fits[1]["lambda.min"] == one["lambda.min"] and fits[1]["lambda.1se"] == one["lambda.1se"]
    for r in (0, 2):
        _hold_cv_fit(fits[r], oa.cv_oem(xc, Y[:, r], **kw))
    # a device Y: the column handed to cv_oem is then a strided view of it -- the same results, bit for bit
    import torch
    dev = oa.cv_oem_multi(xc, torch.as_tensor(Y, device="cuda"), **kw)
    assert [f["route"] for f in dev] == [0, 2, 0]
    for r in range(m):
        _same_cv_bytes(fits[r], dev[r], keep=True)


def test_an_x_that_advises_a_shift_sends_every_response_to_cv_oem(oa):
    n, p, m = 2000, 20, 3
    x, Y = _responses(n, p, m, 63)
    x[:, 4] += 100.0 * x[:, 4].std()
    x = x.astype(np.float32).astype(np.float64)
    xc, fid = _colmajor(x), _folds(n, NF, 64)
    kw = dict(foldid=fid, penalty="lasso", nlambda=12, tol=1e-9)
    fits = oa.cv_oem_multi(xc, Y, **kw)
    assert [f["route"] for f in fits] == [2] * m
    for r in range(m):
        one = oa.cv_oem(xc, Y[:, r], **kw)
        assert np.asarray(fits[r]["cvm"][0]).tobytes() == np.asarray(one["cvm"][0]).tobytes()
        _same_bytes(dict(fits[r]["oem.fit"], route=0), dict(one["oem.fit"], route=0))


# ------------------------------------------------------------------------------------------------ 6. chunk edges
def _hold_alone(oa, xc, Y, fits, kw, loss=False):
    """every element against the call on its column alone (m = 1)"""
    for r, f in enumerate(fits):
        alone = oa.cv_oem_multi(xc, Y[:, r:r + 1], **kw)[0]
        _hold_cv_fit(f, alone, loss=loss)


def test_solve_chunk_edges_small_p(oa, api):
    n, p, K = 600, 8, 4
    plan = api.cv_multi_plan(n, p, K, 1000, nl=5, num_cu=_cus())
    nb = plan["nb"]
    assert nb == plan["cap"] // (K + 1) and nb * (K + 1) <= 513 < (nb + 1) * (K + 1)
    x, Y = _responses(n, p, nb + 1, 51)
    Y = Y / (1.0 + np.arange(nb + 1)) * (1.0 + np.arange(nb + 1) % 7)     # (scales 1..7: every grid finite and its own)
    xc, fid = _colmajor(x), _folds(n, K, 52)
    kw = dict(foldid=fid, penalty="lasso", nlambda=5, tol=1e-9)
    alone = [oa.cv_oem_multi(xc, Y[:, r:r + 1], **kw)[0] for r in range(nb + 1)]
    for m in (nb - 1, nb, nb + 1):                                        # just below, at and one past a full chunk
        assert api.cv_multi_plan(n, p, K, m, nl=5, num_cu=_cus())["solve_chunks"] == (2 if m > nb else 1)
        fits = oa.cv_oem_multi(xc, Y[:, :m], **kw)
        assert [f["route"] for f in fits] == [0] * m
        for r in range(m):
            _hold_cv_fit(fits[r], alone[r])


def test_solve_chunk_edges_cooperating_engine(oa, api):
    n, p, K = 1200, 250, 3
    plan = api.cv_multi_plan(n, p, K, 100, nl=5, num_cu=_cus())
    nb = plan["nb"]
    assert plan["engine"] == 2 and 1 <= nb <= 16
    x, Y = _responses(n, p, nb + 1, 53)
    xc, fid = _colmajor(x), _folds(n, K, 54)
    kw = dict(foldid=fid, penalty="lasso", nlambda=5, tol=1e-9)
    alone = [oa.cv_oem_multi(xc, Y[:, r:r + 1], **kw)[0] for r in range(nb + 1)]
    for m in (nb, nb + 1):
        fits = oa.cv_oem_multi(xc, Y[:, :m], **kw)
        assert [f["route"] for f in fits] == [0] * m
        for r in range(m):
            _hold_cv_fit(fits[r], alone[r])


# ------------------------------------------------------------------------------------------------ 7. bytes
def _same_cv_bytes(a, b, keep=False):
    _same_bytes(dict(a["oem.fit"], route=a["route"]), dict(b["oem.fit"], route=b["route"]))
    for key in ("lambda", "cvm", "cvsd", "nzero") + (("fit.preval",) if keep else ()):
        for k in range(len(a[key])):
            assert np.asarray(a[key][k]).tobytes() == np.asarray(b[key][k]).tobytes(), (key, k)
    assert a["lambda.min"] == b["lambda.min"] and a["lambda.1se"] == b["lambda.1se"] and a["model.min"] == b["model.min"]


@pytest.mark.parametrize("case", [PARITY[1], PARITY[4]], ids=[_PIDS[1], _PIDS[4]])
def test_same_bytes(oa, case):
    import torch
    p, pen, std, icpt, closs, groups, n, m, tm, route = case
    x, Y, fid, kw, okw = _cv_case(case)                                   # (x holds float32 values)
    Yd = torch.as_tensor(Y, device="cuda")
    first = oa.cv_oem_multi(_colmajor(x), Yd, foldid=fid, keep=True, **kw)
    others = [oa.cv_oem_multi(_colmajor(x), Yd, foldid=fid, keep=True, **kw),               # two calls
              oa.cv_oem_multi(_rowmajor(x, "f64", 3), Yd, foldid=fid, keep=True, **kw),     # a row-major float64 x, read in place
              oa.cv_oem_multi(_rowmajor(x, "f32", 5), Yd, foldid=fid, keep=True, **kw),     # a row-major float32 x
              oa.cv_oem_multi(_colmajor(x), Y, foldid=fid, keep=True, **kw)]                # a host Y
    for other in others:
        for r in range(m):
            _same_cv_bytes(first[r], other[r], keep=True)


# ------------------------------------------------------------------------------------------------ 8. keep = True
def test_fit_preval_against_cv_oem_across_chunks(oa, api):
    """p = 250 on the cooperating engine: few responses per chunk, so m = nb + 1 brings the predictions down in two copies"""
    n, p, K = 1200, 250, 3
    nb = api.cv_multi_plan(n, p, K, 100, nl=6, num_cu=_cus(), keep=True)["nb"]
    m = nb + 1
    x, Y = _responses(n, p, m, 81)
    xc, fid = _colmajor(x), _folds(n, K, 82)
    kw = dict(foldid=fid, penalty="lasso", nlambda=6, tol=1e-9, keep=True)
    fits = oa.cv_oem_multi(xc, Y, **kw)
    again = oa.cv_oem_multi(xc, Y, **kw)
    for r in (0, nb - 1, nb):                                             # the first chunk's ends and the second chunk's response
        one = oa.cv_oem(xc, Y[:, r], **kw)
        assert set(fits[r]) == set(one) | {"route"} and np.array_equal(fits[r]["foldid"], fid)
        pv, pr = fits[r]["fit.preval"][0], one["fit.preval"][0]
        assert pv.shape == pr.shape == (n, 6) and np.array_equal(np.isnan(pv), np.isnan(pr))
        ok = ~np.isnan(pr)
        assert np.abs(pv[ok] - pr[ok]).max() < 1e-8 * max(1.0, float(np.abs(pr[ok]).max()))
        _same_cv_bytes(fits[r], again[r], keep=True)


@pytest.mark.parametrize("limit", [1, 2])
def test_a_smaller_chunk_brings_the_same_predictions_down(oa, api, limit):
    """nb forced down as the device's free memory would force it (oemgpu_selftest_cv_multi_nb_limit): m = 5 responses in chunks of 5,
    of 2 + 2 + 1 and of one.  The fits and yhat do not depend on the chunk -- the same bytes; the fold statistics do in their last
    bits (the scoring launch divides the CUs among the chunk's responses, and with them the order of its partial sums): to cvm's bound"""
    n, p, K, m = 1203, 41, 3, 5
    x, Y = _responses(n, p, m, 83)
    xc, fid = _colmajor(x), _folds(n, K, 84)
    kw = dict(foldid=fid, penalty=["lasso", "mcp"], nlambda=7, tol=1e-9, keep=True)
    assert api.cv_multi_plan(n, p, K, m, 2, 7, _cus(), keep=True)["nb"] == m
    assert api.cv_multi_plan(n, p, K, m, 2, 7, _cus(), keep=True, nb_limit=limit)["solve_chunks"] == -(-m // limit)
    whole = oa.cv_oem_multi(xc, Y, **kw)
    api.cv_multi_nb_limit(limit)
    try:
        parts = oa.cv_oem_multi(xc, Y, **kw)
    finally:
        api.cv_multi_nb_limit(0)
    for r in range(m):
        _same_bytes(dict(whole[r]["oem.fit"], route=0), dict(parts[r]["oem.fit"], route=0))
        for k in range(2):
            assert whole[r]["fit.preval"][k].shape == (n, 7) and np.isfinite(whole[r]["fit.preval"][k][:, 0]).all()
            assert whole[r]["fit.preval"][k].tobytes() == parts[r]["fit.preval"][k].tobytes(), (r, k)
        _hold_cv(parts[r], whole[r])
        _hold_min(parts[r], whole[r])


# ------------------------------------------------------------------------------------------------ 9. plumbing
def test_fewer_than_three_rows_per_fold_warns_and_ungroups(oa):
    n, p, m = 11, 2, 2
    x, Y = _responses(n, p, m, 91, )
    xc, fid = _colmajor(x), np.resize(np.arange(1, 5), n)
    kw = dict(foldid=fid, penalty="lasso", nlambda=5)
    with pytest.warns(UserWarning, match="grouped=FALSE enforced") as w:
        fits = oa.cv_oem_multi(xc, Y, grouped=True, **kw)
    assert sum("grouped=FALSE enforced" in str(i.message) for i in w) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rows = oa.cv_oem_multi(xc, Y, grouped=False, **kw)
    for r in range(m):
        assert np.array_equal(fits[r]["cvm"][0], rows[r]["cvm"][0]) and np.array_equal(fits[r]["cvsd"][0], rows[r]["cvsd"][0])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _hold_cv_fit(fits[r], oa.cv_oem(xc, Y[:, r], grouped=True, **kw))


def test_interrupt_between_chunks(oa, api):
    n, p, K = 600, 8, 4
    nb = api.cv_multi_plan(n, p, K, 1000, nl=5, num_cu=_cus())["nb"]
    x, Y = _responses(n, p, nb + 1, 72)
    Y = Y / (1.0 + np.arange(nb + 1))
    xc, fid = _colmajor(x), _folds(n, K, 73)
    calls = []

    def fire():
        calls.append(1)
        return True

    with pytest.raises(oa.OemgpuError) as e:
        oa.cv_oem_multi(xc, Y, foldid=fid, penalty="lasso", nlambda=5, interrupt=fire)
    assert e.value.code == ERR_INTERRUPTED and len(calls) == 1            # polled once: behind the first chunk
    fits = oa.cv_oem_multi(xc, Y[:, :2], foldid=fid, penalty="lasso", nlambda=5)          # the same context serves the next call
    for r in range(2):
        _hold_cv_fit(fits[r], oa.cv_oem(xc, Y[:, r], foldid=fid, penalty="lasso", nlambda=5))


def test_phase_clock(oa, api):
    n, p, K = 600, 8, 4
    nb = api.cv_multi_plan(n, p, K, 1000, nl=5, num_cu=_cus())["nb"]
    x, Y = _responses(n, p, nb + 1, 74)
    Y = Y / (1.0 + np.arange(nb + 1))
    xc, fid = _colmajor(x), _folds(n, K, 75)
    lib, ctx = oa.lib(), api.context()
    names = {"fold_order", "fold_gram", "fold_xty", "compose", "paths", "interp", "score"}
    assert lib.oemgpu_set_timing(ctx, 1) == 0
    try:
        oa.cv_oem_multi(xc, Y[:, :nb], foldid=fid, penalty="lasso", nlambda=5)
        one = api.cv_multi_timings()
        oa.cv_oem_multi(xc, Y, foldid=fid, penalty="lasso", nlambda=5)
        two = api.cv_multi_timings()
    finally:
        assert lib.oemgpu_set_timing(ctx, 0) == 0
    assert set(one) == names and all(v > 0.0 for v in one.values()), one
    assert all(v > 0.0 for v in two.values()), two
    print(f"GAP cv_multi clock: one chunk {one}; two chunks {two}")
    oa.cv_oem_multi(xc, Y[:, :2], foldid=fid, penalty="lasso", nlambda=5)
    assert all(v == 0.0 for v in api.cv_multi_timings().values())         # timing off: nothing waits, nothing is reported


def test_phase_clock_adds_up_over_chunks(oa, api):
    """Twelve responses one per chunk (nb limited to 1) against one response alone: the four phases that run once per chunk report at
    least four times the single call's -- twelve chunks of the same work, a factor of three left for the clock's noise; a clock that
    kept only the last chunk's time would report about one.  The three phases before the chunks run once in both."""
    n, p, K, m = 3000, 41, 4, 12
    x, Y = _responses(n, p, m, 76)
    Y = Y / (1.0 + np.arange(m))                                           # (the same scale: every chunk the same work)
    xc, fid = _colmajor(x), _folds(n, K, 77)
    kw = dict(foldid=fid, penalty="lasso", nlambda=12)
    lib, ctx = oa.lib(), api.context()
    per_chunk = ["compose", "paths", "interp", "score"]
    oa.cv_oem_multi(xc, Y, **kw)                                          # (buffers and code objects exist from here on)
    assert lib.oemgpu_set_timing(ctx, 1) == 0
    api.cv_multi_nb_limit(1)
    try:
        alone = []
        for _ in range(3):
            oa.cv_oem_multi(xc, Y[:, :1], **kw)
            alone.append(api.cv_multi_timings())
        oa.cv_oem_multi(xc, Y, **kw)
        many = api.cv_multi_timings()
    finally:
        api.cv_multi_nb_limit(0)
        assert lib.oemgpu_set_timing(ctx, 0) == 0
    one = {k: min(a[k] for a in alone) for k in many}
    print(f"GAP cv_multi clock: one response {one}; twelve chunks of one {many}")
    for k in per_chunk:
        assert many[k] >= 4.0 * one[k], (k, many[k], one[k])


def test_device_memory_of_a_call_is_the_plans(oa, api):
    """A call without keep on a context of its own, made for this test: the device's free memory (hipMemGetInfo through torch) falls by no
    more than the plan's figure plus the size of x -- the buffer of the call is the plan's, x is read where it lies (a row-major float32
    tensor: no float64 copy through torch either), and what else a first call allocates (the path workspace, Y's and foldid's place in
    torch's pool) fits the allowance of one x.  The fall is also at least half the plan's figure: the measurement sees the buffer."""
    import torch
    n, p, m = 60_000, 64, 4
    rng = np.random.default_rng(71)
    x = torch.as_tensor(rng.normal(size=(n, p)), device="cuda").float()
    Y = torch.as_tensor(rng.normal(size=(n, m)), device="cuda")
    fid = np.resize(np.arange(1, NF + 1), n)
    before = x.clone()
    plan = api.cv_multi_plan(n, p, NF, m, 1, 10, _cus())
    key = (torch.cuda.current_device(), None)
    shared = api._ctx_cache.pop(key, None)                                # (the other tests' context, with buffers of their sizes)
    try:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.max_memory_allocated()
        free0 = torch.cuda.mem_get_info()[0]
        fits = oa.cv_oem_multi(x, Y, foldid=fid, penalty="lasso", nlambda=10)
        torch.cuda.synchronize()
        used = free0 - torch.cuda.mem_get_info()[0]
        grown = torch.cuda.max_memory_allocated() - base
    finally:
        own = api._ctx_cache.pop(key, None)
        if own is not None:
            oa.lib().oemgpu_destroy(own)
        if shared is not None:
            api._ctx_cache[key] = shared
    print(f"GAP cv_oem_multi row-major f32: free device memory fell by {used}, the plan's buffer {plan['bytes']} + x {n * p * 4}; "
          f"torch's peak grew by {grown}")
    assert used <= plan["bytes"] + n * p * 4, (used, plan["bytes"])
    assert used >= plan["bytes"] // 2, (used, plan["bytes"])
    assert grown < n * p * 4
    assert all(np.all(np.isfinite(f["cvm"][0])) for f in fits) and torch.equal(x, before)
