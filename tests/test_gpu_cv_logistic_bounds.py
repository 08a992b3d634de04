"""cv.oem for binomial fits on the MI355X at the limits of its two entries (the cases of tests/test_gpu_cv_logistic.py sit inside them).

The scoring entry (oemgpu_logistic_cv_score_dev) against numpy: workgroups that walk more than one 64-row tile, with random folds,
contiguous folds (most tiles skipped, some shared by two folds) and a fold of one row; x with ld > n; probabilities that saturate at both
clamps, at exactly 1 and at exactly 0; both sides of the table-in-LDS limit, reached through ncol and through p; the p > 8191 refusal;
every shape of the waves' column groups; a fold with no row; recoded y levels.  Each case first asks oemgpu_selftest_cv_score_plan, with
the live CU count, whether its shape lands where it is named for; _check_scores then holds the tolerances and the precondition of
tests/test_gpu_cv_logistic.py (class sums and counts exact, deviance / mse / mae sums rtol 1e-10, predmat 1e-12, the same bits from a
second call; min |prob - 0.5| > 1e-7 on numpy's side; seeds were picked on the CPU so that it holds).

The fold entry (oemgpu_fit_logistic_dense_fold_dev) against the restatement on the gathered rows: the kept-row map of the W floor
beyond the first 1024 rows of foldid; left-out rows that hold other values, or NaN, and must not move a bit; ld > n; the p + intercept
>= n_eff refusal at equality.  And cv_oem(family="binomial") end to end on the near-separable case, where the full fit's lambdas are
trimmed and the fold fits reach the loss clamps.

Preconditions are asserted on the reference side only and exclude no case.  A fold id is in 1 .. nfolds or the entries refuse it
(test_fold_entry_refusals_from_the_device), so a row that no fold scores cannot arise: with predmat asked for, every row is written."""
import ctypes as C

import numpy as np
import pytest

from tests import cv_logistic_restatement as CV
from tests import logistic_restatement as R
from tests.test_gpu_cv_logistic import (_case_a, _case_b, _case_c_rows, _check_cv_oem, _check_folds, _check_scores, _dev, _e2e_reference,
                                        _fold_fit, _interpolated_table, _same, _sparse_table)
from tests.test_gpu_logistic import _data

pytestmark = pytest.mark.gpu

LDS_BYTES = 160 << 10          # LDS of a gfx950 CU


@pytest.fixture(scope="module")
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(n, p, ncol, num_cu):
    import oem_amd
    out = (C.c_int64 * 6)()
    assert oem_amd.lib().oemgpu_selftest_cv_score_plan(n, p, ncol, num_cu, out) == 0
    ch, nchunk, tlds, cb, nlaunch, lds = list(out)
    return dict(ch=ch, nchunk=nchunk, tlds=tlds, cb=cb, nlaunch=nlaunch, lds=lds, tail=n - (nchunk - 1) * ch)


def _bits(a, b):
    """two results of _check_scores' entry side: the same bits"""
    return all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------------------- scoring: rows
def _multi_tile_case(num_cu, layout):
    n = 64 * 4 * num_cu + 4465
    x, y = _data(n, 5, 41)
    rng = np.random.default_rng(42)
    if layout == "random":
        fid = rng.permutation(np.resize(np.arange(1, 5), n))
    elif layout == "contiguous":
        cuts = [0] + [int(n * f) // 64 * 64 + o for f, o in ((0.23, 17), (0.5, 63), (0.81, 1))] + [n]
        assert all(c % 64 for c in cuts[1:])                   # no fold ends where a tile ends
        fid = np.repeat(np.arange(1, 5), np.diff(cuts))
    else:                                                      # fold 4 is the last row of the matrix and nothing else
        fid = rng.permutation(np.resize(np.arange(1, 4), n))
        fid[-1] = 4
        assert (fid == 4).sum() == 1
    x1 = np.column_stack([np.ones(n), x])
    for seed in range(43, 63):                                 # n follows the CU count: the first table that meets _check_scores' precondition
        coef = np.random.default_rng(seed).normal(size=(4, 9, 6)) * np.linspace(0.1, 1.2, 9)[None, :, None]
        if min(np.abs(1.0 / (1.0 + np.exp(-(x1[fid == f + 1] @ coef[f].T))) - 0.5).min() for f in range(4)) > 1e-7:
            break
    return x, y, fid, coef


@pytest.mark.parametrize("layout", ["random", "contiguous", "one_row_fold"])
def test_scoring_multi_tile_chunks(num_cu, layout):
    """n = 64 * 4 * num_cu + 4465: every workgroup owns at least two tiles and n is no multiple of 64 (256 CUs: 128 rows a workgroup, the
    last one 113 = a tile of 64 and one of 49).  The LDS accumulators are carried from tile to tile; with contiguous folds a fold's
    launch skips most tiles and shares its first and last with a neighbour; a fold of one row leaves one lane of one tile"""
    x, y, fid, coef = _multi_tile_case(num_cu, layout)
    n = x.shape[0]
    P = _plan(n, 5, 9, num_cu)
    assert P["ch"] >= 128 and n % 64 != 0 and P["tail"] % 64 != 0 and P["tlds"] == 1 and P["nlaunch"] == 1, P
    if num_cu == 256:
        assert P["ch"] == 128 and P["tail"] == 113, P
    _check_scores(x, y, fid, coef)


def test_scoring_ld_above_n(num_cu):
    """x[j ld + row] but pred[c n + row]: x is a view with ld = n + 37 whose spare rows are NaN; the compact copy gives the same bits"""
    x, y, fid = _case_a()
    coef = _sparse_table(44, 5, 9, 13, density=0.5)
    P = _plan(1500, 12, 9, num_cu)
    assert P["ch"] == 64 and P["tlds"] == 1, P
    padded, _ = _check_scores(x, y, fid, coef, pad=37)
    compact, _ = _check_scores(x, y, fid, coef)
    assert np.all(np.isfinite(padded[2]))
    assert _bits(padded, compact)


def _saturation_case():
    """300 rows, 3 folds, 8 columns.  Column (f, c) is [b0, a u] with a in [0.8, 1.25] and |b0| <= 0.3, and a row is t u / |u|^2 (+ a part
    orthogonal to u for the ordinary rows), so its eta is b0 + a t: |t| <= 2 ordinary, t = +-25 labelled with and against eta, t = 60
    (prob == 1.0), t = -1000 labelled 1 (exp overflows: prob == 0.0, and the row is on the wrong side)"""
    rng = np.random.default_rng(45)
    p, per = 4, 100
    u = np.array([0.7, -1.1, 0.4, 0.9])
    x = np.empty((3 * per, p))
    y = np.empty(3 * per)
    t = np.empty(3 * per)
    for f in range(3):
        tf = np.concatenate([rng.uniform(-2.0, 2.0, per - 6), [25.0, 25.0, -25.0, -25.0, 60.0, -1000.0]])
        yf = np.concatenate([(rng.uniform(size=per - 6) < 0.5).astype(np.float64), [1.0, 0.0, 0.0, 1.0, 1.0, 1.0]])
        w = rng.normal(size=(per, p))
        w -= np.outer(w @ u, u) / (u @ u)
        w[per - 6:] = 0.0
        x[f * per:(f + 1) * per] = np.outer(tf, u) / (u @ u) + w
        y[f * per:(f + 1) * per] = yf
        t[f * per:(f + 1) * per] = tf
    fid = np.repeat(np.arange(1, 4), per)
    order = rng.permutation(3 * per)
    coef = np.empty((3, 8, p + 1))
    coef[:, :, 0] = rng.uniform(-0.3, 0.3, size=(3, 8))
    coef[:, :, 1:] = rng.uniform(0.8, 1.25, size=(3, 8))[:, :, None] * u
    return np.asfortranarray(x[order]), y[order], fid[order], coef, t[order]


def test_scoring_saturated_rows(num_cu):
    """both clamps on wrong and on right rows, prob == 1.0 and prob == 0.0 exactly, in every (fold, column).  The 1e-10 of the sums holds
    by construction: a clamped deviance term is one of two constants, every sum holds three wrong saturated rows (deviance 23.03, mse
    and mae 2 each), and the cancelling y2 - prob of the right ones (1e-11 and below) is 1e-13 of a sum or less"""
    x, y, fid, coef, t = _saturation_case()
    P = _plan(300, 4, 8, num_cu)
    assert P["ch"] == 64 and P["tlds"] == 1 and P["cb"] == 8, P
    (sums, counts, pred), (ref_sums, _, ref_pred) = _check_scores(x, y, fid, coef, over="ignore")
    eta = np.empty((300, 8))
    for f in range(3):
        rows = fid == f + 1
        eta[rows] = np.column_stack([np.ones(rows.sum()), x[rows]]) @ coef[f].T
    a = np.abs(eta)
    assert not np.any((a >= 3.0) & (a < 15.0))                 # nothing near the clamp's edge at |eta| = 11.51
    y1 = (y == 1.0)[:, None]
    for f in range(3):
        rows = fid == f + 1
        e, pr, lab = eta[rows], ref_pred[rows], np.broadcast_to(y1[rows], (rows.sum(), 8))
        for want in ((a[rows] < 3.0), (e >= 15.0) & (e <= 40.0) & lab, (e >= 15.0) & (e <= 40.0) & ~lab, (e <= -15.0) & (e >= -40.0) & lab,
                     (e <= -15.0) & (e >= -40.0) & ~lab, (e >= 40.0) & (pr == 1.0), (e <= -750.0) & (pr == 0.0) & lab):
            assert np.all(want.sum(axis=0) >= 1)               # in every column of the fold
        assert np.all((pr[(e >= 15.0)] > 1.0 - 1e-5)) and np.all(pr[e <= -15.0] < 1e-5)      # the clamp fires on all of them
    assert np.all(ref_sums[:, :, 0] >= 23.0) and np.all(ref_sums[:, :, 4] >= 1.9) and np.all(ref_sums[:, :, 6] >= 1.9)
    assert np.array_equal(pred == 1.0, ref_pred == 1.0) and np.array_equal(pred == 0.0, ref_pred == 0.0)
    assert np.all(np.isfinite(sums))


# ------------------------------------------------------------------------------------------------------------- scoring: the table
@pytest.mark.parametrize("ncol,seed", [(97, 46), (98, 47)])
def test_scoring_lds_limit_small_p(num_cu, ncol, seed):
    """p = 200: 97 columns are the last table in LDS (162 192 of its 163 840 bytes, above the 64 KiB a kernel may ask for unraised); 98
    columns are read through the cache in one launch"""
    x, y, fid = _case_c_rows(200)
    P = _plan(200, 200, ncol, num_cu)
    if ncol == 97:
        assert (P["tlds"], P["cb"], P["nlaunch"], P["lds"]) == (1, 97, 1, 162192), P
    else:
        assert (P["tlds"], P["cb"], P["nlaunch"], P["lds"]) == (0, 98, 1, 8 * (8 * 98 + 1)), P
    assert 8 * (97 * 209 + 1) <= LDS_BYTES < 8 * (98 * 209 + 1)
    _check_scores(x, y, fid, _sparse_table(seed, 3, ncol, 201))


@pytest.mark.parametrize("ncol,seed", [(2, 48), (3, 49)])
def test_scoring_lds_limit_large_p(num_cu, ncol, seed):
    """p = 8191, the largest served: two columns sit in LDS (131 208 bytes), three go through the cache as one batch of three"""
    x, y = _data(130, 8191, 50)
    fid = np.random.default_rng(51).permutation(np.resize(np.arange(1, 4), 130))
    P = _plan(130, 8191, ncol, num_cu)
    if ncol == 2:
        assert (P["tlds"], P["cb"], P["nlaunch"], P["lds"]) == (1, 2, 1, 8 * (2 * 8200 + 1)), P
    else:
        assert (P["tlds"], P["cb"], P["nlaunch"], P["lds"]) == (0, 3, 1, 8 * 25), P
    _check_scores(x, y, fid, _sparse_table(seed, 3, ncol, 8192, density=0.004))      # about 33 coefficients a column: |eta| stays moderate


def test_scoring_refuses_p_above_8191():
    import torch

    import oem_amd
    from oem_amd import api
    xd = torch.zeros((8192, 130), dtype=torch.float64, device="cuda:0").t()
    yd = torch.zeros(130, dtype=torch.float64, device="cuda:0")
    fd = torch.ones(130, dtype=torch.int32, device="cuda:0")
    with pytest.raises(oem_amd.OemgpuError, match="8191") as e:
        api.logistic_cv_score(xd, yd, fd, 3, np.zeros((3, 2, 8193)), y_hi=1.0)
    assert e.value.code == -4


@pytest.mark.parametrize("ncol", [1, 8, 31, 32, 33])
def test_scoring_column_groups(num_cu, ncol):
    """wave w owns columns 32 t + 8 w .. + 8: one column (waves 1-3 idle), one full group, a ragged fourth group, four full groups, and a
    second trip of wave 0 with one column"""
    x, y = _data(200, 7, 52)
    fid = np.random.default_rng(53).permutation(np.resize(np.arange(1, 4), 200))
    P = _plan(200, 7, ncol, num_cu)
    assert (P["ch"], P["nchunk"], P["tail"], P["tlds"], P["cb"]) == (64, 4, 8, 1, ncol), P
    coef = np.random.default_rng(54 + ncol).normal(size=(3, ncol, 8)) * np.linspace(0.2, 1.0, ncol)[None, :, None]
    _check_scores(x, y, fid, coef)


def test_scoring_empty_fold(num_cu):
    """nfolds = 5 and no row in fold 3: its count is 0 and its sums are exactly 0; every row belongs to one of the other folds, is scored
    by it, and predmat keeps none of the NaN it was filled with"""
    x, y = _data(200, 7, 55)
    fid = np.random.default_rng(56).permutation(np.resize(np.array([1, 2, 4, 5]), 200))
    P = _plan(200, 7, 9, num_cu)
    assert P["ch"] == 64 and P["tlds"] == 1, P
    coef = np.random.default_rng(57).normal(size=(5, 9, 8)) * np.linspace(0.2, 1.0, 9)[None, :, None]
    (sums, counts, pred), (ref_sums, ref_counts, _) = _check_scores(x, y, fid, coef)
    assert ref_counts[2] == 0 and counts[2] == 0
    assert np.all(sums[2] == 0.0) and np.all(ref_sums[2] == 0.0)
    assert counts.sum() == 200 and not np.isnan(pred).any()


def test_scoring_y_levels():
    """y2 = (y == y_hi): the table of case a scored with y as {-1, 1} and as {1, 2} gives the bits of the {0, 1} run"""
    E = _e2e_reference()
    x, y, fid = E["x"], E["y"], E["fid"]
    coef = _interpolated_table(x, y, fid, fitted=E["fitted"])
    assert set(np.unique(y)) == {0.0, 1.0}
    base, _ = _check_scores(x, y, fid, coef)
    for yr in (2.0 * y - 1.0, y + 1.0):
        got, _ = _check_scores(x, yr, fid, coef)
        assert _bits(got, base)


# ------------------------------------------------------------------------------------------------------------- the fold entry
def _map_case(first):
    x, y = R.near_separable(5000, 8, 3)
    x, y = np.asfortranarray(np.roll(x, first, axis=0)), np.roll(y, first)      # the ten far rows are rows first .. first + 9
    fid = np.empty(5000, dtype=np.int64)
    fid[:first] = 1
    fid[first:] = np.resize([2, 3, 4], 5000 - first)
    fid[first:first + 10] = 2
    return x, y, fid


@pytest.mark.parametrize("hessian", ["upper.bound", "full"])
@pytest.mark.parametrize("first", [1019, 1024, 2500])
def test_fold_entry_kept_row_map_across_scan_tiles(first, hessian):
    """fold 1 = rows 0 .. first - 1, so the fit without it keeps rows first, first + 1, ...: the W floor of IRLS step i tests row first + i,
    which the scan finds in its second tile of 1024 rows (straddling the boundary, starting at it) or in its third after two tiles without
    a kept row.  The far rows are the first kept rows, where the floor fires; the other folds keep row i as their i-th row.
    W enters the results through Z = sqrt(W) x of a Hessian build alone.  With "upper.bound" the only build is step 0 of the first lambda,
    at beta = 0 and W = 1/4, so the floor fires there (the restatement counts it) without moving a digit: a wrong map is seen by the
    "full" cases only (a scan that forgets the kept rows of the earlier tiles fails all three of them and none of the others)"""
    x, y, fid = _map_case(first)
    kw = dict(nlambda=25, irls_maxit=30, compute_loss=True)
    stats = _check_folds(x, y, fid, ["lasso"], hessian_type=hessian, rkw=dict(hessian_full=hessian == "full", **kw), **kw)
    print("floored", [s["floored"] for s in stats], "clamped", [s["clamped"] for s in stats])
    assert stats[0]["floored"] > 0, stats


def _poison(x, y, left, how):
    x2, y2 = x.copy(order="F"), y.copy()
    if how == "finite":
        x2[left] = 1e6 * np.random.default_rng(58).normal(size=(int(left.sum()), x.shape[1]))
        y2[left] = 1.0 - y[left]
    else:
        x2[left] = np.nan
        y2[left] = np.nan
    return x2, y2


@pytest.mark.parametrize("how", ["finite", "nan"])
@pytest.mark.parametrize("case", ["b", "c-upper.bound", "c-full"])
def test_fold_entry_left_out_rows_never_reach_the_arithmetic(case, how):
    """other values (1e6 x normal, y flipped) or NaN in the left-out rows of x and y on the device: the fold fit keeps every bit (a pass
    that multiplied a left-out value by zero would keep them in the finite variant only).  y on the host, which the front end checks for
    two levels and never sends, is the clean one"""
    if case == "b":
        x, y, fid = _case_b()
        nfolds, leave_out, pens = 4, 3, ["lasso"]
        kw = dict(nlambda=25, irls_maxit=30, compute_loss=True)
    else:
        x, y, fid = _case_c_rows(1500)
        nfolds, leave_out, pens = 3, 2, ["lasso", "grp.lasso"]
        kw = dict(nlambda=6, lambda_min_ratio=0.05, compute_loss=True, groups=np.repeat(np.arange(1, 41), 5), hessian_type=case[2:])
    left = fid == leave_out
    x2, y2 = _poison(x, y, left, how)
    assert np.array_equal(x2[~left], x[~left]) and np.array_equal(y2[~left], y[~left]) and not np.array_equal(y2[left], y[left])
    xd, yd, fd = _dev(x, y, fid)
    xd2, yd2, _ = _dev(x2, y2, fid)
    a = _fold_fit(xd, y, yd, fd, nfolds, leave_out, pens, **kw)
    b = _fold_fit(xd2, y, yd2, fd, nfolds, leave_out, pens, **kw)
    assert all(np.all(np.isfinite(v)) for v in a["beta"])
    _same(a, b, pens)


def test_fold_entry_ld_above_n():
    """case a on a view with ld = n + 37 and NaN in the spare rows: against the restatement, and the bits of the compact x"""
    x, y, fid = _case_a()
    pens = ["lasso", "mcp"]
    kw = dict(nlambda=20, compute_loss=True)
    padded = []
    _check_folds(x, y, fid, pens, pad=37, fits=padded, **kw)
    xd, yd, fd = _dev(x, y, fid)
    for i in range(1, 6):
        _same(padded[i - 1], _fold_fit(xd, y, yd, fd, 5, i, pens, **kw), pens)


def test_fold_entry_refusal_at_equality():
    """n = 60, p = 19 with the intercept: q = 20.  40 rows in fold 1 leave n_eff = 20 = q, which is refused; 39 leave 21, which is fitted
    (one spare degree of freedom: only that it returns, on 21 rows, is held)"""
    import oem_amd
    x, y = _data(60, 19, 59, k=2)
    for size, n_eff in ((40, 20), (39, 21)):
        fid = np.empty(60, dtype=np.int64)
        fid[:size] = 1
        fid[size:] = np.resize([2, 3], 60 - size)
        assert (fid != 1).sum() == n_eff and len(np.unique(y[fid != 1])) == 2
        xd, yd, fd = _dev(x, y, fid)
        if n_eff == 20:
            with pytest.raises(oem_amd.OemgpuError, match="fold 1") as e:
                _fold_fit(xd, y, yd, fd, 3, 1, ["lasso"], nlambda=4)
            assert e.value.code == -4
        else:
            assert _fold_fit(xd, y, yd, fd, 3, 1, ["lasso"], nlambda=4)["nobs"] == 21


# ------------------------------------------------------------------------------------------------------------- end to end
_E2E_B = {}
_E2E_B_KW = dict(nlambda=25, irls_maxit=30, compute_loss=True)       # compute_loss: the restatement counts the clamps where it forms the loss


def _e2e_b_reference():
    if not _E2E_B:
        x, y, fid = _case_b()
        stats = []
        _E2E_B.update(x=x, y=y, fid=fid, stats=stats, fitted=CV.fits(x, y, fid, penalty=["lasso"], stats=stats, **_E2E_B_KW))
    return _E2E_B


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("measure", ["deviance", "class"])
def test_cv_oem_binomial_end_to_end_near_separable(measure, grouped):
    """case b: four uneven folds of near-separable data.  What case a does not guarantee: lambdas of the full fit that a fold would have to
    extrapolate below are trimmed (fewer than the 25 asked for come back), and the fold fits reach the loss clamps"""
    E = _e2e_b_reference()
    ref = _check_cv_oem(E, measure, grouped, **_E2E_B_KW)
    assert len(ref["lambda"][0]) < 25, len(ref["lambda"][0])
    assert len(E["stats"]) == 4 and any(s["clamped"] > 0 for s in E["stats"]), E["stats"]
