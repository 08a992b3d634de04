"""The MASKED shared row pass (logistic_multi.hip) alone, through oemgpu_selftest_logistic_multi_rows_fold_dev: column t is
a response of Y on the rows with foldid != leave[t].  Against tests/test_gpu_logistic_multi_rows._ref on the gathered rows
x[keep], Y[keep, r] with that file's derived tolerance (both modes), and the bytes of a column whatever its companions and their
leave values are.  The paddings of x and Y are NaN: any read of them shows."""
import numpy as np
import pytest

from tests.test_gpu_logistic_multi_rows import _case, _ref, _x, _y

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import oem_amd
    oem_amd.lib()
    from oem_amd import api
    return api


def _folds(n, K, seed):
    """ids in [1, K - 1] at random, except: rows [256, 448) all in fold 1 (three whole 64-row chunks left out at once), exactly 3 rows in
    fold 2, and fold K carried by no row"""
    rng = np.random.default_rng(seed)
    f = rng.integers(3, K, size=n).astype(np.int32)
    if n >= 448:
        f[256:448] = 1
    else:
        f[: n // 3] = 1
    f[[5, n // 2, n - 1]] = 2
    return f


def _check(api, x, Y, bt, f, leave, intercept, mode, xl="cm", yl="rm", ycol=None):
    cols = np.arange(Y.shape[1]) if ycol is None else np.asarray(ycol)
    got = api.logistic_multi_rows_fold(_x(x, xl), _y(Y, yl), f, leave, bt if mode else None, intercept=intercept, mode=mode, ycol=ycol)
    assert got.shape == (len(leave), x.shape[1] + 2) and np.all(np.isfinite(got)), "a NaN: padding was read, or an entry was not written"
    worst = 0.0
    for t, (r, k) in enumerate(zip(cols, leave)):
        keep = f != k
        ref, tol = _ref(x[keep], Y[keep][:, [r]], bt[[t]], intercept, mode)
        err = np.abs(got[t] - ref[0])
        worst = max(worst, float((err / np.maximum(tol[0], 1e-300)).max()))
        assert np.all(err <= tol[0]), (t, r, k, worst)
        if not mode:
            assert got[t, -1] == 0.0
    print(f"n={x.shape[0]} p={x.shape[1]} cols={len(leave)} mode={mode} {xl}/{yl}: worst error / tolerance = {worst:.3g}")
    return got


# ------------------------------------------------------------------------------------------------ against numpy on the gathered rows
@pytest.mark.parametrize("ncol", [1, 16, 17])
def test_mixed_leave_with_a_row_tail(api, ncol):
    """n = 1000: a tail sub-block; 1 / 16 / 17 columns: LT 1 and LT 4; whole chunks left out, a 3-row fold, an id no row has, leave 0"""
    n, p, K = 1000, 12, 7
    x, Y, bt = _case(n, p, ncol, 3100 + ncol)
    f = _folds(n, K, 31)
    leave = np.resize(np.array([1, 0, 2, K, 3, 4, 5, 1, 6], dtype=np.int32), ncol)
    for mode in (1, 0):
        _check(api, x, Y, bt, f, leave, True, mode, "cm", "rm")
    _check(api, x, Y, bt, f, leave, True, 1, "rm", "cm")


@pytest.mark.parametrize("n,p,ncol", [(500, 130, 5), (500, 130, 20), (700, 513, 3)])
def test_column_bands(api, n, p, ncol):
    """p = 130: 4 tiles per wave (LT 1 and 4); p = 513, n = 700: 16 tiles per wave, sub-blocks of 32 rows"""
    K = 6
    x, Y, bt = _case(n, p, ncol, 3200 + p + ncol, f32=True)
    f = _folds(n, K, 32)
    leave = np.resize(np.array([2, 1, 0, K, 4], dtype=np.int32), ncol)
    for xl, yl in (("cm", "rm"), ("rm", "cm"), ("f32", "rm")):
        _check(api, x, Y, bt, f, leave, True, 1, xl, yl)
    _check(api, x, Y, bt, f, leave, False, 0, "f32", "cm")


def test_65_columns_and_a_column_map(api):
    """65 columns: the selftest's chunks of 64, LT 4 then LT 1; then 65 columns drawn from 3 responses through ycol"""
    n, p, K = 600, 20, 5
    x, Y, bt = _case(n, p, 65, 3300)
    f = _folds(n, K, 33)
    leave = np.resize(np.arange(K + 1, dtype=np.int32), 65)
    _check(api, x, Y, bt, f, leave, True, 1, "cm", "cm")
    ycol = np.resize(np.array([2, 0, 1, 1], dtype=np.int32), 65)
    for mode in (1, 0):
        _check(api, x, Y[:, :3], bt, f, leave, True, mode, "rm", "rm", ycol=ycol)


def test_without_intercept(api):
    n, p, K = 300, 17, 5
    x, Y, bt = _case(n, p, 4, 3400, intercept=False)
    f = _folds(n, K, 34)
    for mode in (1, 0):
        _check(api, x, Y, bt, f, np.array([1, 2, 0, 3], dtype=np.int32), False, mode)


# ------------------------------------------------------------------------------------------------ the same bytes
@pytest.mark.parametrize("p", [20, 300, 600])
def test_a_column_has_the_same_bytes_whatever_rides_with_it(api, p):
    n, m, K = 1500, 65, 6
    x, Y, bt = _case(n, p, m, 3500 + p, f32=True)
    f = _folds(n, K, 35)
    xd = {k: _x(x, k) for k in ("cm", "rm", "f32")}
    rng = np.random.default_rng(p)
    leave = rng.integers(0, K + 1, size=m).astype(np.int32)
    for mode in (1, 0):
        b = bt if mode else None
        plain = api.logistic_multi_rows(xd["cm"], _y(Y, "rm"), b, mode=mode)
        # leave all 0, and the id of an empty fold, are the unmasked pass
        for lv in (0, K):
            got = api.logistic_multi_rows_fold(xd["cm"], _y(Y, "rm"), f, np.full(m, lv, dtype=np.int32), b, mode=mode)
            assert np.array_equal(got, plain), (mode, lv)
        full = api.logistic_multi_rows_fold(xd["cm"], _y(Y, "rm"), f, leave, b, mode=mode)
        assert np.all(np.isfinite(full))
        sel = leave == 0
        assert sel.any() and np.array_equal(full[sel], plain[sel])
        # two calls; the three layouts of x; both layouts of Y
        assert np.array_equal(full, api.logistic_multi_rows_fold(xd["cm"], _y(Y, "rm"), f, leave, b, mode=mode))
        assert np.array_equal(full, api.logistic_multi_rows_fold(xd["rm"], _y(Y, "cm"), f, leave, b, mode=mode))
        assert np.array_equal(full, api.logistic_multi_rows_fold(xd["f32"], _y(Y, "rm"), f, leave, b, mode=mode))
        # a column alone (LT 1, block 0) against the same column among 64 others
        for r in (0, 17, 63, 64):
            one = api.logistic_multi_rows_fold(xd["rm"], _y(Y[:, [r]], "rm"), f, leave[[r]], None if b is None else b[[r]], mode=mode)
            assert np.array_equal(one[0], full[r]), (mode, r)
        # a permuted list: other companions, other leave values beside it, another block
        perm = rng.permutation(m)
        shuffled = api.logistic_multi_rows_fold(xd["cm"], _y(Y[:, perm], "cm"), f, leave[perm], None if b is None else b[perm], mode=mode)
        assert np.array_equal(shuffled, full[perm]), mode
        # the same columns through a column map, and its companions' leave values changed
        other = leave.copy()
        other[1::2] = (other[1::2] + 1) % (K + 1)
        mapped = api.logistic_multi_rows_fold(xd["cm"], _y(Y, "rm"), f, other[perm], None if b is None else b[perm], mode=mode, ycol=perm)
        same = (other == leave)[perm]
        assert same.any() and (~same).any()
        assert np.array_equal(mapped[same], full[perm][same]), mode
        part = api.logistic_multi_rows_fold(xd["cm"], _y(Y[:, :17], "rm"), f, leave[:17], None if b is None else b[:17], mode=mode)
        assert np.array_equal(part, full[:17]), mode


def test_live_mask(api):
    import torch
    n, m, K = 300, 40, 5
    f = _folds(n, K, 36)
    for p in (20, 300):
        x, Y, bt = _case(n, p, m, 3600 + p)
        xd, Yd = _x(x, "cm"), _y(Y, "rm")
        leave = np.resize(np.arange(K + 1, dtype=np.int32), m)
        full = api.logistic_multi_rows_fold(xd, Yd, f, leave, bt)
        block = api.logistic_multi_plan(n, p, m)["block"]
        live = np.ones(m, dtype=np.int32)
        live[[1, 5, m - 1]] = 0
        out = torch.full((m, p + 2), -7.5, dtype=torch.float64, device="cuda")
        got = api.logistic_multi_rows_fold(xd, Yd, f, leave, bt, live=live, out=out)
        assert np.array_equal(got[live == 0], np.full((3, p + 2), -7.5))     # a frozen column's output is untouched
        assert np.array_equal(got[live == 1], full[live == 1])
        if block < m:
            live = np.ones(m, dtype=np.int32)
            live[:block] = 0
            out = torch.full((m, p + 2), -7.5, dtype=torch.float64, device="cuda")
            got = api.logistic_multi_rows_fold(xd, Yd, f, leave, bt, live=live, out=out)
            assert np.array_equal(got[:block], np.full((block, p + 2), -7.5)) and np.array_equal(got[block:], full[block:])
            assert api.logistic_multi_stats()["blocks_skipped"] == 1
