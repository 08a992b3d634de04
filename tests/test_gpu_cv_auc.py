"""The AUC of cv.oem for binomial fits on the MI355X (oemgpu_logistic_cv_auc_dev, oem_amd/csrc/logistic_auc.hip) against numpy alone.

Every case but the last feeds a synthetic device predmat (ncol x n) straight to api.logistic_cv_auc and asserts u, n1, n0 EQUAL to
_numpy_counts -- np.argsort(kind="stable") on the fold's rows, then integer counting -- and equal on a second call.  Each hand-placed
case first asks oemgpu_selftest_cv_auc_plan, with the live CU count, whether its shape lands on the form it is named for (T = keys per
tile, L = the longest segment sorted in LDS).  Covered: segment lengths round the wave, the tile and L, an LDS segment and a workspace
segment in one call; fold layouts, a fold without rows, folds of one class; ties (all equal, three values, across a tile boundary both
ways round); digits (bit 0 of the mantissa, an exponent step, 0, the smallest subnormal and normal, 1 - 2^-53, 1, NaN and -NaN, -0.0);
recoded y levels and a y_hi that no row has; one column, seven, and one more than a batch holds; the refusals of a fold id outside
1 .. K; a seeded sweep (OEM_FUZZ_SCALE scales it).  End to end, cv_oem(type_measure="auc", keep=True) on a dense and a scipy.sparse x:
cvm and cvsd recomputed on the host from the returned fit.preval with api._auc_rows and cvcompute's arithmetic, to the last bit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCALE = int(os.environ.get("OEM_FUZZ_SCALE", "1"))
WS_BOUND = 256 << 20


@pytest.fixture(scope="module")
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(n, K, ncol, num_cu, longest):
    from oem_amd import api
    return api.cv_auc_plan(n, K, ncol, num_cu, longest)


def _numpy_counts(pm, y, fid, K, y_hi):
    """pm: ncol x n.  The integers of the issue's section 1, from numpy's stable argsort"""
    ncol = pm.shape[0]
    u = np.zeros((K, ncol), dtype=np.int64)
    n1 = np.zeros(K, dtype=np.int64)
    n0 = np.zeros(K, dtype=np.int64)
    y2 = y == y_hi
    for f in range(K):
        rows = np.flatnonzero(fid == f + 1)
        yy = y2[rows]
        n1[f] = int(yy.sum())
        n0[f] = len(rows) - n1[f]
        for c in range(ncol):
            ys = yy[np.argsort(pm[c, rows], kind="stable")]
            u[f, c] = int(np.cumsum(~ys, dtype=np.int64)[ys].sum())
    return u, n1, n0


def _run(pm, y, fid, K, y_hi, cols=None):
    """the entry twice on (pm, y, fid): equal to each other, and to numpy on `cols` (all columns when None)"""
    import torch
    from oem_amd import api
    pd = torch.as_tensor(pm, device="cuda")
    yd = torch.as_tensor(np.asarray(y, dtype=np.float64), device="cuda")
    fd = torch.as_tensor(np.ascontiguousarray(fid, dtype=np.int32), device="cuda")
    a = api.logistic_cv_auc(pd, yd, fd, K, y_hi=y_hi)
    b = api.logistic_cv_auc(pd, yd, fd, K, y_hi=y_hi)
    for g, h in zip(a, b):
        assert g.dtype == np.int64 and np.array_equal(g, h)
    cols = np.arange(pm.shape[0]) if cols is None else np.asarray(cols)
    u, n1, n0 = _numpy_counts(pm[cols], np.asarray(y, dtype=np.float64), np.asarray(fid), K, y_hi)
    assert np.array_equal(a[1], n1) and np.array_equal(a[2], n0), (a[1], n1, a[2], n0)
    bad = np.argwhere(a[0][:, cols] != u)
    assert bad.size == 0, (bad[:5], a[0][:, cols][tuple(bad[0])], u[tuple(bad[0])])
    return a


def _folds_of_lengths(lens, rng):
    """foldid with len(lens) folds of exactly these lengths, rows of the folds mixed by a seeded permutation"""
    return rng.permutation(np.repeat(np.arange(1, len(lens) + 1), lens))


def _probs(rng, ncol, n, ties=0.0, nan=0.0):
    pm = rng.random((ncol, n))
    if ties > 0:
        q = rng.random((ncol, n)) < ties
        pm[q] = np.round(pm[q], 2)
    if nan > 0:
        pm[rng.random((ncol, n)) < nan] = np.nan
    return pm


# ------------------------------------------------------------------------------------------------------------- segment lengths
def _length_triples(T, L):
    return {"0_1_3L+7": (0, 1, 3 * L + 7), "2_63_L+1": (2, 63, L + 1), "64_65_2T+1": (64, 65, 2 * T + 1), "T-1_T_T+1": (T - 1, T, T + 1),
            "L_L+1_3": (L, L + 1, 3)}


@pytest.mark.parametrize("name", ["0_1_3L+7", "2_63_L+1", "64_65_2T+1", "T-1_T_T+1", "L_L+1_3"])
def test_segment_lengths(name, num_cu):
    P0 = _plan(1000, 3, 2, num_cu, 10)
    T, L = P0["tile"], P0["lmax"]
    assert 64 < T < L
    lens = _length_triples(T, L)[name]
    n = sum(lens)
    P = _plan(n, 3, 2, num_cu, max(lens))
    assert P["form"] == ("hbm" if max(lens) > L else "lds") and P["lmax"] == L and P["tile"] == T
    if name in ("0_1_3L+7", "2_63_L+1", "L_L+1_3"):
        assert min(lens) <= L < max(lens)                              # an LDS segment and a workspace segment side by side
    rng = np.random.default_rng(sum(lens))
    fid = _folds_of_lengths(lens, rng)
    y = (rng.random(n) < 0.4).astype(np.float64)
    pm = _probs(rng, 2, n, ties=0.3)
    u, n1, n0 = _run(pm, y, fid, 3, 1.0)
    assert tuple(n1 + n0) == lens
    for f, ln in enumerate(lens):
        if ln == 0:
            assert u[f].tolist() == [0, 0] and n1[f] == 0 and n0[f] == 0


# ------------------------------------------------------------------------------------------------------------- fold layouts
@pytest.mark.parametrize("layout", ["interleaved", "blocked", "permuted"])
def test_fold_layouts(layout, num_cu):
    n, K = 3 * 9001 + 2, 5                                             # fold 4 has no rows; fold 1 is all y2 = 1, fold 2 all y2 = 0
    P = _plan(n, K, 3, num_cu, 9001)
    assert P["form"] == "hbm" and P["chunks"] > 1
    rng = np.random.default_rng(7)
    live = np.array([1, 2, 3, 5])
    if layout == "interleaved":
        fid = live[np.arange(n) % 4]
    elif layout == "blocked":
        fid = np.sort(live[np.arange(n) % 4])
    else:
        fid = rng.permutation(live[np.arange(n) % 4])
    y = (rng.random(n) < 0.5).astype(np.float64)
    y[fid == 1] = 1.0
    y[fid == 2] = 0.0
    pm = _probs(rng, 3, n, ties=0.2)
    u, n1, n0 = _run(pm, y, fid, K, 1.0)
    assert n1[3] == 0 and n0[3] == 0 and not u[3].any()                # the fold without rows
    assert n0[0] == 0 and not u[0].any() and n1[1] == 0 and not u[1].any()
    assert u[2].all() and u[4].all()


# ------------------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("kind", ["all_equal", "three_values", "tile_boundary_10", "tile_boundary_01"])
def test_ties(kind, num_cu):
    P0 = _plan(1000, 3, 2, num_cu, 10)
    T, L = P0["tile"], P0["lmax"]
    lens = (2 * T + 5, L + T + 3, 700)                                 # an LDS segment, a workspace segment, a short one
    n = sum(lens)
    assert _plan(n, 3, 2, num_cu, max(lens))["form"] == "hbm" and lens[0] <= L
    rng = np.random.default_rng(11)
    fid = np.repeat(np.arange(1, 4), lens)                             # blocked: a segment's position is row - start
    y = (rng.random(n) < 0.5).astype(np.float64)
    if kind == "all_equal":
        pm = np.full((2, n), 0.25)
    elif kind == "three_values":
        pm = rng.choice([0.125, 0.5, 0.7], size=(2, n))
    else:                                                              # sorted but for one pair of equal values at positions T - 1 and T
        pm = np.empty((2, n))
        start = 0
        for ln in lens:
            v = (np.arange(ln) + 1.0) / (ln + 1.0)
            if ln > T:
                v[T] = v[T - 1]
                y[start + T - 1], y[start + T] = (1.0, 0.0) if kind.endswith("10") else (0.0, 1.0)
            pm[0, start:start + ln] = v
            pm[1, start:start + ln] = v[::-1]                          # column 1: the pair meets at the far end, after a full reversal
            start += ln
    _run(pm, y, fid, 3, 1.0)


# ------------------------------------------------------------------------------------------------------------- digits
def _neg_nan(k):
    return np.array([0xFFF8000000000001] * k, dtype=np.uint64).view(np.float64)


@pytest.mark.parametrize("kind", ["mantissa_bit0", "exponent_step", "specials", "nans"])
def test_digits(kind, num_cu):
    P0 = _plan(1000, 3, 2, num_cu, 10)
    L = P0["lmax"]
    lens = (L + 9, 4100, 130)
    n = sum(lens)
    assert _plan(n, 3, 3, num_cu, max(lens))["form"] == "hbm"
    rng = np.random.default_rng(13)
    fid = _folds_of_lengths(lens, rng)
    y = (rng.random(n) < 0.5).astype(np.float64)
    if kind == "mantissa_bit0":
        base = np.float64(0.3).view(np.uint64)
        pm = (base + rng.integers(0, 2, size=(3, n)).astype(np.uint64)).view(np.float64)
    elif kind == "exponent_step":
        pm = rng.choice([np.nextafter(0.5, 0.0), 0.5], size=(3, n))
    else:
        vals = np.array([0.0, -0.0, 5e-324, 2.2250738585072014e-308, 1.0 - 2.0 ** -53, 1.0])
        pm = rng.choice(vals, size=(3, n))
        pm[2] = np.where(rng.random(n) < 0.5, pm[2], rng.random(n))
        if kind == "nans":
            pm[rng.random((3, n)) < 0.1] = np.nan
            q = rng.random((3, n)) < 0.05
            pm[q] = _neg_nan(int(q.sum()))
            assert np.signbit(pm[q]).all() and np.isnan(pm[q]).all()
    _run(pm, y, fid, 3, 1.0)


# ------------------------------------------------------------------------------------------------------------- labels
@pytest.mark.parametrize("levels,y_hi", [((0.0, 1.0), 1.0), ((-1.0, 1.0), 1.0), ((2.0, 5.0), 5.0), ((0.0, 1.0), 3.0)])
def test_labels(levels, y_hi, num_cu):
    n, K = 2500, 4
    assert _plan(n, K, 2, num_cu, 625)["form"] == "lds"
    rng = np.random.default_rng(17)
    fid = np.arange(n) % K + 1
    y = np.asarray(levels)[(rng.random(n) < 0.45).astype(int)]
    u, n1, n0 = _run(_probs(rng, 2, n, ties=0.1), y, fid, K, y_hi)
    if y_hi == 3.0:
        assert not n1.any() and not u.any() and n0.tolist() == [625] * 4


# ------------------------------------------------------------------------------------------------------------- columns
@pytest.mark.parametrize("ncol", [1, 7])
def test_columns(ncol, num_cu):
    n, K = 30011, 3
    assert _plan(n, K, ncol, num_cu, 10004)["form"] == "hbm"
    rng = np.random.default_rng(19 + ncol)
    fid = rng.permutation(np.arange(n) % K + 1)
    y = (rng.random(n) < 0.3).astype(np.float64)
    _run(_probs(rng, ncol, n, ties=0.1, nan=0.01), y, fid, K, 1.0)


def test_one_column_more_than_a_batch(num_cu):
    K = 3
    lo, hi = 1, 10 ** 7                                                # the smallest n at which a batch holds fewer than 40 columns
    while lo < hi:
        mid = (lo + hi) // 2
        if _plan(mid, K, 100, num_cu, (mid + K - 1) // K)["cb"] < 40:
            hi = mid
        else:
            lo = mid + 1
    n = lo
    longest = (n + K - 1) // K
    cb = _plan(n, K, 100, num_cu, longest)["cb"]
    assert cb == 39 and 4 * 10 ** 5 < n < 5 * 10 ** 5, (n, cb)        # 256 MB / (16 B x n) crosses 40 there
    ncol = cb + 1
    P = _plan(n, K, ncol, num_cu, longest)
    assert P["form"] == "hbm" and P["cb"] == cb and P["batches"] == 2 and P["ws"] <= WS_BOUND
    rng = np.random.default_rng(23)
    fid = np.arange(n) % K + 1
    y = (rng.random(n) < 0.5).astype(np.float64)
    pm = rng.random((ncol, n))
    pm[::2] = np.round(pm[::2], 3)                                     # every other column with ties
    _run(pm, y, fid, K, 1.0)                                           # all columns: first and last of both batches among them


# ------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("bad", [0, 4])
def test_fold_id_outside_is_refused(bad):
    import torch
    import oem_amd
    from oem_amd import api
    n, K = 5000, 3
    rng = np.random.default_rng(29)
    fid = (np.arange(n) % K + 1).astype(np.int32)
    fid[3777] = bad
    pd = torch.as_tensor(rng.random((2, n)), device="cuda")
    yd = torch.as_tensor((rng.random(n) < 0.5).astype(np.float64), device="cuda")
    with pytest.raises(oem_amd.OemgpuError) as e:
        api.logistic_cv_auc(pd, yd, torch.as_tensor(fid, device="cuda"), K, y_hi=1.0)
    assert e.value.code == -1 and "fold id" in str(e.value)
    fid[3777] = 1                                                      # and the context serves the next call
    api.logistic_cv_auc(pd, yd, torch.as_tensor(fid, device="cuda"), K, y_hi=1.0)


# ------------------------------------------------------------------------------------------------------------- seeded sweep
@pytest.mark.parametrize("seed", range(20 * SCALE))
def test_random_auc(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 20001))
    K = int(rng.integers(3, 8))
    ncol = int(rng.integers(1, 10))
    ties = float(rng.choice([0.0, 0.1, 0.9, 1.0]))
    nan = float(rng.choice([0.0, 0.0, 0.02, 0.5]))
    fid = rng.integers(1, K + 1, size=n) if seed % 2 else rng.permutation(np.arange(n) % K + 1)
    y = (rng.random(n) < rng.random()).astype(np.float64)
    _run(_probs(rng, ncol, n, ties=ties, nan=nan), y, fid, K, 1.0)


# ------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("sparse", [False, True])
def test_cv_oem_auc_end_to_end(sparse):
    import oem_amd
    from oem_amd import api
    n, p, K, nl = 120, 6, 4, 5
    rng = np.random.default_rng(31)
    x = rng.normal(size=(n, p))
    if sparse:
        import scipy.sparse as sp
        x[rng.random((n, p)) < 0.6] = 0.0
    y = (x @ np.array([1.0, -0.8, 0.5, 0.0, 0.0, 0.3]) + 0.7 * rng.normal(size=n) > 0).astype(np.float64)
    fid = rng.permutation(np.arange(n) % K + 1)
    res = oem_amd.cv_oem(sp.csc_matrix(x) if sparse else x, y, family="binomial", penalty="lasso", nlambda=nl, type_measure="auc", keep=True,
                         foldid=fid)
    assert res["name"] == "AUC"
    pv = res["fit.preval"][0]
    assert pv.shape == (n, nl)
    nlami = int((~np.isnan(pv).all(axis=0)).sum())
    assert nlami >= 2 and not np.isnan(pv[:, :nlami]).any()
    raw = np.full((K, nl), np.nan)
    w = np.array([(fid == i + 1).sum() for i in range(K)], dtype=np.float64)
    y2 = (y == y.max()).astype(np.float64)
    for i in range(K):
        rows = fid == i + 1
        for j in range(nlami):
            raw[i, j] = api._auc_rows(y2[rows], pv[rows, j])
    good = np.zeros((K, nl))
    good[:, :nlami] = 1
    Nm = good.sum(axis=0)                                              # cvcompute (R/utils.R:128-144) as api._cv_oem_binomial_on writes it
    ok = ~np.isnan(raw)
    wsum = (ok * w[:, None]).sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        cm = np.where(ok, raw * w[:, None], 0.0).sum(axis=0) / wsum
        cs = np.sqrt(np.where(ok, (raw - cm) ** 2 * w[:, None], 0.0).sum(axis=0) / wsum / (Nm - 1))
    keep = ~np.isnan(cs)
    assert np.asarray(res["cvm"][0]).tobytes() == cm[keep].tobytes()
    assert np.asarray(res["cvsd"][0]).tobytes() == cs[keep].tobytes()
    assert 0.5 < np.max(res["cvm"][0]) <= 1.0
