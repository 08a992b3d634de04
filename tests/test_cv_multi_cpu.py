"""cv_oem_multi (oemgpu_cv_dense_multi_dev / _rm_dev) without a GPU: the plan against its own arithmetic and against
xval_oem_multi's on the fields they share, the index table of lambda.interp against api._lambda_interp / _cv_gaussian_table, the
vectorised fold statistics against the functions cv_oem calls, and every refusal that comes before a device is looked for.

The bound of the interpolation: the table's coordinate and numpy's may round to different sides of an integer, so (left, right, frac) are
not compared -- the interpolated coefficients are.  Both evaluate beta[left] frac + beta[right] (1 - frac) with frac from quotients of
differences of the normalised grid: an error of a few eps in the normalised coordinate moves the result by that over the local gap g
times the difference of the two neighbours, at most 2 max|beta|.  32 eps max|beta| / g covers sixteen roundings of that size."""
import ctypes as C

import numpy as np
import pytest

ERR_ARG, ERR_UNSUPPORTED = -1, -4
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def oa():
    import oem_amd
    oem_amd.lib()
    return oem_amd


@pytest.fixture(scope="module")
def api(oa):
    from oem_amd import api
    return api


def _r256(v):
    return (v + 255) // 256 * 256


# ------------------------------------------------------------------------------------------------ the plan
SHARED = ["rows", "chunks_max", "passes", "block", "bytes_single", "bytes_col", "bytes_yp", "bytes_cfirst", "bytes_part"]
PARTS = ["bytes_raw", "bytes_idx", "bytes_ncol", "bytes_inv", "bytes_pred", "bytes_tri"]


@pytest.mark.parametrize("num_cu", [256, 64, 8])
def test_plan_arithmetic(api, num_cu):
    seen = set()
    for n, p in [(600, 8), (3000, 41), (3000, 208), (3000, 209), (3000, 250), (3000, 288), (3000, 300), (2000, 1024), (1600, 1040), (10 ** 6, 100)]:
        for K in (3, 4, 10, 100):
            if n - -(-n // K) <= p:
                continue
            for m in (1, 2, 5, 17, 129, 256):
                for npen, nl in [(1, 100), (2, 12), (3, 5)]:
                    for keep in (False, True):
                        P = api.cv_multi_plan(n, p, K, m, npen, nl, num_cu, keep=keep)
                        cap = P["cap"]
                        seen.add((P["engine"], P["route"]))
                        assert 1 <= P["nb"] <= m
                        if P["route"] == 0:
                            assert P["engine"] != 0 and P["nb"] * (K + 1) <= cap <= 513
                            assert P["nb"] == min(m, cap // (K + 1))
                        else:
                            assert P["nb"] == 1 and (P["engine"] == 0 or cap < K + 1)
                        assert P["solve_chunks"] == -(-m // P["nb"]) and (P["solve_chunks"] - 1) * P["nb"] < m      # no empty chunk
                        # the solve plan is oem_multi's (q = p: the intercept is centred out), the passes are xval_oem_multi's
                        M = api.multi_plan(n, p, m, npen, 0, num_cu)
                        assert (cap, P["engine"]) == (M["cap"], M["engine"])
                        Xv = api.xval_multi_plan(n, p, K, m, npen, nl, num_cu)
                        for key in SHARED:
                            assert P[key] == Xv[key], key
                        nb = P["nb"]
                        ldp = (n + 16 * K + 15) // 16 * 16
                        assert P["bytes_raw"] == P["bytes_tab"] == nb * K * npen * nl * (p + 1) * 8
                        assert P["bytes_comp"] == nb * (K + 1) * (p + 2) ** 2 * 8
                        assert P["bytes_idx"] == nb * K * npen * nl * 16 and P["bytes_ncol"] == nb * npen * 4
                        assert P["bytes_inv"] == ldp * 4 and P["bytes_tri"] == nb * K * npen * nl * 24
                        assert P["bytes_pred"] == (nb * npen * nl * n * 8 if keep else 0)
                        assert P["cv_nwg"] >= 1 and P["cv_nwg"] <= max(1, num_cu // (K * npen * nb))
                        xv_parts = ["bytes_col", "bytes_yp", "bytes_cfirst", "bytes_part", "bytes_comp", "bytes_tab", "bytes_cvpart", "bytes_cvout"]
                        assert P["bytes_xval"] == P["bytes_single"] + sum(_r256(P[k]) for k in xv_parts)
                        assert P["bytes"] == P["bytes_xval"] + sum(_r256(P[k]) for k in PARTS)
    if num_cu == 256:
        assert {(1, 0), (2, 0), (0, 1)} <= seen, seen


def test_plan_nb_limit_and_refusals(oa, api):
    full = api.cv_multi_plan(3000, 41, 4, 50, 1, 12, 256)
    half = api.cv_multi_plan(3000, 41, 4, 50, 1, 12, 256, nb_limit=7)
    assert full["nb"] == 50 and half["nb"] == 7 and half["solve_chunks"] == 8 and half["bytes"] < full["bytes"]
    lib = oa.lib()
    out = (C.c_int64 * 27)()
    good = [100, 4, 3, 2, 1, 10, 256]
    for k in range(7):
        args = list(good)
        args[k] = 0
        assert lib.oemgpu_selftest_cv_multi_plan(*args, 0, 0, out) == ERR_ARG, k
    assert lib.oemgpu_selftest_cv_multi_plan(100, 4, 1, 2, 1, 10, 256, 0, 0, out) == ERR_ARG
    assert lib.oemgpu_selftest_cv_multi_plan(100, 4, 513, 2, 1, 10, 256, 0, 0, out) == ERR_ARG
    assert lib.oemgpu_selftest_cv_multi_plan(*good, 0, -1, out) == ERR_ARG
    assert lib.oemgpu_selftest_cv_multi_plan(*good, 0, 0, None) == ERR_ARG
    assert lib.oemgpu_selftest_cv_multi_plan(4, 4, 3, 2, 1, 10, 256, 0, 0, out) == ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ the index table
def _grids(rng, K, npen, nl, spread=0.2):
    """a full grid and K fold grids per penalty, geometric and descending, the folds' ends scattered about the full grid's"""
    full = np.stack([np.geomspace(rng.uniform(0.5, 2.0), rng.uniform(1e-4, 1e-2), nl) for _ in range(npen)]) if nl > 1 else rng.uniform(0.5, 2.0, (npen, 1))
    fold = np.zeros((K, npen, nl))
    for k in range(K):
        for m in range(npen):
            hi, lo = full[m, 0] * np.exp(rng.normal() * spread), full[m, -1] * np.exp(rng.normal() * spread)
            fold[k, m] = np.geomspace(hi, lo, nl) if nl > 1 else hi
    return full, fold


def _fits_of(fold, beta, p):
    """the fold fits as predict() reads them: beta[k][m] is (p + 1) x nl"""
    K, npen, nl = fold.shape
    return [{"beta": [beta[k, m].T.copy() for m in range(npen)], "lambda": [fold[k, m].copy() for m in range(npen)],
             "penalty": ["lasso"] * npen} for k in range(K)]


def _apply(beta, left, right, frac, ncol):
    """what cv_interp_kernel evaluates, in numpy: [K, npen, nl, p + 1]"""
    K, npen, nl, _ = beta.shape
    out = np.zeros_like(beta)
    for k in range(K):
        for m in range(npen):
            c = ncol[m]
            f = frac[k, m, :c, None]
            out[k, m, :c] = beta[k, m, left[k, m, :c]] * f + beta[k, m, right[k, m, :c]] * (1 - f)
    return out


@pytest.mark.parametrize("nl", [2, 3, 7, 16, 17, 100])
def test_index_table_against_lambda_interp(api, nl):
    p, K, npen = 6, 5, 3
    for seed in range(20):
        rng = np.random.default_rng(100 * nl + seed)
        full, fold = _grids(rng, K, npen, nl)
        beta = rng.normal(size=(K, npen, nl, p + 1))
        left, right, frac, ncol = api.cv_multi_interp_table(full, fold)
        which = [full[m] >= max(fold[k, m].min() for k in range(K)) for m in range(npen)]
        ref, ncol_ref = api._cv_gaussian_table(_fits_of(fold, beta, p), list(full), which, p)
        assert np.array_equal(ncol, ncol_ref)
        assert left.min() >= 0 and right.max() < nl
        got = _apply(beta, left, right, frac, ncol)
        for k in range(K):
            for m in range(npen):
                lam = fold[k, m]
                g = np.min(np.abs(np.diff((lam[0] - lam) / (lam[0] - lam[-1]))))          # the smallest gap of lambda.interp's normalised grid
                bound = 32 * EPS * np.abs(beta[k, m]).max() / g
                err = np.abs(got[k, m] - ref[k, m]).max()
                assert err <= bound, (seed, k, m, err, bound)
                assert np.all(got[k, m, ncol[m]:] == 0.0) and np.all(ref[k, m, ncol[m]:] == 0.0)


def test_index_table_on_a_shared_grid_is_exact(api):
    """a user lambda: every fold's grid is the full grid -- left = right, frac = 1, the coefficients pass through bit for bit"""
    rng = np.random.default_rng(7)
    K, npen, nl, p = 4, 2, 17, 5
    full = np.stack([np.geomspace(1.5, 2e-3, nl), np.geomspace(1.0, 1e-3, nl)])
    fold = np.broadcast_to(full, (K, npen, nl)).copy()
    beta = rng.normal(size=(K, npen, nl, p + 1))
    left, right, frac, ncol = api.cv_multi_interp_table(full, fold)
    assert ncol.tolist() == [nl, nl]
    assert np.array_equal(left, right) and np.all(frac == 1.0) and np.array_equal(left, np.broadcast_to(np.arange(nl), left.shape))
    assert np.array_equal(_apply(beta, left, right, frac, ncol), beta)
    ref, _ = api._cv_gaussian_table(_fits_of(fold, beta, p), list(full), [np.ones(nl, bool)] * npen, p)
    assert np.array_equal(ref, beta)


def test_index_table_ncol_edges(api):
    K, nl = 3, 9
    full = np.stack([np.geomspace(1.0, 1e-3, nl), np.geomspace(1.0, 1e-3, nl)])
    fold = np.zeros((K, 2, nl))
    fold[:, 0] = np.geomspace(50.0, 2.0, nl)                       # penalty 0: every fold's smallest lambda lies above the whole full grid
    fold[:, 1] = np.geomspace(2.0, 1e-4, nl)                       # penalty 1: below it
    left, right, frac, ncol = api.cv_multi_interp_table(full, fold)
    assert ncol.tolist() == [0, nl]
    assert np.all(left[:, 0] == 0) and np.all(right[:, 0] == 0) and np.all(frac[:, 0] == 1.0)
    fold[1, 1] = np.geomspace(2.0, full[1, 4], nl)                 # one fold stops at the full grid's column 4: columns 0..4 stay
    assert api.cv_multi_interp_table(full, fold)[3].tolist() == [0, 5]
    # a grid of one lambda: lambda.interp's own case, (0, 0, 1) whatever the values are
    l1, r1, f1, n1 = api.cv_multi_interp_table(np.array([[0.5]]), np.array([[[0.7]], [[0.4]], [[0.5]]]))
    assert n1.tolist() == [0] and np.all(l1 == 0) and np.all(r1 == 0) and np.all(f1 == 1.0)
    l1, r1, f1, n1 = api.cv_multi_interp_table(np.array([[0.9]]), np.array([[[0.7]], [[0.4]], [[0.5]]]))
    assert n1.tolist() == [1] and np.all(l1 == 0) and np.all(r1 == 0) and np.all(f1 == 1.0)
    z, z2, one = api._lambda_interp(np.array([0.7]), np.array([0.9]))
    assert z.tolist() == [0] and z2.tolist() == [0] and one.tolist() == [1.0]


def test_index_table_refusals(oa):
    from oem_amd import _lib as L
    lib = oa.lib()
    d, i = (C.c_double * 8)(), (C.c_int32 * 8)()
    dp, ip = C.cast(d, L._dp), C.cast(i, L._ip)
    assert lib.oemgpu_selftest_cv_interp(2, 1, 2, dp, dp, ip, ip, dp, ip) == 0
    assert lib.oemgpu_selftest_cv_interp(0, 1, 2, dp, dp, ip, ip, dp, ip) == ERR_ARG
    assert lib.oemgpu_selftest_cv_interp(2, 0, 2, dp, dp, ip, ip, dp, ip) == ERR_ARG
    assert lib.oemgpu_selftest_cv_interp(2, 1, 0, dp, dp, ip, ip, dp, ip) == ERR_ARG
    assert lib.oemgpu_selftest_cv_interp(2, 1, 2, None, dp, ip, ip, dp, ip) == ERR_ARG
    assert lib.oemgpu_selftest_cv_interp(2, 1, 2, dp, dp, ip, ip, dp, None) == ERR_ARG


# ------------------------------------------------------------------------------------------------ the vectorised statistics
def _triples(rng, R, K, npen, nl, ncol):
    """per-fold (count, mean, M2) as the scoring writes them: (0, NaN, NaN) from ncol on; fold 2 empty; fold 0 of one row (M2 = 0)"""
    fold_n = rng.integers(5, 40, size=K).astype(np.int64)
    fold_n[0] = 1
    if K > 2:
        fold_n[2] = 0
    t = np.zeros((R, K, npen, nl, 3))
    t[..., 0] = fold_n[None, :, None, None]
    t[..., 1] = rng.uniform(0.5, 2.0, size=(R, K, npen, nl))
    t[..., 2] = rng.uniform(0.1, 1.0, size=(R, K, npen, nl)) * (fold_n[None, :, None, None] > 1)
    for r in range(R):
        for m in range(npen):
            t[r, :, m, ncol[r, m]:] = (0.0, np.nan, np.nan)
    t[:, fold_n == 0] = (0.0, np.nan, np.nan)
    return t, fold_n


@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "rows"])
def test_vectorised_statistics_equal_the_loop(oa, api, grouped):
    rng = np.random.default_rng(11)
    R, K, npen, nl = 6, 5, 3, 13
    ncol = rng.integers(0, nl + 1, size=(R, npen))
    ncol[0], ncol[1], ncol[2, -1] = nl, (0, nl, 3), 0
    t, fold_n = _triples(rng, R, K, npen, nl, ncol)
    a = api._Args(["lasso"] * npen, [np.zeros(0)] * npen, nl, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(4), np.zeros(0, np.int32),
                  np.zeros(0, np.int32), np.zeros(0))
    dev = {"fold_n": fold_n, "args": a}
    cvm, cvsd = api._cv_gaussian_triple_stats_many(fold_n, t, ncol[:, -1], grouped)
    assert cvm.shape == cvsd.shape == (R, npen, nl)
    for r in range(R):
        want_m, want_s = api._cv_gaussian_triple_stats(dev, t[r], np.full(K, ncol[r, -1]), grouped)
        for m in range(npen):
            assert np.allclose(cvm[r, m], want_m[m], rtol=1e-13, atol=0, equal_nan=True), (r, m)
            assert np.allclose(cvsd[r, m], want_s[m], rtol=1e-13, atol=0, equal_nan=True), (r, m)
    assert np.isnan(cvm).any() and np.isfinite(cvsd).any()


def test_vectorised_weighted_statistics_with_nan_columns_an_empty_fold_and_n_of_one(api):
    rng = np.random.default_rng(12)
    R, K, nl = 4, 6, 9
    raw = rng.uniform(0.5, 2.0, size=(R, K, nl))
    raw[:, :, 7] = np.nan                                          # a column no fold has an error for
    raw[:, 3, :] = np.nan                                          # an empty fold
    raw[1, 1:, 2] = np.nan                                         # one entry left
    w = rng.uniform(1.0, 30.0, size=K)
    w[0] = 4.0                                                     # (a power of two: a w / w is a, so the lone entry's deviation is exactly 0)
    # N = 1: cvsd is 0 / 0 = NaN where one entry is left (its deviation is 0), x / 0 = inf elsewhere; N = 0: the root of a negative
    N = np.tile(np.array([K, K, 1, K, 0, 2, K, K, K], dtype=np.float64), (R, 1))
    cvm, cvsd = api._cv_weighted_stats_many(raw, w, N)
    want_m, want_s = api._cv_weighted_stats([raw[r].copy() for r in range(R)], [w] * R, [N[r] for r in range(R)])
    for r in range(R):
        assert np.allclose(cvm[r], want_m[r], rtol=1e-13, atol=0, equal_nan=True)
        assert np.allclose(cvsd[r], want_s[r], rtol=1e-13, atol=0, equal_nan=True)
    assert np.all(np.isnan(cvm[:, 7])) and np.isnan(cvsd[1, 2]) and np.isinf(cvsd[0, 2]) and np.all(np.isnan(cvsd[:, 4]))
    assert np.all(np.isfinite(cvsd[:, 0])) and np.all(np.isfinite(cvm[:, :7]))


# ------------------------------------------------------------------------------------------------ refusals before any device
def test_cv_oem_multi_refuses_before_any_device(oa):
    import scipy.sparse as sp
    rng = np.random.default_rng(0)
    n, p, m = 40, 5, 3
    x, Y = rng.normal(size=(n, p)), rng.normal(size=(n, m))
    lop = np.ones(n, dtype=np.int64)
    lop[:3], lop[3:5] = 2, 3                                       # fold 1 holds 35 rows: its fit would keep 5 <= p
    cases = [
        (dict(x=x, Y=Y), "one response at a time with cv_oem()"),
        (dict(x=sp.csc_matrix(x), Y=Y), "one response at a time with cv_oem()"),
        (dict(x=x, Y=Y, weights=np.ones(n)), "no observation weights"),
        (dict(x=x, Y=Y, ngpus=2), "ngpus / devices"),
        (dict(x=x, Y=Y, devices=[0]), "ngpus / devices"),
        (dict(x=x, Y=Y, penalty=["lasso", "ols"]), "\"ols\" penalty is not served; cv_oem() takes it"),
        (dict(x=x, Y=Y, family="binomial"), "cv_oem_logistic_multi()"),
        (dict(x=x, Y=Y, family="poisson"), "'arg' should be one of"),
        (dict(x=x, Y=Y, type_measure="rmse"), "'arg' should be one of"),
        (dict(x=x, Y=Y[:, 0]), "Y must be a matrix"),
        (dict(x=x, Y=Y[:, :0]), "at least one column"),
        (dict(x=x, Y=Y[:-1]), "x and y lengths do not match"),
        (dict(x=rng.normal(size=(5, 5)), Y=Y[:5]), "serves n > p only"),
        (dict(x=rng.normal(size=(4, 5)), Y=Y[:4]), "cv_oem(x, Y[:, r])"),
        (dict(x=x[:, :1], Y=Y), "x must have at least two columns"),
        (dict(x=x, Y=Y, lambda_=[0.1]), "Need more than one value of lambda for cv.oem"),
        (dict(x=x, Y=Y, nfolds=2), "nfolds must be bigger than 3"),
        (dict(x=x, Y=Y, foldid=np.resize(np.arange(1, 3), n)), "nfolds must be bigger than 3"),
        (dict(x=x, Y=Y, foldid=lop), "fold 1 leaves 5 rows for 5 columns; cv_oem() sends such folds to its host loop"),
        (dict(x=x, Y=Y, foldid=np.resize(np.arange(0, 4), n)), "foldid must hold one integer in 1..nfolds"),
        (dict(x=x, Y=Y, foldid=np.resize(np.arange(1, 5), n - 1)), "foldid must hold one integer in 1..nfolds"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError) as e:
            oa.cv_oem_multi(kw.pop("x"), kw.pop("Y"), **kw)
        assert what in str(e.value), (what, str(e.value))


def test_cv_oem_multi_refuses_a_sparse_handle(oa, api):
    class Handle(api.SparseX):                                     # (a SparseX without a device: only its type is looked at)
        def __init__(self):
            self._h = None
        shape = (40, 5)
    with pytest.raises(ValueError) as e:
        oa.cv_oem_multi(Handle(), np.zeros((40, 2)))
    assert "one response at a time with cv_oem()" in str(e.value)


CTX, PTR = C.c_void_p(0x1000), C.c_void_p(0x2000)
# (ctx, x, dtype or None for the column-major entry, n, ld, p, y, rs, cs, m, foldid, nfolds, type_measure): oemgpu_xval_dense_multi_dev's
# cases and codes (tests/test_xval_multi_cpu.py)
C_CASES = [
    ((None, PTR, None, 40, 40, 4, PTR, 3, 1, 3, PTR, 4, 0), ERR_ARG, "NULL ctx"),
    ((CTX, None, None, 40, 40, 4, PTR, 3, 1, 3, PTR, 4, 0), ERR_ARG, "NULL x"),
    ((CTX, PTR, None, 40, 40, 4, None, 3, 1, 3, PTR, 4, 0), ERR_ARG, "NULL y"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 3, 1, 3, None, 4, 0), ERR_ARG, "NULL foldid"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 3, 1, 0, PTR, 4, 0), ERR_ARG, "m < 1"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 2, 1, 3, PTR, 4, 0), ERR_ARG, "row-major Y with rs < m"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 1, 39, 3, PTR, 4, 0), ERR_ARG, "column-major Y with cs < n"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 3, 2, 3, PTR, 4, 0), ERR_ARG, "no unit stride"),
    ((CTX, PTR, None, 40, 39, 4, PTR, 3, 1, 3, PTR, 4, 0), ERR_ARG, "ld < n"),
    ((CTX, PTR, 0, 40, 3, 4, PTR, 3, 1, 3, PTR, 4, 0), ERR_ARG, "ldr < p"),
    ((CTX, PTR, 2, 40, 4, 4, PTR, 3, 1, 3, PTR, 4, 0), ERR_ARG, "a dtype that is none"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 3, 1, 3, PTR, 1, 0), ERR_ARG, "nfolds < 2"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 3, 1, 3, PTR, 513, 0), ERR_ARG, "nfolds > 512"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 3, 1, 3, PTR, 4, 2), ERR_ARG, "type_measure outside {0, 1}"),
    ((CTX, PTR, None, 4, 4, 4, PTR, 3, 1, 3, PTR, 4, 0), ERR_UNSUPPORTED, "n <= p"),
    ((CTX, PTR, 1, 3, 4, 4, PTR, 3, 1, 3, PTR, 3, 0), ERR_UNSUPPORTED, "n <= p, row-major"),
    ((CTX, PTR, None, 6, 6, 4, PTR, 3, 1, 3, PTR, 3, 0), ERR_UNSUPPORTED, "n - largest fold <= p"),
    ((CTX, PTR, 0, 7, 4, 4, PTR, 3, 1, 3, PTR, 3, 0), ERR_UNSUPPORTED, "n - largest fold <= p, row-major"),
]


# the sentence of every refusal that is an OEMGPU_ERR_ARG (the OEMGPU_ERR_UNSUPPORTED ones name the rows, folds and columns)
SENTENCES = {'NULL ctx': 'NULL argument', 'NULL x': 'NULL argument', 'NULL y': 'NULL argument', 'NULL foldid': 'NULL argument', 'm < 1': 'm < 1 (at least one response)', 'row-major Y with rs < m': 'are neither a row-major n x m matrix', 'column-major Y with cs < n': 'are neither a row-major n x m matrix', 'no unit stride': 'are neither a row-major n x m matrix', 'ld < n': 'ld < n', 'ldr < p': 'ldr < p', 'a dtype that is none': 'dtype is neither OEMGPU_F64 nor OEMGPU_F32', 'nfolds < 2': 'nfolds must be in 2..512', 'nfolds > 512': 'nfolds must be in 2..512', 'type_measure outside {0, 1}': 'type_measure must be 0 (mse) or 1 (mae)'}


def _opts(api, p):
    return api._Args(["lasso"], [np.zeros(0)], 5, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(p), np.zeros(0, np.int32),
                     np.zeros(0, np.int32), np.zeros(0))


def _outs():
    from oem_amd import _lib as L
    i64 = C.POINTER(C.c_int64)
    return [C.cast(PTR, t) for t in (L._dp, L._dp, L._ip, L._dp, L._dp, L._ip, L._dp, i64, L._ip)]


def _call(lib, args, opts, outs, optional=(None, None, None, None)):
    ctx, x, dt, n, ld, p, y, rs, cs, m, fold, K, tm = args
    if dt is None:
        return lib.oemgpu_cv_dense_multi_dev(ctx, x, n, ld, p, y, rs, cs, m, fold, K, 1, 1, tm, opts, *outs, *optional)
    return lib.oemgpu_cv_dense_multi_rm_dev(ctx, x, dt, n, ld, p, y, rs, cs, m, fold, K, 1, 1, tm, opts, *outs, *optional)


@pytest.mark.parametrize("args,code,what", C_CASES, ids=[c[2] for c in C_CASES])
def test_c_entries_refuse_before_any_device(oa, api, args, code, what):
    lib = oa.lib()
    a = _opts(api, args[5])
    rc = _call(lib, args, C.byref(a.c), _outs())
    assert rc == code, (what, rc, lib.oemgpu_last_error())
    # the same arguments, the same code from oemgpu_xval_dense_multi_dev
    from oem_amd import _lib as L
    xouts = [C.cast(PTR, t) for t in (L._dp, L._dp, L._ip, L._dp, L._dp, L._dp, L._dp, L._ip)]
    ctx, x, dt, n, ld, p, y, rs, cs, m, fold, K, tm = args
    if dt is None:
        assert lib.oemgpu_xval_dense_multi_dev(ctx, x, n, ld, p, y, rs, cs, m, fold, K, 1, 1, tm, C.byref(a.c), *xouts) == code
    else:
        assert lib.oemgpu_xval_dense_multi_rm_dev(ctx, x, dt, n, ld, p, y, rs, cs, m, fold, K, 1, 1, tm, C.byref(a.c), *xouts) == code
    _call(lib, args, C.byref(a.c), _outs())
    said = lib.oemgpu_last_error().decode()
    if code == ERR_UNSUPPORTED:
        assert "leave some fit no more rows than the 4 columns" in said and "cv_dense_multi" in said, said
    else:
        assert SENTENCES[what] in said, (what, said)


def test_c_entries_refuse_null_outputs_and_options(oa, api):
    lib = oa.lib()
    a = _opts(api, 4)
    args = (CTX, PTR, None, 40, 40, 4, PTR, 3, 1, 3, PTR, 4, 0)
    for k in range(9):
        outs = _outs()
        outs[k] = None
        assert _call(lib, args, C.byref(a.c), outs) == ERR_ARG, k
    assert _call(lib, args, None, _outs()) == ERR_ARG
    b = _opts(api, 4)
    b.c.npen = 0
    assert _call(lib, args, C.byref(b.c), _outs()) == ERR_ARG
    # "ols": a grid of one lambda, refused by name before a device is looked for (cv_oem_multi refuses it in Python)
    ols = api._Args(["lasso", "ols"], [np.zeros(0)] * 2, 5, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(4), np.zeros(0, np.int32),
                    np.zeros(0, np.int32), np.zeros(0))
    for dt in (None, 1):
        rm = (CTX, PTR, dt, 40, 40, 4, PTR, 3, 1, 3, PTR, 4, 0)
        assert _call(lib, rm, C.byref(ols.c), _outs()) == ERR_UNSUPPORTED
        assert b'the "ols" penalty is not served' in lib.oemgpu_last_error()
    assert lib.oemgpu_selftest_cv_multi_nb_limit(-1) == ERR_ARG and b"negative limit" in lib.oemgpu_last_error()
    assert lib.oemgpu_selftest_cv_multi_nb_limit(3) == 0 and lib.oemgpu_selftest_cv_multi_nb_limit(0) == 0
    assert lib.oemgpu_last_cv_multi_timings(None) == ERR_ARG
    t = (C.c_double * 7)(*([1.0] * 7))
    assert lib.oemgpu_last_cv_multi_timings(t) == 0 and list(t) == [0.0] * 7          # no call on this thread yet


def test_score_selftest_refuses_before_any_device(oa):
    from oem_amd import _lib as L
    lib = oa.lib()
    dp, ip = C.cast(PTR, L._dp), C.cast(PTR, L._ip)
    ncol = (C.c_int32 * 3)(2, 2, 2)
    nc = C.cast(ncol, L._ip)

    def call(ctx=CTX, x=PTR, n=40, ld=40, p=4, y=PTR, rs=3, cs=1, m=3, fold=PTR, K=4, coef=dp, npen=1, nl=2, ncol_=nc, tm=0, nb=2,
             left=None, right=None, frac=None, tri=dp):
        return lib.oemgpu_selftest_cv_score_multi_dev(ctx, x, n, ld, p, y, rs, cs, m, fold, K, coef, npen, nl, ncol_, tm, nb, left, right, frac,
                                                      None, tri, None)
    for kw in (dict(ctx=None), dict(x=None), dict(y=None), dict(fold=None), dict(coef=None), dict(ncol_=None), dict(tri=None), dict(p=0),
               dict(npen=0), dict(nl=0), dict(nb=0), dict(K=1), dict(K=513), dict(tm=2), dict(m=0), dict(rs=2), dict(ld=39), dict(left=ip)):
        assert call(**kw) == ERR_ARG, kw
    bad = (C.c_int32 * 3)(2, 3, 2)
    assert call(ncol_=C.cast(bad, L._ip)) == ERR_ARG and b"ncol[1] = 3" in lib.oemgpu_last_error()
