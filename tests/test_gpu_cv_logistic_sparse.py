"""cv.oem for binomial fits on a sparse x on the MI355X: the fold entry on a resident x (oemgpu_fit_logistic_sparse_fold_res) against the
CPU restatement of the sparse fit on the sliced matrix x[keep], y[keep]; the scoring entry (oemgpu_logistic_cv_score_sparse_res) against
the dense entry on x.toarray(), bit for bit, and against numpy; cv_oem(family="binomial") on a scipy.sparse x end to end against
tests/cv_logistic_restatement.py fed with the sparse restatement's fits; and the Python surface (SparseX, any sparse format, predict_cv).

Tolerances of the fold entry are those of the sparse fit (tests/test_gpu_logistic_sparse._compare): beta 1e-8, lambda 1e-12, loss and d
1e-10, identical niter, and the restatement's step counters against oem_amd.logistic_stats().  Scoring against numpy: deviance / mse /
mae rtol 1e-10, class sums and counts exact, predmat 1e-12 (tests/test_gpu_cv_logistic._check_scores' figures).  End to end, cvm / cvsd /
cvup / cvlo / fit.preval: CV_TOL (1 + |value|), CV_TOL = 100 x the largest difference of the first green run, capped at 1e-6.

The base matrix: n = 9000, p = 40, scipy.sparse.random at density 0.05 (seed 11, normal values), column 0 overwritten by a full N(0, 1)
column; five folds.  9000 rows are two 8192-row chunks of the compressed-column kernels, and at 256 CUs a row-pass workgroup owns 64
rows.  Every fold case runs on both Gram routes (OEM_SPARSE_GRAM = csc / dense, the latter with one 9000-row tile and with 2048-row
tiles) and asserts through the plan selftests that it landed there.

Preconditions are asserted on the restatement, never on the library, and exclude no case (the end-to-end ones are _check_cv_oem's).
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from tests import cv_logistic_restatement as CV
from tests import logistic_sparse_restatement as RS
from tests.test_gpu_cv_logistic import _numpy_scores, _rel
from tests.test_gpu_logistic_sparse import _compare

pytestmark = pytest.mark.gpu

CV_TOL = 2.9e-13         # x (1 + |value|): the first green run's largest difference was 2.83e-15 (fit.preval on the default grid; cvm / cvsd 4.7e-16)

N, P, K = 9000, 40, 5
ROUTES = [pytest.param("csc", None, id="csc"), pytest.param("dense", None, id="one-tile"), pytest.param("dense", 2048, id="tiles-2048")]


@pytest.fixture(scope="module")
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------------------- data, shared references
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _base():
    """(x, y, foldid): the base matrix, the response of coefficients 2 N(0, 1) on the first ten columns (the first 1.5, offset -0.3) and
    random folds from default_rng(5)"""
    def make():
        rng = np.random.default_rng(11)
        x = sp.random(N, P, density=0.05, format="lil", random_state=rng, data_rvs=lambda m: rng.normal(size=m))
        x[:, 0] = rng.normal(size=(N, 1))
        x = sp.csc_matrix(x)
        x.sort_indices()
        b = np.zeros(P)
        b[:10] = 2.0 * rng.normal(size=10)
        b[0] = 1.5
        y = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-(x @ b - 0.3)))).astype(np.float64)
        fid = np.random.default_rng(5).permutation(np.resize(np.arange(1, K + 1), N))
        assert x.nnz > N and np.diff(x.indptr)[0] == N
        return x, y, fid
    return _cached("base", make)


def _ref_fold(key, x, y, fid, i, pens, **kw):
    """the restatement on the sliced matrix, once per (case, fold): (fit, step counts)"""
    def make():
        keep = fid != i
        st = {}
        return RS.fit(x[keep], y[keep], penalty=pens, stats=st, **kw), st
    return _cached((key, i), make)


def _set_route(monkeypatch, num_cu, gram, tile, n, p, nnz, intercept=True):
    """sets the switches of a Gram route and asserts, on the resident plan, that a call lands there"""
    import oem_amd
    monkeypatch.setenv("OEM_SPARSE_GRAM", gram)
    if tile is None:
        monkeypatch.delenv("OEM_SPARSE_TILE_ROWS", raising=False)
    else:
        monkeypatch.setenv("OEM_SPARSE_TILE_ROWS", str(tile))
    out = (C.c_int64 * 8)()
    assert oem_amd.lib().oemgpu_selftest_logistic_sparse_res_plan(n, p, nnz, int(intercept), num_cu, out) == 0
    csc, inner_wg, ws, bound, rows, nch, ch, chunks = list(out)
    assert csc == (1 if gram == "csc" else 0), list(out)
    assert rows == (0 if gram == "csc" else min(n, tile) if tile else n), list(out)
    assert chunks == -(-n // 8192) and inner_wg == 1 and 0 < ws <= bound
    return dict(tile_rows=rows, row_wgs=nch, row_ch=ch, chunks=chunks)


def _dev(y, fid):
    import torch
    return (torch.as_tensor(np.asarray(y, dtype=np.float64), device="cuda:0"),
            torch.as_tensor(np.ascontiguousarray(fid, dtype=np.int32), device="cuda:0"))


def _fold_fit(sx, y, yd, fd, nfolds, leave_out, pens, **kw):
    import oem_amd
    return oem_amd.oem_fit_logistic_sparse(sx, y, penalty=pens, _fold=(sx, fd, nfolds, leave_out, yd), **kw)


def _same(a, b, pens):
    for k in range(len(pens)):
        for key in ("beta", "lambda", "niter", "loss"):
            assert np.asarray(a[key][k]).tobytes() == np.asarray(b[key][k]).tobytes(), (key, pens[k])
    assert a["d"] == b["d"]


def _check_folds(key, x, y, fid, pens, folds=None, fits=None, **kw):
    """the fold entry against the restatement on the sliced matrix for the folds named (all by default), results and step counts;
    returns the restatement's step counts per fold"""
    import oem_amd
    nfolds = int(fid.max())
    yd, fd = _dev(y, fid)
    stats = []
    with oem_amd.SparseX(x) as sx:
        for i in (folds if folds is not None else range(1, nfolds + 1)):
            fit = _fold_fit(sx, y, yd, fd, nfolds, i, pens, **kw)
            ref, st = _ref_fold(key, x, y, fid, i, pens, **kw)
            _compare(fit, ref, pens)
            assert fit["nobs"] == int((fid != i).sum())
            gst = oem_amd.logistic_stats()
            assert gst["irls_steps"] == st["irls"] and gst["inner_iters"] == st["inner"], (i, gst, st)
            assert gst["row_passes"] == st["rows"] and gst["grams"] == st["grams"], (i, gst, st)
            stats.append(st)
            if fits is not None:
                fits.append(fit)
    return stats


# ------------------------------------------------------------------------------------------------------------- the fold entry
@pytest.mark.parametrize("gram,tile", ROUTES)
def test_fold_entry_random_folds(monkeypatch, num_cu, gram, tile):
    x, y, fid = _base()
    plan = _set_route(monkeypatch, num_cu, gram, tile, N, P, x.nnz)
    assert plan["chunks"] == 2 and (num_cu != 256 or plan["row_ch"] == 64)
    _check_folds("random", x, y, fid, ["lasso", "mcp"], nlambda=20, compute_loss=True)


def _contiguous_folds():
    """A: fold 1 is rows 256 .. 447 (three whole 64-row row-pass workgroups), fold 2 rows 8192 .. 8999 (the whole second chunk of the
    compressed-column kernels and, with 2048-row tiles, the whole last tile), folds 3 .. 5 random over the rest.  B: fold 1 is the last
    row and nothing else"""
    x, y, _ = _base()
    rng = np.random.default_rng(21)
    a = rng.permutation(np.resize(np.arange(3, K + 1), N))
    a[256:448] = 1
    a[8192:] = 2
    b = rng.permutation(np.resize(np.arange(2, K + 1), N))
    b[-1] = 1
    assert (a == 1).sum() == 192 and (a == 2).sum() == N - 8192 and (b == 1).sum() == 1
    return x, y, a, b


@pytest.mark.parametrize("gram,tile", ROUTES)
def test_fold_entry_contiguous_folds(monkeypatch, num_cu, gram, tile):
    x, y, a, b = _contiguous_folds()
    _set_route(monkeypatch, num_cu, gram, tile, N, P, x.nnz)
    kw = dict(nlambda=12, compute_loss=True)
    _check_folds("contiguous-a", x, y, a, ["lasso"], folds=(1, 2), **kw)
    _check_folds("contiguous-b", x, y, b, ["lasso"], folds=(1,), **kw)


@pytest.mark.parametrize("gram,tile", ROUTES)
def test_fold_entry_an_emptied_column(monkeypatch, num_cu, gram, tile):
    """every stored entry of column 7 lies in fold 2: without fold 2 its colsq is 0 -> 1, as on the sliced matrix, and its coefficient
    stays 0; the other folds keep some of it"""
    x, y, fid = _base()
    fid = fid.copy()
    rows7 = x.indices[x.indptr[7]:x.indptr[8]]
    fid[rows7] = 2
    assert len(rows7) > 100 and x[fid != 2][:, 7].nnz == 0
    _set_route(monkeypatch, num_cu, gram, tile, N, P, x.nnz)
    fits = []
    _check_folds("emptied", x, y, fid, ["lasso", "mcp"], folds=(2, 1), fits=fits, nlambda=12, compute_loss=True)
    assert np.all(np.asarray(fits[0]["beta"][0])[8] == 0.0) and np.any(np.asarray(fits[1]["beta"][0])[8] != 0.0)


def _floor_case():
    """near-separable: rows 0 .. 15 carry +-30 in column 0 (coefficient 1.5: |eta| = 45, W = 0 in double) with the matching y, so the W
    floor fires at the IRLS steps whose index is one of them.  Folds over these rows: 1 2 3 4 5 1 2 ..., so fold f leaves out row f - 1
    and the map from IRLS index to kept row leaves the identity at index f - 1.  Every one of these rows is saturated, so WHICH of them
    is floored would move the Hessian by a few 1e-4 of single entries and beta by 1e-9 (restatement, rows re-ordered as an identity
    map would see them): under the tolerance.  Row r therefore also carries +-10 (r + 1) in column 1: the floored row adds
    1e-5 (10 (r + 1))^2 to X'WX[1][1], a different amount for every row, and the same re-ordering moves beta by 2e-6 .. 1e-5"""
    def make():
        x, y, fid = _base()
        x = x.tolil(copy=True)
        y = y.copy()
        fid = fid.copy()
        sign = np.where(np.arange(16) % 2 == 0, 1.0, -1.0)
        x[:16, 0] = (30.0 * sign)[:, None]
        x[:16, 1] = (10.0 * np.arange(1, 17) * sign)[:, None]
        y[:16] = (sign > 0).astype(np.float64)
        fid[:16] = np.resize(np.arange(1, K + 1), 16)
        x = sp.csc_matrix(x)
        x.sort_indices()
        return x, y, fid
    return _cached("floor", make)


@pytest.mark.parametrize("gram,tile", ROUTES)
def test_fold_entry_w_floor_tests_the_kept_row(monkeypatch, num_cu, gram, tile):
    """the Hessian is rebuilt at every IRLS step of this fit, so the floored W is felt.  A scratch build whose floor tests row i instead
    of the i-th kept row fails this case on all three routes and no other case of this file"""
    x, y, fid = _floor_case()
    _set_route(monkeypatch, num_cu, gram, tile, N, P, x.nnz)
    pens, kw = ["lasso"], dict(nlambda=15, lambda_min_ratio=1e-3, compute_loss=True)
    stats = _check_folds("floor", x, y, fid, pens, **kw)
    for i, st in enumerate(stats, start=1):
        ref, _ = _ref_fold("floor", x, y, fid, i, pens, **kw)
        steps = int(np.max(ref["niter"][0])) - 1                       # IRLS indices 0 .. steps - 1 were tested by the floor
        first_moved = i - 1                                            # the first index whose kept row is not the row of that number
        assert np.nonzero(fid != i)[0][first_moved] != first_moved
        assert st["floored"] > 0 and steps > first_moved, (i, st, steps)


@pytest.mark.parametrize("gram,tile", ROUTES)
def test_leave_out_zero_is_the_plain_sparse_fit_bit_for_bit(monkeypatch, num_cu, gram, tile):
    import oem_amd
    x, y, fid = _base()
    _set_route(monkeypatch, num_cu, gram, tile, N, P, x.nnz)
    pens, kw = ["lasso", "mcp"], dict(nlambda=10, compute_loss=True)
    yd, fd = _dev(y, fid)
    plain = oem_amd.oem_fit_logistic_sparse(x, y, penalty=pens, **kw)
    with oem_amd.SparseX(x) as sx:
        for f in (fd, None):                                           # foldid may be NULL with nothing left out
            got = _fold_fit(sx, y, yd, f, K, 0, pens, **kw)
            _same(got, plain, pens)
            assert got["nobs"] == N


@pytest.mark.parametrize("gram,tile", ROUTES)
def test_fold_entry_is_repeatable(monkeypatch, num_cu, gram, tile):
    import oem_amd
    x, y, fid = _floor_case()
    _set_route(monkeypatch, num_cu, gram, tile, N, P, x.nnz)
    pens, kw = ["lasso", "scad"], dict(nlambda=10, irls_maxit=30, compute_loss=True)
    yd, fd = _dev(y, fid)
    with oem_amd.SparseX(x) as sx:
        _same(_fold_fit(sx, y, yd, fd, K, 3, pens, **kw), _fold_fit(sx, y, yd, fd, K, 3, pens, **kw), pens)


@pytest.mark.parametrize("gram,tile", ROUTES)
def test_left_out_data_is_ignored(monkeypatch, num_cu, gram, tile):
    """the stored values of the left-out rows become 1e6 N(0, 1) and their y is flipped (even rows) or NaN (odd rows): the fold fit
    returns the bits it returns on the untouched data -- y is never read there and a finite x times W = r = 0 is exact"""
    import oem_amd
    x, y, fid = _base()
    _set_route(monkeypatch, num_cu, gram, tile, N, P, x.nnz)
    pens, kw = ["lasso", "mcp"], dict(nlambda=10, compute_loss=True)
    rng = np.random.default_rng(31)
    for i in (2, 5):
        x2 = x.copy()
        out = fid[x2.indices] == i
        x2.data[out] = 1e6 * rng.normal(size=int(out.sum()))
        y2 = y.copy()
        rows = np.nonzero(fid == i)[0]
        y2[rows[rows % 2 == 0]] = 1.0 - y2[rows[rows % 2 == 0]]
        y2[rows[rows % 2 == 1]] = np.nan
        assert out.sum() > 3000 and np.isnan(y2).sum() > 500
        yd, fd = _dev(y, fid)
        yd2, _ = _dev(y2, fid)
        with oem_amd.SparseX(x) as sx, oem_amd.SparseX(x2) as sx2:
            _same(_fold_fit(sx2, y, yd2, fd, K, i, pens, **kw), _fold_fit(sx, y, yd, fd, K, i, pens, **kw), pens)


def test_fold_entry_refusals():
    import oem_amd
    x, y, fid = _base()
    yd, _ = _dev(y, fid)
    with oem_amd.SparseX(x) as sx:
        for bad in (0, K + 1):                                         # an id outside 1 .. K, whatever is left out
            f2 = fid.copy()
            f2[777] = bad
            _, fd = _dev(y, f2)
            for leave_out in (1, 0):
                with pytest.raises(oem_amd.OemgpuError, match="fold ids") as e:
                    _fold_fit(sx, y, yd, fd, K, leave_out, ["lasso"], nlambda=4)
                assert e.value.code == -1
        _, fd = _dev(y, fid)
        with pytest.raises(oem_amd.OemgpuError, match="colsq_inv") as e:   # intercept without standardize
            _fold_fit(sx, y, yd, fd, K, 1, ["lasso"], nlambda=4, standardize=False)
        assert e.value.code == -4
        for leave_out in (-1, K + 1):
            with pytest.raises(oem_amd.OemgpuError, match="leave_out") as e:
                _fold_fit(sx, y, yd, fd, K, leave_out, ["lasso"], nlambda=4)
            assert e.value.code == -1
    # p + intercept = n_eff is refused and names the fold; one more kept row is fitted: n = 64, p = 50, 51 and 52 rows kept
    rng = np.random.default_rng(32)
    xs = sp.random(64, 50, density=0.3, format="csc", random_state=rng, data_rvs=lambda m: rng.normal(size=m))
    ys = (rng.uniform(size=64) < 0.5).astype(np.float64)
    fs = np.concatenate([np.full(13, 1), np.full(12, 2), np.resize(np.arange(3, 6), 39)])
    yd, fd = _dev(ys, fs)
    with oem_amd.SparseX(xs) as sx:
        with pytest.raises(oem_amd.OemgpuError, match="fold 1") as e:
            _fold_fit(sx, ys, yd, fd, K, 1, ["lasso"], nlambda=4)
        assert e.value.code == -4 and "51 rows" in str(e.value)
        fit = _fold_fit(sx, ys, yd, fd, K, 2, ["lasso"], nlambda=4, lambda_min_ratio=0.1)
    keep = fs != 2
    assert keep.sum() == 52
    _compare(fit, RS.fit(xs[keep], ys[keep], penalty=["lasso"], nlambda=4, lambda_min_ratio=0.1), ["lasso"])


# ------------------------------------------------------------------------------------------------------------- the scoring entry
def _dense_dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x.toarray().T), device="cuda:0").t()


def _check_scores(x, y, fid, coef):
    """the sparse scoring entry: the bits of the dense entry on x.toarray() (with and without predmat, and twice), and numpy at the dense
    test's tolerances.  Returns (sums, counts, predmat) of the sparse entry and numpy's"""
    import oem_amd
    from oem_amd import api
    nfolds = coef.shape[0]
    ref_sums, ref_counts, ref_pred = _numpy_scores(x.toarray(), y, fid, coef)
    gap = np.nanmin(np.abs(ref_pred - 0.5))
    print("min |prob - 0.5| =", gap)
    assert gap > 1e-7
    yd, fd = _dev(y, fid)
    with oem_amd.SparseX(x) as sx:
        got = api.logistic_cv_score(sx, yd, fd, nfolds, coef, predmat=True)
        again = api.logistic_cv_score(sx, yd, fd, nfolds, coef, predmat=True)
        nopred = api.logistic_cv_score(sx, yd, fd, nfolds, coef)
    dense = api.logistic_cv_score(_dense_dev(x), yd, fd, nfolds, coef, predmat=True)
    for a, b in zip(got, dense):
        assert a.tobytes() == b.tobytes()                              # sums, counts, predmat (NaN where a row has no fold)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    assert nopred[2] is None and nopred[0].tobytes() == got[0].tobytes() and nopred[1].tobytes() == got[1].tobytes()
    sums, counts, pred = got
    ok = ~np.isnan(ref_pred)
    assert np.array_equal(np.isnan(pred), ~ok)
    print("predmat max diff", np.abs(pred[ok] - ref_pred[ok]).max(), "sums max rel diff",
          np.max(np.abs(sums - ref_sums) / np.maximum(np.abs(ref_sums), 1e-300)))
    assert np.array_equal(counts, ref_counts)
    assert np.array_equal(sums[:, :, 2:4], ref_sums[:, :, 2:4])
    for t in (0, 4, 6):
        np.testing.assert_allclose(sums[:, :, t:t + 2], ref_sums[:, :, t:t + 2], rtol=1e-10)
    assert np.abs(pred[ok] - ref_pred[ok]).max() <= 1e-12
    return got, (ref_sums, ref_counts, ref_pred)


def _interpolated(fit0, outlist, p, m=0):
    """the table cv.oem scores model m with: the fold fits interpolated onto the full fit's lambdas (R/cv_oem.R:262-286)"""
    lam = np.asarray(fit0["lambda"][m])
    s = lam[lam >= max(np.min(o["lambda"][m]) for o in outlist)]
    coef = np.empty((len(outlist), len(s), p + 1))
    for i, o in enumerate(outlist):
        left, right, frac = CV.lambda_interp(o["lambda"][m], s)
        b = np.asarray(o["beta"][m])
        coef[i] = (b[:, left] * frac + b[:, right] * (1 - frac)).T
    return coef


@pytest.mark.parametrize("table", ["random-folds-mcp", "given-grid-lasso"])
def test_scoring_entry_on_the_cv_tables(table):
    """the tables cv.oem scores with, from the restatement's fits: the mcp fits of the random-folds case (20 lambdas of their own per
    fit) and the lasso fits of the end-to-end case (12 given lambdas).  (The lasso table of the first has a held-out probability
    3.7e-9 from 0.5, under _check_scores' precondition for the class rule; these two are 3.8e-6 and 7.5e-7 away.)"""
    x, y, fid = _base()
    if table == "random-folds-mcp":
        pens, kw = ["lasso", "mcp"], dict(nlambda=20, compute_loss=True)
        fit0 = _cached(("random", 0), lambda: (RS.fit(x, y, penalty=pens, **kw), None))[0]
        outlist = [_ref_fold("random", x, y, fid, i, pens, **kw)[0] for i in range(1, K + 1)]
        coef = _interpolated(fit0, outlist, P, m=1)
    else:
        coef = _interpolated(*_e2e("given")["fitted"], P)
    assert coef.shape[1] >= 10
    _check_scores(x, y, fid, coef)


def _table(seed, nfolds, ncol, q, density=0.1):
    """about `density` of the coefficients set, growing from column to column; every intercept set (a row without a stored entry
    then has prob = sigmoid(beta_0) away from 0.5)"""
    rng = np.random.default_rng(seed)
    t = rng.normal(size=(nfolds, ncol, q)) * (rng.uniform(size=(nfolds, ncol, q)) < density) * np.linspace(0.02, 0.6, ncol)[None, :, None]
    t[:, :, 0] = rng.choice([-1.0, 1.0], size=(nfolds, ncol)) * rng.uniform(0.2, 1.0, size=(nfolds, ncol))
    return t


def _small(n, p, seed, density=0.05):
    rng = np.random.default_rng(seed)
    x = sp.random(n, p, density=density, format="csc", random_state=rng, data_rvs=lambda m: rng.normal(size=m))
    y = (rng.uniform(size=n) < 0.5).astype(np.float64)
    return x, y, rng


@pytest.mark.parametrize("ncol,tlds", [(9, 1), (2100, 0)])
def test_scoring_entry_table_in_lds_and_through_the_cache(num_cu, ncol, tlds):
    """n = 200, p = 200: nine columns sit in LDS; 2100 columns are read through the cache, in two launches of at most 2048 per fold"""
    import oem_amd
    x, y, rng = _small(200, 200, 41)
    fid = rng.permutation(np.resize(np.arange(1, 4), 200))
    out = (C.c_int64 * 6)()
    assert oem_amd.lib().oemgpu_selftest_cv_score_plan(200, 200, ncol, num_cu, out) == 0
    assert out[2] == tlds and out[4] == (1 if tlds else 2), list(out)
    _check_scores(x, y, fid, _table(42, 3, ncol, 201))


@pytest.mark.parametrize("ncol", [1, 8, 33])
def test_scoring_entry_odd_rows(ncol):
    """rows without a stored entry (first, last, in the middle of a tile, and a whole tile of them): prob is sigmoid(beta_0), the same bits
    in every such row of a fold; fold 3 of four has no row; one column, one full column group and a last group of one"""
    x, y, rng = _small(300, 40, 43, density=0.1)
    x = x.tolil()
    empty = np.r_[0, 70, 299, 128:192]
    x[empty, :] = 0.0
    x = sp.csc_matrix(x)
    x.eliminate_zeros()
    assert x[empty].nnz == 0 and x.nnz > 500
    fid = rng.permutation(np.resize(np.array([1, 2, 4]), 300))
    coef = _table(44, 4, ncol, 41, density=0.3)
    (sums, counts, pred), _ = _check_scores(x, y, fid, coef)
    assert counts[2] == 0 and not sums[2].any()
    for f in (1, 2, 4):
        rows = empty[fid[empty] == f]
        assert len(rows) > 3
        assert all(pred[r].tobytes() == pred[rows[0]].tobytes() for r in rows)
        np.testing.assert_allclose(pred[rows[0]], 1.0 / (1.0 + np.exp(-coef[f - 1, :, 0])), rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------------------- end to end
LAMBDA = np.geomspace(0.05, 0.0005, 12)


def _e2e(grid):
    """the K + 1 fits of the sparse restatement on the sliced matrices (CV.cv's own fits() would take the dense restatement)"""
    def make():
        x, y, fid = _base()
        kw = dict(lambda_=[LAMBDA]) if grid == "given" else dict(nlambda=25)
        fit0 = RS.fit(x, y, penalty=["lasso"], **kw)
        folds = [RS.fit(x[fid != i], y[fid != i], penalty=["lasso"], **kw) for i in range(1, K + 1)]
        return dict(x=x, xd=x.toarray(), y=y, fid=fid, fitted=(fit0, folds))
    return _cached(("e2e", grid), make)


def _check_cv_oem(E, measure, grouped, **kw):
    """cv_oem(family="binomial") on the sparse x against the restatement, with tests/test_gpu_cv_logistic._check_cv_oem's preconditions
    and checks; kw: the fit's options"""
    import oem_amd
    ref = CV.cv(E["xd"], E["y"], E["fid"], penalty=["lasso"], type_measure=measure, grouped=grouped, fitted=E["fitted"])
    crit = np.sort(-ref["cvm"][0] if measure == "auc" else ref["cvm"][0])
    if measure == "class":
        crit = np.unique(crit)
    print("two best criteria", crit[:2], "relative gap", (crit[1] - crit[0]) / abs(crit[0]))
    assert (crit[1] - crit[0]) > 1e-5 * abs(crit[0]), crit[:3]
    pv = ref["fit.preval"][0]
    for i in range(1, K + 1):                                          # no tied held-out probabilities in any (fold, column)
        for j in range(pv.shape[1]):
            col = pv[E["fid"] == i, j]
            assert np.isnan(col).all() or len(np.unique(col)) == len(col), (i, j)
    got = oem_amd.cv_oem(E["x"], E["y"], family="binomial", penalty="lasso", type_measure=measure, grouped=grouped, foldid=E["fid"], keep=True,
                         **kw)
    assert got["name"] == ref["name"] and got["penalty"] == ["lasso"] and got["best.model"] == "lasso"
    assert isinstance(got["oem.fit"], oem_amd.OemFitBinomial) and got["oem.fit"]["nobs"] == N
    lam_g, lam_r = np.asarray(got["lambda"][0]), np.asarray(ref["lambda"][0])
    assert lam_g.shape == lam_r.shape                                                   # the same columns survive the NA trimming
    assert np.array_equal(lam_g, np.asarray(got["oem.fit"]["lambda"][0])[:len(lam_g)])    # exactly the full fit's own
    np.testing.assert_allclose(lam_g, lam_r, rtol=1e-12)
    assert np.array_equal(got["nzero"][0], ref["nzero"][0])
    d = {k: _rel(got[k][0], ref[k][0]) for k in ("cvm", "cvsd", "cvup", "cvlo", "fit.preval")}
    print("cv_oem sparse", measure, "grouped" if grouped else "rows", "differences / (1 + |value|):", d)
    assert max(d.values()) <= CV_TOL, d
    assert np.array_equal(got["foldid"], E["fid"])
    for key in ("lambda.min", "lambda.1se"):                                            # the same element of the sequence
        assert got[key] == lam_g[int(np.nonzero(lam_r == ref[key])[0][0])], key
    assert got["model.min"] == ref["model.min"]
    return ref, got


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("measure", ["deviance", "class", "mse", "mae", "auc"])
def test_cv_oem_sparse_end_to_end(measure, grouped):
    ref, _ = _check_cv_oem(_e2e("given"), measure, grouped, lambda_=LAMBDA)
    assert len(ref["lambda"][0]) == len(LAMBDA)                        # the restatement keeps all 12 lambdas


def test_cv_oem_sparse_default_grid_which_lam_and_trimming():
    """no lambda given: every fit has its own sequence, the full fit's smallest lambdas lie below a fold's smallest and are trimmed"""
    ref, got = _check_cv_oem(_e2e("default"), "deviance", True, nlambda=25)
    assert 2 <= len(ref["lambda"][0]) < 25 and not ref["which_lam"][0].all()
    assert len(got["cvm"][0]) == len(ref["lambda"][0])


# ------------------------------------------------------------------------------------------------------------- the Python surface
def test_sparse_x_owns_its_handle():
    import oem_amd
    from oem_amd import api
    x, y, fid = _base()
    yd, fd = _dev(y, fid)
    coef = _table(51, K, 3, P + 1)
    with oem_amd.SparseX(x) as sx:
        assert sx.shape == (N, P) and sx.nnz == x.nnz and not sx.closed and sx.handle
        a = api.logistic_cv_score(sx, yd, fd, K, coef)
    assert sx.closed
    with pytest.raises(ValueError, match="closed"):
        sx.handle
    with pytest.raises(ValueError, match="closed"):
        api.logistic_cv_score(sx, yd, fd, K, coef)
    with pytest.raises(ValueError, match="closed"):
        _fold_fit(sx, y, yd, fd, K, 1, ["lasso"], nlambda=4)
    sx.close()                                                         # closing twice is harmless
    sx2 = oem_amd.SparseX(x.tocsr(), device="cuda:0")                  # any format; without `with`
    b = api.logistic_cv_score(sx2, yd, fd, K, coef)
    sx2.close()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    with pytest.raises(TypeError):
        oem_amd.SparseX(x.toarray())


def test_cv_oem_takes_any_sparse_format_and_predict_cv_a_sparse_newx():
    import oem_amd
    x, y, fid = _base()
    kw = dict(family="binomial", penalty=["lasso", "mcp"], nlambda=8, foldid=fid, hessian_type="full")    # hessian_type: checked, ignored
    a = oem_amd.cv_oem(x, y, **kw)
    for other in (x.tocsr(), x.tocoo()):
        b = oem_amd.cv_oem(other, y, **kw)
        for m in range(2):
            assert np.asarray(a["cvm"][m]).tobytes() == np.asarray(b["cvm"][m]).tobytes()
            assert np.asarray(a["cvsd"][m]).tobytes() == np.asarray(b["cvsd"][m]).tobytes()
        assert a["lambda.min"] == b["lambda.min"] and a["model.min"] == b["model.min"]
    assert a["name"] == "Binomial Deviance" and "fit.preval" not in a
    prob = oem_amd.predict_cv(a, x[:50], type="response")
    dense = oem_amd.predict_cv(a, x[:50].toarray(), type="response")
    assert prob.shape == (50, 1) and np.all((prob > 0) & (prob < 1))
    np.testing.assert_allclose(np.asarray(prob), np.asarray(dense), rtol=1e-12)
    with pytest.raises(ValueError, match="'arg' should be one of"):
        oem_amd.cv_oem(x, y, family="binomial", hessian_type="newton", foldid=fid)
    with pytest.raises(oem_amd.OemgpuError, match="weights not implemented yet."):
        oem_amd.cv_oem(x, y, family="binomial", weights=np.ones(N), foldid=fid)


def test_cv_oem_gaussian_on_a_sparse_x_is_a_value_error():
    import oem_amd
    x, y, fid = _base()
    with pytest.raises(ValueError, match="served for family = \"binomial\" only"):
        oem_amd.cv_oem(x, y, foldid=fid)
    with pytest.raises(ValueError, match="served for family = \"binomial\" only"):
        oem_amd.cv_oem(x.tocsr(), y, family="gaussian", nfolds=5)
