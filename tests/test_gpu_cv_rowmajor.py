"""xval.oem and Gaussian cv.oem on row-major and float32 device tensors read in place (xval.hip: fold_gather_rm_kernel;
oemgpu_xval_dense_rm_dev, oemgpu_cv_fold_fits_rm_dev, oemgpu_selftest_fold_gather_rm_dev).

The fold-ordered copy is column-major float64 whichever way the rows came, so the new route has to build the BYTES the column-major
route builds, and everything after the copy is shared: the gather is held to numpy exactly, and every result to the column-major call
on `_colmajor(x.double())` byte for byte.

Every x sits inside a NaN-filled tensor, one element past an aligned address, with a row stride above p -- a kernel that reads or uses
what it must not shows NaN in its result instead of faulting.  Values are rounded through float16, so float32 holds them exactly (the
offset columns of the shifted case are rounded through float32 itself: 1e5 + v is beyond float16)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS, COLS = 64, 32                     # fold_gather_rm_kernel's tile (xval.hip: GRM_ROWS x GRM_COLS)


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


def _tdtype(name):
    import torch
    return {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16}[name]


def _nan_view(vals, pad, dt):
    """vals (n x p, float64, representable in dt) as a row-major view with row stride p + pad that starts one element into a NaN-filled
    tensor"""
    import torch
    n, p = vals.shape
    ldr = p + pad
    flat = torch.full((1 + n * ldr + 5,), float("nan"), dtype=_tdtype(dt), device="cuda")
    v = torch.as_strided(flat, (n, p), (ldr, 1), 1)
    v.copy_(torch.as_tensor(vals, device="cuda").to(_tdtype(dt)))
    assert flat.data_ptr() % 64 == 0 and v.data_ptr() == flat.data_ptr() + flat.element_size()
    assert v.stride() == (ldr, 1) and int(torch.isnan(flat).sum()) == flat.numel() - n * p
    assert np.array_equal(v.double().cpu().numpy(), vals)
    return v, flat


def _nan_vector(vals):
    import torch
    flat = torch.full((vals.shape[0] + 4,), float("nan"), dtype=torch.float64, device="cuda")
    v = flat[1:1 + vals.shape[0]]
    v.copy_(torch.as_tensor(vals, device="cuda"))
    return v, flat


def _colmajor(x64):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x64.T), device="cuda").t()


def _h(a):
    return np.asarray(a).astype(np.float16).astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1. the gather against numpy
def _foldid(n, kind, order):
    """K2: two folds; K7: seven ids of which 4 never occurs and 6 holds one row; K512: 512 folds.  sorted: long runs; robin: no runs"""
    if kind == "K2":
        K, fid = 2, np.arange(n) % 2 + 1
    elif kind == "K7":
        K, fid = 7, np.array([1, 2, 3, 5, 7])[np.arange(n) % 5]
        fid[n // 2] = 6
    else:
        K, fid = 512, np.arange(n) % 512 + 1
    if order == "sorted":
        fid = np.sort(fid)
    return K, fid.astype(np.int32)


def _gather_cases():
    """every n with every p; the dtype, the fold ids and their order rotate with periods 2, 3 (2 below 63 rows, where K7 has no room) and
    2 over the list, so that every value meets every other somewhere (pinned below)"""
    out, i = [], 0
    for n in (1, 63, 64, 65, 257, 3001):
        for p in (1, 2, 15, 16, 17, 31, 32, 33, 100):
            kinds = ["K2"] if n < 63 else (["K2", "K7", "K512"] if n == 3001 else ["K2", "K7"])
            out.append((n, p, 1 + 6 * ((i // 3) % 2), ("f64", "f32")[i % 2], kinds[(i // 2) % len(kinds)], ("sorted", "robin")[(i // 5) % 2]))
            i += 1
    return out


GATHER_CASES = _gather_cases()


def test_gather_cases_cover_every_value():
    c = GATHER_CASES
    assert {v[0] for v in c} == {1, ROWS - 1, ROWS, ROWS + 1, 257, 3001}
    assert {v[1] for v in c} == {1, 2, 15, 16, 17, COLS - 1, COLS, COLS + 1, 100}
    assert {v[2] for v in c} == {1, 7} and {v[3] for v in c} == {"f64", "f32"}
    assert {(v[4], v[5]) for v in c} == {(k, o) for k in ("K2", "K7", "K512") for o in ("sorted", "robin")}
    for edge in (ROWS - 1, ROWS, ROWS + 1):                                          # each edge of the tile in both element types
        assert {v[3] for v in c if v[0] == edge} == {"f64", "f32"}
    for edge in (COLS - 1, COLS, COLS + 1):
        assert {v[3] for v in c if v[1] == edge} == {"f64", "f32"}
    assert any(v[0] == 3001 and v[4] == "K512" for v in c)
    assert any(v[0] > ROWS and v[1] > COLS for v in c)                               # more than one tile both ways


def _check_gather(x, y, fid, K, got):
    """got = rowmajor_fold_order(...) against the layout built here: folds in order, a fold's rows in the caller's order, each segment on
    the next multiple of the layout's alignment (taken from the returned starts), NaN everywhere else"""
    xo, yo, fold_n, fold_start = got
    n, p = x.shape
    assert xo.shape[1] == p and xo.shape[0] == yo.shape[0] >= n
    assert fold_n.tolist() == np.bincount(fid, minlength=K + 1)[1:].tolist()
    align = functools.reduce(math.gcd, [int(s) for s in fold_start if s > 0], 0)
    assert fold_start[0] == 0
    for k in range(1, K):
        end = int(fold_start[k - 1] + fold_n[k - 1])
        assert fold_start[k] == (-(-end // align) * align if align else end), (k, fold_start[:k + 1], fold_n[:k + 1])
    assert fold_start[K - 1] + fold_n[K - 1] <= xo.shape[0]
    want_x = np.full(xo.shape, np.nan)
    want_y = np.full(yo.shape, np.nan)
    for k in range(K):
        rows = np.flatnonzero(fid == k + 1)
        want_x[fold_start[k]:fold_start[k] + len(rows)] = x[rows]
        want_y[fold_start[k]:fold_start[k] + len(rows)] = y[rows]
    written = ~np.isnan(want_y)
    assert int(written.sum()) == n
    assert np.array_equal(np.isnan(yo), ~written) and np.array_equal(np.isnan(xo), np.isnan(want_x))
    assert xo[written].tobytes() == want_x[written].tobytes() and yo[written].tobytes() == want_y[written].tobytes()


@pytest.mark.parametrize("n,p,pad,dt,kind,order", GATHER_CASES)
def test_gather_against_numpy(api, n, p, pad, dt, kind, order):
    rng = np.random.default_rng(n * 1000 + p)
    x, y = _h(rng.normal(size=(n, p)) * 3), rng.normal(size=n)
    K, fid = _foldid(n, kind, order)
    xv, xkeep = _nan_view(x, pad, dt)
    yv, ykeep = _nan_vector(y)
    before = xkeep.clone()
    got = api.rowmajor_fold_order(xv, yv, fid, K)
    _check_gather(x, y, fid, K, got)
    again = api.rowmajor_fold_order(xv, yv, fid, K)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))               # (NaN padding included)
    assert xkeep.cpu().numpy().tobytes() == before.cpu().numpy().tobytes()           # x is never written


def test_gather_with_element_offsets_past_2_to_the_31(api):
    """2049 rows 2^20 + 3 elements apart: the rows of the last tile start past element 2^31 of the tensor"""
    import torch
    n, p, ldr = 2049, 37, (1 << 20) + 3
    rng = np.random.default_rng(31)
    x, y = _h(rng.normal(size=(n, p)) * 3), rng.normal(size=n)
    flat = torch.empty(1 + n * ldr, dtype=torch.float32, device="cuda")
    xv = torch.as_strided(flat, (n, p), (ldr, 1), 1)
    xv.copy_(torch.as_tensor(x, device="cuda").float())
    assert (n - 1) * ldr > 2 ** 31 and api._xval_rowmajor_in_place(xv) == 1
    fid = (np.arange(n) % 3 + 1).astype(np.int32)
    _check_gather(x, y, fid, 3, api.rowmajor_fold_order(xv, torch.as_tensor(y, device="cuda"), fid, 3))


# ------------------------------------------------------------------------------------------------ 3. xval_oem
G23 = np.repeat(np.arange(1, 9), 3)[:23]
G130 = np.repeat(np.arange(1, 27), 5)
NF = 5


@functools.lru_cache(maxsize=None)
def _xval_data(n, p):
    rng = np.random.default_rng(n + p)
    x = _h(rng.normal(size=(n, p)) * (1.0 + rng.uniform(size=p)) + 0.3)
    b = np.zeros(p); b[rng.choice(p, 6, replace=False)] = rng.uniform(-1, 1, 6)
    y = x @ b + rng.normal(size=n) + 1.0
    fid = rng.permutation(np.resize(np.arange(1, NF + 1), n))
    w = rng.uniform(0.5, 2.0, size=n)
    return x, y, fid, w


def _same_xval(a, b):
    for k in range(len(b["beta"])):
        for key in ("beta", "lambda", "cvm", "cvsd"):
            assert np.asarray(a[key][k]).tobytes() == np.asarray(b[key][k]).tobytes(), (key, k)
        assert np.array_equal(a["niter"][k], b["niter"][k])
    assert a["d"] == b["d"] and a["lambda.min"] == b["lambda.min"] and a["best.model"] == b["best.model"]


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("measure", ["mse", "mae"])
@pytest.mark.parametrize("std,icpt", [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize("n,p", [(3001, 23), (900, 130)])
def test_xval_oem_is_the_column_major_xval_oem(oa, api, n, p, std, icpt, measure, weighted):
    x, y, fid, w = _xval_data(n, p)
    kw = dict(penalty=["lasso", "grp.lasso"], groups=G23 if p == 23 else G130, foldid=fid, type_measure=measure, standardize=std,
              intercept=icpt, nlambda=12, tol=1e-9, weights=w if weighted else ())
    ref = oa.xval_oem(_colmajor(x), y, **kw)
    assert np.all(np.isfinite(ref["cvm"][0])) and np.all(ref["cvsd"][0] > 0)
    for dt, pad in (("f64", 1), ("f32", 7)):
        xv, keep = _nan_view(x, pad, dt)
        assert api._xval_rowmajor_in_place(xv) is not None
        _same_xval(oa.xval_oem(xv, y, **kw), ref)


# ------------------------------------------------------------------------------------------------ 4. the fold fits
def _fits_data(offset):
    rng = np.random.default_rng(404)
    n, p = 3001, 23
    x = rng.normal(size=(n, p)) * 2 + 0.3
    y = x[:, :4] @ np.array([1.0, -1.5, 0.5, 2.0]) + rng.normal(size=n) + 0.4
    if offset:                                                                        # tests/test_gpu_cv_gaussian.py's offset columns
        x[:, [1, 7, 22]] += 1e5
        x = x.astype(np.float32).astype(np.float64)
    else:
        x = _h(x)
    return x, y, rng.permutation(np.resize(np.arange(1, NF + 1), n))


def _same_fits(got, ref):
    (ga, gd), (ra, rd) = got, ref
    assert gd["fold_n"].tolist() == rd["fold_n"].tolist() and len(ga) == len(ra) == NF
    for f, r in zip(ga, ra):
        assert f["d"] == r["d"] and f["nobs"] == r["nobs"]
        for k in range(len(r["beta"])):
            for key in ("beta", "lambda"):
                assert np.asarray(f[key][k]).tobytes() == np.asarray(r[key][k]).tobytes(), (key, k)
            assert np.array_equal(f["niter"][k], r["niter"][k])
            assert np.asarray(f["loss"][k]).tobytes() == np.asarray(r["loss"][k]).tobytes()


@pytest.mark.parametrize("offset", [False, True], ids=["about zero", "shifted"])
def test_fold_fits_are_the_column_major_fold_fits(oa, api, offset):
    x, y, fid = _fits_data(offset)
    pens = ["lasso", "mcp", "grp.lasso"]
    kw = dict(groups=G23, nlambda=15, tol=1e-10, maxit=2000, compute_loss=True)
    ref = api._cv_gaussian_fold_fits(_colmajor(x), y, fid, NF, pens, (), kw)
    assert oa.lib().oemgpu_last_shift_in_effect(ref[1]["ctx"]) == int(offset)
    for dt, pad in (("f64", 7), ("f32", 1)):
        xv, keep = _nan_view(x, pad, dt)
        got = api._cv_gaussian_fold_fits(xv, y, fid, NF, pens, (), kw)
        # the shift was advised and the fits were made again about launch_shift_sums_rm's sums
        assert oa.lib().oemgpu_last_shift_in_effect(got[1]["ctx"]) == int(offset)
        _same_fits(got, ref)


# ------------------------------------------------------------------------------------------------ 5. cv_oem end to end
USER_LAMBDA = [np.geomspace(1.5, 2e-3, 17), np.geomspace(2.0, 5e-3, 17)]


def _cv_kw(fid, user):
    return dict(penalty=["lasso", "grp.lasso"], groups=G23, foldid=fid, keep=True, tol=1e-10, maxit=2000,
                **({"lambda_": USER_LAMBDA} if user else {"nlambda": 21}))


@pytest.mark.parametrize("measure", ["mse", "mae"])
def test_cv_oem_with_a_lambda_list_is_the_column_major_call(oa, measure):
    x, y, fid = _fits_data(False)
    kw = _cv_kw(fid, True)
    ref = oa.cv_oem(_colmajor(x), y, type_measure=measure, **kw)
    for dt, pad in (("f64", 1), ("f32", 7)):
        xv, keep = _nan_view(x, pad, dt)
        f = oa.cv_oem(xv, y, type_measure=measure, **kw)
        for k in range(2):
            for key in ("cvm", "cvsd", "lambda", "fit.preval"):
                assert np.asarray(f[key][k]).tobytes() == np.asarray(ref[key][k]).tobytes(), (key, k)
        assert f["lambda.min"] == ref["lambda.min"] and f["best.model"] == ref["best.model"] and f["model.min"] == ref["model.min"]


def test_cv_oem_on_its_own_lambdas_agrees_with_the_column_major_call(oa):
    """the full fit's lambdas come from oem()'s row-major moment pass and differ from the column-major pass's in the last bits, as they
    did before: the bounds of tests/test_gpu_cv_gaussian.py against its restatement, cvm 1e-9 and cvsd 1e-8 relative"""
    x, y, fid = _fits_data(False)
    kw = _cv_kw(fid, False)
    ref = oa.cv_oem(_colmajor(x), y, **kw)
    for dt, pad in (("f64", 1), ("f32", 7)):
        xv, keep = _nan_view(x, pad, dt)
        f = oa.cv_oem(xv, y, **kw)
        for k in range(2):
            assert f["cvm"][k].shape == ref["cvm"][k].shape
            gm = float(np.max(np.abs(f["cvm"][k] - ref["cvm"][k]) / ref["cvm"][k]))
            gs = float(np.max(np.abs(f["cvsd"][k] - ref["cvsd"][k]) / ref["cvsd"][k]))
            print(f"GAP cv_oem row-major {dt} model {k}: cvm {gm:.1e} cvsd {gs:.1e}")
            assert gm <= 1e-9 and gs <= 1e-8, (k, gm, gs)
            assert int(np.argmin(f["cvm"][k])) == int(np.argmin(ref["cvm"][k]))
        assert f["best.model"] == ref["best.model"] and np.isclose(f["lambda.min"], ref["lambda.min"], rtol=1e-11)


# ------------------------------------------------------------------------------------------------ 6. nothing is copied
@functools.lru_cache(maxsize=None)
def _big(dt):
    import torch
    n, p = 200_000, 16
    g = torch.Generator(device="cuda"); g.manual_seed(6)
    x = torch.randn((n, p), generator=g, device="cuda", dtype=_tdtype(dt))
    y = x[:, :3].double().sum(dim=1) + torch.randn(n, generator=g, device="cuda", dtype=torch.float64)
    fid = np.random.default_rng(6).permutation(np.resize(np.arange(1, 11), n))
    assert x.stride() == (p, 1)
    return x, y, fid


def _calls(oa, x, y, fid):
    return [("cv_oem", lambda: oa.cv_oem(x, y, penalty="lasso", foldid=fid, nlambda=10)),
            ("xval_oem", lambda: oa.xval_oem(x, y, penalty="lasso", foldid=fid, nlambda=10))]


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_peak_memory_stays_below_a_float32_copy(oa, dt):
    import torch
    x, y, fid = _big(dt)
    n, p = x.shape
    before = x.clone()
    for name, call in _calls(oa, x, y, fid):
        call()                                                                        # (the context and its buffers exist from here on)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.max_memory_allocated()
        fit = call()
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - base
        print(f"GAP {name} row-major {dt}: peak allocated bytes grew by {grown} of {n * p * x.element_size()}")
        assert grown < n * p * 4
        assert np.all(np.isfinite(fit["cvm"][0]))
    assert torch.equal(x, before)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_no_copying_call_sees_an_n_by_p_tensor(oa, monkeypatch, dt):
    """torch.Tensor.contiguous and torch.Tensor.to raise on an n x p (or p x n) argument: neither front end asks for either"""
    import torch
    x, y, fid = _big(dt)
    shape = tuple(x.shape)
    real = {name: getattr(torch.Tensor, name) for name in ("contiguous", "to")}

    def guard(name):
        def f(self, *a, **k):
            if tuple(self.shape) in (shape, shape[::-1]):
                raise AssertionError(f"Tensor.{name} on the {self.shape[0]} x {self.shape[1]} matrix")
            return real[name](self, *a, **k)
        return f
    for name in real:
        monkeypatch.setattr(torch.Tensor, name, guard(name))
    for name, call in _calls(oa, x, y, fid):
        assert call() is not None


# ------------------------------------------------------------------------------------------------ 7. what still takes the copy
def test_what_still_takes_the_column_major_copy(oa, api):
    import torch
    rng = np.random.default_rng(7)
    n, p = 600, 24
    x = _h(rng.normal(size=(n, p)))
    y = x[:, :3].sum(axis=1) + rng.normal(size=n)
    fid = rng.permutation(np.resize(np.arange(1, NF + 1), n))
    xkw = dict(penalty="lasso", foldid=fid, nlambda=8, tol=1e-9)
    ckw = dict(penalty="lasso", foldid=fid, lambda_=np.geomspace(1.0, 1e-3, 9), tol=1e-9, keep=True)
    xc = _colmajor(x)
    xref, cref = oa.xval_oem(xc, y, **xkw), oa.cv_oem(xc, y, **ckw)

    def same(t):
        assert api._xval_rowmajor_in_place(t) is None
        _same_xval(oa.xval_oem(t, y, **xkw), xref)
        f = oa.cv_oem(t, y, **ckw)
        for key in ("cvm", "cvsd", "fit.preval"):
            assert np.asarray(f[key][0]).tobytes() == np.asarray(cref[key][0]).tobytes(), key
    h = torch.as_tensor(x, device="cuda").to(torch.float16)                            # a float16 tensor
    assert h.stride() == (p, 1) and torch.equal(h.double().cpu(), torch.as_tensor(x))
    same(h)
    cols = torch.as_tensor(np.repeat(x, 2, axis=1), device="cuda")[:, ::2]             # every second column of a row-major tensor
    assert cols.stride() == (2 * p, 2)
    same(cols)
    same(xc)                                                                           # a column-major tensor goes as it is ...
    big = _colmajor(np.random.default_rng(71).normal(size=(100_000, 16)))
    yb = np.random.default_rng(72).normal(size=100_000)
    fb = np.resize(np.arange(1, NF + 1), 100_000)
    for call in (lambda: oa.xval_oem(big, yb, penalty="lasso", foldid=fb, nlambda=5), lambda: oa.cv_oem(big, yb, penalty="lasso", foldid=fb, nlambda=5)):
        call()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.max_memory_allocated()
        call()
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated() - base < 100_000 * 16 * 4             # ... with no allocation of the matrix's size
    # and the row-major float64 / float32 tensors of the same data do go in place
    assert api._xval_rowmajor_in_place(torch.as_tensor(x, device="cuda")) == 0
    assert api._xval_rowmajor_in_place(torch.as_tensor(x, device="cuda").float()) == 1


# ------------------------------------------------------------------------------------------------ 8. refusals
def _score(oa, dev, n, p, K):
    """oemgpu_cv_score_dev on a table of zeros: 0 while the layout of the fold fits stands"""
    coef, ncol, tri = np.zeros((K, 1, 5, p + 1)), np.array([5], dtype=np.int32), np.zeros((K, 1, 5, 3))
    dp = C.POINTER(C.c_double)
    rc = oa.lib().oemgpu_cv_score_dev(dev["ctx"], n, p, K, coef.ctypes.data_as(dp), 1, 5, ncol.ctypes.data_as(C.POINTER(C.c_int32)), 0,
                                      tri.ctypes.data_as(dp), None)
    return rc, oa.lib().oemgpu_last_error().decode()


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_refusals_keep_their_messages(oa, api, dt):
    rng = np.random.default_rng(8)
    n, p, K = 100, 20, 3
    x, y = _h(rng.normal(size=(n, p))), rng.normal(size=n)
    xv, keep = _nan_view(x, 3, dt)
    xc = _colmajor(x)
    kw = dict(nlambda=5)
    served = np.concatenate([np.full(79, 1), np.full(11, 2), np.full(10, 3)])            # fold 1 leaves 21 rows for 20 columns: served
    got = api._cv_gaussian_fold_fits(xv, y, served, K, ["lasso"], (), kw)
    _same = api._cv_gaussian_fold_fits(xc, y, served, K, ["lasso"], (), kw)
    assert got[1]["fold_n"].tolist() == [79, 11, 10]
    assert all(np.asarray(a["beta"][0]).tobytes() == np.asarray(b["beta"][0]).tobytes() for a, b in zip(got[0], _same[0]))
    got = api._cv_gaussian_fold_fits(xv, y, served, K, ["lasso"], (), kw)
    assert _score(oa, got[1], n, p, K)[0] == 0
    for bad_id in (0, K + 1):
        fid = np.resize(np.arange(1, K + 1), n); fid[7] = bad_id
        calls = [lambda: api._cv_gaussian_fold_fits(xv, y, fid, K, ["lasso"], (), kw), lambda: api.rowmajor_fold_order(xv, y, fid, K)]
        if bad_id == 0:                                                                 # (xval_oem takes nfolds from the largest id)
            calls.append(lambda: oa.xval_oem(xv, y, penalty="lasso", foldid=fid, **kw))
        for call in calls:
            with pytest.raises(oa.OemgpuError, match="foldid must hold values in 1..nfolds") as e:
                call()
            assert e.value.code == -1
        rc, msg = _score(oa, got[1], n, p, K)                                          # the layout stamp is void afterwards
        assert rc == -1 and "call oemgpu_cv_fold_fits_dev" in msg
        got = api._cv_gaussian_fold_fits(xv, y, served, K, ["lasso"], (), kw)
        assert _score(oa, got[1], n, p, K)[0] == 0
    refused = np.concatenate([np.full(80, 1), np.full(10, 2), np.full(10, 3)])           # fold 1 leaves 20 rows for 20 columns
    with pytest.raises(oa.OemgpuError, match="fold 1 leaves 20 rows for 20 columns") as e:
        api._cv_gaussian_fold_fits(xv, y, refused, K, ["lasso"], (), kw)
    assert e.value.code == -4
    with pytest.raises(oa.OemgpuError, match="dimension of x larger than number of observations") as e:
        oa.xval_oem(xv, y, penalty="lasso", foldid=refused, **kw)
    assert e.value.code == -4
