"""Binomial fits, fold fits and scoring on row-major float64 / float32 device tensors read in place (logistic_rm.hip, the row-major
reader of logistic_cv.hip; oemgpu_fit_logistic_dense_rm_dev, oemgpu_fit_logistic_dense_fold_rm_dev, oemgpu_logistic_cv_score_rm_dev).

The yardstick is the existing column-major entry on x.double() laid out column-major -- itself held to tests/logistic_restatement.py
by test_gpu_logistic*.py -- and the comparison is `==` on the bytes: the row-major kernels take every sum in the column-major
kernels' order.  A float32 input is first rounded to float32, so both calls see the same values.

Every x is a view one element past an aligned address inside a NaN-filled flat tensor with row stride p + pad (the _nan_view pattern of
tests/test_gpu_rowmajor.py): a load outside the matrix poisons the result instead of faulting.

Band boundaries: the row pass stages a 64-row sub-block in column bands (oemgpu_selftest_logistic_rm_plan).  The cases take the p on
each side of the steps from one band to two and from two to three, read from the selftest (the second also gives three bands), and
p = 8191 with the narrowest bands and the largest LDS request."""
import ctypes as C

import numpy as np
import pytest

from tests import logistic_restatement as R

pytestmark = pytest.mark.gpu

LDS_BYTES = 160 << 10


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


@pytest.fixture(scope="module")
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _tdtype(name):
    import torch
    return {"f64": torch.float64, "f32": torch.float32}[name]


def _round(vals, dt):
    """the values both calls see: a float32 input is rounded to float32 first"""
    return vals.astype(np.float32).astype(np.float64) if dt == "f32" else np.asarray(vals, dtype=np.float64)


def _nan_view(vals, pad, dtype):
    """vals (n x p, float64, representable in dtype) as a row-major view with row stride p + pad that starts one element into a
    NaN-filled tensor"""
    import torch
    n, p = vals.shape
    ldr = p + pad
    flat = torch.full((1 + n * ldr + 5,), float("nan"), dtype=dtype, device="cuda")
    v = torch.as_strided(flat, (n, p), (ldr, 1), 1)
    v.copy_(torch.as_tensor(vals, device="cuda").to(dtype))
    assert flat.data_ptr() % 64 == 0 and v.data_ptr() == flat.data_ptr() + flat.element_size()
    assert v.stride() == (ldr, 1) and int(torch.isnan(flat).sum()) == flat.numel() - n * p
    assert np.array_equal(v.double().cpu().numpy(), vals)
    return v, flat


def _colmajor(vals):
    import torch
    x = torch.as_tensor(np.ascontiguousarray(vals.T), device="cuda").t()
    assert x.stride() == (1, vals.shape[0]) and x.dtype == torch.float64
    return x


def _bits(t):
    import torch
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32).clone()


def _data(n, p, seed, k=4, intercept=0.3):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, p)) * rng.uniform(0.5, 2.0, size=p) + rng.normal(size=p) * 0.2
    b = np.zeros(p)
    b[:min(k, p)] = rng.uniform(-1.0, 1.0, min(k, p))
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-(x @ b + intercept)))).astype(np.float64)
    return x, y


def _same_fit(a, b):
    assert len(a["beta"]) == len(b["beta"])
    for k in range(len(a["beta"])):
        assert np.asarray(a["beta"][k]).tobytes() == np.asarray(b["beta"][k]).tobytes(), (k, np.abs(np.asarray(a["beta"][k]) - np.asarray(b["beta"][k])).max())
        assert np.asarray(a["lambda"][k]).tobytes() == np.asarray(b["lambda"][k]).tobytes(), k
        assert np.asarray(a["loss"][k], dtype=np.float64).tobytes() == np.asarray(b["loss"][k], dtype=np.float64).tobytes(), k
        assert np.array_equal(np.asarray(a["niter"][k]), np.asarray(b["niter"][k])), k
    assert np.float64(a["d"]).tobytes() == np.float64(b["d"]).tobytes()
    assert a["nobs"] == b["nobs"]


def _ragged_groups(p):
    """groups of 1, 2, 3, ... columns"""
    sizes, g = [], 1
    while sum(sizes) < p:
        sizes.append(g)
        g += 1
    return np.repeat(np.arange(1, len(sizes) + 1), sizes)[:p]


# the option sets: standardize and intercept on and off, both Hessian types, lasso / mcp / grp.lasso with ragged groups, a zero in
# penalty_factor; compute_loss everywhere
OPTS = {
    "A": dict(penalty=["lasso"], standardize=True, intercept=True, hessian_type="upper.bound", pf0=False),
    "B": dict(penalty=["mcp", "grp.lasso"], standardize=False, intercept=False, hessian_type="full", pf0=True),
    "C": dict(penalty=["grp.lasso", "lasso"], standardize=True, intercept=False, hessian_type="upper.bound", pf0=True),
    "D": dict(penalty=["lasso", "mcp"], standardize=False, intercept=True, hessian_type="full", pf0=False),
    "E": dict(penalty=["lasso", "grp.lasso"], standardize=True, intercept=True, hessian_type="full", pf0=True),
}


def _kw(opt, p, **more):
    o = dict(OPTS[opt])
    pf = np.ones(p)
    if o.pop("pf0"):
        pf[p // 2] = 0.0
    kw = dict(o, penalty_factor=pf, compute_loss=True, nlambda=4, lambda_min_ratio=0.05)
    if any("grp" in q for q in o["penalty"]):
        kw["groups"] = _ragged_groups(p)
    kw.update(more)
    return kw


def _fit_both(oa, api, vals, y, pad, dt, kw, fold=None):
    """the fit on the row-major NaN-framed view and on the column-major float64 copy of the same values; the view must go in place and
    must come back untouched"""
    import torch
    vals = _round(vals, dt)
    xv, flat = _nan_view(vals, pad, _tdtype(dt))
    assert api._logistic_rowmajor_in_place(xv) == (1 if dt == "f32" else 0)
    before = _bits(flat)
    xc = _colmajor(vals)
    if fold is not None:
        fid, nfolds, leave_out = fold
        fd = torch.as_tensor(np.asarray(fid, dtype=np.int32), device="cuda")
        yd = torch.as_tensor(y, device="cuda")
        f = (fd, nfolds, leave_out, yd)
        got = oa.oem_fit_logistic_dense(xv, y, _fold=f, **kw)
        ref = oa.oem_fit_logistic_dense(xc, y, _fold=f, **kw)
    else:
        got = oa.oem_fit_logistic_dense(xv, y, **kw)
        ref = oa.oem_fit_logistic_dense(xc, y, **kw)
    assert torch.equal(_bits(flat), before)
    _same_fit(got, ref)
    assert all(np.all(np.isfinite(np.asarray(b))) for b in got["beta"])
    return got, ref


def _cm_plan(oa, n, p, intercept, num_cu):
    out = (C.c_int64 * 8)()
    assert oa.lib().oemgpu_selftest_logistic_plan(n, p, int(intercept), 0, num_cu, out) == 0
    return dict(zip(("ch", "nchunk", "rbz", "nzblk", "inner_wg", "staged"), list(out)[:6]))


def _rm_plan(oa, n, p, dt, intercept, num_cu):
    out = (C.c_int64 * 8)()
    assert oa.lib().oemgpu_selftest_logistic_rm_plan(n, p, 1 if dt == "f32" else 0, int(intercept), num_cu, out) == 0
    return dict(zip(("nband", "bw", "last", "lds", "ch", "nchunk", "rbz", "nzblk"), list(out)))


# ------------------------------------------------------------------------------------------------ A. the fit: rows, columns, options
# (n, p, pad, dtype, options).  n: one sub-block short, full, plus one row, two sub-blocks plus one (63, 64, 65, 129); p: each residue of
# the four eta partials (2, 3, 4, 5), the 64-column groups of the staging loop (63, 64, 65; 192, 193: the column-major kernel's own
# staging limit; 255, 256, 257: the workgroup's threads in phase 3); pad 0, 1, 7 over both dtypes
FIT_CASES = [
    (63, 2, 0, "f64", "A"), (63, 3, 1, "f32", "B"), (64, 4, 7, "f64", "C"), (64, 5, 0, "f32", "D"), (65, 2, 1, "f64", "E"),
    (65, 5, 7, "f32", "A"), (129, 3, 7, "f32", "E"), (129, 4, 1, "f64", "B"), (129, 63, 0, "f32", "C"), (129, 64, 1, "f64", "D"),
    (129, 65, 7, "f32", "A"), (700, 192, 0, "f64", "B"), (700, 193, 1, "f32", "D"), (700, 255, 7, "f64", "E"), (700, 256, 0, "f32", "B"),
    (700, 257, 1, "f64", "C"),
]


def test_fit_cases_cover_every_value():
    assert {c[0] for c in FIT_CASES} >= {63, 64, 65, 129}
    assert {c[1] for c in FIT_CASES} == {2, 3, 4, 5, 63, 64, 65, 192, 193, 255, 256, 257}
    assert {(c[2], c[3]) for c in FIT_CASES} == {(pad, dt) for pad in (0, 1, 7) for dt in ("f64", "f32")}
    assert {c[4] for c in FIT_CASES} == set(OPTS)


@pytest.mark.parametrize("n,p,pad,dt,opt", FIT_CASES)
def test_fit_is_the_column_major_fit(oa, api, n, p, pad, dt, opt):
    x, y = _data(n, p, 100 + n + p)
    _fit_both(oa, api, x, y, pad, dt, _kw(opt, p))


@pytest.mark.parametrize("p,pad,dt,opt", [(5, 1, "f32", "E"), (64, 7, "f64", "A")])
def test_fit_chunks_of_several_sub_blocks(oa, api, num_cu, p, pad, dt, opt):
    """70,001 rows: with 256 CUs the chunks leave 64 rows only above 65,536 rows"""
    n = 70001
    P = _cm_plan(oa, n, p, True, num_cu)
    assert P["ch"] > 64, P
    assert _rm_plan(oa, n, p, dt, True, num_cu)["ch"] == P["ch"]
    x, y = _data(n, p, 200 + p)
    _fit_both(oa, api, x, y, pad, dt, _kw(opt, p))


def test_two_z_blocks(oa, api, num_cu):
    """n q 8 > 256 MB: the Z blocks of the Hessian build are the column-major call's"""
    n, p = 70001, 480
    P, Rm = _cm_plan(oa, n, p, True, num_cu), _rm_plan(oa, n, p, "f32", True, num_cu)
    assert n * (p + 1) * 8 > 256 << 20 and P["nzblk"] >= 2 and (Rm["rbz"], Rm["nzblk"]) == (P["rbz"], P["nzblk"]), (P, Rm)
    assert Rm["nband"] == 2
    x, y = _data(n, p, 300)
    _fit_both(oa, api, x, y, 1, "f32", _kw("A", p, hessian_type="full", nlambda=3))


def _band_steps(oa):
    """(the last p with one band, the last p with two bands), read from the plan"""
    nb = [_rm_plan(oa, 10 ** 5, p, "f64", True, 256)["nband"] for p in range(1, 1200)]
    p12 = max(p for p, b in zip(range(1, 1200), nb) if b == 1)
    p23 = max(p for p, b in zip(range(1, 1200), nb) if b == 2)
    assert nb[p12] == 2 and nb[p23] == 3 and nb == sorted(nb)      # (nb[p] is the plan of p + 1)
    return p12, p23


@pytest.mark.parametrize("which,dt,pad,opt", [("one_band", "f64", 0, "E"), ("two_bands", "f32", 1, "B"), ("two_bands_last", "f64", 7, "D"),
                                              ("three_bands", "f32", 0, "E")])
def test_fit_at_the_band_steps(oa, api, num_cu, which, dt, pad, opt):
    p12, p23 = _band_steps(oa)
    p = {"one_band": p12, "two_bands": p12 + 1, "two_bands_last": p23, "three_bands": p23 + 1}[which]
    n = p + 150
    Rm = _rm_plan(oa, n, p, dt, True, num_cu)
    assert Rm["nband"] == {"one_band": 1, "two_bands": 2, "two_bands_last": 2, "three_bands": 3}[which], Rm
    assert Rm["lds"] <= LDS_BYTES and (Rm["nband"] - 1) * Rm["bw"] + Rm["last"] == p
    if which == "two_bands":
        assert Rm["last"] < 4                                    # a last band narrower than the four eta partials
    x, y = _data(n, p, 400 + p)
    _fit_both(oa, api, x, y, pad, dt, _kw(opt, p, nlambda=3))


def test_fit_at_the_largest_p(oa, api, num_cu):
    """p = 8191: the narrowest bands beside the most accumulators, the largest LDS request"""
    n, p = 8300, 8191
    Rm = _rm_plan(oa, n, p, "f32", True, num_cu)
    assert Rm["nband"] >= 40 and Rm["bw"] % 4 == 0 and LDS_BYTES - 8 * 65 * 4 < Rm["lds"] <= LDS_BYTES, Rm
    x, y = _data(n, p, 500)
    _fit_both(oa, api, x, y, 1, "f32", _kw("A", p, nlambda=2, irls_maxit=2, maxit=30))


def test_fit_with_element_offsets_past_2_to_the_31(oa, api):
    """129 rows 2^24 + 3 elements apart: the last row starts past element 2^31 of the tensor"""
    import torch
    n, p, ldr = 129, 5, (1 << 24) + 3
    vals = _round(_data(n, p, 600)[0], "f32")
    y = _data(n, p, 600)[1]
    flat = torch.empty(1 + n * ldr, dtype=torch.float32, device="cuda")
    xv = torch.as_strided(flat, (n, p), (ldr, 1), 1)
    xv.copy_(torch.as_tensor(vals, device="cuda").float())
    assert (n - 1) * ldr > 2 ** 31 and api._logistic_rowmajor_in_place(xv) == 1
    kw = _kw("E", p)
    _same_fit(oa.oem_fit_logistic_dense(xv, y, **kw), oa.oem_fit_logistic_dense(_colmajor(vals), y, **kw))


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("full", [False, True])
def test_w_floor_on_an_indexed_row(oa, api, dt, full):
    """the near-separable construction of tests/test_gpu_logistic_bounds.py: the floor is hit on the row with the IRLS index"""
    x, y = R.near_separable(6000, 20, 29)
    vals = _round(np.asarray(x), dt)
    kw = dict(penalty=["lasso", "mcp", "grp.lasso"], groups=np.arange(20) // 4 + 1, hessian_type="full" if full else "upper.bound", nlambda=8,
              lambda_min_ratio=1e-3, compute_loss=True)
    got, _ = _fit_both(oa, api, vals, y, 1, dt, kw)
    st = {}
    from oem_amd import api as A
    g, ug, _ = A._group_setup(kw["penalty"], kw["groups"], None, 20, True)
    ref = R.fit(vals, y, penalty=kw["penalty"], groups=g, unique_groups=ug, intercept=True, hessian_full=full, nlambda=8, lambda_min_ratio=1e-3,
                compute_loss=True, stats=st)
    assert st["floored"] > 0 and st["clamped"] > 0, st
    assert len(ref["beta"]) == len(got["beta"])


# ------------------------------------------------------------------------------------------------ B. fold fits
def _fold_case(name):
    """(n, p, foldid, nfolds, leave_out, separable)"""
    rng = np.random.default_rng(700)
    if name == "empty_sub_block":                    # rows 64 .. 127, a whole sub-block of the first chunk, are left out
        n, p = 300, 7
        fid = rng.integers(1, 4, size=n)
        fid[fid == 2] = 3
        fid[64:128] = 2
        return n, p, fid, 3, 2, False
    if name == "first_and_last_row":
        n, p = 257, 6
        fid = rng.integers(2, 5, size=n)
        fid[0] = fid[n - 1] = 1
        return n, p, fid, 4, 1, False
    if name == "first_irls_rows_left_out":           # rows 0 .. 4 are left out: IRLS index i is row 5 + i, among them the far rows 5 .. 9
        n, p = 3000, 20
        fid = rng.integers(2, 4, size=n)
        fid[:5] = 1
        return n, p, fid, 3, 1, True
    raise KeyError(name)


@pytest.mark.parametrize("dt,pad", [("f64", 1), ("f32", 7)])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("name", ["empty_sub_block", "first_and_last_row", "first_irls_rows_left_out"])
def test_fold_fit_is_the_column_major_fold_fit(oa, api, name, full, dt, pad):
    n, p, fid, nfolds, leave_out, separable = _fold_case(name)
    x, y = R.near_separable(n, p, 701) if separable else _data(n, p, 702)
    vals = _round(np.asarray(x), dt)
    kw = dict(penalty=["lasso", "grp.lasso"], groups=_ragged_groups(p), hessian_type="full" if full else "upper.bound", nlambda=6,
              lambda_min_ratio=1e-3 if separable else 0.05, compute_loss=True)
    got, _ = _fit_both(oa, api, vals, y, pad, dt, kw, fold=(fid, nfolds, leave_out))
    assert got["nobs"] == int((fid != leave_out).sum())
    # a left-out row is never loaded: NaN in those rows of the row-major tensor changes nothing
    import torch
    xv, _flat = _nan_view(vals, pad, _tdtype(dt))
    xv[torch.as_tensor(fid == leave_out, device="cuda")] = float("nan")
    fd = torch.as_tensor(fid.astype(np.int32), device="cuda")
    again = oa.oem_fit_logistic_dense(xv, y, _fold=(fd, nfolds, leave_out, torch.as_tensor(y, device="cuda")), **kw)
    _same_fit(again, got)
    if separable:                                    # the floor is hit on a mapped row
        st = {}
        keep = fid != leave_out
        from oem_amd import api as A
        g, ug, _ = A._group_setup(kw["penalty"], kw["groups"], None, p, True)
        R.fit(vals[keep], y[keep], penalty=kw["penalty"], groups=g, unique_groups=ug, intercept=True, hessian_full=full, nlambda=6,
              lambda_min_ratio=1e-3, compute_loss=True, stats=st)
        assert st["floored"] > 0, st


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_fold_fit_refusal_at_equality_and_fit_one_row_above(oa, api, dt):
    import torch
    n, p = 40, 9                                     # q = 10
    x, y = _data(n, p, 703, k=2)
    vals = _round(x, dt)
    xv, _flat = _nan_view(vals, 1, _tdtype(dt))
    yd = torch.as_tensor(y, device="cuda")
    kw = dict(penalty=["lasso"], nlambda=4, lambda_min_ratio=0.2, compute_loss=True)
    fid = np.resize([1, 2], n)
    fid[:30] = 3                                     # 10 rows stay: p + intercept = n_eff
    with pytest.raises(oa.OemgpuError) as ei:
        oa.oem_fit_logistic_dense(xv, y, _fold=(torch.as_tensor(fid.astype(np.int32), device="cuda"), 3, 3, yd), **kw)
    assert ei.value.code == -4 and "the 10 rows outside fold 3" in str(ei.value), str(ei.value)
    fid[29] = 1                                      # 11 rows stay
    _fit_both(oa, api, vals, y, 1, dt, kw, fold=(fid, 3, 3))


# ------------------------------------------------------------------------------------------------ C. scoring
def _score_plan(oa, n, p, ncol, num_cu):
    out = (C.c_int64 * 6)()
    assert oa.lib().oemgpu_selftest_cv_score_plan(n, p, ncol, num_cu, out) == 0
    return dict(zip(("ch", "nchunk", "tlds", "cb", "nlaunch", "lds"), list(out)))


def _score_both(oa, api, n, p, ncol, nfolds, fid, pad, dt, seed):
    import torch
    rng = np.random.default_rng(seed)
    vals = _round(rng.normal(size=(n, p)), dt)
    y = (rng.uniform(size=n) < 0.5).astype(np.float64)
    coef = rng.normal(size=(nfolds, ncol, p + 1)) * (0.7 / np.sqrt(p))
    xv, flat = _nan_view(vals, pad, _tdtype(dt))
    before = _bits(flat)
    yd = torch.as_tensor(y, device="cuda")
    fd = torch.as_tensor(np.asarray(fid, dtype=np.int32), device="cuda")
    assert api._logistic_rowmajor_in_place(xv) is not None
    s1, c1, p1 = api.logistic_cv_score(xv, yd, fd, nfolds, coef, y_hi=1.0, predmat=True)
    s0, c0, p0 = api.logistic_cv_score(_colmajor(vals), yd, fd, nfolds, coef, y_hi=1.0, predmat=True)
    assert torch.equal(_bits(flat), before)
    assert s1.tobytes() == s0.tobytes() and np.array_equal(c1, c0) and p1.tobytes() == p0.tobytes()
    assert c1.tolist() == [int((np.asarray(fid) == f).sum()) for f in range(1, nfolds + 1)]
    assert np.all(np.isfinite(s1)) and np.all(np.isfinite(p1[np.asarray(fid) >= 1]))


@pytest.mark.parametrize("n,ncol,p,pad,dt", [(64, 1, 5, 0, "f64"), (64, 9, 33, 1, "f32"), (65, 8, 64, 7, "f64"), (65, 33, 3, 0, "f32"),
                                               (70001, 9, 17, 7, "f32"), (70001, 33, 6, 1, "f64")])
def test_scoring_is_the_column_major_scoring(oa, api, num_cu, n, ncol, p, pad, dt):
    rng = np.random.default_rng(800 + n + ncol)
    if n == 70001:                                   # contiguous folds: whole chunks without a row of a fold
        fid = np.minimum(np.arange(n) // (n // 4 + 1) + 1, 4)
        P = _score_plan(oa, n, p, ncol, num_cu)
        assert P["nchunk"] >= 8 and P["tlds"] == 1, P
    else:
        fid = rng.permutation(np.resize(np.arange(1, 5), n))
    _score_both(oa, api, n, p, ncol, 4, fid, pad, dt, 801 + n + ncol)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_scoring_with_the_table_past_lds(oa, api, num_cu, dt):
    n, p, ncol = 300, 255, 81
    assert ncol * (p + 1) * 8 > LDS_BYTES and _score_plan(oa, n, p, ncol, num_cu)["tlds"] == 0
    fid = np.random.default_rng(810).permutation(np.resize(np.arange(1, 4), n))
    _score_both(oa, api, n, p, ncol, 3, fid, 1, dt, 811)


# ------------------------------------------------------------------------------------------------ D. cv.oem end to end
@pytest.fixture(scope="module")
def cv_data():
    x, y = _data(2000, 12, 900)
    fid = np.random.default_rng(901).permutation(np.resize(np.arange(1, 5), 2000))
    return x, y, fid


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("measure", ["deviance", "class", "auc"])
def test_cv_oem_binomial_end_to_end(oa, api, cv_data, measure, dt):
    x, y, fid = cv_data
    vals = _round(x, dt)
    xv, _flat = _nan_view(vals, 1, _tdtype(dt))
    kw = dict(family="binomial", penalty=["lasso", "mcp"], type_measure=measure, keep=True, foldid=fid, nlambda=8, lambda_min_ratio=0.01)
    got = oa.cv_oem(xv, y, **kw)
    ref = oa.cv_oem(_colmajor(vals), y, **kw)
    for m in range(2):
        for key in ("cvm", "cvsd", "fit.preval"):
            assert np.asarray(got[key][m]).tobytes() == np.asarray(ref[key][m]).tobytes(), (key, m)
        assert np.all(np.isfinite(np.asarray(got["cvm"][m])))
    assert np.asarray(got["lambda.min"]).tobytes() == np.asarray(ref["lambda.min"]).tobytes()
    assert np.asarray(got["lambda.1se"]).tobytes() == np.asarray(ref["lambda.1se"]).tobytes()


# ------------------------------------------------------------------------------------------------ E. nothing is copied
def _big(dt):
    import torch
    n, p = 200_000, 32
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    x = torch.randn((n, p), generator=g, device="cuda", dtype=_tdtype(dt))
    y = (torch.rand(n, generator=g, device="cuda", dtype=torch.float64) < torch.sigmoid(x[:, 0].double() - 0.5 * x[:, 1].double())).double()
    assert x.stride() == (p, 1)
    return x, y.cpu().numpy(), np.random.default_rng(6).permutation(np.resize(np.arange(1, 4), n))


def _calls(oa, x, y, fid):
    return [lambda: oa.oem_fit_logistic_dense(x, y, penalty="lasso", nlambda=5),
            lambda: oa.cv_oem(x, y, family="binomial", penalty="lasso", type_measure="deviance", foldid=fid, nlambda=5)]


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_nothing_is_copied(oa, dt):
    """across a fit and a cross-validation the peak of torch's allocations grows by less than n p 4 bytes: the smallest copy the
    column-major route makes is n p 8"""
    import torch
    x, y, fid = _big(dt)
    n, p = x.shape
    before = x.clone()
    for call in _calls(oa, x, y, fid):
        call()                                       # (the context and its workspace exist from here on)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.max_memory_allocated()
        call()
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - base
        print(f"GAP row-major binomial {dt}: peak allocated bytes grew by {grown}; n p 4 = {n * p * 4}")
        assert grown < n * p * 4
    assert torch.equal(x, before)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_no_copying_call_sees_an_n_by_p_tensor(oa, monkeypatch, dt):
    """torch.Tensor.contiguous and torch.Tensor.to raise on an n x p argument: the fit and the cross-validation never ask for either"""
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
    for call in _calls(oa, x, y, fid):
        fit = call()
        assert fit is not None


# ------------------------------------------------------------------------------------------------ F. what still takes the copy
def test_what_still_takes_the_column_major_copy(oa, api):
    import torch
    n, p = 600, 24
    x, y = _data(n, p, 950)
    vals = x.astype(np.float16).astype(np.float64)
    kw = _kw("E", p)
    xc = _colmajor(vals)
    ref = oa.oem_fit_logistic_dense(xc, y, **kw)
    # a float16 tensor
    h = torch.as_tensor(vals, device="cuda").to(torch.float16)
    assert h.stride() == (p, 1) and api._logistic_rowmajor_in_place(h) is None and torch.equal(h.double().cpu(), torch.as_tensor(vals))
    _same_fit(oa.oem_fit_logistic_dense(h, y, **kw), ref)
    # every second column of a row-major tensor
    cols = torch.as_tensor(np.repeat(vals, 2, axis=1), device="cuda")[:, ::2]
    assert cols.stride() == (2 * p, 2) and api._logistic_rowmajor_in_place(cols) is None
    _same_fit(oa.oem_fit_logistic_dense(cols, y, **kw), ref)
    # a column-major tensor goes as it is: no allocation of the matrix's size
    assert api._logistic_rowmajor_in_place(xc) is None
    big = _colmajor(np.random.default_rng(951).normal(size=(100_000, 16)))
    yb = (np.random.default_rng(952).uniform(size=100_000) < 0.5).astype(np.float64)
    oa.oem_fit_logistic_dense(big, yb, penalty="lasso", nlambda=3)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    oa.oem_fit_logistic_dense(big, yb, penalty="lasso", nlambda=3)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 100_000 * 16 * 8 / 4
    # ... and the row-major float64 / float32 tensors of the same data do go in place
    assert api._logistic_rowmajor_in_place(torch.as_tensor(vals, device="cuda")) == 0
    assert api._logistic_rowmajor_in_place(torch.as_tensor(vals, device="cuda").float()) == 1
    assert api._logistic_rowmajor_in_place(torch.as_tensor(np.repeat(vals, 2, axis=0), device="cuda")[::2]) == 0     # rows apart, columns together
