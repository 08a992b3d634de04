"""predict() on a device tensor and on a resident SparseX (oemgpu_predict_dev / _rm_dev / _sparse_res, predict.hip) against numpy on the
host copy -- never against the code under test.

1. exact: dyadic x and coefficients, every partial sum exact, `link` array_equal to the numpy product for the four layouts over the
   grid of n, p, ncol and on each side of every limit the launch plan reports (asserted through oemgpu_selftest_predict_plan with the
   live CU count);
2. general data: |eta_gpu - eta| <= (p + 2) 2^-52 (|b0| + sum_j |x_ij| |b_j|) per element against a longdouble reference -- the bound of a
   (p + 1)-term FP64 sum in any order, doubled; the three dense layouts torch.equal;
3. strides, NaN padding, NaN rows, columns and rows more than 4 GiB apart: the bits of the compact call;
4. the three types;
5. end to end through oem / oem_fit_logistic_dense / cv_oem and predict / predict_cv."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAYOUTS = ["cm", "rm64", "rm32", "sparse"]
DENSE = LAYOUTS[:3]
U52 = 2.0 ** -52


def _ncu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(n, p, ncol, layout=-1):
    from oem_amd import _lib as L
    out = (C.c_int64 * 8)()
    L.check(L.lib().oemgpu_selftest_predict_plan(n, p, ncol, layout, _ncu(), out))
    return dict(zip(["rpw", "nwg", "lt", "passes", "chunk", "krows", "lds", "nchunks"], list(out)))


def _place(x, layout):
    """the host matrix x (float64; for rm32 its values must be float32 values) as the layout's newx"""
    import scipy.sparse as sp
    import torch
    import oem_amd
    if layout == "sparse":
        return oem_amd.SparseX(sp.csc_matrix(x))
    xd = torch.as_tensor(x, device="cuda")
    if layout == "cm":
        v = xd.t().contiguous().t()
        assert v.stride() == (1, x.shape[0]) or x.shape[0] == 1 or x.shape[1] == 1
        return v
    return xd.contiguous() if layout == "rm64" else xd.float().contiguous()


def _run(newx, b, kind="link"):
    """b: (p + 1, ncol), row 0 the intercepts -> the n x ncol device result"""
    from oem_amd import api
    return api._predict_device(newx, b, kind)


# ------------------------------------------------------------------------------------------ 1. exact
@functools.lru_cache(maxsize=None)
def _dyadic_x(n, p, sparse):
    rng = np.random.default_rng(1000 * n + p)
    x = rng.integers(-4, 5, size=(n, p)) / 2.0                                # {-2, -1.5, ..., 2}
    if sparse:
        x = x * (rng.random((n, p)) < 0.1)
        x[0, 0] = 1.5                                                         # (never an empty matrix)
    return x


@functools.lru_cache(maxsize=None)
def _dyadic_b(p, ncol):
    rng = np.random.default_rng(77 * p + ncol)
    return rng.integers(-32, 33, size=(p + 1, ncol)) / 16.0                   # multiples of 2^-4


def _exact_case(layout, n, p, ncol):
    x, b = _dyadic_x(n, p, layout == "sparse"), _dyadic_b(p, ncol)
    want = b[0] + x @ b[1:]
    newx = _place(x, layout)
    got = _run(newx, b)
    assert got.shape == (n, ncol) and got.stride() == (1, n) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want), (layout, n, p, ncol)
    if layout == "sparse":
        newx.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_exact_over_the_grid(layout):
    for n in (1, 15, 16, 17, 63, 64, 65, 4099):
        for p in (1, 3, 4, 5, 55, 56, 57, 113, 300):
            for ncol in (1, 15, 16, 17, 112, 113):
                _exact_case(layout, n, p, ncol)


def test_the_grid_crosses_the_plans_limits():
    """what the grid above is meant to reach, said by the plan: one pass and two, the table whole in LDS and in chunks (with one pass
    and with two), one workgroup and several"""
    a, b = _plan(4099, 57, 112), _plan(4099, 57, 113)
    assert (a["passes"], a["lt"], a["chunk"]) == (1, 7, 0) and (b["passes"], b["lt"], b["chunk"]) == (2, 4, 0)
    a, b = _plan(4099, 300, 112), _plan(4099, 300, 113)
    assert (a["passes"], a["chunk"], a["nchunks"]) == (1, 1, 3) and (b["passes"], b["chunk"], b["nchunks"]) == (2, 1, 3)
    assert _plan(4099, 300, 17)["chunk"] == 0
    P = _plan(4099, 300, 1)
    assert _plan(64, 300, 1)["nwg"] == 1 and P["nwg"] == -(-4099 // P["rpw"]) > 1


@pytest.mark.parametrize("layout", LAYOUTS)
def test_exact_on_each_side_of_the_plans_limits(layout):
    ncu = _ncu()
    # a last workgroup of 1 row | none
    assert _plan(129, 5, 1)["nwg"] == 2 and _plan(129, 5, 1)["rpw"] == 128 and _plan(128, 5, 1)["nwg"] == 1
    _exact_case(layout, 129, 5, 1)
    _exact_case(layout, 128, 5, 1)
    # the table of one column tile: whole in LDS up to K4 = 1120 coefficient rows, in chunks beyond
    assert _plan(17, 1119, 1)["chunk"] == 0 and _plan(17, 1120, 1)["chunk"] == 1 and _plan(17, 1120, 1)["nchunks"] == 11
    _exact_case(layout, 17, 1119, 1)
    _exact_case(layout, 17, 1120, 1)
    # of seven: up to K4 = 160
    assert _plan(65, 159, 112)["chunk"] == 0 and _plan(65, 160, 112)["chunk"] == 1 and _plan(65, 160, 112)["nchunks"] == 2
    _exact_case(layout, 65, 159, 112)
    _exact_case(layout, 65, 160, 112)
    # the wide fits: p = 20,000
    P = _plan(64, 20000, 17)
    assert P["chunk"] == 1 and P["nchunks"] == 179 and P["lt"] == 2
    _exact_case(layout, 64, 20000, 1)
    _exact_case(layout, 64, 20000, 17)
    # workgroups that take several rounds of 128 rows and a ragged last one: table in LDS (two workgroups per CU) and in chunks (one)
    n = 2 * 128 * ncu + 1
    P = _plan(n, 57, 17)
    assert P["chunk"] == 0 and P["rpw"] == 256 and P["nwg"] == -(-n // 256)
    _exact_case(layout, n, 57, 17)
    P = _plan(n, 300, 112)
    assert P["chunk"] == 1 and P["rpw"] == 384 and P["nwg"] == -(-n // 384)
    _exact_case(layout, n, 300, 112)
    _dyadic_x.cache_clear()


# ------------------------------------------------------------------------------------------ 2. general data
def _bound(x, b):
    """(p + 2) 2^-52 (|b0| + sum_j |x_ij| |b_j|), n x ncol"""
    p = x.shape[1]
    return (p + 2) * U52 * (np.abs(b[0]) + np.abs(x) @ np.abs(b[1:]))


def _eta_ref(x, b):
    xl, bl = x.astype(np.longdouble), b.astype(np.longdouble)
    return bl[0] + xl @ bl[1:]


@pytest.mark.parametrize("n,p,ncol", [(4099, 300, 17), (65, 113, 113), (1000, 57, 1), (300, 1200, 3)])
def test_general_data_is_within_the_bound_of_an_fp64_sum(n, p, ncol):
    import torch
    rng = np.random.default_rng(5 * n + p)
    x = rng.standard_normal((n, p)).astype(np.float32).astype(np.float64)      # float32 values: one matrix for the four layouts
    b = rng.standard_normal((p + 1, ncol))
    ref, bound = _eta_ref(x, b), _bound(x, b)
    outs = {}
    for layout in DENSE:
        outs[layout] = _run(_place(x, layout), b)
        err = np.abs(outs[layout].cpu().numpy().astype(np.longdouble) - ref)
        print(f"GENERAL {layout} {n}x{p}x{ncol}: worst error / bound {float(np.max(err / bound)):.3f}")
        assert np.all(err <= bound), layout
    assert torch.equal(outs["cm"], outs["rm64"]) and torch.equal(outs["cm"], outs["rm32"])
    # float64 values that are no float32 values: the float64 layouts
    x2 = rng.standard_normal((n, p))
    ref2, bound2 = _eta_ref(x2, b), _bound(x2, b)
    o_cm, o_rm = _run(_place(x2, "cm"), b), _run(_place(x2, "rm64"), b)
    assert torch.equal(o_cm, o_rm)
    assert np.all(np.abs(o_cm.cpu().numpy().astype(np.longdouble) - ref2) <= bound2)
    # the sparse source against the dense reference of the same matrix
    xs = x2 * (rng.random((n, p)) < 0.1)
    xs[0, 0] = 1.0
    with _place(xs, "sparse") as sx:
        err = np.abs(_run(sx, b).cpu().numpy().astype(np.longdouble) - _eta_ref(xs, b))
    print(f"GENERAL sparse {n}x{p}x{ncol}: worst error / bound {float(np.max(err / _bound(xs, b))):.3f}")
    assert np.all(err <= _bound(xs, b))


# ------------------------------------------------------------------------------------------ 3. strides and padding
def _strided(x, layout):
    """x inside a NaN parent: row stride p + 3 (row-major; float32 from an odd element offset), column stride n + 5 (column-major), and
    three more rows of NaN below the row-major matrices"""
    import torch
    n, p = x.shape
    nan = float("nan")
    if layout == "cm":
        parent = torch.full((p, n + 5), nan, dtype=torch.float64, device="cuda")
        parent[:, :n] = torch.as_tensor(x.T, device="cuda")
        v = parent[:, :n].t()
        assert v.stride() == (1, n + 5)
        return v
    dt = torch.float64 if layout == "rm64" else torch.float32
    flat = torch.full(((n + 3) * (p + 3) + 1,), nan, dtype=dt, device="cuda")
    v = flat.as_strided((n, p), (p + 3, 1), 1)
    v.copy_(torch.as_tensor(x, device="cuda"))
    assert v.stride() == (p + 3, 1) and v.storage_offset() == 1
    if layout == "rm32":
        assert v.data_ptr() % 8 == 4
    return v


@pytest.mark.parametrize("layout", DENSE)
@pytest.mark.parametrize("n,p,ncol", [(4099, 57, 17), (65, 300, 113), (17, 5, 1)])
def test_strides_and_nan_padding_leave_the_bits_alone(layout, n, p, ncol):
    import torch
    rng = np.random.default_rng(n + p)
    x = rng.standard_normal((n, p)).astype(np.float32).astype(np.float64)
    b = rng.standard_normal((p + 1, ncol))
    compact = _run(_place(x, layout), b)
    assert not torch.isnan(compact).any()
    assert torch.equal(_run(_strided(x, layout), b), compact)
    # a NaN at x[i, j] makes exactly row i of out NaN
    for i, j in [(0, 0), (n - 1, p - 1), (n // 2, p // 2)]:
        xn = x.copy()
        xn[i, j] = np.nan
        got = _run(_strided(xn, layout), b)
        bad = torch.isnan(got)
        assert bad[i].all() and int(bad.sum()) == ncol
        keep = torch.ones(n, dtype=torch.bool, device="cuda")
        keep[i] = False
        assert torch.equal(got[keep], compact[keep])


def test_a_nan_in_a_sparse_row_stays_in_its_row():
    rng = np.random.default_rng(8)
    n, p, ncol = 300, 40, 9
    x = rng.standard_normal((n, p)) * (rng.random((n, p)) < 0.2)
    x[7, 3] = np.nan
    b = rng.standard_normal((p + 1, ncol))
    with _place(x, "sparse") as sx:
        got = _run(sx, b).cpu().numpy()
    assert np.isnan(got[7]).all() and int(np.isnan(got).sum()) == ncol


def test_column_major_with_the_last_column_more_than_4_gib_from_the_first():
    """small n, a huge ld: a view of one flat buffer that is never filled (whatever it holds between the columns is never read)"""
    import torch
    n, p, ncol = 65, 5, 3
    ld = (1 << 29) // (p - 1) + 1
    assert (p - 1) * ld * 8 > 1 << 32
    rng = np.random.default_rng(4)
    x, b = rng.standard_normal((n, p)), rng.standard_normal((p + 1, ncol))
    flat = torch.empty((p - 1) * ld + n, dtype=torch.float64, device="cuda")
    v = flat.as_strided((n, p), (1, ld))
    v.copy_(torch.as_tensor(x, device="cuda"))
    got = _run(v, b)
    del v, flat
    torch.cuda.empty_cache()
    assert torch.equal(got, _run(_place(x, "cm"), b))
    assert np.all(np.abs(got.cpu().numpy().astype(np.longdouble) - _eta_ref(x, b)) <= _bound(x, b))


def test_row_major_with_the_last_row_more_than_4_gib_from_the_first():
    import torch
    n, p, ncol, ldr = 4099, 5, 3, 131073
    assert n * ldr * 8 > 1 << 32
    rng = np.random.default_rng(6)
    x, b = rng.standard_normal((n, p)), rng.standard_normal((p + 1, ncol))
    flat = torch.empty((n - 1) * ldr + p, dtype=torch.float64, device="cuda")
    v = flat.as_strided((n, p), (ldr, 1))
    v.copy_(torch.as_tensor(x, device="cuda"))
    got = _run(v, b)
    del v, flat
    torch.cuda.empty_cache()
    assert torch.equal(got, _run(_place(x, "rm64"), b))
    assert np.all(np.abs(got.cpu().numpy().astype(np.longdouble) - _eta_ref(x, b)) <= _bound(x, b))


# ------------------------------------------------------------------------------------------ 4. types
@pytest.mark.parametrize("layout", LAYOUTS)
def test_class_and_response(layout):
    """class = (link > 0) of the device's own link exactly and = (eta_ref > 0) on every row (no |eta_ref| lies within the bound of the sum,
    which is asserted, so nothing is left out); response = 1 / (1 + exp(-link)) of the device's link at rtol 2^-49: three roundings of at
    most 1 ulp on each side"""
    import torch
    n, p, ncol = 4099, 57, 17
    rng = np.random.default_rng(21)
    x = rng.standard_normal((n, p)).astype(np.float32).astype(np.float64)
    if layout == "sparse":
        x = x * (rng.random((n, p)) < 0.1)
    b = rng.standard_normal((p + 1, ncol))
    ref, bound = _eta_ref(x, b), _bound(x, b)
    assert np.all(np.abs(ref) > bound)
    newx = _place(x, layout)
    link, cls, resp = _run(newx, b), _run(newx, b, "class"), _run(newx, b, "response")
    assert cls.dtype == torch.int64 and cls.shape == (n, ncol) and resp.dtype == torch.float64
    assert torch.equal(cls, (link > 0).to(torch.int64))
    assert np.array_equal(cls.cpu().numpy(), (ref > 0).astype(np.int64))
    lh = link.cpu().numpy()
    want = 1.0 / (1.0 + np.exp(-lh))
    rel = np.abs(resp.cpu().numpy() - want) / want
    print(f"RESPONSE {layout}: worst relative error {float(rel.max()):.3e} = {float(rel.max()) / U52:.2f} x 2^-52")
    assert np.all(rel <= 2.0 ** -49)
    if layout == "sparse":
        newx.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_ends_of_the_logistic_and_eta_zero(layout):
    x = np.array([[800.0, 0.0], [-800.0, 0.0], [0.0, 0.0], [1.0, 2.0]])
    b = np.array([[0.0], [1.0], [0.0]])
    newx = _place(x, layout)
    assert np.array_equal(_run(newx, b).cpu().numpy(), x[:, :1])
    resp = _run(newx, b, "response").cpu().numpy()[:, 0]
    assert resp[0] == 1.0 and resp[1] == 0.0 and resp[2] == 0.5 and not np.isnan(resp).any()
    assert np.array_equal(_run(newx, b, "class").cpu().numpy()[:, 0], [1, 0, 0, 1])
    if layout == "sparse":
        newx.close()


# ------------------------------------------------------------------------------------------ 5. end to end
def _check_all(fit, predict, newx_dev, newx_host, xh, kinds, models):
    from oem_amd import api
    lam0 = np.asarray(fit["lambda"][0] if "oem.fit" not in fit else fit["oem.fit"]["lambda"][0])
    s_list = [float(lam0[1]), float(0.5 * (lam0[1] + lam0[2])), float(np.sqrt(lam0[-1] * lam0[-2])), float(lam0[0] * 2)]
    base = fit["oem.fit"] if "oem.fit" in fit else fit
    for kw in [dict(s=None), dict(s=s_list)] + [dict(s=s_list, which_model=m) for m in models]:
        if "oem.fit" in fit and kw["s"] is None:
            kw = dict(kw, s="lambda.min")
        for kind in kinds:
            got = predict(fit, newx_dev, type=kind, **kw)
            want = predict(fit, newx_host, type=kind, **kw)
            assert got.is_cuda and tuple(got.shape) == want.shape
            # the table the call used, for the bound: predict(type="coefficients") is host code the device path does not touch
            wm = kw.get("which_model", None)
            if "oem.fit" in fit:
                sv = fit[kw["s"]] if isinstance(kw["s"], str) else kw["s"]
                mod = fit["model.min"] - 1 if wm is None else fit["penalty"].index(wm)
                nbeta = api.predict(base, type="coefficients", s=sv, which_model=mod)
            else:
                nbeta = api.predict(base, type="coefficients", s=kw["s"], which_model=0 if wm is None else wm)
            nbeta = np.asarray(nbeta).reshape(nbeta.shape[0], -1)
            bound = _bound(xh, nbeta)
            g = got.cpu().numpy()
            if kind == "class" and base.get("family") == "binomial":
                link = predict(fit, newx_host, type="link", **kw)
                sure = np.abs(link) > bound
                assert sure.mean() > 0.99 and np.array_equal(g[sure], want[sure]) and g.dtype == np.int64
            elif kind == "response" and base.get("family") == "binomial":
                assert np.all(np.abs(g - want) <= bound / 4 + 2.0 ** -49 * want)
            else:
                assert g.dtype == np.float64 and np.all(np.abs(g - want) <= bound)
            assert np.array_equal(predict(fit, newx_dev, type=kind, **kw).cpu().numpy(), g)      # two calls: the same bits


def _data(n, p, seed, binomial=False):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, p)).astype(np.float32).astype(np.float64)
    beta = np.zeros(p)
    beta[:5] = [1.0, -0.7, 0.5, 0.3, -0.2]
    eta = 0.3 + x @ beta
    y = (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(np.float64) if binomial else eta + 0.5 * rng.standard_normal(n)
    return x, y


def test_oem_on_a_device_tensor_predicts_on_that_tensor(monkeypatch):
    import torch
    import oem_amd
    x, y = _data(2000, 30, 1)
    xd, yd = torch.as_tensor(x, device="cuda"), torch.as_tensor(y, device="cuda")
    fit = oem_amd.oem(xd, yd, penalty=["lasso", "mcp"], nlambda=8)
    cpu = torch.Tensor.cpu

    def guarded(self, *a, **k):
        assert tuple(self.shape) != tuple(xd.shape), "x was copied to the host"
        return cpu(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", guarded)
    _check_all(fit, oem_amd.predict, xd, x, x, ["link", "response", "class"], ["mcp"])
    monkeypatch.undo()
    assert oem_amd.predict(fit, xd).device == xd.device


def test_a_binomial_fit_on_a_float32_row_major_tensor_predicts_on_it(monkeypatch):
    import torch
    import oem_amd
    x, y = _data(3000, 20, 2, binomial=True)
    xd = torch.as_tensor(x, device="cuda").float()
    fit = oem_amd.oem_fit_logistic_dense(xd, torch.as_tensor(y, device="cuda"), penalty=["lasso", "mcp"], nlambda=8)
    assert fit["family"] == "binomial"
    cpu = torch.Tensor.cpu

    def guarded(self, *a, **k):
        assert tuple(self.shape) != tuple(xd.shape), "x was copied to the host"
        return cpu(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", guarded)
    _check_all(fit, oem_amd.predict, xd, x, x, ["link", "response", "class"], ["mcp"])
    monkeypatch.undo()
    cls = oem_amd.predict(fit, xd, type="class")
    assert cls.dtype == torch.int64 and set(np.unique(cls.cpu().numpy())) <= {0, 1}


def test_cv_oem_on_a_device_tensor_predicts_on_that_tensor():
    import torch
    import oem_amd
    x, y = _data(1500, 25, 3)
    xd, yd = torch.as_tensor(x, device="cuda"), torch.as_tensor(y, device="cuda")
    cv = oem_amd.cv_oem(xd, yd, penalty=["lasso", "mcp"], nlambda=8, nfolds=5, foldid=np.resize(np.arange(1, 6), 1500))
    _check_all(cv, oem_amd.predict_cv, xd, x, x, ["link"], ["mcp", "lasso"])
    one = oem_amd.predict_cv(cv, xd, s="lambda.1se")
    assert one.is_cuda and one.shape == (1500, 1)


def test_cv_oem_on_a_sparse_x_predicts_on_that_handle():
    import scipy.sparse as sp
    import oem_amd
    rng = np.random.default_rng(4)
    x, y = _data(1500, 25, 4)
    x = x * (rng.random(x.shape) < 0.3)
    y = 0.3 + x[:, :3] @ np.array([1.0, -0.7, 0.5]) + 0.5 * rng.standard_normal(1500)
    xs = sp.csc_matrix(x)
    with oem_amd.SparseX(xs) as sx:
        cv = oem_amd.cv_oem(sx, y, penalty=["lasso", "mcp"], nlambda=8, nfolds=5, foldid=np.resize(np.arange(1, 6), 1500))
        _check_all(cv, oem_amd.predict_cv, sx, xs, x, ["link"], ["mcp"])
        assert oem_amd.predict_cv(cv, sx).device == sx.device


def test_refusals():
    import scipy.sparse as sp
    import torch
    import oem_amd
    x, y = _data(500, 10, 5)
    xd = torch.as_tensor(x, device="cuda")
    fit = oem_amd.oem(xd, torch.as_tensor(y, device="cuda"), nlambda=5)
    with pytest.raises(ValueError, match="columns"):
        oem_amd.predict(fit, xd[:, :8])
    with pytest.raises(ValueError, match="columns"):
        oem_amd.predict(fit, torch.zeros((5, 12), device="cuda"))
    with pytest.raises(ValueError, match="2-d"):
        oem_amd.predict(fit, xd[0])
    with pytest.raises(ValueError, match="2-d"):
        oem_amd.predict(fit, xd.reshape(50, 10, 10))
    sx = oem_amd.SparseX(sp.csc_matrix(x))
    sx.close()
    with pytest.raises(ValueError, match="closed"):
        oem_amd.predict(fit, sx)
    with oem_amd.SparseX(sp.csc_matrix(x[:, :8])) as s8:
        with pytest.raises(ValueError, match="columns"):
            oem_amd.predict(fit, s8)


def test_other_tensors_go_through_the_copy_and_a_leading_column_of_ones_is_taken_as_it_is():
    import torch
    import oem_amd
    x, y = _data(700, 10, 6)
    xd = torch.as_tensor(x, device="cuda")
    fit = oem_amd.oem(xd, torch.as_tensor(y, device="cuda"), nlambda=5)
    want = oem_amd.predict(fit, xd)
    wide = torch.zeros((700, 20), dtype=torch.float64, device="cuda")
    wide[:, ::2] = xd
    assert torch.equal(oem_amd.predict(fit, wide[:, ::2]), want)                                  # strided in its columns: the copy
    assert torch.equal(oem_amd.predict(fit, xd.half()), oem_amd.predict(fit, xd.half().double()))  # another element type: the copy
    ones = torch.cat([torch.ones((700, 1), dtype=torch.float64, device="cuda"), xd], dim=1)
    got = oem_amd.predict(fit, ones).cpu().numpy()
    host = oem_amd.predict(fit, ones.cpu().numpy())
    nbeta = np.array(fit["beta"][0])
    assert np.all(np.abs(got - host) <= _bound(ones.cpu().numpy(), np.vstack([np.zeros((1, nbeta.shape[1])), nbeta])))


def test_no_n_by_p_temporary_at_20000_by_300_float32():
    import torch
    import oem_amd
    x, y = _data(20000, 300, 7)
    xd, yd = torch.as_tensor(x, device="cuda").float(), torch.as_tensor(y, device="cuda")
    fit = oem_amd.oem(xd, yd, nlambda=6)
    oem_amd.predict(fit, xd)                                                                      # (the context's workspace is made)
    torch.cuda.synchronize()
    for kw in (dict(s=None), dict(s=[float(fit["lambda"][0][2])])):
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = oem_amd.predict(fit, xd, **kw)
        peak = torch.cuda.max_memory_allocated() - before
        assert peak <= out.numel() * 8 + (1 << 20), (peak, out.numel() * 8)
        assert out.numel() * 8 + (1 << 20) < 20000 * 300 * 4
