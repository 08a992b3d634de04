"""Row-major and float32 device tensors read in place (gram_rm.hip; oemgpu_shift_sums_rm_dev, oemgpu_moments_rm_dev,
oemgpu_fit_dense_rm_dev): the moment buffer against numpy long double, the sample sums against the column-major call bit for bit, the
shifted route and parity with the oracle and the column-major call, that nothing is copied, and what still goes the old way.

Every x of the moment and sample-sum tests is a view inside a larger NaN-filled tensor -- NaN in the row padding, in front of the first
row and behind the last, the base pointer one element past an aligned address -- so a kernel that reads or uses what it must not shows
NaN in its result instead of faulting."""
import ctypes as C
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc

LD = np.longdouble
U = LD(2.0) ** -53

# the tolerances of tests/test_gpu_configs.py for a device-resident oem() against orc.fit_dense(native=True)
DTOL = 1e-10
TIGHT = 1e-9


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
    return {"f64": torch.float64, "f32": torch.float32}[name]


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


def _nan_vector(vals):
    import torch
    flat = torch.full((vals.shape[0] + 4,), float("nan"), dtype=torch.float64, device="cuda")
    v = flat[1:1 + vals.shape[0]]
    v.copy_(torch.as_tensor(vals, device="cuda"))
    return v, flat


def _grid_data(n, p, seed, offset):
    """multiples of 2^-10 in [-4, 4] (13 bits: exact in float32); offset: column 0 and y moved by 128 -- mean^2 >= 124^2 > 2^8 * 16 >= 2^8 var
    whatever the sample: the shift predicate of include/oemgpu.h holds for every n"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-4096, 4097, size=(n, p)).astype(np.float64) / 1024.0
    y = rng.integers(-4096, 4097, size=n).astype(np.float64) / 1024.0
    if offset:
        x[:, 0] += 128.0
        y += 128.0
    return x, y


def _reference_moments(x, y, c=None):
    """(M, A): the moment buffer of Z = [x - c | y - c_y | 1] and the same of |Z|, in long double.  About 0 every product is a multiple of
    2^-20 no larger than 2^4 and every sum of n <= 2^20 of them has at most 45 bits: float64 arithmetic is then EXACT in any order, so the large
    cases take the float64 matrix product and say why they may."""
    n, p = x.shape
    z = np.concatenate([x, y[:, None], np.ones((n, 1))], axis=1)
    if c is None:
        assert np.abs(z).max() <= 4.0 and n <= 2 ** 20 and np.array_equal(z * 1024.0, np.round(z * 1024.0))
        if n * (p + 2) ** 2 > 5e7:
            return (z.T @ z).astype(LD), (np.abs(z).T @ np.abs(z)).astype(LD)
        z = z.astype(LD)
    else:
        z = z.astype(LD)
        z[:, :p + 1] -= np.asarray(c[:p + 1], dtype=np.float64).astype(LD)
    return z.T @ z, np.abs(z).T @ np.abs(z)


# (n, p, row padding, dtype): every n, every p, every padding, both dtypes; 4099 and 70001 rows take several row chunks, p >= 63
# several tile blocks, p + 2 = 17, 18, 33, 34, 35 the tile-column edges
MOMENT_CASES = [
    (1, 1, 0, "f64"), (1, 17, 1, "f32"), (3, 2, 7, "f64"), (3, 512, 0, "f32"), (63, 15, 1, "f32"), (63, 130, 7, "f64"),
    (64, 16, 0, "f32"), (64, 257, 1, "f64"), (65, 17, 7, "f32"), (65, 31, 0, "f64"), (257, 32, 1, "f32"), (257, 33, 7, "f64"),
    (257, 100, 0, "f32"), (4099, 1, 1, "f64"), (4099, 2, 0, "f32"), (4099, 130, 7, "f32"), (4099, 257, 0, "f64"), (4099, 512, 1, "f32"),
    (4099, 512, 7, "f64"), (70001, 15, 7, "f64"), (70001, 16, 1, "f32"), (70001, 31, 0, "f32"), (70001, 32, 7, "f64"),
    (70001, 33, 0, "f64"), (70001, 100, 1, "f64"), (70001, 100, 7, "f32"),
]


def test_moment_cases_cover_every_value():
    assert {c[0] for c in MOMENT_CASES} == {1, 3, 63, 64, 65, 257, 4099, 70001}
    assert {c[1] for c in MOMENT_CASES} == {1, 2, 15, 16, 17, 31, 32, 33, 100, 130, 257, 512}
    assert {c[2] for c in MOMENT_CASES} == {0, 1, 7} and {c[3] for c in MOMENT_CASES} == {"f64", "f32"}


@pytest.mark.parametrize("n,p,pad,dt", MOMENT_CASES)
def test_moments_about_zero(api, n, p, pad, dt):
    x, y = _grid_data(n, p, 1000 + n + p, offset=False)
    xv, xkeep = _nan_view(x, pad, _tdtype(dt))
    yv, ykeep = _nan_vector(y)
    before = xkeep.clone()
    got = api.rowmajor_moments(xv, yv)
    M, A = _reference_moments(x, y)
    assert got.shape == (p + 2, p + 2) and np.all(np.isfinite(got)), np.argwhere(~np.isfinite(got))[:5]
    err, bound = np.abs(got.astype(LD) - M), LD(n) * U * A
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))
    print(f"GAP row-major moments {n} x {p} + {pad} {dt}: worst error / bound {worst:.3f}")
    assert np.all(err <= bound), (worst, np.argwhere(err > bound)[:5])
    # sum x_j, sum y and n: exact to the bit
    assert np.array_equal(got[p + 1, :p], x.sum(axis=0)) and got[p + 1, p] == y.sum() and got[p + 1, p + 1] == n
    assert np.array_equal(got, got.T)                                     # both triangles are written
    assert api.rowmajor_moments(xv, yv).tobytes() == got.tobytes()        # two calls, the same bytes
    if dt == "f32":                                                       # a float32 x is its float64 copy
        assert api.rowmajor_moments(xv.double(), yv).tobytes() == got.tobytes()
    assert xkeep.cpu().numpy().tobytes() == before.cpu().numpy().tobytes()     # x is never written


def _sample_count(n):
    """rows of the sample pass: at most 256 evenly spaced 16-row chunks, the last of which may be ragged"""
    nch = (n + 15) // 16
    nsamp = min(nch, 256)
    chunks = {(k * (nch - 1)) // (nsamp - 1) if nsamp > 1 else 0 for k in range(nsamp)}
    assert len(chunks) == nsamp
    return sum(min(16, n - 16 * c) for c in chunks)


# (the long double products of the larger cases would take the test's seconds: they stay with the exact test above)
SHIFT_CASES = [c for c in MOMENT_CASES if c[0] * (c[1] + 2) ** 2 <= 5e7]


@pytest.mark.parametrize("n,p,pad,dt", SHIFT_CASES)
def test_moments_about_the_shift(api, n, p, pad, dt):
    """column 0 and y sit at 128 +- 4: the sums buffer asks for the shift, and the buffer is taken about c = sums[j] / sums[p + 1]"""
    x, y = _grid_data(n, p, 2000 + n + p, offset=True)
    xv, xkeep = _nan_view(x, pad, _tdtype(dt))
    yv, ykeep = _nan_vector(y)
    sums = api.rowmajor_shift_sums(xv, yv)
    assert np.all(np.isfinite(sums)) and sums[p + 1] == _sample_count(n)
    c = sums[:p + 1] / sums[p + 1]                                        # the kernel's own shift
    var = sums[p + 2] / sums[p + 1] - c[0] * c[0]
    assert c[0] * c[0] > 256.0 * max(var, 0.0) + 1000.0                   # the predicate holds, far from its edge
    got = api.rowmajor_moments(xv, yv, sums)
    M, A = _reference_moments(x, y, c)
    assert np.all(np.isfinite(got))
    err, bound = np.abs(got.astype(LD) - M), LD(n + 4) * U * A
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))
    print(f"GAP row-major shifted moments {n} x {p} + {pad} {dt}: worst error / bound {worst:.3f}")
    assert np.all(err <= bound), (worst, np.argwhere(err > bound)[:5])
    assert got[p + 1, p + 1] == n and np.array_equal(got, got.T)
    assert abs(got[0, 0]) < 0.01 * n * 128.0 ** 2                         # taken about the shift: nowhere near sum x_0^2
    assert api.rowmajor_moments(xv, yv, sums).tobytes() == got.tobytes()
    if dt == "f32":
        assert api.rowmajor_moments(xv.double(), yv, sums).tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------------ B. sample sums
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4096, 4097, 70001])
def test_shift_sums_equal_the_column_major_call(oa, api, n, dt):
    import torch
    p, pad = 37, 3
    rng = np.random.default_rng(n)
    x = (rng.normal(size=(n, p)) * 3.0 + rng.uniform(-50, 50, p)).astype(np.float32).astype(np.float64)
    y = rng.normal(size=n) + 7.0
    xv, xkeep = _nan_view(x, pad, _tdtype(dt))
    yv, ykeep = _nan_vector(y)
    got = api.rowmajor_shift_sums(xv, yv)
    xt = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda")       # (p, n) row-major: the column-major float64 copy
    yd = torch.as_tensor(y, device="cuda")
    ref = torch.full((2 * (p + 1) + 2,), float("nan"), dtype=torch.float64, device="cuda")
    ctx = api.context()
    torch.cuda.synchronize()
    assert oa.lib().oemgpu_shift_sums_dev(ctx, xt.data_ptr(), n, n, p, yd.data_ptr(), ref.data_ptr()) == 0
    assert oa.lib().oemgpu_synchronize(ctx) == 0
    ref = ref.cpu().numpy()
    assert np.all(np.isfinite(got)) and got.tobytes() == ref.tobytes()
    assert got[p + 1] == _sample_count(n)


# ------------------------------------------------------------------------------------------------ fits
def _cmp(fit, ref, tol=TIGHT):
    for k in range(len(ref["beta"])):
        a, b = np.asarray(fit["beta"][k]), np.asarray(ref["beta"][k])
        assert a.shape == b.shape
        err = np.abs(a - b).max()
        assert err <= tol, (fit["penalty"][k], err)
        assert np.allclose(fit["lambda"][k], ref["lambda"][k], rtol=1e-12, atol=0)
    assert abs(fit["d"] - ref["d"]) <= DTOL * abs(ref["d"])


def _colmajor(x64):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x64.T), device="cuda").t()


def _rowmajor(x64, dt, pad=0):
    import torch
    n, p = x64.shape
    buf = torch.zeros((n, p + pad), dtype=_tdtype(dt), device="cuda")
    v = buf[:, :p]
    v.copy_(torch.as_tensor(x64, device="cuda").to(_tdtype(dt)))
    assert v.stride() == (p + pad, 1)
    return v


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_shifted_route_end_to_end(oa, api, dt):
    """columns with mean 1e4 and sd 1: the first solve advises the shift, the sample pass and the shifted pass run on the rows"""
    rng = np.random.default_rng(77)
    n, p = 5000, 20
    x = (rng.normal(size=(n, p)) + 1e4).astype(np.float32).astype(np.float64)
    b = np.zeros(p); b[:5] = rng.uniform(-1, 1, 5)
    y = (x - 1e4) @ b + rng.normal(size=n)
    kw = dict(penalty=["lasso", "mcp"], nlambda=20, tol=1e-9)
    fit = oa.oem(_rowmajor(x, dt, pad=3), y, **kw)
    assert oa.lib().oemgpu_last_shift_in_effect(api.context()) == 1
    ref = orc.fit_dense(np.asfortranarray(x), y, native=True, **kw)
    _cmp(fit, ref)


G130 = np.repeat(np.arange(1, 27), 5)
G300 = np.repeat(np.arange(1, 51), 6)
# (p, penalty, standardize, intercept, compute_loss, groups)
PARITY = [
    (41, "lasso", True, True, False, None),
    (41, "mcp", False, False, False, None),
    (130, "grp.lasso", True, False, False, G130),
    (130, "lasso", False, True, False, None),
    (300, "mcp", True, True, True, None),
    (300, "grp.lasso", False, True, False, G300),
]


@pytest.mark.parametrize("p,pen,std,icpt,closs,groups", PARITY, ids=[f"p{c[0]}-{c[1]}-s{int(c[2])}i{int(c[3])}" for c in PARITY])
def test_parity_with_the_oracle_and_the_column_major_call(oa, p, pen, std, icpt, closs, groups):
    rng = np.random.default_rng(p + len(pen))
    n = 3000
    x = (rng.normal(size=(n, p)) * (1.0 + rng.uniform(size=p)) + 0.3).astype(np.float32).astype(np.float64)
    b = np.zeros(p); b[rng.choice(p, 10, replace=False)] = rng.uniform(-1, 1, 10)
    y = x @ b + rng.normal(size=n) + 1.0
    kw = dict(penalty=pen, nlambda=15, tol=1e-9, standardize=std, intercept=icpt, compute_loss=closs)
    okw = dict(kw)
    if groups is not None:
        kw["groups"] = groups
        okw.update(groups=groups, unique_groups=np.unique(groups))
    ref = orc.fit_dense(np.asfortranarray(x), y, native=True, **okw)
    col = oa.oem(_colmajor(x), y, **kw)
    _cmp(col, ref)
    for dt, pad in (("f64", 0), ("f32", 5)):
        fit = oa.oem(_rowmajor(x, dt, pad), y, **kw)
        _cmp(fit, ref)
        _cmp(fit, col)
        assert np.abs(np.ravel(fit["niter"][0]).astype(int) - np.ravel(col["niter"][0]).astype(int)).max() <= 1
        if closs:
            assert np.allclose(np.ravel(fit["loss"][0]), np.ravel(ref["loss"][0]), rtol=1e-9)
            assert np.allclose(np.ravel(fit["loss"][0]), np.ravel(col["loss"][0]), rtol=1e-9)


# ------------------------------------------------------------------------------------------------ E. nothing is copied
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_nothing_is_copied(oa, dt):
    import torch
    n, p = 200_000, 16
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    x = torch.randn((n, p), generator=g, device="cuda", dtype=_tdtype(dt))
    y = torch.randn(n, generator=g, device="cuda", dtype=torch.float64)
    assert x.stride() == (p, 1)
    before = x.clone()
    oa.oem(x, y, penalty="lasso", nlambda=5)                               # (the context and its workspace exist from here on)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    fit = oa.oem(x, y, penalty="lasso", nlambda=5)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"GAP row-major {dt}: peak allocated bytes grew by {grown} of {n * p * x.element_size()}")
    assert grown < n * p * x.element_size() / 4
    assert torch.equal(x, before)
    assert np.all(np.isfinite(fit["beta"][0]))


# ------------------------------------------------------------------------------------------------ F. what still goes the old way
def _same_bytes(a, b):
    for k in range(len(a["beta"])):
        assert np.asarray(a["beta"][k]).tobytes() == np.asarray(b["beta"][k]).tobytes()
        assert np.asarray(a["lambda"][k]).tobytes() == np.asarray(b["lambda"][k]).tobytes()
        assert np.array_equal(a["niter"][k], b["niter"][k])
    assert a["d"] == b["d"]


def test_what_still_takes_the_column_major_copy(oa, api):
    import torch
    rng = np.random.default_rng(9)
    kw = dict(penalty="lasso", nlambda=8, tol=1e-9)
    n, p = 600, 24
    x = rng.normal(size=(n, p)).astype(np.float16).astype(np.float64) + 0.0
    y = x[:, :3].sum(axis=1) + rng.normal(size=n)
    # a row-major tensor with p >= n
    xw = rng.normal(size=(30, 40)); yw = rng.normal(size=30)
    xr = torch.as_tensor(xw, device="cuda")
    assert xr.stride() == (40, 1) and api._rowmajor_in_place(xr) is None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _same_bytes(oa.oem(xr, yw, **kw), oa.oem(_colmajor(xw), yw, **kw))
    # strided in both dimensions: every second row of a column-major tensor, every second column of a row-major one
    big = _colmajor(np.repeat(x, 2, axis=0))
    half = big[::2]
    assert half.stride() == (2, 2 * n) and api._rowmajor_in_place(half) is None and torch.equal(half, torch.as_tensor(x, device="cuda"))
    ref = oa.oem(_colmajor(x), y, **kw)
    _same_bytes(oa.oem(half, y, **kw), ref)
    cols = torch.as_tensor(np.repeat(x, 2, axis=1), device="cuda")[:, ::2]
    assert cols.stride() == (2 * p, 2) and api._rowmajor_in_place(cols) is None
    _same_bytes(oa.oem(cols, y, **kw), ref)
    # a float16 tensor
    h = torch.as_tensor(x, device="cuda").to(torch.float16)
    assert h.stride() == (p, 1) and api._rowmajor_in_place(h) is None and torch.equal(h.double().cpu(), torch.as_tensor(x))
    _same_bytes(oa.oem(h, y, **kw), ref)
    # a column-major tensor
    assert api._rowmajor_in_place(_colmajor(x)) is None
    # ... and the row-major float64 / float32 tensors of the same data do go in place
    assert api._rowmajor_in_place(torch.as_tensor(x, device="cuda")) == 0
    assert api._rowmajor_in_place(torch.as_tensor(x, device="cuda").float()) == 1
    assert api._rowmajor_in_place(torch.as_tensor(np.repeat(x, 2, axis=0), device="cuda")[::2]) == 0      # rows apart, columns together


# ------------------------------------------------------------------------------------------------ G. the entry itself
def test_entry_refuses_the_shapes_of_the_column_major_entry(oa, api):
    import torch
    from oem_amd import _lib as L
    lib = oa.lib()
    ctx = api.context()
    for n, p, what in ((500, 2500, "p >= n"), (3000, L.RM_P_MAX + 1, "p <= 1024")):
        x = torch.zeros((n, p), dtype=torch.float32, device="cuda")
        y = torch.zeros(n, dtype=torch.float64, device="cuda")
        a = api._Args(["lasso"], [np.zeros(0)], 5, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(p), np.zeros(0, np.int32),
                      np.zeros(0, np.int32), np.zeros(0))
        rc = lib.oemgpu_fit_dense_rm_dev(ctx, x.data_ptr(), L.OEMGPU_F32, n, p, p, y.data_ptr(), 1, 1, C.byref(a.c), *a.outputs(p + 1))
        msg = lib.oemgpu_last_error().decode()
        assert rc == -4, (rc, msg)
        assert "column-major entry" in msg and "oemgpu_fit_dense_dev" in msg and what in msg
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert api._rowmajor_in_place(x) is None
