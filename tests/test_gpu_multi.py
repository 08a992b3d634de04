"""Many responses on one resident x (oem_multi; multi.hip; oemgpu_fit_dense_multi_dev / _rm_dev): the composed moment buffers against exact
sums and the single-response pass, every element of the result against oem() on its column and against the oracle, the edges of the solve
chunks, the options through the batched launch, the shift rule, one degenerate response, bytes, memory and the interrupt.

Every x and Y of the moment tests is a view inside a larger NaN-filled tensor (tests/test_gpu_rowmajor.py: _nan_view), so a kernel that
reads what it must not shows NaN in its result instead of faulting."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests.exact_gram import exact_gram
from tests.test_gpu_rowmajor import DTOL, TIGHT, _colmajor, _nan_view, _rowmajor

ERR_INTERRUPTED = -6


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


# ------------------------------------------------------------------------------------------------ A. exact moments
def _nan_colmajor(vals, pad):
    """vals (n x c, float64) as a column-major view with column stride n + pad that starts one element into a NaN-filled tensor"""
    import torch
    n, c = vals.shape
    ld = n + pad
    flat = torch.full((1 + c * ld + 5,), float("nan"), dtype=torch.float64, device="cuda")
    v = torch.as_strided(flat, (n, c), (1, ld), 1)
    v.copy_(torch.as_tensor(vals, device="cuda"))
    assert v.stride() == (1, ld) and int(torch.isnan(flat).sum()) == flat.numel() - n * c
    return v, flat


@pytest.mark.parametrize("p", [2, 15, 16, 17, 100])
def test_composed_moments_are_exact(oa, api, p):
    import torch
    lib, ctx = oa.lib(), api.context()
    for m in (1, 15, 16, 17, 33):
        n = 515
        plan = api.multi_plan(n, p, m, num_cu=_cus())
        assert n == 2 * plan["rows"] + 3 and plan["row_chunks"] == 3 and n % 4 != 0          # two chunks and three rows
        rng = np.random.default_rng(100 * p + m)
        kx, ky = rng.integers(-32, 33, size=(n, p)), rng.integers(-32, 33, size=(n, m))
        x, Y = kx / 8.0, ky / 8.0
        xs = {"cm": _nan_colmajor(x, 7), "rm64": _nan_view(x, 0, torch.float64), "rm32": _nan_view(x, 5, torch.float32)}
        Ys = {"cm": _nan_colmajor(Y, 3), "rm": _nan_view(Y, 2, torch.float64)}
        got = {(a, b): api.multi_moments(xs[a][0], Ys[b][0]) for a in xs for b in Ys}
        first = got[("cm", "cm")]
        assert first.shape == (m, p + 2, p + 2) and np.all(np.isfinite(first))
        for key, g in got.items():                                       # all forms of x and of Y: the same bytes
            assert g.tobytes() == first.tobytes(), key
        ones = 8 * np.ones((n, 1), dtype=np.int64)
        single = torch.full((p + 2, p + 2), float("nan"), dtype=torch.float64, device="cuda")
        xcm = xs["cm"][0]
        for r in range(m):
            exact = exact_gram(np.concatenate([kx, ky[:, r:r + 1], ones], axis=1)).astype(np.float64) / 64.0
            assert np.array_equal(first[r], exact), (m, r)
            yr = torch.as_tensor(np.ascontiguousarray(Y[:, r]), device="cuda")
            torch.cuda.synchronize()
            assert lib.oemgpu_moments_dev(ctx, xcm.data_ptr(), n, xcm.stride(1), p, yr.data_ptr(), None, single.data_ptr()) == 0
            assert lib.oemgpu_synchronize(ctx) == 0
            one = single.cpu().numpy().T
            assert np.tril(first[r]).tobytes() == np.tril(one).tobytes(), (m, r)


# ------------------------------------------------------------------------------------------------ fits against oem() and the oracle
def _hold(fit, ref, loss=False, niter=True, tol=TIGHT):
    """the bounds of tests/test_gpu_rowmajor.py for the same comparison"""
    for k in range(len(ref["beta"])):
        a, b = np.asarray(fit["beta"][k]), np.asarray(ref["beta"][k])
        assert a.shape == b.shape
        assert np.array_equal(np.isnan(a), np.isnan(b))
        err = np.nanmax(np.abs(a - b)) if np.any(~np.isnan(a)) else 0.0
        assert err <= tol, (fit["penalty"][k], err)
        assert np.allclose(fit["lambda"][k], ref["lambda"][k], rtol=1e-12, atol=0, equal_nan=True)
        if niter:
            assert np.abs(np.ravel(fit["niter"][k]).astype(int) - np.ravel(ref["niter"][k]).astype(int)).max() <= 1
        if loss:
            assert np.allclose(np.ravel(fit["loss"][k]), np.ravel(ref["loss"][k]), rtol=1e-9)
    assert abs(fit["d"] - ref["d"]) <= DTOL * abs(ref["d"])


def _same_bytes(a, b):
    for k in range(len(a["beta"])):
        assert np.asarray(a["beta"][k]).tobytes() == np.asarray(b["beta"][k]).tobytes()
        assert np.asarray(a["lambda"][k]).tobytes() == np.asarray(b["lambda"][k]).tobytes()
        assert np.array_equal(a["niter"][k], b["niter"][k])
    assert a["d"] == b["d"] and a["route"] == b["route"]


def _data(n, p, m, seed, nz=10):
    """x as tests/test_gpu_rowmajor.py's PARITY makes it (float32 values); one sparse coefficient vector and noise per response"""
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(n, p)) * (1.0 + rng.uniform(size=p)) + 0.3).astype(np.float32).astype(np.float64)
    B = np.zeros((p, m))
    for r in range(m):
        B[rng.choice(p, min(nz, p), replace=False), r] = rng.uniform(-1, 1, min(nz, p))
    Y = x @ B + rng.normal(size=(n, m)) + 1.0
    return x, Y


G130 = np.repeat(np.arange(1, 27), 5)
# (p, penalty, standardize, intercept, compute_loss, groups, n, m, route)
PARITY = [
    (41, "lasso", True, True, False, None, 3000, 5, 0),
    (41, "mcp", False, False, False, None, 3000, 5, 0),
    (130, "grp.lasso", True, False, False, G130, 3000, 5, 0),
    (250, "lasso", True, True, False, None, 3000, 5, 0),
    (300, "mcp", True, True, True, None, 3000, 5, 0),
    (1040, "lasso", True, True, False, None, 1200, 3, 1),
]
_PIDS = [f"p{c[0]}-{c[1]}" for c in PARITY]


def _parity_case(case):
    p, pen, std, icpt, closs, groups, n, m, route = case
    x, Y = _data(n, p, m, p + len(pen))
    kw = dict(penalty=pen, nlambda=15, tol=1e-9, standardize=std, intercept=icpt, compute_loss=closs)
    okw = dict(kw)
    if groups is not None:
        kw["groups"] = groups
        okw.update(groups=groups, unique_groups=np.unique(groups))
    return x, Y, kw, okw


@pytest.mark.parametrize("case", PARITY, ids=_PIDS)
def test_parity_with_oem_and_the_oracle(oa, case):
    import torch
    p, pen, std, icpt, closs, groups, n, m, route = case
    x, Y, kw, okw = _parity_case(case)
    xc = _colmajor(x)
    fits = oa.oem_multi(xc, torch.as_tensor(Y, device="cuda"), **kw)
    assert len(fits) == m and [f["route"] for f in fits] == [route] * m
    for r in range(m):
        one = oa.oem(xc, Y[:, r], **kw)
        ref = orc.fit_dense(np.asfortranarray(x), Y[:, r], native=True, **okw)
        _hold(fits[r], one, loss=closs)
        _hold(fits[r], ref, loss=closs, niter=False)
    # predict and logLik take an element as they take oem()'s result
    assert np.asarray(oa.predict(fits[0], x[:7])).shape[0] == 7
    if closs:
        assert np.all(np.isfinite(np.ravel(oa.logLik(fits[0]))))
    # a host Y, and a row-major float32 x read in place: the same fits to the bounds above
    if p <= 300:
        rm = oa.oem_multi(_rowmajor(x, "f32", 5), Y, **kw)
        for r in range(m):
            _hold(rm[r], fits[r], loss=closs)


@pytest.mark.parametrize("case", PARITY[:5], ids=_PIDS[:5])
def test_response_entries_have_the_same_bytes_from_every_layout_of_x(oa, api, case):
    """what this call adds to a moment buffer -- X'y, sum y^2, sum y of every response -- on the parity data (no exact sums there)"""
    import torch
    p, pen, std, icpt, closs, groups, n, m, route = case
    x, Y, kw, okw = _parity_case(case)
    Yd = torch.as_tensor(Y, device="cuda")
    col = api.multi_moments(_colmajor(x), Yd)
    for xr in (_rowmajor(x, "f32", 5), _rowmajor(x, "f64", 0)):
        row = api.multi_moments(xr, Yd.t().contiguous().t())
        assert col[:, p, :].tobytes() == row[:, p, :].tobytes() and col[:, :, p].tobytes() == row[:, :, p].tobytes()
        assert col[:, p + 1, p].tobytes() == row[:, p + 1, p].tobytes()


@pytest.mark.parametrize("case", PARITY, ids=_PIDS)
def test_same_bytes_x_rowmajor_float32_and_column_major(oa, case):
    """The fits from a row-major float32 x and from a column-major x are the same bytes: the response entries are (the test above), and
    the Gram block of either layout comes from one summation order -- gram_rm.hip's pass, which reads a column-major x too (p <= 1024;
    beyond, both take the column-major copy)."""
    import torch
    p, pen, std, icpt, closs, groups, n, m, route = case
    x, Y, kw, okw = _parity_case(case)
    Yd = torch.as_tensor(Y, device="cuda")
    col = oa.oem_multi(_colmajor(x), Yd, **kw)
    row = oa.oem_multi(_rowmajor(x, "f32", 5), Yd, **kw)
    worst = max(float(np.nanmax(np.abs(np.asarray(a["beta"][0]) - np.asarray(b["beta"][0])))) for a, b in zip(col, row))
    print(f"GAP multi p = {p} {pen}: row-major float32 against column-major x, largest coefficient difference {worst:.3e}")
    for a, b in zip(col, row):
        _same_bytes(a, b)


# ------------------------------------------------------------------------------------------------ C. chunk edges
@pytest.mark.parametrize("n,p,engine", [(200, 20, 1), (700, 300, 2)], ids=["p20-rows", "p300-coop"])
def test_chunk_edges(oa, api, n, p, engine):
    import torch
    plan = api.multi_plan(n, p, 2, num_cu=_cus())
    cap = plan["cap"]
    assert plan["engine"] == engine and cap >= 1
    m = cap + 1
    assert api.multi_plan(n, p, m, num_cu=_cus())["solve_chunks"] == 2
    x, Y = _data(n, p, m, 7 * p, nz=5)
    kw = dict(penalty="lasso", nlambda=10, tol=1e-9)
    xc = _colmajor(x)
    fits = oa.oem_multi(xc, torch.as_tensor(Y, device="cuda"), **kw)
    assert len(fits) == m and all(f["route"] == 0 for f in fits)
    for r in sorted({0, cap - 1, cap, m - 1}):
        _hold(fits[r], oa.oem(xc, Y[:, r], **kw))
    for f in fits:
        assert np.all(np.isfinite(f["beta"][0])) and np.all(np.isfinite(f["lambda"][0]))
        assert abs(f["d"] - fits[0]["d"]) <= DTOL * abs(fits[0]["d"])


# ------------------------------------------------------------------------------------------------ D. options through the batch
PF = np.ones(41)
PF[[0, 3, 17]] = 0.0
OPTIONS = {
    "three-penalties": dict(penalty=["lasso", "mcp", "scad"]),
    "user-lambda": dict(penalty="lasso", lambda_=np.geomspace(1.0, 0.005, 8)),
    "ols": dict(penalty="ols"),
    "penalty-factor": dict(penalty="lasso", penalty_factor=PF),
    "accelerate": dict(penalty="lasso", accelerate=True),
    "s0i0": dict(penalty="lasso", standardize=False, intercept=False),
    "s0i1": dict(penalty="lasso", standardize=False, intercept=True),
    "s1i0": dict(penalty="lasso", standardize=True, intercept=False),
    "s1i1": dict(penalty="lasso", standardize=True, intercept=True),
}


@pytest.fixture(scope="module")
def option_data():
    x, Y = _data(3000, 41, 7, 4141)
    return x, Y, _colmajor(x)


@pytest.mark.parametrize("name", list(OPTIONS))
def test_options_through_the_batch(oa, option_data, name):
    x, Y, xc = option_data
    kw = dict(nlambda=12, tol=1e-9, **OPTIONS[name])
    fits = oa.oem_multi(xc, Y, **kw)
    assert len(fits) == 7 and all(f["route"] == 0 for f in fits)
    for r in range(7):
        one = oa.oem(xc, Y[:, r], **kw)
        _hold(fits[r], one)
        if name == "user-lambda":
            assert np.array_equal(fits[r]["lambda"][0], fits[0]["lambda"][0])


# ------------------------------------------------------------------------------------------------ E. shift
def test_x_that_advises_a_shift_refits_every_response(oa, api):
    rng = np.random.default_rng(77)
    n, p, m = 5000, 20, 4
    x = (rng.normal(size=(n, p)) + 1e4).astype(np.float32).astype(np.float64)
    B = np.zeros((p, m)); B[:5] = rng.uniform(-1, 1, (5, m))
    Y = (x - 1e4) @ B + rng.normal(size=(n, m))
    kw = dict(penalty=["lasso", "mcp"], nlambda=20, tol=1e-9)
    xc = _colmajor(x)
    fits = oa.oem_multi(xc, Y, **kw)
    assert [f["route"] for f in fits] == [2] * m
    for r in range(m):
        _hold(fits[r], oa.oem(xc, Y[:, r], **kw))
        _hold(fits[r], orc.fit_dense(np.asfortranarray(x), Y[:, r], native=True, **kw), niter=False)


def test_one_response_that_advises_a_shift(oa, api):
    rng = np.random.default_rng(78)
    n, p, m = 5000, 20, 4
    x = rng.normal(size=(n, p)).astype(np.float32).astype(np.float64)
    x -= x.mean(axis=0)
    B = np.zeros((p, m)); B[:5] = rng.uniform(-1, 1, (5, m))
    Y = x @ B + rng.normal(size=(n, m))
    Y[:, 2] += 1e6
    kw = dict(penalty="lasso", nlambda=20, tol=1e-9)
    xc = _colmajor(x)
    one = oa.oem(xc, Y[:, 2], **kw)
    ctx = api.context()
    looks_at_y = oa.lib().oemgpu_last_shift_in_effect(ctx) == 1 or oa.lib().oemgpu_last_shift_advised(ctx) == 1
    fits = oa.oem_multi(xc, Y, **kw)
    _hold(fits[2], one)
    assert [fits[r]["route"] for r in (0, 1, 3)] == [0, 0, 0]
    assert fits[2]["route"] == (2 if looks_at_y else 0)
    for r in (0, 1, 3):
        _hold(fits[r], oa.oem(xc, Y[:, r], **kw))


# ------------------------------------------------------------------------------------------------ F. one degenerate instance
def test_a_constant_response_among_ordinary_ones(oa):
    x, Y = _data(3000, 41, 5, 99)
    Y[:, 3] = 2.0                                                     # (sums of 2 and 4 are exact in any order: centred to exactly zero)
    kw = dict(penalty="lasso", nlambda=10, tol=1e-9, standardize=True, intercept=True)
    xc = _colmajor(x)
    fits = oa.oem_multi(xc, Y, **kw)
    for r in range(5):
        one = oa.oem(xc, Y[:, r], **kw)
        if r == 3:
            a, b = np.asarray(fits[r]["beta"][0]), np.asarray(one["beta"][0])
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))
            assert np.array_equal(np.isnan(fits[r]["lambda"][0]), np.isnan(one["lambda"][0]))
            ok = np.isfinite(a)
            assert np.allclose(a[ok], b[ok], rtol=0, atol=TIGHT)
        else:
            _hold(fits[r], one)
            assert np.all(np.isfinite(fits[r]["beta"][0]))


# ------------------------------------------------------------------------------------------------ G. bytes and memory
def test_two_calls_return_the_same_bytes(oa):
    x, Y = _data(3000, 41, 9, 5)
    kw = dict(penalty=["lasso", "scad"], nlambda=10, tol=1e-9)
    xr = _rowmajor(x, "f32", 3)
    a, b = oa.oem_multi(xr, Y, **kw), oa.oem_multi(xr, Y, **kw)
    for fa, fb in zip(a, b):
        _same_bytes(fa, fb)


def test_nothing_is_copied(oa):
    import torch
    n, p, m = 200_000, 16, 8
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    x = torch.randn((n, p), generator=g, device="cuda", dtype=torch.float32)
    Y = torch.randn((n, m), generator=g, device="cuda", dtype=torch.float64)
    assert x.stride() == (p, 1) and Y.stride() == (m, 1)
    before, ybefore = x.clone(), Y.clone()
    oa.oem_multi(x, Y, penalty="lasso", nlambda=5)                   # (the context and its buffers exist from here on)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    fits = oa.oem_multi(x, Y, penalty="lasso", nlambda=5)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"GAP multi row-major f32: peak allocated bytes grew by {grown} of {n * p * x.element_size()}")
    assert grown < n * p * x.element_size()
    assert torch.equal(x, before) and torch.equal(Y, ybefore)
    assert all(np.all(np.isfinite(f["beta"][0])) for f in fits)


# ------------------------------------------------------------------------------------------------ H. interrupt
def test_interrupt_between_chunks(oa, api):
    n, p = 200, 20
    cap = api.multi_plan(n, p, 2, num_cu=_cus())["cap"]
    x, Y = _data(n, p, cap + 1, 11, nz=5)
    xc = _colmajor(x)
    calls = []

    def fire():
        calls.append(1)
        return True

    with pytest.raises(oa.OemgpuError) as e:
        oa.oem_multi(xc, Y, penalty="lasso", nlambda=5, interrupt=fire)
    assert e.value.code == ERR_INTERRUPTED and len(calls) == 1          # polled once: behind the first chunk
    fits = oa.oem_multi(xc, Y[:, :3], penalty="lasso", nlambda=5)      # the same context serves the next call
    for r in range(3):
        _hold(fits[r], oa.oem(xc, Y[:, r], penalty="lasso", nlambda=5))
