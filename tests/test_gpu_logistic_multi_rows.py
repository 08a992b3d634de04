"""The shared row pass of the many-response binomial fit (logistic_multi.hip) alone, through oemgpu_selftest_logistic_multi_rows_dev:
against numpy at the edges of its tiling with a derived tolerance, exact sums in mode 0, the live mask, and the bytes of a
response's sums whatever it is computed among.  The paddings of x and Y are NaN: any read of them shows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def api():
    import oem_amd
    oem_amd.lib()
    from oem_amd import api
    return api


@pytest.fixture(scope="module")
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _x(xh, layout):
    """xh on the device: 'cm' column-major float64 with ld = n + 3, 'rm' row-major float64 with ldr = p + 5, 'f32' row-major float32
    with ldr = p + 3; every padding element is NaN"""
    import torch
    n, p = xh.shape
    if layout == "cm":
        buf = torch.full((p, n + 3), float("nan"), dtype=torch.float64, device="cuda")
        x = buf.t()[:n]
    else:
        dt, pad = (torch.float64, 5) if layout == "rm" else (torch.float32, 3)
        buf = torch.full((n, p + pad), float("nan"), dtype=dt, device="cuda")
        x = buf[:, :p]
    x.copy_(torch.as_tensor(xh))
    return x


def _y(Yh, layout):
    """Yh on the device, float64: 'rm' row stride m + 2, 'cm' column stride n + 7; NaN padding"""
    import torch
    n, m = Yh.shape
    if layout == "rm":
        Y = torch.full((n, m + 2), float("nan"), dtype=torch.float64, device="cuda")[:, :m]
    else:
        Y = torch.full((m, n + 7), float("nan"), dtype=torch.float64, device="cuda").t()[:n]
    Y.copy_(torch.as_tensor(Yh))
    return Y


def _case(n, p, m, seed, intercept=True, f32=False):
    """x, 0/1 Y and Bt with |eta| well below 10 (the loss clamps are not straddled)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, p))
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    Y = (rng.uniform(size=(n, m)) < 0.4).astype(np.float64)
    q = p + (1 if intercept else 0)
    bt = rng.uniform(-1.0, 1.0, size=(m, q)) * (1.5 / np.sqrt(p))
    if intercept:
        bt[:, 0] = rng.uniform(-1.0, 1.0, size=m)
    return x, Y, bt


def _ref(x, Y, bt, intercept, mode):
    """g and its tolerance.  Entry j of response r: |g - g_ref| <= 4 [n u sum_i |x_ij r_i| + sum_i |x_ij| s (p + 1) u sum_k |x_ik bt_k|],
    u = 2^-53: any summation order of X'r, plus eta's rounding carried through the link, whose slope s is at most 1/4 (sum r and X'r:
    x_ij = 1 for sum r) and at most 1 for the loss (d/d eta of log(1 / prob) is prob - 1); 4 covers the ulps of exp, log and the
    division.  The reference itself is summed in extended precision."""
    n, p = x.shape
    m = Y.shape[1]
    o = 1 if intercept else 0
    xl, ax = x.astype(np.longdouble), np.abs(x)
    g, tol = np.zeros((m, p + 2)), np.zeros((m, p + 2))
    for r in range(m):
        y = Y[:, r]
        if mode:
            b = bt[r]
            eta = xl @ b[o:].astype(np.longdouble) + (b[0] if intercept else 0.0)
            aeta = ax @ np.abs(b[o:]) + (abs(b[0]) if intercept else 0.0)
            assert float(np.abs(eta).max()) < 10.0
            prob = 1.0 / (1.0 + np.exp(-eta))
            res = y - prob
            loss = np.where(y == 1.0, np.log(1.0 / prob), np.log(1.0 / (1.0 - prob)))
        else:
            res, aeta, loss = y.astype(np.longdouble), np.zeros(n), np.zeros(n, dtype=np.longdouble)
        e_eta = (p + 1) * U * aeta
        ares = np.abs(res).astype(np.float64)
        g[r, 0], g[r, 1:p + 1], g[r, p + 1] = float(res.sum()), (xl.T @ res).astype(np.float64), float(loss.sum())
        tol[r, 0] = 4.0 * (n * U * ares.sum() + 0.25 * e_eta.sum())
        tol[r, 1:p + 1] = 4.0 * (n * U * (ax.T @ ares) + ax.T @ (0.25 * e_eta))
        tol[r, p + 1] = 4.0 * (n * U * float(np.abs(loss).sum()) + e_eta.sum())
    return g, tol


def _check(api, x, Y, bt, intercept, mode, xl="cm", yl="rm"):
    got = api.logistic_multi_rows(_x(x, xl), _y(Y, yl), bt if mode else None, intercept=intercept, mode=mode)
    ref, tol = _ref(x, Y, bt, intercept, mode)
    err = np.abs(got - ref)
    assert np.all(np.isfinite(got)), "a NaN: padding was read, or an entry was not written"
    worst = float((err / np.maximum(tol, 1e-300)).max()) if mode else float(err.max())
    print(f"n={x.shape[0]} p={x.shape[1]} m={Y.shape[1]} mode={mode} {xl}/{yl}: worst error / tolerance = {worst:.3g}")
    if mode:
        assert np.all(err <= tol), (worst, np.unravel_index(np.argmax(err / np.maximum(tol, 1e-300)), err.shape))
    else:
        assert np.all(err <= tol)
        assert np.array_equal(got[:, -1], np.zeros(Y.shape[1]))            # no link, no loss
    return got


# ------------------------------------------------------------------------------------------------ against numpy, at the tiling's edges
def test_row_edges(api, num_cu):
    """row tiles of 16, sub-blocks of 64, a short last chunk, more than one chunk"""
    rows = api.logistic_multi_plan(131, 17, 3, num_cu=num_cu)["rows"]     # (64 at these n on any device)
    for n in sorted({1, 15, 16, 17, 63, 64, 65, rows - 1, rows + 1, 2 * rows - 1, 2 * rows + 3, 5 * rows + 33}):
        assert api.logistic_multi_plan(n, 17, 3, num_cu=num_cu)["rows"] == rows
        x, Y, bt = _case(n, 17, 3, 100 + n)
        for mode in (1, 0):
            _check(api, x, Y, bt, True, mode)


@pytest.mark.parametrize("p", [2, 3, 15, 16, 17, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023])
def test_column_edges(api, p):
    """16-column tiles, the wave split and the band edges 128 / 256 / 512 (2, 4, 8, 16 tiles per wave)"""
    x, Y, bt = _case(130, p, 2, 200 + p, f32=True)
    for xl, yl in (("cm", "rm"), ("rm", "cm"), ("f32", "rm")):
        _check(api, x, Y, bt, True, 1, xl, yl)
    _check(api, x, Y, bt, True, 0, "rm", "cm")


@pytest.mark.parametrize("m", [1, 15, 16, 17, 33, 64, 65])
def test_response_edges(api, m):
    """response tiles, blocks of 16 LT, and the chunk of 64"""
    for p in (20, 300):                                                  # LT 4 and LT 2 for a full chunk
        x, Y, bt = _case(200, p, m, 300 + m + p)
        _check(api, x, Y, bt, True, 1, "cm", "cm")
        _check(api, x, Y, bt, True, 1, "rm", "rm")
    x, Y, bt = _case(100, 600, m, 400 + m, f32=True)                     # 16 tiles per wave: LT 1
    _check(api, x, Y, bt, True, 1, "f32", "rm")


def test_without_intercept(api):
    for n, p, m in ((65, 17, 3), (200, 129, 17), (130, 1024, 2)):
        x, Y, bt = _case(n, p, m, 500 + p, intercept=False, f32=True)
        for mode in (1, 0):
            _check(api, x, Y, bt, False, mode, "cm", "rm")
            _check(api, x, Y, bt, False, mode, "f32", "cm")


def test_mode0_sums_are_exact(api):
    """small-integer x and 0/1 Y: every product and partial sum is an integer, so any order gives the same double"""
    rng = np.random.default_rng(7)
    for n, p, m in ((1, 2, 1), (131, 17, 5), (2000, 129, 33), (700, 513, 65)):
        x = rng.integers(-8, 9, size=(n, p)).astype(np.float64)
        Y = (rng.uniform(size=(n, m)) < 0.5).astype(np.float64)
        want = np.zeros((m, p + 2))
        want[:, 0], want[:, 1:p + 1] = Y.sum(axis=0), (x.T @ Y).T
        for xl, yl in (("cm", "rm"), ("rm", "cm"), ("f32", "cm")):
            got = api.logistic_multi_rows(_x(x, xl), _y(Y, yl), None, mode=0)
            assert np.array_equal(got, want), (n, p, m, xl, yl)


# ------------------------------------------------------------------------------------------------ the live mask
def test_live_mask(api):
    import torch
    n, p, m = 300, 20, 40                                                # LT 4: blocks [0, 40) -- one block; with p = 300 (LT 2): two blocks
    for p in (20, 300):
        x, Y, bt = _case(n, p, m, 600 + p)
        xd, Yd = _x(x, "cm"), _y(Y, "rm")
        full = api.logistic_multi_rows(xd, Yd, bt)
        assert api.logistic_multi_stats()["blocks_skipped"] == 0
        block = api.logistic_multi_plan(n, p, m)["block"]
        live = np.ones(m, dtype=np.int32)
        live[[1, 5, m - 1]] = 0                                          # frozen among live ones
        out = torch.full((m, p + 2), -7.5, dtype=torch.float64, device="cuda")
        got = api.logistic_multi_rows(xd, Yd, bt, live=live, out=out)
        assert np.array_equal(got[live == 0], np.full((3, p + 2), -7.5))   # the sentinel stays
        assert np.array_equal(got[live == 1], full[live == 1])             # the bytes of the pass with every response live
        assert api.logistic_multi_stats()["blocks_skipped"] == 0
        if block < m:                                                    # a whole block frozen: untouched and counted
            live = np.ones(m, dtype=np.int32)
            live[:block] = 0
            out = torch.full((m, p + 2), -7.5, dtype=torch.float64, device="cuda")
            got = api.logistic_multi_rows(xd, Yd, bt, live=live, out=out)
            assert np.array_equal(got[:block], np.full((block, p + 2), -7.5))
            assert np.array_equal(got[block:], full[block:])
            assert api.logistic_multi_stats()["blocks_skipped"] == 1
    # every response frozen: nothing is written, every block is skipped
    out = torch.full((m, p + 2), -7.5, dtype=torch.float64, device="cuda")
    got = api.logistic_multi_rows(xd, Yd, bt, live=np.zeros(m, dtype=np.int32), out=out)
    assert np.array_equal(got, np.full((m, p + 2), -7.5))
    assert api.logistic_multi_stats()["blocks_skipped"] == api.logistic_multi_plan(n, p, m)["blocks"]


# ------------------------------------------------------------------------------------------------ the same bytes
@pytest.mark.parametrize("p", [20, 300, 600])
def test_a_response_has_the_same_bytes_whatever_it_is_computed_among(api, p):
    n, m = 1500, 65
    x, Y, bt = _case(n, p, m, 700 + p, f32=True)
    xd = {k: _x(x, k) for k in ("cm", "rm", "f32")}
    for mode in (1, 0):
        b = bt if mode else None
        full = api.logistic_multi_rows(xd["cm"], _y(Y, "rm"), b, mode=mode)
        assert np.all(np.isfinite(full))
        # two calls; all three layouts of x; both layouts of Y
        assert np.array_equal(full, api.logistic_multi_rows(xd["cm"], _y(Y, "rm"), b, mode=mode))
        assert np.array_equal(full, api.logistic_multi_rows(xd["rm"], _y(Y, "cm"), b, mode=mode))
        assert np.array_equal(full, api.logistic_multi_rows(xd["f32"], _y(Y, "rm"), b, mode=mode))
        # m = 1 against m = 65, whatever its column index
        for r in (0, 17, 63, 64):
            one = api.logistic_multi_rows(xd["rm"], _y(Y[:, [r]], "rm"), None if b is None else b[[r]], mode=mode)
            assert np.array_equal(one[0], full[r]), (mode, r)
        perm = np.random.default_rng(p).permutation(m)
        shuffled = api.logistic_multi_rows(xd["cm"], _y(Y[:, perm], "cm"), None if b is None else b[perm], mode=mode)
        assert np.array_equal(shuffled, full[perm]), mode
        part = api.logistic_multi_rows(xd["cm"], _y(Y[:, :17], "rm"), None if b is None else b[:17], mode=mode)
        assert np.array_equal(part, full[:17]), mode
