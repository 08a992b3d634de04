"""xval.oem for many responses on one resident x (xval_oem_multi; oemgpu_xval_dense_multi_dev / _rm_dev): every element
against xval_oem on its column and against the oracle, odd folds, the fold X'Y pass against exact sums, bytes, the edges of the solve
chunks, the single-response batch against the bytes it returned before lambda groups existed, memory, the interrupt and the phase clock.

Bounds: TIGHT / DTOL of tests/test_gpu_rowmajor.py through _hold of tests/test_gpu_multi.py for beta, lambda, niter, loss and d; cvm to
rtol 1e-9 and cvsd to rtol 1e-8, as tests/test_gpu_cv_gaussian.py holds them.

lambda.min: the two calls form X'y in different summation orders (gram.hip's fold pass / multi.hip's fold X'Y pass), so a lambda grid may
differ in its last bits -- _hold bounds that at rtol 1e-12 -- and lambda.min, a member of that grid, with it.  "Equal" is therefore held as:
the same position in the grid, the same model.min and best.model, and the value to the grid's own bound of 1e-12."""
import json
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc
from tests import xval_batch_golden as golden
from tests.exact_gram import exact_gram
from tests.test_gpu_multi import _data, _hold, _nan_colmajor, _same_bytes
from tests.test_gpu_rowmajor import _colmajor, _nan_view, _rowmajor

ERR_ARG, ERR_UNSUPPORTED, ERR_INTERRUPTED = -1, -4, -6
NF = 4


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


def _responses(n, p, m, seed):
    """_data's x and Y with response r scaled by 1 + r: every response has a lambda grid (and a lambda.min) of its own"""
    x, Y = _data(n, p, m, seed)
    return x, Y * (1.0 + np.arange(m))


def _folds(n, K, seed):
    return np.random.default_rng(seed).permutation(np.resize(np.arange(1, K + 1), n))


def _hold_cv(fit, ref):
    for k in range(len(ref["cvm"])):
        assert np.allclose(fit["cvm"][k], ref["cvm"][k], rtol=1e-9, atol=0), (k, fit["cvm"][k], ref["cvm"][k])
        assert np.allclose(fit["cvsd"][k], ref["cvsd"][k], rtol=1e-8, atol=0), (k, fit["cvsd"][k], ref["cvsd"][k])


def _hold_min(fit, ref):
    """the same member of the grid (see the module's docstring)"""
    assert fit["model.min"] == ref["model.min"] and fit["best.model"] == ref["best.model"]
    k = ref["model.min"] - 1
    assert int(np.nonzero(fit["lambda"][k] == fit["lambda.min"])[0][0]) == int(np.nonzero(ref["lambda"][k] == ref["lambda.min"])[0][0])
    assert np.isclose(fit["lambda.min"], ref["lambda.min"], rtol=1e-12, atol=0)


def _hold_all(fit, ref, loss=False):
    _hold(fit, ref, loss=loss)
    _hold_cv(fit, ref)
    _hold_min(fit, ref)


# ------------------------------------------------------------------------------------------------ 1. parity
G130 = np.repeat(np.arange(1, 27), 5)
# (p, penalty, standardize, intercept, compute_loss, groups, n, m, type_measure, route)
PARITY = [
    (41, "lasso", True, True, False, None, 3000, 5, "mse", 0),
    (41, ["lasso", "mcp"], True, True, False, None, 3000, 5, "mae", 0),
    (41, "mcp", False, False, False, None, 3000, 5, "mae", 0),
    (130, "grp.lasso", True, True, False, G130, 3000, 5, "mse", 0),
    (250, "lasso", True, True, False, None, 3000, 5, "mse", 0),
    (300, "mcp", True, True, True, None, 3000, 5, "mae", 0),
    (1040, "lasso", True, True, False, None, 1600, 2, "mse", 1),
]
_PIDS = [f"p{c[0]}-{c[1] if isinstance(c[1], str) else '+'.join(c[1])}-{c[8]}" for c in PARITY]


def _parity_case(case):
    p, pen, std, icpt, closs, groups, n, m, tm, route = case
    x, Y = _responses(n, p, m, p + len(pen))
    kw = dict(penalty=pen, nlambda=10 if p > 1000 else 12, tol=1e-9, standardize=std, intercept=icpt, compute_loss=closs, type_measure=tm)
    okw = dict(kw, lambda_min_ratio=1e-4)
    if groups is not None:
        kw["groups"] = groups
        g = np.concatenate([[0], groups]) if icpt else np.asarray(groups)              # R/oem_xval.R:279-283
        okw.update(groups=g, unique_groups=np.unique(g))
    return x, Y, _folds(n, NF, p), kw, okw


@pytest.mark.parametrize("case", PARITY, ids=_PIDS)
def test_parity_with_xval_oem_and_the_oracle(oa, case):
    import torch
    p, pen, std, icpt, closs, groups, n, m, tm, route = case
    x, Y, fid, kw, okw = _parity_case(case)
    xc = _colmajor(x)
    fits = oa.xval_oem_multi(xc, torch.as_tensor(Y, device="cuda"), foldid=fid, **kw)
    assert len(fits) == m and [f["route"] for f in fits] == [route] * m
    # every response on its own grid: fitting them all on instance 0's would fail the lambda bound below
    assert not np.allclose(fits[0]["lambda"][0], fits[1]["lambda"][0], rtol=1e-3)
    assert len({f["lambda.min"] for f in fits}) >= 2
    for r in range(m):
        one = oa.xval_oem(xc, Y[:, r], foldid=fid, **kw)
        assert set(one) | {"route"} == set(fits[r])
        _hold_all(fits[r], one, loss=closs)
        ref = orc.xval_dense(np.asfortranarray(x), Y[:, r], fid, **okw)
        worst = max(float(np.nanmax(np.abs(np.asarray(fits[r]["beta"][k]) - np.asarray(ref["beta"][k])))) for k in range(len(ref["beta"])))
        print(f"GAP xval_multi p = {p} {pen} response {r}: largest coefficient difference to the oracle {worst:.3e}")
        _hold(fits[r], ref, loss=closs, niter=False)
        _hold_cv(fits[r], ref)
    # predict_xval and summary_xval take an element as they take xval_oem's result
    assert np.asarray(oa.predict_xval(fits[0], x[:7])).shape[0] == 7
    assert oa.summary_xval(fits[0]) is not None


# ------------------------------------------------------------------------------------------------ 2. folds
def _small(n, p, m, seed):
    x, Y = _responses(n, p, m, seed)
    return x, Y, _colmajor(x)


def test_fold_sizes_off_every_tile(oa):
    n, p, m = 515, 7, 3
    x, Y, xc = _small(n, p, m, 21)
    fid = _folds(n, 3, 22)
    assert all(int((fid == k).sum()) % 16 != 0 for k in (1, 2, 3))
    fits = oa.xval_oem_multi(xc, Y, foldid=fid, penalty="lasso", nlambda=10, tol=1e-9)
    for r in range(m):
        _hold_all(fits[r], oa.xval_oem(xc, Y[:, r], foldid=fid, penalty="lasso", nlambda=10, tol=1e-9))


def test_folds_of_one_row(oa):
    n, p, m = 300, 5, 3
    x, Y, xc = _small(n, p, m, 23)
    fid = np.resize(np.array([1, 4]), n)
    fid[10], fid[200] = 2, 3                                              # folds 2 and 3 hold one row each
    fits = oa.xval_oem_multi(xc, Y, foldid=fid, penalty="lasso", nlambda=10, tol=1e-9)
    for r in range(m):
        _hold_all(fits[r], oa.xval_oem(xc, Y[:, r], foldid=fid, penalty="lasso", nlambda=10, tol=1e-9))


def test_an_empty_fold_goes_as_xval_oem_takes_it(oa):
    n, p, m = 300, 5, 2
    x, Y, xc = _small(n, p, m, 24)
    fid = np.resize(np.array([1, 2, 4, 5]), n)                            # nfolds = 5, no row in fold 3
    kw = dict(foldid=fid, penalty="lasso", nlambda=10, tol=1e-9)
    try:
        ones = [oa.xval_oem(xc, Y[:, r], **kw) for r in range(m)]
    except oa.OemgpuError as e:
        with pytest.raises(oa.OemgpuError) as e2:
            oa.xval_oem_multi(xc, Y, **kw)
        assert e2.value.code == e.code
        return
    fits = oa.xval_oem_multi(xc, Y, **kw)
    for r in range(m):
        _hold_all(fits[r], ones[r])


def test_fold_refusals_from_the_device(oa):
    n, p, m = 60, 5, 2
    x, Y, xc = _small(n, p, m, 25)
    fid = np.ones(n, dtype=np.int64)
    fid[:3], fid[3:5] = 2, 3                                              # fold 1 keeps 55 rows: its fit would have n - 55 = 5 <= p
    with pytest.raises(oa.OemgpuError) as e:
        oa.xval_oem_multi(xc, Y, foldid=fid, penalty="lasso", nlambda=5)
    assert e.value.code == ERR_UNSUPPORTED and "dimension of x larger than number of observations" in str(e.value)
    bad = _folds(n, 3, 26)
    bad[7] = 0
    with pytest.raises(oa.OemgpuError) as e:
        oa.xval_oem_multi(xc, Y, foldid=bad, penalty="lasso", nlambda=5)
    assert e.value.code == ERR_ARG and "foldid" in str(e.value)
    good = oa.xval_oem_multi(xc, Y, foldid=_folds(n, 3, 26), penalty="lasso", nlambda=5)       # the same context serves the next call
    assert len(good) == m


# ------------------------------------------------------------------------------------------------ 3. exact fold X'Y
@pytest.mark.parametrize("p", [2, 16, 17, 100])
def test_composed_fold_moments_are_exact(api, p):
    import torch
    n, K = 515, 3
    for m in (1, 15, 16, 17, 33):
        rng = np.random.default_rng(1000 * p + m)
        kx, ky = rng.integers(-32, 33, size=(n, p)), rng.integers(-32, 33, size=(n, m))
        x, Y = kx / 8.0, ky / 8.0
        fid = _folds(n, K, p + m)
        xs = {"cm": _nan_colmajor(x, 7), "rm64": _nan_view(x, 0, torch.float64), "rm32": _nan_view(x, 5, torch.float32)}
        Ys = {"cm": _nan_colmajor(Y, 3), "rm": _nan_view(Y, 2, torch.float64)}
        got = {(a, b): api.xval_multi_fold_moments(xs[a][0], Ys[b][0], fid, K) for a in xs for b in Ys}
        first = got[("cm", "cm")]
        # finite everywhere: no padding row between the folds and no NaN neighbour of x or Y was read
        assert first.shape == (m, K, p + 2, p + 2) and np.all(np.isfinite(first))
        for key, g in got.items():                                       # all forms of x and of Y: the same bytes
            assert g.tobytes() == first.tobytes(), key
        ones = 8 * np.ones((n, 1), dtype=np.int64)
        for k in range(K):
            rows = fid == k + 1
            for r in range(m):
                exact = exact_gram(np.concatenate([kx, ky[:, r:r + 1], ones], axis=1)[rows]).astype(np.float64) / 64.0
                assert np.array_equal(first[r, k], exact), (m, r, k)


def test_composed_fold_moments_with_an_empty_and_a_one_row_fold(api):
    n, p, m, K = 200, 5, 3, 4
    rng = np.random.default_rng(3)
    kx, ky = rng.integers(-32, 33, size=(n, p)), rng.integers(-32, 33, size=(n, m))
    fid = np.resize(np.array([1, 4]), n)
    fid[17] = 2                                                           # fold 2: one row; fold 3: none
    got = api.xval_multi_fold_moments(_colmajor(kx / 8.0), ky / 8.0, fid, K)
    ones = 8 * np.ones((n, 1), dtype=np.int64)
    for k in range(K):
        for r in range(m):
            exact = exact_gram(np.concatenate([kx, ky[:, r:r + 1], ones], axis=1)[fid == k + 1]).astype(np.float64) / 64.0
            assert np.array_equal(got[r, k], exact), (r, k)


# ------------------------------------------------------------------------------------------------ 4. bytes
def _same_xval_bytes(a, b):
    _same_bytes(a, b)
    for k in range(len(a["cvm"])):
        assert np.asarray(a["cvm"][k]).tobytes() == np.asarray(b["cvm"][k]).tobytes()
        assert np.asarray(a["cvsd"][k]).tobytes() == np.asarray(b["cvsd"][k]).tobytes()


@pytest.mark.parametrize("case", [PARITY[0], PARITY[5]], ids=[_PIDS[0], _PIDS[5]])
def test_same_bytes(oa, case):
    import torch
    p, pen, std, icpt, closs, groups, n, m, tm, route = case
    x, Y, fid, kw, okw = _parity_case(case)
    xc, Yd = _colmajor(x), torch.as_tensor(Y, device="cuda")
    first = oa.xval_oem_multi(xc, Yd, foldid=fid, **kw)
    again = oa.xval_oem_multi(xc, Yd, foldid=fid, **kw)                                   # two calls
    row = oa.xval_oem_multi(_rowmajor(x, "f32", 5), Yd, foldid=fid, **kw)                 # a row-major float32 x, read in place
    host = oa.xval_oem_multi(xc, Y, foldid=fid, **kw)                                     # a host Y
    colY = oa.xval_oem_multi(xc, Yd.t().contiguous().t(), foldid=fid, **kw)               # a column-major Y
    for r in range(m):
        for other in (again, row, host, colY):
            _same_xval_bytes(first[r], other[r])
    # A response alone (m = 1): to the bounds of the parity test, NOT bit for bit -- the rows of an X'Y chunk are planned from the
    # number of response blocks, so the order of the sums may depend on m
    r = m - 1
    alone = oa.xval_oem_multi(xc, Yd[:, r:r + 1], foldid=fid, **kw)
    _hold_all(alone[0], first[r], loss=closs)


# ------------------------------------------------------------------------------------------------ 5. chunk edges
def test_solve_chunk_edges_small_p(oa, api):
    n, p, K = 300, 5, 3
    nb = api.xval_multi_plan(n, p, K, 1000, nl=5, num_cu=_cus())["nb"]
    assert nb * (K + 1) <= 513 < (nb + 1) * (K + 1)
    x, Y = _responses(n, p, nb + 1, 51)
    Y = Y / (1.0 + np.arange(nb + 1)) * (1.0 + np.arange(nb + 1) % 7)                    # (scales 1..7: finite grids at 129 responses)
    xc, fid = _colmajor(x), _folds(n, K, 52)
    kw = dict(foldid=fid, penalty="lasso", nlambda=5, tol=1e-9)
    ones = [oa.xval_oem(xc, Y[:, r], **kw) for r in range(nb + 1)]
    for m in (nb, nb + 1):                                               # one full chunk; a second chunk of one response
        assert api.xval_multi_plan(n, p, K, m, nl=5, num_cu=_cus())["solve_chunks"] == (1 if m == nb else 2)
        fits = oa.xval_oem_multi(xc, Y[:, :m], **kw)
        assert [f["route"] for f in fits] == [0] * m
        for r in range(m):
            _hold_all(fits[r], ones[r])


def test_solve_chunk_edges_cooperating_engine(oa, api):
    n, p, K = 1200, 300, 3
    nb = api.xval_multi_plan(n, p, K, 100, nl=5, num_cu=_cus())["nb"]
    assert 1 <= nb <= 16
    x, Y = _responses(n, p, nb + 1, 53)
    xc, fid = _colmajor(x), _folds(n, K, 54)
    kw = dict(foldid=fid, penalty="lasso", nlambda=5, tol=1e-9)
    ones = [oa.xval_oem(xc, Y[:, r], **kw) for r in range(nb + 1)]
    for m in (nb, nb + 1):
        fits = oa.xval_oem_multi(xc, Y[:, :m], **kw)
        assert [f["route"] for f in fits] == [0] * m
        for r in range(m):
            _hold_all(fits[r], ones[r])


# ------------------------------------------------------------------------------------------------ 6. the existing batch is untouched
@pytest.mark.parametrize("name", sorted(golden.PROBLEMS))
def test_xval_oem_returns_the_bytes_it_returned_before_lambda_groups(oa, name):
    """tests/golden/xval_batch_bytes.json: recorded on the parent of the commit that gave the batch its lambda groups (g = 0: all
    instances on instance 0's grid, bit for bit)"""
    want = json.loads((Path(__file__).parent / "golden" / "xval_batch_bytes.json").read_text())[name]
    got = golden.run(oa, name)
    for key in ("lambda", "cvm", "beta"):
        assert got[key] == want[key], (name, key)


# ------------------------------------------------------------------------------------------------ 7. memory, interrupt, clock
def test_peak_memory_stays_below_a_float32_copy(oa):
    import torch
    n, p, m = 60_000, 64, 4
    rng = np.random.default_rng(71)
    x = torch.as_tensor(rng.normal(size=(n, p)), device="cuda").float()
    Y = torch.as_tensor(rng.normal(size=(n, m)), device="cuda")
    fid = np.resize(np.arange(1, NF + 1), n)
    before = x.clone()
    call = lambda: oa.xval_oem_multi(x, Y, foldid=fid, penalty="lasso", nlambda=10)
    call()                                                                # (the context and its buffers exist from here on)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    fits = call()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"GAP xval_oem_multi row-major f32: peak allocated bytes grew by {grown} of {n * p * 4}")
    assert grown < n * p * 4
    assert all(np.all(np.isfinite(f["cvm"][0])) for f in fits) and torch.equal(x, before)


def test_interrupt_between_chunks(oa, api):
    n, p, K = 300, 5, 3
    nb = api.xval_multi_plan(n, p, K, 1000, nl=5, num_cu=_cus())["nb"]
    x, Y = _responses(n, p, nb + 1, 72)
    Y = Y / (1.0 + np.arange(nb + 1))
    xc, fid = _colmajor(x), _folds(n, K, 73)
    calls = []

    def fire():
        calls.append(1)
        return True

    with pytest.raises(oa.OemgpuError) as e:
        oa.xval_oem_multi(xc, Y, foldid=fid, penalty="lasso", nlambda=5, interrupt=fire)
    assert e.value.code == ERR_INTERRUPTED and len(calls) == 1          # polled once: behind the first chunk
    fits = oa.xval_oem_multi(xc, Y[:, :2], foldid=fid, penalty="lasso", nlambda=5)     # the same context serves the next call
    for r in range(2):
        _hold_all(fits[r], oa.xval_oem(xc, Y[:, r], foldid=fid, penalty="lasso", nlambda=5))


def test_phase_clock(oa, api):
    x, Y = _responses(3000, 41, 5, 74)
    xc, fid = _colmajor(x), _folds(3000, NF, 75)
    lib, ctx = oa.lib(), api.context()
    assert lib.oemgpu_set_timing(ctx, 1) == 0
    try:
        oa.xval_oem_multi(xc, Y, foldid=fid, penalty="lasso", nlambda=10)
        t = api.xval_multi_timings()
    finally:
        assert lib.oemgpu_set_timing(ctx, 0) == 0
    assert set(t) == {"fold_order", "fold_gram", "fold_xty", "compose", "paths", "cv_error"} and all(v > 0.0 for v in t.values()), t
    oa.xval_oem_multi(xc, Y, foldid=fid, penalty="lasso", nlambda=10)
    assert all(v == 0.0 for v in api.xval_multi_timings().values())      # timing off: nothing waits, nothing is reported
