"""xval.oem's CV-error kernel (oem_amd/csrc/xval.hip: cv_error_kernel<LT, KC, SINGLE, CHUNK> and cv_finish_kernel) on the MI355X against
numpy in long double, at every launch form -- the cases of tests/test_gpu_xval.py reach it only through fitted coefficient tables, whose
rows beyond the signal are zero and whose neighbouring lambdas and folds are nearly equal.

The entry oemgpu_selftest_xval_cv_error_dev runs the phase on a coefficient table of the caller's: the fold layout, the gather, the
weight scaling and the launch are those of oemgpu_xval_dense_dev.  The tables here are dense -- normal draws / sqrt(p + 1), different for
every fold, penalty and lambda -- and every case asserts ON NUMPY'S SIDE, before the GPU is called, that a subtly wrong kernel would
show: zeroing the coefficient row of the last x column, zeroing the intercepts, rolling the table by one fold, by one lambda (where there
are two) and by one penalty (where there are two) each move every cvm by more than 1e-6 relative, a million times the tolerance.  Seeds
were picked on the CPU so that this holds; no case is excluded.  Every case first asks oemgpu_selftest_xval_cv_plan, with the live CU
count, for the form, the lambda tiles, the passes and the chunking it is named for.

Reference: with b = coef[foldid_i - 1, pen, lam], v_i = (y_i - b[0] - x_i . b[1:])^2 or |.|, times w_i with weights
(ref src/oem_xval_dense.cpp:389-437); cvm = mean v, cvsd = sqrt(sum (v - cvm)^2 / (n - 1)) / sqrt(n); triples (n, mean, M2).
Tolerances: cvm and triple means rtol 1e-12 (the figure of test_cv_error_variance_with_a_tiny_spread for this kernel), cvsd and M2 1e-11
(the ratio _compare uses), counts exact.  The yardstick is the reference's own float64 error: every case evaluates numpy in float64 too
and asserts that it lies within 1e-13 of long double, so the reference is not what limits the comparison.

Largest gaps measured on an MI355X against long double (relative), per form, over the cases of this file:
    SINGLE  cvm 2.8e-16  cvsd 3.6e-16
    multi   cvm 3.1e-16  cvsd 1.2e-15
    CHUNK   cvm 3.1e-16  cvsd 5.6e-16
-- the size of numpy's own float64 gap on the same cases (cvm 2.5e-16, cvsd 2.9e-16), three to four orders below the tolerances."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_gpu_xval import _compare
from tests.test_xval_cv_plan_cpu import CHUNK, MULTI, PINNED, SINGLE

pytestmark = pytest.mark.gpu

RTOL_M, RTOL_S = 1e-12, 1e-11
FORMS = {SINGLE: "single", MULTI: "multi", CHUNK: "chunk"}
LD = np.longdouble


@pytest.fixture(scope="module")
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def api():
    from oem_amd import api
    return api


# ------------------------------------------------------------------------------------------------------------- the reference
def _errors(x, y, fid, coef, measure, w, dtype):
    """v[npen, nl, n] in `dtype`"""
    K, npen, nl, _ = coef.shape
    xx, yy = x.astype(dtype), y.astype(dtype)
    v = np.zeros((npen, nl, len(y)), dtype=dtype)
    for k in range(K):
        rows = np.nonzero(fid == k + 1)[0]
        if len(rows) == 0:
            continue
        b = coef[k].astype(dtype)
        res = yy[rows] - (b[..., :1] + b[..., 1:] @ xx[rows].T)
        e = res * res if measure == "mse" else np.abs(res)
        v[:, :, rows] = e if w is None else e * w[rows].astype(dtype)
    return v


def _moments(v):
    n = v.shape[-1]
    m = v.mean(axis=-1)
    m2 = ((v - m[..., None]) ** 2).sum(axis=-1)
    sd = np.sqrt(m2 / max(n - 1, 1)) / np.sqrt(v.dtype.type(n))
    return m, sd, m2


def _reference(x, y, fid, coef, measure, w=None):
    """(cvm, cvsd, M2) in long double, after the assertions that belong to numpy alone: float64 numpy is within 1e-13 of it, and the
    table discriminates (module docstring)"""
    cvm, cvsd, m2 = _moments(_errors(x, y, fid, coef, measure, w, LD))
    c64, s64, _ = _moments(_errors(x, y, fid, coef, measure, w, np.float64))
    gap_m, gap_s = float(np.max(np.abs(c64 - cvm) / cvm)), float(np.max(np.abs(s64 - cvsd) / cvsd))
    print(f"numpy float64 against long double: cvm {gap_m:.1e} cvsd {gap_s:.1e}")
    assert gap_m < 1e-13 and gap_s < 1e-13, (gap_m, gap_s)
    K, npen, nl, _ = coef.shape
    wrong = {}
    t = coef.copy(); t[..., -1] = 0.0; wrong["last column zeroed"] = t
    t = coef.copy(); t[..., 0] = 0.0; wrong["intercept zeroed"] = t
    wrong["folds rolled"] = np.roll(coef, 1, axis=0)
    if nl > 1:
        wrong["lambdas rolled"] = np.roll(coef, 1, axis=2)
    if npen > 1:
        wrong["penalties rolled"] = np.roll(coef, 1, axis=1)
        wrong["fold and penalty swapped"] = coef.reshape(K * npen, nl, -1)[
            [(pen * npen + k) % (K * npen) for k in range(K) for pen in range(npen)]].reshape(coef.shape)
    for name, tab in wrong.items():
        moved = np.abs(_moments(_errors(x, y, fid, tab, measure, w, np.float64))[0] - c64) / c64
        assert moved.min() > 1e-6, (name, float(moved.min()))
    return cvm, cvsd, m2


def _gap(got, ref):
    return float(np.max(np.abs(got.astype(LD) - ref) / np.abs(ref)))


def _meets(got_m, got_s, ref, label):
    gm, gs = _gap(got_m, ref[0]), _gap(got_s, ref[1])
    print(f"GAP {label}: cvm {gm:.1e} cvsd {gs:.1e}")
    assert np.all(np.isfinite(got_m)) and np.all(np.isfinite(got_s))
    assert gm <= RTOL_M, (label, gm)
    assert gs <= RTOL_S, (label, gs)


def _dev(x, y, fid, w=None, pad=0):
    """x, y, foldid (and w) on the device; pad > 0: x is a view of a taller column-major buffer (ld = n + pad) whose spare rows are NaN"""
    import torch
    n, p = x.shape
    buf = torch.full((p, n + pad), float("nan"), dtype=torch.float64, device="cuda:0")
    xd = buf.t()[:n]
    xd.copy_(torch.as_tensor(np.ascontiguousarray(x)))
    assert xd.stride() == (1, n + pad)
    return (xd, torch.as_tensor(np.asarray(y, dtype=np.float64), device="cuda:0"),
            torch.as_tensor(np.ascontiguousarray(fid, dtype=np.int32), device="cuda:0"),
            None if w is None else torch.as_tensor(np.asarray(w, dtype=np.float64), device="cuda:0"))


def _table(seed, K, npen, nl, p):
    return np.random.default_rng(seed).normal(size=(K, npen, nl, p + 1)) / np.sqrt(p + 1.0)


def _weights(rng, fid, K):
    """uniform weights with zeros, one of them on the first row of every fold -- where the wave takes its centre"""
    w = rng.uniform(0.1, 4.0, len(fid))
    w[rng.integers(0, len(fid), 9)] = 0.0
    for k in range(1, K + 1):
        rows = np.nonzero(fid == k)[0]
        if len(rows):
            w[rows[0]] = 0.0
    return w


def _assert_plan(api, num_cu, n, p, K, npen, nl, form, lt=None, passes=None, chunks=None, last=None):
    P = api.xval_cv_plan(n, p, K, npen, nl, num_cu)
    want = dict(form=FORMS[form], lt=lt, passes=passes, chunks=chunks, last=last)
    assert all(P[k] == v for k, v in want.items() if v is not None), (P, want)
    return P


# ------------------------------------------------------------------------------------------------------------- A: forms and tiles
TABLE_SEED = {(160, 112): 1, (224, 100): 1, (230, 224): 1}
# picked on the CPU: the first table seed at which the preconditions of _reference hold at mse and mae, with and without weights (0 elsewhere)


@functools.lru_cache(maxsize=None)
def _case_a(p, nl):
    n, K = (403 if p > 1000 else 703), 3
    rng = np.random.default_rng(1000 * p + nl)
    x = np.asfortranarray(rng.normal(size=(n, p)) + 0.1)
    y = rng.normal(size=n) + 0.3
    fid = rng.permutation(np.resize(np.arange(1, K + 1), n))
    assert all((fid == k).sum() % 16 for k in range(1, K + 1))
    return x, y, fid, _table(7 * p + nl + 100000 * TABLE_SEED.get((p, nl), 0), K, 1, nl, p), _weights(rng, fid, K)


WEIGHTED = {(55, 112), (7, 32), (8, 48), (20, 250), (56, 113), (159, 112), (160, 112), (224, 100), (230, 224), (1120, 16)}
assert {PINNED[c][0] for c in WEIGHTED} == {SINGLE, MULTI, CHUNK}


def _a_params():
    for (p, nl) in PINNED:
        for weighted in ((False, True) if (p, nl) in WEIGHTED else (False,)):
            yield pytest.param(p, nl, weighted, id=f"p{p}-nl{nl}" + ("-w" if weighted else ""))


@pytest.mark.parametrize("measure", ["mse", "mae"])
@pytest.mark.parametrize("p,nl,weighted", list(_a_params()))
def test_forms_and_tiles(api, num_cu, p, nl, weighted, measure):
    """every pinned shape of tests/test_xval_cv_plan_cpu.py, in the form the plan reports for it on this device: n = 703 (403 at
    p ~ 1120), three random folds of 235 / 234 / 234 (135 / 134 / 134) rows -- no multiple of 16 -- one penalty"""
    form, lt, passes, chunks, last = PINNED[(p, nl)]
    x, y, fid, coef, w = _case_a(p, nl)
    w = w if weighted else None
    _assert_plan(api, num_cu, x.shape[0], p, 3, 1, nl, form, lt, passes, chunks, last)
    ref = _reference(x, y, fid, coef, measure, w)
    xd, yd, fd, wd = _dev(x, y, fid, w)
    cvm, cvsd = api.xval_cv_error(xd, yd, fd, 3, coef, measure, weights=wd)
    _meets(cvm, cvsd, ref, f"{FORMS[form]} p={p} nl={nl} {measure}{' weighted' if weighted else ''}")


# ------------------------------------------------------------------------------------------------------------- B: rows and grid
@functools.lru_cache(maxsize=None)
def _fold_size_case(p, nl):
    sizes = {1: 1, 2: 15, 3: 16, 4: 17, 5: 129, 7: 2822}               # id 6 never occurs
    rng = np.random.default_rng(500 + p)
    fid = rng.permutation(np.concatenate([np.full(c, k) for k, c in sizes.items()]))
    n = len(fid)
    x = np.asfortranarray(rng.normal(size=(n, p)) + 0.1)
    y = rng.normal(size=n) + 0.3
    return x, y, fid, _table(501 + p, 7, 1, nl, p), sizes


@pytest.mark.parametrize("measure", ["mse", "mae"])
@pytest.mark.parametrize("p,nl,form", [(20, 40, SINGLE), (160, 112, CHUNK)])
def test_fold_sizes(api, num_cu, p, nl, form, measure):
    """folds of 1, 15, 16, 17 and 129 rows, an id that never occurs, and one fold of 2822 rows that takes several rounds of nwg * 8 row
    tiles with a partial last one: in CHUNK form the idle waves of that round still meet the staging barriers"""
    x, y, fid, coef, sizes = _fold_size_case(p, nl)
    n = len(fid)
    assert n == 3000 and not np.any(fid == 6)
    P = _assert_plan(api, num_cu, n, p, 7, 1, nl, form, lt=(nl + 15) // 16, passes=1)
    tiles, per = -(-sizes[7] // 16), P["nwg"] * 8
    assert P["nwg"] > 1 and tiles > 2 * per and tiles % per != 0 and tiles % 8 != 0, (P, tiles)
    ref = _reference(x, y, fid, coef, measure)
    xd, yd, fd, _ = _dev(x, y, fid)
    cvm, cvsd = api.xval_cv_error(xd, yd, fd, 7, coef, measure)
    _meets(cvm, cvsd, ref, f"{FORMS[form]} fold sizes {measure}")


@pytest.mark.parametrize("n,p,K,npen,nl", [(4001, 10, 130, 3, 20), (701, 10, 2, 1, 20), (3001, 3, 512, 1, 20)],
                         ids=["K130-npen3", "K2", "K512"])
def test_grid_limits(api, num_cu, n, p, K, npen, nl):
    """more (fold, penalty) pairs than CUs -- one workgroup each; the fewest folds; the most"""
    rng = np.random.default_rng(600 + K)
    x = np.asfortranarray(rng.normal(size=(n, p)) + 0.1)
    y = rng.normal(size=n) + 0.3
    fid = rng.integers(1, K + 1, n)
    coef = _table(601 + K, K, npen, nl, p)
    P = _assert_plan(api, num_cu, n, p, K, npen, nl, SINGLE, lt=2, passes=1)
    if K * npen > num_cu:
        assert P["nwg"] == 1, P
    else:
        assert K == 2 and P["nwg"] == min(num_cu // 2, 3), P
    w = _weights(rng, fid, K) if K == 130 else None
    for measure in ("mse", "mae"):
        ref = _reference(x, y, fid, coef, measure, w)
        xd, yd, fd, wd = _dev(x, y, fid, w)
        cvm, cvsd = api.xval_cv_error(xd, yd, fd, K, coef, measure, weights=wd)
        _meets(cvm, cvsd, ref, f"single K={K} npen={npen} {measure}")


@pytest.mark.parametrize("K", [1, 513])
def test_fold_counts_refused(api, K):
    import oem_amd
    x, y, fid, _, _ = _case_a(7, 32)
    xd, yd, fd, _ = _dev(x, y, np.ones_like(fid))
    with pytest.raises(oem_amd.OemgpuError, match="nfolds must be in 2..512") as e:
        api.xval_cv_error(xd, yd, fd, K, _table(1, K, 1, 32, 7))
    assert e.value.code == -1


@pytest.mark.parametrize("p,nl,weighted", [(55, 112, False), (160, 112, True)])
def test_leading_dimension_and_repeatability(api, num_cu, p, nl, weighted):
    """x as a view with ld = n + 37 whose spare rows are NaN: finite, and the bits of the compact copy; a second identical call: the
    same bits again"""
    x, y, fid, coef, w = _case_a(p, nl)
    w = w if weighted else None
    _assert_plan(api, num_cu, x.shape[0], p, 3, 1, nl, PINNED[(p, nl)][0])
    ref = _reference(x, y, fid, coef, "mse", w)
    xd, yd, fd, wd = _dev(x, y, fid, w, pad=37)
    assert xd.stride(1) == x.shape[0] + 37
    padded = api.xval_cv_error(xd, yd, fd, 3, coef, "mse", weights=wd)
    xc, _, _, _ = _dev(x, y, fid)
    compact = api.xval_cv_error(xc, yd, fd, 3, coef, "mse", weights=wd)
    again = api.xval_cv_error(xc, yd, fd, 3, coef, "mse", weights=wd)
    _meets(padded[0], padded[1], ref, f"{FORMS[PINNED[(p, nl)][0]]} ld = n + 37")
    for a, b in ((padded, compact), (compact, again)):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_stale_scratch(api, monkeypatch):
    """The fold-ordered copy in the context's scratch keeps what an earlier call of the same layout left in the rows that are padding
    now.  (1) the entry on NaN data with folds of 160 rows; (2) the same layout with folds of 161, 175, 145 and 159 rows, whose padding
    rows hold step 1's NaN: finite, and the reference's numbers; (3) xval_oem on the same context and layout: the bits of the same
    call made first on a context created fresh for it -- the moment kernels do not read the padding rows either"""
    import oem_amd
    import torch
    n, p, K, nl = 640, 12, 4, 10
    rng = np.random.default_rng(700)
    x = np.asfortranarray(rng.normal(size=(n, p)) + 0.1)
    y = x[:, :3] @ np.array([1.0, -1.0, 0.5]) + rng.normal(size=n)
    fid1 = np.repeat(np.arange(1, K + 1), 160)
    fid2 = np.repeat(np.arange(1, K + 1), [161, 175, 145, 159])
    assert [c % 16 for c in np.bincount(fid2)[1:]] == [1, 15, 1, 15] and len(fid2) == n
    coef = _table(701, K, 1, nl, p)
    xd, yd, fd2, _ = _dev(x, y, fid2)
    kw = dict(foldid=fid2, penalty="lasso", nlambda=nl, tol=1e-9)

    L = oem_amd.lib()
    fresh = L.oemgpu_create(0, None)
    assert fresh
    with monkeypatch.context() as m:
        m.setattr(api, "_ctx_cache", {(0, None): fresh})
        first = oem_amd.xval_oem(xd, y, **kw)
    L.oemgpu_destroy(fresh)

    ctx = oem_amd.context()
    nan_x, nan_y, fd1, _ = _dev(np.full((n, p), np.nan), np.full(n, np.nan), fid1)
    cvm, _ = api.xval_cv_error(nan_x, nan_y, fd1, K, coef, ctx=ctx)
    assert np.all(np.isnan(cvm))                                   # the NaN went through the copy
    ref = _reference(x, y, fid2, coef, "mse")
    cvm, cvsd = api.xval_cv_error(xd, yd, fd2, K, coef, ctx=ctx)
    _meets(cvm, cvsd, ref, "single after NaN scratch")
    assert oem_amd.context(torch.device("cuda:0").index) == ctx
    second = oem_amd.xval_oem(xd, y, **kw)
    for key in ("beta", "cvm", "cvsd"):
        assert np.all(np.isfinite(second[key][0]))
        assert first[key][0].tobytes() == second[key][0].tobytes(), key


@pytest.mark.parametrize("p,nl", [(20, 250), (160, 112)])
def test_triples_and_their_merge(api, num_cu, p, nl):
    """(count, mean, M2) of all rows, and of two unequal row shards merged by oemgpu_xval_merge"""
    import oem_amd
    x, y, fid, coef, _ = _case_a(p, nl)
    n = len(y)
    _assert_plan(api, num_cu, n, p, 3, 1, nl, PINNED[(p, nl)][0])
    cvm_r, cvsd_r, m2_r = _reference(x, y, fid, coef, "mse")
    xd, yd, fd, _ = _dev(x, y, fid)
    tri = api.xval_cv_error(xd, yd, fd, 3, coef, "mse", triples=True)
    assert tri.shape == (1, nl, 3) and np.all(tri[..., 0] == n)
    assert _gap(tri[..., 1], cvm_r) <= RTOL_M and _gap(tri[..., 2], m2_r) <= RTOL_S
    cut = 263
    shards = []
    for rows in (slice(0, cut), slice(cut, n)):
        sd = _dev(np.asfortranarray(x[rows]), y[rows], fid[rows])
        shards.append(api.xval_cv_error(sd[0], sd[1], sd[2], 3, coef, "mse", triples=True))
        assert np.all(shards[-1][..., 0] == len(y[rows]))
    a = api._Args(["lasso"], [], nl, 1e-4, 1.0, 3.0, 0.5, 1e-7, 500, False, False, np.ones(p), np.zeros(0, np.int32), np.zeros(0, np.int32),
                  np.zeros(0))
    both = np.ascontiguousarray(np.stack(shards))
    cvm, cvsd = np.zeros((1, nl)), np.zeros((1, nl))
    dp = C.POINTER(C.c_double)
    assert oem_amd.lib().oemgpu_xval_merge(both.ctypes.data_as(dp), 2, C.byref(a.c), cvm.ctypes.data_as(dp), cvsd.ctypes.data_as(dp)) == 0
    _meets(cvm, cvsd, (cvm_r, cvsd_r), f"{FORMS[PINNED[(p, nl)][0]]} merged shards")


# ------------------------------------------------------------------------------------------------------------- C: end to end
@pytest.mark.parametrize("nl", [113, 250])
def test_xval_oem_beyond_112_lambdas(api, num_cu, nl):
    """two and three passes over the lambdas, the second case with two tiles of the last pass beyond the 16 there are"""
    import oem_amd
    rng = np.random.default_rng(800 + nl)
    n, p, K = 1000, 20, 4
    x = np.asfortranarray(rng.normal(size=(n, p)) * 1.5 + 0.2)
    y = x[:, :5] @ np.array([1.0, -1.5, 0.5, 2.0, -0.7]) + rng.normal(size=n) + 0.4
    fid = rng.permutation(np.resize(np.arange(1, K + 1), n))
    P = _assert_plan(api, num_cu, n, p, K, 2, nl, SINGLE, lt={113: 4, 250: 6}[nl], passes={113: 2, 250: 3}[nl])
    assert P["passes"] * P["lt"] - (nl + 15) // 16 == {113: 0, 250: 2}[nl]
    kw = dict(penalty=["lasso", "mcp"], nlambda=nl, tol=1e-10, maxit=5000, lambda_min_ratio=1e-3)
    r = orc.xval_dense(x, y, fid, **kw)
    f = oem_amd.xval_oem(x, y, foldid=fid, **kw)
    _compare(f, r, 2)


@functools.lru_cache(maxsize=None)
def _chunk_e2e(weighted):
    rng = np.random.default_rng(900)
    n, p, K = 900, 170, 3
    x = np.asfortranarray(rng.normal(size=(n, p)))
    y = x[:, -6:] @ np.array([1.0, -1.5, 0.5, 2.0, -0.8, 1.2]) + rng.normal(size=n) + 0.4
    fid = rng.permutation(np.resize(np.arange(1, K + 1), n))
    w = rng.uniform(0.5, 2.0, n) if weighted else None
    kw = dict(penalty=["lasso"], nlambda=100, tol=1e-10, maxit=20000, lambda_min_ratio=1e-2)
    r = orc.xval_dense(x, y, fid, weights=w, **kw)
    nz = (r["beta"][0][-6:] != 0).sum(axis=1)                             # lambdas at which each of the six is in the model
    print("lambdas with a non-zero coefficient, last six columns:", nz)
    assert nz.min() >= 51 and nz.max() >= 90                              # the second chunk multiplies non-zero rows at most lambdas
    return x, y, fid, w, kw, r


@pytest.mark.parametrize("how", ["host", "device", "weighted"])
def test_xval_oem_chunk_form_with_the_signal_in_the_last_columns(api, num_cu, how):
    """p = 170 at 100 lambdas: CHUNK with lt = 7, two chunks of 112 and 60 coefficient rows, and y built from the last six columns of x,
    so that the fitted rows the second chunk multiplies are not zero"""
    import oem_amd
    x, y, fid, w, kw, r = _chunk_e2e(how == "weighted")
    _assert_plan(api, num_cu, 900, 170, 3, 1, 100, CHUNK, lt=7, passes=1, chunks=2, last=60)
    xin = _dev(x, y, fid)[0] if how == "device" else x
    f = oem_amd.xval_oem(xin, y, foldid=fid, **({} if w is None else dict(weights=w)), **kw)
    _compare(f, r, 1)
