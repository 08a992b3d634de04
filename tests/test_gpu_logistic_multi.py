"""oem_fit_logistic_dense_multi on the device, end to end: parity per response with oem_fit_logistic_dense on the same tensors and with
the numpy restatement (tests/logistic_restatement.py) at the single fit's own tolerances, the boundaries of its plan, the independence
of a response from its companions (to the byte), the layouts of x, the interrupt and the counters."""
import numpy as np
import pytest

from tests import logistic_restatement as R
from tests.logistic_multi_restatement import data
from tests.test_gpu_logistic import _compare, _groups

pytestmark = pytest.mark.gpu

ERR_INTERRUPTED = -6
KW = dict(nlambda=12, tol=1e-9, irls_tol=1e-5, compute_loss=True)


@pytest.fixture(scope="module")
def oa():
    import oem_amd
    oem_amd.lib()
    return oem_amd


def _dev(a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    return t if dtype is None else t.to(dtype)


def _colmajor(x):
    """x on the device, column-major float64 (strides (1, n))"""
    return _dev(np.ascontiguousarray(np.asarray(x).T)).t()


def _same(a, b):
    """two fits are the same bytes (NaN included: a constant response has a NaN lambda grid in the reference too)"""
    for key in ("beta", "lambda", "niter", "loss"):
        for u, v in zip(a[key], b[key]):
            if np.asarray(u).tobytes() != np.asarray(v).tobytes():
                return False
    return np.float64(a["d"]).tobytes() == np.float64(b["d"]).tobytes()


def _hold(oa, x, Y, pens, kw, groups=None, restatement=True, single=True):
    """multi against the single fit on the device and against the restatement, per response; returns the fits"""
    xd = _colmajor(x)
    fits = oa.oem_fit_logistic_dense_multi(xd, _dev(Y), penalty=pens, **({} if groups is None else dict(groups=groups)), **kw)
    assert len(fits) == Y.shape[1]
    icpt = kw.get("intercept", True)
    g, ug = _groups(pens, groups, icpt) if groups is not None else (None, None)
    for r, fit in enumerate(fits):
        if single:
            one = oa.oem_fit_logistic_dense(xd, Y[:, r], penalty=pens, **({} if groups is None else dict(groups=groups)), **kw)
            _compare(fit, one, pens)
        if restatement:
            rkw = dict(kw)
            if "lambda_" in kw:                                          # (one shared vector: the restatement takes a row per penalty)
                rkw["lambda_"] = [np.sort(np.asarray(kw["lambda_"], dtype=np.float64))[::-1]] * len(pens)
            _compare(fit, R.fit(x, Y[:, r], penalty=pens, groups=g, unique_groups=ug, **rkw), pens)
        assert fit["family"] == "binomial" and type(fit).__name__ == "OemFitBinomial"
        assert np.float64(fit["d"]).tobytes() == np.float64(fits[0]["d"]).tobytes()                # d: equal bytes for all m
    return fits


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("n,p,m,seed", [(3000, 24, 4, 11), (2000, 17, 5, 12)])
def test_parity_on_the_cpu_cases_and_the_counters(oa, n, p, m, seed):
    x, Y = data(n, p, m, seed)
    pens = ["lasso", "mcp"]
    fits = _hold(oa, x, Y, pens, KW)
    # (the last call in _hold was a single fit: the multi stats are this thread's last multi call)
    st = oa.logistic_multi_stats()
    ni = np.array([[f["niter"][k] for k in range(len(pens))] for f in fits])                       # [m, npen, nl]
    steps = int(np.minimum(ni, 100).max(axis=0).sum())
    assert st["steps"] == steps, (st, steps)                                                     # sum over (penalty, lambda) of max_r niter
    assert st["row_passes"] == steps - len(pens) * (KW["nlambda"] - 1), st                        # less the skipped first steps
    assert st["grams"] == 1 and st["lanczos"] == 1, st
    assert int(np.sum(ni.max(axis=0) != ni.min(axis=0))) > ni.shape[1] * ni.shape[2] // 2          # the freeze was exercised
    # the methods of a single fit work on each
    from oem_amd import api
    ll = api.logLik(fits[1])
    pr = api.predict(fits[1], x[:5], type="response")
    assert np.all(np.isfinite(np.asarray(ll, dtype=np.float64))) and np.asarray(pr).shape[0] == 5


ALL_KW = dict(nlambda=12, compute_loss=True, alpha=0.6, gamma=3.7, tau=0.4, tol=1e-9, irls_tol=1e-5)
ALL_GROUPS = np.repeat(np.arange(1, 7), 4)


@pytest.fixture(scope="module")
def all_penalties(oa):
    """all 14 penalties at 3000 x 24, m = 3: the data and the one multi call the three cases below share"""
    x, Y = data(3000, 24, 3, 13)
    fits = oa.oem_fit_logistic_dense_multi(_colmajor(x), _dev(Y), penalty=list(R.PENALTIES), groups=ALL_GROUPS, **ALL_KW)
    return x, Y, fits


@pytest.mark.parametrize("r", [0, 1, 2])
def test_all_penalties(oa, all_penalties, r):
    """(a case per response: the numpy restatement of 14 penalties is what takes the time, as in test_gpu_logistic.test_all_penalties_small)"""
    x, Y, fits = all_penalties
    pens = list(R.PENALTIES)
    _compare(fits[r], oa.oem_fit_logistic_dense(_colmajor(x), Y[:, r], penalty=pens, groups=ALL_GROUPS, **ALL_KW), pens)
    g, ug = _groups(pens, ALL_GROUPS, True)
    _compare(fits[r], R.fit(x, Y[:, r], penalty=pens, groups=g, unique_groups=ug, **ALL_KW), pens)
    assert np.float64(fits[r]["d"]).tobytes() == np.float64(fits[0]["d"]).tobytes()


@pytest.mark.parametrize("kw", [dict(intercept=False), dict(standardize=False), dict(lambda_=[0.08, 0.03, 0.01, 0.002])],
                         ids=["no-intercept", "no-standardize", "user-lambda"])
def test_options(oa, kw):
    x, Y = data(1500, 20, 3, 14)
    _hold(oa, x, Y, ["lasso", "scad"], dict(nlambda=8, compute_loss=True, tol=1e-9, irls_tol=1e-5, **kw))


def test_ols_among_the_penalties(oa):
    x, Y = data(1500, 20, 3, 15)
    fits = _hold(oa, x, Y, ["lasso", "ols", "mcp"], dict(nlambda=6, compute_loss=True, tol=1e-9, irls_tol=1e-5))
    assert np.asarray(fits[0]["beta"][1]).shape == (21, 1)


# ------------------------------------------------------------------------------------------------ boundaries
@pytest.mark.parametrize("p", [109, 110])
def test_a_in_lds_or_not(oa, p):
    """q = 110: A in the inner kernel's LDS; q = 111: read from global memory"""
    x, Y = data(1500, p, 2, 16 + p)
    _hold(oa, x, Y, ["lasso"], dict(nlambda=5, compute_loss=True))


def test_q_1024(oa):
    x, Y = data(3000, 1023, 2, 17)
    _hold(oa, x, Y, ["lasso"], dict(nlambda=4, compute_loss=True, lambda_min_ratio=0.05))


def test_one_more_than_a_chunk_and_one(oa):
    from oem_amd import api
    mch = api.logistic_multi_plan(500, 8, 1)["mch"]
    x, Y = data(500, 8, mch + 1, 18, k=3)
    fits = _hold(oa, x, Y, ["lasso"], dict(nlambda=3, compute_loss=True), restatement=False)
    _compare(fits[mch], R.fit(x, Y[:, mch], penalty=["lasso"], nlambda=3, compute_loss=True), ["lasso"])
    one = _hold(oa, x, Y[:, :1], ["lasso"], dict(nlambda=3, compute_loss=True))                    # m = 1
    assert _same(one[0], fits[0])


# ------------------------------------------------------------------------------------------------ a response alone and among others
def test_a_fit_does_not_depend_on_its_companions(oa):
    n, p = 2000, 12
    x, ysep = R.near_separable(n, p, 5)
    rng = np.random.default_rng(19)
    Y = np.zeros((n, 6))
    for r in (0, 2, 4):                                                  # ordinary ones
        b = np.zeros(p)
        b[:4] = rng.uniform(-0.4, 0.4, 4)
        Y[:, r] = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-(x @ b)))).astype(np.float64)
    Y[:, 1] = 0.0                                                        # constant columns
    Y[:, 3] = 1.0
    Y[:, 5] = ysep                                                       # runs to irls_maxit
    kw = dict(penalty=["lasso"], nlambda=8, compute_loss=True, irls_maxit=30)
    xd = _colmajor(x)
    with np.errstate(all="ignore"):
        fits = oa.oem_fit_logistic_dense_multi(xd, _dev(Y), **kw)
        assert np.max(fits[5]["niter"][0]) == 31                         # the cap, among responses that all stopped before it
        assert max(int(np.max(fits[r]["niter"][0])) for r in (0, 2, 4)) < 31
        for r in range(6):
            alone = oa.oem_fit_logistic_dense_multi(xd, _dev(Y[:, [r]]), **kw)
            assert _same(alone[0], fits[r]), r
        perm = [5, 3, 0, 1, 4, 2]
        shuffled = oa.oem_fit_logistic_dense_multi(xd, _dev(Y[:, perm]), **kw)
        for k, r in enumerate(perm):
            assert _same(shuffled[k], fits[r]), r
        # the ordinary ones' bytes do not move when their companions are ordinary too
        plain = oa.oem_fit_logistic_dense_multi(xd, _dev(Y[:, [0, 2, 4]]), **kw)
        for k, r in enumerate((0, 2, 4)):
            assert _same(plain[k], fits[r]), r
            _compare(fits[r], R.fit(x, Y[:, r], **kw), ["lasso"])
        _compare(fits[5], R.fit(x, ysep, **kw), ["lasso"])


def test_same_bytes_from_every_layout_and_from_two_calls(oa):
    import torch
    x, Y = data(1800, 30, 5, 20)
    x = x.astype(np.float32).astype(np.float64)
    kw = dict(penalty=["lasso", "grp.lasso"], groups=np.repeat(np.arange(1, 7), 5), nlambda=6, compute_loss=True)
    cm = oa.oem_fit_logistic_dense_multi(_colmajor(x), _dev(Y), **kw)
    again = oa.oem_fit_logistic_dense_multi(_colmajor(x), _dev(Y), **kw)
    rm = oa.oem_fit_logistic_dense_multi(_dev(x), _dev(Y), **kw)
    f32 = oa.oem_fit_logistic_dense_multi(_dev(x, torch.float32), _dev(Y), **kw)
    ycm = oa.oem_fit_logistic_dense_multi(_dev(x, torch.float32), _colmajor(Y), **kw)                # Y column-major, read where it lies
    host_y = oa.oem_fit_logistic_dense_multi(_dev(x), Y, **kw)                                    # a host Y is uploaded once
    for r in range(5):
        for other in (again, rm, f32, ycm, host_y):
            assert _same(cm[r], other[r]), r


def test_nothing_is_copied(oa):
    import torch
    n, p, m = 200_000, 16, 8
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    x = torch.randn((n, p), generator=g, device="cuda", dtype=torch.float32)
    Y = (torch.rand((n, m), generator=g, device="cuda", dtype=torch.float64) < 0.3).to(torch.float64)
    assert x.stride() == (p, 1) and Y.stride() == (m, 1)
    before, ybefore = x.clone(), Y.clone()
    oa.oem_fit_logistic_dense_multi(x, Y, penalty="lasso", nlambda=5)    # (the context and its buffers exist from here on)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    fits = oa.oem_fit_logistic_dense_multi(x, Y, penalty="lasso", nlambda=5)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"logistic multi row-major f32: peak allocated bytes grew by {grown} of {n * p * x.element_size()}")
    assert grown < n * p * x.element_size()
    assert torch.equal(x, before) and torch.equal(Y, ybefore)
    assert all(np.all(np.isfinite(f["beta"][0])) for f in fits)


def test_a_non_binary_device_column_is_named_without_a_host_copy(oa, monkeypatch):
    import torch
    x, Y = data(300, 6, 3, 21)
    Yd = _dev(Y)
    Yd[7, 2] = 0.5
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("Y was copied to the host")))
    with pytest.raises(ValueError) as e:
        oa.oem_fit_logistic_dense_multi(_colmajor(x), Yd, penalty="lasso")
    assert "column 2 of Y" in str(e.value)


def test_interrupt(oa):
    x, Y = data(800, 10, 3, 22)
    xd, Yd = _colmajor(x), _dev(Y)
    calls = []

    def fire():
        calls.append(1)
        return len(calls) >= 3

    with pytest.raises(oa.OemgpuError) as e:
        oa.oem_fit_logistic_dense_multi(xd, Yd, penalty="lasso", nlambda=5, interrupt=fire)
    assert e.value.code == ERR_INTERRUPTED and len(calls) == 3          # polled once per lock-step IRLS step
    fits = oa.oem_fit_logistic_dense_multi(xd, Yd, penalty="lasso", nlambda=5)                    # the same context serves the next call
    for r in range(3):
        _compare(fits[r], oa.oem_fit_logistic_dense(xd, Y[:, r], penalty="lasso", nlambda=5), ["lasso"])
