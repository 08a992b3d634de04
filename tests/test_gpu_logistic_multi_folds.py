"""oem_fit_logistic_dense_multi_folds on the device: every instance (response r, fold k left out) of the one lock-step
call against the single fold entry on the same tensors and against the numpy restatement on the gathered rows, at DESIGN 3.20's own
tolerances (tests/test_gpu_logistic._compare: beta 1e-8, lambda 1e-12, loss and d 1e-10, equal niter); the bytes of an instance whatever
rides with it; the layouts of x; the fold edges; the counters; the refusals; the interrupt."""
import numpy as np
import pytest

from tests import logistic_restatement as R
from tests.logistic_multi_restatement import data
from tests.test_gpu_logistic import _compare, _groups
from tests.test_gpu_logistic_multi import _colmajor, _dev, _same

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED, ERR_INTERRUPTED = -1, -4, -6


@pytest.fixture(scope="module")
def oa():
    import oem_amd
    oem_amd.lib()
    return oem_amd


def _fd(fid):
    import torch
    return torch.as_tensor(np.ascontiguousarray(fid, dtype=np.int32), device="cuda")


def _single(oa, xd, Y, fd, K, r, k, pens, kw):
    if k == 0:
        return oa.oem_fit_logistic_dense(xd, Y[:, r], penalty=pens, **kw)
    return oa.oem_fit_logistic_dense(xd, Y[:, r], penalty=pens, _fold=(fd, K, k, _dev(Y[:, r])), **kw)


def _hold(oa, x, Y, fid, pens, kw, groups=None, restatement=True, instances=None):
    """every instance against the single entries on the device (d to the byte: the same Hessian pass) and the restatement on the gathered
    rows; returns the fits as a flat list in the order of `instances`"""
    xd, fd, K = _colmajor(x), _fd(fid), int(fid.max())
    gk = {} if groups is None else dict(groups=groups)
    pairs = [(r, k) for r in range(Y.shape[1]) for k in range(K + 1)] if instances is None else list(instances)
    fits = oa.oem_fit_logistic_dense_multi_folds(xd, _dev(Y), fid, instances=pairs, penalty=pens, **gk, **kw)
    assert len(fits) == len(pairs)
    icpt = kw.get("intercept", True)
    g, ug = _groups(pens, groups, icpt) if groups is not None else (None, None)
    for (r, k), fit in zip(pairs, fits):
        keep = fid != k
        one = _single(oa, xd, Y, fd, K, r, k, pens, dict(kw, **gk))
        _compare(fit, one, pens)
        assert np.float64(fit["d"]).tobytes() == np.float64(one["d"]).tobytes(), (r, k)
        assert fit["nobs"] == one["nobs"] == int(keep.sum())
        if restatement:
            rkw = dict(kw)
            if "lambda_" in kw:
                rkw["lambda_"] = [np.sort(np.asarray(kw["lambda_"], dtype=np.float64))[::-1]] * len(pens)
            _compare(fit, R.fit(x[keep], Y[keep, r], penalty=pens, groups=g, unique_groups=ug, **rkw), pens)
        assert fit["family"] == "binomial" and type(fit).__name__ == "OemFitBinomial"
    return fits


def _random_folds(n, K, seed):
    return np.random.default_rng(seed).permutation(np.resize(np.arange(1, K + 1), n))


# ------------------------------------------------------------------------------------------------ (a), (b), (f)
def test_parity_plain_call_and_counters(oa):
    x, Y = data(1500, 12, 3, 41)
    fid, K, pens = _random_folds(1500, 5, 42), 5, ["lasso", "mcp"]
    kw = dict(nlambda=20, compute_loss=True)
    fits = _hold(oa, x, Y, fid, pens, kw)
    xd, Yd = _colmajor(x), _dev(Y)
    nested = oa.oem_fit_logistic_dense_multi_folds(xd, Yd, fid, penalty=pens, **kw)            # the default: m lists [full, fold 1 .. K]
    st = oa.logistic_multi_stats()
    assert st["grams"] == K + 1 and st["lanczos"] == K + 1, st
    assert len(nested) == 3 and all(len(v) == K + 1 for v in nested)
    for r in range(3):
        for k in range(K + 1):
            assert _same(nested[r][k], fits[r * (K + 1) + k]), (r, k)
    # (b) the k = 0 instances are the plain call's bytes
    plain = oa.oem_fit_logistic_dense_multi(xd, Yd, penalty=pens, **kw)
    for r in range(3):
        assert _same(plain[r], nested[r][0]), r
    # (f) one lock-step call makes fewer row passes than the K + 1 calls of one group each
    all_passes = st["row_passes"]
    single = 0
    for k in range(K + 1):
        oa.oem_fit_logistic_dense_multi_folds(xd, Yd, fid, instances=[(r, k) for r in range(3)], penalty=pens, **kw)
        s1 = oa.logistic_multi_stats()
        assert s1["grams"] == 1 and s1["lanczos"] == 1, s1
        single += s1["row_passes"]
    print(f"row passes: {all_passes} for all pairs, {single} over single-group calls")
    assert all_passes < single


# ------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("m,K", [(3, 5), (13, 4)], ids=["18-instances", "65-instances"])
def test_an_instance_does_not_depend_on_its_companions(oa, m, K):
    n, p = 800, 8
    x, Y = data(n, p, m, 43 + m, k=3)
    fid = _random_folds(n, K, 44)
    xd, Yd = _colmajor(x), _dev(Y)
    kw = dict(penalty=["lasso"], nlambda=5, compute_loss=True)
    pairs = [(r, k) for r in range(m) for k in range(K + 1)]
    assert len(pairs) == m * (K + 1)
    fits = oa.oem_fit_logistic_dense_multi_folds(xd, Yd, fid, instances=pairs, **kw)
    by = dict(zip(pairs, fits))
    for pr in (pairs[0], pairs[K + 2], pairs[-1]):                        # one pair alone
        alone = oa.oem_fit_logistic_dense_multi_folds(xd, Yd, fid, instances=[pr], **kw)
        assert _same(alone[0], by[pr]), pr
    perm = [pairs[i] for i in np.random.default_rng(45).permutation(len(pairs))]
    perm = perm[: len(perm) // 2] + [perm[0]] + perm[len(perm) // 2:]    # a permuted list with a duplicate: other chunks, other neighbours
    shuffled = oa.oem_fit_logistic_dense_multi_folds(xd, Yd, fid, instances=perm, **kw)
    for pr, fit in zip(perm, shuffled):
        assert _same(fit, by[pr]), pr


# ------------------------------------------------------------------------------------------------ (d)
def test_same_bytes_from_every_layout_and_from_two_calls(oa):
    import torch
    x, Y = data(1200, 30, 3, 46)
    x = x.astype(np.float32).astype(np.float64)
    fid = _random_folds(1200, 3, 47)
    kw = dict(penalty=["lasso", "grp.lasso"], groups=np.repeat(np.arange(1, 7), 5), nlambda=6, compute_loss=True)
    cm = oa.oem_fit_logistic_dense_multi_folds(_colmajor(x), _dev(Y), fid, **kw)
    others = [oa.oem_fit_logistic_dense_multi_folds(_colmajor(x), _dev(Y), _fd(fid), **kw),                 # again, foldid on the device
              oa.oem_fit_logistic_dense_multi_folds(_dev(x), _colmajor(Y), fid, **kw),
              oa.oem_fit_logistic_dense_multi_folds(_dev(x, torch.float32), Y, fid, **kw)]
    for other in others:
        for r in range(3):
            for k in range(4):
                assert _same(cm[r][k], other[r][k]), (r, k)


# ------------------------------------------------------------------------------------------------ (e)
def test_folds_of_whole_chunks_and_three_rows_on_near_separable(oa):
    """tests/test_gpu_cv_logistic._case_b's folds: rows 256 .. 447 leave together, fold 1 has 3 rows; response 1 is near separable and
    hits irls_maxit, response 0 stops early"""
    from tests.test_gpu_cv_logistic import _case_b
    x, ysep, fid = _case_b()
    rng = np.random.default_rng(48)
    b = np.zeros(x.shape[1]); b[:3] = rng.uniform(-0.4, 0.4, 3)
    y0 = (rng.uniform(size=len(ysep)) < 1.0 / (1.0 + np.exp(-(x @ b)))).astype(np.float64)
    Y = np.column_stack([y0, ysep])
    with np.errstate(all="ignore"):
        fits = _hold(oa, x, Y, fid, ["lasso"], dict(nlambda=25, irls_maxit=30, compute_loss=True))
    ni = np.array([np.max(f["niter"][0]) for f in fits]).reshape(2, 5)
    print("largest niter per (response, fold):", ni.tolist())
    assert ni[1].max() > ni[0].max(), ni                                  # the instances of a lock-step chunk stop at very different steps


@pytest.mark.parametrize("p", [109, 110])
def test_a_in_lds_or_not(oa, p):
    x, Y = data(1500, p, 2, 49 + p)
    _hold(oa, x, Y, _random_folds(1500, 3, 50), ["lasso"], dict(nlambda=4, compute_loss=True, lambda_min_ratio=0.05), restatement=False,
          instances=[(0, 0), (1, 2), (0, 3), (1, 1)])


def test_q_1024(oa):
    x, Y = data(1700, 1023, 2, 51)
    _hold(oa, x, Y, _random_folds(1700, 3, 52), ["lasso"], dict(nlambda=3, compute_loss=True, lambda_min_ratio=0.2), restatement=False,
          instances=[(1, 3), (0, 1)])


@pytest.mark.parametrize("kw,pens", [(dict(intercept=False), ["lasso"]), (dict(standardize=False), ["scad"]),
                                     (dict(lambda_=[0.08, 0.03, 0.01, 0.002]), ["lasso"]), (dict(groups=np.repeat(np.arange(1, 6), 4)), ["grp.lasso"])],
                         ids=["no-intercept", "no-standardize", "user-lambda", "group-penalty"])
def test_options(oa, kw, pens):
    x, Y = data(900, 20, 2, 53)
    kw = dict(kw)
    groups = kw.pop("groups", None)
    _hold(oa, x, Y, _random_folds(900, 3, 54), pens, dict(nlambda=6, compute_loss=True, tol=1e-9, irls_tol=1e-5, **kw), groups=groups)


# ------------------------------------------------------------------------------------------------ (g)
def _raw_call(oa, xd, Yd, fd, K, resp, leave, m=None, hessian_full=0, intercept=1, nlambda=4):
    """the C entry itself with sentinel-filled outputs -> (rc, message, outputs)"""
    import ctypes as C
    from oem_amd import api, _lib as L
    n, p = xd.shape
    groups, ug, gw = api._group_setup(["lasso"], (), None, p, True)
    a = api._Args(["lasso"], api._lambda_list((), 1), nlambda, 1e-4, 1.0, 3.0, 0.5, 1e-7, 500, False, False, np.ones(p), groups, ug, gw)
    resp, leave = np.ascontiguousarray(resp, dtype=np.int32), np.ascontiguousarray(leave, dtype=np.int32)
    ni = len(resp)
    outs = [np.full((max(ni, 1), 1, nlambda, p + 1), -7.5), np.full((max(ni, 1), 1, nlambda), -7.5), np.full((max(ni, 1), 1, nlambda), -7, dtype=np.int32),
            np.full((max(ni, 1), 1, nlambda), -7.5), np.full(max(ni, 1), -7.5), np.full(max(ni, 1), -7, dtype=np.int64)]
    m = Yd.shape[1] if m is None else m
    rc = L.lib().oemgpu_fit_logistic_dense_multi_fold_dev(api.context(0), xd.data_ptr(), n, xd.stride(1), p, Yd.data_ptr(), Yd.stride(0), Yd.stride(1), m,
                                                          fd.data_ptr(), K, ni, api._iptr(resp), api._iptr(leave), 1, intercept, hessian_full, 100, 1e-3,
                                                          C.byref(a.c), api._dptr(outs[0]), api._dptr(outs[1]), api._iptr(outs[2]), api._dptr(outs[3]),
                                                          api._dptr(outs[4]), outs[5].ctypes.data_as(C.POINTER(C.c_int64)))
    untouched = all(np.all(o == (-7 if o.dtype.kind == "i" else -7.5)) for o in outs)
    return rc, L.lib().oemgpu_last_error().decode(), untouched


def test_refusals_write_nothing(oa):
    import torch
    x, Y = data(300, 6, 2, 55)
    fid = _random_folds(300, 4, 56)
    xd, Yd, fd = _colmajor(x), _dev(Y), _fd(fid)
    torch.cuda.synchronize()
    for args, code, word in [((2, [0], [1]), ERR_ARG, "nfolds must be bigger than 3"),
                             ((4, [0], [5]), ERR_ARG, "leave_out must be in [0, nfolds]"),
                             ((4, [0], [-1]), ERR_ARG, "leave_out"),
                             ((4, [2], [1]), ERR_ARG, "resp must be in [0, m)"),
                             ((4, [-1], [1]), ERR_ARG, "resp"),
                             ((4, [], []), ERR_ARG, "ninst")]:
        rc, msg, untouched = _raw_call(oa, xd, Yd, fd, *args)
        assert rc == code and word in msg and untouched, (args, rc, msg)
    rc, msg, untouched = _raw_call(oa, xd, Yd, fd, 4, [0, 1], [0, 1], hessian_full=1)
    assert rc == ERR_UNSUPPORTED and "full Hessian" in msg and untouched
    for bad in (0, 5):                                                   # a fold id outside [1, nfolds], found on the device; also with leave 0 only
        f2 = fid.copy(); f2[123] = bad
        for leave in ([0, 1], [0, 0]):
            rc, msg, untouched = _raw_call(oa, xd, Yd, _fd(f2), 4, [0, 1], leave)
            assert rc == ERR_ARG and "fold ids" in msg and untouched, (bad, leave, msg)
    # p + intercept = the rows outside fold 1: refused, naming the fold; one more row: fitted
    x, Y = data(40, 20, 2, 57, k=2)
    for kept, ok in ((21, False), (22, True)):
        fid = np.resize(np.arange(2, 4), 40)
        fid[: 40 - kept] = 1
        fid[40 - kept:] = np.resize(np.arange(2, 4), kept)
        rc, msg, untouched = _raw_call(oa, _colmajor(x), _dev(Y), _fd(fid), 3, [0, 1, 1], [0, 2, 1])
        if ok:
            assert rc == 0 and not untouched, msg
        else:
            assert rc == ERR_UNSUPPORTED and "fold 1" in msg and untouched, (rc, msg)
    x, Y = data(1100, 1024, 1, 58)
    rc, msg, untouched = _raw_call(oa, _colmajor(x), _dev(Y), _fd(_random_folds(1100, 3, 59)), 3, [0], [1])
    assert rc == ERR_UNSUPPORTED and "1024" in msg and untouched
    # the Python entry's own
    x, Y = data(300, 6, 2, 55)
    xd, Yd = _colmajor(x), _dev(Y)
    fid = _random_folds(300, 4, 56)
    for bad in ([(2, 0)], [(0, 5)], [(0, -1)], []):
        with pytest.raises(ValueError):
            oa.oem_fit_logistic_dense_multi_folds(xd, Yd, fid, instances=bad, penalty="lasso")
    with pytest.raises(ValueError, match="nfolds"):
        oa.oem_fit_logistic_dense_multi_folds(xd, Yd, np.resize([1, 2], 300), penalty="lasso")
    with pytest.raises(ValueError, match="lengths"):
        oa.oem_fit_logistic_dense_multi_folds(xd, Yd, fid[:-1], penalty="lasso")


# ------------------------------------------------------------------------------------------------ (h)
def test_interrupt(oa):
    x, Y = data(800, 10, 2, 60)
    fid = _random_folds(800, 3, 61)
    xd, Yd = _colmajor(x), _dev(Y)
    calls = []

    def fire():
        calls.append(1)
        return len(calls) >= 3

    with pytest.raises(oa.OemgpuError) as e:
        oa.oem_fit_logistic_dense_multi_folds(xd, Yd, fid, penalty="lasso", nlambda=5, interrupt=fire)
    assert e.value.code == ERR_INTERRUPTED and len(calls) == 3          # polled once per lock-step IRLS step
    fits = oa.oem_fit_logistic_dense_multi_folds(xd, Yd, fid, penalty="lasso", nlambda=5)         # the same context serves the next call
    _compare(fits[1][2], _single(oa, xd, Y, _fd(fid), 3, 1, 2, ["lasso"], dict(nlambda=5)), ["lasso"])
