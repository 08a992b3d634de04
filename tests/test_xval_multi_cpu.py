"""xval.oem for many responses on one x (xval_oem_multi, oemgpu_xval_dense_multi_dev / _rm_dev) without a GPU: the host plan swept over
its edges against a restatement of its rules, and every refusal that must come before any device work."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests.multi_restatement import ENGINE_COOP, ENGINE_ROWS, MAX_INSTANCES, coop_workgroups, waiting_workgroups

ERR_ARG, ERR_UNSUPPORTED = -1, -4
PLAN_LEN = 20


@pytest.fixture(scope="module")
def oa():
    import oem_amd
    oem_amd.lib()
    return oem_amd


@pytest.fixture(scope="module")
def api(oa):
    from oem_amd import api
    return api


# ------------------------------------------------------------------------------------------------ the plan
def _r256(b):
    return (b + 255) // 256 * 256


def _instances(q, npen, num_cu):
    """api.hip: multi_solve_plan at q = p + intercept without a group penalty -> (instances one batched launch may hold, engine)"""
    cus = num_cu * 3 // 4
    if 209 <= q <= 1024:                                               # the cooperating engine takes the batch from COOP_MIN_Q on
        cap, engine = cus // coop_workgroups(q), ENGINE_COOP
    elif q <= 208:
        cap, engine = MAX_INSTANCES, ENGINE_ROWS
    else:
        cap, engine = 0, 0
    return (min(cap, MAX_INSTANCES), engine) if cap >= 1 else (1, 0)


PS = [2, 41, 207, 208, 250, 287, 288, 300, 511, 512, 1023, 1024, 1100]


@pytest.mark.parametrize("p", PS)
def test_plan_sweep(oa, api, p):
    lib = oa.lib()
    out = (C.c_int64 * PLAN_LEN)()
    cvp = (C.c_int64 * 7)()
    q = p + 1
    for K, m, npen, num_cu, n, nl in itertools.product((3, 10, 512), (1, 5, 42, 128, 129, 600), (1, 3), (64, 256), (p + 700, 100000), (5, 100)):
        where = (n, p, K, m, npen, nl, num_cu)
        assert lib.oemgpu_selftest_xval_multi_plan(n, p, K, m, npen, nl, num_cu, out) == 0, (where, lib.oemgpu_last_error())
        v = [int(t) for t in out]
        nb, nsolve, engine, route, rows, chunks_max, passes, block, nwg, b_single = v[:10]
        b_col, b_yp, b_cf, b_part, b_comp, b_tab, b_cvpart, b_cvout, total, cap = v[10:]
        # the batched launch: never more than 513 instances, whole responses only
        assert nb >= 1 and nb * (K + 1) <= MAX_INSTANCES, where
        want_cap, want_engine = _instances(q, npen, num_cu)
        assert (cap, engine) == (want_cap, want_engine), where
        # route 1 exactly where no batch engine takes the shape or a launch cannot hold one response's K + 1 fits
        assert route == (1 if (want_engine == 0 or want_cap < K + 1) else 0), where
        assert nb == (min(want_cap // (K + 1), m) if route == 0 else 1), where
        # workgroups that wait for each other: all of a launch within 3/4 of the CUs
        if route == 0:
            assert waiting_workgroups(q, npen, engine, nb * (K + 1), num_cu) <= num_cu * 3 // 4, where
        # the solve chunks cover the responses, none is empty
        assert nsolve * nb >= m and (nsolve - 1) * nb < m, where
        # the X'Y pass: multi_plan's rows and blocks; room for every fold's last, short chunk
        mp = api.multi_plan(n, p, m, npen=npen, layout=0, num_cu=num_cu)
        assert (rows, passes, block) == (mp["rows"], mp["passes"], mp["block"]) and chunks_max == mp["row_chunks"] + K, where
        # the CV-error launch: the CUs divided by K npen nb, within the single-response plan's bound, at least one workgroup
        assert lib.oemgpu_selftest_xval_cv_plan(n, p, K, npen, nl, num_cu, cvp) == 0
        assert nwg == max(1, min(num_cu // (K * npen * nb), int(cvp[6]))), where
        # the bytes are the sum of the buffers
        ldp = (n + 16 * K + 15) // 16 * 16
        nl16 = (nl + 15) // 16 * 16
        want = [8 * n, 8 * ldp * m, 4 * (K + 1), 8 * chunks_max * passes * (p + 2) * block, 8 * nb * (K + 1) * (p + 2) ** 2,
                8 * nb * K * npen * nl * (p + 1), 8 * nb * nwg * K * 8 * npen * nl16 * 4, 8 * nb * 2 * npen * nl]
        assert [b_col, b_yp, b_cf, b_part, b_comp, b_tab, b_cvpart, b_cvout] == want, where
        assert total == b_single + sum(_r256(b) for b in want), where


def test_plan_chunks_of_the_gpu_tests(api):
    """the shapes tests/test_gpu_xval_multi.py relies on: more than one solve chunk at p = 300, route 1 at p = 1,040"""
    a = api.xval_multi_plan(3000, 300, 4, 5, nl=12, num_cu=256)
    assert (a["route"], a["engine"], a["nb"], a["solve_chunks"]) == (0, ENGINE_COOP, 3, 2)
    b = api.xval_multi_plan(1600, 1040, 4, 2, nl=12, num_cu=256)
    assert (b["route"], b["engine"], b["nb"], b["solve_chunks"]) == (1, 0, 1, 2)
    c = api.xval_multi_plan(300, 5, 3, 200, nl=5, num_cu=256)
    assert (c["route"], c["nb"]) == (0, 128)


def test_plan_refuses_bad_arguments(oa):
    lib = oa.lib()
    out = (C.c_int64 * PLAN_LEN)()
    good = [100, 4, 3, 2, 1, 10, 256]
    for k in range(7):
        args = list(good)
        args[k] = 0
        assert lib.oemgpu_selftest_xval_multi_plan(*args, out) == ERR_ARG, k
    assert lib.oemgpu_selftest_xval_multi_plan(100, 4, 1, 2, 1, 10, 256, out) == ERR_ARG          # nfolds outside 2..512
    assert lib.oemgpu_selftest_xval_multi_plan(100, 4, 513, 2, 1, 10, 256, out) == ERR_ARG
    assert lib.oemgpu_selftest_xval_multi_plan(*good, None) == ERR_ARG
    assert lib.oemgpu_selftest_xval_multi_plan(4, 4, 3, 2, 1, 10, 256, out) == ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ refusals before any device
def test_xval_oem_multi_refuses_before_any_device(oa):
    import scipy.sparse as sp
    rng = np.random.default_rng(0)
    n, p, m = 40, 5, 3
    x, Y = rng.normal(size=(n, p)), rng.normal(size=(n, m))
    fid = np.resize(np.arange(1, 5), n)
    cases = [
        (dict(x=x, Y=Y), "one response at a time with xval_oem()"),
        (dict(x=sp.csc_matrix(x), Y=Y), "one response at a time with xval_oem()"),
        (dict(x=x, Y=Y, weights=np.ones(n)), "xval_oem(weights=)"),
        (dict(x=x, Y=Y, ngpus=2), "ngpus / devices"),
        (dict(x=x, Y=Y, devices=[0]), "ngpus / devices"),
        (dict(x=x, Y=Y, family="binomial"), "binomial models not yet supported for xval, use cv.oem() instead"),
        (dict(x=x, Y=Y, family="poisson"), "'arg' should be one of"),
        (dict(x=x, Y=Y, type_measure="rmse"), "'arg' should be one of"),
        (dict(x=x, Y=Y[:, 0]), "Y must be a matrix"),
        (dict(x=x, Y=Y[:, :0]), "at least one column"),
        (dict(x=x, Y=Y[:-1]), "x and y lengths do not match"),
        (dict(x=x, Y=Y, foldid=fid[:-1]), "x and y lengths do not match"),
        (dict(x=rng.normal(size=(5, 5)), Y=Y[:5]), "number of observations must be greater than the number of variables"),
        (dict(x=rng.normal(size=(4, 5)), Y=Y[:4]), "number of observations must be greater than the number of variables"),
        (dict(x=x[:, :1], Y=Y), "x must have at least two columns"),
        (dict(x=x, Y=Y, nfolds=2), "nfolds must be bigger than 3"),
        (dict(x=x, Y=Y, foldid=np.resize(np.arange(1, 3), n)), "nfolds must be bigger than 3"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError) as e:
            oa.xval_oem_multi(kw.pop("x"), kw.pop("Y"), **kw)
        assert what in str(e.value), (what, str(e.value))


def test_xval_oem_multi_refuses_a_sparse_handle(oa, api):
    class Handle(api.SparseX):                                     # (a SparseX without a device: only its type is looked at)
        def __init__(self):
            self._h = None
        shape = (40, 5)
    with pytest.raises(ValueError) as e:
        oa.xval_oem_multi(Handle(), np.zeros((40, 2)))
    assert "one response at a time with xval_oem()" in str(e.value)


CTX, PTR = C.c_void_p(0x1000), C.c_void_p(0x2000)
# (ctx, x, dtype or None for the column-major entry, n, ld, p, y, rs, cs, m, foldid, nfolds, type_measure): the code, what is wrong
C_CASES = [
    ((None, PTR, None, 40, 40, 4, PTR, 3, 1, 3, PTR, 4, 0), ERR_ARG, "NULL ctx"),
    ((CTX, None, None, 40, 40, 4, PTR, 3, 1, 3, PTR, 4, 0), ERR_ARG, "NULL x"),
    ((CTX, PTR, None, 40, 40, 4, None, 3, 1, 3, PTR, 4, 0), ERR_ARG, "NULL y"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 3, 1, 3, None, 4, 0), ERR_ARG, "NULL foldid"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 3, 1, 0, PTR, 4, 0), ERR_ARG, "m < 1"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 2, 1, 3, PTR, 4, 0), ERR_ARG, "row-major Y with rs < m"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 1, 39, 3, PTR, 4, 0), ERR_ARG, "column-major Y with cs < n"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 3, 2, 3, PTR, 4, 0), ERR_ARG, "no unit stride"),
    ((CTX, PTR, None, 40, 39, 4, PTR, 3, 1, 3, PTR, 4, 0), ERR_ARG, "ld < n"),
    ((CTX, PTR, 0, 40, 3, 4, PTR, 3, 1, 3, PTR, 4, 0), ERR_ARG, "ldr < p"),
    ((CTX, PTR, 2, 40, 4, 4, PTR, 3, 1, 3, PTR, 4, 0), ERR_ARG, "a dtype that is none"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 3, 1, 3, PTR, 1, 0), ERR_ARG, "nfolds < 2"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 3, 1, 3, PTR, 513, 0), ERR_ARG, "nfolds > 512"),
    ((CTX, PTR, None, 40, 40, 4, PTR, 3, 1, 3, PTR, 4, 2), ERR_ARG, "type_measure outside {0, 1}"),
    ((CTX, PTR, None, 4, 4, 4, PTR, 3, 1, 3, PTR, 4, 0), ERR_UNSUPPORTED, "n <= p"),
    ((CTX, PTR, 1, 3, 4, 4, PTR, 3, 1, 3, PTR, 3, 0), ERR_UNSUPPORTED, "n <= p, row-major"),
    ((CTX, PTR, None, 6, 6, 4, PTR, 3, 1, 3, PTR, 3, 0), ERR_UNSUPPORTED, "n - largest fold <= p"),
    ((CTX, PTR, 0, 7, 4, 4, PTR, 3, 1, 3, PTR, 3, 0), ERR_UNSUPPORTED, "n - largest fold <= p, row-major"),
]


def _opts(api, p):
    return api._Args(["lasso"], [np.zeros(0)], 5, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(p), np.zeros(0, np.int32),
                     np.zeros(0, np.int32), np.zeros(0))


def _call(lib, args, opts, outs):
    ctx, x, dt, n, ld, p, y, rs, cs, m, fold, K, tm = args
    if dt is None:
        return lib.oemgpu_xval_dense_multi_dev(ctx, x, n, ld, p, y, rs, cs, m, fold, K, 1, 1, tm, opts, *outs)
    return lib.oemgpu_xval_dense_multi_rm_dev(ctx, x, dt, n, ld, p, y, rs, cs, m, fold, K, 1, 1, tm, opts, *outs)


@pytest.mark.parametrize("args,code,what", C_CASES, ids=[c[2] for c in C_CASES])
def test_c_entries_refuse_before_any_device(oa, api, args, code, what):
    from oem_amd import _lib as L
    lib = oa.lib()
    a = _opts(api, args[5])
    outs = [C.cast(PTR, t) for t in (L._dp, L._dp, L._ip, L._dp, L._dp, L._dp, L._dp, L._ip)]
    rc = _call(lib, args, C.byref(a.c), outs)
    assert rc == code, (what, rc, lib.oemgpu_last_error())
    if code == ERR_UNSUPPORTED:
        assert b"dimension of x larger than number of observations" in lib.oemgpu_last_error()


def test_c_entries_refuse_null_outputs_and_options(oa, api):
    from oem_amd import _lib as L
    lib = oa.lib()
    a = _opts(api, 4)
    good = [C.cast(PTR, t) for t in (L._dp, L._dp, L._ip, L._dp, L._dp, L._dp, L._dp, L._ip)]
    args = (CTX, PTR, None, 40, 40, 4, PTR, 3, 1, 3, PTR, 4, 0)
    for k in range(8):
        outs = list(good)
        outs[k] = None
        assert _call(lib, args, C.byref(a.c), outs) == ERR_ARG, k
    assert _call(lib, args, None, good) == ERR_ARG
    # the options go through the checks of every fit entry: no penalty
    b = _opts(api, 4)
    b.c.npen = 0
    assert _call(lib, args, C.byref(b.c), good) == ERR_ARG
    # the fold-moment self-test has the same rules for x, Y and the folds
    assert lib.oemgpu_selftest_xval_multi_fold_moments_dev(CTX, PTR, -1, 40, 40, 4, PTR, 3, 1, 3, PTR, 4, None) == ERR_ARG
    assert lib.oemgpu_selftest_xval_multi_fold_moments_dev(CTX, PTR, -1, 40, 39, 4, PTR, 3, 1, 3, PTR, 4, PTR) == ERR_ARG
    assert lib.oemgpu_selftest_xval_multi_fold_moments_dev(CTX, PTR, 1, 40, 4, 4, PTR, 2, 1, 3, PTR, 4, PTR) == ERR_ARG
    assert lib.oemgpu_selftest_xval_multi_fold_moments_dev(CTX, PTR, 1, 40, 4, 4, PTR, 3, 1, 3, PTR, 1, PTR) == ERR_ARG
    assert lib.oemgpu_last_xval_multi_timings(None) == ERR_ARG
