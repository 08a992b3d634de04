"""Many responses on one x (oem_multi, oemgpu_fit_dense_multi_dev / _rm_dev) without a GPU: the host plan swept over its edges, the numpy
restatement of the composed moment buffer against exact integer sums, and every refusal that must come before any device work."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests.exact_gram import exact_gram
from tests.multi_restatement import ENGINE_COOP, ENGINE_ROWS, MAX_INSTANCES, composed_moments, waiting_workgroups

ERR_ARG, ERR_UNSUPPORTED = -1, -4
RM_P_MAX = 1024


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
PS = [2, 15, 16, 17, 100, 208, 209, 288, 289, 512, 513, 1024, 1025, 4096]
MS = [1, 15, 16, 17, 513, 514, 5000]


@pytest.mark.parametrize("p", PS)
def test_plan_sweep(oa, api, p):
    lib = oa.lib()
    out = (C.c_int64 * 8)()
    for m, npen, n, num_cu, layout in itertools.product(MS, (1, 3), (p + 1, 1003, 10 ** 6), (64, 256), (0, 1)):
        rc = lib.oemgpu_selftest_multi_plan(n, p, m, npen, layout, num_cu, out)
        where = (n, p, m, npen, layout, num_cu)
        if n <= p or (layout == 1 and p > RM_P_MAX):
            assert rc == ERR_UNSUPPORTED, where
            continue
        assert rc == 0, (where, lib.oemgpu_last_error())
        rows, nchunk, block, passes, cap, nsolve, engine, nbytes = [int(v) for v in out]
        # the row chunks cover n exactly: multiples of 4 (of 64) rows, the last one short but not empty
        assert rows % 64 == 0 and rows % 4 == 0 and nchunk >= 1, where
        assert (nchunk - 1) * rows < n <= nchunk * rows, where
        # the response blocks of the X'Y kernel cover m
        assert block in (16, 32, 64) and (passes - 1) * block < m <= passes * block, where
        # the solve chunks cover 0 .. m - 1 once, in order: chunk k is [k cap, min(m, (k + 1) cap))
        assert 1 <= cap <= MAX_INSTANCES and nsolve == -(-m // cap), where
        covered = [r for k in range(nsolve) for r in range(k * cap, min(m, (k + 1) * cap))]
        assert covered == list(range(m)), where
        if p > 1024:
            assert engine == 0 and cap == 1 and nsolve == m, where
        else:
            assert engine in (ENGINE_ROWS, ENGINE_COOP) or cap == 1, where
        # workgroups that wait for each other: all of a launch within 3/4 of the CUs (times npen where the penalties are split)
        assert waiting_workgroups(p, npen, engine, min(cap, m), num_cu) <= num_cu * 3 // 4, where
        if engine == ENGINE_ROWS and p <= 208:
            assert cap == MAX_INSTANCES, where
        # at least the arithmetic sum of its parts: base moments, one response column, chunk partials, the composed buffers of a launch
        q = p + 2
        parts = 8 * (q * q + n + nchunk * passes * q * block + min(cap, m) * q * q)
        assert nbytes >= parts, where


def test_plan_refuses_bad_arguments(oa):
    lib = oa.lib()
    out = (C.c_int64 * 8)()
    for args in ((0, 4, 1, 1, 0, 256), (10, 0, 1, 1, 0, 256), (10, 4, 0, 1, 0, 256), (10, 4, 1, 0, 0, 256), (10, 4, 1, 1, 2, 256), (10, 4, 1, 1, 0, 0)):
        assert lib.oemgpu_selftest_multi_plan(*args, out) == ERR_ARG, args
    assert lib.oemgpu_selftest_multi_plan(10, 4, 1, 1, 0, 256, None) == ERR_ARG
    assert lib.oemgpu_selftest_multi_plan(4, 4, 1, 1, 0, 256, out) == ERR_UNSUPPORTED
    assert b"n <= p" in lib.oemgpu_last_error()


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n,p,m", [(7, 2, 1), (515, 17, 33), (5000, 100, 5)])
def test_restatement_equals_exact_sums(n, p, m):
    rng = np.random.default_rng(n + p + m)
    kx = rng.integers(-32, 33, size=(n, p))
    ky = rng.integers(-32, 33, size=(n, m))
    got = composed_moments(kx / 8.0, ky / 8.0)
    gx = exact_gram(np.concatenate([kx, 8 * np.ones((n, 1), dtype=np.int64)], axis=1))         # [8 x | 8]' [8 x | 8]
    for r in range(m):
        g = exact_gram(np.concatenate([kx, ky[:, r:r + 1], 8 * np.ones((n, 1), dtype=np.int64)], axis=1))
        assert np.array_equal(got[r] * 64.0, g.astype(np.float64)), r
        # ... and what does not depend on the response is the same in every buffer
        keep = [j for j in range(p + 2) if j != p]
        assert np.array_equal(got[r][np.ix_(keep, keep)] * 64.0, gx.astype(np.float64))
        assert np.array_equal(got[r][np.ix_(keep, keep)], got[0][np.ix_(keep, keep)])
        assert np.array_equal(got[r], got[r].T)


# ------------------------------------------------------------------------------------------------ refusals before any device
def test_oem_multi_refuses_before_any_device(oa):
    import scipy.sparse as sp
    rng = np.random.default_rng(0)
    n, p, m = 40, 5, 3
    x, Y = rng.normal(size=(n, p)), rng.normal(size=(n, m))
    cases = [
        (dict(x=x, Y=Y[:, 0]), "Y must be a matrix"),
        (dict(x=x, Y=Y[:-1]), "x and y lengths do not match"),
        (dict(x=x, Y=Y[:, :0]), "at least one column"),
        (dict(x=rng.normal(size=(4, 5)), Y=Y[:4]), "oem(x, Y[:, r])"),
        (dict(x=x, Y=Y), "dense torch tensor on a GPU"),
        (dict(x=sp.csc_matrix(x), Y=Y), "dense torch tensor on a GPU"),
        (dict(x=x, Y=Y, weights=np.ones(n)), "weights not implemented yet."),
        (dict(x=x, Y=Y, ngpus=2), "ngpus / devices"),
        (dict(x=x, Y=Y, devices=[0]), "ngpus / devices"),
        (dict(x=x, Y=Y, family="binomial"), "binomial"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError) as e:
            oa.oem_multi(kw.pop("x"), kw.pop("Y"), **kw)
        assert what in str(e.value), (what, str(e.value))


def test_oem_multi_refuses_a_closed_or_open_sparse_handle(oa, api):
    class Handle(api.SparseX):                                     # (a SparseX without a device: only its type is looked at)
        def __init__(self):
            self._h = None
        shape = (40, 5)
    with pytest.raises(ValueError) as e:
        oa.oem_multi(Handle(), np.zeros((40, 2)))
    assert "dense torch tensor on a GPU" in str(e.value)


CTX, PTR = C.c_void_p(0x1000), C.c_void_p(0x2000)
# (ctx, x, dtype or None for the column-major entry, n, ld, p, y, rs, cs, m): the code, what is wrong
C_CASES = [
    ((None, PTR, None, 10, 10, 4, PTR, 3, 1, 3), ERR_ARG, "NULL ctx"),
    ((CTX, None, None, 10, 10, 4, PTR, 3, 1, 3), ERR_ARG, "NULL x"),
    ((CTX, PTR, None, 10, 10, 4, None, 3, 1, 3), ERR_ARG, "NULL y"),
    ((CTX, PTR, None, 10, 10, 4, PTR, 3, 1, 0), ERR_ARG, "m < 1"),
    ((CTX, PTR, None, 10, 10, 4, PTR, 2, 1, 3), ERR_ARG, "row-major Y with rs < m"),
    ((CTX, PTR, None, 10, 10, 4, PTR, 1, 9, 3), ERR_ARG, "column-major Y with cs < n"),
    ((CTX, PTR, None, 10, 10, 4, PTR, 3, 2, 3), ERR_ARG, "no unit stride"),
    ((CTX, PTR, None, 10, 9, 4, PTR, 3, 1, 3), ERR_ARG, "ld < n"),
    ((CTX, PTR, 0, 10, 3, 4, PTR, 3, 1, 3), ERR_ARG, "ldr < p"),
    ((CTX, PTR, 2, 10, 4, 4, PTR, 3, 1, 3), ERR_ARG, "a dtype that is none"),
    ((CTX, PTR, -1, 10, 4, 4, PTR, 3, 1, 3), ERR_ARG, "a negative dtype"),
    ((CTX, PTR, None, 4, 4, 4, PTR, 3, 1, 3), ERR_UNSUPPORTED, "n <= p"),
    ((CTX, PTR, 1, 3, 4, 4, PTR, 3, 1, 3), ERR_UNSUPPORTED, "n <= p, row-major"),
]


@pytest.mark.parametrize("args,code,what", C_CASES, ids=[c[2] for c in C_CASES])
def test_c_entries_refuse_before_any_device(oa, api, args, code, what):
    lib = oa.lib()
    ctx, x, dt, n, ld, p, y, rs, cs, m = args
    a = api._Args(["lasso"], [np.zeros(0)], 5, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(p), np.zeros(0, np.int32),
                  np.zeros(0, np.int32), np.zeros(0))
    mm = max(m, 1)
    beta, lam, loss, d = np.zeros((mm, 1, 5, p + 1)), np.zeros((mm, 5)), np.zeros((mm, 5)), np.zeros(mm)
    niter, route = np.zeros((mm, 5), np.int32), np.zeros(mm, np.int32)
    outs = [api._dptr(beta), api._dptr(lam), api._iptr(niter), api._dptr(loss), api._dptr(d), api._iptr(route)]
    if dt is None:
        rc = lib.oemgpu_fit_dense_multi_dev(ctx, x, n, ld, p, y, rs, cs, m, 1, 1, C.byref(a.c), *outs)
    else:
        rc = lib.oemgpu_fit_dense_multi_rm_dev(ctx, x, dt, n, ld, p, y, rs, cs, m, 1, 1, C.byref(a.c), *outs)
    assert rc == code, (what, rc, lib.oemgpu_last_error())
    if code == ERR_UNSUPPORTED:
        assert b"n <= p" in lib.oemgpu_last_error() and b"oemgpu_fit_dense_dev" in lib.oemgpu_last_error()
    # the moments self-test has the same rules for x and Y (n <= p is fine there, but needs a device)
    if code == ERR_ARG:
        assert lib.oemgpu_selftest_multi_moments_dev(ctx, x, -1 if dt is None else (7 if dt < 0 else dt), n, ld, p, y, rs, cs, m, PTR) == ERR_ARG, what


def test_row_major_entry_refuses_p_beyond_its_pass_by_name(oa, api):
    from oem_amd import _lib as L
    lib = oa.lib()
    p = L.RM_P_MAX + 1
    a = api._Args(["lasso"], [np.zeros(0)], 5, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(p), np.zeros(0, np.int32),
                  np.zeros(0, np.int32), np.zeros(0))
    outs = [C.cast(PTR, t) for t in (L._dp, L._dp, L._ip, L._dp, L._dp, L._ip)]
    assert lib.oemgpu_fit_dense_multi_rm_dev(CTX, PTR, 1, 10 * p, p, p, PTR, 3, 1, 3, 1, 1, C.byref(a.c), *outs) == ERR_UNSUPPORTED
    assert b"column-major entry" in lib.oemgpu_last_error()
    assert lib.oemgpu_selftest_multi_moments_dev(CTX, PTR, 1, 10 * p, p, p, PTR, 3, 1, 3, PTR) == ERR_UNSUPPORTED


def test_c_entries_refuse_null_outputs_and_options(oa, api):
    lib = oa.lib()
    a = api._Args(["lasso"], [np.zeros(0)], 5, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(4), np.zeros(0, np.int32),
                  np.zeros(0, np.int32), np.zeros(0))
    from oem_amd import _lib as L
    good = [C.cast(PTR, t) for t in (L._dp, L._dp, L._ip, L._dp, L._dp, L._ip)]
    for k in range(6):
        outs = list(good)
        outs[k] = None
        assert lib.oemgpu_fit_dense_multi_dev(CTX, PTR, 10, 10, 4, PTR, 3, 1, 3, 1, 1, C.byref(a.c), *outs) == ERR_ARG, k
    assert lib.oemgpu_fit_dense_multi_dev(CTX, PTR, 10, 10, 4, PTR, 3, 1, 3, 1, 1, None, *good) == ERR_ARG
    assert lib.oemgpu_selftest_multi_moments_dev(CTX, PTR, -1, 10, 10, 4, PTR, 3, 1, 3, None) == ERR_ARG
