"""Many binomial responses on one x (oem_fit_logistic_dense_multi, oemgpu_fit_logistic_dense_multi_dev / _rm_dev) without a GPU: the
numpy restatement of the lock-step driver against the single-response restatement (to the byte), the host plan swept over its
edges, and every refusal that must come before any device work."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import logistic_restatement as R
from tests.logistic_multi_restatement import data, fit_multi

ERR_ARG, ERR_UNSUPPORTED = -1, -4
KW = dict(nlambda=12, tol=1e-9, irls_tol=1e-5, compute_loss=True)
PENS = ["lasso", "mcp"]


@pytest.fixture(scope="module")
def oa():
    import oem_amd
    oem_amd.lib()
    return oem_amd


@pytest.fixture(scope="module")
def api(oa):
    from oem_amd import api
    return api


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n,p,m,seed", [(3000, 24, 4, 11), (2000, 17, 5, 12)])
def test_lockstep_restatement_equals_the_single_fits(n, p, m, seed):
    x, Y = data(n, p, m, seed)
    st = {}
    got = fit_multi(x, Y, penalty=PENS, stats=st, **KW)
    refs = [R.fit(x, Y[:, r], penalty=PENS, **KW) for r in range(m)]
    for r in range(m):
        for k in range(len(PENS)):
            assert np.array_equal(got[r]["beta"][k], refs[r]["beta"][k]), (r, k)
            assert np.array_equal(got[r]["niter"][k], refs[r]["niter"][k]), (r, k)
            assert np.array_equal(got[r]["loss"][k], refs[r]["loss"][k]), (r, k)
            assert np.array_equal(got[r]["lambda"][k], refs[r]["lambda"][k]), (r, k)
        assert got[r]["d"] == refs[r]["d"], r
    # the data must exercise the freeze: the responses stop at different steps at more than half of the (penalty, lambda) cells
    ni = np.array([[refs[r]["niter"][k] for k in range(len(PENS))] for r in range(m)])          # [m, npen, nl]
    differing = int(np.sum(ni.max(axis=0) != ni.min(axis=0)))
    print("cells with differing niter:", differing, "of", ni.shape[1] * ni.shape[2])
    assert differing > ni.shape[1] * ni.shape[2] // 2, differing
    # the lock-step counts: a step per max niter, a row pass per step but the skipped first of a later lambda, one Gram build
    steps = int(np.minimum(ni, 100).max(axis=0).sum())
    assert st["steps"] == steps and st["rows"] == steps - len(PENS) * (KW["nlambda"] - 1) and st["grams"] == 1


def test_lockstep_restatement_on_every_penalty_and_option():
    x, Y = data(600, 12, 3, 13)
    groups = np.concatenate([[0], np.repeat(np.arange(1, 4), 4)])
    kw = dict(penalty=list(R.PENALTIES), groups=groups, unique_groups=np.unique(groups), nlambda=5, alpha=0.6, gamma=3.7, tau=0.4, compute_loss=True)
    got = fit_multi(x, Y, **kw)
    for r in range(3):
        ref = R.fit(x, Y[:, r], **kw)
        for k in range(len(R.PENALTIES)):
            assert np.array_equal(got[r]["beta"][k], ref["beta"][k]) and np.array_equal(got[r]["niter"][k], ref["niter"][k]), (r, k)
    lam = [np.array([0.1, 0.05, 0.01])]
    for kw in (dict(intercept=False), dict(standardize=False), dict(lambda_=lam)):
        got = fit_multi(x, Y, **kw, nlambda=4)
        for r in range(3):
            ref = R.fit(x, Y[:, r], **kw, nlambda=4)
            assert np.array_equal(got[r]["beta"][0], ref["beta"][0]) and np.array_equal(got[r]["lambda"][0], ref["lambda"][0]), (kw, r)


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("p", [2, 3, 15, 16, 17, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024])
def test_plan_sweep(oa, api, p):
    for n, m, layout, num_cu, icpt in itertools.product((p + 2, 1003, 10 ** 6), (1, 15, 16, 17, 33, 64, 65, 200), (0, 1), (64, 256), (0, 1)):
        where = (n, p, m, layout, num_cu, icpt)
        if p + icpt > 1024:
            with pytest.raises(oa.OemgpuError) as e:
                api.logistic_multi_plan(n, p, m, icpt, layout, num_cu)
            assert e.value.code == ERR_UNSUPPORTED, where
            continue
        pl = api.logistic_multi_plan(n, p, m, icpt, layout, num_cu)
        # the row chunks cover [0, n) once: multiples of 64 rows, the last one short but not empty; n and the CU count alone decide
        assert pl["rows"] % 64 == 0 and (pl["row_chunks"] - 1) * pl["rows"] < n <= pl["row_chunks"] * pl["rows"], where
        assert pl["rows"] == api.logistic_multi_plan(n, p, 1, icpt, layout, num_cu)["rows"], where
        # MCH responses at a time, their blocks cover the widest chunk once
        mch = min(m, pl["mch"])
        assert pl["mch"] == 64 and pl["response_chunks"] == -(-m // 64), where
        assert pl["block"] == 16 * pl["lt"] and pl["lt"] in (1, 2, 4), where
        assert (pl["blocks"] - 1) * pl["block"] < mch <= pl["blocks"] * pl["block"], where
        # the column band covers p; a wave's Bt slice and accumulators stay within 128 doubles each
        assert pl["band"] == 64 * pl["tiles_per_wave"] and pl["band"] >= p and (pl["band"] == 128 or pl["band"] // 2 < p), where
        assert pl["tiles_per_wave"] * pl["lt"] <= 16, where
        assert pl["lds_bytes"] <= 160 * 1024, where
        assert pl["panel_bytes"] == 8 * pl["row_chunks"] * pl["blocks"] * (p + 2) * pl["block"], where
        assert pl["bytes"] == pl["panel_bytes"] + pl["shared_bytes"] + pl["chunk_bytes"] + pl["hessian_bytes"], where
        assert pl["a_in_lds"] == int(p + icpt <= 110), where


def test_plan_refuses_bad_arguments(oa):
    lib = oa.lib()
    out = (C.c_int64 * 16)()
    for args in ((0, 4, 1, 1, 0, 256), (10, 0, 1, 1, 0, 256), (10, 4, 0, 1, 0, 256), (10, 4, 1, 1, 2, 256), (10, 4, 1, 1, 0, 0)):
        assert lib.oemgpu_selftest_logistic_multi_plan(*args, out) == ERR_ARG, args
    assert lib.oemgpu_selftest_logistic_multi_plan(10, 4, 1, 1, 0, 256, None) == ERR_ARG


# ------------------------------------------------------------------------------------------------ refusals before any device
def test_python_refuses_before_any_device(oa, api, monkeypatch):
    import scipy.sparse as sp
    import torch

    def no_cpu(self, *a, **k):
        raise AssertionError("a refused call copied a tensor to the host")
    monkeypatch.setattr(torch.Tensor, "cpu", no_cpu)
    rng = np.random.default_rng(0)
    n, p, m = 40, 5, 3
    x = rng.normal(size=(n, p))
    Y = (rng.uniform(size=(n, m)) < 0.5).astype(np.float64)
    Y3 = Y.copy()
    Y3[:3, 1] = [0.0, 1.0, 2.0]

    class Handle(api.SparseX):                                     # (a SparseX without a device: only its type is looked at)
        def __init__(self):
            self._h = None
        shape = (n, p)
    cases = [
        (dict(x=x, Y=Y[:, 0]), "Y must be a matrix"),
        (dict(x=x, Y=Y[:-1]), "x and y lengths do not match"),
        (dict(x=x, Y=Y[:, :0]), "at least one column"),
        (dict(x=x, Y=Y3), "column 1 of Y takes more than two values"),
        (dict(x=x, Y=torch.as_tensor(Y3)), "column 1 of Y takes more than two values"),
        (dict(x=x, Y=Y, hessian_type="full"), "fit each column with oem_fit_logistic_dense"),
        (dict(x=rng.normal(size=(1100, 1024)), Y=np.zeros((1100, 2))), "p + intercept <= 1024"),
        (dict(x=x, Y=Y), "takes a dense torch tensor on a GPU: "),
        (dict(x=torch.as_tensor(x), Y=Y), "takes a dense torch tensor on a GPU: "),
        (dict(x=sp.csc_matrix(x), Y=Y), "takes a dense torch tensor on a GPU: "),
        (dict(x=Handle(), Y=Y), "takes a dense torch tensor on a GPU: "),
        (dict(x=x, Y=Y, hessian_type="exact"), "'upper.bound', 'full'"),
        (dict(x=x[:, :1], Y=Y), "at least two columns"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError) as e:
            oa.oem_fit_logistic_dense_multi(kw.pop("x"), kw.pop("Y"), **kw)
        assert what in str(e.value), (what, str(e.value))
    # p = 1024 without an intercept is q = 1024: served (refused only for being on the host)
    with pytest.raises(ValueError) as e:
        oa.oem_fit_logistic_dense_multi(np.zeros((1100, 1024)), np.zeros((1100, 2)), intercept=False)
    assert "dense torch tensor on a GPU" in str(e.value)
    # weights: oem_fit_logistic_dense's own error and sentence
    with pytest.raises(oa.OemgpuError) as e:
        oa.oem_fit_logistic_dense_multi(x, Y, weights=np.ones(n))
    assert e.value.code == ERR_UNSUPPORTED and "weights not implemented yet." in str(e.value)
    with pytest.raises(oa.OemgpuError) as e1:
        oa.oem_fit_logistic_dense(x, Y[:, 0], weights=np.ones(n))
    assert str(e1.value) == str(e.value)
    # the entries above it keep their sentences
    with pytest.raises(ValueError) as e:
        oa.oem_multi(x, Y, family="binomial")
    assert "outside the dense Gaussian hot path" in str(e.value)


CTX, PTR = C.c_void_p(0x1000), C.c_void_p(0x2000)
# (ctx, x, dtype or None for the column-major entry, n, ld, p, y, rs, cs, m, intercept, hessian_full): the code, a piece of the sentence
C_CASES = [
    ((None, PTR, None, 100, 100, 4, PTR, 3, 1, 3, 1, 0), ERR_ARG, b"NULL argument", "NULL ctx"),
    ((CTX, None, None, 100, 100, 4, PTR, 3, 1, 3, 1, 0), ERR_ARG, b"NULL argument", "NULL x"),
    ((CTX, PTR, None, 100, 100, 4, None, 3, 1, 3, 1, 0), ERR_ARG, b"NULL argument", "NULL Y"),
    ((CTX, PTR, None, 100, 100, 4, PTR, 3, 1, 0, 1, 0), ERR_ARG, b"m < 1", "m < 1"),
    ((CTX, PTR, None, 100, 100, 4, PTR, 2, 1, 3, 1, 0), ERR_ARG, b"y strides", "row-major Y with rs < m"),
    ((CTX, PTR, None, 100, 100, 4, PTR, 1, 99, 3, 1, 0), ERR_ARG, b"y strides", "column-major Y with cs < n"),
    ((CTX, PTR, None, 100, 100, 4, PTR, 3, 2, 3, 1, 0), ERR_ARG, b"y strides", "no unit stride"),
    ((CTX, PTR, None, 100, 99, 4, PTR, 3, 1, 3, 1, 0), ERR_ARG, b"", "ld < n"),
    ((CTX, PTR, 0, 100, 3, 4, PTR, 3, 1, 3, 1, 0), ERR_ARG, b"", "ldr < p"),
    ((CTX, PTR, 2, 100, 4, 4, PTR, 3, 1, 3, 1, 0), ERR_ARG, b"", "a dtype that is none"),
    ((CTX, PTR, -1, 100, 4, 4, PTR, 3, 1, 3, 1, 0), ERR_ARG, b"", "a negative dtype"),
    ((CTX, PTR, None, 100, 100, 4, PTR, 3, 1, 3, 1, 1), ERR_UNSUPPORTED, b"a full Hessian is one per response and step: fit each column with fit_logistic_dense",
     "hessian_full"),
    ((CTX, PTR, 1, 100, 4, 4, PTR, 3, 1, 3, 1, 1), ERR_UNSUPPORTED, b"a full Hessian is one per response and step", "hessian_full, row-major"),
    ((CTX, PTR, None, 100, 100, 4, PTR, 3, 1, 3, 1, 2), ERR_ARG, b"hessian.type", "hessian_full = 2"),
    ((CTX, PTR, None, 5000, 5000, 1024, PTR, 3, 1, 3, 1, 0), ERR_UNSUPPORTED, b"p + intercept > 1024", "q = 1025"),
    ((CTX, PTR, 0, 5000, 1025, 1025, PTR, 3, 1, 3, 0, 0), ERR_UNSUPPORTED, b"p + intercept > 1024", "q = 1025 without an intercept"),
    ((CTX, PTR, None, 5, 5, 4, PTR, 3, 1, 3, 1, 0), ERR_UNSUPPORTED, b"p + intercept >= n is not supported", "q >= n"),
    ((CTX, PTR, 1, 4, 4, 4, PTR, 3, 1, 3, 0, 0), ERR_UNSUPPORTED, b"p + intercept >= n is not supported", "q >= n, row-major"),
]


@pytest.mark.parametrize("args,code,piece,what", C_CASES, ids=[c[3] for c in C_CASES])
def test_c_entries_refuse_before_any_device(oa, api, args, code, piece, what):
    """fake non-NULL pointers: a refusal that dereferenced one of them would not return"""
    lib = oa.lib()
    ctx, x, dt, n, ld, p, y, rs, cs, m, icpt, hf = args
    a = api._Args(["lasso"], [np.zeros(0)], 5, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(p), np.zeros(0, np.int32),
                  np.zeros(0, np.int32), np.zeros(0))
    from oem_amd import _lib as L
    outs = [C.cast(PTR, t) for t in (L._dp, L._dp, L._ip, L._dp, L._dp)]
    tail = (y, rs, cs, m, 1, icpt, hf, 100, 1e-3, C.byref(a.c), *outs)
    if dt is None:
        rc = lib.oemgpu_fit_logistic_dense_multi_dev(ctx, x, n, ld, p, *tail)
    else:
        rc = lib.oemgpu_fit_logistic_dense_multi_rm_dev(ctx, x, dt, n, ld, p, *tail)
    assert rc == code, (what, rc, lib.oemgpu_last_error())
    assert piece in lib.oemgpu_last_error(), (what, lib.oemgpu_last_error())
    # the row-pass self-test has the same rules for x and Y
    if code == ERR_ARG and hf == 0:
        assert lib.oemgpu_selftest_logistic_multi_rows_dev(ctx, x, -1 if dt is None else (7 if dt < 0 else dt), n, ld, p, y, rs, cs, m, PTR, icpt, 1,
                                                           None, PTR) == ERR_ARG, what


def test_c_entries_refuse_null_outputs_options_and_bad_irls(oa, api):
    lib = oa.lib()
    from oem_amd import _lib as L
    a = api._Args(["lasso"], [np.zeros(0)], 5, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(4), np.zeros(0, np.int32),
                  np.zeros(0, np.int32), np.zeros(0))
    good = [C.cast(PTR, t) for t in (L._dp, L._dp, L._ip, L._dp, L._dp)]
    head = (CTX, PTR, 100, 100, 4, PTR, 3, 1, 3, 1, 1, 0)
    for k in range(5):
        outs = list(good)
        outs[k] = None
        assert lib.oemgpu_fit_logistic_dense_multi_dev(*head, 100, 1e-3, C.byref(a.c), *outs) == ERR_ARG, k
    assert lib.oemgpu_fit_logistic_dense_multi_dev(*head, 100, 1e-3, None, *good) == ERR_ARG
    assert lib.oemgpu_fit_logistic_dense_multi_dev(*head, 0, 1e-3, C.byref(a.c), *good) == ERR_ARG
    assert b"irls.maxit should be positive" in lib.oemgpu_last_error()
    assert lib.oemgpu_fit_logistic_dense_multi_dev(*head, 100, -1.0, C.byref(a.c), *good) == ERR_ARG
    assert lib.oemgpu_selftest_logistic_multi_rows_dev(CTX, PTR, -1, 100, 100, 4, PTR, 3, 1, 3, None, 1, 1, None, PTR) == ERR_ARG     # mode 1 needs Bt
    assert lib.oemgpu_selftest_logistic_multi_rows_dev(CTX, PTR, -1, 100, 100, 4, PTR, 3, 1, 3, PTR, 1, 2, None, PTR) == ERR_ARG
    assert lib.oemgpu_selftest_logistic_multi_rows_dev(CTX, PTR, -1, 100, 100, 4, PTR, 3, 1, 3, PTR, 1, 1, None, None) == ERR_ARG
    assert lib.oemgpu_last_logistic_multi_stats(None) == ERR_ARG


def test_the_new_entry_is_exported(oa):
    assert "oem_fit_logistic_dense_multi" in oa.__all__ and callable(oa.oem_fit_logistic_dense_multi)
    assert callable(oa.logistic_multi_stats) and callable(oa.logistic_multi_plan)
