"""The fold fits and the cross-validation of many binomial responses (oem_fit_logistic_dense_multi_folds, cv_oem_logistic_multi,
oemgpu_fit_logistic_dense_multi_fold_dev / _rm_dev) without a GPU: every Python refusal before a device is looked for,
the C entries' refusals on fake pointers, the workspace plan against a restatement, and the header, the bindings and EXPORTS in step."""
import ctypes as C
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

ERR_ARG, ERR_UNSUPPORTED = -1, -4
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def oa():
    import oem_amd
    oem_amd.lib()
    return oem_amd


@pytest.fixture(scope="module")
def api(oa):
    from oem_amd import api
    return api


@pytest.fixture()
def no_device(api, monkeypatch):
    """a refusal that asked for a context, loaded the library or copied a tensor would raise this instead of its own sentence"""
    import torch
    from oem_amd import _lib as L

    def boom(*a, **k):
        raise AssertionError("a refused call looked for a device")
    monkeypatch.setattr(api, "context", boom)
    monkeypatch.setattr(L, "lib", boom)
    monkeypatch.setattr(L, "sync_switches", lambda: None)
    monkeypatch.setattr(torch.Tensor, "cpu", boom)
    monkeypatch.setattr(torch.Tensor, "cuda", boom)


class _FakeCuda:
    """what the checks look at of a dense device tensor, without a device: any use beyond its shape raises"""
    ndim, is_cuda, is_sparse, layout = 2, True, False, None

    def __init__(self, n, p):
        self.shape = (n, p)

    def __getattr__(self, k):
        raise AssertionError(f"a refused call touched x.{k}")


def _inputs():
    rng = np.random.default_rng(0)
    n, p, m = 60, 5, 3
    x = rng.normal(size=(n, p))
    Y = (rng.uniform(size=(n, m)) < 0.5).astype(np.float64)
    return n, p, m, x, Y, np.resize(np.arange(1, 5), n)


def test_fold_fits_refuse_before_any_device(oa, api, no_device, monkeypatch):
    import scipy.sparse as sp
    import torch
    n, p, m, x, Y, fid = _inputs()
    monkeypatch.setattr(api, "_is_torch_cuda", lambda t: isinstance(t, _FakeCuda))
    xd = _FakeCuda(n, p)
    Y3 = Y.copy()
    Y3[:3, 1] = [0.0, 1.0, 2.0]
    cases = [
        (dict(x=x, Y=Y[:, 0]), "Y must be a matrix"),
        (dict(x=x, Y=Y[:-1]), "x and y lengths do not match"),
        (dict(x=x, Y=Y3), "column 1 of Y takes more than two values"),
        (dict(x=x, Y=Y, hessian_type="full"), "fit each column with oem_fit_logistic_dense"),
        (dict(x=np.zeros((1100, 1024)), Y=np.zeros((1100, 2)), foldid=np.resize(np.arange(1, 5), 1100)), "p + intercept <= 1024"),
        (dict(x=x, Y=Y), "oem_fit_logistic_dense_multi_folds() takes a dense torch tensor on a GPU: "),
        (dict(x=torch.as_tensor(x), Y=Y), "takes a dense torch tensor on a GPU: "),
        (dict(x=sp.csc_matrix(x), Y=Y), "takes a dense torch tensor on a GPU: "),
        (dict(x=x[:, :1], Y=Y), "at least two columns"),
        # the fold ones, on an x that passes for a device tensor
        (dict(x=xd, Y=Y, foldid=fid[:-1]), "x and y lengths do not match"),
        (dict(x=xd, Y=Y, foldid=np.resize([1, 2], n)), "nfolds must be bigger than 3"),
        (dict(x=xd, Y=Y, instances=[(3, 0)]), "the response must be in [0, 3)"),
        (dict(x=xd, Y=Y, instances=[(-1, 0)]), "the response must be in"),
        (dict(x=xd, Y=Y, instances=[(0, 5)]), "the fold left out must be in [0, 4]"),
        (dict(x=xd, Y=Y, instances=[(0, -1)]), "the fold left out must be in"),
        (dict(x=xd, Y=Y, instances=[]), "at least one"),
    ]
    for kw, what in cases:
        kw.setdefault("foldid", fid)
        with pytest.raises(ValueError) as e:
            oa.oem_fit_logistic_dense_multi_folds(kw.pop("x"), kw.pop("Y"), kw.pop("foldid"), **kw)
        assert what in str(e.value), (what, str(e.value))
    with pytest.raises(oa.OemgpuError) as e:
        oa.oem_fit_logistic_dense_multi_folds(x, Y, fid, weights=np.ones(n))
    assert e.value.code == ERR_UNSUPPORTED and "weights not implemented yet." in str(e.value)


def test_cv_refuses_before_any_device(oa, api, no_device, monkeypatch):
    import scipy.sparse as sp
    import torch
    n, p, m, x, Y, fid = _inputs()
    monkeypatch.setattr(api, "_is_torch_cuda", lambda t: isinstance(t, _FakeCuda))
    xd = _FakeCuda(n, p)
    cases = [
        (dict(x=xd, Y=Y, hessian_type="full"), "hessian_type='full'"),
        (dict(x=xd, Y=Y, weights=np.ones(n)), "weights not implemented yet."),
        (dict(x=x, Y=Y), "cv_oem_logistic_multi() takes a dense torch tensor on a GPU"),
        (dict(x=torch.as_tensor(x), Y=Y), "takes a dense torch tensor on a GPU"),
        (dict(x=sp.csr_matrix(x), Y=Y), "takes a dense torch tensor on a GPU"),
        (dict(x=xd, Y=Y, ngpus=2), "ngpus / devices"),
        (dict(x=xd, Y=Y, devices=[0]), "ngpus / devices"),
        (dict(x=_FakeCuda(1100, 1024), Y=np.zeros((1100, 2))), "p + intercept <= 1024"),
        (dict(x=xd, Y=Y, lambda_=[0.1]), "Need more than one value of lambda"),
        (dict(x=xd, Y=Y, nfolds=2), "nfolds must be bigger than 3"),
        (dict(x=xd, Y=Y, foldid=np.resize([1, 2], n)), "nfolds must be bigger than 3"),
        (dict(x=xd, Y=Y, type_measure="r2"), "'arg' should be one of"),
        (dict(x=xd, Y=Y[:, 0]), "Y must be a matrix"),
        (dict(x=xd, Y=Y[:-1]), "x and y lengths do not match"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError) as e:
            oa.cv_oem_logistic_multi(kw.pop("x"), kw.pop("Y"), penalty="lasso", **kw)
        assert what in str(e.value), (what, str(e.value))


# ------------------------------------------------------------------------------------------------ the C entries, on fake pointers
CTX, PTR = C.c_void_p(0x1000), C.c_void_p(0x2000)


def _c_call(oa, api, rm, n=100, p=4, m=3, fold=PTR, nfolds=4, resp=(0, 1), leave=(0, 1), icpt=1, hf=0, nobs=True, ninst=None):
    from oem_amd import _lib as L
    lib = oa.lib()
    a = api._Args(["lasso"], [np.zeros(0)], 5, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(p), np.zeros(0, np.int32),
                  np.zeros(0, np.int32), np.zeros(0))
    outs = [C.cast(PTR, t) for t in (L._dp, L._dp, L._ip, L._dp, L._dp)]
    r = None if resp is None else np.ascontiguousarray(resp, dtype=np.int32)
    lv = None if leave is None else np.ascontiguousarray(leave, dtype=np.int32)
    ni = (len(r) if r is not None else 1) if ninst is None else ninst
    tail = (PTR, m, 1, m, fold, nfolds, ni, api._iptr(r), api._iptr(lv), 1, icpt, hf, 100, 1e-3, C.byref(a.c), *outs,
            C.cast(PTR, C.POINTER(C.c_int64)) if nobs else None)
    rc = lib.oemgpu_fit_logistic_dense_multi_fold_rm_dev(CTX, PTR, 0, n, p, p, *tail) if rm else lib.oemgpu_fit_logistic_dense_multi_fold_dev(CTX, PTR, n, n, p, *tail)
    return rc, lib.oemgpu_last_error()


@pytest.mark.parametrize("rm", [False, True])
def test_c_entries_refuse_before_any_device(oa, api, rm):
    """fake non-NULL pointers: a refusal that dereferenced one of them would not return"""
    for kw, code, piece in [(dict(fold=None), ERR_ARG, b"NULL argument"), (dict(resp=None), ERR_ARG, b"NULL argument"),
                            (dict(leave=None), ERR_ARG, b"NULL argument"), (dict(nobs=False), ERR_ARG, b"NULL argument"),
                            (dict(nfolds=2), ERR_ARG, b"nfolds must be bigger than 3; nfolds=10 recommended"),
                            (dict(ninst=0), ERR_ARG, b"ninst must be at least 1"), (dict(ninst=-3), ERR_ARG, b"ninst"),
                            (dict(leave=(0, 5)), ERR_ARG, b"leave_out must be in [0, nfolds]"), (dict(leave=(-1, 0)), ERR_ARG, b"leave_out"),
                            (dict(resp=(0, 3)), ERR_ARG, b"resp must be in [0, m)"), (dict(resp=(-1, 0)), ERR_ARG, b"resp"),
                            (dict(m=0), ERR_ARG, b"m < 1"),
                            (dict(hf=1), ERR_UNSUPPORTED, b"a full Hessian is one per response and step"),
                            (dict(hf=2), ERR_ARG, b"hessian.type"),
                            (dict(n=5000, p=1024), ERR_UNSUPPORTED, b"p + intercept > 1024"),
                            (dict(n=5), ERR_UNSUPPORTED, b"p + intercept >= n is not supported")]:
        rc, msg = _c_call(oa, api, rm, **kw)
        assert rc == code and piece in msg, (kw, rc, msg)
    lib = oa.lib()
    assert lib.oemgpu_selftest_logistic_multi_rows_fold_dev(CTX, PTR, -1, 100, 100, 4, PTR, 3, 1, 3, None, 3, None, None, PTR, 1, 1, None, PTR) == ERR_ARG
    lv = np.zeros(3, dtype=np.int32)
    assert lib.oemgpu_selftest_logistic_multi_rows_fold_dev(CTX, PTR, -1, 100, 100, 4, PTR, 3, 1, 3, PTR, 2, api._iptr(lv), None, PTR, 1, 1, None, PTR) == ERR_ARG
    assert lib.oemgpu_selftest_logistic_multi_rows_fold_dev(CTX, PTR, -1, 100, 100, 4, PTR, 3, 1, 3, PTR, 3, api._iptr(lv), None, None, 1, 1, None, PTR) == ERR_ARG
    yc = np.array([0, 3, 1], dtype=np.int32)
    assert lib.oemgpu_selftest_logistic_multi_rows_fold_dev(CTX, PTR, -1, 100, 100, 4, PTR, 3, 1, 3, PTR, 3, api._iptr(lv), api._iptr(yc), PTR, 1, 1, None,
                                                            PTR) == ERR_ARG


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("p", [2, 17, 109, 110, 129, 513, 1023, 1024])
def test_fold_plan_against_a_restatement(oa, api, p):
    PENK = 40                                                            # sizeof(PenK): an int (padded) and four doubles
    for n, ninst, G, layout, num_cu, icpt in itertools.product((p + 5, 1003, 10 ** 6), (1, 11, 64, 65, 176), (1, 4, 11), (0, 1), (64, 256), (0, 1)):
        where = (n, p, ninst, G, layout, num_cu, icpt)
        q = p + icpt
        if q > 1024:
            with pytest.raises(oa.OemgpuError) as e:
                api.logistic_multi_fold_plan(n, p, ninst, G, icpt, layout, num_cu)
            assert e.value.code == ERR_UNSUPPORTED, where
            continue
        pl = api.logistic_multi_fold_plan(n, p, ninst, G, icpt, layout, num_cu)
        base = api.logistic_multi_plan(n, p, ninst, icpt, layout, num_cu)
        mch = min(ninst, 64)
        assert pl["rows"] == base["rows"] and pl["row_chunks"] == base["row_chunks"] and pl["panel_bytes"] == base["panel_bytes"], where
        assert pl["chunk_instances"] == mch and pl["instance_chunks"] == -(-ninst // 64) and pl["groups"] == G, where
        assert pl["group_bytes"] == 8 * G * (p + 2 * q * q + 1), where    # s, XX, A and the row count of every group
        assert pl["shared_bytes"] == 8 * (q + p + 2) + (8 * 256 * p if layout == 1 else 0), where
        assert pl["chunk_bytes"] == 8 * (4 * mch * q + mch * (p + 2) + 2 * mch) + 4 * 5 * mch + PENK * mch, where
        assert pl["hessian_bytes"] == base["hessian_bytes"], where
        assert pl["bytes"] == pl["panel_bytes"] + pl["group_bytes"] + pl["shared_bytes"] + pl["chunk_bytes"] + pl["hessian_bytes"], where
        # one group and the plain call's instances: the plain plan's groups plus the row count
        if G == 1:
            assert pl["group_bytes"] + pl["shared_bytes"] == base["shared_bytes"] + 8, where
    big = api.logistic_multi_fold_plan(10 ** 6, 1023, 176, 11, True, 0, 256)
    print("q = 1024, K = 10: the groups hold", big["group_bytes"] / 1e6, "MB of", big["bytes"] / 1e6)
    assert 180e6 < big["group_bytes"] < 190e6


def test_fold_plan_refuses_bad_arguments(oa):
    lib = oa.lib()
    out = (C.c_int64 * 11)()
    for args in ((0, 4, 1, 1, 1, 0, 256), (10, 0, 1, 1, 1, 0, 256), (10, 4, 0, 1, 1, 0, 256), (10, 4, 1, 0, 1, 0, 256), (10, 4, 1, 1, 1, 2, 256),
                 (10, 4, 1, 1, 1, 0, 0)):
        assert lib.oemgpu_selftest_logistic_multi_fold_plan(*args, out) == ERR_ARG, args
    assert lib.oemgpu_selftest_logistic_multi_fold_plan(10, 4, 1, 1, 1, 0, 256, None) == ERR_ARG


# ------------------------------------------------------------------------------------------------ header, bindings, exports
def test_header_bindings_and_exports_in_step(oa):
    from oem_amd import _lib as L
    header = (ROOT / "include" / "oemgpu.h").read_text()
    for name, nargs in (("oemgpu_fit_logistic_dense_multi_fold_dev", 26), ("oemgpu_fit_logistic_dense_multi_fold_rm_dev", 27),
                        ("oemgpu_selftest_logistic_multi_fold_plan", 8), ("oemgpu_selftest_logistic_multi_rows_fold_dev", 19)):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl, name
        args = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S)
        assert len(args.split(",")) == nargs == len(L._SIGS[name][1]), name
        assert name in L.EXPORTS and name in oa.EXPORTS
        assert callable(getattr(oa.lib(), name))
    for name in ("oem_fit_logistic_dense_multi_folds", "cv_oem_logistic_multi"):
        assert name in oa.__all__ and callable(getattr(oa, name))
