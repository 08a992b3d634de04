"""cv.oem on a resident sparse x with n <= p, the part that needs no GPU: the three new symbols; every refusal that comes back before
a device is looked for; the scoring plan over (n, K, npen, nl); and, on the reference side alone, that every input of the GPU parity
test (tests/test_gpu_cv_sparse_wide.py) stays inside the agreement rule -- the masked restatement against the restatement and the
oracle on the SLICED data."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as orc
from tests import cv_sparse_wide_restatement as M
from tests import sparse_wide_restatement as R
from tests.test_gpu_sparse_wide import DTOL, _agree

ROOT = Path(__file__).resolve().parent.parent
NEW = ("oemgpu_fit_sparse_wide_fold_res", "oemgpu_cv_sparse_wide_score_res", "oemgpu_selftest_cv_sparse_wide_score_plan")
ERR_ARG, ERR_UNSUPPORTED = -1, -4
CU = 256


def _c_args(text, name):
    """the parameter types of `name` in the header, as a list of normalised strings"""
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, name
    out = []
    for a in m.group(1).split(","):
        a = re.sub(r"\s+", " ", a).strip()
        out.append(re.sub(r"\s*\b\w+$", "", a).replace(" *", "*").strip())       # drop the parameter's name
    return out


def test_new_symbols_are_exported_and_declared_alike():
    import oem_amd
    from oem_amd import _lib
    h = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "oemgpu.h").read_text(), flags=re.S)
    L = oem_amd.lib()
    scalar = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    for name in NEW:
        assert hasattr(L, name), name
        assert name in oem_amd.EXPORTS, name
        want = _c_args(h, name)
        res, args = _lib._SIGS[name]
        assert res is C.c_int and len(args) == len(want), (name, len(args), len(want))
        for t, a in zip(want, args):
            if t.endswith("*"):                                      # a pointer in the header is a pointer (or an address) in the binding
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, t, a)
            else:
                assert a is scalar[t.replace("const ", "")], (name, t, a)
    assert len(L.oemgpu_switch_names().split()) == 34                # no new diagnostic switch


# ------------------------------------------------------------------------------------------------- refusals without a device
def _opts(p, nlambda=5):
    from oem_amd import api
    return api._Args(["lasso"], [], nlambda, 0.05, 1.0, 3.0, 0.5, 1e-7, 500, False, False, np.ones(p), np.zeros(0, np.int32),
                     np.zeros(0, np.int32), np.zeros(0))


class _Handle(C.Structure):
    """the leading fields of oemgpu_sparse_x (oem_amd/csrc/logistic.hpp) that the entries' checks read; the device arrays behind them
    stay NULL and are never followed by the checks under test"""
    _fields_ = [("device", C.c_int), ("n", C.c_int64), ("nnz", C.c_int64), ("maxcol", C.c_int64), ("p", C.c_int32), ("rest", C.c_char * 256)]


def test_fold_entry_refuses_before_any_device_work():
    import oem_amd
    L = oem_amd.lib()
    p = 8
    a = _opts(p)
    out = tuple(a.outputs(p + 1))
    scratch = (C.c_double * 64)()                                   # a zeroed "context": device 0, never followed further
    ptr = C.addressof(scratch)
    h = _Handle(); h.device = 0; h.n = 5; h.p = p
    kept = C.c_int64(-7)

    def call(ctx=ptr, x=C.addressof(h), y=ptr, fid=ptr, nfolds=3, leave=1, opts=C.byref(a.c), outs=out, kp=C.byref(kept)):
        rc = L.oemgpu_fit_sparse_wide_fold_res(ctx, x, y, fid, nfolds, leave, 1, opts, *outs, kp)
        return rc, L.oemgpu_last_error().decode()
    for kw in (dict(ctx=None), dict(x=None), dict(y=None), dict(opts=None), dict(outs=(None,) + out[1:]), dict(outs=out[:4] + (None,)),
               dict(kp=None)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "NULL argument" in msg, kw
    for nf in (2, 513, 0, -1):
        rc, msg = call(nfolds=nf, leave=0)
        assert rc == ERR_ARG and "3..512" in msg, nf
    assert call(nfolds=3)[0] != 0 and call(nfolds=512)[0] != 0      # (both in range: refused further on, below)
    for lo in (-1, 4):
        rc, msg = call(leave=lo)
        assert rc == ERR_ARG and "leave_out" in msg, lo
    rc, msg = call(fid=None, leave=2)
    assert rc == ERR_ARG and "NULL foldid" in msg
    h.device = 1
    rc, msg = call(fid=None, leave=0)                                # a NULL foldid is fine with leave_out = 0: the next check answers
    assert rc == ERR_ARG and "different devices" in msg
    h.device = 0; h.n = 1
    rc, msg = call()
    assert rc == ERR_ARG and "two rows" in msg
    h.n = p + 1
    rc, msg = call()
    assert rc == ERR_UNSUPPORTED and "oemgpu_fit_sparse serves it" in msg and "n > p" in msg
    rc0 = L.oemgpu_fit_sparse_wide_res(ptr, C.addressof(h), ptr, 1, C.byref(a.c), *out)
    assert rc0 == ERR_UNSUPPORTED and L.oemgpu_last_error().decode() == msg      # the existing entry: the same sentence (one body)
    h.n = p                                                          # n = p is served: the next refusal is the options'
    a.c.nlambda = 0
    rc, msg = call()
    assert rc == ERR_ARG and "n > p" not in msg
    assert kept.value == -7                                          # nothing was written


def test_score_entry_refuses_before_any_device_work():
    import oem_amd
    L = oem_amd.lib()
    p, K, npen, nl = 8, 3, 2, 4
    scratch = (C.c_double * 64)()
    ptr = C.addressof(scratch)
    h = _Handle(); h.device = 0; h.n = 5; h.p = p
    coef = np.zeros((K, npen, nl, p + 1)); tri = np.zeros((K, npen, nl, 3))
    ncol = np.array([4, 2], dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def call(ctx=ptr, x=C.addressof(h), y=ptr, fid=ptr, nfolds=K, cf=coef.ctypes.data_as(dp), np_=npen, nl_=nl, nc=ncol, tm=0,
             tr=tri.ctypes.data_as(dp)):
        rc = L.oemgpu_cv_sparse_wide_score_res(ctx, x, y, fid, nfolds, cf, np_, nl_, None if nc is None else nc.ctypes.data_as(ip), tm, tr, None)
        return rc, L.oemgpu_last_error().decode()
    for kw in (dict(ctx=None), dict(x=None), dict(y=None), dict(fid=None), dict(cf=None), dict(nc=None), dict(tr=None)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "NULL argument" in msg, kw
    for kw in (dict(np_=0), dict(nl_=0)):
        assert call(**kw)[0] == ERR_ARG, kw
    for nf in (2, 513):
        rc, msg = call(nfolds=nf)
        assert rc == ERR_ARG and "3..512" in msg
    for tm in (-1, 2):
        rc, msg = call(tm=tm)
        assert rc == ERR_ARG and "type_measure" in msg
    for bad in ([5, 2], [4, -1]):
        rc, msg = call(nc=np.array(bad, dtype=np.int32))
        assert rc == ERR_ARG and "ncol" in msg
    h.device = 1
    rc, msg = call()
    assert rc == ERR_ARG and "different devices" in msg


# ------------------------------------------------------------------------------------------------- the scoring plan
KEYS = ("waves", "nwg", "lblk", "table_bytes", "part_bytes", "nl16", "ws_bytes")


def _plan(n, p, K, npen, nl, cu=CU):
    import oem_amd
    out = (C.c_int64 * 7)()
    rc = oem_amd.lib().oemgpu_selftest_cv_sparse_wide_score_plan(n, p, K, npen, nl, cu, out)
    assert rc == 0, oem_amd.lib().oemgpu_last_error()
    return dict(zip(KEYS, list(out)))


@pytest.mark.parametrize("nl", [1, 16, 17, 64, 65, 100])
@pytest.mark.parametrize("K", [3, 10, 512])
def test_score_plan_sweep(K, nl):
    r256 = lambda b: (b + 255) // 256 * 256
    for n, p in [(2, 300), (60, 400), (2000, 200000), (5000, 50000)]:      # n = 2 < K: folds with no rows
        for npen in (1, 3, 9):
            P = _plan(n, p, K, npen, nl)
            nl16 = (nl + 15) // 16 * 16
            lblk = (nl + 63) // 64
            assert P["nl16"] == nl16 and P["lblk"] == lblk
            assert P["table_bytes"] == (p + 1) * nl16 * 8             # one fold's, one penalty's transposed table
            per_fold = -(-n // K)
            want = min(CU * 4 // (npen * lblk), -(-per_fold // 4), 1024, (64000000 // (K * npen * nl16 * 32)) // 4)
            assert P["nwg"] == max(1, want) and P["waves"] == 4 * P["nwg"]
            assert P["part_bytes"] == K * P["waves"] * npen * nl16 * 32
            assert P["part_bytes"] <= 64000000 or P["nwg"] == 1
            assert P["ws_bytes"] == (r256(4 * n) + r256(8 * npen * nl * (p + 1)) + r256(npen * P["table_bytes"]) + r256(P["part_bytes"])
                                     + r256(24 * K * npen * nl) + r256(4 * npen))
            # one fold's tables at a time: nothing of K tables
            assert P["ws_bytes"] < 2 * 8 * npen * (p + 1) * nl16 + P["part_bytes"] + 4 * n + 24 * K * npen * nl + 2048


def test_score_plan_argument_errors():
    import oem_amd
    L = oem_amd.lib()
    out = (C.c_int64 * 7)()
    for args in [(0, 10, 3, 1, 1, CU), (10, 0, 3, 1, 1, CU), (10, 20, 2, 1, 1, CU), (10, 20, 513, 1, 1, CU), (10, 20, 3, 0, 1, CU),
                 (10, 20, 3, 1, 0, CU), (10, 20, 3, 1, 1, 0)]:
        assert L.oemgpu_selftest_cv_sparse_wide_score_plan(*args, out) == ERR_ARG, args
    assert L.oemgpu_selftest_cv_sparse_wide_score_plan(10, 20, 3, 1, 1, CU, None) == ERR_ARG


# ------------------------------------------------------------------------------------------------- the reference side alone
@pytest.mark.parametrize("n,p,dens,K", M.PARITY_CASES)
@pytest.mark.parametrize("standardize", [False, True])
def test_masked_restatement_agrees_with_the_sliced_fits_on_the_parity_inputs(n, p, dens, K, standardize):
    """every fold of every parity input: the masked restatement against sparse_wide_restatement.fit and against the oracle, both on
    x[keep], y[keep] -- the _agree rule of tests/test_gpu_sparse_wide.py, d to DTOL, lambda to 1e-12, the loss to 1e-7.  y is NaN in
    the left-out rows of the masked call: excluded by a select."""
    x, y, fid = M.parity_input(n, p, dens, K)
    assert sorted(np.unique(fid)) == list(range(1, K + 1))
    kw = dict(M.PARITY_KW, standardize=standardize)
    pens = ["lasso", "elastic.net", "mcp"]
    xr = x.tocsr()
    for k in range(1, K + 1):
        keep = fid != k
        xs = xr[keep].tocsc(); ys = y[keep]
        f = M.fit(x, np.where(keep, y, np.nan), keep, pens, alpha=0.7, compute_loss=True, **kw)
        s = R.fit(xs, ys, pens, alpha=0.7, compute_loss=True, **kw)
        r = orc.fit_sparse(xs, ys, native=True, penalty=pens, alpha=0.7, intercept=False, compute_loss=True, **kw)
        assert f["kept"] == int(keep.sum()) == xs.shape[0]
        for ref, name in ((s, "restatement"), (r, "oracle")):
            assert abs(f["d"] - ref["d"]) <= DTOL * ref["d"], (name, k)
            for i, pen in enumerate(pens):
                assert np.allclose(f["lambda"][i], ref["lambda"][i], rtol=1e-12, atol=0), (name, k, pen)
                _agree(f, ref, i, kw["tol"], (name, k, pen))
                assert np.allclose(np.ravel(f["loss"][i]), np.ravel(ref["loss"][i]), rtol=1e-7), (name, k, pen)
        for i, pen in enumerate(pens):
            assert np.count_nonzero(np.asarray(r["beta"][i])[1:, -1]) >= 3, (k, pen)       # (a path that selects something)
