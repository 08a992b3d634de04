"""oem() on a sparse x with p >= n from its non-zeros, the part that needs no GPU: the restatement the GPU tests lean on agrees with
the oracle on every input of the GPU parity test (so those inputs stay inside the parity rule's caps on the reference side alone);
the host plan on both sides of each of its limits; the refusals that come back before a device is looked for; the new symbols."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as orc
from tests import sparse_wide_restatement as R

ROOT = Path(__file__).resolve().parent.parent
NEW = ("oemgpu_fit_sparse_wide_res", "oemgpu_selftest_sparse_wide_plan", "oemgpu_last_host_path_engine")
ERR_ARG, ERR_UNSUPPORTED = -1, -4
DTOL = 1e-10
CU = 256


def test_new_symbols_are_declared_exported_and_bound():
    import oem_amd
    h = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "oemgpu.h").read_text(), flags=re.S)
    L = oem_amd.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, h), name
        assert hasattr(L, name), name
        assert name in oem_amd.EXPORTS, name
    assert re.search(r"OEMGPU_ENGINE_SPARSE_WIDE\s*=\s*10\b", h)
    from oem_amd import api
    assert api.ENGINES[10] == "sparse-wide"
    assert len(L.oemgpu_switch_names().split()) == 34              # the table is full: the route is forced by values of OEM_SPARSE_GRAM


@pytest.mark.parametrize("n,p,dens", R.PARITY_SHAPES)
@pytest.mark.parametrize("standardize", [False, True])
def test_restatement_agrees_with_the_oracle_on_the_parity_inputs(n, p, dens, standardize):
    """niter identical at every lambda, beta to 1e-9 of its scale, d to the eigen tolerance, lambda to 1e-12: the restatement (sparse
    products, ARPACK's d) against the oracle (dense products, exact dense eigen-solve) on the (shape, seed) of the GPU parity test.
    Equal counts on the reference side show that these inputs do not graze the stop rule: the GPU test's "within one, 75 % equal"
    then has room only for the device's own rounding."""
    x, y = R.parity_data(n, p, dens)
    assert x.shape == (n, p) and x.nnz <= 0.02 * n * p and np.diff(x.indptr)[5] == 0
    kw = dict(R.PARITY_KW, standardize=standardize)
    pens = ["lasso", "elastic.net", "mcp"]
    r = orc.fit_sparse(x, y, native=True, penalty=pens, alpha=0.7, intercept=False, compute_loss=True, **kw)
    f = R.fit(x, y, pens, alpha=0.7, compute_loss=True, **kw)
    assert abs(f["d"] - r["d"]) <= DTOL * r["d"]
    for k, pen in enumerate(pens):
        assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-12, atol=0), pen
        fn, rn = np.ravel(f["niter"][k]).astype(int), np.ravel(r["niter"][k]).astype(int)
        assert np.array_equal(fn, rn), (pen, fn, rn)
        rb = np.asarray(r["beta"][k])
        scale = max(1.0, float(np.abs(rb).max()))
        assert np.abs(np.asarray(f["beta"][k]) - rb).max() <= 1e-9 * scale, pen
        assert np.all(rb[0] == 0.0) and np.count_nonzero(rb[1:, -1]) >= 3, pen       # (a path that selects something)
        assert np.allclose(np.ravel(f["loss"][k]), np.ravel(r["loss"][k]), rtol=1e-7), pen


def _plan(n, p, nnz, lrow=0, lcol=0, cu=CU):
    import oem_amd
    out = (C.c_int64 * 8)()
    rc = oem_amd.lib().oemgpu_selftest_sparse_wide_plan(n, p, nnz, lrow, lcol, cu, out)
    assert rc == 0, oem_amd.lib().oemgpu_last_error()
    return dict(zip(("route", "rows_per_wave", "cols_per_wave", "long_rows", "long_cols", "row_wgs", "col_wgs", "ws_bytes"), list(out)))


def test_route_on_both_sides_of_each_limit(monkeypatch):
    n, p = 500, 4000
    assert _plan(n, p, n * p // 50)["route"] == 1                    # exactly 2 %
    assert _plan(n, p, n * p // 50 + 1)["route"] == 0
    assert _plan(300, 1025, 300)["route"] == 1 and _plan(300, 1024, 300)["route"] == 0
    assert _plan(2000, 2000, 1000)["route"] == 1 and _plan(2001, 2000, 1000)["route"] == 0     # n = p, n = p + 1
    # WIDE_MAX_N (32,768 rows: where the dense wide engine ends) does not apply
    assert _plan(32768, 40000, 10 ** 6)["route"] == 1 and _plan(32769, 40000, 10 ** 6)["route"] == 1
    assert _plan(20000, 1000000, 2 * 10 ** 7)["route"] == 1
    # the switch forces the route for any n <= p and forbids it; n > p is never this engine's
    monkeypatch.setenv("OEM_SPARSE_GRAM", "wide")
    assert _plan(40, 100, 40 * 100)["route"] == 1 and _plan(300, 1024, 300)["route"] == 1 and _plan(101, 100, 10)["route"] == 0
    monkeypatch.setenv("OEM_SPARSE_GRAM", "nowide")
    assert _plan(n, p, 100)["route"] == 0 and _plan(20000, 1000000, 2 * 10 ** 7)["route"] == 0
    monkeypatch.delenv("OEM_SPARSE_GRAM")
    assert _plan(n, p, 100)["route"] == 1


def test_plan_lanes_workgroups_and_long_forms():
    """lanes per line: about four entries per lane, raised while the launch would leave CUs idle; 64 / lanes lines to a wave, 256
    threads to a workgroup; a line of more than 32 entries per lane is the long form's"""
    P = _plan(2000, 200000, 4 * 10 ** 6)                           # 2,000-entry rows, 20-entry columns
    assert P["rows_per_wave"] == 1 and P["cols_per_wave"] == 8
    assert P["row_wgs"] == 2000 * 64 // 256 and P["col_wgs"] == 200000 * 8 // 256
    P = _plan(33000, 34000, 336600)                                # ~10 entries a line on both sides
    assert P["rows_per_wave"] == 16 and P["cols_per_wave"] == 16
    assert P["row_wgs"] == -(-33000 * 4 // 256) and P["col_wgs"] == -(-34000 * 4 // 256)
    P = _plan(40, 1100, 880)                                       # few lines: more lanes to each until the CUs are busy
    assert P["rows_per_wave"] == 1 and P["row_wgs"] == 10 and P["cols_per_wave"] == 1 and P["col_wgs"] == 275
    assert _plan(40, 1100, 880, cu=4)["rows_per_wave"] == 2        # (a device of 4 CUs is busy with fewer lanes to a row)
    # the long forms, on either side of their switch: 32 entries per lane
    for n, p, nnz in [(2000, 200000, 4 * 10 ** 6), (33000, 34000, 336600), (200, 20000, 40000)]:
        P = _plan(n, p, nnz)
        lr, lc = 32 * 64 // P["rows_per_wave"], 32 * 64 // P["cols_per_wave"]
        Q = _plan(n, p, nnz, lr, lc)
        assert (Q["long_rows"], Q["long_cols"]) == (0, 0)
        Q = _plan(n, p, nnz, lr + 1, lc)
        assert (Q["long_rows"], Q["long_cols"]) == (1, 0)
        Q = _plan(n, p, nnz, lr, lc + 1)
        assert (Q["long_rows"], Q["long_cols"]) == (0, 1)
        assert {k: v for k, v in Q.items() if not k.startswith("long")} == {k: v for k, v in P.items() if not k.startswith("long")}
    # the GPU structure test's shape: a full row and a full column are long there
    P = _plan(200, 20000, 40000, 20000, 200)
    assert (P["long_rows"], P["long_cols"]) == (1, 1)


def test_plan_workspace_is_vectors_table_and_lists():
    r256 = lambda b: (b + 255) // 256 * 256
    for n, p in [(40, 1100), (33000, 34000), (20000, 1000000)]:
        P = _plan(n, p, n * 10)
        assert P["ws_bytes"] == r256(8 * (4 * n + 1024)) + r256(4 * (n + 1)) + r256(4 * (p + 1)) + 256
        assert P["ws_bytes"] < 64 * (n + p) + 16384                # nothing of n p entries


def test_plan_argument_errors():
    import oem_amd
    L = oem_amd.lib()
    out = (C.c_int64 * 8)()
    for args in [(0, 10, 1, 0, 0, CU), (10, 0, 1, 0, 0, CU), (10, 20, -1, 0, 0, CU), (10, 20, 1, -1, 0, CU), (10, 20, 1, 0, -1, CU), (10, 20, 1, 0, 0, 0)]:
        assert L.oemgpu_selftest_sparse_wide_plan(*args, out) == ERR_ARG
    assert L.oemgpu_selftest_sparse_wide_plan(10, 20, 1, 0, 0, CU, None) == ERR_ARG


def _opts(p, nlambda=5):
    from oem_amd import api
    return api._Args(["lasso"], [], nlambda, 0.05, 1.0, 3.0, 0.5, 1e-7, 500, False, False, np.ones(p), np.zeros(0, np.int32),
                     np.zeros(0, np.int32), np.zeros(0))


class _Handle(C.Structure):
    """the leading fields of oemgpu_sparse_x (oem_amd/csrc/logistic.hpp) that the entry's checks read; the device arrays behind them
    stay NULL and are never followed by the checks under test"""
    _fields_ = [("device", C.c_int), ("n", C.c_int64), ("nnz", C.c_int64), ("maxcol", C.c_int64), ("p", C.c_int32), ("rest", C.c_char * 256)]


def test_res_entry_refuses_before_any_device_work():
    import oem_amd
    L = oem_amd.lib()
    p = 8
    a = _opts(p)
    out = a.outputs(p + 1)
    scratch = (C.c_double * 64)()                                   # a zeroed "context": device 0, never followed further
    ptr = C.addressof(scratch)
    h = _Handle(); h.device = 0; h.n = 5; h.p = p
    hp = C.addressof(h)

    def call(ctx=ptr, x=hp, y=ptr, opts=C.byref(a.c), outs=out):
        rc = L.oemgpu_fit_sparse_wide_res(ctx, x, y, 1, opts, *outs)
        return rc, L.oemgpu_last_error().decode()
    for kw in (dict(ctx=None), dict(x=None), dict(y=None), dict(opts=None), dict(outs=(None,) + tuple(out[1:])), dict(outs=tuple(out[:4]) + (None,))):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "NULL" in msg, kw
    h.device = 1
    rc, msg = call()
    assert rc == ERR_ARG and "different devices" in msg
    h.device = 0; h.n = 1
    rc, msg = call()
    assert rc == ERR_ARG and "two rows" in msg
    h.n = p + 1
    rc, msg = call()
    assert rc == ERR_UNSUPPORTED and "oemgpu_fit_sparse" in msg and "n > p" in msg
    h.n = p                                                         # n = p is served: the next refusal is the options'
    a.c.nlambda = 0
    rc, msg = call()
    assert rc != 0 and "n > p" not in msg


def test_the_intercept_is_refused_before_the_arrays_are_checked_and_before_any_device(monkeypatch):
    """the sentence and the place of the parent commit: before csc_check (malformed arrays do not get their own message) and before
    a device is looked for (this machine has none), on either route"""
    import oem_amd
    from oem_amd import api
    L = oem_amd.lib()
    n, p = 40, 1100
    x = sp.random(n, p, density=0.01, format="csc", random_state=np.random.default_rng(1))
    cp, ri, va = np.ascontiguousarray(x.indptr, np.int64), np.ascontiguousarray(x.indices, np.int32), np.ascontiguousarray(x.data, np.float64)
    bad = cp.copy(); bad[0] = 1                                     # (csc_check would refuse this first)
    y = np.zeros(n)
    a = _opts(p)
    for sw in (None, "wide", "nowide"):
        if sw is None:
            monkeypatch.delenv("OEM_SPARSE_GRAM", raising=False)
        else:
            monkeypatch.setenv("OEM_SPARSE_GRAM", sw)
        for cptr in (cp, bad):
            rc = L.oemgpu_fit_sparse(n, p, cptr.ctypes.data, api._iptr(ri), api._dptr(va), api._dptr(y), 1, 1, C.byref(a.c), *a.outputs(p + 1))
            msg = L.oemgpu_last_error().decode()
            assert rc == ERR_UNSUPPORTED and "p + 1 entries" in msg and "intercept = FALSE is served" in msg
    # without an intercept the arrays are checked before any device is looked for, on the new route too
    rc = L.oemgpu_fit_sparse(n, p, bad.ctypes.data, api._iptr(ri), api._dptr(va), api._dptr(y), 1, 0, C.byref(a.c), *a.outputs(p + 1))
    assert rc == ERR_ARG and L.oemgpu_last_error().decode() == "fit_sparse: colptr[0] must be 0"
    with pytest.raises(ValueError, match="SparseX"):
        api.oem(object.__new__(api.SparseX), y)                     # oem() on a SparseX stays the ValueError it is
