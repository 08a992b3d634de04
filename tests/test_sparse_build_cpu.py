"""SparseX from device arrays, the part that needs no GPU: the numpy restatement of the sort passes against scipy's conversions, the plan
selftest against its restatement and the arithmetic of DESIGN.md 3.17, the refusals oemgpu_sparse_x_create_dev makes before a device is
looked for (the context and the device pointers point at zeroed host scratch and are never followed), the new entries' NULL checks,
and the host-tensor -> scipy helper."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from tests.sparse_build_restatement import CSC, CSR, build, from_scipy, plan, same

ROOT = Path(__file__).resolve().parent.parent
NEW = ("oemgpu_sparse_x_create_dev", "oemgpu_selftest_sparse_build_plan", "oemgpu_sparse_x_export", "oemgpu_sparse_x_dims",
       "oemgpu_fit_sparse_res", "oemgpu_xval_sparse_res")
KEYS = ("passes", "digit_bits", "nwg", "ws_bytes", "handle_bytes", "per", "key_bits", "T")


def test_new_symbols_are_declared_exported_and_bound():
    import oem_amd
    h = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "oemgpu.h").read_text(), flags=re.S)
    L = oem_amd.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, h), name
        assert hasattr(L, name), name
        assert name in oem_amd.EXPORTS, name
    assert "oem_fit_sparse" in oem_amd.__all__ and callable(oem_amd.oem_fit_sparse)
    assert hasattr(oem_amd.SparseX, "to_scipy")


def _plan(n, p, nnz, layout, num_cu):
    import oem_amd
    out = (C.c_int64 * 8)()
    rc = oem_amd.lib().oemgpu_selftest_sparse_build_plan(n, p, nnz, layout, num_cu, out)
    return rc, dict(zip(KEYS, list(out)))


def _pass_limits():
    """the largest number of target lines served by one and by two passes, read from the plan selftest"""
    lim = []
    for want in (1, 2):
        lo, hi = 1, 2 ** 31 - 2
        while lo < hi:                                        # the largest T with passes <= want
            mid = (lo + hi + 1) // 2
            if _plan(3, mid, 10, CSR, 256)[1]["passes"] <= want:
                lo = mid
            else:
                hi = mid - 1
        lim.append(lo)
    return lim


def test_plan_selftest_is_the_restatement_and_designs_arithmetic():
    one, two = _pass_limits()
    assert (one, two) == (2 ** 11, 2 ** 22)                  # digits of at most 11 bits
    seen = set()
    for n in (1, 2, 3, 40, 2047, 2048, 2049, 8192, 8193, 20000, 10 ** 6, two, two + 1, 2 ** 31 - 1):
        for p in (1, 2, 37, 512, one, one + 1, 70001, two, two + 1, 2 ** 31 - 1):
            for nnz in (0, 1, 2048, 2049, 5000, 10 ** 6, 5 * 10 ** 6 + 7, 2 ** 31 - 1):
                for layout in (CSC, CSR):
                    for num_cu in (1, 64, 256, 304):
                        rc, got = _plan(n, p, nnz, layout, num_cu)
                        assert rc == 0
                        want = plan(n, p, nnz, layout, num_cu)
                        assert got == want, (n, p, nnz, layout, num_cu, got, want)
                        # digits of at most 11 bits that cover the largest index; whole tiles to a workgroup; at most
                        # four workgroups to a CU; every non-zero in exactly one workgroup
                        assert got["digit_bits"] <= 11 and got["passes"] * got["digit_bits"] >= got["key_bits"]
                        assert (1 << got["key_bits"]) >= got["T"] and (got["key_bits"] == 0 or (1 << (got["key_bits"] - 1)) < got["T"])
                        assert got["per"] % 2048 == 0 and got["nwg"] <= max(1, 4 * num_cu)
                        assert got["nwg"] * got["per"] >= nnz and (got["nwg"] - 1) * got["per"] < max(nnz, 1)
                        seen.add(got["passes"])
    assert seen == {1, 2, 3}
    import oem_amd
    L = oem_amd.lib()
    out = (C.c_int64 * 8)()
    assert L.oemgpu_selftest_sparse_build_plan(0, 5, 1, CSC, 256, out) == -1
    assert L.oemgpu_selftest_sparse_build_plan(5, 0, 1, CSC, 256, out) == -1
    assert L.oemgpu_selftest_sparse_build_plan(5, 5, -1, CSC, 256, out) == -1
    assert L.oemgpu_selftest_sparse_build_plan(5, 5, 1, 2, 256, out) == -1
    assert L.oemgpu_selftest_sparse_build_plan(5, 5, 1, CSC, 0, out) == -1
    assert L.oemgpu_selftest_sparse_build_plan(5, 5, 1, CSC, 256, None) == -1
    assert L.oemgpu_selftest_sparse_build_plan(2 ** 31, 5, 1, CSC, 256, out) == -4
    assert L.oemgpu_selftest_sparse_build_plan(5, 5, 2 ** 31, CSC, 256, out) == -4


def _random(n, p, density, seed, full_row=None, full_col=None, empty_rows=(), empty_cols=()):
    rng = np.random.default_rng(seed)
    x = sp.random(n, p, density=density, format="lil", random_state=rng, data_rvs=lambda k: rng.normal(size=k))
    if full_row is not None:
        x[full_row, :] = rng.normal(size=p)
    if full_col is not None:
        x[:, full_col] = rng.normal(size=(n, 1))
    for r in empty_rows:
        x[r, :] = 0
    for c in empty_cols:
        x[:, c] = 0
    x = x.tocsr()
    x.eliminate_zeros()
    return x


def _both_ways(x, num_cu=256):
    n, p = x.shape
    want = from_scipy(x)
    c = sp.csc_matrix(x); c.sort_indices()
    r = sp.csr_matrix(x); r.sort_indices()
    for layout, m in ((CSC, c), (CSR, r)):
        got = build(layout, m.indptr, m.indices, m.data, n, p, num_cu)
        assert same(got, want) is None, (layout, x.shape, same(got, want))


def test_restatement_of_the_passes_is_scipys_transposition():
    one, two = _pass_limits()
    _both_ways(_random(300, 37, 0.05, 0, empty_rows=(0, 7, 299), empty_cols=(0, 36)))
    _both_ways(_random(9000, 5, 0.3, 1, full_col=2))                    # a full column; more than one workgroup's share at num_cu = 1
    _both_ways(_random(9000, 5, 0.3, 1, full_col=2), num_cu=1)
    _both_ways(_random(6, 5000, 0.05, 2, full_row=3))                   # a full row, two passes
    _both_ways(sp.csr_matrix((50, 9)))                                  # nnz = 0
    _both_ways(_random(1, 40, 0.5, 3))
    _both_ways(_random(40, 1, 0.5, 4))
    # index values on both sides of every digit boundary the plan has: the last index of a digit, the first of the next, for every pass
    for T in (one, one + 1, two, two + 1):
        P = plan(3, T, 10, CSR, 256)
        cols = {0, T - 1}
        for ps in range(1, P["passes"]):
            b = 1 << (ps * P["digit_bits"])
            cols |= {c for c in (b - 1, b, b + 1, 2 * b - 1, 2 * b) if c < T}
        cols = np.array(sorted(cols))
        rows = np.arange(len(cols)) % 3
        x = sp.csr_matrix((np.arange(1, len(cols) + 1, dtype=np.float64), (rows, cols)), shape=(3, T))
        assert plan(3, T, x.nnz, CSR, 256)["passes"] == P["passes"]
        r = sp.csr_matrix(x); r.sort_indices()
        got = build(CSR, r.indptr, r.indices, r.data, 3, T)
        c = sp.csc_matrix(x); c.sort_indices()
        assert np.array_equal(got["colptr"], c.indptr) and np.array_equal(got["rowidx"], c.indices) and np.array_equal(got["val"], c.data)


def test_restatement_moves_values_bit_for_bit():
    x = _random(200, 30, 0.2, 5).tocsr()
    x.data[:6] = [0.0, -0.0, 5e-324, -2.5e-310, np.nan, np.inf]        # stored zeros, denormals, NaN: kept as stored
    got = build(CSR, x.indptr, x.indices, x.data, 200, 30)
    assert np.array_equal(np.sort(got["val"].view(np.int64)), np.sort(x.data.view(np.int64)))
    assert np.array_equal(got["cval"].view(np.int64), x.data.view(np.int64))
    d = np.zeros((200, 30)); d[:] = np.nan
    rr = np.repeat(np.arange(200), np.diff(x.indptr))
    d[rr, x.indices] = x.data
    cc = np.repeat(np.arange(30), np.diff(got["colptr"]))
    assert np.array_equal(d[got["rowidx"], cc].view(np.int64), got["val"].view(np.int64))


def test_create_dev_refuses_before_any_device():
    import oem_amd
    L = oem_amd.lib()
    scratch = (C.c_double * 64)()
    ptr = C.addressof(scratch)

    def call(ctx=ptr, n=50, p=5, layout=CSC, ptr_=ptr, pt=1, idx=ptr, it=0, val=ptr, vt=0, nnz=10, out=True):
        h = C.c_void_p(12345)
        rc = L.oemgpu_sparse_x_create_dev(ctx, n, p, layout, ptr_, pt, idx, it, val, vt, nnz, C.byref(h) if out else None)
        assert rc != 0 and (not out or not h.value)            # a refused create leaves a NULL handle behind
        return rc, L.oemgpu_last_error().decode()
    assert call(ctx=None) == (-1, "sparse_x_create_dev: NULL argument")
    assert call(ptr_=None) == (-1, "sparse_x_create_dev: NULL argument")
    assert call(out=False) == (-1, "sparse_x_create_dev: NULL argument")
    for layout in (-1, 2, 3):
        rc, msg = call(layout=layout)
        assert rc == -1 and "layout" in msg
    for kw in (dict(pt=2), dict(pt=-1), dict(it=2), dict(it=7)):
        rc, msg = call(**kw)
        assert rc == -1 and "OEMGPU_I32 or OEMGPU_I64" in msg
    for vt in (-1, 2):
        rc, msg = call(vt=vt)
        assert rc == -1 and "OEMGPU_F64 or OEMGPU_F32" in msg
    for kw in (dict(n=0), dict(p=0), dict(nnz=-1), dict(n=-5)):
        assert call(**kw) == (-1, "sparse_x_create_dev: bad dimensions")
    assert call(idx=None) == (-1, "sparse_x_create_dev: NULL row indices or values")
    assert call(val=None, layout=CSR) == (-1, "sparse_x_create_dev: NULL column indices or values")
    rc, msg = call(n=2 ** 31)
    assert rc == -4 and "n >= 2^31" in msg
    rc, msg = call(nnz=2 ** 31)
    assert rc == -4 and "nnz >= 2^31" in msg


def test_new_entries_refuse_null_arguments_before_any_device():
    import oem_amd
    from oem_amd import api
    L = oem_amd.lib()
    scratch = (C.c_double * 64)()
    ptr = C.addressof(scratch)
    a = api._Args(["lasso"], [], 5, 1e-4, 1.0, 3.0, 0.5, 1e-7, 500, False, False, np.ones(4), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    out = a.outputs(5)
    cv = (C.c_double * 8)()
    for ctx, x, y in ((None, ptr, ptr), (ptr, None, ptr), (ptr, ptr, None)):
        assert L.oemgpu_fit_sparse_res(ctx, x, y, 1, 0, C.byref(a.c), *out) == -1
        assert b"NULL" in L.oemgpu_last_error()
        assert L.oemgpu_xval_sparse_res(ctx, x, y, ptr, 5, 1, 0, 0, C.byref(a.c), *out, cv, cv) == -1
        assert b"NULL" in L.oemgpu_last_error()
    assert L.oemgpu_xval_sparse_res(ptr, ptr, ptr, None, 5, 1, 0, 0, C.byref(a.c), *out, cv, cv) == -1
    assert L.oemgpu_sparse_x_export(None, None, None, None, None, None, None, None) == -1
    assert L.oemgpu_sparse_x_dims(None, None) == -1


def test_a_host_sparse_tensor_becomes_the_scipy_matrix_of_its_components():
    import torch
    from oem_amd import api
    x = _random(40, 9, 0.3, 6)
    c = x.tocsc()
    tensors = {
        "csr": torch.sparse_csr_tensor(torch.as_tensor(x.indptr, dtype=torch.int64), torch.as_tensor(x.indices, dtype=torch.int32),
                                       torch.as_tensor(x.data), size=x.shape),
        "csc": torch.sparse_csc_tensor(torch.as_tensor(c.indptr, dtype=torch.int32), torch.as_tensor(c.indices, dtype=torch.int64),
                                       torch.as_tensor(c.data), size=x.shape),
        "coo": torch.sparse_coo_tensor(np.vstack([x.tocoo().row, x.tocoo().col]), x.tocoo().data, size=x.shape),
    }
    for name, t in tensors.items():
        assert api._is_torch_sparse(t) and not api._is_torch_cuda(t)
        m = api._sparse_tensor_arg(t)
        assert sp.issparse(m) and m.dtype == np.float64 and m.shape == x.shape, name
        assert (m != x).nnz == 0, name
    t32 = torch.sparse_csr_tensor(torch.as_tensor(x.indptr), torch.as_tensor(x.indices), torch.as_tensor(x.data.astype(np.float32)), size=x.shape)
    m = api._torch_sparse_to_scipy(t32)
    assert m.dtype == np.float64 and np.array_equal(m.data, x.data.astype(np.float32).astype(np.float64))
    dense = torch.zeros(4, 3)
    assert not api._is_torch_sparse(dense) and api._sparse_tensor_arg(dense) is dense
    assert api._sparse_tensor_arg(x) is x
    # what is not served says why
    bsr = torch.sparse_bsr_tensor(torch.tensor([0, 1, 2]), torch.tensor([0, 1]), torch.ones(2, 2, 2, dtype=torch.float64), size=(4, 4))
    with pytest.raises(ValueError, match="layout torch.sparse_bsr is not served"):
        api._torch_sparse_parts(bsr)
    half = torch.sparse_coo_tensor(np.array([[0, 1], [1, 2]]), torch.ones(2, dtype=torch.float16), size=(3, 3))
    with pytest.raises(ValueError, match="float64 or float32, not torch.float16"):
        api._torch_sparse_parts(half)
    three = torch.sparse_coo_tensor(np.array([[0, 1], [1, 2], [0, 0]]), torch.ones(2, dtype=torch.float64), size=(3, 3, 2))
    with pytest.raises(ValueError, match="not one of 3 dimensions"):
        api._torch_sparse_parts(three)
    with pytest.raises(TypeError):
        import oem_amd
        oem_amd.SparseX(np.zeros((4, 3)))
