"""SparseX from torch sparse tensors on the device (oem_amd/csrc/sparse_build.hip) and the front ends that take one.

A. The handle's arrays: oemgpu_sparse_x_export of SparseX(tensor) against the export of SparseX(scipy matrix of the same entries) --
   all seven arrays and maxcol EXACTLY, values as int64 bit patterns -- for CSR, CSC and COO input, int32 and int64 indices (a torch
   COO tensor only has int64 ones), float32 and float64 values (every value is float32-representable, so the scipy side of the widened
   float32 values is the float64 matrix itself and one reference serves a shape).  Shapes: 20,000 x 37 (three 8,192-row chunks),
   40 x 70,001 (past 2^16 target lines), both sides of every pass-count limit READ FROM THE PLAN SELFTEST in both orientations, empty
   rows and columns, nnz = 0, a full column of 20,000 entries, a full row, 1 x p, n x 1, stored zeros / -0.0 / denormals / NaN.  The C
   entry with its arrays one element past an aligned address inside garbage; two builds give equal arrays.
B. Every device refusal with the offending line named, nothing leaked and the next build served.  No invalid input is ever indexed
   with: the validation kernels reject it first.
C. The same bits from a device-born and a scipy-born handle: cv_oem Gaussian tall and wide, cv_oem binomial, predict.
D. The new fits: oem_fit_sparse(SparseX) / oem(tensor) against oem(scipy) at the sparse parity tolerances (beta 1e-8 max(1, |beta|_inf),
   d 1e-10, lambda rtol 1e-11, niter +- 1) and, without an intercept, bit for bit; the wide shape against oem(SparseX) exactly;
   xval_oem and oem_fit_logistic_sparse on a handle and on a tensor against the scipy call exactly.
E. The front ends: the temporary handle closed on every exit, x never on the host, the ValueErrors."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests.sparse_build_restatement import CSC, CSR

pytestmark = pytest.mark.gpu

ARRAYS = ("colptr", "rowidx", "val", "rowptr", "ccol", "cval", "cptr")


# ---------------------------------------------------------------------------------------------------- helpers
def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _rand(n, p, nnz, seed):
    """nnz distinct cells of an n x p matrix with float32-representable normal values"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(n * p, size=min(nnz, n * p), replace=False)
    r, c = np.divmod(cells, p)
    return sp.csr_matrix((_f32(rng.normal(size=len(cells))), (r, c)), shape=(n, p))


def _with(x, rows=None, cols=None, full_row=None, full_col=None, seed=0):
    rng = np.random.default_rng(seed)
    x = x.tolil()
    if full_row is not None:
        x[full_row, :] = _f32(rng.normal(size=x.shape[1]))
    if full_col is not None:
        x[:, full_col] = _f32(rng.normal(size=(x.shape[0], 1)))
    for r in rows or ():
        x[r, :] = 0
    for c in cols or ():
        x[:, c] = 0
    x = x.tocsr()
    x.eliminate_zeros()
    return x


def _plan_passes(T):
    import oem_amd
    out = (C.c_int64 * 8)()
    assert oem_amd.lib().oemgpu_selftest_sparse_build_plan(3, T, 10, CSR, 256, out) == 0
    return int(out[0])


@functools.lru_cache(maxsize=None)
def _pass_limits():
    """the most target lines one pass and two passes serve, read from the plan selftest"""
    lim = []
    for want in (1, 2):
        lo, hi = 1, 2 ** 31 - 2
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if _plan_passes(mid) <= want else (lo, mid - 1)
        lim.append(lo)
    return tuple(lim)


def _special():
    x = _rand(300, 23, 900, 11).tocsr()
    x.sort_indices()
    x.data[:8] = [0.0, -0.0, float(np.float32(1e-40)), float(-np.float32(3e-42)), np.nan, np.inf, -np.inf, 0.0]
    return x


@functools.lru_cache(maxsize=None)
def _case(name):
    one, two = _pass_limits()
    if name.startswith(("wide_T", "tall_T")):
        T = {"1": one, "1+": one + 1, "2": two, "2+": two + 1}[name.split("T")[1]]
        x = _rand(3, T, 5000, T % 1000)
        x = x.tolil(); x[0, 0] = 1.5; x[2, T - 1] = -2.5; x = x.tocsr()             # the first and the last target line are in use
        return x if name.startswith("wide") else sp.csr_matrix(x.T)
    return {
        "tall_chunks": lambda: _rand(20000, 37, int(0.05 * 20000 * 37), 1),
        "wide_64k": lambda: _rand(40, 70001, int(0.002 * 40 * 70001), 2),
        "empty_lines": lambda: _with(_rand(300, 37, 600, 3), rows=(0, 7, 299), cols=(0, 36)),
        "nnz0": lambda: sp.csr_matrix((50, 9)),
        "full_column": lambda: _with(_rand(20000, 5, 300, 4), full_col=2),
        "full_row": lambda: _with(_rand(6, 5000, 200, 5), full_row=3),
        "one_row": lambda: _rand(1, 40, 17, 6),
        "one_column": lambda: _rand(40, 1, 17, 7),
        "special_values": _special,
    }[name]()


CASES = ("tall_chunks", "wide_64k", "wide_T1", "wide_T1+", "wide_T2", "wide_T2+", "tall_T1", "tall_T1+", "tall_T2", "tall_T2+", "empty_lines",
         "nnz0", "full_column", "full_row", "one_row", "one_column", "special_values")
FORMS = [("csr", "int32"), ("csr", "int64"), ("csc", "int32"), ("csc", "int64"), ("coo", "int64")]


def _tensor(x, layout, itype="int64", vtype="float64", device="cuda", coalesced=None):
    import torch
    it, vt = getattr(torch, itype), getattr(torch, vtype)
    if layout == "coo":
        m = sp.coo_matrix(sp.csr_matrix(x))                      # (row-major, columns ascending in a row: what a coalesced tensor holds)
        ind = torch.as_tensor(np.vstack([m.row, m.col]).astype(np.int64), device=device)
        return torch.sparse_coo_tensor(ind, torch.as_tensor(m.data, device=device).to(vt), size=x.shape, is_coalesced=coalesced)
    m = sp.csr_matrix(x) if layout == "csr" else sp.csc_matrix(x)
    m.sort_indices()
    make = torch.sparse_csr_tensor if layout == "csr" else torch.sparse_csc_tensor
    return make(torch.as_tensor(m.indptr, device=device).to(it), torch.as_tensor(m.indices, device=device).to(it),
                torch.as_tensor(m.data, device=device).to(vt), size=x.shape)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the export of SparseX(scipy matrix): computed once per shape, shared and left unchanged"""
    import oem_amd
    with oem_amd.SparseX(_case(name)) as sx:
        e = sx.export()
    for v in e.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return e


def _assert_same(got, want, label):
    for k in ARRAYS:
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (label, k)
        if a.dtype == np.float64:
            a, b = a.view(np.int64), b.view(np.int64)
        assert np.array_equal(a, b), (label, k)
    assert got["maxcol"] == want["maxcol"], label


# ---------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("vtype", ["float64", "float32"])
@pytest.mark.parametrize("form", FORMS, ids=lambda f: "-".join(f))
@pytest.mark.parametrize("name", CASES)
def test_handle_from_a_device_tensor_is_the_scipy_handle(name, form, vtype):
    import oem_amd
    x = _case(name)
    want = _reference(name)
    # torch's own coalesce adds every entry onto +0.0, which turns a stored -0.0 into +0.0 before the builder sees it: the signed zero
    # is held to its bits in a COO tensor that is already coalesced (torch hands its values over untouched), and through torch's
    # coalesce everything but that sign is (test_special_values_through_torchs_coalesce)
    t = _tensor(x, form[0], form[1], vtype, coalesced=True if name == "special_values" else None)
    with oem_amd.SparseX(t) as sx:
        del t                                                    # the handle holds copies
        assert sx.shape == x.shape and sx.nnz == x.nnz and str(sx.device).startswith("cuda")
        _assert_same(sx.export(), want, (name, form, vtype))
    # and the scipy side is what scipy's own conversions say (one look per shape is enough)
    if form == FORMS[0] and vtype == "float64":
        from tests.sparse_build_restatement import from_scipy, same
        assert same(want, from_scipy(x)) is None


@pytest.mark.parametrize("vtype", ["float64", "float32"])
def test_special_values_through_torchs_coalesce(vtype):
    """an uncoalesced COO tensor: stored zeros, denormals, NaN and the infinities as stored; -0.0 as torch's coalesce leaves it (+0.0)"""
    import oem_amd
    x = _case("special_values")
    want = dict(_reference("special_values"))
    assert np.signbit(want["val"][want["val"] == 0.0]).any()
    for k in ("val", "cval"):
        v = want[k].copy()
        v[v == 0.0] = 0.0
        want[k] = v
    with oem_amd.SparseX(_tensor(x, "coo", "int64", vtype)) as sx:
        assert sx.nnz == x.nnz                                   # the stored zeros are still stored
        _assert_same(sx.export(), want, ("special_values", "coo", vtype))


def test_pass_counts_of_the_boundary_cases_are_the_plans():
    one, two = _pass_limits()
    assert [_plan_passes(T) for T in (one, one + 1, two, two + 1)] == [1, 2, 2, 3]
    assert _case("wide_T2+").shape == (3, two + 1) and _case("tall_T2+").shape == (two + 1, 3)


def _create_dev(layout, ptr, idx, val, n, p, nnz=None):
    """the C entry on torch component tensors; returns (rc, message, handle)"""
    import torch
    import oem_amd
    from oem_amd import _lib as L
    code = {torch.int32: 0, torch.int64: 1, torch.float64: 0, torch.float32: 1}
    h = C.c_void_p()
    torch.cuda.synchronize()
    rc = oem_amd.lib().oemgpu_sparse_x_create_dev(oem_amd.context(0), n, p, layout, ptr.data_ptr(), code[ptr.dtype], idx.data_ptr(), code[idx.dtype],
                                                  val.data_ptr(), code[val.dtype], int(idx.shape[0]) if nnz is None else nnz, C.byref(h))
    return rc, L.lib().oemgpu_last_error().decode(), h


def _export(h, n, p):
    import oem_amd
    L = oem_amd.lib()
    dims = (C.c_int64 * 4)()
    assert L.oemgpu_sparse_x_dims(h, dims) == 0 and (dims[0], dims[1]) == (n, p)
    nnz, chunks = int(dims[2]), (n + 8191) // 8192
    out = {"colptr": np.zeros(p + 1, np.int64), "rowidx": np.zeros(nnz, np.int32), "val": np.zeros(nnz), "rowptr": np.zeros(n + 1, np.int64),
           "ccol": np.zeros(nnz, np.int32), "cval": np.zeros(nnz), "cptr": np.zeros((chunks + 1, p), np.int32), "maxcol": int(dims[3])}
    assert L.oemgpu_sparse_x_export(h, *[out[k].ctypes.data for k in ARRAYS]) == 0
    return out


@pytest.mark.parametrize("layout", ["csr", "csc"])
@pytest.mark.parametrize("itype,vtype", [("int32", "float32"), ("int64", "float64"), ("int32", "float64")])
def test_c_entry_with_arrays_aligned_to_their_element_only(layout, itype, vtype):
    """every component one element past a 256-byte boundary inside a buffer of garbage"""
    import torch
    import oem_amd
    x = _case("empty_lines")
    n, p = x.shape
    m = sp.csr_matrix(x) if layout == "csr" else sp.csc_matrix(x)
    m.sort_indices()
    it, vt = getattr(torch, itype), getattr(torch, vtype)

    def place(a, dt):
        a = torch.as_tensor(a).to(dt)
        size = a.element_size()
        buf = torch.full((a.numel() * size + 1024,), 0xA5, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 256 == 0
        view = buf[256 + size:256 + size + a.numel() * size].view(dt)
        view.copy_(a)
        assert view.data_ptr() % 256 == size and view.data_ptr() % size == 0
        return buf, view
    keep, parts = zip(*[place(m.indptr, it), place(m.indices, it), place(m.data, vt)])
    rc, msg, h = _create_dev(CSR if layout == "csr" else CSC, parts[0], parts[1], parts[2], n, p)
    assert rc == 0, msg
    try:
        _assert_same(_export(h, n, p), _reference("empty_lines"), (layout, itype, vtype))
    finally:
        oem_amd.lib().oemgpu_sparse_x_destroy(h)
    del keep


def test_two_builds_give_equal_arrays():
    import oem_amd
    for name in ("tall_chunks", "wide_64k"):
        t = _tensor(_case(name), "csr", "int64", "float64")
        with oem_amd.SparseX(t) as a, oem_amd.SparseX(t) as b:
            _assert_same(a.export(), b.export(), name)


def test_to_scipy_round_trips():
    import oem_amd
    for name in ("empty_lines", "special_values", "nnz0"):
        x = sp.csc_matrix(_case(name)); x.sort_indices()
        for src in (x, _tensor(x, "coo", coalesced=True), _tensor(x, "csc", "int32", "float32")):
            with oem_amd.SparseX(src) as sx:
                back = sx.to_scipy()
                assert sx.nnz == x.nnz
            assert sp.isspmatrix_csc(back) and back.shape == x.shape and back.dtype == np.float64
            assert np.array_equal(back.indptr, x.indptr) and np.array_equal(back.indices, x.indices)
            assert np.array_equal(back.data.view(np.int64), x.data.view(np.int64))


# ---------------------------------------------------------------------------------------------------- B
def _parts(x, layout, itype="int64"):
    import torch
    m = sp.csr_matrix(x) if layout == CSR else sp.csc_matrix(x)
    m.sort_indices()
    it = getattr(torch, itype)
    return [torch.as_tensor(m.indptr, device="cuda").to(it), torch.as_tensor(m.indices, device="cuda").to(it), torch.as_tensor(m.data, device="cuda")]


@pytest.mark.parametrize("itype", ["int32", "int64"])
@pytest.mark.parametrize("layout", [CSC, CSR])
def test_device_refusals_name_the_first_offending_line(layout, itype):
    import oem_amd
    L = oem_amd.lib()
    x = _rand(60, 45, 900, 21)
    n, p = x.shape
    pn, ln, iname, rng_ = ("colptr", "column", "row", "n") if layout == CSC else ("rowptr", "row", "column", "p")
    nline, T = (p, n) if layout == CSC else (n, p)
    who = "sparse_x_create_dev: "

    def refused(ptr, idx, val, want, nnz=None):
        rc, msg, h = _create_dev(layout, ptr, idx, val, n, p, nnz)
        assert rc == -1 and not h.value and L.oemgpu_sparse_x_bytes(h) == 0, (rc, msg)        # nothing is handed out, nothing leaks
        assert msg == who + want, msg
        rc, msg, h = _create_dev(layout, *_parts(x, layout, itype), n, p)                     # and the next valid build is served
        assert rc == 0 and L.oemgpu_sparse_x_bytes(h) > 0, msg
        L.oemgpu_sparse_x_destroy(h)

    ptr, idx, val = _parts(x, layout, itype)
    lens = np.diff(ptr.cpu().numpy())
    long_lines = np.flatnonzero(lens >= 3)
    a, b = int(long_lines[2]), int(long_lines[-2])               # two lines with at least three entries, a < b
    start = ptr.cpu().numpy()
    bad = ptr.clone(); bad[0] = 1
    refused(bad, idx, val, f"{pn}[0] must be 0")
    bad = ptr.clone(); bad[-1] -= 1
    refused(bad, idx, val, f"{pn}[{'p' if layout == CSC else 'n'}] must be nnz")
    refused(ptr, idx, val, f"{pn}[{'p' if layout == CSC else 'n'}] must be nnz", nnz=int(idx.shape[0]) - 1)
    assert int(ptr[a]) > 0
    bad = ptr.clone(); bad[a + 1] = bad[a] - 1
    refused(bad, idx, val, f"{pn} must be non-decreasing")
    for v in ([-1, T, 2 ** 31 - 1] + ([2 ** 40] if itype == "int64" else [])):
        bad = idx.clone(); bad[int(start[b]) + 1] = v; bad[int(start[a]) + 2] = v             # two offenders: the smaller line is named
        refused(ptr, bad, val, f"{iname} index {v} of {ln} {a} outside [0, {rng_})")
    bad = idx.clone(); bad[int(start[b]) + 1] = bad[int(start[b])]; bad[int(start[a]) + 1] = bad[int(start[a])]     # duplicates
    refused(ptr, bad, val, f"{iname} indices of {ln} {a} are not strictly increasing")
    bad = idx.clone()
    k = int(start[b])
    bad[k], bad[k + 1] = idx[k + 1], idx[k]                                                    # an unsorted line
    refused(ptr, bad, val, f"{iname} indices of {ln} {b} are not strictly increasing")
    # an index that is out of range AND not above its predecessor: csc_check looks at the range first
    bad = idx.clone(); bad[int(start[a]) + 1] = -1
    refused(ptr, bad, val, f"{iname} index -1 of {ln} {a} outside [0, {rng_})")


def test_sparsex_refuses_unsorted_and_duplicate_tensors():
    import torch
    import oem_amd
    x = _rand(30, 20, 200, 22)
    t = _tensor(x, "csr")
    col = t.col_indices().clone()
    crow = t.crow_indices().cpu().numpy()
    r = int(np.flatnonzero(np.diff(crow) >= 2)[0])
    col[crow[r]], col[crow[r] + 1] = t.col_indices()[crow[r] + 1], t.col_indices()[crow[r]]
    bad = torch.sparse_csr_tensor(t.crow_indices(), col, t.values(), size=x.shape)
    with pytest.raises(oem_amd.OemgpuError, match=f"column indices of row {r} are not strictly increasing") as e:
        oem_amd.SparseX(bad)
    assert e.value.code == -1
    # an uncoalesced COO tensor is coalesced by torch on the device: duplicates are summed there, as scipy sums them
    m = sp.coo_matrix(x)
    ind = torch.as_tensor(np.vstack([np.r_[m.row, m.row[:5]], np.r_[m.col, m.col[:5]]]).astype(np.int64), device="cuda")
    dup = torch.sparse_coo_tensor(ind, torch.as_tensor(np.r_[m.data, m.data[:5]], device="cuda"), size=x.shape)
    want = sp.csc_matrix((np.r_[m.data, m.data[:5]], (np.r_[m.row, m.row[:5]], np.r_[m.col, m.col[:5]])), shape=x.shape)
    with oem_amd.SparseX(dup) as a, oem_amd.SparseX(want) as b:
        _assert_same(a.export(), b.export(), "coo duplicates")


# ---------------------------------------------------------------------------------------------------- C, D: data
def _gauss(n, p, dens, seed):
    rng = np.random.default_rng(seed)
    x = sp.random(n, p, density=dens, format="csc", random_state=rng, data_rvs=lambda k: _f32(rng.normal(size=k) * 2.0 + 0.5))
    b = np.zeros(p); b[:5] = [1.5, -2.0, 1.0, 0.5, -1.0]
    y = x @ b + rng.normal(size=n)
    return x, y


def _fit_equal(f, g, label):
    assert f["d"] == g["d"], label
    for k in range(len(g["beta"])):
        for key in ("beta", "lambda", "niter", "loss"):
            assert np.array_equal(np.asarray(f[key][k]), np.asarray(g[key][k]), equal_nan=True), (label, key, k)


def _fit_close(f, g, label):
    assert abs(f["d"] - g["d"]) < 1e-10 * g["d"], label
    worst = 0.0
    for k in range(len(g["beta"])):
        assert np.allclose(f["lambda"][k], g["lambda"][k], rtol=1e-11, atol=0), (label, k)
        scale = max(1.0, float(np.abs(g["beta"][k]).max()))
        gap = float(np.abs(f["beta"][k] - g["beta"][k]).max()) / scale
        worst = max(worst, gap)
        assert gap < 1e-8, (label, k, gap)
        assert np.abs(np.ravel(f["niter"][k]).astype(int) - np.ravel(g["niter"][k]).astype(int)).max() <= 1, (label, k)
    print(f"GAP {label}: beta {worst:.1e} of max(1, |beta|_inf)")


# ---------------------------------------------------------------------------------------------------- C
def test_cv_oem_gaussian_gives_the_same_bits_on_either_handle():
    import oem_amd
    for (n, p, dens, icpt) in ((600, 20, 0.2, True), (60, 1500, 0.05, False)):
        x, y = _gauss(n, p, dens, n)
        fid = np.random.default_rng(1).permutation(np.resize(np.arange(1, 6), n))
        kw = dict(penalty=["lasso", "mcp"], foldid=fid, nlambda=12, intercept=icpt, keep=True)
        with oem_amd.SparseX(x) as a, oem_amd.SparseX(_tensor(x, "csr")) as b:
            fa, fb = oem_amd.cv_oem(a, y, **kw), oem_amd.cv_oem(b, y, **kw)
        ft = oem_amd.cv_oem(_tensor(x, "coo"), y, **kw)                                   # the tensor itself: a handle for the call
        for f in (fb, ft):
            for k in range(2):
                for key in ("cvm", "cvsd", "lambda"):
                    assert np.array_equal(f[key][k], fa[key][k]), (n, key, k)
                assert np.array_equal(f["fit.preval"][k], fa["fit.preval"][k], equal_nan=True)
            _fit_equal(f["oem.fit"], fa["oem.fit"], (n, "oem.fit"))
            assert f["lambda.min"] == fa["lambda.min"] and f["best.model"] == fa["best.model"]


def test_cv_oem_binomial_gives_the_same_bits_on_a_tensor():
    import oem_amd
    rng = np.random.default_rng(5)
    x, _ = _gauss(400, 12, 0.3, 6)
    y = (rng.uniform(size=400) < 1.0 / (1.0 + np.exp(-(x @ np.r_[1.0, -1.0, np.zeros(10)])))).astype(np.float64)
    fid = rng.permutation(np.resize(np.arange(1, 6), 400))
    kw = dict(family="binomial", penalty=["lasso", "mcp"], foldid=fid, nlambda=8, type_measure="deviance", keep=True)
    fa = oem_amd.cv_oem(x, y, **kw)
    for layout, it, vt in (("csr", "int32", "float32"), ("csc", "int64", "float64")):
        fb = oem_amd.cv_oem(_tensor(x, layout, it, vt), y, **kw)
        for k in range(2):
            for key in ("cvm", "cvsd", "lambda"):
                assert np.array_equal(fb[key][k], fa[key][k]), (layout, key, k)
            assert np.array_equal(fb["fit.preval"][k], fa["fit.preval"][k], equal_nan=True)
        _fit_equal(fb["oem.fit"], fa["oem.fit"], layout)


@pytest.mark.parametrize("ncol", [1, 33])
def test_predict_gives_the_same_bits_on_either_handle(ncol):
    import torch
    import oem_amd
    x, y = _gauss(700, 15, 0.2, 8)
    fit = oem_amd.oem(x, y, penalty=["lasso"], nlambda=40)
    s = None if ncol == 33 else [float(fit["lambda"][0][5])]
    if ncol == 33:
        fit = oem_amd.oem(x, y, penalty=["lasso"], nlambda=33)
    with oem_amd.SparseX(x) as a, oem_amd.SparseX(_tensor(x, "csc", "int32", "float32")) as b:
        pa, pb = oem_amd.predict(fit, a, s=s), oem_amd.predict(fit, b, s=s)
    pt = oem_amd.predict(fit, _tensor(x, "coo"), s=s)
    assert tuple(pa.shape) == (700, ncol) and pt.is_cuda
    assert torch.equal(pa, pb) and torch.equal(pa, pt)
    lam = float(fit["lambda"][0][3])
    cvfit = {"oem.fit": fit, "lambda.min": lam, "model.min": 1, "penalty": ["lasso"]}
    assert torch.equal(oem_amd.predict_cv(cvfit, _tensor(x, "csr")), oem_amd.predict(fit, _tensor(x, "csr"), s=lam))


# ---------------------------------------------------------------------------------------------------- D
GROUPS = np.repeat(np.arange(1, 6), 4)


@pytest.mark.parametrize("route", ["csc", "dense"])
@pytest.mark.parametrize("std,icpt", [(True, True), (True, False), (False, True), (False, False)])
def test_tall_fit_on_a_handle_and_on_a_tensor_is_oem_on_the_scipy_matrix(monkeypatch, route, std, icpt):
    import oem_amd
    monkeypatch.setenv("OEM_SPARSE_GRAM", route)
    x, y = _gauss(900, 20, 0.15, 31)
    kw = dict(penalty=["lasso", "grp.lasso"], groups=GROUPS, standardize=std, intercept=icpt, nlambda=15, tol=1e-10, maxit=2000, compute_loss=True)
    ref = oem_amd.oem(x, y, **kw)
    with oem_amd.SparseX(x) as sx:
        on_handle = oem_amd.oem_fit_sparse(sx, y, **kw)
        with pytest.raises(ValueError, match="oem\\(\\) on a SparseX is not built"):             # oem() itself keeps its sentence on a tall handle
            oem_amd.oem(sx, y, **kw)
    on_tensor = oem_amd.oem(_tensor(x, "csr", "int32", "float32"), y, **kw)
    via_entry = oem_amd.oem_fit_sparse(_tensor(x, "coo"), y, **kw)
    _fit_equal(on_tensor, on_handle, "tensor = handle")
    _fit_equal(via_entry, on_handle, "oem_fit_sparse(tensor) = handle")
    _fit_close(on_handle, ref, f"oem_fit_sparse(SparseX) {route} std={std} icpt={icpt}")
    assert on_handle["nobs"] == 900 and on_handle["nvars"] == 20 and list(on_handle["penalty"]) == ["lasso", "grp.lasso"]
    if not icpt:                         # intval = 1: the moments are the same kernel's on the same bytes, and so is everything after
        _fit_equal(on_handle, ref, f"bits, {route} std={std}")
    assert oem_amd.oem_fit_sparse(x, y, **kw)["d"] == ref["d"]                                   # a scipy x: oem()'s own route


def test_wide_fit_is_oem_on_the_handle_exactly():
    import torch
    import oem_amd
    x, y = _gauss(60, 1500, 0.05, 32)
    kw = dict(penalty=["lasso", "mcp"], intercept=False, nlambda=10, compute_loss=True)
    with oem_amd.SparseX(x) as sx:
        ref = oem_amd.oem(sx, y, **kw)
        _fit_equal(oem_amd.oem_fit_sparse(sx, y, **kw), ref, "wide handle")
        with pytest.raises(oem_amd.OemgpuError, match="p >= n and an intercept"):
            oem_amd.oem_fit_sparse(sx, y, penalty="lasso", nlambda=5)
    _fit_equal(oem_amd.oem(_tensor(x, "csc"), torch.as_tensor(y, device="cuda"), **kw), ref, "wide tensor")


def test_xval_on_a_handle_and_on_a_tensor_is_xval_on_the_scipy_matrix_exactly():
    import oem_amd
    x, y = _gauss(1200, 18, 0.15, 33)
    fid = np.random.default_rng(2).permutation(np.resize(np.arange(1, 7), 1200))
    for tm in ("mse", "mae"):
        kw = dict(penalty=["lasso", "scad"], foldid=fid, nlambda=12, type_measure=tm)
        ref = oem_amd.xval_oem(x, y, **kw)
        with oem_amd.SparseX(x) as sx:
            got = [oem_amd.xval_oem(sx, y, **kw)]
        got.append(oem_amd.xval_oem(_tensor(x, "csr", "int32", "float32"), y, **kw))
        for g in got:
            _fit_equal(g, ref, "xval")
            for k in range(2):
                assert np.array_equal(g["cvm"][k], ref["cvm"][k]) and np.array_equal(g["cvsd"][k], ref["cvsd"][k])
            assert g["lambda.min"] == ref["lambda.min"] and g["best.model"] == ref["best.model"]


def test_logistic_fit_on_a_handle_and_on_a_tensor_is_the_scipy_fit_exactly():
    import oem_amd
    rng = np.random.default_rng(9)
    x, _ = _gauss(500, 10, 0.3, 34)
    y = (rng.uniform(size=500) < 0.5).astype(np.float64)
    kw = dict(penalty=["lasso", "mcp"], nlambda=8, compute_loss=True)
    ref = oem_amd.oem_fit_logistic_sparse(x, y, **kw)
    with oem_amd.SparseX(_tensor(x, "coo")) as sx:
        _fit_equal(oem_amd.oem_fit_logistic_sparse(sx, y, **kw), ref, "logistic handle")
    g = oem_amd.oem_fit_logistic_sparse(_tensor(x, "csc", "int32", "float32"), y, **kw)
    _fit_equal(g, ref, "logistic tensor")
    assert g["family"] == "binomial" and g["nobs"] == 500


# ---------------------------------------------------------------------------------------------------- E
def _track_handles(monkeypatch):
    from oem_amd import api
    made = []
    init = api.SparseX.__init__

    def tracking(self, *a, **k):
        made.append(self)
        return init(self, *a, **k)
    monkeypatch.setattr(api.SparseX, "__init__", tracking)
    return made


def test_front_ends_close_their_handle_and_never_bring_x_to_the_host(monkeypatch):
    import torch
    import oem_amd
    x, y = _gauss(800, 14, 0.2, 41)
    yb = (y > np.median(y)).astype(np.float64)
    fid = np.random.default_rng(3).permutation(np.resize(np.arange(1, 6), 800))
    t = _tensor(x, "csr")
    fit = oem_amd.oem(x, y, penalty="lasso", nlambda=6)
    made = _track_handles(monkeypatch)
    cpu = torch.Tensor.cpu
    sizes = {x.nnz, 2 * x.nnz, x.shape[0] + 1}                   # values / column indices, COO indices, row pointers

    def guarded(self, *a, **k):
        assert self.layout == torch.strided and self.numel() not in sizes, "x was copied to the host"
        return cpu(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", guarded)
    monkeypatch.setattr(torch.Tensor, "to_dense", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("x was densified")))
    calls = [lambda: oem_amd.oem(t, y, penalty="lasso", nlambda=6),
             lambda: oem_amd.oem_fit_sparse(t, y, penalty="lasso", nlambda=6),
             lambda: oem_amd.oem_fit_logistic_sparse(t, yb, penalty="lasso", nlambda=6),
             lambda: oem_amd.xval_oem(t, y, penalty="lasso", nlambda=6, foldid=fid),
             lambda: oem_amd.cv_oem(t, y, penalty="lasso", nlambda=6, foldid=fid),
             lambda: oem_amd.cv_oem(t, yb, family="binomial", penalty="lasso", nlambda=6, foldid=fid),
             lambda: oem_amd.predict(fit, t),
             lambda: oem_amd.predict_cv({"oem.fit": fit, "lambda.min": float(fit["lambda"][0][2]), "model.min": 1, "penalty": ["lasso"]}, t),
             lambda: oem_amd.predict_xval(dict(fit, **{"lambda.min": float(fit["lambda"][0][2]), "model.min": 1, "cvm": [0]}), t)]
    for i, call in enumerate(calls):
        del made[:]
        call()
        assert len(made) == 1 and made[0].closed, i
    # every refusal of the handle routes closes it too
    refusals = [(lambda: oem_amd.cv_oem(t, y, penalty=["lasso", "ols"], foldid=fid), ValueError, "\"ols\" penalty is not served"),
                (lambda: oem_amd.cv_oem(t, y, penalty="lasso", foldid=fid, ngpus=2), ValueError, "not split over devices"),
                (lambda: oem_amd.oem(t, y, penalty="lasso", ngpus=2), ValueError, "not split over devices"),
                (lambda: oem_amd.xval_oem(t, y, penalty="lasso", foldid=fid, weights=np.ones(800)), ValueError, "need a dense x"),
                (lambda: oem_amd.xval_oem(t, y, penalty="lasso", foldid=fid, ngpus=2), ValueError, "not split over devices"),
                (lambda: oem_amd.oem(t, y[:-1], penalty="lasso"), ValueError, "x and y lengths do not match"),
                (lambda: oem_amd.oem_fit_logistic_sparse(t, yb, penalty="lasso", standardize=False), oem_amd.OemgpuError, "standardize")]
    for i, (call, exc, text) in enumerate(refusals):
        del made[:]
        with pytest.raises(exc, match=text):
            call()
        assert len(made) <= 1 and all(m.closed for m in made), i
    with pytest.raises(ValueError, match="weights not implemented yet"):
        oem_amd.oem(t, y, weights=np.ones(800))
    with pytest.raises(ValueError, match="weights not implemented yet"):
        oem_amd.cv_oem(t, y, weights=np.ones(800))
    wide = _tensor(_gauss(40, 900, 0.05, 42)[0], "csr")
    del made[:]
    with pytest.raises(oem_amd.OemgpuError, match="p >= n and an intercept"):
        oem_amd.oem(wide, np.zeros(40), penalty="lasso", nlambda=4)
    assert len(made) == 1 and made[0].closed


def test_what_sparsex_does_not_take_says_why():
    import torch
    import oem_amd
    bsr = torch.sparse_bsr_tensor(torch.tensor([0, 1, 2]), torch.tensor([0, 1]), torch.ones(2, 2, 2, dtype=torch.float64), size=(4, 4)).cuda()
    with pytest.raises(ValueError, match="layout torch.sparse_bsr is not served"):
        oem_amd.SparseX(bsr)
    bsc = torch.sparse_bsc_tensor(torch.tensor([0, 1, 2]), torch.tensor([0, 1]), torch.ones(2, 2, 2, dtype=torch.float64), size=(4, 4)).cuda()
    with pytest.raises(ValueError, match="layout torch.sparse_bsc is not served"):
        oem_amd.SparseX(bsc)
    ind = torch.tensor([[0, 1], [1, 2]], device="cuda")
    for dt in (torch.float16, torch.int64):
        with pytest.raises(ValueError, match="float64 or float32"):
            oem_amd.SparseX(torch.sparse_coo_tensor(ind, torch.ones(2, dtype=dt, device="cuda"), size=(3, 3)))
    with pytest.raises(ValueError, match="not one of 3 dimensions"):
        oem_amd.SparseX(torch.sparse_coo_tensor(torch.tensor([[0, 1], [1, 2], [0, 0]], device="cuda"), torch.ones(2, dtype=torch.float64, device="cuda"),
                                                size=(3, 3, 2)))
    with pytest.raises(TypeError, match="x must be a scipy.sparse matrix"):
        oem_amd.SparseX(torch.zeros(4, 3, device="cuda"))
    # a host tensor takes the scipy route
    x = _case("empty_lines")
    with oem_amd.SparseX(_tensor(x, "csr", device="cpu")) as a:
        _assert_same(a.export(), _reference("empty_lines"), "host tensor")
    sx = oem_amd.SparseX(_tensor(x, "csr"))
    sx.close()
    with pytest.raises(ValueError, match="this SparseX is closed"):
        sx.to_scipy()
