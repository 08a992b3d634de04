"""xval.oem on a sparse x without a device: the host plan (oemgpu_selftest_xval_sparse_plan -- the function the call itself takes its
shape from) over a sweep of shapes, and the argument checks of oem_amd.xval_oem that stop before the library is called.

The plan is checked for what the kernels rely on:
  * the route is sparse_route's (the rule of oemgpu_fit_sparse: the Gram kernel's LDS fits 160 KB, nnz <= 2 % of n p, n < 2^31), the
    same answer oemgpu_selftest_logistic_sparse_plan gives;
  * no chunk range and no tile spans a fold boundary.  Fold segments start on multiples of out[10] = 8192 rows, so a fold is whole
    chunks; the worst case for one fold -- n - K + 1 rows in fold 1, one row in each of the others -- is cut by the function the call
    uses and must end fold 1's last range exactly at fold 1's last chunk, with no more ranges per fold, ranges and chunks than the
    bounds the buffers are sized by.  Tiles are multiples of 64 rows (or the whole matrix), are laid from a fold's first row and the
    last one is cut at the fold's last row (csc_tiles / csc_tile_rows, the functions csc_tile_moments walks: out[16], out[17]);
  * on the compressed-column route the device bytes stay under a bound linear in n, nnz, K p^2 and K npen nl p -- nothing of n p
    doubles -- with the terms written out in _bound below.
"""
import ctypes as C

import numpy as np
import pytest

CH = 8192


@pytest.fixture(scope="module")
def api():
    from oem_amd import api
    return api


def _bound(n, p, nnz, K, npen, nl):
    """Device bytes of the call on the compressed-column route, term by term (oem_amd/csrc/api.hip: xval_layout's sparse form, and
    xval_sparse.hip: xval_sparse_plan).
      rows      40 n: positions 4, y twice 16, foldid 4, row pointers 8, layout block counts K / 256 <= 2, chunk pointers p / 2048 <= 3
                (p <= 6140 where the Gram kernel fits LDS)
      entries   40 (nnz + 1): row indices and values three times (as uploaded, in fold order, as compressed rows): 3 (4 + 8) = 36
      folds     56 K (p + 2)^2: fold moments 8, leave-one-out sums 8 (K + 1) / K <= 12, their sum <= 4, the range sums of the Gram
                kernel (at most 2 K + 1 ranges beyond the 256 MB it may spend on more) <= 20, column offsets and sums per fold
      tables    16 K npen nl16 (p + 1): the fold coefficients and their transposed copy
      padding   131072 K: 8192 padding rows per fold in y and the row pointers
      partials  131072 npen nl16: at most 4096 waves x 4 doubles
      fixed     512 MB of range sums at most where K p^2 leaves room, 64 KB of granules"""
    nl16 = (nl + 15) // 16 * 16
    return (40 * n + 40 * (nnz + 1) + 56 * K * (p + 2) ** 2 + 16 * K * npen * nl16 * (p + 1) + 131072 * (K + npen * nl16) + 512 * 10 ** 6
            + 65536)


def _route_rule(n, p, nnz):
    return (CH * 8 + 16 * p + 64 <= 160 * 1024) and nnz <= 0.02 * n * p and n < 2 ** 31


def test_plan_sweep(api):
    import oem_amd
    lib = oem_amd.lib()
    out8 = (C.c_int64 * 8)()
    seen = set()
    for n in (600, 8192, 24577, 250_000, 3_000_000):
        for p in (2, 41, 130, 200, 2000):
            if p >= n:
                continue
            for dens in (0.001, 0.01, 0.03, 0.1):
                nnz = int(dens * n * p)
                for K in (2, 3, 10, 130, 512):
                    for cu, npen, nl in ((64, 1, 21), (256, 1, 100), (304, 3, 65)):
                        d = api.xval_sparse_plan(n, p, nnz, K, npen, nl, cu)
                        tag = (n, p, nnz, K, cu)
                        assert d["csc"] == _route_rule(n, p, nnz), tag
                        assert lib.oemgpu_selftest_logistic_sparse_plan(n, p, nnz, 1, cu, out8) == 0 and bool(out8[0]) == d["csc"], tag
                        seen.add(d["csc"])
                        # ---- fold boundaries
                        assert d["align"] == CH and d["chunks_max"] == n // CH + K
                        per = d["chunks_per_range"]
                        assert per >= 1
                        sizes = [n - K + 1] + [1] * (K - 1) if n >= K else [n] + [0] * (K - 1)
                        chunks = [-(-s // CH) for s in sizes]
                        assert d["worst_rows"] == CH * sum(chunks) <= CH * d["chunks_max"]
                        assert d["worst_fold_end_chunk"] == chunks[0], tag                 # fold 1's last range ends where fold 1 does
                        assert d["worst_fold_ranges"] == -(-chunks[0] // per) <= d["ranges_per_fold_max"], tag
                        assert d["worst_ranges"] == sum(-(-c // per) for c in chunks) <= d["ranges_max"] <= d["chunks_max"], tag
                        # any folds at all: a fold of c chunks is ceil(c / per) ranges, and the sum stays inside the bound
                        for sizes in ([n // K + (i < n % K) for i in range(K)], [n] + [0] * (K - 1)):
                            ch = [-(-s // CH) for s in sizes]
                            assert sum(ch) <= d["chunks_max"] and sum(-(-c // per) for c in ch) <= d["ranges_max"], tag
                            assert max(-(-c // per) for c in ch) <= d["ranges_per_fold_max"], tag
                        # ---- tiles: from a fold's first row in steps of tile_rows, which the MFMA pass wants as multiples of 64
                        assert 1 <= d["tile_rows"] <= n and (d["tile_rows"] % 64 == 0 or d["tile_rows"] == n), tag
                        assert d["tile_rows"] * p * 8 <= 2 ** 31
                        n1 = n - K + 1 if n >= K else n                                    # fold 1 of the worst case, tiled by the call's function
                        assert d["worst_fold_tiles"] == -(-n1 // d["tile_rows"]) and d["worst_fold_tile_end"] == n1, tag
                        assert (d["worst_fold_tiles"] - 1) * d["tile_rows"] < n1                   # the last tile starts inside the fold
                        # ---- the CV-error launch
                        assert d["cv_lblk"] == -(-nl // 64) and d["cv_waves"] == 4 * d["cv_nwg"] and 1 <= d["cv_nwg"] <= 1024
                        assert d["cv_nwg"] <= max(1, 4 * cu // (npen * d["cv_lblk"]))
                        # ---- the workspace
                        if d["csc"]:
                            assert d["gram_lds"] == CH * 8 + 16 * p + 64
                            assert d["bytes"] <= _bound(n, p, nnz, K, npen, nl), (tag, d["bytes"], _bound(n, p, nnz, K, npen, nl))
    assert seen == {True, False}


def test_workspace_of_a_large_sparse_design_is_far_below_the_dense_copy(api):
    n, p, nnz = 10 ** 7, 200, 2 * 10 ** 7
    d = api.xval_sparse_plan(n, p, nnz, 10, 1, 100, 256)
    assert d["csc"]
    assert d["bytes"] <= _bound(n, p, nnz, 10, 1, 100) < 8 * n * p
    assert d["bytes"] < 8 * n * p


def test_limits(api):
    from oem_amd import OemgpuError
    K = 10
    nmax = 2 ** 31 - CH * K                                     # n + 8192 K >= 2^31 is refused
    with pytest.raises(OemgpuError, match="too large for 32-bit row positions") as e:
        api.xval_sparse_plan(nmax, 50, 10 ** 6, K, 1, 10, 256)
    assert e.value.code == -4
    assert api.xval_sparse_plan(nmax - 1, 50, 10 ** 6, K, 1, 10, 256)["chunks_max"] == (nmax - 1) // CH + K
    for bad in ((0, 5, 1, 3, 1, 1, 256), (10, 0, 1, 3, 1, 1, 256), (10, 5, -1, 3, 1, 1, 256), (10, 5, 1, 1, 1, 1, 256),
                (10, 5, 1, 513, 1, 1, 256), (10, 5, 1, 3, 0, 1, 256), (10, 5, 1, 3, 1, 0, 256), (10, 5, 1, 3, 1, 1, 0)):
        with pytest.raises(OemgpuError) as e:
            api.xval_sparse_plan(*bad)
        assert e.value.code == -1


def test_forced_routes_show_in_the_plan(api, monkeypatch):
    monkeypatch.setenv("OEM_SPARSE_GRAM", "dense")
    monkeypatch.setenv("OEM_SPARSE_TILE_ROWS", "1024")
    d = api.xval_sparse_plan(24577, 41, 15000, 4, 1, 21, 256)
    assert not d["csc"] and d["tile_rows"] == 1024 and d["gram_lds"] == 0
    monkeypatch.setenv("OEM_SPARSE_GRAM", "csc")
    d = api.xval_sparse_plan(24577, 41, 10 ** 6, 4, 1, 21, 256)  # denser than the rule takes, forced
    assert d["csc"]


# ------------------------------------------------------------------------------------------------ Python argument checks, no device
def _design(n=60, p=5, seed=0):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    x = sp.random(n, p, density=0.3, format="csc", random_state=np.random.RandomState(seed))
    return x, rng.normal(size=n), np.resize(np.arange(1, 4), n)


def test_weights_and_devices_need_a_dense_x():
    import oem_amd
    x, y, fid = _design()
    with pytest.raises(ValueError, match="observation weights of xval.oem need a dense x"):
        oem_amd.xval_oem(x, y, foldid=fid, weights=np.ones(60))
    with pytest.raises(ValueError, match="ngpus / devices of xval.oem need a dense x"):
        oem_amd.xval_oem(x, y, foldid=fid, ngpus=2)
    with pytest.raises(ValueError, match="ngpus / devices of xval.oem need a dense x"):
        oem_amd.xval_oem(x.tocsr(), y, foldid=fid, devices=[0])


def test_the_dense_calls_checks_come_first_and_unchanged():
    import oem_amd
    import scipy.sparse as sp
    x, y, fid = _design()
    with pytest.raises(ValueError, match="number of observations must be greater than the number of variables"):
        oem_amd.xval_oem(sp.csc_matrix(np.ones((4, 5))), np.ones(4), foldid=[1, 2, 3, 1])
    with pytest.raises(ValueError, match="binomial models not yet supported for xval, use cv.oem\\(\\) instead"):
        oem_amd.xval_oem(x, y, foldid=fid, family="binomial")
    with pytest.raises(ValueError, match="nfolds must be bigger than 3"):
        oem_amd.xval_oem(x, y, foldid=np.resize(np.arange(1, 3), 60))
    with pytest.raises(ValueError, match="x and y lengths do not match"):
        oem_amd.xval_oem(x, y[:-1], foldid=fid)
    with pytest.raises(ValueError, match="groups must have same length as number of columns in x"):
        oem_amd.xval_oem(x, y, foldid=fid, penalty="grp.lasso", groups=[1, 1, 2])
    with pytest.raises(ValueError, match="penalty.factor must have same length"):
        oem_amd.xval_oem(x, y, foldid=fid, penalty_factor=[1.0, 1.0])


def test_malformed_columns_are_refused_before_a_device_is_looked_for():
    """csc_check runs first, as in oemgpu_fit_sparse: OEMGPU_ERR_ARG (-1), not 'no HIP device' (-2), on a machine without a GPU too"""
    import oem_amd
    lib = oem_amd.lib()
    n, p, K = 12, 3, 3
    colptr = np.array([0, 2, 3, 4], dtype=np.int64)
    rowidx = np.array([5, 2, 1, 0], dtype=np.int32)              # column 0 not increasing
    vals = np.ones(4)
    y = np.ones(n); fid = np.resize(np.arange(1, K + 1), n).astype(np.int32)
    out = np.zeros(K * (p + 2) ** 2)
    rc = lib.oemgpu_selftest_xval_sparse_fold_moments(n, p, colptr.ctypes.data, rowidx.ctypes.data, vals.ctypes.data, y.ctypes.data,
                                                      fid.ctypes.data, K, out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == -1 and b"not strictly increasing" in lib.oemgpu_last_error()
    # ... before the other argument checks too: the same arrays with nfolds = 1 still name the column
    rc = lib.oemgpu_selftest_xval_sparse_fold_moments(n, p, colptr.ctypes.data, rowidx.ctypes.data, vals.ctypes.data, y.ctypes.data,
                                                      fid.ctypes.data, 1, out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == -1 and b"not strictly increasing" in lib.oemgpu_last_error()
    rowidx[:2] = [2, 5]                                          # well-formed now: the next check speaks
    rc = lib.oemgpu_selftest_xval_sparse_fold_moments(n, p, colptr.ctypes.data, rowidx.ctypes.data, vals.ctypes.data, y.ctypes.data,
                                                      fid.ctypes.data, 1, out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == -1 and b"nfolds must be in 2..512" in lib.oemgpu_last_error()
