"""xval.oem on a sparse x (oemgpu_xval_sparse, oem_amd/csrc/xval_sparse.hip) on the MI355X: the fold-ordered compressed columns and the
K fold moment buffers against numpy in long double, the CV-error kernel over the compressed rows alone with dense random coefficient
tables (fitted tables hide swapped indices: tests/test_gpu_xval_bounds.py), and the whole call against the CPU restatement of
ref src/oem_xval_dense.{h,cpp} on x.toarray().

Shapes: n = 24,577 is three 8192-row chunks and one row, p = 41 is odd (csc_gram_kernel's middle column), density 1.5 % leaves about
half of the rows without a non-zero; the contiguous folds 8192 / 8193 / 17 / 8175 are exactly one chunk, one chunk and a row (two
chunk ranges), a fold most columns miss, and a ragged last one.  p = 130 is more than 64 columns b per workgroup of the Gram kernel and
more than 128 columns.  Both routes run: OEM_SPARSE_GRAM=csc, and =dense with OEM_SPARSE_TILE_ROWS=1024 (several tiles per fold).

Fold moments.  Bound per entry: m 2^-53 sum |terms|, m the number of non-zero terms summed into the entry -- the sequential-summation
bound, which holds for any order of the adds (exact zeros add no error); an entry without terms is exactly 0.  y holds multiples of
2^-10, so sum y and n_k are exact in any order and must match to the bit.
CV error: cvm 1e-12, cvsd 1e-11 relative against long double (the tolerances of tests/test_gpu_xval_bounds.py).
The CV-error selftest takes a coefficient table and no penalties, so it masks nothing: an `ols` member's use of lambda slot 0 only is
host code after the kernel and is checked end to end alone (test_parity_p41: penalties lasso / mcp / ols, one cvm entry for ols, equal to
the restatement's).
End to end: the tolerances of tests/test_gpu_xval.py::_compare; niter within 1 of the restatement's, because the moments differ from
the dense pass in their last bits."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.test_gpu_xval import _compare, _oracle
from tests.test_gpu_xval_bounds import LD, RTOL_M, RTOL_S, _errors, _gap, _meets, _moments

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CH = 8192
ROUTES = [("csc", None), ("dense", 1024)]
CONTIG = (8192, 8193, 17, 8175)


@pytest.fixture(scope="module")
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def api():
    from oem_amd import api
    return api


def _route(monkeypatch, route, tile_rows):
    for name, val in (("OEM_SPARSE_GRAM", route), ("OEM_SPARSE_TILE_ROWS", tile_rows)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))


# ------------------------------------------------------------------------------------------------------------- designs
@functools.lru_cache(maxsize=None)
def _design(n, p, dens, seed, empty_ends=False):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    mask = rng.random((n, p)) < dens
    if empty_ends:
        mask[:, 0] = False; mask[:, -1] = False
    xd = np.where(mask, rng.normal(size=(n, p)) * 1.5 + 0.25, 0.0)
    beta = np.zeros(p); beta[1:6] = [2.0, -1.5, 1.0, 0.5, -2.5]
    y = np.round((xd @ beta + rng.normal(size=n) + 0.4) * 1024.0) / 1024.0          # multiples of 2^-10: sums of y are exact
    x = sp.csc_matrix(xd)
    x.sort_indices()
    xd.setflags(write=False); y.setflags(write=False)
    return x, xd, y


def _folds(kind, n, seed=3):
    rng = np.random.default_rng(seed)
    if kind == "contig":
        assert sum(CONTIG) == n
        return np.repeat(np.arange(1, 5), CONTIG), 4
    if kind == "k5":
        return rng.permutation(np.resize(np.arange(1, 6), n)), 5
    if kind == "k5_no4":
        f = rng.permutation(np.resize(np.arange(1, 6), n))
        f[f == 4] = 5
        return f, 5
    if kind == "k4":
        return rng.permutation(np.resize(np.arange(1, 5), n)), 4
    if kind == "k3":
        return rng.permutation(np.resize(np.arange(1, 4), n)), 3
    if kind == "k130":                                           # fold 7 has one row, fold 99 none
        f = rng.permutation(np.resize(np.arange(1, 131), n))
        f[f == 99] = 98
        seven = np.nonzero(f == 7)[0]
        f[seven[1:]] = 8
        return f, 130
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _moment_reference(n, p, dens, seed, empty_ends, kind):
    """per fold, in long double on the dense copy's rows: M = Z'Z for Z = [X | y | 1], sum |terms|, and the number of non-zero terms"""
    _, xd, y = _design(n, p, dens, seed, empty_ends)
    fid, K = _folds(kind, n)
    z = np.column_stack([xd, y, np.ones(n)])
    M, A, T = [], [], []
    for k in range(1, K + 1):
        zk = z[fid == k]
        zl = zk.astype(LD)
        M.append(zl.T @ zl)
        A.append(np.abs(zl).T @ np.abs(zl))
        nz = (zk != 0).astype(np.float64)
        T.append(nz.T @ nz)                                     # integers: exact
    return np.stack(M), np.stack(A), np.stack(T), fid, K


MOMENT_CASES = [(24577, 41, 0.015, 1, False, "contig"), (24577, 41, 0.015, 1, True, "contig"), (24577, 41, 0.015, 1, False, "k5"),
                (24577, 41, 0.015, 1, False, "k5_no4"), (16500, 130, 0.01, 2, False, "k4")]


def _assert_lands(api, num_cu, n, p, nnz, K, route, tile_rows, fid):
    d = api.xval_sparse_plan(n, p, nnz, K, 1, 1, num_cu)
    assert d["csc"] == (route == "csc"), d
    sizes = np.bincount(fid, minlength=K + 1)[1:]
    if route == "csc":
        assert d["chunks_per_range"] == 1                        # so a fold of two chunks is two ranges, added in range order
    else:
        assert d["tile_rows"] == tile_rows and sizes.max() > 2 * tile_rows      # several tiles per fold
    return d


@pytest.mark.parametrize("route,tile_rows", ROUTES)
@pytest.mark.parametrize("n,p,dens,seed,empty_ends,kind", MOMENT_CASES)
def test_fold_moments(api, num_cu, monkeypatch, n, p, dens, seed, empty_ends, kind, route, tile_rows):
    x, xd, y = _design(n, p, dens, seed, empty_ends)
    M, A, T, fid, K = _moment_reference(n, p, dens, seed, empty_ends, kind)
    _route(monkeypatch, route, tile_rows)
    _assert_lands(api, num_cu, n, p, x.nnz, K, route, tile_rows, fid)
    if kind == "contig":
        assert [-(-s // CH) for s in CONTIG] == [1, 2, 1, 1]
    if empty_ends:
        assert x.indptr[1] == 0 and x.indptr[-1] == x.indptr[-2]
    got = api.xval_sparse_fold_moments(x, y, fid, K)
    assert got.shape == (K, p + 2, p + 2) and np.all(np.isfinite(got))
    err = np.abs(got.astype(LD) - M)
    bound = T.astype(LD) * U * A
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))
    print(f"GAP fold moments {kind} {route}: worst error / bound {worst:.3f}")
    assert np.all(err <= bound), (kind, route, worst, np.argwhere(err > bound)[:5])
    sizes = np.bincount(fid, minlength=K + 1)[1:]
    for k in range(K):
        assert got[k, p + 1, p + 1] == sizes[k]                  # n_k
        assert got[k, p, p + 1] == float(M[k, p, p + 1]) and got[k, p + 1, p] == got[k, p, p + 1]      # sum y: exact
        assert np.array_equal(got[k], got[k].T)
        if sizes[k] == 0:
            assert not got[k].any()
    if kind == "k5_no4":
        assert sizes[3] == 0 and got[3].tobytes() == np.zeros((p + 2, p + 2)).tobytes()
    # two calls give the same bytes
    assert api.xval_sparse_fold_moments(x, y, fid, K).tobytes() == got.tobytes()
    # the K buffers added in fold order are the moments of the whole matrix, within the same bound over all rows
    total = np.zeros((p + 2, p + 2))
    for k in range(K):
        total = total + got[k]
    assert np.all(np.abs(total.astype(LD) - M.sum(axis=0)) <= T.sum(axis=0).astype(LD) * U * A.sum(axis=0))


def test_fold_ids_outside_the_folds_are_the_dense_calls_error(api):
    from oem_amd import OemgpuError
    x, xd, y = _design(24577, 41, 0.015, 1, False)
    fid, K = _folds("k5", 24577)
    bad = fid.copy(); bad[11] = 6
    with pytest.raises(OemgpuError, match="foldid must hold values in 1..nfolds") as e:
        api.xval_sparse_fold_moments(x, y, bad, K)
    assert e.value.code == -1
    bad[11] = 0
    with pytest.raises(OemgpuError, match="foldid must hold values in 1..nfolds"):
        api.xval_sparse_fold_moments(x, y, bad, K)


# ------------------------------------------------------------------------------------------------------------- CV error alone
def _table(K, npen, nl, p, seed):
    return np.random.default_rng(seed).normal(size=(K, npen, nl, p + 1)) / np.sqrt(p + 1.0)


def _cv_reference(xd, y, fid, coef, measure):
    """(cvm, cvsd, M2) in long double; numpy's own float64 lies within 1e-13 of it, and tables with the folds, the lambdas or the
    penalties rolled by one, or without the intercepts, move every cvm by more than 1e-6 -- a wrong index would show"""
    cvm, cvsd, m2 = _moments(_errors(xd, y, fid, coef, measure, None, LD))
    c64, s64, _ = _moments(_errors(xd, y, fid, coef, measure, None, np.float64))
    assert _gap(c64, cvm) < 1e-13 and _gap(s64, cvsd) < 1e-13
    K, npen, nl, _ = coef.shape
    present = np.unique(fid)
    wrong = {"folds rolled": coef[np.roll(np.arange(K), 1)] if len(present) == K else None}
    t = coef.copy(); t[..., 0] = 0.0; wrong["intercept zeroed"] = t
    if nl > 1:
        wrong["lambdas rolled"] = np.roll(coef, 1, axis=2)
    if npen > 1:
        wrong["penalties rolled"] = np.roll(coef, 1, axis=1)
    for name, tab in wrong.items():
        if tab is None:
            continue
        moved = np.abs(_moments(_errors(xd, y, fid, tab, measure, None, np.float64))[0] - c64) / c64
        assert moved.min() > 1e-6, (name, float(moved.min()))
    return cvm, cvsd, m2


CV_CASES = [  # design (n, p, dens, seed, empty_ends), folds, npen, nl, measure
    ((24577, 41, 0.015, 1, False), "contig", 1, 21, "mse"),
    ((24577, 41, 0.015, 1, False), "k3", 3, 65, "mae"),
    ((24577, 41, 0.015, 1, False), "k130", 1, 100, "mse"),
    ((24577, 41, 0.015, 1, True), "k5_no4", 1, 1, "mae"),
    ((16500, 130, 0.01, 2, False), "k4", 3, 64, "mse"),
]


@pytest.mark.parametrize("design,kind,npen,nl,measure", CV_CASES)
def test_cv_error_alone(api, num_cu, design, kind, npen, nl, measure):
    x, xd, y = _design(*design)
    n, p = xd.shape
    fid, K = _folds(kind, n)
    sizes = np.bincount(fid, minlength=K + 1)[1:]
    if kind == "k130":
        assert sizes[6] == 1 and sizes[98] == 0                 # a fold of one row, an empty fold
    if p == 41:
        empty_rows = float(np.mean(np.diff(x.tocsr().indptr) == 0))
        assert 0.4 < empty_rows < 0.65, empty_rows               # about half of the rows have no non-zero: eta = the intercept
    d = api.xval_sparse_plan(n, p, x.nnz, K, npen, nl, num_cu)
    assert d["cv_lblk"] == -(-nl // 64) and d["cv_waves"] == 4 * d["cv_nwg"]
    coef = _table(K, npen, nl, p, 100 + nl)
    ref = _cv_reference(xd, y, fid, coef, measure)
    cvm, cvsd = api.xval_sparse_cv_error(x, y, fid, K, coef, measure)
    _meets(cvm, cvsd, ref, f"sparse {kind} npen {npen} nl {nl} {measure}")
    tri = api.xval_sparse_cv_error(x, y, fid, K, coef, measure, triples=True)
    assert tri.shape == (npen, nl, 3) and np.all(tri[..., 0] == n)          # the padding rows between fold segments do not count
    assert _gap(tri[..., 1], ref[0]) <= RTOL_M and _gap(tri[..., 2], ref[2]) <= RTOL_S


def test_cv_triples_merge(api):
    """(count, mean, M2) of two unequal row sets, each a call of its own, merged by oemgpu_xval_merge"""
    import oem_amd
    x, xd, y = _design(24577, 41, 0.015, 1, False)
    n, p = xd.shape
    fid, K = _folds("k3", n)
    nl = 21
    coef = _table(K, 1, nl, p, 7)
    ref = _cv_reference(xd, y, fid, coef, "mse")
    cut = 9001
    xr = x.tocsr()
    sets = []
    for rows in (slice(0, cut), slice(cut, n)):
        sets.append(api.xval_sparse_cv_error(xr[rows].tocsc(), y[rows], fid[rows], K, coef, "mse", triples=True))
        assert np.all(sets[-1][..., 0] == len(y[rows]))
    a = api._Args(["lasso"], [], nl, 1e-4, 1.0, 3.0, 0.5, 1e-7, 500, False, False, np.ones(p), np.zeros(0, np.int32), np.zeros(0, np.int32),
                  np.zeros(0))
    both = np.ascontiguousarray(np.stack(sets))
    cvm, cvsd = np.zeros((1, nl)), np.zeros((1, nl))
    dp = C.POINTER(C.c_double)
    assert oem_amd.lib().oemgpu_xval_merge(both.ctypes.data_as(dp), 2, C.byref(a.c), cvm.ctypes.data_as(dp), cvsd.ctypes.data_as(dp)) == 0
    _meets(cvm, cvsd, ref, "sparse merged row sets")


# ------------------------------------------------------------------------------------------------------------- end to end
def _min_index(lam, cvm):
    """the index getmin (R/utils.R:3-26) picks: the largest lambda among the minimisers"""
    lam = np.asarray(lam)[:len(cvm)]
    lmin = np.max(lam[cvm <= np.min(cvm)])
    return int(np.nonzero(lam == lmin)[0][0])


def _end_to_end(f, r, npen, loss):
    _compare(f, r, npen)
    for k in range(npen):
        nf, nr = np.ravel(f["niter"][k]), np.ravel(r["niter"][k])
        assert np.max(np.abs(nf.astype(int) - nr.astype(int))) <= 1, (k, nf, nr)
        if loss:
            assert np.allclose(np.ravel(f["loss"][k]), np.ravel(r["loss"][k]), rtol=1e-9)
        assert _min_index(f["lambda"][k], f["cvm"][k]) == _min_index(r["lambda"][k], r["cvm"][k])
        assert f["lambda.min.models"][k] == f["lambda"][k][_min_index(f["lambda"][k], f["cvm"][k])]


@functools.lru_cache(maxsize=None)
def _oracle_41(std, icpt):
    _, xd, y = _design(24577, 41, 0.015, 1, False)
    fid, _ = _folds("k5", 24577)
    r = _oracle(np.asfortranarray(xd), np.array(y), fid, ["lasso", "mcp", "ols"], intercept=icpt, standardize=std, nlambda=21, tol=1e-9,
                maxit=5000, compute_loss=True, lambda_min_ratio=1e-4)
    assert max(int(np.max(v)) for v in r["niter"]) < 5000       # no fit reaches the cap
    return r


@pytest.mark.parametrize("route,tile_rows", ROUTES)
@pytest.mark.parametrize("std,icpt", [(True, True), (False, True), (True, False), (False, False)])
def test_parity_p41(api, num_cu, monkeypatch, std, icpt, route, tile_rows):
    import oem_amd
    x, xd, y = _design(24577, 41, 0.015, 1, False)
    fid, K = _folds("k5", 24577)
    r = _oracle_41(std, icpt)
    _route(monkeypatch, route, tile_rows)
    _assert_lands(api, num_cu, 24577, 41, x.nnz, K, route, tile_rows, fid)
    f = oem_amd.xval_oem(x, y, foldid=fid, penalty=["lasso", "mcp", "ols"], intercept=icpt, standardize=std, nlambda=21, tol=1e-9, maxit=5000,
                         compute_loss=True)
    _end_to_end(f, r, 3, True)
    assert len(f["cvm"][2]) == 1                                 # ols: lambda slot 0 only


P130 = [  # name, intercept, penalties, measure, extra
    ("lasso", True, ["lasso"], "mse"), ("mae no intercept", False, ["lasso"], "mae"), ("groups", True, ["grp.lasso"], "mse"),
    ("user lambda", True, ["elastic.net", "scad"], "mse"),
]


@pytest.mark.parametrize("name,icpt,pens,measure", P130)
def test_parity_p130(api, num_cu, monkeypatch, name, icpt, pens, measure):
    import oem_amd
    n, p = 16500, 130
    x, xd, y = _design(n, p, 0.01, 2, False)
    fid, K = _folds("k4", n)
    kw = dict(tol=1e-9, maxit=2000, standardize=True, type_measure=measure)
    if name == "user lambda":
        kw.update(lambda_=[np.geomspace(0.5, 1e-3, 33), np.geomspace(1.0, 5e-3, 33)], alpha=0.7)
    else:
        kw.update(nlambda=65)
    groups = np.arange(p) // 10 + 1 if name == "groups" else None
    okw = dict(kw) if name == "user lambda" else dict(kw, lambda_min_ratio=1e-4)
    r = _oracle(np.asfortranarray(xd), np.array(y), fid, pens, groups=groups, intercept=icpt, **okw)
    assert max(int(np.max(v)) for v in r["niter"]) < 2000
    _route(monkeypatch, None, None)
    assert api.xval_sparse_plan(n, p, x.nnz, K, len(pens), 65, num_cu)["csc"]
    f = oem_amd.xval_oem(x, y, foldid=fid, penalty=pens, intercept=icpt, **(dict(kw, groups=groups) if groups is not None else kw))
    _end_to_end(f, r, len(pens), False)


@pytest.mark.parametrize("no_coop", [False, True])
def test_parity_p300_and_predict(api, num_cu, monkeypatch, no_coop):
    """q = 301 is beyond the one-workgroup batched launch (288).  As the library stands, the K + 1 = 4 fits then share one launch of the
    cooperating engine (10 workgroups each: they fit beside each other); with OEM_NO_COOP set that engine is off and the fold fits
    run on child contexts, one thread each, over the sparse layout's moment buffers -- both ways through xval_solve are run."""
    import oem_amd
    import scipy.sparse as sp
    n, p = 20000, 300
    x, xd, y = _design(n, p, 0.01, 5, False)
    fid, K = _folds("k3", n)
    kw = dict(nlambda=5, tol=1e-9, maxit=2000, standardize=True)
    r = _oracle_300()
    if no_coop:
        monkeypatch.setenv("OEM_NO_COOP", "1")
    f = oem_amd.xval_oem(x, y, foldid=fid, penalty="lasso", intercept=True, **kw)
    _end_to_end(f, r, 1, False)
    newx = sp.csr_matrix(xd[:50])
    pred = oem_amd.predict_xval(f, newx)
    b = oem_amd.predict_xval(f, type="coefficients")
    assert pred.shape[0] == 50 and np.allclose(np.ravel(pred), b[0] + xd[:50] @ np.ravel(b[1:]), rtol=1e-12, atol=1e-12)


@functools.lru_cache(maxsize=None)
def _oracle_300():
    _, xd, y = _design(20000, 300, 0.01, 5, False)
    fid, _ = _folds("k3", 20000)
    return _oracle(np.asfortranarray(xd), np.array(y), fid, ["lasso"], intercept=True, lambda_min_ratio=1e-4, nlambda=5, tol=1e-9, maxit=2000,
                   standardize=True)


def test_sparse_call_equals_the_dense_call_and_repeats_bit_for_bit(api):
    import oem_amd
    x, xd, y = _design(24577, 41, 0.015, 1, False)
    fid, _ = _folds("k5", 24577)
    kw = dict(foldid=fid, penalty=["lasso"], nlambda=21, tol=1e-9, maxit=5000)
    fs = oem_amd.xval_oem(x, y, **kw)
    again = oem_amd.xval_oem(x.tocsr(), y, **kw)                 # any scipy.sparse form
    fd = oem_amd.xval_oem(np.asfortranarray(xd), np.array(y), **kw)
    for key in ("beta", "cvm", "cvsd"):
        assert fs[key][0].tobytes() == again[key][0].tobytes(), key
    assert np.allclose(fs["cvm"][0], fd["cvm"][0], rtol=1e-9) and np.allclose(fs["cvsd"][0], fd["cvsd"][0], rtol=1e-8)
    assert np.abs(fs["beta"][0] - fd["beta"][0]).max() < 1e-8 * max(1.0, np.abs(fd["beta"][0]).max())
    t = api.xval_sparse_timings()
    assert set(t) == {"upload", "fold_order", "fold_moments", "compressed_rows", "fits", "cv_error"} and all(v >= 0 for v in t.values())
