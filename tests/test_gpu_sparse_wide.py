"""oem() on a sparse x with p >= n from its non-zeros (oem_amd/csrc/sparse_wide.hip) on the GPU: parity with the oracle on the route
the library chooses, the structures a compressed matrix can have with the route forced, the dense-copy route it replaces, bit
identity, a shape past the dense wide engine's row limit, and a seeded sweep (OEM_FUZZ_SCALE scales it, as in test_gpu_fuzz).
tests/test_sparse_wide_cpu.py shows on the CPU that the parity inputs stay inside the agreement rule on the reference side alone.
The lanes per row and per column of these fits follow the shape and the device's CU count (on 256 CUs: rows at 64 or 4 lanes, columns
at 4 .. 64; DESIGN.md section 3.6a has the table); tests/test_gpu_sparse_wide_pass.py holds the single passes at all seven lane counts
to exact sums."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as orc
from tests import sparse_wide_restatement as R

pytestmark = pytest.mark.gpu

DTOL = 1e-10            # tests/test_gpu_parity.py: d against an exact eigenvalue
SCALE = int(os.environ.get("OEM_FUZZ_SCALE", "1"))
PENS = ["lasso", "mcp", "scad", "elastic.net", "grp.lasso", "sparse.grp.lasso"]


@pytest.fixture(scope="module")
def oa():
    import torch
    assert torch.cuda.is_available()
    import oem_amd
    oem_amd.lib()
    return oem_amd


def _agree(f, r, k, tol, label):
    """_agree_with_oracle of tests/test_gpu_parity.py: niter within one, at least 75 % of the lambdas with equal counts, coefficients
    to 1e-9 of their scale where the counts are equal and to max(1e-9, 4 tol) where one side took one iteration more"""
    fb, rb = np.asarray(f["beta"][k]), np.asarray(r["beta"][k])
    fn, rn = np.ravel(f["niter"][k]).astype(int), np.ravel(r["niter"][k]).astype(int)
    dn = np.abs(fn - rn)
    assert dn.max() <= 1, (label, dn)
    scale = max(1.0, float(np.abs(rb).max()))
    colerr = np.abs(fb - rb).reshape(fb.shape[0], -1).max(axis=0) / scale
    same = dn == 0
    assert same.mean() >= 0.75, (label, dn)
    assert colerr[same].max() <= 1e-9, (label, colerr.max())
    if (~same).any():
        assert colerr[~same].max() <= max(1e-9, 4.0 * tol), (label, colerr[~same].max())


def _oem(oa, x, y, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                             # ("oem() is optimized for n >> p")
        return oa.oem(x, y, intercept=False, **kw)


def _groups(p):
    return np.arange(p) // 4 + 1


_cache = {}


def _parity_case(n, p, dens, standardize):
    """the inputs, the options and the oracle's two fits of a parity case, computed once and left unchanged"""
    key = (n, p, standardize)
    if key not in _cache:
        x, y = R.parity_data(n, p, dens)
        g = _groups(p)
        kw = dict(R.PARITY_KW, penalty=PENS, groups=g, alpha=0.7, standardize=standardize)
        lkw = dict(R.PARITY_KW, penalty=["lasso", "scad"], standardize=standardize, compute_loss=True)
        r = orc.fit_sparse(x, y, native=True, intercept=False, unique_groups=np.unique(g), **kw)
        rl = orc.fit_sparse(x, y, native=True, intercept=False, **lkw)
        _cache[key] = (x, y, kw, lkw, r, rl)
    return _cache[key]


@pytest.mark.parametrize("n,p,dens", R.PARITY_SHAPES)
@pytest.mark.parametrize("standardize", [False, True])
def test_parity_with_the_oracle_on_the_chosen_route(oa, n, p, dens, standardize, monkeypatch):
    monkeypatch.delenv("OEM_SPARSE_GRAM", raising=False)
    x, y, kw, lkw, r, rl = _parity_case(n, p, dens, standardize)
    f = _oem(oa, x, y, **kw)
    assert oa.last_host_path_engine() == "sparse-wide"              # OEMGPU_ENGINE_SPARSE_WIDE = 10, without the switch
    assert abs(f["d"] - r["d"]) <= DTOL * r["d"]
    for k, pen in enumerate(PENS):
        assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-12, atol=0), pen
        _agree(f, r, k, kw["tol"], pen)
        assert np.all(np.asarray(f["beta"][k])[0] == 0.0)
        assert np.all(np.ravel(f["loss"][k]) == 1e99)
    g = _oem(oa, x, y, **lkw)
    assert oa.last_host_path_engine() == "sparse-wide"
    assert abs(g["d"] - rl["d"]) <= DTOL * rl["d"]
    for k, pen in enumerate(lkw["penalty"]):
        _agree(g, rl, k, lkw["tol"], pen)
        assert np.allclose(np.ravel(g["loss"][k]), np.ravel(rl["loss"][k]), rtol=1e-7, atol=0), (pen, g["loss"][k], rl["loss"][k])


def _base(n, p, dens, seed):
    rng = np.random.default_rng(seed)
    x = sp.random(n, p, density=dens, format="lil", random_state=rng, data_rvs=lambda k: rng.normal(size=k) * 1.5)
    return x, rng


def _structure(name):
    """(x as handed to oem, its canonical form for the oracle, y)"""
    if name == "long row and column":
        n, p = 200, 20000                                           # tests/test_sparse_wide_cpu.py: both long forms at this shape
        x, rng = _base(n, p, 0.01, 11)
        x[7, :] = 0.1 * rng.normal(size=p)                          # one row stores all p entries
        x[:, 123] = 1.0                                             # one column stores all n: all ones
    else:
        n = {"n=63": 63, "n=64": 64, "n=65": 65, "p=n": 80}.get(name, 50)
        p = 80 if name == "p=n" else 300
        x, rng = _base(n, p, 0.06, len(name) + n)
        if name == "empty column":
            x[:, 17] = 0.0; x[:, 0] = 0.0; x[:, p - 1] = 0.0
        if name == "empty row":
            x[0, :] = 0.0; x[31, :] = 0.0; x[n - 1, :] = 0.0
    x = sp.csc_matrix(x)
    x.sum_duplicates(); x.sort_indices()
    canon = x.copy()
    b = np.zeros(p); b[np.argsort(-np.diff(x.indptr), kind="stable")[:5]] = rng.uniform(1, 2, 5)
    y = canon @ b + 0.3 * rng.normal(size=n)
    if name == "stored zeros":
        x.data[::7] = 0.0                                           # explicit zeros stay stored
        canon = x.copy()
        assert canon.nnz == x.nnz and np.count_nonzero(x.data) < x.nnz
    if name == "duplicates unsorted":
        coo = x.tocoo()
        half = coo.data * 0.5
        perm = rng.permutation(2 * coo.nnz)
        x = sp.coo_matrix((np.concatenate([half, half])[perm], (np.concatenate([coo.row, coo.row])[perm], np.concatenate([coo.col, coo.col])[perm])),
                          shape=coo.shape)                          # every entry twice, in no order: oem() sums and sorts (R's dgCMatrix)
    return x, canon, y


@pytest.mark.parametrize("name", ["empty column", "empty row", "long row and column", "n=63", "n=64", "n=65", "stored zeros",
                                  "duplicates unsorted", "p=n"])
def test_structures_with_the_route_forced(oa, name, monkeypatch):
    monkeypatch.setenv("OEM_SPARSE_GRAM", "wide")
    x, canon, y = _structure(name)
    n, p = canon.shape
    g = _groups(p)
    big = name == "long row and column"
    kw = dict(penalty=["lasso", "grp.lasso"] if big else ["lasso", "mcp", "grp.lasso"], groups=g, standardize=True, nlambda=3 if big else 5,
              lambda_min_ratio=0.05, tol=1e-9, maxit=400)
    if big:
        assert np.diff(canon.indptr).max() == n and np.diff(sp.csr_matrix(canon).indptr).max() == p
    f = _oem(oa, x, y, **kw)
    assert oa.last_host_path_engine() == "sparse-wide"
    r = orc.fit_sparse(canon, y, native=True, intercept=False, unique_groups=np.unique(g), **kw)
    assert abs(f["d"] - r["d"]) <= DTOL * r["d"]
    for k, pen in enumerate(kw["penalty"]):
        assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-12, atol=0), pen
        _agree(f, r, k, kw["tol"], pen)


@pytest.mark.parametrize("n,p,dens", R.PARITY_SHAPES[1:3])
def test_against_the_dense_copy_route(oa, n, p, dens, monkeypatch):
    """the same call with OEM_SPARSE_GRAM=nowide runs as before this engine: the dense n x p copy through the dense p >= n engines"""
    x, y, kw, lkw, r, rl = _parity_case(n, p, dens, True)
    monkeypatch.delenv("OEM_SPARSE_GRAM", raising=False)
    f = _oem(oa, x, y, **kw)
    assert oa.last_host_path_engine() == "sparse-wide"
    monkeypatch.setenv("OEM_SPARSE_GRAM", "nowide")
    g = _oem(oa, x, y, **kw)
    assert oa.last_host_path_engine() != "sparse-wide"
    assert abs(f["d"] - g["d"]) <= 1e-12 * abs(g["d"]), (f["d"], g["d"])
    for k, pen in enumerate(PENS):
        assert np.allclose(f["lambda"][k], g["lambda"][k], rtol=1e-12, atol=0), pen
        _agree(f, g, k, kw["tol"], pen)


def _same_bits(f, g):
    assert f["d"] == g["d"]
    for k in range(len(f["beta"])):
        for key in ("beta", "lambda", "niter", "loss"):
            assert np.array_equal(np.asarray(f[key][k]), np.asarray(g[key][k])), (key, k)


def test_two_calls_and_the_resident_entry_give_the_same_bits(oa, monkeypatch):
    import torch
    from oem_amd import api, _lib as L
    monkeypatch.delenv("OEM_SPARSE_GRAM", raising=False)
    n, p, dens = R.PARITY_SHAPES[2]
    x, y, kw, lkw, r, rl = _parity_case(n, p, dens, True)
    kw = dict(kw, compute_loss=True)
    f = _oem(oa, x, y, **kw)
    g = _oem(oa, x, y, **kw)
    _same_bits(f, g)
    # oemgpu_fit_sparse_wide_res on an open SparseX: the option block of the same oem() call, y on the device
    with oa.SparseX(x) as sx:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            a, varnames, std, icpt = api.oem(sx, y, intercept=False, _args_only=True, **kw)
        assert std and not icpt
        yd = torch.as_tensor(np.asarray(y, dtype=np.float64), device=sx.device)
        ctx = oa.context(sx.device.index)
        torch.cuda.current_stream(sx.device).synchronize()
        L.check(L.lib().oemgpu_fit_sparse_wide_res(ctx, sx.handle, yd.data_ptr(), 1, C.byref(a.c), *a.outputs(p + 1)))
        assert oa.last_path_engine(ctx)[0] == "sparse-wide"
        h = api._decorate(a, kw["penalty"], varnames, True, n, p)
    _same_bits(f, h)


def test_past_the_dense_wide_engines_row_limit(oa, monkeypatch):
    """n = 33,000 > WIDE_MAX_N = 32,768: the dense wide engine ends there and the oracle's dense n x n eigen-solve cannot run; the fit is
    held to the CPU restatement (d handed over), d to ARPACK on the X X'/n operator"""
    monkeypatch.delenv("OEM_SPARSE_GRAM", raising=False)
    n, p = 33000, 34000
    rng = np.random.default_rng(5)
    x = sp.random(n, p, density=3e-4, format="csc", random_state=rng, data_rvs=lambda k: rng.normal(size=k) * 1.5)
    x.sort_indices()
    b = np.zeros(p); b[np.argsort(-np.diff(x.indptr), kind="stable")[:6]] = rng.uniform(1, 2, 6)
    y = x @ b + 0.3 * rng.normal(size=n)
    kw = dict(penalty=["lasso", "mcp"], standardize=True, nlambda=3, lambda_min_ratio=0.2, tol=1e-9, maxit=400)
    f = _oem(oa, x, y, **kw)
    assert oa.last_host_path_engine() == "sparse-wide"
    dref = R.d_of(x)
    assert abs(f["d"] - dref) <= DTOL * dref, (f["d"], dref)
    r = R.fit(x, y, d_override=f["d"], **kw)
    for k, pen in enumerate(kw["penalty"]):
        assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-12, atol=0), pen
        _agree(f, r, k, kw["tol"], pen)


@pytest.mark.parametrize("seed", range(12 * SCALE))
def test_seeded_sweep(oa, seed, monkeypatch):
    """small n and p around the plan's switches: 63 / 64 / 65 rows (a wave of lanes), rows on either side of 32 x 64 = 2048 stored
    entries (the switch to the long-row form AT 64 LANES PER ROW, which is what these few rows get on a device of 256 CUs; the switch
    at the other lane counts, 32 L against 32 L + 1 entries, is tests/test_gpu_sparse_wide_pass.py's), n = p, very sparse and dense-ish,
    either value of standardize"""
    monkeypatch.setenv("OEM_SPARSE_GRAM", "wide")
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.choice([2, 3, 17, 63, 64, 65, 70]))
    p = int(rng.choice([n, n + 1, 97, 256, 257, 1030, 2047, 2049, 2100]))
    p = max(p, n)
    dens = float(rng.choice([0.004, 0.02, 0.1, 0.3]))
    x = sp.random(n, p, density=dens, format="lil", random_state=rng, data_rvs=lambda k: rng.normal(size=k) * 1.5)
    if p >= 2047 and seed % 2 == 0:
        x[n // 2, :] = 0.2 * rng.normal(size=p)                     # a full row: the long-row form from 2049 columns on
    if x.nnz == 0:
        x[0, 0] = 1.5                                               # (an empty matrix has no lambda_zero: nothing to fit)
    x = sp.csc_matrix(x); x.sort_indices()
    nb = min(4, p)
    b = np.zeros(p); b[np.argsort(-np.diff(x.indptr), kind="stable")[:nb]] = rng.uniform(1, 2, nb)
    y = x @ b + 0.3 * rng.normal(size=n)
    g = _groups(p)
    pens = [PENS[i] for i in sorted(rng.choice(len(PENS), size=2, replace=False))]
    kw = dict(penalty=pens, groups=g, alpha=0.7, standardize=bool(seed % 3), nlambda=4, lambda_min_ratio=0.05, tol=1e-9, maxit=400)
    f = _oem(oa, x, y, **kw)
    assert oa.last_host_path_engine() == "sparse-wide"
    r = orc.fit_sparse(x, y, native=True, intercept=False, unique_groups=np.unique(g), **kw)
    assert abs(f["d"] - r["d"]) <= DTOL * max(r["d"], 1e-300), (f["d"], r["d"])
    for k, pen in enumerate(pens):
        assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-12, atol=0), pen
        _agree(f, r, k, kw["tol"], pen)
