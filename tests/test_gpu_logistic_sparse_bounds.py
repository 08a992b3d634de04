"""oemgpu_fit_logistic_sparse on the MI355X against the CPU restatement (tests/logistic_sparse_restatement.py) at the limits of its
plan and of the compressed-column Gram it shares with the Gaussian sparse fit (sparse.hip): the 160 KiB LDS limit of csc_gram_kernel
(p = 6140 / 6141) under both instantiations, p = LOGIT_P_LIMIT on the forced tile route (lsp_rows_kernel above 64 KiB of LDS), an empty
trailing chunk range, a structured edge matrix ON the compressed-column route (odd p, empty first / last column, a column that fills
whole chunks, a chunk with nothing in it, entries at rows 8191 / 8192 / n - 1, a last chunk of one row), tiles with a one-row tail,
the smallest n, q > 1024 under every operator kind on this data path, and saturated rows on both routes.

Each hand-placed case first asks oemgpu_selftest_logistic_sparse_plan (live CU count, the switches of the call) and
oemgpu_selftest_csc_plan whether its shape lands where it is named for, then compares beta / lambda / niter / loss / d with the
restatement (_compare of test_gpu_logistic_sparse) and the library's step counts with the restatement's, fits a second time and asks
for the same bits, and asserts ON THE REFERENCE that at least 0.95 of the coefficients that can be non-zero are non-zero at the last
lambda: a Gram entry X'WX[a][b] whose two coefficients stay zero reaches the result only through d, so a Gram test has to end with
(almost) everything alive.  "Can be non-zero": a column without a single non-zero value has X'r = 0 and a zero Gram row, so its
coefficient stays 0 under every lambda; such columns (the edge matrix has two on purpose) are left out of the share.
test_random_logistic_sparse is a seeded sweep over the same limits; it scales with OEM_FUZZ_SCALE like test_gpu_fuzz."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests import logistic_restatement as R
from tests import logistic_sparse_restatement as RS
from tests.test_gpu_fuzz import _check
from tests.test_gpu_logistic_sparse import _compare, _sparse

pytestmark = pytest.mark.gpu

SCALE = int(os.environ.get("OEM_FUZZ_SCALE", "1"))
SRC = 8192                     # rows per chunk of the compressed-column kernels (sparse.hip)
LDS_BYTES = 160 << 10          # LDS of a gfx950 CU
EDGE_MIN_P = 9                 # the edge matrix gives five columns a structure of their own


@pytest.fixture(scope="module")
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _edge_matrix(n, p, seed, k=5, intercept=0.0, scale=1.0):
    """A compressed-column matrix with the structures the layouts can trip over, and y drawn as _sparse draws it.  On a base of
    density 0.005, in this order (a later step wins where two meet):
      column 1 stores every row (whole chunks: eight trips of the 1024-thread scatter); column 2 holds one entry, row n - 1; column 3
      lives only in the last chunk (from its first row on); rows 0-99 are empty, and with three chunks or more so is the whole chunk
      before the last; column 4 then gets entries at rows 0, 8191, 8192 and n - 1 (those that exist and lie outside the emptied chunk),
      so row 0 holds that entry alone and rows 1-99 nothing; columns 0 and p - 1 are empty; every 17th stored value is an explicit 0.0."""
    assert p >= EDGE_MIN_P and n > 200
    rng = np.random.default_rng(seed)
    xd = sp.random(n, p, density=0.005, random_state=rng, data_rvs=lambda m: rng.normal(size=m)).toarray()
    nchunk = (n + SRC - 1) // SRC
    last = (nchunk - 1) * SRC
    xd[:, 1] = rng.normal(size=n)
    xd[:, 2] = 0.0
    xd[n - 1, 2] = 1.5
    xd[:, 3] = 0.0
    xd[last:, 3] = np.where(rng.random(n - last) < 0.3, rng.normal(size=n - last), 0.0)
    xd[last, 3] = -0.75
    xd[:100, :] = 0.0
    gone = range(0)
    if nchunk >= 3:
        gone = range((nchunk - 2) * SRC, (nchunk - 1) * SRC)
        xd[gone.start:gone.stop, :] = 0.0
    for r in (0, SRC - 1, SRC, n - 1):
        if r < n and r not in gone:
            xd[r, 4] = 2.0 + 0.25 * (r % 3)
    xd[:, 0] = 0.0
    xd[:, p - 1] = 0.0
    x = sp.csc_matrix(xd * scale)
    x.data[::17] = 0.0
    assert x.has_sorted_indices and x.nnz > np.count_nonzero(x.toarray())
    b = np.zeros(p)
    b[:k] = rng.uniform(-1.5, 1.5, k)
    prob = 1.0 / (1.0 + np.exp(-((x @ b) / scale + intercept)))
    y = (rng.uniform(size=n) < prob).astype(np.float64)
    return x, y


def _lsp_plan(n, p, nnz, intercept, num_cu):
    import oem_amd
    out = (C.c_int64 * 8)()
    assert oem_amd.lib().oemgpu_selftest_logistic_sparse_plan(n, p, nnz, int(intercept), num_cu, out) == 0
    csc, inner_wg, _, _, rows, nch, ch, chunks = list(out)
    return dict(csc=csc, inner_wg=inner_wg, tile_rows=rows, tiles=(n + rows - 1) // rows if rows else 0,
                tile_tail=n - (n - 1) // rows * rows if rows else 0, row_wgs=nch, row_ch=ch, chunks=chunks)


def _csc_plan(n, p):
    import oem_amd
    out = (C.c_int64 * 4)()
    assert oem_amd.lib().oemgpu_selftest_csc_plan(n, p, out) == 0
    return dict(zip(("chunks", "ranges", "cper", "lds"), list(out)))


def _groups(pens, groups, p, intercept):
    """what the C entry receives (api._group_setup), for the restatement"""
    from oem_amd import api
    g, ug, _ = api._group_setup(pens, groups, None, p, intercept)
    return dict(groups=g, unique_groups=ug) if g.size else dict()


def _alive_share(x, ref):
    """the least share, over the penalties, of non-zero coefficients at the last lambda among the columns that hold a non-zero value"""
    can = np.asarray(abs(x).sum(axis=0)).ravel() > 0
    return min(float(np.mean(np.asarray(b)[1:, -1][can] != 0.0)) for b in ref["beta"])


@pytest.fixture
def run(monkeypatch, num_cu):
    def _run(x, y, pens, route=None, tile_rows=None, exact_niter=True, want=None, beta_rel=False, alive=0.95, groups=(), intercept=True,
             **kw):
        """Sets the switches, asserts the plan (`want`: keys of _lsp_plan and _csc_plan with the value each must have), fits on the GPU
        (twice: the same bits) and with the restatement, compares results and step counts.  Returns (fit, ref, restatement stats)."""
        import oem_amd
        pens = list(pens)
        n, p = x.shape
        for name, val in (("OEM_SPARSE_GRAM", route), ("OEM_SPARSE_TILE_ROWS", tile_rows)):
            if val is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(val))
        plan = dict(_csc_plan(n, p), **_lsp_plan(n, p, x.nnz, intercept, num_cu))
        if route is not None:
            assert plan["csc"] == int(route == "csc"), plan
        for key, val in (want or {}).items():
            assert plan[key] == val, (key, val, plan)
        gkw = dict(penalty=pens, groups=groups, intercept=intercept, **kw)
        fit = oem_amd.oem_fit_logistic_sparse(x, y, **gkw)
        gst = oem_amd.logistic_stats()
        again = oem_amd.oem_fit_logistic_sparse(x, y, **gkw)
        for k in range(len(pens)):                                     # no float atomics, no race for a row's cursor: the same bits
            assert np.array_equal(fit["beta"][k], again["beta"][k]), pens[k]
            assert np.array_equal(fit["loss"][k], again["loss"][k]), pens[k]
        assert fit["d"] == again["d"]
        rkw = dict(kw)
        if "lambda_" in rkw:
            rkw["lambda_"] = [np.asarray(v, dtype=np.float64) for v in rkw["lambda_"]]
        st = {}
        ref = RS.fit(x, y, penalty=pens, intercept=intercept, stats=st, **_groups(pens, groups, p, intercept), **rkw)
        if alive is not None:
            share = _alive_share(x, ref)
            assert share >= alive, share
        if exact_niter:
            tol = 1e-8 * max(1.0, max(float(np.abs(b).max()) for b in ref["beta"])) if beta_rel else 1e-8
            _compare(fit, ref, pens, beta_tol=tol)
            assert gst["irls_steps"] == st["irls"], (gst, st)
            assert gst["row_passes"] == st["rows"], (gst, st)
            assert gst["grams"] == st["grams"] == st["rows"], (gst, st)
            assert abs(gst["inner_iters"] - st["inner"]) <= 0.005 * st["inner"], (gst, st)
        else:
            _check(fit, ref, pens)
        return fit, ref, st
    return _run


# ------------------------------------------------------------------------------------------------- the compressed-column kernel
# seeds: those at which the restatement ends with >= 0.95 of the coefficients alive at lambda_min_ratio = 1e-3 (at p = 33 that allows one
# dead coefficient among the 31 columns that hold a value)
@pytest.mark.parametrize("n,p,chunks,seed", [(8192, 33, 1, 63), (8193, 33, 2, 63), (16384, 101, 2, 143), (24577, 101, 4, 145)])
@pytest.mark.parametrize("intercept", [True, False])
def test_csc_edge_matrix(run, n, p, chunks, seed, intercept):
    """chunk edges (rows 8191 / 8192 / n - 1, a last chunk of one row at 8193 and 24577), the middle column of an odd p, an empty first
    and last column (ka0 == ka1 in every chunk), a column that fills whole chunks, an empty chunk (24577)"""
    x, y = _edge_matrix(n, p, seed, intercept=0.3 if intercept else 0.0)
    assert p % 2 == 1
    run(x, y, ["lasso", "grp.lasso"], route="csc", want=dict(chunks=chunks, tiles=0), groups=np.arange(p) // 3 + 1, intercept=intercept,
        nlambda=4, lambda_min_ratio=1e-3, compute_loss=True, tol=1e-9)


def test_csc_edge_matrix_both_routes(run):
    n, p = 24577, 101
    x, y = _edge_matrix(n, p, 46, intercept=0.3)
    kw = dict(nlambda=4, lambda_min_ratio=1e-3, compute_loss=True, tol=1e-9)
    a, _, _ = run(x, y, ["lasso", "mcp"], route="csc", want=dict(chunks=4, ranges=4, cper=1), **kw)
    d, _, _ = run(x, y, ["lasso", "mcp"], route="dense", tile_rows=8192, want=dict(tile_rows=8192, tiles=4, tile_tail=1), **kw)
    for k in range(2):
        assert np.abs(np.asarray(a["beta"][k]) - np.asarray(d["beta"][k])).max() < 1e-10
        assert np.array_equal(a["niter"][k], d["niter"][k])


def test_csc_empty_trailing_range(run):
    """five chunks in four ranges of two: [0, 2) [2, 4) [4, 5) and a fourth that holds none (its range sums must still be zeros)"""
    x, y = _sparse(32769, 411, 0.004, 47, k=8, intercept=0.2)
    run(x, y, ["lasso"], want=dict(csc=1, chunks=5, ranges=4, cper=2), nlambda=3, lambda_min_ratio=1e-3, compute_loss=True, tol=1e-9)


@pytest.fixture(scope="module")
def lds_limit_x():
    """(8193, 6140) at density 0.002: the last p csc_gram_kernel takes, 163840 bytes of LDS, the whole of a CU's"""
    rng = np.random.default_rng(48)
    x = sp.random(8193, 6140, density=0.002, format="csc", random_state=rng, data_rvs=lambda m: rng.normal(size=m))
    x.sort_indices()
    return x


LIMIT_KW = dict(lambda_=[[1e-4]], irls_maxit=1, maxit=30, compute_loss=True)     # one Gram build; every coefficient alive


@pytest.mark.parametrize("p", [6140, 6141])
def test_csc_lds_limit(run, lds_limit_x, p):
    if p == 6140:
        x = lds_limit_x
        want = dict(csc=1, lds=LDS_BYTES, chunks=2, inner_wg=0)
    else:
        x = _sparse(8193, p, 0.002, 49)[0]
        want = dict(csc=0, chunks=2, inner_wg=0, tiles=1, tile_rows=8193)
        assert _csc_plan(8193, p)["lds"] > LDS_BYTES
    rng = np.random.default_rng(50)
    b = np.zeros(p)
    b[:8] = rng.uniform(-1.5, 1.5, 8)
    y = (rng.uniform(size=8193) < 1.0 / (1.0 + np.exp(-(x @ b)))).astype(np.float64)
    run(x, y, ["lasso"], want=want, intercept=False, **LIMIT_KW)


def test_p_limit(run):
    """p = LOGIT_P_LIMIT: beta o s takes 65528 bytes of dynamic LDS in lsp_rows_kernel on top of its 6 KiB static; the tile route
    whatever the density; the launch-form inner solve; one tile with ld == n.
    Measured on an MI355X: 9.2-9.5 s, nearly all of it the restatement's eigenvalue problem at q = 8192, against 6.5-7.4 s of
    test_singleton_groups_beyond_lds, the time this file's cases were meant to stay under: over it by 2 to 3 s."""
    n, p = 8300, 8191
    assert 8 * p + 6144 > 64 << 10
    x, y = _sparse(n, p, 0.004, 51, k=8, intercept=0.2)
    run(x, y, ["lasso"], want=dict(csc=0, inner_wg=0, tiles=1, tile_rows=n), **LIMIT_KW)


# ------------------------------------------------------------------------------------------------- the tile route
@pytest.mark.parametrize("n,p,tile_rows,tiles,seed", [(641, 33, 64, 11, 62), (8193, 9, 2048, 5, 61)])
def test_tiles_one_row_tail(run, n, p, tile_rows, tiles, seed):
    x, y = _edge_matrix(n, p, seed, k=3, intercept=0.3)
    for intercept in (True, False):
        run(x, y, ["lasso", "grp.lasso"], route="dense", tile_rows=tile_rows, want=dict(tile_rows=tile_rows, tiles=tiles, tile_tail=1),
            groups=np.arange(p) // 3 + 1, intercept=intercept, nlambda=4, lambda_min_ratio=1e-3, compute_loss=True, tol=1e-9)


@pytest.mark.parametrize("n,p,intercept", [(4, 2, True), (3, 2, False), (65, 10, True)])
def test_tiny_n(run, n, p, intercept):
    """n < 64 (one row-pass workgroup of 64 rows, one tile of n rows), p + intercept = n - 1"""
    rng = np.random.default_rng(63 + n)                                        # (a seed at which the restatement keeps every coefficient alive)
    xd = np.where(rng.random((n, p)) < 0.6, rng.normal(size=(n, p)), 0.0)
    xd[:2, :] = rng.normal(size=(2, p))                                       # no empty column, and X'y != 0 (y is 0, 1, 0, 1, ...)
    x = sp.csc_matrix(xd)
    y = (np.arange(n) % 2).astype(np.float64)
    if n < 64:
        assert p + intercept == n - 1
    for route in ("csc", "dense"):
        want = dict(chunks=1, ranges=1, row_ch=64, row_wgs=(n + 63) // 64)
        if route == "dense":
            want.update(tiles=1, tile_rows=n)
        run(x, y, ["lasso", "grp.lasso"], route=route, want=want, groups=np.arange(p) // 2 + 1, intercept=intercept, nlambda=4,
            lambda_min_ratio=1e-3, compute_loss=True, irls_maxit=8, beta_rel=True)


# ------------------------------------------------------------------------------------------------- operators, saturation
def test_all_operators_on_csc_launch_form(run):
    """q > 1024 (the launch form of the inner solve) under every operator kind, X'WX from the compressed columns"""
    n, p = 2600, 1100
    x, y = _sparse(n, p, 0.004, 54, k=8)
    pens = [pn for pn in R.PENALTIES if pn != "ols"]
    run(x, y, pens, route="csc", want=dict(inner_wg=0, chunks=1), groups=np.arange(p) // 4 + 1, nlambda=2, lambda_min_ratio=1e-3,
        alpha=0.7, gamma=3.5, tau=0.3, irls_maxit=2, maxit=30, compute_loss=True)


@pytest.mark.parametrize("route", ["csc", "dense"])
def test_saturated_rows(run, route):
    """rows with W = 0 to the last bit, the W floor and both loss clamps, on both routes"""
    xd, y = R.near_separable(6000, 20, 55)
    xd[np.abs(xd) < 0.7] = 0.0                                                # sparse, the far rows keep their weight
    x = sp.csc_matrix(xd * 30.0)
    _, _, st = run(x, y, ["lasso", "grp.lasso"], route=route, groups=np.arange(20) // 4 + 1, nlambda=8, lambda_min_ratio=1e-3,
                   compute_loss=True, irls_maxit=30, beta_rel=True)
    assert st["floored"] > 0 and st["clamped"] > 0, st


# ------------------------------------------------------------------------------------------------- the Gaussian instantiation
GAUSS_MAXIT = 100              # both sides stop at the cap alike; it keeps the oracle's q^2 products to seconds
P_ORACLE = 2048                # the oracle's one-thread Householder reduction for d grows as p^3: seconds here, minutes at 6140


def test_gaussian_csc_lds_limit(lds_limit_x, monkeypatch):
    """csc_gram_kernel<false> at the same 163840 bytes: oem() on the p = 6140 matrix, with the assertions of
    test_sparse_x_compressed_column_gram (test_gpu_parity).  At p = 6140 the two routes are held to each other and the compressed
    columns to their own bits; the oracle, which would take minutes there, is the yardstick on the first P_ORACLE columns."""
    import oem_amd as oa
    from oracle import oracle as orc
    x = lds_limit_x
    n, p = x.shape
    assert _csc_plan(n, p)["lds"] == LDS_BYTES and _csc_plan(n, p + 1)["lds"] > LDS_BYTES
    rng = np.random.default_rng(56)
    b = np.zeros(p)
    b[:5] = [1.0, -1.0, 0.5, 2.0, -0.7]
    y = x @ b + rng.normal(size=n) * 0.5 + 0.8
    kw = dict(penalty=["lasso", "mcp"], nlambda=2, tol=1e-9, maxit=GAUSS_MAXIT)
    monkeypatch.setenv("OEM_SPARSE_GRAM", "csc")
    a = oa.oem(x, y, **kw)
    a2 = oa.oem(x, y, **kw)
    assert np.array_equal(a["beta"][0], a2["beta"][0])                            # fixed summation order: bitwise reproducible
    xs = sp.csc_matrix(x[:, :P_ORACLE])
    s = oa.oem(xs, y, **kw)
    monkeypatch.setenv("OEM_SPARSE_GRAM", "dense")
    d = oa.oem(x, y, **kw)
    assert abs(a["d"] - d["d"]) < 1e-10 * d["d"]
    for k in range(2):
        assert np.abs(a["beta"][k] - d["beta"][k]).max() < 1e-9
        assert np.any(a["beta"][k][1:, -1] != 0.0)
    r = orc.fit_sparse(xs, y, lambda_min_ratio=1e-4, **kw)
    assert abs(s["d"] - r["d"]) < 1e-10 * r["d"]
    for k in range(2):
        assert np.abs(s["beta"][k] - r["beta"][k]).max() < 1e-8 * max(1.0, float(np.abs(r["beta"][k]).max()))


# ------------------------------------------------------------------------------------------------- seeded sweep
P_CHOICES = [2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1024, 1025]
NNZ_CAP = 2_000_000            # keeps the restatement's sparse X'WX product to a fraction of a second; both routes stay reachable


@pytest.mark.parametrize("seed", list(range(24)) + list(range(1000, 1000 + 24 * (SCALE - 1))))
def test_random_logistic_sparse(run, seed):
    rng = np.random.default_rng(7000 + seed)
    p = int(rng.choice(P_CHOICES))
    intercept = bool(rng.random() < 0.6)
    standardize = True if intercept else bool(rng.random() < 0.5)
    q = p + intercept
    n = q + 1 + int(rng.integers(0, 3 * q + 400))
    u = rng.random()
    if p <= 257 and u < 0.1:
        n = 32769 + int(rng.integers(0, 8000))                                # five chunks; ranges < chunks for p >= 409 only
    elif u < 0.35:
        special = [v for v in (8191, 8192, 8193, 16385) if v > q + 1]
        if special:
            n = int(rng.choice(special))
    dens = float(np.exp(rng.uniform(np.log(0.002), np.log(min(0.3, max(0.03, NNZ_CAP / (n * p)))))))
    dens = max(dens, min(0.3, 20.0 / n))                                      # ~20 entries a column at least: X'y = 0 has no lambda grid
    route = str(rng.choice(["csc", "dense"])) if rng.random() < 0.3 else None
    tile_rows = int(rng.choice([64, 128, 2048])) if rng.random() < 0.3 else None
    scale = float(rng.choice([1e-3, 1.0, 30.0]))
    k, shift = int(rng.integers(1, 6)), float(rng.uniform(-1, 1))
    if rng.random() < 0.5 and p >= EDGE_MIN_P and n > 200:
        x, y = _edge_matrix(n, p, 8000 + seed, k=min(k, p), intercept=shift, scale=scale)
    else:
        rs = np.random.default_rng(8000 + seed)
        x = sp.random(n, p, density=dens, format="csc", random_state=rs, data_rvs=lambda m: rs.normal(size=m) * scale)
        b = np.zeros(p)
        b[:min(k, p)] = rs.uniform(-1.5, 1.5, min(k, p))
        y = (rs.uniform(size=n) < 1.0 / (1.0 + np.exp(-((x @ b) / scale + shift)))).astype(np.float64)
    pool = [pn for pn in R.PENALTIES if pn != "ols" or n > 5 * q]
    pens = list(rng.choice(pool, int(rng.integers(1, 4)), replace=False))
    gsz = int(rng.integers(1, 7))
    groups = np.arange(p) // gsz + (0 if rng.random() < 0.25 else 1)
    pf = np.where(rng.random(p) < 0.1, 0.0, rng.uniform(0.5, 2.0, p))
    kw = dict(nlambda=int(rng.integers(1, 6 if p <= 512 else 4)),
              lambda_min_ratio=float(rng.uniform(0.02, 0.3) if n < 4 * q else rng.uniform(1e-3, 0.1)),
              alpha=float(rng.uniform(0.3, 1.0)), gamma=float(rng.uniform(2.5, 5.0)), tau=float(rng.uniform(0.1, 0.9)),
              tol=float(10.0 ** rng.uniform(-9, -6)), penalty_factor=pf, compute_loss=True)
    # a few stored values a column are often separable: such fits run to the default caps (100 IRLS steps of 500 iterations, each step
    # an eigenvalue problem in the restatement), so the sweep draws the caps; both sides stop at them alike
    kw.update(irls_maxit=int(rng.choice([4, 12] if p <= 512 else [2, 4])), maxit=int(rng.choice([100, 500] if p <= 512 else [30, 100])))
    print(f"seed {seed}: n {n} p {p} nnz {x.nnz} route {route} tile_rows {tile_rows} scale {scale} intercept {intercept} "
          f"standardize {standardize} {pens} nlambda {kw['nlambda']}")
    run(x, y, pens, route=route, tile_rows=tile_rows, exact_niter=False, alive=None,
        groups=groups if any("grp" in pn for pn in pens) else (), intercept=intercept, standardize=standardize, **kw)
