"""Parity of the HIP path (through the C ABI) against the CPU oracle and the reference's doc KATs.
Tolerance contract (BASELINE.json north_star): coefficients <= 1e-7 max-abs; observed ~1e-12."""
import ctypes as C
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc

# d = 1.005 lambda_max: the reference's own Spectra tolerance is 1e-10 (ref src/oem_dense.h:494-498); the device recurrence stops
# at a 1e-12 tail estimate, so every comparison of d with the oracle's exact eigenvalue holds to 1e-10 relative (it was 1e-8: a
# regression of the eigen step by three orders of magnitude would have passed -- VERDICT r2)
DTOL = 1e-10
from tests import kat_inputs as K

TOL = 1e-7          # north_star contract
TIGHT = 1e-9        # what the implementation is expected to deliver


@pytest.fixture(scope="module")
def oa():
    import torch
    assert torch.cuda.is_available()
    import oem_amd
    oem_amd.lib()
    return oem_amd


def _printed_equal(v, expected, decimals):
    return np.all(np.abs(np.asarray(v) - np.asarray(expected)) <= 0.5 * 10.0 ** (-decimals) * (1 + 1e-9))


def _cmp(fit, ref, tol=TIGHT, rows=None):
    for k in range(len(ref["beta"])):
        a, b = np.asarray(fit["beta"][k]), np.asarray(ref["beta"][k])
        assert a.shape == b.shape
        err = np.abs(a - b).max()
        assert err <= tol, (fit["penalty"][k], err)
        assert np.allclose(fit["lambda"][k], ref["lambda"][k], rtol=1e-12, atol=0)
    assert abs(fit["d"] - ref["d"]) <= DTOL * abs(ref["d"])


def _report(tag, f, r, k, tol, maxit):
    """OEM_TEST_REPORT=file: per (test, penalty) the statistics the p >= n tolerances are set from"""
    import os
    path = os.environ.get("OEM_TEST_REPORT")
    if not path:
        return
    fb, rb = np.asarray(f["beta"][k]), np.asarray(r["beta"][k])
    fn, rn = np.ravel(f["niter"][k]).astype(int), np.ravel(r["niter"][k]).astype(int)
    scale = max(1.0, float(np.abs(rb).max()))
    colerr = np.abs(fb - rb).max(axis=0) / scale
    same = fn == rn
    capped = (rn > maxit) | (fn > maxit)
    with open(path, "a") as fh:
        fh.write(f"{tag} tol={tol:g} maxit={maxit} nlam={len(fn)} same={int(same.sum())} capped_both={int(((rn > maxit) & (fn > maxit)).sum())} capped_one={int(((rn > maxit) ^ (fn > maxit)).sum())} "
                 f"err_same={colerr[same].max() if same.any() else 0:.2e} err_diff={colerr[~same].max() if (~same).any() else 0:.2e} "
                 f"dn={list(np.abs(fn - rn)[~same])} rn_diff={list(rn[~same])} err_over_tol={(colerr[~same].max() / tol if (~same).any() else 0):.2f} capped={int(capped.sum())}\n")


def _agree_with_oracle(f, r, k, tol, label):
    """the p >= n engines against the oracle, at the resolution they deliver (these tests accepted 1e-7 and let a quarter
    of the lambdas differ by more than one iteration).  Measured over all 608 (shape, flag, penalty) cases of this file, round 4:
    the iteration counts are IDENTICAL to the oracle's at every lambda -- also where the loop runs into maxit, both sides report
    maxit + 1 -- and the coefficients agree to 3e-11 of their scale.  Asserted: niter within one (a coordinate may graze the stop
    rule), coefficients to 1e-9 where the counts are equal, and to four steps of the size the stop rule lets through where one side
    took one iteration more."""
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


def _oracle_wide(x, y, f, **kw):
    """the oracle's p >= n branch for the larger shapes of this file: its exact dense eigen-solve of the n x n matrix Xs Xs'/n is
    O(n^3) Jacobi sweeps (a minute at n = 2048, most of this file's run time).  From 600 rows on, d is held against LAPACK instead
    (2-norm of the standardised data, ref src/DataStd.h:94-267 restated in three numpy lines, 1e-10) and handed to the oracle, as
    the config-4 tests do: the comparison that remains is the path's."""
    n = x.shape[0]
    if n < 600:
        return orc.fit_dense(x, y, native=True, **kw)
    std, icpt = kw.get("standardize", True), kw.get("intercept", True)
    mu = x.mean(axis=0)
    xs = x - mu if icpt else x.copy()
    if std:
        sd = np.sqrt(((x - mu) ** 2).sum(axis=0) / n); sd[sd == 0] = 1.0
        xs = xs / sd
    dref = 1.005 * np.linalg.norm(xs, 2) ** 2 / n
    assert abs(f["d"] - dref) <= DTOL * dref, (f["d"], dref)
    return orc.fit_dense(x, y, native=True, d_override=f["d"], **kw)


def _data(n, p, seed, mean=0.0, sd=3.0, nnz=10):
    rng = np.random.default_rng(seed)
    x = np.asfortranarray(rng.normal(size=(n, p)) * sd + mean)
    b = np.concatenate([rng.uniform(-0.5, 0.5, nnz), np.zeros(p - nnz)])
    y = x @ b + rng.normal(size=n) + 0.7
    return x, y


# ------------------------------------------------------------------ reference documentation known answers
def test_kat1_loglik(oa, doc_kats):
    x, y = K.kat1()
    fit = oa.oem(x, y, penalty=["lasso", "mcp"], compute_loss=True)
    k = doc_kats["kat1"]
    assert _printed_equal(oa.logLik(fit), k["loglik_lasso"], 3)
    assert _printed_equal(oa.logLik(fit, "mcp"), k["loglik_mcp"], 3)
    ref = orc.fit_dense(x, y, penalty=["lasso", "mcp"], compute_loss=True)
    _cmp(fit, ref)
    assert fit["niter"][0][0] == 1
    fit25 = oa.oem(x, y, penalty=["lasso", "mcp"], compute_loss=True, nlambda=25)
    assert _printed_equal(oa.logLik(fit25), doc_kats["kat1b"]["loglik_lasso"], 3)
    assert _printed_equal(oa.logLik(fit25, "mcp"), doc_kats["kat1b"]["loglik_mcp"], 3)


def test_kat2_predict_mse(oa, doc_kats):
    x, y, xt, yt = K.kat2()
    fit = oa.oem(x, y, penalty=["lasso", "grp.lasso"], groups=np.repeat(np.arange(1, 11), 10), nlambda=10)
    for m, key in enumerate(["mse_lasso", "mse_grp_lasso"]):
        pred = oa.predict(fit, xt, which_model=m, type="response")
        assert _printed_equal(((yt[:, None] - pred) ** 2).mean(0), doc_kats["kat2"][key], 6), key


def test_kat3_big_vs_dense(oa, doc_kats):
    x, y = K.kat3()
    g = np.repeat(np.arange(1, 21), 5)
    big = oa.big_oem(x, y, penalty=["lasso", "grp.lasso"], groups=g)
    dense = oa.oem(x, y, penalty=["lasso", "grp.lasso"], groups=g)
    diff = np.abs(big["beta"][0] - dense["beta"][0]).max()
    assert float(f"{diff:.7g}") == doc_kats["kat3"]["max_abs_big_minus_dense_lasso"]
    ref = orc.fit_big(x, y, penalty=["lasso", "grp.lasso"], groups=np.concatenate([[0], g]), unique_groups=np.arange(0, 21))
    _cmp(big, ref)
    # row shards == one matrix (the slices of ref src/oem_big.h:319-361)
    cut = [0, 7001, 7001 + 12345, 50000]
    sh = oa.big_oem([x[cut[i]:cut[i + 1]] for i in range(3)], [y[cut[i]:cut[i + 1]] for i in range(3)],
                    penalty=["lasso", "grp.lasso"], groups=g)
    _cmp(sh, ref)


# ------------------------------------------------------------------ seeded comparisons with the oracle
@pytest.mark.parametrize("standardize,intercept", [(False, False), (True, False), (False, True), (True, True)])
def test_datastd_flags(oa, standardize, intercept):
    x, y = _data(3001, 37, 11, mean=2.0)
    pens = ["elastic.net", "lasso", "ols", "mcp", "scad", "mcp.net", "scad.net"]
    kw = dict(penalty=pens, standardize=standardize, intercept=intercept, alpha=0.6, nlambda=20, tol=1e-10)
    _cmp(oa.oem(x, y, **kw), orc.fit_dense(x, y, **kw))


def test_group_penalties(oa):
    x, y = _data(4000, 60, 5)
    groups = np.array(([0] * 4) + list(np.repeat(np.arange(1, 8), 8)))          # group 0 = unpenalised
    pens = ["grp.lasso", "grp.lasso.net", "grp.mcp", "grp.scad", "grp.mcp.net", "grp.scad.net", "sparse.grp.lasso"]
    kw = dict(penalty=pens, alpha=0.7, tau=0.4, gamma=3.5, nlambda=25, tol=1e-10)
    fit = oa.oem(x, y, groups=groups, **kw)
    ref = orc.fit_dense(x, y, groups=groups, unique_groups=np.unique(groups), **kw)
    _cmp(fit, ref)
    gw = np.linspace(0.5, 2.0, 8)
    fit = oa.oem(x, y, groups=groups, group_weights=gw, **kw)
    ref = orc.fit_dense(x, y, groups=groups, unique_groups=np.unique(groups), group_weights=gw, **kw)
    _cmp(fit, ref)


@pytest.mark.parametrize("p", [40, 96, 150, 230])
def test_mixed_group_and_elementwise_penalties(oa, p):
    """a call with group AND element-wise penalties stays in the replicated-vector kernel, whose element-wise
    operators take the sliced form (p <= 192) or the four-workgroup form"""
    x, y = _data(3 * p + 300, p, 300 + p)
    groups = np.arange(p) // 5 + 1
    pens = ["lasso", "grp.lasso", "mcp", "grp.scad", "ols"]
    kw = dict(penalty=pens, groups=groups, gamma=3.5, nlambda=9, tol=1e-9)
    fit = oa.oem(x, y, **kw)
    ref = orc.fit_dense(x, y, unique_groups=np.unique(groups), **kw)
    _cmp(fit, ref)


@pytest.mark.parametrize("p", [32, 33, 64, 65, 80, 81, 104, 105, 128, 129, 160, 161, 176, 177, 208, 209, 256, 257, 260])
def test_path_kernel_size_boundaries(oa, p):
    """both sides of every size at which another path kernel / configuration takes over"""
    x, y = _data(2 * p + 400, p, 500 + p, mean=0.4)
    kw = dict(penalty=["lasso", "scad"], nlambda=8, tol=1e-9)
    f, r = oa.oem(x, y, **kw), orc.fit_dense(x, y, **kw)
    _cmp(f, r)
    n = x.shape[0]
    _cmp(oa.oem_xtx(x.T @ x / n, x.T @ y / n, penalty=["mcp"], nlambda=6), orc.fit_xtx(x.T @ x / n, x.T @ y / n, penalty=["mcp"], nlambda=6))


def test_user_lambda_penalty_factor_accelerate_maxit(oa):
    x, y = _data(2500, 30, 9)
    pf = np.linspace(0.0, 2.0, 30)
    lam = [np.geomspace(2.0, 0.01, 15), np.geomspace(1.0, 0.02, 15)]
    kw = dict(penalty=["lasso", "scad"], penalty_factor=pf, tol=1e-9, gamma=4.0)
    _cmp(oa.oem(x, y, lambda_=lam, **kw), orc.fit_dense(x, y, lambda_=lam, **kw))
    kw = dict(penalty=["lasso", "mcp"], accelerate=True, nlambda=15, tol=1e-9)
    f, r = oa.oem(x, y, **kw), orc.fit_dense(x, y, **kw)
    _cmp(f, r)
    assert all(np.array_equal(f["niter"][k], r["niter"][k]) for k in range(2))
    kw = dict(penalty=["lasso"], maxit=3, nlambda=12, tol=1e-12)                 # quirk Q2: niter = maxit + 1
    f, r = oa.oem(x, y, **kw), orc.fit_dense(x, y, **kw)
    _cmp(f, r)
    assert f["niter"][0].max() == 4 and np.array_equal(f["niter"][0], r["niter"][0])


@pytest.mark.parametrize("p", [72, 100, 128, 150, 200])
def test_every_option_on_every_small_p_path_kernel(oa, p):
    """the options of test_datastd_flags / test_user_lambda_... again at sizes that select the other single-launch path
    kernels: row-split (64 < p <= 128), sliced with 8 waves (<= 192), four cooperating workgroups (<= 256)"""
    x, y = _data(3 * p + 500, p, 40 + p, mean=0.5)
    pens = ["elastic.net", "lasso", "ols", "mcp", "scad", "mcp.net", "scad.net"]
    for std, icpt in ((True, True), (False, False)):
        kw = dict(penalty=pens, standardize=std, intercept=icpt, alpha=0.6, nlambda=12, tol=1e-10, compute_loss=True)
        f, r = oa.oem(x, y, **kw), orc.fit_dense(x, y, **kw)
        _cmp(f, r)
        for k in range(len(pens)):
            # iteration counts: the GEMV is summed in another order than on the CPU, so a stop-rule comparison that
            # lands within an ulp of tol may resolve one iteration apart (seen on the non-convex operators)
            dn = np.abs(np.ravel(f["niter"][k]).astype(int) - np.ravel(r["niter"][k]).astype(int))   # "ols": a scalar in R
            assert dn.max() <= 1 and (dn != 0).mean() <= 0.2, (pens[k], dn)
            assert np.allclose(np.ravel(f["loss"][k]), np.ravel(r["loss"][k]), rtol=1e-9, atol=1e-9), pens[k]
    pf = np.linspace(0.0, 2.0, p)
    lam = [np.geomspace(2.0, 0.01, 9), np.geomspace(1.0, 0.02, 9)]
    kw = dict(penalty=["lasso", "scad"], penalty_factor=pf, tol=1e-9, gamma=4.0)
    _cmp(oa.oem(x, y, lambda_=lam, **kw), orc.fit_dense(x, y, lambda_=lam, **kw))
    kw = dict(penalty=["lasso", "mcp", "elastic.net"], accelerate=True, alpha=0.5, nlambda=10, tol=1e-9)
    f, r = oa.oem(x, y, **kw), orc.fit_dense(x, y, **kw)
    _cmp(f, r)
    assert all(np.array_equal(f["niter"][k], r["niter"][k]) for k in range(3))
    kw = dict(penalty=["lasso"], maxit=3, nlambda=8, tol=1e-12)                  # quirk Q2: niter = maxit + 1
    f, r = oa.oem(x, y, **kw), orc.fit_dense(x, y, **kw)
    _cmp(f, r)
    assert f["niter"][0].max() == 4 and np.array_equal(f["niter"][0], r["niter"][0])
    n = x.shape[0]
    xtx, xty = x.T @ x / n, x.T @ y / n
    sf = np.linspace(0.5, 2.0, p)                                                # quirk Q5: in-place rescaling
    _cmp(oa.oem_xtx(xtx, xty, penalty=["lasso", "scad"], scale_factor=sf, nlambda=10),
         orc.fit_xtx(xtx, xty, penalty=["lasso", "scad"], scale_factor=sf, nlambda=10))


def test_more_lambdas_than_one_lds_chunk(oa):
    """the row-split kernel stages lambdas in LDS 1024 at a time"""
    x, y = _data(800, 72, 77)
    kw = dict(penalty=["lasso"], nlambda=1100, tol=1e-7)
    f, r = oa.oem(x, y, **kw), orc.fit_dense(x, y, **kw)
    _cmp(f, r)
    assert np.array_equal(f["niter"][0], r["niter"][0])
    lam = np.geomspace(3.0, 0.003, 1030)
    f, r = oa.oem(x, y, lambda_=[lam], penalty=["mcp"], tol=1e-7), orc.fit_dense(x, y, lambda_=[lam], penalty=["mcp"], tol=1e-7)
    _cmp(f, r)


@pytest.mark.parametrize("n", [129, 1000, 4097, 33331])
def test_ragged_rows_and_alignment(oa, n):
    """row counts that are not multiples of 8 / 32 / 64; odd n exercises the 8-byte-aligned host path"""
    x, y = _data(n, 21, n, mean=-4.0)
    kw = dict(penalty=["lasso"], nlambda=10, tol=1e-10)
    _cmp(oa.oem(x, y, **kw), orc.fit_dense(x, y, **kw))
    import torch
    xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t()          # device resident, column-major, ld = n
    _cmp(oa.oem(xd, y, **kw), orc.fit_dense(x, y, **kw))
    xr = torch.as_tensor(np.ascontiguousarray(x), device="cuda")                # row-major: transposed on the device
    _cmp(oa.oem(xr, y, **kw), orc.fit_dense(x, y, **kw))


def test_large_mean_and_constant_column(oa):
    x, y = _data(5000, 16, 3, mean=1.0e4, sd=1.0)                               # |mean| >> sd: no cancellation
    x[:, 5] = 3.25                                                               # zero variance -> scaleX := 1
    x = np.asfortranarray(x)
    kw = dict(penalty=["lasso", "mcp"], nlambda=12, tol=1e-10)
    _cmp(oa.oem(x, y, **kw), orc.fit_dense(x, y, **kw), tol=1e-8)


def test_tile_count_boundaries(oa):
    for p in (2, 14, 15, 16, 17, 110):                                           # p + 2 across the 16-column tile edges
        x, y = _data(1500, p, p, nnz=min(p, 5))
        kw = dict(penalty=["lasso"], nlambda=8, tol=1e-10)
        _cmp(oa.oem(x, y, **kw), orc.fit_dense(x, y, **kw))


@pytest.mark.parametrize("p", [46, 50, 54, 62, 66, 70, 82, 86, 94, 98, 102, 106])
@pytest.mark.parametrize("n", [4096, 3001, 10007])
def test_ring_strip_forms_of_the_moment_kernel(oa, p, n):
    """LDS-DMA ring Gram kernel, every strip form (last tile row with <= 4 / <= 8 / more real columns: 4x4x4 MFMA
    sub-blocks vs plain tiles), full and ragged slabs, against numpy"""
    import torch
    from oem_amd import _lib as L
    x, y = _data(n, p, 100 + p, mean=0.2)
    ld = n + (n & 1)
    xd = torch.zeros((p, ld), dtype=torch.float64, device="cuda")
    xd[:, :n] = torch.as_tensor(np.ascontiguousarray(x.T))
    yd = torch.as_tensor(y, device="cuda")
    sums = torch.zeros(L.sums_len(p), dtype=torch.float64, device="cuda")
    M = torch.zeros((p + 2, p + 2), dtype=torch.float64, device="cuda")
    ctx = oa.context()
    torch.cuda.synchronize()
    L.check(L.lib().oemgpu_shift_sums_dev(ctx, xd.data_ptr(), n, ld, p, yd.data_ptr(), sums.data_ptr()))
    L.check(L.lib().oemgpu_moments_dev(ctx, xd.data_ptr(), n, ld, p, yd.data_ptr(), sums.data_ptr(), M.data_ptr()))
    L.check(L.lib().oemgpu_synchronize(ctx))
    z = np.column_stack([x, y, np.ones(n)])
    want = np.tril(z.T @ z)
    got = np.tril(M.cpu().numpy().T)          # column-major buffer, lower triangle valid
    scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))
    assert np.abs((got - want) / scale).max() < 1e-12
    assert got[p + 1, p + 1] == n


# p -> super-block rows (eights, six, four) of gram_sb_deal: 111, 113, 120 (1, 0, 0); 130, 150 (0, 1, 1); 176, 192 (1, 0, 1);
# 200, 224 (1, 1, 0); 225 ... 256: 15-16 tile columns, the one-read eight-wave workgroup of gram_wd.hip; 272 (1, 1, 1); 300 (2, 0, 1); 330 (2, 1, 0); 400 (2, 1, 1); 520 (3, 1, 1); 700 (5, 0, 1); 720 (5, 1, 0)
@pytest.mark.parametrize("p,n", [(p, n) for p in (120, 200, 256, 300, 520) for n in (4096, 3001, 1000, 10010)]
                         + [(p, n) for p in (111, 113, 130, 150, 176, 192, 224, 225, 240, 241, 250, 272, 330, 400, 700, 720) for n in (3001, 4104)])
def test_shared_slab_moment_kernel(oa, p, n):
    """the workgroup-shared-slab Gram kernel (p + 2 > 112, aligned X): diagonal and off-diagonal super-blocks of every shape the
    deal into eights, a six and a four makes (8 x 8, 6 x 8, 4 x 8, 4 x 6 tiles; diagonal 8, 6 and 4), partial super-blocks (tile columns
    of padding), ragged row tails; shifted and un-shifted accumulation"""
    import torch
    from oem_amd import _lib as L
    from tests.checker_backend import shift_in_effect
    for mean in (0.2, 60.0):
        x, y = _data(n, p, 200 + p, mean=mean)
        ld = n + (n & 1)
        xd = torch.zeros((p, ld), dtype=torch.float64, device="cuda")
        xd[:, :n] = torch.as_tensor(np.ascontiguousarray(x.T))
        yd = torch.as_tensor(y, device="cuda")
        sums = torch.zeros(L.sums_len(p), dtype=torch.float64, device="cuda")
        M = torch.zeros((p + 2, p + 2), dtype=torch.float64, device="cuda")
        ctx = oa.context()
        torch.cuda.synchronize()
        L.check(L.lib().oemgpu_shift_sums_dev(ctx, xd.data_ptr(), n, ld, p, yd.data_ptr(), sums.data_ptr()))
        L.check(L.lib().oemgpu_moments_dev(ctx, xd.data_ptr(), n, ld, p, yd.data_ptr(), sums.data_ptr(), M.data_ptr()))
        L.check(L.lib().oemgpu_synchronize(ctx))
        c = shift_in_effect(sums.cpu().numpy(), p)
        z = np.column_stack([x - c[:p], y - c[p], np.ones(n)])
        want = z.T @ z
        got = M.cpu().numpy()
        scale = np.sqrt(np.outer(np.diag(want), np.diag(want))) + 1e-300
        assert np.abs((got - want) / scale).max() < 1e-11, (mean,)
        assert got[p + 1, p + 1] == n


@pytest.mark.parametrize("p", [161, 192, 225, 256, 497, 512, 1024])
@pytest.mark.parametrize("n,mean", [(20011, 0.3), (5000, 75.0), (64, 0.0), (70, 80.0), (200000, 0.0)])
def test_one_read_moment_kernel_against_numpy(oa, p, n, mean):
    """225 <= p <= 256 (config 5), 161 <= p <= 192 and the units of sixteen tile columns (p = 512, 1,024 and the fifteen below each):
    gram_wd.hip -- eight-wave workgroups that hold whole units of the triangle, X read once per unit -- against numpy, shifted and not,
    down to one 64-row step; and the plan says it IS that kernel (a planner regression that routed p = 512 back to the super-blocks
    of gram_sb_kernel would stay green otherwise: VERDICT r5)."""
    import torch
    from oem_amd import _lib as L
    from tests.checker_backend import shift_in_effect
    x, y = _data(n, p, 900 + p, mean=mean)
    ld = n + (n & 1)
    xd = torch.zeros((p, ld), dtype=torch.float64, device="cuda")
    xd[:, :n] = torch.as_tensor(np.ascontiguousarray(x.T))
    yd = torch.as_tensor(y, device="cuda")
    import ctypes as C
    ctx = oa.context()
    plan = (C.c_int64 * 8)()
    L.check(L.lib().oemgpu_selftest_gram_plan(n, p, 256, plan))
    assert plan[1] == plan[2] == plan[7] == -1, ("not the eight-wave one-read form", p, list(plan))
    sums = torch.zeros(L.sums_len(p), dtype=torch.float64, device="cuda")
    M = torch.zeros((p + 2, p + 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L.check(L.lib().oemgpu_shift_sums_dev(ctx, xd.data_ptr(), n, ld, p, yd.data_ptr(), sums.data_ptr()))
    L.check(L.lib().oemgpu_moments_dev(ctx, xd.data_ptr(), n, ld, p, yd.data_ptr(), sums.data_ptr(), M.data_ptr()))
    L.check(L.lib().oemgpu_synchronize(ctx))
    got = M.cpu().numpy()
    c = shift_in_effect(sums.cpu().numpy(), p)
    z = np.column_stack([x - c[:p], y - c[p], np.ones(n)])
    want = z.T @ z
    scale = np.sqrt(np.outer(np.diag(want), np.diag(want))) + 1e-300
    assert np.abs((got - want) / scale).max() < 1e-11
    assert got[p + 1, p + 1] == n


def test_xtx_matches_dense_and_oracle(oa, doc_kats):
    x, y = K.kat1()
    n = x.shape[0]
    xtx, xty = x.T @ x / n, x.T @ y / n
    a = oa.oem(x, y, penalty=["lasso", "mcp"], standardize=False, intercept=False)
    b = oa.oem_xtx(xtx, xty, penalty=["lasso", "mcp"])
    for m in range(2):
        assert np.abs(a["beta"][m][1:] - b["beta"][m]).max() < 1e-11       # ref docs: 8.8e-16 between its own two paths
    _cmp(b, orc.fit_xtx(xtx, xty, penalty=["lasso", "mcp"]))
    sf = np.linspace(0.5, 2.0, 50)
    _cmp(oa.oem_xtx(xtx, xty, penalty=["lasso", "scad"], scale_factor=sf, nlambda=20),
         orc.fit_xtx(xtx, xty, penalty=["lasso", "scad"], scale_factor=sf, nlambda=20))


@pytest.mark.parametrize("mean,shifted", [(0.3, False), (100.0, True)])
def test_moments_kernel_against_numpy(oa, mean, shifted):
    """the MFMA moment build alone: M = Z'Z for Z = [X - c | y - c_y | 1]; c = 0 unless a column has |mean| > 16 sd"""
    import torch
    from oem_amd import _lib as L
    from tests.checker_backend import shift_in_effect
    n, p = 10007, 100
    x, y = _data(n, p, 21, mean=mean)
    xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda")
    yd = torch.as_tensor(y, device="cuda")
    sums = torch.zeros(L.sums_len(p), dtype=torch.float64, device="cuda")
    M = torch.zeros((p + 2, p + 2), dtype=torch.float64, device="cuda")
    ctx = oa.context()
    torch.cuda.synchronize()
    L.check(L.lib().oemgpu_shift_sums_dev(ctx, xd.data_ptr(), n, n, p, yd.data_ptr(), sums.data_ptr()))
    L.check(L.lib().oemgpu_moments_dev(ctx, xd.data_ptr(), n, n, p, yd.data_ptr(), sums.data_ptr(), M.data_ptr()))
    L.check(L.lib().oemgpu_synchronize(ctx))
    c = shift_in_effect(sums.cpu().numpy(), p)
    assert bool(np.any(c != 0)) == shifted
    z = np.column_stack([x - c[:p], y - c[p], np.ones(n)])
    want = z.T @ z
    got = M.cpu().numpy()
    scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))
    assert np.abs(got - want).max() / scale.max() < 1e-13
    assert np.abs((got - want) / scale).max() < 1e-11
    assert got[p + 1, p + 1] == n


def test_eig_max(oa):
    import torch
    from oem_amd import _lib as L
    rng = np.random.default_rng(2)
    for p in (3, 50, 100, 190):
        a = rng.normal(size=(4 * p, p)); a = a.T @ a / (4 * p)
        ad = torch.as_tensor(a, device="cuda")
        out = C.c_double(0)
        L.check(L.lib().oemgpu_eig_max_dev(oa.context(), ad.data_ptr(), p, C.byref(out)))
        want = np.linalg.eigvalsh(a)[-1]
        assert abs(out.value - want) <= 1e-10 * want, (p, out.value, want)


def test_config1_shape_reduced_n(oa):
    """BASELINE config 1 (README.md:44-66) at n = 2e5: elastic.net alpha=1, intercept, no standardize, tol 1e-10"""
    rng = np.random.default_rng(123)
    n, p, m = 200000, 100, 25
    b = np.concatenate([rng.uniform(size=m), np.zeros(p - m)])
    x = np.asfortranarray(rng.normal(size=(n, p)) * 3.0)
    y = x @ b + rng.normal(size=n)
    kw = dict(penalty="elastic.net", intercept=True, standardize=False, tol=1e-10)
    fit, ref = oa.oem(x, y, **kw), orc.fit_dense(x, y, native=True, **kw)
    _cmp(fit, ref)
    assert np.abs(fit["niter"][0] - ref["niter"][0]).max() <= 1


def test_errors_are_the_references(oa):
    x, y = _data(100, 5, 1, nnz=3)
    with pytest.raises(ValueError, match="lambda.min.ratio must be between 0 and 1"):
        oa.oem(x, y, lambda_min_ratio=1.5)
    with pytest.raises(ValueError, match="x and y lengths do not match"):
        oa.oem(x, y[:-1])
    with pytest.raises(ValueError, match="groups must have same length"):
        oa.oem(x, y, penalty="grp.lasso", groups=[1, 2])
    with pytest.raises(oa.OemgpuError):
        oa.big_oem(x[:4], y[:4], penalty="lasso")                                #  big.oem's p >= n branch is out of the path


@pytest.mark.gpu
@pytest.mark.parametrize("n,p", [(40, 100), (64, 64), (3, 5), (120, 200), (200, 260), (150, 300)])
@pytest.mark.parametrize("std,icpt", [(True, True), (False, False)])
def test_wide_branch(oa, n, p, std, icpt):
    """p >= n (ref src/oem_dense.h:476-482,513-521): the reference takes d from XXt/n and iterates through X twice; the
    library runs the same iteration on the Gram.  Checked against the oracle's restatement of the reference's form."""
    x, y = _data(n, p, 21, nnz=min(6, p))
    groups = np.arange(p) // 5 + 1
    kw = dict(penalty=["lasso", "mcp", "grp.lasso"], groups=groups, nlambda=12, tol=1e-8, maxit=800,
              standardize=std, intercept=icpt)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = oa.oem(x, y, **kw)
    # R/oem.R:348-354: lambda.min.ratio defaults to 0.01 when n < p
    r = orc.fit_dense(x, y, lambda_min_ratio=0.01 if n < p else 0.0001, unique_groups=np.unique(groups), **kw)
    assert abs(f["d"] - r["d"]) < 1e-11 * r["d"]
    for k in range(3):
        assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-11)
        scale = max(1.0, float(np.abs(r["beta"][k]).max()))
        _report(f"branch n={n} p={p} std={std} {kw['penalty'][k]}", f, r, k, kw["tol"], kw["maxit"])
        _agree_with_oracle(f, r, k, kw["tol"], kw["penalty"][k])      # (the Gram form of the iteration against the reference's two products: same counts, 1e-13)


@pytest.mark.gpu
def test_results_written_straight_into_host_memory(oa, monkeypatch):
    """the row-split path kernel (p <= 208) stores its results into pinned host memory while it runs (no device-to-host copy
    behind it); OEM_NO_ZERO_COPY=1 takes the copy: the same bits, every output, several penalties, compute.loss, big.oem"""
    x, y = _data(5000, 60, 77, mean=0.5)
    groups = np.arange(60) // 4 + 1
    kw = dict(penalty=["lasso", "mcp", "grp.lasso", "ols"], groups=groups, nlambda=12, tol=1e-9, compute_loss=True)
    a = oa.oem(x, y, **kw)
    b_ = oa.big_oem(x, y, penalty=["lasso", "scad"], nlambda=9, tol=1e-9)
    monkeypatch.setenv("OEM_NO_ZERO_COPY", "1")
    c = oa.oem(x, y, **kw)
    d_ = oa.big_oem(x, y, penalty=["lasso", "scad"], nlambda=9, tol=1e-9)
    for u, v in ((a, c), (b_, d_)):
        assert u["d"] == v["d"]
        for key in ("beta", "lambda", "niter", "loss"):
            for k in range(len(u[key])):
                assert np.array_equal(np.asarray(u[key][k]), np.asarray(v[key][k])), key


@pytest.mark.gpu
@pytest.mark.parametrize("n,p", [(40, 100), (64, 64), (3, 5), (130, 200), (200, 1030), (700, 701)])
@pytest.mark.parametrize("flag", [0, 1, 2, 3])
def test_wide_engine(oa, n, p, flag, monkeypatch):
    """p >= n through the reference's OWN iteration (ref src/oem_dense.h:363-366, 476-482, 513-521): the standardised copy of X
    on the device, d from Lanczos on XXt/n applied as two products, u = X'(Y - X beta)/n + d beta -- no Gram matrix
    (wide.hip, path_large.hip: run_path_wide; OEM_WIDE=1 takes it at every size it can run).  All four DataStd flags; the fused
    form (element-wise operators: one read of X per iteration) and the general form (group operators, Nesterov's step,
    compute.loss around path_update_kernel), each against the oracle's restatement of the same branch."""
    monkeypatch.setenv("OEM_WIDE", "1")
    std, icpt = bool(flag & 1), bool(flag & 2)
    x, y = _data(n, p, 300 + n + flag, mean=0.4, nnz=min(6, p))
    groups = np.arange(p) // 5 + 1
    lmr = 0.01 if n < p else 0.0001                                   # R/oem.R:348-354
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for kw in (dict(penalty=["lasso", "mcp", "scad", "elastic.net", "ols"], alpha=0.6, nlambda=9, tol=1e-8, maxit=700),
                   dict(penalty=["lasso", "grp.lasso", "sparse.grp.lasso"], groups=groups, nlambda=7, tol=1e-8, maxit=700, compute_loss=True),
                   dict(penalty=["lasso"], nlambda=5, tol=1e-12, maxit=3),
                   dict(penalty=["mcp"], nlambda=6, tol=1e-8, maxit=700, accelerate=True)):
            f = oa.oem(x, y, standardize=std, intercept=icpt, **kw)
            okw = dict(kw)
            if "groups" in okw:
                okw["unique_groups"] = np.unique(groups)
            r = orc.fit_dense(x, y, lambda_min_ratio=lmr, standardize=std, intercept=icpt, **okw)
            assert abs(f["d"] - r["d"]) < 1e-10 * r["d"], (kw["penalty"], f["d"], r["d"])
            for k in range(len(kw["penalty"])):
                assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-11)
                _report(f"site1 n={n} p={p} {kw['penalty'][k]}", f, r, k, kw["tol"], kw["maxit"])
                _agree_with_oracle(f, r, k, kw["tol"], kw["penalty"][k])
                if kw.get("compute_loss"):
                    assert np.allclose(f["loss"][k], r["loss"][k], rtol=1e-8)
            if kw["maxit"] == 3:
                assert f["niter"][0].max() == 4
    # the same call on the Gram form: the two forms of the iteration agree
    monkeypatch.delenv("OEM_WIDE")
    monkeypatch.setenv("OEM_NO_WIDE", "1")
    kw = dict(penalty=["lasso", "mcp"], nlambda=8, tol=1e-9, maxit=700, standardize=std, intercept=icpt)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g = oa.oem(x, y, **kw)
        monkeypatch.delenv("OEM_NO_WIDE")
        monkeypatch.setenv("OEM_WIDE", "1")
        w = oa.oem(x, y, **kw)
    for k in range(2):
        assert np.abs(np.asarray(g["beta"][k]) - np.asarray(w["beta"][k])).max() < 1e-7 * max(1.0, float(np.abs(g["beta"][k]).max()))


def _path_kernel_cycles(oa, x, y, **kw):
    """shader cycles of the last persistent eigen + path kernel (0 for the launch-per-iteration engines), one device-resident call"""
    import ctypes as C
    import torch
    from oem_amd import _lib as L
    xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t()
    ctx = oa.context()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        oa.oem(xd, y, **kw)
    ms = (C.c_double * L.NTIMERS)()
    L.check(L.lib().oemgpu_last_timings(ctx, ms))
    return ms[6]                                                  # OEMGPU_T_PATHCYC



@pytest.mark.gpu
@pytest.mark.parametrize("n,p", [(3, 5), (30, 40), (64, 1100), (100, 1500), (130, 2100), (190, 700), (256, 3000), (300, 1300), (384, 900),
                                 (500, 2000), (513, 1100), (700, 1410), (1000, 1000), (1024, 1300), (200, 5000)])
def test_wide_cooperating_engine(oa, n, p, monkeypatch):
    """p >= n as ONE persistent launch of cooperating workgroups with the standardised X in registers (path_wcoop.hip): every column
    height (1 .. 16 registers per column and lane, 16 .. 4 columns per wave), one workgroup up to 141 (the engine takes up to 192), all-reduce slices that are
    ragged or empty, the element-wise operators with penalty factors, maxit reached, user lambdas, OLS, several penalties side by
    side in workgroup sets of their own -- against the oracle's restatement of the branch, and against the launch-per-iteration
    engine (OEM_NO_WCOOP=1), which must agree to rounding with the same iteration counts."""
    monkeypatch.setenv("OEM_WIDE", "1")
    x, y = _data(n, max(p, n), 900 + n + p, mean=0.3, nnz=min(7, p))
    p = x.shape[1]
    rng = np.random.default_rng(n + p)
    pf = rng.uniform(0.5, 2.0, p); pf[rng.integers(p)] = 0.0
    nlam = 6 if n * p < 1_000_000 else 4
    grp = np.minimum(np.arange(p) // 7, max(1, p // 9))            # ragged: the last group is long; ids start at 0 (group 0: unpenalised)
    grp = grp[rng.permutation(p)] if p < 600 else grp             # small p: members scattered over the workgroups
    calls = (dict(penalty=["lasso", "mcp", "scad", "elastic.net", "mcp.net", "scad.net", "ols"], alpha=0.7, gamma=3.5, nlambda=nlam, tol=1e-8, maxit=400,
                  penalty_factor=pf, standardize=True, intercept=True),
             dict(penalty=["lasso"], nlambda=4, tol=1e-12, maxit=3, standardize=False, intercept=True, compute_loss=True),
             dict(penalty=["scad", "lasso"], nlambda=5, tol=1e-9, maxit=300, standardize=False, intercept=False, compute_loss=True),
             dict(penalty=["mcp", "lasso"], lambda_=[np.array([0.5, 0.2, 0.05]), np.array([0.4, 0.1, 0.02])], tol=1e-8, maxit=300,
                  standardize=True, intercept=False),
             # the general form: u all-gathered, the operator stage replicated -- group operators (ragged groups, group 0, weights),
             # the sparse group lasso, Nesterov's step
             dict(penalty=["grp.lasso", "sparse.grp.lasso", "grp.mcp", "grp.scad.net", "lasso"], groups=grp, alpha=0.6, tau=0.4,
                  nlambda=nlam, tol=1e-8, maxit=400, penalty_factor=pf, standardize=True, intercept=True, compute_loss=True),
             dict(penalty=["lasso", "mcp", "grp.lasso"], groups=grp, nlambda=nlam, tol=1e-8, maxit=400, accelerate=True, standardize=False, intercept=True))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for kw in calls:
            f = oa.oem(x, y, **kw)
            monkeypatch.setenv("OEM_NO_WCOOP", "1")
            g = oa.oem(x, y, **kw)
            monkeypatch.delenv("OEM_NO_WCOOP")
            monkeypatch.setenv("OEM_WCOOP_ONE_SET", "1")
            h = oa.oem(x, y, **kw)
            monkeypatch.delenv("OEM_WCOOP_ONE_SET")
            if "groups" in kw:                                    # columns dealt in whole groups or 4 CW each: the same coefficients
                monkeypatch.setenv("OEM_WCOOP_NO_ALIGN", "1")
                h2 = oa.oem(x, y, **kw)
                monkeypatch.delenv("OEM_WCOOP_NO_ALIGN")
                for k in range(len(kw["penalty"])):
                    sc = max(1.0, float(np.abs(np.asarray(h2["beta"][k])).max()))
                    assert np.abs(np.asarray(f["beta"][k]) - np.asarray(h2["beta"][k])).max() < 1e-9 * sc
                    assert np.abs(np.ravel(f["niter"][k]).astype(int) - np.ravel(h2["niter"][k]).astype(int)).max() <= 1
            okw = dict(kw)
            if "groups" in okw:
                okw["unique_groups"] = np.unique(grp)
            r = _oracle_wide(x, y, f, lambda_min_ratio=0.01 if n < p else 0.0001, **okw)
            assert abs(f["d"] - r["d"]) < DTOL * r["d"], (f["d"], r["d"])
            assert abs(f["d"] - g["d"]) < DTOL * g["d"]
            for k in range(len(kw["penalty"])):
                # one workgroup set per penalty or one set walking them: the same bits
                assert np.array_equal(np.asarray(f["beta"][k]), np.asarray(h["beta"][k])) and np.array_equal(f["niter"][k], h["niter"][k])
                assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-11)
                scale = max(1.0, float(np.abs(r["beta"][k]).max()))
                assert np.abs(np.asarray(f["beta"][k]) - np.asarray(g["beta"][k])).max() < 1e-9 * scale, kw["penalty"][k]
                _report(f"site2 n={n} p={p} {kw['penalty'][k]}", f, r, k, kw["tol"], kw["maxit"])
                _agree_with_oracle(f, r, k, kw["tol"], kw["penalty"][k])
                dg = np.abs(np.ravel(f["niter"][k]).astype(int) - np.ravel(g["niter"][k]).astype(int))
                assert dg.max() <= 1, (kw["penalty"][k], dg)
                if kw.get("compute_loss"):
                    assert np.allclose(f["loss"][k], r["loss"][k], rtol=1e-8), kw["penalty"][k]
                    assert np.allclose(f["loss"][k], g["loss"][k], rtol=1e-9), kw["penalty"][k]
            if kw["maxit"] == 3:
                assert f["niter"][0].max() == 4
    # ONE persistent launch did the work (its cycle counter comes back), and the switch really selects the other engine
    kw1 = dict(penalty=["lasso"], nlambda=3, tol=1e-6, maxit=50)
    assert _path_kernel_cycles(oa, x, y, **kw1) > 0
    monkeypatch.setenv("OEM_NO_WCOOP", "1")
    assert _path_kernel_cycles(oa, x, y, **kw1) == 0
    monkeypatch.delenv("OEM_NO_WCOOP")


@pytest.mark.gpu
@pytest.mark.parametrize("n,p,forced", [(60, 13000, False), (128, 12600, False), (250, 13000, False), (3, 40, True), (100, 700, True),
                                        (130, 1900, True), (300, 1300, True), (500, 2100, True)])
def test_wide_streamed_engine(oa, n, p, forced, monkeypatch):
    """p >= n where the standardised X does not fit the registers: the STREAMED persistent form (path_wcoop.hip: path_wstream_kernel;
    the workgroups stay for the whole call and re-read their column tiles every iteration, the all-reduce in-kernel) -- where the
    library takes it by itself (short columns, p beyond the resident form) and forced onto small problems (OEM_WSTREAM=1 with
    OEM_NO_WCOOP=1: every column height it is built for, one chunk and several, ragged last chunks) -- against the oracle's
    restatement of the branch and against the launch-per-iteration engine."""
    monkeypatch.setenv("OEM_WIDE", "1")
    monkeypatch.setenv("OEM_NO_WRES", "1")                        # (round 4: these sizes now stay in registers, path_wres_kernel; the streamed form serves what is beyond it)
    if forced:
        monkeypatch.setenv("OEM_WSTREAM", "1"); monkeypatch.setenv("OEM_NO_WCOOP", "1")
    x, y = _data(n, p, 1700 + n + p, mean=0.3, nnz=min(7, p))
    rng = np.random.default_rng(n + p)
    pf = rng.uniform(0.5, 2.0, p); pf[rng.integers(p)] = 0.0
    calls = (dict(penalty=["lasso", "mcp", "scad.net", "ols"], alpha=0.7, gamma=3.5, nlambda=4, tol=1e-8, maxit=300, penalty_factor=pf,
                  standardize=True, intercept=True, compute_loss=True),
             dict(penalty=["lasso"], nlambda=3, tol=1e-12, maxit=3, standardize=False, intercept=True),
             dict(penalty=["scad"], lambda_=[np.array([0.5, 0.2, 0.05])], tol=1e-8, maxit=300, standardize=True, intercept=False))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for kw in calls:
            f = oa.oem(x, y, **kw)
            monkeypatch.setenv("OEM_NO_WSTREAM", "1")
            g = oa.oem(x, y, **kw)
            monkeypatch.delenv("OEM_NO_WSTREAM")
            r = _oracle_wide(x, y, f, lambda_min_ratio=0.01 if n < p else 0.0001, **kw)
            assert abs(f["d"] - r["d"]) < DTOL * r["d"], (f["d"], r["d"])
            assert abs(f["d"] - g["d"]) < DTOL * g["d"]
            for k in range(len(kw["penalty"])):
                assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-11)
                scale = max(1.0, float(np.abs(r["beta"][k]).max()))
                assert np.abs(np.asarray(f["beta"][k]) - np.asarray(g["beta"][k])).max() < 1e-9 * scale, kw["penalty"][k]
                _report(f"site3 n={n} p={p} {kw['penalty'][k]}", f, r, k, kw["tol"], kw["maxit"])
                _agree_with_oracle(f, r, k, kw["tol"], kw["penalty"][k])
                dg = np.abs(np.ravel(f["niter"][k]).astype(int) - np.ravel(g["niter"][k]).astype(int))
                assert dg.max() <= 1, (kw["penalty"][k], dg)
                if kw.get("compute_loss"):
                    assert np.allclose(f["loss"][k], r["loss"][k], rtol=1e-8), kw["penalty"][k]
            if kw["maxit"] == 3:
                assert f["niter"][0].max() == 4
    kw1 = dict(penalty=["lasso"], nlambda=3, tol=1e-6, maxit=50)
    assert _path_kernel_cycles(oa, x, y, **kw1) > 0               # the persistent kernel's cycle counter
    monkeypatch.setenv("OEM_NO_WSTREAM", "1")
    assert _path_kernel_cycles(oa, x, y, **kw1) == 0
    monkeypatch.delenv("OEM_NO_WSTREAM")


@pytest.mark.gpu
@pytest.mark.parametrize("streamed", [False, True])
def test_persistent_wide_engines_fall_back_when_their_exchange_times_out(oa, streamed, monkeypatch):
    """the persistent p >= n engines need all their workgroups resident at once; when somebody else holds the CUs their exchanges time
    out and poison the result (d_out[6]) -- the host then makes the call again on the launch-per-iteration engine instead of failing.
    OEM_WCOOP_FAKE_TIMEOUT=1 sets the poison behind a kernel that ran: the caller must get exactly the launch engine's answer."""
    monkeypatch.setenv("OEM_WIDE", "1")
    if streamed:
        monkeypatch.setenv("OEM_WSTREAM", "1"); monkeypatch.setenv("OEM_NO_WCOOP", "1")
    x, y = _data(200, 1500, 4242, mean=0.2, nnz=6)
    kw = dict(penalty=["lasso", "mcp"], nlambda=5, tol=1e-8, maxit=300)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        good = oa.oem(x, y, **kw)
        monkeypatch.setenv("OEM_WCOOP_FAKE_TIMEOUT", "1")
        back = oa.oem(x, y, **kw)
        assert _path_kernel_cycles(oa, x, y, **kw) == 0           # what answered in the end was the launch-per-iteration engine
        monkeypatch.delenv("OEM_WCOOP_FAKE_TIMEOUT")
        assert _path_kernel_cycles(oa, x, y, **kw) > 0
        monkeypatch.setenv("OEM_NO_WSTREAM" if streamed else "OEM_NO_WCOOP", "1")
        launches = oa.oem(x, y, **kw)
    for k in range(2):
        assert np.array_equal(np.asarray(back["beta"][k]), np.asarray(launches["beta"][k])) and np.array_equal(back["niter"][k], launches["niter"][k])
        assert np.abs(np.asarray(back["beta"][k]) - np.asarray(good["beta"][k])).max() < 1e-9


@pytest.mark.gpu
def test_cooperating_gram_engine_falls_back_when_its_exchange_times_out(oa, monkeypatch):
    """the same for 208 < p <= 1024 (path_coop.hip): a poisoned exchange sends the call to the launch-per-iteration engine"""
    x, y = _data(3000, 400, 777, mean=0.1, nnz=8)
    kw = dict(penalty=["grp.lasso"], groups=np.arange(400) // 8 + 1, nlambda=8, tol=1e-9, compute_loss=True)
    good = oa.oem(x, y, **kw)
    monkeypatch.setenv("OEM_WCOOP_FAKE_TIMEOUT", "1")
    back = oa.oem(x, y, **kw)
    monkeypatch.delenv("OEM_WCOOP_FAKE_TIMEOUT")
    monkeypatch.setenv("OEM_NO_COOP", "1")
    launches = oa.oem(x, y, **kw)
    assert np.array_equal(np.asarray(back["beta"][0]), np.asarray(launches["beta"][0])) and np.array_equal(back["niter"][0], launches["niter"][0])
    assert np.abs(np.asarray(back["beta"][0]) - np.asarray(good["beta"][0])).max() < 1e-9
    assert np.allclose(back["loss"][0], good["loss"][0], rtol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("n,p", [(1100, 1200), (1500, 1501), (2048, 2100), (2049, 2100), (2500, 2600)])
def test_wide_engine_tall_columns(oa, n, p, monkeypatch):
    """the column heights that take 24 and 32 registers per lane (four waves per workgroup), and beyond 2048 rows the ROW-BLOCKED
    form: the rows in blocks of <= 2048, the two products as passes of their own (t = Xs beta block by block, g = Xs' t / n as
    per-block partial sums added in block order) around the single-workgroup update kernel -- element-wise and group penalties,
    compute.loss, against the oracle's restatement of the branch"""
    monkeypatch.setenv("OEM_WIDE", "1")
    x, y = _data(n, p, 40 + n, mean=0.2, nnz=8)
    groups = np.arange(p) // 6 + 1
    kw = dict(penalty=["lasso", "mcp", "grp.lasso"], groups=groups, nlambda=4, tol=1e-8, maxit=80, compute_loss=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = oa.oem(x, y, **kw)
        r = _oracle_wide(x, y, f, lambda_min_ratio=0.01, unique_groups=np.unique(groups), **kw)
    assert abs(f["d"] - r["d"]) < DTOL * r["d"]
    for k in range(3):
        _report(f"tall n={n} p={p} {kw['penalty'][k]}", f, r, k, kw["tol"], kw["maxit"])
        _agree_with_oracle(f, r, k, kw["tol"], kw["penalty"][k])
        assert np.allclose(f["loss"][k], r["loss"][k], rtol=1e-8)
    kw = dict(penalty=["lasso"], nlambda=4, tol=1e-8, maxit=80)       # element-wise alone: the fused form up to 2048 rows
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = oa.oem(x, y, **kw)
        r = _oracle_wide(x, y, f, lambda_min_ratio=0.01, **kw)
    _report(f"tall-fused n={n} p={p} lasso", f, r, 0, kw["tol"], kw["maxit"])
    _agree_with_oracle(f, r, 0, kw["tol"], "lasso, fused form")


@pytest.mark.gpu
def test_wide_engine_group_penalties_beyond_one_workgroups_lds(oa):
    """p >= n with group penalties where the operand of the group stage (u and the group factors: p + ngroups doubles) does not
    fit the LDS of the update kernel's one workgroup -- p + ngroups beyond about 19,900 used to return OEMGPU_ERR_UNSUPPORTED
    (the reference has no such limit, ref src/oem_dense.h:277-315, 513-521).  They now live in global memory there.
    500 x 30,000, 3,000 groups of 10 (group 0 unpenalised, weights), grp.lasso + sparse.grp.lasso + grp.mcp, against the oracle."""
    rng = np.random.default_rng(4)
    n, p = 500, 30_000
    x = np.asfortranarray(rng.normal(size=(n, p)) + 0.1)
    b = np.zeros(p); b[:20] = rng.uniform(0.5, 1.5, 20)
    y = x @ b + rng.normal(size=n)
    groups = np.arange(p) // 10                                     # ids 0 .. 2999: group 0 is not penalised
    gw = rng.uniform(0.5, 2.0, 3000)
    kw = dict(penalty=["grp.lasso", "sparse.grp.lasso", "grp.mcp"], groups=groups, group_weights=gw, tau=0.3, nlambda=3, tol=1e-8, maxit=25,
              compute_loss=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = oa.oem(x, y, **kw)
        r = _oracle_wide(x, y, f, lambda_min_ratio=0.01, unique_groups=np.unique(groups), **kw)
    assert abs(f["d"] - r["d"]) < DTOL * r["d"]
    for k in range(3):
        _agree_with_oracle(f, r, k, kw["tol"], kw["penalty"][k])
        assert np.allclose(f["loss"][k], r["loss"][k], rtol=1e-8)
        assert np.any(np.asarray(f["beta"][k])[1:, -1] != 0)
    # without compute.loss the groups -- runs of neighbouring columns -- take the fused group kernel: the same coefficients
    kw.pop("compute_loss")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        h = oa.oem(x, y, **kw)
    for k in range(3):
        _agree_with_oracle(h, r, k, kw["tol"], kw["penalty"][k])


@pytest.mark.gpu
@pytest.mark.parametrize("n,p", [(120, 9000), (300, 14000), (600, 5000), (1100, 4100), (2000, 2600)])
def test_wide_fused_group_kernel(oa, n, p, monkeypatch):
    """p >= n beyond the persistent engines with group penalties whose groups are runs of neighbouring columns: ONE launch + the
    reduction per iteration (path_large.hip: wide_groups_kernel -- a run is coordinate-local to a wave: u of its members, the norm
    in member order, the factor, the coefficients; a column is read again only where its coefficient is not zero) instead of four
    launches around the one-workgroup update kernel.  Ragged runs (1 .. 23 members), group 0 unpenalised, weights, all four group
    operators and element-wise penalties in the same call, penalty factors, maxit reached, several column heights -- against the
    oracle and against the general form (OEM_WIDE_NO_GROUP_FUSED=1), which must agree to rounding with the same iteration counts."""
    monkeypatch.setenv("OEM_WIDE", "1"); monkeypatch.setenv("OEM_NO_WCOOP", "1"); monkeypatch.setenv("OEM_NO_WSTREAM", "1")
    x, y = _data(n, p, 5100 + n, mean=0.2, nnz=8)
    rng = np.random.default_rng(n + p)
    sizes = []
    while sum(sizes) < p:
        sizes.append(int(rng.integers(1, 24)))
    sizes[-1] -= sum(sizes) - p
    ids = rng.permutation(len(sizes))                                # group ids in no particular order along the columns; id 0 is unpenalised
    groups = np.repeat(ids, sizes)
    gw = rng.uniform(0.5, 2.0, len(sizes))
    pf = rng.uniform(0.5, 2.0, p); pf[rng.integers(p)] = 0.0
    for kw in (dict(penalty=["grp.lasso", "sparse.grp.lasso", "lasso", "grp.mcp", "grp.scad.net"], groups=groups, group_weights=gw, penalty_factor=pf, alpha=0.6,
                    tau=0.4, nlambda=3, tol=1e-8, maxit=60),
               dict(penalty=["grp.lasso"], groups=groups, nlambda=3, tol=1e-12, maxit=3, standardize=False, intercept=True)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            f = oa.oem(x, y, **kw)
            monkeypatch.setenv("OEM_WIDE_NO_GROUP_FUSED", "1")
            g = oa.oem(x, y, **kw)
            monkeypatch.delenv("OEM_WIDE_NO_GROUP_FUSED")
            r = _oracle_wide(x, y, f, lambda_min_ratio=0.01, unique_groups=np.unique(groups), **kw)
        assert abs(f["d"] - r["d"]) < DTOL * r["d"]
        for k in range(len(kw["penalty"])):
            _agree_with_oracle(f, r, k, kw["tol"], kw["penalty"][k])
            scale = max(1.0, float(np.abs(np.asarray(g["beta"][k])).max()))
            assert np.abs(np.asarray(f["beta"][k]) - np.asarray(g["beta"][k])).max() < 1e-10 * scale, kw["penalty"][k]
            assert np.abs(np.ravel(f["niter"][k]).astype(int) - np.ravel(g["niter"][k]).astype(int)).max() <= 1
        if kw["maxit"] == 3:
            assert f["niter"][0].max() == 4


@pytest.mark.gpu
@pytest.mark.parametrize("n,p,route", [(40, 100, "chosen"), (45, 131, "chosen"), (64, 600, "chosen"), (200, 1030, "chosen"), (300, 2500, "chosen"), (120, 9000, "chosen"),
                                       (40, 100, "two products"), (64, 600, "two products")])
@pytest.mark.parametrize("standardize", [False, True])
def test_big_and_sparse_wide_branch_without_an_intercept(oa, n, p, route, standardize, monkeypatch):
    """big.oem() and oem() on a sparse x with nobs <= nvars and intercept = FALSE (ref src/oem_big.h:537-541, 568-584, 743-764,
    880-897; src/oem_sparse.h:607-612, 638-647; VERDICT r3: refused until round 4): the reference iterates on the data as they
    are, takes lambda_zero from the scaled X'y and returns beta colsq_inv -- the wide engines on the DataStd-flag-0 copy with the
    column scales applied where the reference applies them.  Against the oracle (pinned on the dense branch and on the KKT
    conditions, tests/test_oracle_independent.py): element-wise and group penalties, row shards, a sparse x.  With an intercept
    the reference's expression is ill-formed: refused, with the reason."""
    import scipy.sparse as sp
    if route == "two products":                                     # (round 5: the library takes the Gram form of the same iteration where
        monkeypatch.setenv("OEM_WIDE", "1")                         #  that is faster -- p <= 1024 -- as it does for oemDense; this forces the other)
    rng = np.random.default_rng(n + p)
    x = rng.normal(size=(n, p)) * rng.uniform(0.5, 3.0, p)
    x[rng.random((n, p)) < 0.7] = 0.0
    x[:, 5] = 0.0                                                   # (a column of zeros: colsq falls back to 1, ref src/oem_big.h:757-760)
    x = np.asfortranarray(x)
    b = np.zeros(p); b[:6] = rng.uniform(1, 2, 6)
    y = x @ b + 0.5 * rng.normal(size=n)
    groups = np.arange(p) // 4 + 1
    kw = dict(penalty=["lasso", "mcp", "grp.lasso", "elastic.net"], groups=groups, alpha=0.7, nlambda=5, lambda_min_ratio=0.05, tol=1e-9, maxit=400,
              standardize=standardize, intercept=False)
    r = orc.fit_big(x, y, native=True, unique_groups=np.unique(groups), **kw)
    f = oa.big_oem(x, y, **kw)
    cuts = [0, n // 3, n // 3, n]                                   # three row shards, one of them empty
    fs = oa.big_oem([x[cuts[i]:cuts[i + 1]] for i in range(3)], [y[cuts[i]:cuts[i + 1]] for i in range(3)], **kw)
    assert abs(f["d"] - r["d"]) <= DTOL * r["d"]
    for k in range(4):
        assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-12)
        _agree_with_oracle(f, r, k, kw["tol"], kw["penalty"][k])
        assert np.array_equal(np.asarray(f["beta"][k]), np.asarray(fs["beta"][k]))
        assert np.all(np.asarray(f["beta"][k])[0] == 0.0)
    # (with compute.loss: oemSparse::get_loss takes the residual of the returned coefficients, ref src/oem_sparse.h:932-941)
    skw = dict(penalty=["lasso", "scad"], nlambda=5, lambda_min_ratio=0.05, tol=1e-9, maxit=400, standardize=standardize, intercept=False, compute_loss=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g = oa.oem(sp.csc_matrix(x), y, **skw)
    rs = orc.fit_sparse(sp.csc_matrix(x), y, native=True, **skw)
    assert abs(g["d"] - rs["d"]) <= DTOL * rs["d"]
    for k in range(2):
        _agree_with_oracle(g, rs, k, skw["tol"], skw["penalty"][k])
        assert np.allclose(np.ravel(g["loss"][k]), np.ravel(rs["loss"][k]), rtol=1e-7), (g["loss"][k], rs["loss"][k])
    with pytest.raises(oa.OemgpuError, match="p \\+ 1 entries"):
        oa.big_oem(x, y, penalty="lasso", standardize=standardize, intercept=True)
    with pytest.raises(oa.OemgpuError, match="p \\+ 1 entries"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        oa.oem(sp.csc_matrix(x), y, penalty="lasso", standardize=standardize, intercept=True)


@pytest.mark.gpu
def test_p_ge_n_on_the_register_resident_gram_engine(oa, monkeypatch):
    """p >= n with 1024 < p <= 4096 where the persistent wide engine cannot hold X (here n > 1024): since round 4 the Gram form of the
    iteration on the register-resident engine (path_symcoop.hip: ~6 us per iteration) instead of the wide engine's launches (~20):
    api.hip: wide_pays.  Same iteration (the non-zero spectra of XX' and X'X coincide): against the oracle's two-product restatement
    and against the wide engine (OEM_WIDE=1)."""
    import ctypes as C
    import torch
    rng = np.random.default_rng(77)
    n, p = 1300, 3000
    x = np.asfortranarray(rng.normal(size=(n, p)) + 0.2)
    y = x[:, :8] @ rng.uniform(0.5, 1.5, 8) + rng.normal(size=n)
    xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t()
    kw = dict(penalty=["lasso", "mcp"], nlambda=5, tol=1e-9, maxit=300)
    ms = (C.c_double * 8)()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = oa.oem(xd, y, **kw)
        assert oa.lib().oemgpu_last_timings(oa.context(), ms) == 0 and ms[6] > 0          # one persistent launch
        monkeypatch.setenv("OEM_WIDE", "1")
        w = oa.oem(xd, y, **kw)
        monkeypatch.delenv("OEM_WIDE")
    r = _oracle_wide(x, y, f, lambda_min_ratio=0.01, **kw)
    for k in range(2):
        _agree_with_oracle(f, r, k, kw["tol"], kw["penalty"][k])
        _agree_with_oracle(w, r, k, kw["tol"], kw["penalty"][k])


@pytest.mark.gpu
def test_wide_engine_where_it_is_chosen(oa):
    """the sizes the library itself sends to the wide engine (p > 1024, 2 n < p): device-resident and host x, against the oracle;
    and p = 20,000 (a Gram matrix would be 3.2 GB per iteration) through the lasso KKT conditions on the standardised data."""
    import torch
    rng = np.random.default_rng(8)
    n, p = 300, 2500
    x = np.asfortranarray(rng.normal(size=(n, p)) * 2.0 + 0.3)
    y = x[:, :8] @ rng.uniform(0.5, 1.5, 8) + rng.normal(size=n)
    kw = dict(penalty=["lasso", "mcp"], nlambda=10, tol=1e-8, maxit=1000)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fh = oa.oem(x, y, **kw)
        fd = oa.oem(torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t(), y, **kw)
        buf = torch.zeros((p, n + 7), dtype=torch.float64, device="cuda")      # a column-major view with a leading dimension > n
        buf[:, :n] = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda")
        fl = oa.oem(buf[:, :n].t(), y, **kw)
    r = _oracle_wide(x, y, fh, lambda_min_ratio=0.01, **kw)
    assert all(np.array_equal(np.asarray(fl["beta"][k]), np.asarray(fd["beta"][k])) for k in range(2))
    for f in (fh, fd):
        assert abs(f["d"] - r["d"]) < 1e-10 * r["d"]
        for k in range(2):
            _report(f"chosen n={n} p={p} {kw['penalty'][k]}", f, r, k, kw["tol"], kw["maxit"])
            _agree_with_oracle(f, r, k, kw["tol"], kw["penalty"][k])
    # beyond 2048 rows the library takes the row-blocked form by itself (here two blocks of 1050 rows)
    n, p = 2100, 4300
    x = np.asfortranarray(rng.normal(size=(n, p)) + 0.1)
    y = x[:, :8] @ rng.uniform(0.5, 1.5, 8) + rng.normal(size=n)
    kw = dict(penalty=["lasso"], nlambda=3, tol=1e-8, maxit=100)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = oa.oem(x, y, **kw)
    r = _oracle_wide(x, y, f, lambda_min_ratio=0.01, **kw)
    assert abs(f["d"] - r["d"]) < 1e-10 * r["d"]
    _report(f"chosen-blocks n={n} p={p} lasso", f, r, 0, kw["tol"], kw["maxit"])
    _agree_with_oracle(f, r, 0, kw["tol"], "lasso, row blocks")
    n, p = 500, 20_000
    x = np.asfortranarray(rng.normal(size=(n, p)))
    b = np.zeros(p); b[:10] = rng.uniform(1.0, 2.0, 10)
    y = x @ b + rng.normal(size=n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = oa.oem(x, y, penalty="lasso", nlambda=12, tol=1e-9, maxit=5000, standardize=False, intercept=False)
    beta, lam = f["beta"][0][1:], f["lambda"][0]
    assert np.all(beta[:, 0] == 0) and f["niter"][0][0] == 1
    grad = x.T @ (y[:, None] - x @ beta) / n
    for i in (1, 4, 8):
        if f["niter"][0][i] > 5000:
            continue
        nz = beta[:, i] != 0
        assert np.abs(grad[~nz, i]).max() <= lam[i] * (1 + 1e-6)
        assert np.abs(grad[nz, i] - lam[i] * np.sign(beta[nz, i])).max() <= 1e-6 * lam[0]
    s = np.linalg.svd(x, compute_uv=False)[0]
    assert abs(f["d"] - 1.005 * s * s / n) <= 1e-9 * f["d"]


@pytest.mark.gpu
@pytest.mark.parametrize("std,icpt", [(True, True), (False, True), (True, False), (False, False)])
def test_sparse_x(oa, std, icpt):
    """oem() on a sparse x (ref src/oem_sparse.{h,cpp}, n > p): oemSparse's own standardisation and intercept handling (the
    intercept as a Gram column of value sqrt(mean diag / n), rescaled in place after every lambda), against the oracle's
    restatement; without intercept and standardisation it is the dense fit (the reference's doc example: 1.6e-15)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(41)
    n, p = 6000, 57
    x = sp.random(n, p, density=0.03, random_state=5, format="csc", data_rvs=lambda k: rng.normal(size=k) * 2.0)
    b = np.zeros(p); b[:6] = [1.0, -1.0, 0.5, 2.0, -0.7, 0.3]
    y = x @ b + rng.normal(size=n) * 0.5 + 0.8
    groups = np.arange(p) // 4 + 1
    pens = ["lasso", "mcp", "grp.lasso", "ols"]
    kw = dict(penalty=pens, groups=groups, nlambda=15, tol=1e-9, maxit=1000, standardize=std, intercept=icpt)
    f = oa.oem(x, y, compute_loss=True, **kw)
    rg, rug = orc.r_sparse_groups(groups, icpt)
    r = orc.fit_sparse(x, y, lambda_min_ratio=1e-4, compute_loss=True, **dict(kw, groups=rg, unique_groups=rug))
    assert abs(f["d"] - r["d"]) < 1e-11 * r["d"]
    for k in range(len(pens)):
        assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-11)
        assert np.allclose(np.ravel(f["loss"][k]), np.ravel(r["loss"][k]), rtol=1e-9)
        assert np.abs(f["beta"][k] - r["beta"][k]).max() < 1e-8 * max(1.0, float(np.abs(r["beta"][k]).max())), pens[k]
        dn = np.abs(np.ravel(f["niter"][k]).astype(int) - np.ravel(r["niter"][k]))
        assert dn.max() <= 1, (pens[k], dn)
    if not std and not icpt:
        g = oa.oem(np.asfortranarray(x.toarray()), y, **kw)
        for k in range(len(pens)):
            assert np.abs(f["beta"][k] - g["beta"][k]).max() < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("n,p,dens", [(20000, 57, 0.01), (9000, 130, 0.03), (40000, 8, 0.2), (8193, 33, 0.002), (5000, 300, 0.01)])
def test_sparse_x_compressed_column_gram(oa, monkeypatch, n, p, dens):
    """the compressed-column moment kernel (sparse.hip: LDS copy of a row chunk of one column, the other columns gathered against it)
    and the zero-filled tiles through the MFMA pass are two routes to the same moment buffer: same fits, both the oracle's"""
    import scipy.sparse as sp
    rng = np.random.default_rng(n + p)
    x = sp.random(n, p, density=dens, random_state=3, format="csc", data_rvs=lambda k: rng.normal(size=k) * 1.5)
    x = sp.csc_matrix(x); x[:, p - 1] = 0.0; x.eliminate_zeros()                 # an empty column on the way
    b = np.zeros(p); b[:5] = [1.0, -1.0, 0.5, 2.0, -0.7]
    y = x @ b + rng.normal(size=n) * 0.5 + 0.8
    kw = dict(penalty=["lasso", "mcp"], nlambda=8, tol=1e-9, maxit=2000)
    monkeypatch.setenv("OEM_SPARSE_GRAM", "csc")
    a = oa.oem(x, y, **kw)
    monkeypatch.setenv("OEM_SPARSE_GRAM", "dense")
    d = oa.oem(x, y, **kw)
    r = orc.fit_sparse(x, y, lambda_min_ratio=1e-4, **kw)
    assert abs(a["d"] - r["d"]) < 1e-10 * r["d"]
    for k in range(2):
        assert np.abs(a["beta"][k] - d["beta"][k]).max() < 1e-9
        assert np.abs(a["beta"][k] - r["beta"][k]).max() < 1e-8 * max(1.0, float(np.abs(r["beta"][k]).max()))
    monkeypatch.setenv("OEM_SPARSE_GRAM", "csc")
    a2 = oa.oem(x, y, **kw)
    assert np.array_equal(a["beta"][0], a2["beta"][0])                            # fixed summation order: bitwise reproducible


@pytest.mark.gpu
def test_sparse_x_groups_follow_the_variables(oa):
    """with an intercept the group vector of a sparse x has p + 1 entries, slot 0 the intercept's unpenalised group 0
    (ref R/oem.R:296-338, src/oem_sparse.h:465).  The LAST variable sits in an active group here: one slot off, it would be in no
    group and forced to 0.  Converged group-lasso fits of the sparse and the dense copy of x are the same optimum (standardize =
    FALSE, unpenalised intercept on both sides)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(47)
    n, p = 4000, 24
    x = sp.random(n, p, density=0.2, random_state=3, format="csc", data_rvs=lambda k: rng.normal(size=k))
    b = np.zeros(p); b[-4:] = [1.5, -1.0, 0.8, 2.0]; b[:4] = [0.5, 0.0, -0.6, 0.0]
    y = x @ b + rng.normal(size=n) * 0.3 + 0.4
    groups = np.arange(p) // 4 + 1
    dense = oa.oem(np.asfortranarray(x.toarray()), y, penalty=["grp.lasso"], groups=groups, nlambda=8, standardize=False, tol=1e-13, maxit=100000)
    lam = dense["lambda"][0]
    f = oa.oem(x, y, penalty=["grp.lasso"], groups=groups, lambda_=lam, standardize=False, tol=1e-13, maxit=100000)
    assert np.abs(f["beta"][0][-1, 1:]).min() > 0.5                      # the last variable is alive from the second lambda on
    assert np.abs(f["beta"][0] - dense["beta"][0]).max() < 1e-7
    rg, rug = orc.r_sparse_groups(groups, True)
    assert rg.shape == (p + 1,) and rg[0] == 0 and rug[0] == 0
    r = orc.fit_sparse(x, y, penalty=["grp.lasso"], groups=rg, unique_groups=rug, lambda_=lam, standardize=False, tol=1e-13, maxit=100000)
    assert np.abs(f["beta"][0] - r["beta"][0]).max() < 1e-9


@pytest.mark.gpu
def test_sparse_x_large_p_engine(oa):
    """p + 1 = 301 > 288: the sparse fit on the launch-per-iteration engine (the in-place rescale of the intercept slot rides on
    its scale.factor path)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(43)
    n, p = 5000, 300
    x = sp.random(n, p, density=0.04, random_state=9, format="csc", data_rvs=lambda k: rng.normal(size=k))
    b = np.zeros(p); b[:8] = rng.uniform(0.5, 1.5, 8)
    y = x @ b + rng.normal(size=n) * 0.3 + 1.2
    kw = dict(penalty=["lasso", "scad"], nlambda=10, tol=1e-9, maxit=600)
    f = oa.oem(x, y, **kw)
    r = orc.fit_sparse(x, y, lambda_min_ratio=1e-4, **kw)
    assert abs(f["d"] - r["d"]) < 1e-11 * r["d"]
    for k in range(2):
        assert np.abs(f["beta"][k] - r["beta"][k]).max() < 1e-8 * max(1.0, float(np.abs(r["beta"][k]).max()))
        assert np.abs(np.ravel(f["niter"][k]).astype(int) - np.ravel(r["niter"][k])).max() <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("n,p", [(3, 700), (40, 1200), (64, 5200), (100, 2500), (128, 9000), (130, 2100), (192, 5000), (200, 1000), (256, 3000), (300, 1300),
                                 (384, 2000), (500, 2000), (512, 1300), (380, 2500), (700, 1410), (768, 1100), (1000, 1000), (1024, 1300)])
def test_wide_engine_resident_in_the_accumulator_file(oa, n, p, monkeypatch):
    """p >= n with more column sets of every wave in the ACCUMULATOR file (path_wcoop.hip: path_wres_kernel, round 4 -- Xs up to ~11 M
    entries stays in registers).  OEM_WRES=1 takes it also where the vector registers alone would do, so every
    column height it is built for (1, 2, 3, 4, 6, 8, 12, 16 registers per column and lane: 9 .. 3 column sets per wave), ragged last sets and
    workgroups, all-reduce slices that are ragged or empty run here at sizes the oracle finishes: element-wise operators with penalty
    factors, maxit reached, user lambdas, OLS, compute.loss, all four standardisation flags -- against the oracle's restatement of
    the branch and the launch-per-iteration engine; and the host's fallback when its exchange times out."""
    monkeypatch.setenv("OEM_WIDE", "1")
    monkeypatch.setenv("OEM_WRES", "1")
    x, y = _data(n, p, 4100 + n + p, mean=0.3, nnz=min(7, p))
    rng = np.random.default_rng(n + p)
    pf = rng.uniform(0.5, 2.0, p); pf[rng.integers(p)] = 0.0
    nlam = 6 if n * p < 1_000_000 else 4
    calls = (dict(penalty=["lasso", "mcp", "scad", "elastic.net", "mcp.net", "scad.net", "ols"], alpha=0.7, gamma=3.5, nlambda=nlam, tol=1e-8, maxit=400,
                  penalty_factor=pf, standardize=True, intercept=True, compute_loss=True),
             dict(penalty=["lasso"], nlambda=4, tol=1e-12, maxit=3, standardize=False, intercept=True, compute_loss=True),
             dict(penalty=["scad", "lasso"], nlambda=5, tol=1e-9, maxit=300, standardize=False, intercept=False),
             dict(penalty=["mcp", "lasso"], lambda_=[np.array([0.5, 0.2, 0.05]), np.array([0.4, 0.1, 0.02])], tol=1e-8, maxit=300,
                  standardize=True, intercept=False))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for ci, kw in enumerate(calls):
            f = oa.oem(x, y, **kw)
            monkeypatch.setenv("OEM_NO_WCOOP", "1")               # (also switches path_wres_kernel off: the launches)
            g = oa.oem(x, y, **kw)
            monkeypatch.delenv("OEM_NO_WCOOP")
            monkeypatch.delenv("OEM_WRES")                        # the default selection: path_wcoop_kernel where it fits
            h = oa.oem(x, y, **kw)
            monkeypatch.setenv("OEM_WRES", "1")
            r = _oracle_wide(x, y, f, lambda_min_ratio=0.01 if n < p else 0.0001, **kw)
            assert abs(f["d"] - r["d"]) < DTOL * r["d"], (f["d"], r["d"])
            for k in range(len(kw["penalty"])):
                assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-11)
                scale = max(1.0, float(np.abs(r["beta"][k]).max()))
                for other in (g, h):
                    assert np.abs(np.asarray(f["beta"][k]) - np.asarray(other["beta"][k])).max() < 1e-9 * scale, kw["penalty"][k]
                    assert np.abs(np.ravel(f["niter"][k]).astype(int) - np.ravel(other["niter"][k]).astype(int)).max() <= 1
                _agree_with_oracle(f, r, k, kw["tol"], kw["penalty"][k])
                if kw.get("compute_loss"):
                    assert np.allclose(f["loss"][k], r["loss"][k], rtol=1e-8), kw["penalty"][k]
            if ci == 0:                                           # which kernel family ran (device-resident x: the call is on oa.context())
                import torch
                xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t()
                f2 = oa.oem(xd, y, **kw)
                assert oa.last_path_engine()[0] == "wres"
                assert all(np.array_equal(np.asarray(f2["beta"][k]), np.asarray(f["beta"][k])) for k in range(len(kw["penalty"])))
                monkeypatch.delenv("OEM_WRES")
                oa.oem(xd, y, **kw)
                assert oa.last_path_engine()[0] == "wcoop"
                monkeypatch.setenv("OEM_WRES", "1")
            if ci == 0 and n in (64, 500):
                monkeypatch.setenv("OEM_WCOOP_FAKE_TIMEOUT", "1")
                t = oa.oem(x, y, **kw)
                monkeypatch.delenv("OEM_WCOOP_FAKE_TIMEOUT")
                for k in range(len(kw["penalty"])):                # the launch-per-iteration engine's bits
                    assert np.array_equal(np.asarray(t["beta"][k]), np.asarray(g["beta"][k])) and np.array_equal(t["niter"][k], g["niter"][k])


@pytest.mark.gpu
def test_wide_call_with_group_and_elementwise_penalties_is_made_in_two_parts(oa, monkeypatch):
    """p >= n where the standardised X fits the chip's registers only WITH the accumulator file (path_wres_kernel: element-wise operators):
    a call that mixes group and element-wise penalties is made in two parts -- penalties are independent cold starts (ref
    src/oem_dense.cpp:206-246) -- so that one group penalty does not send the lasso to the engine that re-reads X every iteration
    (api.hip: run_paths_parts).  Same results as the one-call form (OEM_NO_PENALTY_SPLIT=1) in the caller's order, user lambdas and
    compute.loss included; against the oracle."""
    import torch
    n, p = 120, 12800                                              # 200 workgroups of path_wcoop_kernel (it takes 192): path_wres_kernel's size, 40 workgroups
    rng = np.random.default_rng(99)
    x = np.asfortranarray(rng.normal(size=(n, p)) * rng.uniform(0.5, 2.0, p))
    b = np.zeros(p); b[:8] = rng.uniform(0.5, 1.5, 8)
    y = x @ b + rng.normal(size=n)
    groups = np.arange(p) // 5 + 1
    lam = [np.array([0.6, 0.3, 0.1])] * 4
    calls = (dict(penalty=["grp.lasso", "lasso", "grp.mcp", "scad"], groups=groups, nlambda=4, lambda_min_ratio=0.05, tol=1e-8, maxit=300, compute_loss=True),
             dict(penalty=["lasso", "grp.lasso", "mcp", "ols"], groups=groups, lambda_=lam, tol=1e-8, maxit=300, standardize=False))
    xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for kw in calls:
            f = oa.oem(xd, y, **kw)
            assert oa.last_path_engine()[0] == "wlaunches"        # the second part: the group penalties
            monkeypatch.setenv("OEM_NO_PENALTY_SPLIT", "1")
            g = oa.oem(xd, y, **kw)
            monkeypatch.delenv("OEM_NO_PENALTY_SPLIT")
            r = orc.fit_dense(x, y, native=True, unique_groups=np.unique(groups), **kw)
            assert abs(f["d"] - r["d"]) < DTOL * r["d"]
            for k in range(4):
                assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-11)
                sc = max(1.0, float(np.abs(r["beta"][k]).max()))
                assert np.abs(np.asarray(f["beta"][k]) - np.asarray(g["beta"][k])).max() < 1e-9 * sc, kw["penalty"][k]
                assert np.abs(np.ravel(f["niter"][k]).astype(int) - np.ravel(g["niter"][k]).astype(int)).max() <= 1
                _agree_with_oracle(f, r, k, kw["tol"], kw["penalty"][k])
                if kw.get("compute_loss"):
                    assert np.allclose(np.ravel(f["loss"][k]), np.ravel(r["loss"][k]), rtol=1e-8)


@pytest.mark.gpu
@pytest.mark.parametrize("n,p", [(3000, 40), (2500, 300), (3000, 1100), (40, 70), (150, 400), (300, 1100)])
@pytest.mark.parametrize("std,icpt", [(False, False), (True, False), (False, True), (True, True)])
def test_observation_weights_of_the_compiled_entry(oa, n, p, std, icpt):
    """oem_fit_dense with a non-empty weights vector (ref src/oem_dense.h:368-414, 699-707, 759-770,
    src/DataStd.h:94-202): R's oem() -- and oem() here -- stop with "weights not implemented yet" (R/oem.R:244); the compiled entry
    computes sqrt(w)-weighted DataStd statistics (unweighted for x under both flags), X'WX / n, X'(Yw) / n and loss = sum w r^2.  Here
    (weighted.hip): the statistics, the standardised sqrt(w)-scaled copy, the ordinary MFMA moment pass over it, the path engines
    of every size class -- and for nobs <= nvars d from that Gram, the iteration on the Gram of the w-scaled copy (the reference squares
    the weights there, src/oem_dense.h:513-517), the loss from the first again -- against the oracle's restatement (held against numpy
    and the KKT conditions in tests/test_oracle_independent.py; no reference-held number exists), from host and from device memory."""
    import torch
    rng = np.random.default_rng(n + p + 2 * std + icpt)
    x = np.asfortranarray(rng.normal(size=(n, p)) * rng.uniform(0.5, 2.5, p) + rng.uniform(-1, 1, p))
    b = np.zeros(p); b[:6] = rng.uniform(0.5, 1.5, 6)
    y = x @ b + rng.normal(size=n) + 0.6
    w = rng.uniform(0.1, 3.0, n); w[rng.integers(n, size=5)] = 0.0           # (a few rows out)
    if n <= p:
        w = w / 3.0       # nobs <= nvars: d bounds X'WX / n but the reference iterates on X'W^2 X / n -- with weights above 1 ITS iteration
                          # diverges at the small lambdas (1e21 in the oracle, inf here); weights <= 1 keep W^2 below W
    groups = np.arange(p) // 4 + 1
    kw = dict(penalty=["lasso", "mcp", "grp.lasso", "ols"], groups=groups, nlambda=5, lambda_min_ratio=0.02, tol=1e-9, maxit=2000,
              standardize=std, intercept=icpt, compute_loss=True)
    with pytest.raises(ValueError, match="weights not implemented yet"):
        oa.oem(x, y, weights=w, penalty="lasso")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = oa.oem_fit_dense_weighted(x, y, w, **kw)
        xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t()
        fd = oa.oem_fit_dense_weighted(xd, y, w, **kw)
    r = orc.fit_dense_w(x, y, w, native=True, unique_groups=np.unique(groups), **kw)
    assert abs(f["d"] - r["d"]) < DTOL * r["d"]
    for k in range(4):
        assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-11)
        sc = max(1.0, float(np.abs(r["beta"][k]).max()))
        assert np.abs(np.asarray(f["beta"][k]) - np.asarray(r["beta"][k])).max() < 1e-8 * sc, kw["penalty"][k]
        assert np.abs(np.ravel(f["niter"][k]).astype(int) - np.ravel(r["niter"][k]).astype(int)).max() <= 1
        assert np.allclose(np.ravel(f["loss"][k]), np.ravel(r["loss"][k]), rtol=1e-8)
        assert np.abs(np.asarray(f["beta"][k]) - np.asarray(fd["beta"][k])).max() < 1e-10 * sc
    # unit weights: the unweighted fit (another route to the same moments: agreement to rounding)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        one = oa.oem_fit_dense_weighted(x, y, np.ones(n), penalty="lasso", nlambda=5, tol=1e-9, standardize=std, intercept=icpt)
        ref = oa.oem(x, y, penalty="lasso", nlambda=5, tol=1e-9, standardize=std, intercept=icpt)
    assert np.abs(np.asarray(one["beta"][0]) - np.asarray(ref["beta"][0])).max() < 1e-9 * max(1.0, float(np.abs(ref["beta"][0]).max()))
    with pytest.raises(ValueError, match="length of weights"):
        oa.oem_fit_dense_weighted(x, y, w[:-1], penalty="lasso")
    with pytest.raises(oa.OemgpuError, match="finite and >= 0"):
        oa.oem_fit_dense_weighted(x, y, -w, penalty="lasso")


@pytest.mark.gpu
@pytest.mark.parametrize("p,icpt,knob", [(300, True, None), (300, True, "OEM_NO_COOP"), (640, True, None), (1100, True, None), (1100, False, None),
                                         (1100, False, "OEM_NO_SYMCOOP"), (2300, True, None), (2300, False, None)])
def test_sparse_compute_loss_beyond_one_workgroup(oa, monkeypatch, p, icpt, knob):
    """compute.loss of oemSparse (ref src/oem_sparse.h:919-944) beyond p + intercept = 288 (refused until round 4).  Without
    an intercept the engines' own loss (the Gram identity of the dense path); with one the member is rescaled in place before the
    product that loss would come from, so it is a pass of its own behind the engine (sparse.hip: gram_loss_kernel) -- on the
    cooperating engine, the launches, and the register-resident ones.  Against the oracle's residual of the same fitted values."""
    import scipy.sparse as sp
    if knob:
        monkeypatch.setenv(knob, "1")
    rng = np.random.default_rng(p + icpt)
    n = 3 * p
    x = sp.random(n, p, density=0.03, random_state=p, format="csc", data_rvs=lambda k: rng.normal(size=k) * 1.5)
    b = np.zeros(p); b[:8] = rng.uniform(0.5, 1.5, 8)
    y = x @ b + rng.normal(size=n) * 0.3 + (1.2 if icpt else 0.0)
    groups = np.arange(p) // 5 + 1
    pens = ["lasso", "grp.lasso", "ols"]
    kw = dict(penalty=pens, groups=groups, nlambda=6, tol=1e-9, maxit=800, intercept=icpt)
    f = oa.oem(x, y, compute_loss=True, **kw)
    rg, rug = orc.r_sparse_groups(groups, icpt)
    r = orc.fit_sparse(x, y, lambda_min_ratio=1e-4, compute_loss=True, native=True, d_override=f["d"], **dict(kw, groups=rg, unique_groups=rug))
    for k in range(len(pens)):
        assert np.abs(f["beta"][k] - r["beta"][k]).max() < 1e-8 * max(1.0, float(np.abs(r["beta"][k]).max())), pens[k]
        fl, rl = np.ravel(f["loss"][k]), np.ravel(r["loss"][k])
        assert fl.shape == rl.shape and np.all(fl < 1e98) and np.allclose(fl, rl, rtol=1e-8), (pens[k], fl, rl)


@pytest.mark.gpu
def test_sparse_x_in_several_row_tiles(oa, monkeypatch):
    """the dense staging tile of the sparse Gram is capped (2 GiB); OEM_SPARSE_TILE_ROWS forces several tiles, with a ragged last one"""
    import scipy.sparse as sp
    rng = np.random.default_rng(44)
    n, p = 7001, 33
    x = sp.random(n, p, density=0.05, random_state=11, format="csc", data_rvs=lambda k: rng.normal(size=k))
    y = x[:, :4] @ np.array([1.0, -2.0, 0.5, 1.5]) + rng.normal(size=n) * 0.3 + 0.7
    kw = dict(penalty=["lasso", "mcp"], nlambda=9, tol=1e-10)
    one = oa.oem(x, y, **kw)
    monkeypatch.setenv("OEM_SPARSE_TILE_ROWS", "1024")
    many = oa.oem(x, y, **kw)
    r = orc.fit_sparse(x, y, lambda_min_ratio=1e-4, **kw)
    for k in range(2):
        assert np.abs(one["beta"][k] - many["beta"][k]).max() < 1e-12
        assert np.abs(many["beta"][k] - r["beta"][k]).max() < 1e-9
    # every entry stored twice as two halves, in random order inside its column: oem() sums them as R's dgCMatrix coercion does (no
    # two stores to one slot of a tile), and leaves the caller's matrix as it was
    xc = sp.csc_matrix(x)
    cols = np.repeat(np.arange(p), np.diff(xc.indptr))
    order = np.lexsort((rng.permutation(2 * xc.nnz), np.concatenate([cols, cols])))
    dup = sp.csc_matrix((np.concatenate([xc.data, xc.data])[order] * 0.5, np.concatenate([xc.indices, xc.indices])[order], 2 * xc.indptr),
                        shape=x.shape)
    kept = [a.copy() for a in (dup.indptr, dup.indices, dup.data)]
    summed = dup.copy(); summed.sum_duplicates()
    twice, once = oa.oem(dup, y, **kw), oa.oem(summed, y, **kw)
    for key in ("beta", "lambda", "niter", "loss"):
        assert all(np.array_equal(u, v) for u, v in zip(twice[key], once[key])), key
    assert twice["d"] == once["d"]
    assert all(np.array_equal(a, b) for a, b in zip((dup.indptr, dup.indices, dup.data), kept))


@pytest.mark.gpu
@pytest.mark.parametrize("p", [5, 65, 100, 111, 300])
def test_moments_of_a_handful_of_rows(oa, p):
    """1 .. 65 rows with garbage behind the last one (a 1-row shard of big.oem, a tiny fold): every moment kernel must stay inside
    its input.  (The LDS-DMA ring's pre-decremented 32-bit lane offsets wrapped around at ld < 8 -- found by tests/test_gpu_fuzz.py --
    so launches of fewer than 64 rows take the plain kernels.)"""
    import torch
    from oem_amd import _lib as L
    from oem_amd.distributed import HipBackend
    be = HipBackend(0)
    rng = np.random.default_rng(p)
    for n in (1, 2, 3, 7, 8, 9, 63, 64, 65):
        for pad in (0, 2):
            ld = (n + 1) // 2 * 2 + pad
            x = rng.normal(size=(n, p)); y = rng.normal(size=n)
            buf = torch.full((p, ld), 7.5, device="cuda", dtype=torch.float64)
            buf[:, :n] = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda")
            yd = torch.full((ld + 8,), -3.25, device="cuda", dtype=torch.float64); yd[:n] = torch.as_tensor(y, device="cuda")
            with be.section():
                mom = be.new_buffer(L.moments_len(p))
                be.moments(buf[:, :n].t(), n, ld, p, yd, None, mom)
            torch.cuda.synchronize()
            z = np.column_stack([x, y, np.ones(n)])
            ref = z.T @ z
            assert np.abs(mom.cpu().numpy().reshape(p + 2, p + 2) - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (n, ld)


def _hash_start(p):
    """the device Lanczos start vector (path_small.hip / path_coop.hip / path_large.hip: a fixed hash of the row index)"""
    j = np.arange(p, dtype=np.uint64)
    h = (j * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)
    return (h >> np.uint64(8)).astype(np.float64) / 16777216.0 - 0.5


def _adversarial(p, ratio, seed):
    """a symmetric positive definite matrix whose TOP eigenvector is orthogonal (to rounding) to the device's start vector"""
    rng = np.random.default_rng(seed)
    v0 = _hash_start(p); v0 /= np.linalg.norm(v0)
    e1 = rng.normal(size=p); e1 -= (e1 @ v0) * v0; e1 /= np.linalg.norm(e1)
    q_, _ = np.linalg.qr(np.column_stack([e1, rng.normal(size=(p, p - 1))]))
    q_[:, 0] = e1
    q_, _ = np.linalg.qr(q_)                                                # first column stays +-e1
    lam = np.concatenate([[ratio], np.linspace(1.0, 0.05, p - 1)])
    m = (q_ * lam) @ q_.T
    return (m + m.T) / 2, lam[0], lam[1], q_[:, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("p", [60, 100, 200, 270, 400])
def test_eigen_step_with_the_top_eigenvector_hidden_from_the_start_vector(oa, p):
    """a Krylov method started orthogonally to the top eigenvector sees it only through rounding noise, which the
    recurrence amplifies by the Chebyshev growth factor of the gap.  (Spectra's start vector is fixed too -- seed 0 -- so the
    reference shares the blind spot.)  Two regimes:
      * lambda_1 = 3 lambda_2: the noise grows ~6x per step and takes over within ~20 steps, before the stagnation test can fire
        (first possible stop: step 32): lambda_max comes out right;
      * lambda_1 = 1.1 lambda_2: the recurrence may settle on lambda_2 first.  Then d = 1.005 lambda_2 < lambda_1, but OEM is a
        proximal-gradient iteration with step 1 / d and converges for every d > lambda_1 / 2: the fit is still the optimum."""
    import ctypes as C
    import torch
    from oem_amd import _lib as L
    lib = L.lib(); ctx = oa.context()
    out = C.c_double(0.0)
    m, l1, l2, e1 = _adversarial(p, 3.0, p)
    assert abs(e1 @ _hash_start(p)) < 1e-13
    md = torch.as_tensor(m, device="cuda")
    L.check(lib.oemgpu_eig_max_dev(ctx, md.data_ptr(), p, C.byref(out)))
    assert abs(out.value - l1) < 1e-9 * l1, (out.value, l1)
    m, l1, l2, e1 = _adversarial(p, 1.1, p + 1)
    md = torch.as_tensor(m, device="cuda")
    L.check(lib.oemgpu_eig_max_dev(ctx, md.data_ptr(), p, C.byref(out)))
    assert out.value >= l2 * (1 - 1e-9) and out.value <= l1 * (1 + 1e-9)    # one of the two, never below lambda_2
    rng = np.random.default_rng(p)
    b = np.zeros(p); b[:5] = [1.0, -1.0, 0.5, 2.0, -0.7]
    xty = m @ b + 0.05 * rng.normal(size=p) + 0.3 * e1                      # the solution HAS a component along the hidden direction
    lam = np.geomspace(np.abs(xty).max() * 0.5, np.abs(xty).max() * 0.01, 5)
    f = oa.oem_xtx(torch.as_tensor(m, device="cuda"), xty, penalty=["lasso", "mcp"], lambda_=lam, tol=1e-12, maxit=100000)
    r = orc.fit_xtx(m, xty, penalty=["lasso", "mcp"], lambda_=lam, tol=1e-12, maxit=100000)
    assert abs(r["d"] - 1.005 * l1) < 1e-9 * l1                             # the oracle solves the dense eigenproblem exactly
    assert np.abs(f["beta"][0] - r["beta"][0]).max() < 1e-7                 # the convex fit: the same optimum whatever d was used
    for i in range(len(lam)):                                               # both fits: stationary points of their objective
        for k, pen in enumerate(["lasso", "mcp"]):
            bb = f["beta"][k][:, i]
            g = m @ bb - xty
            nz = bb != 0
            dp = lam[i] if pen == "lasso" else np.maximum(lam[i] - np.abs(bb[nz]) / 3.0, 0.0)
            assert np.abs(g[nz] + dp * np.sign(bb[nz])).max() < 1e-8 and (np.abs(g[~nz]) <= lam[i] * (1 + 1e-9)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("p", [40, 100, 230, 400])
def test_eigen_step_reports_its_steps_and_a_reached_cap(oa, p, monkeypatch):
    """the Lanczos recurrence has a step cap the reference's restarted Spectra call has not.  oemgpu_last_eigen_info says
    how many steps were taken and whether the cap (not the stop rule, not breakdown) ended them; a fit whose cap was reached still
    ends at the optimum (OEM is a proximal-gradient iteration that converges for every d > lambda_max / 2)."""
    import ctypes as C
    import torch
    from oem_amd import _lib as L
    lib = L.lib()
    rng = np.random.default_rng(p)
    n = 5 * p
    x = np.asfortranarray(rng.normal(size=(n, p)))
    y = x[:, :4] @ np.array([1.0, -1.0, 0.5, 2.0]) + rng.normal(size=n)
    xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t()
    steps, capped = C.c_int32(-1), C.c_int32(-1)
    kw = dict(penalty="lasso", nlambda=6, tol=1e-11, maxit=5000)
    fit = oa.oem(xd, y, **kw)
    assert lib.oemgpu_last_eigen_info(oa.context(), C.byref(steps), C.byref(capped)) == 0
    assert 8 <= steps.value <= max(2 * p, 32) and capped.value == 0, (steps.value, capped.value)
    monkeypatch.setenv("OEMGPU_LANCZOS_CAP", "8")
    short = oa.oem(xd, y, **kw)
    assert lib.oemgpu_last_eigen_info(oa.context(), C.byref(steps), C.byref(capped)) == 0
    if p <= 1024 and steps.value <= 8:                      # (the host-checked engines look every 16 steps: their cap is theirs)
        assert capped.value == 1 and short["d"] <= fit["d"] * (1 + 1e-12)
    assert np.abs(short["beta"][0] - fit["beta"][0]).max() < 1e-7
