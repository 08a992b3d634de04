"""Every kernel that reads a column-major x as x + j ld, with columns more than 2 and 4 GiB apart.

All cases are (p, ld) views of ONE flat float64 buffer filled with the 7.5 sentinel of test_random_moment_kernels: small n, a huge
leading dimension.  (a) holds the moment buffer of each kernel form -- asserted first through oemgpu_selftest_gram_form -- to the exact
sums of dyadic data (array_equal), on both sides of the two guards of the scalar-base forms: lane offsets in [2^31, 2^32), then the
64-bit forms behind the guards.  (b) runs the other kernels that take ld through the Python front ends against their oracles and,
bit for bit, against the same call on a compact copy."""
import ctypes as C
import functools
import time
import warnings

import numpy as np
import pytest

from oracle import oracle as orc
from tests.exact_gram import exact_gram

pytestmark = pytest.mark.gpu

TRI, RING_SADDR, RING_LANE, SB, WD3, WD4, WD_UNITS, BLK = range(8)
TWO32 = 1 << 32
LD_T = 17_895_698                 # the first even ld at which lane 15 of a shared-slab / one-read fragment passes 2^31 bytes
NS = (4099, 40002)                # one step per chunk, ragged against 8 and 64 | several slabs per chunk: the per-slab base advance runs
PMAX = 225


def ld_max(p):
    """the largest even ld with p ld 8 + 65536 < 2^32: the ring kernel's scalar-base guard"""
    m = (TWO32 - 65536 - 1) // (8 * p)
    return m - (m & 1)


def ld_far(p, odd=False):
    """the first even (odd) ld with (p - 1) ld 8 > 2^32: the last column more than 4 GiB from the first"""
    ld = (1 << 29) // (p - 1) + 1
    return ld + ((ld & 1) != (1 if odd else 0))


# (p, ld, the form it is meant to reach, strips)
RING_CASES = [(p, ld_max(p) + d, RING_LANE if d else RING_SADDR, 0 if d else s)
              for p, s in ((62, 0), (78, 0), (94, 0), (98, 1), (100, 2), (110, 0)) for d in (0, 2)]
TRI_CASES = [(p, ld_far(p, odd=True), TRI, 0) for p in (5, 40, 110)]
SB_CASES = [(p, ld, f, 0) for p in (120, 130) for ld, f in ((LD_T, SB), ((1 << 25) - 2, SB), (1 << 25, BLK))]
WD_CASES = [(161, LD_T, WD3, 0), (225, LD_T, WD4, 0)]
EXACT_CASES = RING_CASES + TRI_CASES + SB_CASES + WD_CASES
SHIFT_CASES = [(100, ld_max(100), RING_SADDR, 2), (120, LD_T, SB, 0), (161, LD_T, WD3, 0)]
# the buffer holds the largest view of any case: p = 130 at ld = 2^25, 4.36e9 elements (p = 225 at ld = 17,895,698 is 4.03e9)
BIG_ELEMS = max(p * ld for p, ld, _, _ in EXACT_CASES) + 64


@pytest.fixture(scope="module")
def big():
    import torch
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    flat = torch.full((BIG_ELEMS,), 7.5, device="cuda", dtype=torch.float64)
    yield flat
    _dyadic.cache_clear()
    peak = torch.cuda.max_memory_allocated()
    # pytest keeps the fixture's value until this finalizer has returned: the storage itself is given up here, so that empty_cache() can
    # hand the block back to the device before the next module runs
    flat.untyped_storage().resize_(0)
    del flat
    torch.cuda.empty_cache()
    assert torch.cuda.memory_reserved() < BIG_ELEMS * 8
    print(f"LARGE_LD module: {time.time() - t0:.1f} s wall, peak allocated {peak} bytes ({peak / 2 ** 30:.2f} GiB)")


@pytest.fixture(scope="module")
def be():
    from oem_amd.distributed import HipBackend
    return HipBackend(0)


class _View:
    """x (n x p, host, column j = x[:, j]) written into the first n rows of a (p, ld) view of the buffer `off` elements in; the sentinel is
    put back on exit"""

    def __init__(self, big, x_dev_t, ld, off=0):
        self.p, self.n = x_dev_t.shape
        assert off + self.p * ld <= big.numel() and ld >= self.n
        self.rows = big[off:off + self.p * ld].view(self.p, ld)[:, :self.n]
        self.src = x_dev_t
        self.ld = ld

    def __enter__(self):
        self.rows.copy_(self.src)
        v = self.rows.t()
        assert v.stride() == (1, self.ld) and v.shape == (self.n, self.p)
        return v

    def __exit__(self, *exc):
        self.rows.fill_(7.5)


def _form(n, ld, p, aligned):
    from oem_amd import _lib as L
    out = (C.c_int64 * 2)()
    L.check(L.lib().oemgpu_selftest_gram_form(n, ld, p, int(aligned), 256, out))
    return int(out[0]), int(out[1])


def _padded_y(y):
    import torch
    yflat = torch.full((len(y) + 16,), -3.25, device="cuda", dtype=torch.float64)
    yd = yflat[:len(y)]
    yd[:] = torch.as_tensor(y, device="cuda")
    return yd


def _moments(be, xv, n, ld, p, yd, shift):
    import torch
    from oem_amd import _lib as L
    with be.section():
        mom = be.new_buffer(L.moments_len(p)); sums = be.new_buffer(L.sums_len(p))
        if shift:
            be.shift_sums(xv, n, ld, p, yd, sums)
        be.moments(xv, n, ld, p, yd, sums if shift else None, mom)
    torch.cuda.synchronize()
    return mom.cpu().numpy().reshape(p + 2, p + 2), sums.cpu().numpy()


# ------------------------------------------------------------------------------------------------ (a) the moment buffer
@functools.lru_cache(maxsize=None)
def _dyadic(n, kmax, seed):
    """(k: n x (PMAX + 2) integers -- PMAX columns of x, y, the ones column as 8 --, its exact Gram in int64, x' on the device, y on the
    device): entries k / 8.  A case of p columns takes the first p columns of x."""
    import torch
    rng = np.random.default_rng(seed)
    k = rng.integers(-kmax, kmax + 1, size=(n, PMAX + 2))
    k[:, PMAX + 1] = 8
    g = exact_gram(k)
    xt = torch.as_tensor(np.ascontiguousarray(k[:, :PMAX].T / 8.0), device="cuda")
    return k, g, xt, k[:, PMAX] / 8.0


def _sub(g, p):
    idx = np.r_[0:p, PMAX, PMAX + 1]
    return g[np.ix_(idx, idx)]


def _sampled_rows(n):
    """the rows shift_sums_kernel reads: at most 256 evenly spaced chunks of 16 (all rows when n <= 4096)"""
    nch = (n + 15) // 16
    nsamp = min(nch, 256)
    rows = []
    for t in range(nsamp):
        c = (t * (nch - 1)) // (nsamp - 1) if nsamp > 1 else 0
        rows.extend(range(16 * c, min(16 * c + 16, n)))
    return np.array(rows)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("p,ld,form,strips", EXACT_CASES, ids=[f"p{c[0]}-ld{c[1]}" for c in EXACT_CASES])
def test_moments_are_the_exact_sums(big, be, p, ld, form, strips, n):
    """unshifted pass on entries k / 8, |k| <= 32: every product is a multiple of 1 / 64 and every sum far below 2^53 of them, so any
    order of summation is exact (tests/test_gram_form_cpu.py confirms the reference): the whole (p + 2)^2 buffer, both halves"""
    aligned = ld % 2 == 0
    assert _form(n, ld, p, aligned) == (form, strips)
    assert form == TRI and not aligned and (p - 1) * ld * 8 > TWO32 or form != TRI and aligned
    if form == RING_SADDR:
        assert (16 * (p // 16) - 1) * ld * 8 >= 1 << 31 and p * ld * 8 + 65536 < TWO32      # columns on both sides of 2^31, none at 2^32
    if form == RING_LANE:
        assert (p - 1) * ld * 8 >= 1 << 31 and p * ld * 8 + 65536 >= TWO32                  # one step past the scalar-base guard
    if form in (SB, WD3, WD4):
        assert 1 << 31 <= 15 * ld * 8 and 16 * ld * 8 < TWO32 < (p - 1) * ld * 8            # lane 15 past 2^31; tile bases past 4 GiB
    k, g, xt, y = _dyadic(n, 32, 11)
    yd = _padded_y(y)
    with _View(big, xt[:p], ld) as xv:
        M, _ = _moments(be, xv, n, ld, p, yd, False)
        # the sums of the rows shift_sums samples, on the same view
        import torch
        from oem_amd import _lib as L
        with be.section():
            sums = be.new_buffer(L.sums_len(p))
            be.shift_sums(xv, n, ld, p, yd, sums)
        torch.cuda.synchronize()
        sh = sums.cpu().numpy()
    ref = _sub(g, p) / 64.0
    assert np.array_equal(M, ref), (p, n, ld, int(np.argmax(np.abs(M - ref))), float(np.abs(M - ref).max()))
    rows = _sampled_rows(n)
    ks = np.c_[k[rows, :p], k[rows, PMAX]]
    assert np.array_equal(sh[:p + 1], ks.sum(axis=0) / 8.0) and sh[p + 1] == len(rows)
    assert np.array_equal(sh[p + 2:2 * p + 3], (ks * ks).sum(axis=0) / 64.0)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("p,ld,form,strips", SHIFT_CASES, ids=[f"p{c[0]}-ld{c[1]}" for c in SHIFT_CASES])
def test_shifted_moments(big, be, p, ld, form, strips, n):
    """columns 50 + k / 8, |k| <= 14 (mean 50, sd 1.0), shift_sums first: the buffer about the centre the sums define, against that sum in
    np.longdouble -- with u = x - 50 exact and d = c - 50, sum (u_i - d_i)(u_j - d_j) = U_ij - d_j S_i - d_i S_j + n d_i d_j from the exact
    integer U and S, nothing cancels -- at test_random_moment_kernels' tolerance"""
    assert _form(n, ld, p, True) == (form, strips)
    k, g, xt, y = _dyadic(n, 14, 12)
    yd = _padded_y(y + 50.0)
    with _View(big, xt[:p] + 50.0, ld) as xv:
        M, sh = _moments(be, xv, n, ld, p, yd, True)
    rows = _sampled_rows(n)
    ks = np.c_[k[rows, :p], k[rows, PMAX]]
    assert np.array_equal(sh[:p + 1], 50.0 * len(rows) + ks.sum(axis=0) / 8.0) and sh[p + 1] == len(rows)      # (exact: multiples of 1 / 8 below 2^53 / 8)
    m = sh[:p + 1] * (1.0 / sh[p + 1])                          # the kernels' centre: sums times the reciprocal of the count
    var = np.maximum(sh[p + 2:2 * p + 3] / sh[p + 1] - m * m, 0.0)
    assert np.all(m * m > 256.0 * var)                          # the shift is taken
    ld_ = np.longdouble
    G = _sub(g, p).astype(ld_) / ld_(64)                        # [u | 1]' [u | 1], exact
    U, S = G[:p + 1, :p + 1], G[:p + 1, p + 1]
    d = m.astype(ld_) - ld_(50)
    ref = np.empty((p + 2, p + 2), dtype=ld_)
    ref[:p + 1, :p + 1] = U - np.outer(S, d) - np.outer(d, S) + ld_(n) * np.outer(d, d)
    ref[:p + 1, p + 1] = ref[p + 1, :p + 1] = S - ld_(n) * d
    ref[p + 1, p + 1] = n
    err = float(np.abs(M.astype(ld_) - ref).max())
    print(f"SHIFTED p={p} n={n} ld={ld}: max error {err:.2e}, bound {1e-11 * max(1.0, float(np.abs(ref).max())):.2e}")
    assert err <= 1e-11 * max(1.0, float(np.abs(ref).max())), (p, n, ld, err)


# ------------------------------------------------------------------------------------------------ (b) the other kernels that take ld
def _gauss(n, p, seed, mean=0.0):
    rng = np.random.default_rng(seed)
    x = np.asfortranarray(rng.normal(size=(n, p)) * (1.0 + rng.uniform(size=p)) + mean)
    b = np.zeros(p); b[:4] = [1.0, -0.7, 0.5, 0.3]
    y = x @ b + rng.normal(size=n) + 0.4
    return x, y


def _dev_t(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x.T), device="cuda")


def _same_bits(a, b, keys=("beta", "lambda", "niter", "loss")):
    for key in keys:
        for u, v in zip(a[key], b[key]):
            assert np.asarray(u).tobytes() == np.asarray(v).tobytes(), key
    assert a["d"] == b["d"]


def _against(f, r, npen, label):
    assert abs(f["d"] - r["d"]) <= 1e-10 * abs(r["d"]), (label, f["d"], r["d"])
    worst = 0.0
    for k in range(npen):
        fb, rb = np.asarray(f["beta"][k]), np.asarray(r["beta"][k])
        assert fb.shape == rb.shape
        assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-10)
        worst = max(worst, float(np.abs(fb - rb).max()))
        dn = np.abs(np.ravel(f["niter"][k]).astype(int) - np.ravel(r["niter"][k]).astype(int))
        assert dn.max() <= 1, (label, k, dn)
    print(f"LARGE_LD {label}: beta gap {worst:.1e}")
    assert worst <= 1e-9, (label, worst)


def _far_view(big, xt):
    p, n = xt.shape
    ld = ld_far(p)
    assert (p - 1) * ld * 8 > TWO32
    assert _form(n, ld, p, True) == _form(n, n, p, True) and n % 2 == 0      # the premise of bit equality with the compact copy: one moment form
    return _View(big, xt, ld), ld


@pytest.mark.parametrize("mean", [0.0, 300.0], ids=["centred", "mean_far_above_sd"])
def test_oem(big, mean):
    """shift_sums and, with |mean| >> sd, the shifted redo of the moment pass"""
    import oem_amd
    n, p = 3000, 24
    x, y = _gauss(n, p, 21, mean)
    xt = _dev_t(x)
    kw = dict(penalty=["lasso", "mcp"], nlambda=8, tol=1e-9, maxit=800, compute_loss=True)
    view, ld = _far_view(big, xt)
    with view as xv:
        f = oem_amd.oem(xv, y, **kw)
    _same_bits(f, oem_amd.oem(xt.t(), y, **kw))
    _against(f, orc.fit_dense(x, y, lambda_min_ratio=1e-4, **kw), 2, f"oem mean={mean}")


@pytest.mark.parametrize("n,p", [(40, 100), (130, 200)])
def test_oem_wide(big, n, p):
    """p >= n: wide.hip's standardisation reads the view"""
    import oem_amd
    x, y = _gauss(n, p, 22, 0.3)
    xt = _dev_t(x)
    kw = dict(penalty=["lasso", "mcp"], nlambda=8, lambda_min_ratio=0.1, tol=1e-8, maxit=800)      # (test_wide_branch's tol and maxit)
    view, ld = _far_view(big, xt)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with view as xv:
            f = oem_amd.oem(xv, y, **kw)
        _same_bits(f, oem_amd.oem(xt.t(), y, **kw), keys=("beta", "lambda", "niter"))
    _against(f, orc.fit_dense(x, y, **kw), 2, f"oem wide {n}x{p}")


def test_weighted_fit_on_the_device_view(big):
    """oemgpu_fit_dense_weighted_dev: weighted.hip's statistics and scaled copy read the view"""
    import oem_amd
    n, p = 3000, 24
    x, y = _gauss(n, p, 23, 0.5)
    w = np.random.default_rng(24).uniform(0.5, 2.0, size=n)
    xt = _dev_t(x)
    kw = dict(penalty=["lasso", "scad"], nlambda=8, tol=1e-9, maxit=800)
    view, ld = _far_view(big, xt)
    with view as xv:
        f = oem_amd.oem_fit_dense_weighted(xv, y, w, **kw)
    _same_bits(f, oem_amd.oem_fit_dense_weighted(xt.t(), y, w, **kw), keys=("beta", "lambda", "niter"))
    _against(f, orc.fit_dense_w(x, y, w, lambda_min_ratio=1e-4, **kw), 2, "weighted")


@functools.lru_cache(maxsize=None)
def _binomial(n, p):
    rng = np.random.default_rng(25)
    x = np.asfortranarray(rng.normal(size=(n, p)))
    b = np.zeros(p); b[:3] = [0.8, -0.6, 0.4]
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-(x @ b + 0.2)))).astype(np.float64)
    return x, y


@pytest.mark.parametrize("hessian", ["upper.bound", "full"])
def test_logistic_fit(big, hessian):
    """logistic.hip: the row pass, Z and X'r on the view"""
    import oem_amd
    from tests import logistic_restatement as R
    n, p = 3000, 24
    x, y = _binomial(n, p)
    xt = _dev_t(x)
    kw = dict(penalty=["lasso", "mcp"], nlambda=6, lambda_min_ratio=1e-2, tol=1e-9, maxit=800, compute_loss=True)
    view, ld = _far_view(big, xt)
    with view as xv:
        f = oem_amd.oem_fit_logistic_dense(xv, y, hessian_type=hessian, **kw)
    _same_bits(f, oem_amd.oem_fit_logistic_dense(xt.t(), y, hessian_type=hessian, **kw))
    r = R.fit(x, y, hessian_full=hessian == "full", **kw)
    _against(f, r, 2, f"logistic {hessian}")


def test_logistic_cv_score(big):
    """logistic_cv.hip: the held-out rows of the view scored; the linear predictor against numpy"""
    import torch
    from oem_amd import api
    n, p, nf, ncol = 3000, 24, 3, 5
    x, y = _binomial(n, p)
    rng = np.random.default_rng(26)
    coef = rng.normal(size=(nf, ncol, p + 1)) * 0.3
    fid = (np.arange(n) % nf + 1).astype(np.int32)
    xt = _dev_t(x)
    yd, fd = torch.as_tensor(y, device="cuda"), torch.as_tensor(fid, device="cuda")
    view, ld = _far_view(big, xt)
    with view as xv:
        s, c, pm = api.logistic_cv_score(xv, yd, fd, nf, coef, predmat=True)
    s0, c0, pm0 = api.logistic_cv_score(xt.t(), yd, fd, nf, coef, predmat=True)
    assert s.tobytes() == s0.tobytes() and c.tolist() == c0.tolist() == [1000] * nf and pm.tobytes() == pm0.tobytes()
    eta = np.stack([np.c_[np.ones(n), x][i] @ coef[fid[i] - 1].T for i in range(n)])
    prob = 1.0 / (1.0 + np.exp(-eta.astype(np.longdouble)))
    assert float(np.abs(pm - prob).max()) <= 1e-12
    mse = np.stack([((y[fid == k + 1, None] - prob[fid == k + 1]) ** 2).sum(axis=0) for k in range(nf)])
    assert np.allclose(s[:, :, 4], 2.0 * mse.astype(np.float64), rtol=1e-10, atol=0)      # (both columns of the indicator matrix)


def test_xval_oem(big):
    """xval.hip: gather_rows_kernel reads the view, then the CV scoring"""
    import oem_amd
    n, p, nf = 3000, 24, 5
    x, y = _gauss(n, p, 27, 0.3)
    fid = np.random.default_rng(28).permutation(np.resize(np.arange(1, nf + 1), n))
    xt = _dev_t(x)
    kw = dict(penalty=["lasso", "mcp"], foldid=fid, nlambda=8, tol=1e-9, maxit=800)
    view, ld = _far_view(big, xt)
    with view as xv:
        f = oem_amd.xval_oem(xv, y, **kw)
    g = oem_amd.xval_oem(xt.t(), y, **kw)
    _same_bits(f, g, keys=("beta", "lambda", "niter", "cvm", "cvsd"))
    r = orc.xval_dense(x, y, fid, lambda_min_ratio=1e-4, **{k: v for k, v in kw.items() if k != "foldid"})
    _against(f, r, 2, "xval_oem")
    for k in range(2):                                            # the bounds of tests/test_gpu_xval.py: cvm 1e-9, cvsd 1e-8 relative
        gm = float(np.max(np.abs(f["cvm"][k] - r["cvm"][k]) / np.abs(r["cvm"][k])))
        gs = float(np.max(np.abs(f["cvsd"][k] - r["cvsd"][k]) / np.abs(r["cvsd"][k])))
        print(f"LARGE_LD xval_oem model {k}: cvm {gm:.1e} cvsd {gs:.1e}")
        assert gm <= 1e-9 and gs <= 1e-8, (k, gm, gs)


CV_PENS = ["lasso", "grp.lasso"]      # (not mcp: its cvm has a plateau at the minimum, ties to rounding -- tests/test_gpu_cv_gaussian.py)
CV_GROUPS = np.arange(24) // 4 + 1


@functools.lru_cache(maxsize=None)
def _cv_case():
    """(x, y, foldid, the restatement of cv.oem on oracle fits): tests/test_gpu_cv_gaussian.py's options"""
    from tests import cv_gaussian_restatement as R
    n, p, nf = 3000, 24, 5
    rng = np.random.default_rng(29)
    x = np.asfortranarray(rng.normal(size=(n, p)) * 2 + 0.3)
    y = x[:, :4] @ np.array([1.0, -1.5, 0.5, 2.0]) + rng.normal(size=n) + 0.4
    fid = rng.permutation(np.resize(np.arange(1, nf + 1), n))
    ref = R.cv_oem(x, y, fid, CV_PENS, groups=CV_GROUPS, unique_groups=np.unique(CV_GROUPS), nlambda=21, tol=1e-10, maxit=2000)
    mins = []
    for c in ref["cvm"]:                                          # no near-tie at the minimum
        srt = np.sort(c)
        assert srt[1] - srt[0] > 1e-6 * srt[0]
        mins.append(srt[0])
    assert abs(mins[0] - mins[1]) > 1e-6 * min(mins)
    return x, y, fid, ref


def test_cv_oem_keep(big):
    """Gaussian cv.oem on the resident view, keep=True: the fold-order gather, the fold fits and the scoring with fit.preval, against the
    restatement of cv.oem on the oracle's full and fold fits at the bounds of tests/test_gpu_cv_gaussian.py (cvm 1e-9, cvsd 1e-8, fit.preval
    1e-8 of its scale), and bit for bit against the compact copy"""
    import oem_amd
    import torch
    x, y, fid, ref = _cv_case()
    xt = _dev_t(x)
    yd = torch.as_tensor(y, device="cuda")
    kw = dict(penalty=CV_PENS, groups=CV_GROUPS, foldid=fid, nlambda=21, tol=1e-10, maxit=2000, keep=True)
    view, ld = _far_view(big, xt)
    with view as xv:
        f = oem_amd.cv_oem(xv, yd, **kw)
    g = oem_amd.cv_oem(xt.t(), yd, **kw)
    for k in range(2):
        for key in ("cvm", "cvsd", "lambda", "fit.preval"):
            assert np.asarray(f[key][k]).tobytes() == np.asarray(g[key][k]).tobytes(), (key, k)
        assert np.allclose(f["lambda"][k], ref["lambda"][k], rtol=1e-11)
        gm = float(np.max(np.abs(f["cvm"][k] - ref["cvm"][k]) / ref["cvm"][k]))
        gs = float(np.max(np.abs(f["cvsd"][k] - ref["cvsd"][k]) / ref["cvsd"][k]))
        print(f"LARGE_LD cv_oem {CV_PENS[k]}: cvm {gm:.1e} cvsd {gs:.1e}")
        assert gm <= 1e-9 and gs <= 1e-8, (k, gm, gs)
        pv, pr = f["fit.preval"][k], ref["predmat"][k]
        assert pv.shape == pr.shape and np.array_equal(np.isnan(pv), np.isnan(pr))
        ok = ~np.isnan(pr)
        assert np.abs(pv[ok] - pr[ok]).max() < 1e-8 * max(1.0, float(np.abs(pr[ok]).max()))
    assert f["lambda.min"] == g["lambda.min"] and f["best.model"] == g["best.model"] and f["model.min"] == g["model.min"]
    assert f["model.min"] - 1 == ref["model_min"] and f["best.model"] == CV_PENS[ref["model_min"]]
    assert np.isclose(f["lambda.min"], ref["lambda_min"], rtol=1e-11)
    assert np.array_equal(f["foldid"], fid)


def test_oem_sharded_big_one_rank(big):
    """the sharded driver (big.oem semantics) on the view as its one shard"""
    from oem_amd.distributed import oem_sharded
    n, p = 3000, 24
    x, y = _gauss(n, p, 31, 0.3)
    xt = _dev_t(x)
    import torch
    yd = torch.as_tensor(y, device="cuda")
    kw = dict(penalty=["lasso", "mcp"], nlambda=8, tol=1e-9, maxit=800)
    view, ld = _far_view(big, xt)
    with view as xv:
        f = oem_sharded(xv, yd, big=True, **kw)
    _same_bits(f, oem_sharded(xt.t(), yd, big=True, **kw), keys=("beta", "lambda", "niter"))
    _against(f, orc.fit_big(x, y, lambda_min_ratio=1e-4, **kw), 2, "oem_sharded big")
