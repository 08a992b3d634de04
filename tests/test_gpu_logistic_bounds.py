"""oemgpu_fit_logistic_dense on the MI355X against the CPU restatement (tests/logistic_restatement.py) at the plan's boundaries: more
than one 64-row sub-block per row-pass chunk and a short last chunk, two Z row blocks, the Gram engines fed Z, both sides of the
A-in-LDS, staged-row-pass and one-workgroup limits, the launch form under every operator kind, the maxit / irls_maxit caps, the _dev
entry with ld > n, the smallest n, the host-side option tables, the W floor and loss clamps, and one group per coordinate at p >= 6826.

Each hand-placed case first asks oemgpu_selftest_logistic_plan (with the live CU count) whether its shape lands where it is meant
to, then compares beta / lambda / niter / loss / d with the restatement (_compare of test_gpu_logistic) and the library's step
counts (logistic_stats) with the restatement's.  test_random_logistic is a seeded sweep across the same limits; it scales with
OEM_FUZZ_SCALE like test_gpu_fuzz."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import logistic_restatement as R
from tests.test_gpu_fuzz import _check
from tests.test_gpu_logistic import _compare, _data

pytestmark = pytest.mark.gpu

SCALE = int(os.environ.get("OEM_FUZZ_SCALE", "1"))
LDS_BYTES = 160 << 10          # LDS of a gfx950 CU


@pytest.fixture(scope="module")
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(n, p, intercept, full, num_cu):
    import oem_amd
    out = (C.c_int64 * 8)()
    assert oem_amd.lib().oemgpu_selftest_logistic_plan(n, p, int(intercept), int(full), num_cu, out) == 0
    ch, nchunk, rbz, nzblk, inner_wg, staged, _, _ = list(out)
    return dict(ch=ch, nchunk=nchunk, rbz=rbz, nzblk=nzblk, inner_wg=inner_wg, staged=staged, tail=n - (nchunk - 1) * ch)


def _pick_n(n256, p, intercept, full, num_cu, want):
    """n256 on a 256-CU part; elsewhere the first n from n256 scaled by the CU count whose plan satisfies `want`"""
    n0 = n256 if num_cu == 256 else max(p + 2, n256 * num_cu // 256)
    for n in range(n0, n0 + 200000):
        P = _plan(n, p, intercept, full, num_cu)
        if want(P):
            return n, P
    raise AssertionError("no n reaches the plan asked for")


def _groups(pens, groups, group_weights, p, intercept):
    """what the C entry receives (api._group_setup), for the restatement"""
    from oem_amd import api
    g, ug, gw = api._group_setup(pens, groups, group_weights, p, intercept)
    if g.size == 0:
        return dict()
    return dict(groups=g, unique_groups=ug, group_weights=gw if gw.size else None)


def _run(x, y, pens, groups=(), group_weights=None, intercept=True, full=False, beta_rel=False, exact_niter=True, **kw):
    """fit on the GPU and with the restatement; compare results and step counts; return (fit, ref, restatement stats)"""
    import oem_amd
    pens = list(pens)
    fit = oem_amd.oem_fit_logistic_dense(x, y, penalty=pens, groups=groups, group_weights=group_weights, intercept=intercept,
                                         hessian_type="full" if full else "upper.bound", **kw)
    gst = oem_amd.logistic_stats()
    xh = x.cpu().numpy() if hasattr(x, "cpu") else x
    p = xh.shape[1]
    if "lambda_" in kw:
        kw["lambda_"] = [np.asarray(v, dtype=np.float64) for v in kw["lambda_"]]
    st = {}
    ref = R.fit(xh, y, penalty=pens, intercept=intercept, hessian_full=full, stats=st, **_groups(pens, groups, group_weights, p, intercept),
                **kw)
    if exact_niter:
        tol = 1e-8 * max(1.0, max(float(np.abs(b).max()) for b in ref["beta"])) if beta_rel else 1e-8
        _compare(fit, ref, pens, beta_tol=tol)
        assert gst["irls_steps"] == st["irls"], (gst, st)
        assert gst["row_passes"] == st["rows"], (gst, st)
        assert gst["grams"] == st["grams"], (gst, st)
        assert abs(gst["inner_iters"] - st["inner"]) <= 0.005 * st["inner"], (gst, st)
    else:
        _check(fit, ref, pens)
    return fit, ref, st


# ------------------------------------------------------------------------------------------------------------- row pass chunks
def test_multi_sub_block_and_one_row_last_chunk(num_cu):
    n, P = _pick_n(65537, 50, True, False, num_cu, lambda P: P["ch"] >= 128 and P["tail"] == 1)
    assert P["ch"] > 64 and P["tail"] == 1 and P["staged"] == 1 and P["inner_wg"] == 1 and P["nzblk"] == 1, P
    x, y = _data(n, 50, 11)                          # q = 51 <= 110: A in LDS; one-wave Gram
    _run(x, y, R.PENALTIES, groups=np.repeat(np.arange(1, 11), 5), nlambda=8, compute_loss=True, alpha=0.6, gamma=3.7, tau=0.4,
         tol=1e-9, irls_tol=1e-5)


@pytest.mark.parametrize("full", [False, True])
def test_big_n_five_sub_blocks(num_cu, full):
    # the 1e6-row shapes of DESIGN 3.9 need ~2.5 GB of restatement temporaries; 3e5 rows give five sub-blocks per chunk
    n, P = _pick_n(300000, 100, True, full, num_cu, lambda P: P["ch"] >= 320)
    assert P["ch"] >= 5 * 64 and P["staged"] == 1 and P["inner_wg"] == 1, P
    x, y = _data(n, 100, 12)                         # q = 101: A in LDS, one-wave Gram
    _run(x, y, ["lasso", "grp.lasso"], groups=np.repeat(np.arange(1, 21), 5), full=full, nlambda=10, compute_loss=True)


# ------------------------------------------------------------------------------------------------------------- Z row blocks
def test_two_z_blocks_wd4_gram(num_cu):
    n, P = _pick_n(140000, 255, False, True, num_cu, lambda P: P["nzblk"] == 2 and P["tail"] < P["ch"] // 2)
    assert P["nzblk"] == 2 and P["staged"] == 0 and P["inner_wg"] == 1 and P["tail"] < P["ch"], P
    if num_cu == 256:
        assert P["ch"] == 192 and P["tail"] == 32, P
    x, y = _data(n, 255, 13)                         # q = 255: A in global memory; Gram engine with wd = 4 (q 225-256)
    _run(x, y, ["mcp", "grp.scad"], groups=np.repeat(np.arange(1, 52), 5), intercept=False, full=True, nlambda=4,
         lambda_min_ratio=0.05, compute_loss=True)


def test_two_z_blocks_shared_slab_gram(num_cu):
    n, P = _pick_n(170000, 200, True, True, num_cu, lambda P: P["nzblk"] == 2 and P["tail"] < P["ch"])
    assert P["nzblk"] == 2 and P["staged"] == 0 and P["inner_wg"] == 1, P
    if num_cu == 256:
        assert P["ch"] == 192 and P["tail"] == 80, P
    x, y = _data(n, 200, 14)                         # q = 201: A in global memory; shared-slab Gram
    _run(x, y, ["lasso", "sparse.grp.lasso"], groups=np.repeat(np.arange(1, 41), 5), full=True, nlambda=4, lambda_min_ratio=0.05,
         compute_loss=True)


# ------------------------------------------------------------------------------------------------------------- q and p limits
@pytest.mark.parametrize("p", [109, 110])
def test_a_in_lds_limit(num_cu, p):
    # q = 110: A in LDS and the one-wave Gram; q = 111: A in global memory (logit_inner_kernel<false>) and the next Gram engine
    n = 4000
    P = _plan(n, p, True, True, num_cu)
    assert P["staged"] == 1 and P["inner_wg"] == 1, P
    x, y = _data(n, p, 15 + p)
    _run(x, y, ["lasso", "grp.mcp"], groups=np.arange(p) // 5 + 1, full=True, nlambda=6, lambda_min_ratio=0.02, compute_loss=True)


@pytest.mark.parametrize("p", [192, 193])
def test_staged_limit(num_cu, p):
    n = 8000
    P = _plan(n, p, True, True, num_cu)
    assert P["staged"] == (1 if p == 192 else 0) and P["inner_wg"] == 1, P
    x, y = _data(n, p, 17 + p)                      # q = 193 / 194: A in global memory; q = 193 on the shared-slab Gram
    _run(x, y, ["scad", "grp.lasso"], groups=np.arange(p) // 4 + 1, full=True, nlambda=5, lambda_min_ratio=0.02, compute_loss=True)


@pytest.mark.parametrize("p", [160, 511])
def test_wd3_and_multi_unit_gram(num_cu, p):
    # q = 161: Gram engine with wd = 3 (q 161-192); q = 512: the multi-unit Gram engine (q 481-512)
    n = 6000
    P = _plan(n, p, True, True, num_cu)
    assert P["staged"] == (1 if p <= 192 else 0) and P["inner_wg"] == 1, P
    x, y = _data(n, p, 19 + p)
    _run(x, y, ["grp.lasso.net", "grp.scad"], groups=np.arange(p) // 7 + 1, full=True, nlambda=4, lambda_min_ratio=0.05, alpha=0.7,
         compute_loss=True)


@pytest.mark.parametrize("p", [1023, 1024])
def test_one_workgroup_limit(num_cu, p):
    full = p == 1023
    n, P = _pick_n(35000, p, True, full, num_cu, lambda P: P["nzblk"] == 2)
    assert P["inner_wg"] == (1 if p == 1023 else 0) and P["staged"] == 0 and P["nzblk"] == 2, P
    x, y = _data(n, p, 21)                           # q = 1024: the multi-unit Gram (q 993-1024), last one-workgroup size
    _run(x, y, ["lasso"], full=full, nlambda=3, lambda_min_ratio=0.1, compute_loss=True)


def test_launch_form_every_operator(num_cu):
    p, n = 1100, 3000
    P = _plan(n, p, True, False, num_cu)
    assert P["inner_wg"] == 0 and P["staged"] == 0, P
    rng = np.random.default_rng(22)
    sizes = rng.integers(1, 20, size=p)              # groups of 1 to 19, the first one the unpenalised group 0
    groups = np.repeat(np.arange(len(sizes)), sizes)[:p]
    x, y = _data(n, p, 22)
    _run(x, y, ["grp.mcp", "grp.scad.net", "sparse.grp.lasso", "mcp", "scad"], groups=groups, nlambda=4, lambda_min_ratio=0.1,
         alpha=0.7, gamma=3.5, tau=0.3, compute_loss=True)


# ------------------------------------------------------------------------------------------------------------- caps
@pytest.mark.parametrize("p", [40, 1030])
def test_maxit_cap(num_cu, p):
    n = 3000
    assert _plan(n, p, True, False, num_cu)["inner_wg"] == (1 if p < 1024 else 0)
    x, y = _data(n, p, 23)
    _, ref, st = _run(x, y, ["lasso", "grp.lasso"], groups=np.arange(p) // 5 + 1, nlambda=4, lambda_min_ratio=0.05, maxit=3,
                      compute_loss=True)
    assert st["inner"] == 3 * st["irls"]                 # every inner solve stopped at the cap


@pytest.mark.parametrize("full", [False, True])
def test_irls_maxit_cap(num_cu, full):
    x, y = _data(3000, 30, 24)
    _, ref, st = _run(x, y, ["lasso", "mcp"], full=full, nlambda=5, irls_maxit=2, irls_tol=0.0, compute_loss=True)
    for k in range(2):
        assert np.all(np.asarray(ref["niter"][k]) == 3)  # irls_maxit + 1


# ------------------------------------------------------------------------------------------------------------- entries and edges
@pytest.mark.parametrize("full", [False, True])
def test_dev_entry_ld_above_n(num_cu, full):
    import torch
    n, p = 5000, 30
    x, y = _data(n, p, 25)
    buf = torch.full((p, n + 37), float("nan"), dtype=torch.float64, device="cuda:0")
    xd = buf.t()[:n]                                 # column-major, ld = n + 37; rows n .. n + 36 are NaN
    xd.copy_(torch.as_tensor(x))
    assert xd.stride() == (1, n + 37)
    fit, ref, _ = _run(xd, y, ["lasso", "grp.lasso"], groups=np.arange(p) // 3 + 1, full=full, nlambda=8, compute_loss=True)
    assert all(np.all(np.isfinite(b)) for b in fit["beta"])


@pytest.mark.parametrize("n,p", [(22, 20), (65, 10)])
def test_tiny_n(num_cu, n, p):
    P = _plan(n, p, True, True, num_cu)
    if n == 65:
        assert P["nchunk"] == 2 and P["tail"] == 1, P     # two chunks, the second one row
    else:
        assert P["nchunk"] == 1, P                         # n = q + 1: one chunk
    x, y = _data(n, p, 26, k=2)
    for full in (False, True):
        _run(x, y, ["lasso", "grp.lasso"], groups=np.arange(p) // 2 + 1, full=full, nlambda=5, lambda_min_ratio=0.2, compute_loss=True,
             beta_rel=True)


def test_options_on_the_device(num_cu):
    """standardize = False, zero penalty factors, a user lambda list, group weights, an all-zero column (colsq 0 -> 1), no intercept
    with the full Hessian"""
    n, p = 4000, 24
    x, y = _data(n, p, 27)
    x[:, 7] = 0.0
    pf = np.ones(p)
    pf[[0, 5]] = 0.0
    groups = np.arange(p) // 4 + 1
    gw = np.linspace(0.5, 2.0, 6)
    pens = ["lasso", "grp.lasso", "mcp.net"]
    lam = [np.geomspace(0.05, 0.002, 6) for _ in pens]
    for intercept, full, std in ((True, False, False), (False, True, False), (True, True, True), (False, False, True)):
        fit, _, _ = _run(x, y, pens, groups=groups, group_weights=gw, intercept=intercept, full=full, standardize=std, penalty_factor=pf,
                         lambda_=lam, alpha=0.8, compute_loss=True)
        assert np.all(fit["beta"][0][8, :] == 0.0)      # the all-zero column


def test_unique_groups_not_covering_every_coordinate(num_cu):
    """through the C ABI: coordinates whose group id is not among unique_groups keep beta = 0"""
    import oem_amd
    from oem_amd import api
    n, p = 3000, 20
    x, y = _data(n, p, 28)
    pens = ["grp.lasso", "grp.mcp"]
    groups = np.concatenate([[0], np.arange(p) // 4 + 1]).astype(np.int32)
    ug = np.array([0, 1, 2, 4], np.int32)              # groups 3 and 5 (coordinates 9-12, 17-20) left out
    a = api._Args(pens, [], 6, 1e-3, 1.0, 3.0, 0.5, 1e-8, 500, False, True, np.ones(p), groups, ug, np.zeros(0))
    xh = np.asfortranarray(x)
    rc = oem_amd.lib().oemgpu_fit_logistic_dense(api._dptr(xh), n, p, api._dptr(y), 1, 1, 0, 100, 1e-3, C.byref(a.c), *a.outputs(p + 1))
    assert rc == 0, oem_amd.lib().oemgpu_last_error()
    fit = api._decorate(a, pens, [f"V{i + 1}" for i in range(p)], True, n, p, family="binomial")
    gst = oem_amd.logistic_stats()
    st = {}
    ref = R.fit(x, y, penalty=pens, groups=groups, unique_groups=ug, nlambda=6, lambda_min_ratio=1e-3, tol=1e-8, compute_loss=True,
                stats=st)
    _compare(fit, ref, pens)
    assert (gst["irls_steps"], gst["row_passes"], gst["grams"]) == (st["irls"], st["rows"], st["grams"])
    for k in range(2):
        assert np.all(fit["beta"][k][[9, 10, 11, 12, 17, 18, 19, 20], :] == 0.0)
        assert np.any(fit["beta"][k][1:9, :] != 0.0)


@pytest.mark.parametrize("full", [False, True])
def test_w_floor_and_loss_clamps(num_cu, full):
    x, y = R.near_separable(6000, 20, 29)
    _, _, st = _run(x, y, ["lasso", "mcp", "grp.lasso"], groups=np.arange(20) // 4 + 1, full=full, nlambda=8, lambda_min_ratio=1e-3,
                    compute_loss=True, beta_rel=True)
    assert st["floored"] > 0 and st["clamped"] > 0, st


def test_singleton_groups_beyond_lds(num_cu):
    """one group per coordinate at p = 6830: the threshold's 8 (2 q + ngroups) bytes of scratch exceed the LDS of a CU, so the
    launch form keeps it in the workspace"""
    n, p = 7100, 6830
    q = p + 1
    assert 8 * (2 * q + q) > LDS_BYTES
    P = _plan(n, p, True, False, num_cu)
    assert P["inner_wg"] == 0 and P["staged"] == 0, P
    x, y = _data(n, p, 30)
    _run(x, y, ["grp.lasso"], groups=np.arange(1, p + 1), nlambda=2, irls_maxit=2, maxit=30, compute_loss=True)


# ------------------------------------------------------------------------------------------------------------- seeded sweep
P_CHOICES = [20, 109, 110, 111, 159, 160, 161, 191, 192, 193, 223, 224, 225, 255, 256, 257, 511, 512, 513, 1022, 1023, 1024, 1025]


@pytest.mark.parametrize("seed", list(range(24)) + list(range(1000, 1000 + 24 * (SCALE - 1))))
def test_random_logistic(num_cu, seed):
    rng = np.random.default_rng(5000 + seed)
    p = int(rng.choice(P_CHOICES))
    intercept = bool(rng.random() < 0.7)
    q = p + intercept
    if p <= 256 and rng.random() < 0.15:
        n = 65536 + int(rng.integers(1, 4 * num_cu * 64))   # past the one-sub-block chunks
    else:
        n = q + 1 + int(rng.integers(0, 3 * q + 400))
    full = bool(rng.random() < (0.5 if q <= 512 else 0.25))
    x, y = _data(n, p, 6000 + seed, k=int(rng.integers(1, 6)), intercept=float(rng.uniform(-1, 1)))
    pool = [pn for pn in R.PENALTIES if pn != "ols" or n > 5 * q]
    pens = list(rng.choice(pool, int(rng.integers(1, 4)), replace=False))
    gsz = int(rng.integers(1, 7))
    groups = np.arange(p) // gsz + (0 if rng.random() < 0.25 else 1)
    pf = np.where(rng.random(p) < 0.1, 0.0, rng.uniform(0.5, 2.0, p))
    kw = dict(nlambda=int(rng.integers(1, 6)), lambda_min_ratio=float(rng.uniform(0.02, 0.3) if n < 4 * q else rng.uniform(1e-3, 0.1)),
              alpha=float(rng.uniform(0.3, 1.0)), gamma=float(rng.uniform(2.5, 5.0)), tau=float(rng.uniform(0.1, 0.9)),
              tol=float(10.0 ** rng.uniform(-9, -6)), penalty_factor=pf, compute_loss=True)
    _run(x, y, pens, groups=groups if any("grp" in pn for pn in pens) else (), intercept=intercept, full=full,
         standardize=bool(rng.random() < 0.8), exact_niter=False, **kw)
