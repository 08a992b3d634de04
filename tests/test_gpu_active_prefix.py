"""The ranked layout and the short round of the row-split path kernel (path_small.hip, p <= 208).

Rows and columns are taken in the order of |X'y| / penalty.factor, and while the non-zeros of beta stay within the first 32 ranked
rows a round multiplies 8 column pairs per lane instead of all.  Every case here is held
  * against the CPU oracle, with the tolerances of tests/test_gpu_parity.py::_agree_with_oracle and d to 1e-10, and
  * against itself with OEM_NO_ACTIVE_PREFIX=1 (the same layout, never the short round): the SAME BITS in beta, niter, lambda, loss
    and d -- a skipped FMA would have added a * 0.
oemgpu_last_path_rounds says how many rounds ran short (device-resident inputs: their calls run on `oa.context()`)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_gpu_parity import DTOL, _agree_with_oracle

pytestmark = pytest.mark.gpu

SWITCH = "OEM_NO_ACTIVE_PREFIX"


@pytest.fixture(scope="module")
def oa():
    import torch
    assert torch.cuda.is_available()
    import oem_amd
    oem_amd.lib()
    return oem_amd


def _same_bits(f, g, label=""):
    assert f["d"] == g["d"], (label, f["d"], g["d"])
    assert len(f["beta"]) == len(g["beta"])
    for k in range(len(f["beta"])):
        for key in ("beta", "niter", "lambda", "loss"):
            assert np.array_equal(np.asarray(f[key][k]), np.asarray(g[key][k]), equal_nan=True), (label, key, k)


def _ab(monkeypatch, run, label=""):
    """run() as shipped and with the short round switched off: the same bits; returns the shipped fit"""
    f = run()
    monkeypatch.setenv(SWITCH, "1")
    g = run()
    monkeypatch.delenv(SWITCH)
    _same_bits(f, g, label)
    return f


def _oracle_check(f, r, tol, label=""):
    assert abs(f["d"] - r["d"]) <= DTOL * abs(r["d"]), (label, f["d"], r["d"])
    for k in range(len(r["beta"])):
        assert np.allclose(f["lambda"][k], r["lambda"][k], rtol=1e-12, atol=0), (label, k)
        _agree_with_oracle(f, r, k, tol, (label, k))


def _problem(n, p, support, seed, coef=(0.5, 1.5), sd=3.0, noise=1.0):
    rng = np.random.default_rng(seed)
    x = np.asfortranarray(rng.normal(size=(n, p)) * sd)
    b = np.zeros(p)
    b[np.asarray(support)] = rng.uniform(coef[0], coef[1], len(support)) * rng.choice([-1.0, 1.0], len(support))
    y = x @ b + noise * rng.normal(size=n) + 0.3
    return x, y


def _dev(oa, x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t()          # column-major on the device


def _rounds(oa, monkeypatch, x, y, **kw):
    """(short_rounds, rounds) of a device-resident call as shipped; with the switch: no short round, as many rounds"""
    xd = _dev(oa, x)
    f = oa.oem(xd, y, **kw)
    s, t = oa.api.last_path_rounds()
    monkeypatch.setenv(SWITCH, "1")
    g = oa.oem(xd, y, **kw)
    s0, t0 = oa.api.last_path_rounds()
    monkeypatch.delenv(SWITCH)
    _same_bits(f, g)
    assert s0 == 0 and t0 == t, (s0, t0, t)
    assert t == int(np.sum(np.minimum(np.ravel(f["niter"][0]), kw.get("maxit", 500)))), (t, f["niter"][0])
    return f, s, t


# ---------------------------------------------------------------------------------------------- where the support sits
@pytest.mark.parametrize("where", ["last", "scattered", "first"])
def test_support_anywhere(oa, monkeypatch, where):
    p = 100
    support = {"last": np.arange(75, 100), "first": np.arange(25), "scattered": np.random.default_rng(3).choice(p, 25, replace=False)}[where]
    x, y = _problem(3000, p, support, 10)
    kw = dict(penalty=["lasso"], nlambda=30, lambda_min_ratio=0.05, tol=1e-10)
    f = _ab(monkeypatch, lambda: oa.oem(x, y, **kw), where)
    _oracle_check(f, orc.fit_dense(x, y, **kw), 1e-10, where)
    _, s, t = _rounds(oa, monkeypatch, x, y, **kw)
    print(f"support {where}: {s} of {t} rounds short")
    # The bound, from the design: a true variable has |x'y| / n >= 9 * 0.5 = 4.5 (minus noise), a null one sd(x) sd(y) / sqrt(n)
    # = 3 * 15 / 55 = 0.8, at most about 2.2 = 0.16 lambda_max over 75 of them: the 25 true variables take the first 25 ranks, and no
    # null variable can be active while lambda > 0.16 lambda_max, i.e. on the first 60 % of this log grid (ln 0.16 / ln 0.05).
    # Those rounds are short; half of all rounds leaves room for the later lambdas taking more rounds each.  With the columns in
    # their given order ("last", "scattered") every round with a non-zero would be a full one and the share a few per cent.
    assert s / t >= 0.5, (s, t)


def test_short_form_is_taken(oa, monkeypatch):
    """n = 2e5, p = 100, 25 coefficients U(0.5, 1.5), X ~ N(0, 9), unit noise, lambda.min.ratio 0.05, tol 1e-10: in a CPU model of the
    iteration (three seeds, 852-859 rounds) every round's support lies within ranked positions 0..27 -- below the cap of 32"""
    rng = np.random.default_rng(2024)
    n, p = 200000, 100
    x = np.asfortranarray(rng.normal(size=(n, p)) * 3.0)
    b = np.zeros(p); b[rng.choice(p, 25, replace=False)] = rng.uniform(0.5, 1.5, 25)
    y = x @ b + rng.normal(size=n)
    kw = dict(penalty=["lasso"], nlambda=100, lambda_min_ratio=0.05, tol=1e-10)
    f, s, t = _rounds(oa, monkeypatch, x, y, **kw)
    print(f"short form: {s} of {t} rounds")
    _oracle_check(f, orc.fit_dense(x, y, **kw), 1e-10)
    assert t > 0 and s / t >= 0.9, (s, t)


def test_dense_solutions(oa, monkeypatch):
    """ols and an almost-ridge elastic net: nothing is zero, the short round (almost) never applies, the results are right"""
    rng = np.random.default_rng(5)
    n, p = 3000, 100
    x = np.asfortranarray(rng.normal(size=(n, p)) * 2.0 + 0.5)
    y = x @ rng.uniform(-1.0, 1.0, p) + rng.normal(size=n)
    kw = dict(penalty=["ols", "elastic.net"], alpha=0.05, nlambda=12, tol=1e-9)
    f = _ab(monkeypatch, lambda: oa.oem(x, y, **kw))
    _oracle_check(f, orc.fit_dense(x, y, lambda_min_ratio=1e-4, **kw), 1e-9)
    _, s, t = _rounds(oa, monkeypatch, x, y, penalty=["ols"], tol=1e-9)
    print(f"ols: {s} of {t} rounds short")
    assert s <= 1                                           # (the first round multiplies the zero vector)
    # elastic.net, alpha = 0.05: the threshold is lambda as for the lasso, and with 100 true coefficients U(-1, 1) a third of the
    # |x'y| lie above 0.68 lambda_max -- the second of these 12 lambdas (0.43 lambda_max) already has more than 32 non-zeros, and
    # the path never comes back: at most the rounds of two lambdas of twelve, the cheapest two, are short
    _, s, t = _rounds(oa, monkeypatch, x, y, penalty=["elastic.net"], alpha=0.05, nlambda=12, tol=1e-9)
    print(f"elastic.net alpha 0.05: {s} of {t} rounds short")
    assert s / t <= 0.25, (s, t)


def test_support_jumps_over_the_cap_inside_a_lambda(oa, monkeypatch):
    """five lambdas over three decades, sixty true variables: the warm start of a lambda has a handful of non-zeros, its solution
    dozens -- the short round meets the first non-zero beyond its cap, completes that product itself and hands over to the full loop"""
    x, y = _problem(4000, 100, np.arange(20, 80), 17, coef=(0.2, 2.0))
    kw = dict(penalty=["lasso"], nlambda=5, lambda_min_ratio=1e-3, tol=1e-10)
    f, s, t = _rounds(oa, monkeypatch, x, y, **kw)
    print(f"jump: {s} of {t} rounds short; non-zeros per lambda {list(f['nzero'][0])}")
    assert 0 < s < t, (s, t)
    _oracle_check(f, orc.fit_dense(x, y, **kw), 1e-10)
    g = _ab(monkeypatch, lambda: oa.oem(x, y, **kw))
    _same_bits(f, g)                                        # (device-resident and host inputs: the same path kernel)


def test_ties_duplicates_and_zero_columns(oa, monkeypatch):
    rng = np.random.default_rng(23)
    n, p = 2500, 70
    x = rng.normal(size=(n, p))
    x[:, 11] = x[:, 3]; x[:, 40] = x[:, 3]; x[:, 41] = x[:, 60]            # equal keys
    x[:, 5] = 0.0; x[:, 69] = 0.0                                           # zero keys
    x = np.asfortranarray(x)
    y = x[:, [3, 20, 60, 68]] @ np.array([1.0, -2.0, 0.7, 1.5]) + rng.normal(size=n)
    for std in (True, False):
        kw = dict(penalty=["lasso", "mcp"], nlambda=15, tol=1e-9, standardize=std)
        f = _ab(monkeypatch, lambda: oa.oem(x, y, **kw), std)
        _oracle_check(f, orc.fit_dense(x, y, lambda_min_ratio=1e-4, **kw), 1e-9, std)


def test_penalty_factor_with_zeros(oa, monkeypatch):
    x, y = _problem(3000, 90, [1, 30, 31, 77, 89], 31)
    pf = np.random.default_rng(1).uniform(0.3, 3.0, 90)
    pf[[0, 44, 89]] = 0.0                                    # unpenalised: ranked first, never zero
    kw = dict(penalty=["lasso", "scad"], penalty_factor=pf, nlambda=20, tol=1e-10)
    f = _ab(monkeypatch, lambda: oa.oem(x, y, **kw))
    _oracle_check(f, orc.fit_dense(x, y, lambda_min_ratio=1e-4, **kw), 1e-10)
    assert np.all(f["beta"][0][[1, 45, 90], 1:] != 0.0)
    # penalty.factor = 0 ranks FIRST: variables 0 and 44 have no true coefficient (their |x'y| is a null variable's) and are never
    # zero.  Ranked by |x'y| alone they would land somewhere among the 85 null variables, beyond rank 32 with probability
    # 1 - (32 / 85)^2 = 0.86, and every round after the first would be a full one.  Ranked first, the support is the three of them
    # and up to five true variables while lambda > 0.16 lambda_max as above: the first 60 % of the grid.
    _, s, t = _rounds(oa, monkeypatch, x, y, penalty=["lasso"], penalty_factor=pf, nlambda=20, lambda_min_ratio=0.05, tol=1e-10)
    print(f"penalty.factor zeros: {s} of {t} rounds short")
    assert s / t >= 0.5, (s, t)


@pytest.mark.parametrize("opt", ["accelerate", "compute_loss"])
def test_accelerate_and_loss(oa, monkeypatch, opt):
    x, y = _problem(3000, 100, np.arange(40, 60), 41)
    kw = dict(penalty=["lasso", "mcp"], nlambda=25, lambda_min_ratio=0.01, tol=1e-10, **{opt: True})
    f = _ab(monkeypatch, lambda: oa.oem(x, y, **kw), opt)
    r = orc.fit_dense(x, y, **kw)
    _oracle_check(f, r, 1e-10, opt)
    if opt == "compute_loss":
        for k in range(2):
            assert np.allclose(np.ravel(f["loss"][k]), np.ravel(r["loss"][k]), rtol=1e-9)
    _, s, t = _rounds(oa, monkeypatch, x, y, **dict(kw, penalty=["lasso"]))
    print(f"{opt}: {s} of {t} rounds short")
    # twenty true variables in columns 40 .. 59, lambda down to 0.01 lambda_max: no null variable is active above 0.16 lambda_max
    # (see test_support_anywhere), 40 % of this log grid; a third of the rounds, as the later lambdas take more rounds each
    assert s / t >= 1.0 / 3.0, (s, t)


@pytest.mark.parametrize("p", [100, 200])
def test_mcp_scad(oa, monkeypatch, p):
    x, y = _problem(3000, p, np.arange(p - 12, p), 50 + p)
    kw = dict(penalty=["mcp", "scad", "mcp.net", "scad.net"], alpha=0.8, gamma=3.7, nlambda=25, lambda_min_ratio=0.01, tol=1e-10)
    f = _ab(monkeypatch, lambda: oa.oem(x, y, **kw), p)
    _oracle_check(f, orc.fit_dense(x, y, **kw), 1e-10, p)


@pytest.mark.parametrize("p", [60, 100, 150])
def test_mixed_call_shares_d_and_bits(oa, monkeypatch, p):
    """lasso, mcp, grp.lasso, ols in one call: one d, and each penalty's bits are those of the same penalty fitted alone (the
    layout is the same for every operator the kernel serves)"""
    x, y = _problem(2 * p + 2000, p, np.arange(p // 2, p // 2 + 10), 60 + p)
    groups = np.arange(p) // 5 + 1
    pens = ["lasso", "mcp", "grp.lasso", "ols"]
    kw = dict(groups=groups, nlambda=12, lambda_min_ratio=0.01, tol=1e-9)
    f = _ab(monkeypatch, lambda: oa.oem(x, y, penalty=pens, **kw), p)
    _oracle_check(f, orc.fit_dense(x, y, penalty=pens, unique_groups=np.unique(groups), **kw), 1e-9, p)
    for k, pen in enumerate(pens):
        alone = oa.oem(x, y, penalty=[pen], **kw)
        assert alone["d"] == f["d"], pen
        for key in ("beta", "niter", "lambda"):
            assert np.array_equal(np.asarray(alone[key][0]), np.asarray(f[key][k])), (pen, key)


def test_big_oem_with_intercept(oa, monkeypatch):
    x, y = _problem(5000, 99, np.arange(80, 99), 71)
    y = y + 4.0
    kw = dict(penalty=["lasso", "mcp"], nlambda=20, tol=1e-9)
    f = _ab(monkeypatch, lambda: oa.big_oem(x, y, **kw))
    _oracle_check(f, orc.fit_big(x, y, lambda_min_ratio=1e-4, **kw), 1e-9)
    assert np.all(f["beta"][0][0, :] != 0.0)               # the intercept column: unpenalised, ranked first


def test_oem_xtx_with_scale_factor(oa, monkeypatch):
    x, y = _problem(3000, 100, np.arange(70, 90), 81)
    n = x.shape[0]
    xtx, xty = x.T @ x / n, x.T @ y / n
    sf = np.random.default_rng(2).uniform(0.5, 2.0, 100)
    kw = dict(penalty=["lasso", "scad"], nlambda=15, tol=1e-9)
    f = _ab(monkeypatch, lambda: oa.oem_xtx(xtx, xty, scale_factor=sf, **kw))
    _oracle_check(f, orc.fit_xtx(xtx, xty, scale_factor=sf, lambda_min_ratio=1e-4, **kw), 1e-9)
    g = _ab(monkeypatch, lambda: oa.oem_xtx(xtx, xty, **kw))
    _oracle_check(g, orc.fit_xtx(xtx, xty, lambda_min_ratio=1e-4, **kw), 1e-9)


def test_xval_several_instances_per_launch(oa, monkeypatch):
    rng = np.random.default_rng(91)
    n, p, nf = 4000, 60, 5
    x = np.asfortranarray(rng.normal(size=(n, p)) * 2.0)
    y = x[:, 50:58] @ rng.uniform(0.5, 1.5, 8) + rng.normal(size=n) + 0.4
    foldid = rng.permutation(np.resize(np.arange(1, nf + 1), n))
    kw = dict(penalty=["lasso", "mcp"], nlambda=15, tol=1e-9)
    f = oa.xval_oem(x, y, foldid=foldid, **kw)
    monkeypatch.setenv(SWITCH, "1")
    g = oa.xval_oem(x, y, foldid=foldid, **kw)
    monkeypatch.delenv(SWITCH)
    _same_bits(f, g)
    for key in ("cvm", "cvsd"):
        for k in range(2):
            assert np.array_equal(f[key][k], g[key][k]), key
    r = orc.xval_dense(x, y, foldid, lambda_min_ratio=1e-4, **kw)
    _oracle_check(f, r, 1e-9)
    for k in range(2):
        assert np.allclose(f["cvm"][k], r["cvm"][k], rtol=1e-9) and np.allclose(f["cvsd"][k], r["cvsd"][k], rtol=1e-8)


@pytest.mark.parametrize("q", [3, 32, 33, 64, 65, 100, 104, 105, 128, 129, 176, 177, 200, 208])
def test_layout_boundaries(oa, monkeypatch, q):
    """both sides of every size at which the row-split kernel changes its configuration (waves, registers per lane, LDS columns)"""
    nnz = min(q, 12)
    x, y = _problem(2 * q + 600, q, np.arange(q - nnz, q), 100 + q, sd=1.5)
    kw = dict(penalty=["lasso", "scad"], nlambda=10, lambda_min_ratio=0.02, tol=1e-9)
    f = _ab(monkeypatch, lambda: oa.oem(x, y, **kw), q)
    _oracle_check(f, orc.fit_dense(x, y, **kw), 1e-9, q)
    n = x.shape[0]
    g = _ab(monkeypatch, lambda: oa.oem_xtx(x.T @ x / n, x.T @ y / n, penalty=["mcp"], nlambda=6), q)
    _oracle_check(g, orc.fit_xtx(x.T @ x / n, x.T @ y / n, penalty=["mcp"], nlambda=6, lambda_min_ratio=1e-4), 1e-7, q)
