"""oemgpu_fit_logistic_dense on the MI355X against the CPU restatement (tests/logistic_restatement.py): the man page's and the
vignette's shapes (R/oem.R:125-158, vignettes/oem_vignette.R:55-70), all 14 penalties, the launch-per-iteration inner form (q > 1024),
bitwise repeatability, the _dev entry, and the interrupt."""
import ctypes as C

import numpy as np
import pytest

from tests import logistic_restatement as R

pytestmark = pytest.mark.gpu


def _data(n, p, seed, k=5, intercept=0.3):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, p)) * rng.uniform(0.5, 2.0, size=p) + rng.normal(size=p) * 0.2
    b = np.zeros(p)
    b[:k] = rng.uniform(-1.0, 1.0, k)
    prob = 1.0 / (1.0 + np.exp(-(x @ b + intercept)))
    y = (rng.uniform(size=n) < prob).astype(np.float64)
    return np.asfortranarray(x), y


def _groups(pen, groups, intercept):
    if not any("grp" in q for q in pen):
        return None, None
    g = np.concatenate([[0], groups]) if intercept else np.asarray(groups)
    return g, np.unique(g)


def _compare(fit, ref, pens, beta_tol=1e-8):
    for k, name in enumerate(pens):
        gb, rb = np.asarray(fit["beta"][k]), np.asarray(ref["beta"][k])
        assert gb.shape == rb.shape, name
        err = np.abs(gb - rb).max()
        assert err < beta_tol, (name, err)
        np.testing.assert_allclose(fit["lambda"][k], ref["lambda"][k], rtol=1e-12, err_msg=name)
        assert np.array_equal(np.atleast_1d(fit["niter"][k]), np.atleast_1d(ref["niter"][k])), (name, fit["niter"][k], ref["niter"][k])
        np.testing.assert_allclose(fit["loss"][k], ref["loss"][k], rtol=1e-10, err_msg=name)
    assert abs(fit["d"] - ref["d"]) <= 1e-10 * ref["d"], (fit["d"], ref["d"])


def test_man_page_shape():
    import oem_amd
    x, y = _data(5000, 50, 1, intercept=0.0)
    pens = ["lasso", "sparse.grp.lasso", "mcp"]
    groups = np.repeat(np.arange(1, 11), 5)
    kw = dict(nlambda=10, irls_tol=1e-3, tol=1e-8, compute_loss=True)
    fit = oem_amd.oem_fit_logistic_dense(x, y, penalty=pens, groups=groups, intercept=False, **kw)
    g, ug = _groups(pens, groups, False)
    ref = R.fit(x, y, penalty=pens, groups=g, unique_groups=ug, intercept=False, **kw)
    _compare(fit, ref, pens)
    assert fit["family"] == "binomial"


@pytest.mark.parametrize("hessian", ["upper.bound", "full"])
def test_vignette_shape(hessian):
    import oem_amd
    x, y = _data(50000, 100, 2)
    pens = ["lasso", "mcp", "scad", "elastic.net", "grp.lasso"]
    groups = np.repeat(np.arange(1, 21), 5)
    kw = dict(nlambda=100, compute_loss=True)
    fit = oem_amd.oem_fit_logistic_dense(x, y, penalty=pens, groups=groups, hessian_type=hessian, **kw)
    g, ug = _groups(pens, groups, True)
    ref = R.fit(x, y, penalty=pens, groups=g, unique_groups=ug, hessian_full=hessian == "full", **kw)
    _compare(fit, ref, pens)


def test_all_penalties_small():
    import oem_amd
    x, y = _data(3000, 24, 3)
    pens = list(R.PENALTIES)
    groups = np.repeat(np.arange(1, 7), 4)
    kw = dict(nlambda=12, compute_loss=True, alpha=0.6, gamma=3.7, tau=0.4, tol=1e-9, irls_tol=1e-5)
    fit = oem_amd.oem_fit_logistic_dense(x, y, penalty=pens, groups=groups, **kw)
    g, ug = _groups(pens, groups, True)
    ref = R.fit(x, y, penalty=pens, groups=g, unique_groups=ug, **kw)
    _compare(fit, ref, pens)


def test_launch_form_q_above_1024():
    import oem_amd
    x, y = _data(6000, 1500, 4)
    kw = dict(nlambda=10, compute_loss=True, lambda_min_ratio=0.05)
    fit = oem_amd.oem_fit_logistic_dense(x, y, penalty="lasso", **kw)
    ref = R.fit(x, y, penalty=["lasso"], **kw)
    _compare(fit, ref, ["lasso"])


def test_repeatable_and_dev_equals_host():
    import torch

    import oem_amd
    x, y = _data(20000, 60, 5)
    pens = ["lasso", "grp.mcp"]
    groups = np.repeat(np.arange(1, 13), 5)
    kw = dict(penalty=pens, groups=groups, nlambda=20, compute_loss=True, hessian_type="full")
    a = oem_amd.oem_fit_logistic_dense(x, y, **kw)
    b = oem_amd.oem_fit_logistic_dense(x, y, **kw)
    xd = torch.as_tensor(x, device="cuda:0")
    c = oem_amd.oem_fit_logistic_dense(xd, torch.as_tensor(y, device="cuda:0"), **kw)
    for other in (b, c):
        for k in range(len(pens)):
            assert np.array_equal(a["beta"][k], other["beta"][k])
            assert np.array_equal(a["loss"][k], other["loss"][k])
            assert np.array_equal(a["niter"][k], other["niter"][k])
        assert a["d"] == other["d"]


def test_interrupt_returns_minus_6():
    import oem_amd
    x, y = _data(4000, 30, 6)
    calls = []

    def stop():
        calls.append(1)
        return len(calls) > 3
    with pytest.raises(oem_amd.OemgpuError) as ei:
        oem_amd.oem_fit_logistic_dense(x, y, penalty="lasso", nlambda=20, interrupt=stop)
    assert ei.value.code == -6
    fit = oem_amd.oem_fit_logistic_dense(x, y, penalty="lasso", nlambda=5)      # the library is usable afterwards
    assert np.all(np.isfinite(fit["beta"][0]))
