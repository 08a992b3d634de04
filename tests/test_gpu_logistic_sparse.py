"""oemgpu_fit_logistic_sparse on the MI355X against the CPU restatement (tests/logistic_sparse_restatement.py): the man page's sparse
shape (R/oem.R:141-158) and the dense fit on the same matrix, all 14 penalties with an intercept, both X'WX routes (compressed columns,
row tiles) on one matrix, the edges of the compressed layouts, the W floor and loss clamps, q > 1024, bitwise repeatability, the
interrupt and the step counters."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import logistic_restatement as RD
from tests import logistic_sparse_restatement as RS

pytestmark = pytest.mark.gpu


def _sparse(n, p, density, seed, k=5, intercept=0.0, scale=1.0):
    rng = np.random.default_rng(seed)
    x = sp.random(n, p, density=density, format="csc", random_state=rng, data_rvs=lambda m: rng.normal(size=m) * scale)
    b = np.zeros(p)
    b[:k] = rng.uniform(-1.5, 1.5, k)
    prob = 1.0 / (1.0 + np.exp(-(x @ b + intercept)))
    y = (rng.uniform(size=n) < prob).astype(np.float64)
    return x, y


def _groups(pen, groups, intercept):
    if groups is None or not any("grp" in q for q in pen):
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


def _both(x, y, pens, intercept=True, standardize=True, groups=None, stats=None, **kw):
    import oem_amd
    g, ug = _groups(pens, groups, intercept)
    fit = oem_amd.oem_fit_logistic_sparse(x, y, penalty=pens, intercept=intercept, standardize=standardize,
                                          groups=groups if groups is not None else (), **kw)
    lam = kw.pop("lambda_", None)
    ref = RS.fit(x, y, penalty=pens, intercept=intercept, standardize=standardize, groups=g, unique_groups=ug,
                 lambda_=lam, stats=stats, **kw)
    return fit, ref


def test_man_page_sparse_shape_and_the_dense_fit():
    import oem_amd
    x, y = _sparse(20000, 50, 0.01, 1)
    groups = np.repeat(np.arange(1, 6), 10)
    kw = dict(nlambda=10, irls_tol=1e-3, tol=1e-8)
    fit, ref = _both(x, y, ["grp.lasso"], intercept=False, groups=groups, **kw)
    _compare(fit, ref, ["grp.lasso"])
    dense = oem_amd.oem_fit_logistic_dense(np.asfortranarray(x.toarray()), y, penalty="grp.lasso", intercept=False, groups=groups,
                                           hessian_type="full", **kw)
    assert np.abs(np.asarray(dense["beta"][0]) - np.asarray(fit["beta"][0])).max() < 1e-8
    assert np.array_equal(dense["niter"][0], fit["niter"][0])


def test_all_penalties_with_intercept():
    x, y = _sparse(3000, 12, 0.08, 2, intercept=0.4)
    groups = np.array([0, 1, 1, 2, 2, 2, 3, 3, 4, 4, 5, 5])            # group 0 among the user's groups
    pf = np.ones(12); pf[[1, 7]] = 0.0
    pens = RD.PENALTIES
    fit, ref = _both(x, y, pens, groups=groups, nlambda=5, penalty_factor=pf, alpha=0.6, gamma=3.7, tau=0.3, compute_loss=True,
                     irls_tol=1e-5, tol=1e-9)
    _compare(fit, ref, pens)
    lam = [np.array([0.05, 0.02, 0.008])] * 2
    fit, ref = _both(x, y, ["lasso", "scad"], lambda_=lam, compute_loss=True, tol=1e-9)
    _compare(fit, ref, ["lasso", "scad"])


@pytest.mark.parametrize("standardize", [True, False])
def test_both_routes_agree(monkeypatch, standardize):
    import oem_amd
    x, y = _sparse(9000, 30, 0.015, 3)
    icpt = standardize
    out = {}
    for route in ("csc", "dense"):
        monkeypatch.setenv("OEM_SPARSE_GRAM", route)
        monkeypatch.setenv("OEM_SPARSE_TILE_ROWS", "2048")               # five tiles, the last a partial one
        out[route] = oem_amd.oem_fit_logistic_sparse(x, y, penalty=["lasso", "mcp"], nlambda=6, intercept=icpt, standardize=standardize,
                                                     compute_loss=True, tol=1e-9)
        a = oem_amd.oem_fit_logistic_sparse(x, y, penalty=["lasso", "mcp"], nlambda=6, intercept=icpt, standardize=standardize,
                                            compute_loss=True, tol=1e-9)
        for k in range(2):                                                 # repeatable to the bit on either route
            assert np.array_equal(a["beta"][k], out[route]["beta"][k]) and np.array_equal(a["loss"][k], out[route]["loss"][k])
        assert a["d"] == out[route]["d"]
    ref = RS.fit(x, y, penalty=["lasso", "mcp"], nlambda=6, intercept=icpt, standardize=standardize, compute_loss=True, tol=1e-9)
    for route in ("csc", "dense"):
        _compare(out[route], ref, ["lasso", "mcp"])
    for k in range(2):
        assert np.abs(np.asarray(out["csc"]["beta"][k]) - np.asarray(out["dense"]["beta"][k])).max() < 1e-10
        assert np.array_equal(out["csc"]["niter"][k], out["dense"]["niter"][k])


def test_edges_of_the_compressed_layout():
    rng = np.random.default_rng(5)
    n, p = 8291, 9                                                         # n a multiple of no chunk (64, 8192, the row pass)
    xd = sp.random(n, p, density=0.05, random_state=rng, data_rvs=lambda m: rng.normal(size=m)).toarray()
    xd[:, 4] = 0.0                                                         # an empty column
    xd[:200, :] = 0.0                                                      # empty rows
    xd[:, 6] = 0.0; xd[7, 6] = 2.5                                         # a column with a single non-zero
    x = sp.csc_matrix(xd)
    x.data[::17] = 0.0                                                     # explicitly stored zeros
    assert x.nnz > np.count_nonzero(x.toarray())
    y = (rng.uniform(size=n) < 0.4).astype(np.float64)
    for icpt in (True, False):
        fit, ref = _both(x, y, ["lasso", "grp.lasso"], intercept=icpt, groups=np.array([1, 1, 2, 2, 3, 3, 4, 4, 5]), nlambda=5,
                         compute_loss=True, tol=1e-9)
        _compare(fit, ref, ["lasso", "grp.lasso"])


def test_near_separable_rows_fire_the_floor_and_the_clamps():
    import oem_amd
    xd, y = RD.near_separable(3000, 10, 7)
    xd[np.abs(xd) < 0.7] = 0.0                                             # sparse, the far rows keep their weight
    x = sp.csc_matrix(xd)
    st = {}
    fit, ref = _both(x, y, ["lasso"], nlambda=8, lambda_min_ratio=1e-3, compute_loss=True, irls_maxit=30, stats=st)
    _compare(fit, ref, ["lasso"])
    assert st["floored"] > 0 and st["clamped"] > 0, st
    gst = oem_amd.logistic_stats()
    assert gst["irls_steps"] == st["irls"] and gst["inner_iters"] == st["inner"]
    assert gst["row_passes"] == st["rows"] and gst["grams"] == st["grams"] == st["rows"]


def test_launch_form_q_over_1024():
    x, y = _sparse(6000, 1100, 0.004, 8, k=8)
    fit, ref = _both(x, y, ["lasso"], nlambda=3, lambda_min_ratio=0.3, intercept=False, tol=1e-8)
    _compare(fit, ref, ["lasso"])


def test_interrupt_returns_minus_6():
    import oem_amd
    x, y = _sparse(4000, 30, 0.05, 9)
    calls = []

    def stop():
        calls.append(1)
        return len(calls) > 3
    with pytest.raises(oem_amd.OemgpuError) as ei:
        oem_amd.oem_fit_logistic_sparse(x, y, penalty="lasso", nlambda=20, interrupt=stop)
    assert ei.value.code == -6
    fit = oem_amd.oem_fit_logistic_sparse(x, y, penalty="lasso", nlambda=5)   # the library is usable afterwards
    assert np.all(np.isfinite(fit["beta"][0]))
