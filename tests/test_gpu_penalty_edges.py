"""The table of tests/test_penalty_edges_cpu.py -- alpha in {0, 1}, tau in {0, 1}, gamma just above its lower limit, exact zeros among
penalty factors and group weights -- through every path engine at the smallest shape that selects it, against the oracle: coefficients to
1e-9, d to 1e-10, iteration counts within one, the engine that ran asserted after every fit, with no fall-back to another on the way
(oa.last_path_engine: device-resident inputs).  The CPU file shows for the n > p and the p >= n problems that these cases reach the
regions of the operators they are meant for, with margin (the problems of the sparse, weighted, big.oem and binomial tests below are not
censused: those entries run the path kernels already held by the censused runs, logistic.hip apart); here every copy of the operators runs
them:

  path_small.hip      p = 40, 100, 150, 200 (four waves, eight, eight with columns in LDS: chosen by size alone, launch_path_small -- the
                      row-split kernel is told from the next form by oa.api.last_path_rounds) and 230 with the cooperating engine off
                      (the four-workgroup form), through oem()
  path_coop.hip       p = 300 through oem() with ragged group runs, 640 through oem.xtx with ragged runs and with aligned runs of eight
                      (q a multiple of 8, every group eight neighbours: the condition of the eight-lane form; nothing reports which
                      form ran)
  path_symcoop.hip    p = 1030 through oem.xtx: the row-split kernel (element-wise), the symmetric kernel (OEM_NO_ROWCOOP=1: both kinds)
  path_large.hip      p = 300 (OEM_NO_COOP=1) and 1030 (OEM_NO_SYMCOOP=1 OEM_NO_ROWCOOP=1)
  p >= n              (n, p) = (40, 100) and (130, 200) under the forcing switches of test_gpu_parity.py's wide tests: path_wcoop.hip,
                      path_wres.hip, the streamed form, the launches
  sparse.hip, weighted.hip, big.oem (one block and row shards): one element-wise and one group case each
  logistic.hip        the dense, row-major and sparse binomial fits against their restatements

and on the device itself: every .net penalty at alpha = 1 gives the bits of its plain penalty fitted in the same call; sparse.grp.lasso
at tau = 1 is the lasso and at tau = 0 grp.lasso to 1e-9 of the coefficients' scale (other kernels: not the same bits); nothing is NaN or
inf.  OEM_TEST_REPORT=file appends the largest coefficient error of every fit, as test_gpu_parity.py's _report does."""
import functools
import os
import warnings

import numpy as np
import pytest

from oracle import oracle as orc
from tests import logistic_restatement as R
from tests import logistic_sparse_restatement as RS
from tests import test_penalty_edges_cpu as E
from tests.test_gpu_configs import DTOL, TIGHT, _cmp
from tests.test_gpu_logistic import _compare
from tests.test_gpu_parity import _agree_with_oracle

pytestmark = pytest.mark.gpu

PLAIN_OF = {"elastic.net": "lasso", "mcp.net": "mcp", "scad.net": "scad", "grp.lasso.net": "grp.lasso", "grp.mcp.net": "grp.mcp",
            "grp.scad.net": "grp.scad"}


@pytest.fixture(scope="module")
def oa():
    import torch
    assert torch.cuda.is_available()
    import oem_amd
    oem_amd.lib()
    return oem_amd


_DEV = {}


def _dev(key, make):
    """a device tensor kept for the module"""
    if key not in _DEV:
        _DEV[key] = make()
    return _DEV[key]


@functools.lru_cache(maxsize=None)
def _lam_max(p):
    return float(np.linalg.eigvalsh(E.problem(p)["xtx"])[-1])


def _colmajor(a):
    import torch
    return torch.as_tensor(np.array(np.asarray(a).T, order="C"), device="cuda").t()      # (a copy: the cached problems are read-only)


def _record(tag, engine, case, fit, ref):
    path = os.environ.get("OEM_TEST_REPORT")
    if not path:
        return
    with open(path, "a") as fh:
        for k, pen in enumerate(case.penalty):
            err = float(np.abs(np.asarray(fit["beta"][k]) - np.asarray(ref["beta"][k])).max())
            dn = int(np.abs(np.ravel(fit["niter"][k]).astype(int) - np.ravel(ref["niter"][k]).astype(int)).max())
            fh.write(f"edges {tag} engine={engine} case={case.name} pen={pen} err={err:.3e} dniter={dn} niter_max={int(np.max(ref['niter'][k]))}\n")


def _finite(fit, loss=False):
    for k in range(len(fit["beta"])):
        assert np.isfinite(np.asarray(fit["beta"][k])).all(), fit["penalty"][k]
        assert np.isfinite(np.asarray(fit["niter"][k], dtype=np.float64)).all() and np.all(np.asarray(fit["niter"][k]) >= 1)
        if loss:
            assert np.isfinite(np.asarray(fit["loss"][k], dtype=np.float64)).all(), fit["penalty"][k]


def _identities(case, fit):
    """what the edge parameters make of the operators, on the device's own results"""
    pens = list(case.penalty)
    beta = {q: np.asarray(fit["beta"][k]) for k, q in enumerate(pens)}
    niter = {q: np.ravel(fit["niter"][k]) for k, q in enumerate(pens)}
    if case.alpha == 1.0:
        # L = lam * 1 and D = d + 0 * lam are lam and d exactly (pen_consts), and pen_from_linear takes its cL == 1 / cD == 0 shortcuts:
        # the same operator on the same numbers, in the same call on the same engine -- the same bits
        for net, plain in PLAIN_OF.items():
            if net in beta and plain in beta:
                assert np.array_equal(beta[net], beta[plain]) and np.array_equal(niter[net], niter[plain]), net
    for other, tau in (("lasso", 1.0), ("grp.lasso", 0.0)):
        if case.tau == tau and "sparse.grp.lasso" in beta and other in beta:
            scale = max(1.0, float(np.abs(beta[other]).max()))
            assert np.abs(beta["sparse.grp.lasso"] - beta[other]).max() <= 1e-9 * scale, (other, tau)


def _niter_within_one(fit, ref):
    for k in range(len(ref["beta"])):
        dn = np.abs(np.ravel(fit["niter"][k]).astype(int) - np.ravel(ref["niter"][k]).astype(int))
        assert dn.max() <= 1, (fit["penalty"][k], dn)


def _run_params(runs):
    return [pytest.param(run, name, lay, id=f"{run.id}-{name}" + ("" if lay == "ragged" else "-" + lay)) for run in runs for name, lay in run.cases()]


@pytest.mark.parametrize("run,name,lay", _run_params(E.RUNS))
def test_gram_engines_at_the_edges(oa, run, name, lay, monkeypatch):
    """n > p: every engine that iterates on the Gram matrix"""
    case = E.CASE_BY_NAME[name].subset(run.which)
    pr = E.problem(run.p)
    kw, _ = E.call_kwargs(case, run.p, lay)
    for e in run.env:
        monkeypatch.setenv(e, "1")
    fallbacks = oa.last_path_engine()[1]                 # (persistent launches so far that timed out and were made again with launches)
    if run.entry == "oem":
        xd = _dev(("x", run.p), lambda: _colmajor(pr["x"]))
        fit = oa.oem(xd, pr["y"].copy(), **kw)
        assert oa.last_path_engine() == (run.engine, fallbacks)
        if run.engine == "rows":                         # the row-split kernel counts its rounds; the four-workgroup form leaves 0
            assert (oa.api.last_path_rounds()[1] > 0) == (run.p <= 208)
        ref = E.oracle_dense(name, run.p, lay, run.which)
    else:
        kw.pop("compute_loss", None)
        xd = _dev(("xtx", run.p), lambda: _colmajor(pr["xtx"]))
        fit = oa.oem_xtx(xd, pr["xty"].copy(), **kw)
        assert oa.last_path_engine() == (run.engine, fallbacks)
        assert abs(fit["d"] - 1.005 * _lam_max(run.p)) <= DTOL * _lam_max(run.p)
        ref = E.oracle_xtx(name, run.p, lay, run.which, d=fit["d"])
    loss = run.entry == "oem" and case.compute_loss
    _finite(fit, loss)
    _record(run.id, run.engine, case, fit, ref)
    _cmp(fit, ref, TIGHT)
    _niter_within_one(fit, ref)
    if loss:
        for k in range(len(case.penalty)):
            assert np.allclose(np.ravel(fit["loss"][k]), np.ravel(ref["loss"][k]), rtol=1e-9), case.penalty[k]
    _identities(case, fit)


@pytest.mark.parametrize("run,name,lay", _run_params(E.WIDE_RUNS + E.WIDE_ELEM_RUNS))
def test_wide_engines_at_the_edges(oa, run, name, lay, monkeypatch):
    """p >= n: the engines that iterate on the standardised X itself, against the oracle's restatement of that branch"""
    case = E.CASE_BY_NAME[name].subset(run.which)
    pr = E.problem(run.p, run.n)
    kw, _ = E.call_kwargs(case, run.p, lay, n=run.n)
    for e in run.env:
        monkeypatch.setenv(e, "1")
    fallbacks = oa.last_path_engine()[1]
    xd = _dev(("x", run.p, run.n), lambda: _colmajor(pr["x"]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fit = oa.oem(xd, pr["y"].copy(), **kw)
    engine = run.engine_for(case)
    assert oa.last_path_engine() == (engine, fallbacks)
    ref = E.oracle_wide(name, run.n, run.p, run.which)
    _finite(fit, case.compute_loss)
    _record(run.id, engine, case, fit, ref)
    assert abs(fit["d"] - ref["d"]) <= DTOL * ref["d"]
    for k, pen in enumerate(case.penalty):
        assert np.allclose(fit["lambda"][k], ref["lambda"][k], rtol=1e-12)
        _agree_with_oracle(fit, ref, k, kw["tol"], pen)
        if case.compute_loss:
            assert np.allclose(np.ravel(fit["loss"][k]), np.ravel(ref["loss"][k]), rtol=1e-8), pen
    _identities(case, fit)


# ------------------------------------------------------------------------------------------ the other entries: one case of each kind
OTHER_CASES = ["scad-gamma-2.5", "net-alpha-0", "tau-1", "zeros-group"]


def _other_data(n, p, seed, sparse=False):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, p)) * rng.uniform(0.5, 2.0, p)
    if sparse:
        x[rng.random((n, p)) < 0.9] = 0.0
    else:
        x += rng.uniform(-0.5, 0.5, p)
    b = np.zeros(p); b[rng.choice(p, 8, replace=False)] = rng.choice([-1.0, 1.0], 8) * np.geomspace(0.1, 1.5, 8)
    y = x @ b + rng.normal(size=n) + 0.7
    return np.asfortranarray(x), y


def _other_kwargs(case, p, lmax):
    kw, extra = E.options(case, p)
    kw.update(tol=E.TOL, maxit=E.MAXIT, lambda_=np.geomspace(0.9, 0.05, 6) * lmax)
    return kw, extra


def _check_other(tag, case, fit, ref):
    _finite(fit, case.compute_loss)
    _record(tag, tag, case, fit, ref)
    assert all(r.max() <= E.MAXIT // 2 for r in ref["niter"])               # the oracle alone reaches no cap
    assert abs(fit["d"] - ref["d"]) <= DTOL * abs(ref["d"])
    for k, pen in enumerate(case.penalty):
        scale = max(1.0, float(np.abs(ref["beta"][k]).max()))
        assert np.abs(np.asarray(fit["beta"][k]) - np.asarray(ref["beta"][k])).max() <= TIGHT * scale, pen
        assert np.allclose(fit["lambda"][k], ref["lambda"][k], rtol=1e-12, atol=0)
        if case.compute_loss:
            assert np.allclose(np.ravel(fit["loss"][k]), np.ravel(ref["loss"][k]), rtol=1e-8), pen
    _niter_within_one(fit, ref)
    _identities(case, fit)


@pytest.mark.parametrize("name", OTHER_CASES)
def test_sparse_x_at_the_edges(oa, name):
    """oem() on a compressed-column x (sparse.hip; the shape of test_sparse_x)"""
    import scipy.sparse as sp
    case = E.CASE_BY_NAME[name]
    n, p = 6000, 57
    xdense, y = _other_data(n, p, 41, sparse=True)
    x = sp.csc_matrix(xdense)
    lmax = orc.fit_sparse(x, y, penalty="lasso", nlambda=2)["lambda"][0][0]
    kw, _ = _other_kwargs(case, p, lmax)
    fit = oa.oem(x, y, **kw)
    okw = dict(kw)
    if case.has_groups:
        okw["groups"], okw["unique_groups"] = orc.r_sparse_groups(kw["groups"], True)
    _check_other("sparse", case, fit, orc.fit_sparse(x, y, native=True, **okw))


@pytest.mark.parametrize("name", OTHER_CASES)
def test_observation_weights_at_the_edges(oa, name):
    """the compiled entry's observation weights (weighted.hip; the smallest shape of test_observation_weights_of_the_compiled_entry)"""
    case = E.CASE_BY_NAME[name]
    n, p = 3000, 40
    x, y = _other_data(n, p, 43)
    w = np.random.default_rng(44).uniform(0.1, 3.0, n)
    lmax = orc.fit_dense_w(x, y, w, penalty="lasso", nlambda=2)["lambda"][0][0]
    kw, extra = _other_kwargs(case, p, lmax)
    fit = oa.oem_fit_dense_weighted(_colmajor(x), y, w, **kw)
    _check_other("weighted", case, fit, orc.fit_dense_w(x, y, w, native=True, **kw, **extra))


@pytest.mark.parametrize("name", OTHER_CASES)
def test_big_oem_at_the_edges(oa, name):
    """big.oem (the intercept a coordinate of its own, the unpenalised group 0 prepended for it): one block, and three row shards of
    which one is empty"""
    case = E.CASE_BY_NAME[name]
    n, p = 3000, 60
    x, y = _other_data(n, p, 45)
    lmax = orc.fit_big(x, y, penalty="lasso", nlambda=2)["lambda"][0][0]
    kw, _ = _other_kwargs(case, p, lmax)
    kw.pop("compute_loss", None)
    okw = dict(kw)
    if case.has_groups:
        okw["groups"], okw["unique_groups"] = orc.r_sparse_groups(kw["groups"], True)
    ref = orc.fit_big(x, y, native=True, **okw)
    fit = oa.big_oem(x, y, **kw)
    case = E.Case(**{**case.__dict__, "compute_loss": False})
    _check_other("big", case, fit, ref)
    cuts = [0, n // 3, n // 3, n]
    shards = oa.big_oem([x[cuts[i]:cuts[i + 1]] for i in range(3)], [y[cuts[i]:cuts[i + 1]] for i in range(3)], **kw)
    _check_other("big-shards", case, shards, ref)


# --------------------------------------------------------------------------------------------------------------------------- binomial
BINOMIAL_CASES = [c.name for c in E.CASES if not c.name.startswith("zeros")]


def _binomial_problem(sparse):
    key = ("binomial", sparse)
    if key not in _DEV:
        rng = np.random.default_rng(7 + sparse)
        n, p = 3000, 24
        x = rng.normal(size=(n, p)) * rng.uniform(0.5, 2.0, size=p)
        if sparse:
            x[rng.random((n, p)) < 0.8] = 0.0
        else:
            x += rng.normal(size=p) * 0.2
        b = np.zeros(p); b[rng.choice(p, 6, replace=False)] = rng.choice([-1.0, 1.0], 6) * np.geomspace(0.2, 1.5, 6)
        y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-(x @ b + 0.3)))).astype(np.float64)
        x = np.asfortranarray(x)
        fit = RS.fit if sparse else R.fit
        lmax = float(fit(x, y, penalty=["lasso"], nlambda=1)["lambda"][0][0])
        _DEV[key] = (x, y, lmax)
    return _DEV[key]


_BINOMIAL_REFS = {}


@pytest.mark.parametrize("form", ["dense", "rowmajor", "sparse"])
@pytest.mark.parametrize("name", BINOMIAL_CASES)
def test_binomial_fits_at_the_edges(oa, name, form):
    """logistic.hip's copy of the operators inside the IRLS loop: the dense fit, the fit on a row-major device tensor and the sparse fit,
    each against its restatement with the tolerances of test_gpu_logistic_bounds.py (coefficients 1e-8, the same IRLS counts, loss
    1e-10, d 1e-10)"""
    import scipy.sparse as sp
    import torch
    from oem_amd import api
    case = E.CASE_BY_NAME[name]
    x, y, lmax = _binomial_problem(form == "sparse")
    p = x.shape[1]
    pens = list(case.penalty)
    kw, _ = E.options(case, p)
    lam = np.geomspace(0.9, 0.05, 6) * lmax
    kw.update(tol=1e-9, maxit=500, irls_tol=1e-5, compute_loss=True, lambda_=[lam] * len(pens))
    key = (name, form == "sparse")
    if key not in _BINOMIAL_REFS:
        rkw = {k: v for k, v in kw.items() if k not in ("groups", "group_weights")}
        g, ug, gw = api._group_setup(pens, kw.get("groups", ()), kw.get("group_weights"), p, True)
        if g.size:
            rkw.update(groups=g, unique_groups=ug, group_weights=gw if gw.size else None)
        _BINOMIAL_REFS[key] = (RS.fit if form == "sparse" else R.fit)(x, y, **rkw)
    ref = _BINOMIAL_REFS[key]
    assert all(np.max(r) <= 100 for r in ref["niter"])                           # the restatement alone reaches no IRLS cap
    if form == "dense":
        fit = oa.oem_fit_logistic_dense(x, y, **kw)
    elif form == "rowmajor":
        xr = torch.as_tensor(np.ascontiguousarray(x), device="cuda")
        assert api._logistic_rowmajor_in_place(xr) is not None
        fit = oa.oem_fit_logistic_dense(xr, y, **kw)
    else:
        fit = oa.oem_fit_logistic_sparse(sp.csc_matrix(x), y, **kw)
    _finite(fit, True)
    _record("binomial-" + form, "logistic", case, fit, ref)
    _compare(fit, ref, pens, beta_tol=1e-8)
    _identities(case, fit)
