"""cv_oem_logistic_multi on the device: per response against tests/cv_logistic_restatement.cv fed the call's OWN fits
(oem_fit_logistic_dense_multi_folds), which isolates the cv layer -- tests/test_gpu_cv_logistic.py's code path, held to its CV_TOL --
and against cv_oem(family="binomial") on the same column, whose fits agree to 1e-8 in beta.

Against cv_oem, cvm and fit.preval: 2 (1 + max_i ||x_i||_1) 1e-8.  Every error term (deviance, (y - p)^2 twice, |y - p| twice, and the
probability itself) is at most 2-Lipschitz in eta where the deviance is not clamped, eta is linear in beta with |d eta| <=
(1 + ||x_i||_1) max |d beta|, and the interpolation onto the full fit's lambdas is a convex combination of two columns of beta.
Preconditions (tests/test_gpu_cv_logistic.py's) are asserted on the reference side only and exclude no case."""
import numpy as np
import pytest

from tests import cv_logistic_restatement as CV
from tests.logistic_multi_restatement import data
from tests.test_gpu_cv_logistic import CV_TOL, _rel
from tests.test_gpu_logistic_multi import _colmajor, _dev

pytestmark = pytest.mark.gpu

KW = dict(nlambda=20)
MEASURES = ["deviance", "class", "mse", "mae", "auc"]


@pytest.fixture(scope="module")
def oa():
    import oem_amd
    oem_amd.lib()
    return oem_amd


@pytest.fixture(scope="module")
def E(oa):
    """the data(1500, 12, 3) case with 5 random folds, and the one fold-fit call every case shares.  The seed: data()'s response 0 has the
    weakest signal, and on most seeds its fits keep every coefficient at zero over the first lambdas -- the held-out probabilities of a
    fold are then one value, which the "auc" precondition rules out (ties are a draw in the reference).  233 is the first seed of
    71 .. 299 on which, for every response and fold, max |s o X'(y - mean y)| / n of the kept rows exceeds the full fit's lambda_0
    by a tenth: the first lambda already has a non-zero coefficient, and the restatement on its own fits meets every precondition."""
    x, Y = data(1500, 12, 3, 233)
    fid = np.random.default_rng(72).permutation(np.resize(np.arange(1, 6), 1500))
    xd, Yd = _colmajor(x), _dev(Y)
    fits = oa.oem_fit_logistic_dense_multi_folds(xd, Yd, fid, penalty="lasso", **KW)
    return dict(x=x, Y=Y, fid=fid, xd=xd, Yd=Yd, fits=fits, single={})


def _gap(cvm, measure):
    crit = np.sort(-cvm if measure == "auc" else cvm)
    if measure == "class":
        crit = np.unique(crit)
    assert (crit[1] - crit[0]) > 1e-5 * abs(crit[0]), crit[:3]


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("measure", MEASURES)
def test_against_the_restatement_on_the_calls_own_fits(oa, E, measure, grouped):
    res = oa.cv_oem_logistic_multi(E["xd"], E["Yd"], penalty="lasso", type_measure=measure, grouped=grouped, foldid=E["fid"], keep=True, **KW)
    assert len(res) == 3
    for r, got in enumerate(res):
        mine = E["fits"][r]
        ref = CV.cv(E["x"], E["Y"][:, r], E["fid"], penalty=["lasso"], type_measure=measure, grouped=grouped, fitted=(mine[0], mine[1:]), **KW)
        _gap(ref["cvm"][0], measure)
        if measure == "auc":
            pv = ref["fit.preval"][0]
            for i in range(1, 6):
                for j in range(pv.shape[1]):
                    col = pv[E["fid"] == i, j]
                    assert np.isnan(col).all() or len(np.unique(col)) == len(col)
        assert got["route"] == "multi_folds" and got["name"] == ref["name"] and got["penalty"] == ["lasso"] and got["best.model"] == "lasso"
        assert isinstance(got["oem.fit"], oa.OemFitBinomial)
        lam_g, lam_r = np.asarray(got["lambda"][0]), np.asarray(ref["lambda"][0])
        assert lam_g.shape == lam_r.shape                                                # the same number of surviving lambdas
        assert np.array_equal(lam_g, np.asarray(mine[0]["lambda"][0])[:len(lam_g)])       # the full fit's own sequence
        np.testing.assert_allclose(lam_g, lam_r, rtol=1e-12)
        assert np.array_equal(got["nzero"][0], ref["nzero"][0])
        d = {k: _rel(got[k][0], ref[k][0]) for k in ("cvm", "cvsd", "cvup", "cvlo", "fit.preval")}
        print("cv_oem_logistic_multi", r, measure, "grouped" if grouped else "rows", "differences / (1 + |value|):", d)
        assert max(d.values()) <= CV_TOL, d
        assert np.array_equal(got["foldid"], E["fid"])
        for key in ("lambda.min", "lambda.1se"):
            assert got[key] == lam_g[int(np.nonzero(lam_r == ref[key])[0][0])], key
        assert got["model.min"] == ref["model.min"]


@pytest.mark.parametrize("measure", ["deviance", "mse", "mae"])
def test_against_cv_oem(oa, E, measure):
    res = oa.cv_oem_logistic_multi(E["xd"], E["Yd"], penalty="lasso", type_measure=measure, foldid=E["fid"], keep=True, **KW)
    tol = 2.0 * (1.0 + float(np.abs(E["x"]).sum(axis=1).max())) * 1e-8
    for r, got in enumerate(res):
        one = oa.cv_oem(E["xd"], E["Y"][:, r], family="binomial", penalty="lasso", type_measure=measure, foldid=E["fid"], keep=True, **KW)
        _gap(np.asarray(one["cvm"][0]), measure)
        assert set(one.keys()) | {"route"} == set(got.keys())
        lam_g, lam_o = np.asarray(got["lambda"][0]), np.asarray(one["lambda"][0])
        assert lam_g.shape == lam_o.shape
        np.testing.assert_allclose(lam_g, lam_o, rtol=1e-12)
        for key in ("cvm", "fit.preval"):
            a, b = np.asarray(got[key][0]), np.asarray(one[key][0])
            assert np.array_equal(np.isnan(a), np.isnan(b))
            err = float(np.nanmax(np.abs(a - b)))
            print("against cv_oem", r, measure, key, err, "of", tol)
            assert err <= tol, (key, err, tol)
        assert int(np.nonzero(lam_g == got["lambda.min"])[0][0]) == int(np.nonzero(lam_o == one["lambda.min"])[0][0])


def test_layouts_consumers_and_a_drawn_foldid(oa, E):
    import torch
    x32 = E["x"].astype(np.float32).astype(np.float64)
    kw = dict(penalty=["lasso", "mcp"], nlambda=8, foldid=E["fid"])
    a = oa.cv_oem_logistic_multi(_colmajor(x32), E["Yd"], **kw)
    for xd, Yd in ((_dev(x32), E["Y"]), (_dev(x32, torch.float32), _colmajor(E["Y"]))):
        b = oa.cv_oem_logistic_multi(xd, Yd, **kw)
        for r in range(3):
            for mdl in range(2):
                assert np.array_equal(a[r]["cvm"][mdl], b[r]["cvm"][mdl]) and np.array_equal(a[r]["cvsd"][mdl], b[r]["cvsd"][mdl]), (r, mdl)
            assert a[r]["lambda.min"] == b[r]["lambda.min"]
    one = a[1]
    assert one["name"] == "Binomial Deviance" and "fit.preval" not in one
    prob = oa.predict_cv(one, E["x"][:50], type="response")
    assert prob.shape == (50, 1) and np.all((prob > 0) & (prob < 1))
    s = oa.summary_cv(one)
    assert s["model"] == "logistic" and s["n"] == 1500 and "logistic regression" in oa.format_summary(s)
    drawn = oa.plot_cv(one, which_model=1, show=False)
    assert drawn["main"] == "mcp" and np.array_equal(drawn["cvm"], one["cvm"][1])
    # a drawn foldid: once, shared by all responses, the rng's
    res = oa.cv_oem_logistic_multi(E["xd"], E["Yd"], penalty="lasso", nlambda=5, nfolds=4, keep=True, rng=np.random.default_rng(9))
    want = np.random.default_rng(9).permutation(np.resize(np.arange(1, 5), 1500))
    assert np.array_equal(res[0]["foldid"], want) and np.array_equal(res[0]["foldid"], res[1]["foldid"]) and np.array_equal(res[1]["foldid"], res[2]["foldid"])


def test_small_fold_warnings(oa):
    x, Y = data(60, 4, 2, 73, k=2)
    xd, Yd = _colmajor(x), _dev(Y)
    with pytest.warns(UserWarning, match="Too few"):
        r = oa.cv_oem_logistic_multi(xd, Yd, penalty="lasso", nlambda=5, type_measure="auc", foldid=np.resize(np.arange(1, 8), 60))
    assert r[0]["name"] == "Binomial Deviance" and r[1]["name"] == "Binomial Deviance"
    with pytest.warns(UserWarning, match="grouped=FALSE enforced"):
        oa.cv_oem_logistic_multi(xd, Yd, penalty="lasso", nlambda=5, lambda_min_ratio=0.1, foldid=np.resize(np.arange(1, 25), 60))
