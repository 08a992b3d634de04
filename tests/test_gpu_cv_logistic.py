"""cv.oem for binomial fits on the MI355X: the fold entry (oemgpu_fit_logistic_dense_fold_dev) against the CPU restatement of the dense
fit on the gathered rows x[keep], y[keep]; the scoring entry (oemgpu_logistic_cv_score_dev) against numpy on the same coefficient
table; and cv_oem(family="binomial") end to end against tests/cv_logistic_restatement.py.

Tolerances of the fold entry are those of the dense fit (tests/test_gpu_logistic._compare): beta 1e-8, lambda 1e-12, loss and d 1e-10,
identical niter.  The scoring sums: deviance / mse / mae rtol 1e-10, class sums and counts exact, predmat 1e-12.  End to end, cvm / cvsd /
fit.preval: CV_TOL (1 + |value|), CV_TOL = 100 x the largest difference of the first green run, capped at 1e-6.

Preconditions are asserted on the restatement, never on the library, and exclude no case:
  * scoring: min |prob - 0.5| > 1e-7 (the class rule is a comparison with 0.5);
  * end to end: the two smallest cvm differ by more than 1e-5 relative (lambda.min is an argmin).  For "class" the cvm are ratios of exact
    counts and tie exactly (the two smallest ARE equal on case A): there the two smallest DISTINCT values must differ by that much,
    and lambda.min / lambda.1se are still compared for equality;
  * "auc": no two held-out rows of a fold share a probability in any column (ties are a draw in the reference).
`lambda`: lambda_0 = max |s o X'y| / n is a floating-point sum, which the device and numpy take in different orders, so the values are
held to the restatement's at the dense fit's own 1e-12 (test_gpu_logistic._compare); exact are the number of lambdas that survive the
trimming, their equality with the full fit's own sequence, nzero, and WHICH element of the sequence lambda.min / lambda.1se are.

tests/test_gpu_cv_logistic_bounds.py takes the same helpers to the limits of both entries: scoring workgroups of more than one tile,
ld > n, saturated probabilities, both sides of the table-in-LDS limit, the waves' column groups, an empty fold, the kept-row map
beyond its first tile, poisoned left-out rows and the refusal at equality.
"""
import numpy as np
import pytest

from tests import cv_logistic_restatement as CV
from tests import logistic_restatement as R
from tests.test_gpu_logistic import _compare, _data

pytestmark = pytest.mark.gpu

CV_TOL = 7.2e-14         # x (1 + |value|): the first green run's largest difference was 7.2e-16 (fit.preval; cvm / cvsd 2.1e-16)


def _dev(x, y, fid, pad=0):
    """x, y, foldid on the device; pad > 0: x is a view of a taller column-major buffer (ld = n + pad) whose rows n .. n + pad - 1 are NaN"""
    import torch
    if pad:
        n, p = x.shape
        buf = torch.full((p, n + pad), float("nan"), dtype=torch.float64, device="cuda:0")
        xd = buf.t()[:n]
        xd.copy_(torch.as_tensor(np.ascontiguousarray(x)))
        assert xd.stride() == (1, n + pad)
    else:
        xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda:0").t()
    return xd, torch.as_tensor(np.asarray(y, dtype=np.float64), device="cuda:0"), torch.as_tensor(np.ascontiguousarray(fid, dtype=np.int32), device="cuda:0")


def _fold_fit(xd, y, yd, fd, nfolds, leave_out, pens, **kw):
    import oem_amd
    return oem_amd.oem_fit_logistic_dense(xd, y, penalty=pens, _fold=(fd, nfolds, leave_out, yd), **kw)


def _case_a():
    x, y = _data(1500, 12, 11)
    return x, y, np.random.default_rng(5).permutation(np.resize(np.arange(1, 6), 1500))


def _case_b():
    x, y = R.near_separable(1200, 8, 3)
    fid = np.resize(np.arange(1, 5), 1200)
    fid[:3] = 1; fid[3:10] = 2; fid[256:448] = 3
    return x, y, fid


def _same(a, b, pens):
    for k in range(len(pens)):
        for key in ("beta", "lambda", "niter", "loss"):
            assert np.array_equal(np.asarray(a[key][k]), np.asarray(b[key][k])), (key, pens[k])
    assert a["d"] == b["d"]


def _check_folds(x, y, fid, pens, rkw=None, pad=0, fits=None, **kw):
    """every fold of the fold entry against the restatement on the gathered rows; returns the restatement's step counts per fold.
    pad: _dev's; fits: a list that receives the fold fits"""
    xd, yd, fd = _dev(x, y, fid, pad)
    nfolds = int(fid.max())
    stats = []
    for i in range(1, nfolds + 1):
        fit = _fold_fit(xd, y, yd, fd, nfolds, i, pens, **kw)
        keep = fid != i
        st = {}
        ref = R.fit(x[keep], y[keep], penalty=pens, stats=st, **(rkw if rkw is not None else kw))
        _compare(fit, ref, pens)
        assert fit["nobs"] == int(keep.sum())
        stats.append(st)
        if fits is not None:
            fits.append(fit)
    return stats


# ------------------------------------------------------------------------------------------------------------- the fold entry
def test_fold_entry_case_a_random_folds():
    x, y, fid = _case_a()
    _check_folds(x, y, fid, ["lasso", "mcp"], nlambda=20, compute_loss=True)


def test_fold_entry_case_b_whole_sub_blocks_and_the_w_floor():
    """rows 256 .. 447 (three whole 64-row sub-blocks) leave together in fold 3; folds 1 and 2 take rows 0 .. 9, where the W floor fires:
    the floored element is the i-th KEPT row, which is not row i"""
    x, y, fid = _case_b()
    stats = _check_folds(x, y, fid, ["lasso"], nlambda=25, irls_maxit=30, compute_loss=True)
    assert [s["floored"] for s in stats] == [85, 40, 87, 121], stats
    assert sum(s["clamped"] > 0 for s in stats) == 3, stats


@pytest.mark.parametrize("hessian", ["upper.bound", "full"])
def test_fold_entry_case_c_unstaged_pass(hessian):
    x, y = _data(1500, 200, 31)
    fid = np.random.default_rng(6).permutation(np.resize(np.arange(1, 4), 1500))
    fid[640:768] = 2                                                  # two whole sub-blocks of the unstaged pass as well
    kw = dict(nlambda=6, lambda_min_ratio=0.05, compute_loss=True)
    _check_folds(x, y, fid, ["lasso", "grp.lasso"], groups=np.repeat(np.arange(1, 41), 5), hessian_type=hessian,
                 rkw=dict(groups=np.concatenate([[0], np.repeat(np.arange(1, 41), 5)]), unique_groups=np.arange(0, 41),
                          hessian_full=hessian == "full", **kw), **kw)


def test_fold_entry_case_d_two_z_blocks_one_left_out_whole():
    """the shape of test_gpu_logistic_bounds.test_two_z_blocks_shared_slab_gram; the second Z block belongs to fold 2 entirely, so that
    the moment pass is fed a block of zeros, and fold 2 also takes a random third of the first block"""
    import torch
    from tests.test_gpu_logistic_bounds import _pick_n
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n, P = _pick_n(170000, 200, True, True, num_cu, lambda P: P["nzblk"] == 2 and P["tail"] < P["ch"])
    assert P["nzblk"] == 2 and P["staged"] == 0, P
    x, y = _data(n, 200, 14)
    fid = np.random.default_rng(7).permutation(np.resize(np.arange(1, 4), n))
    fid[P["rbz"]:] = 2
    xd, yd, fd = _dev(x, y, fid)
    kw = dict(nlambda=4, lambda_min_ratio=0.05, compute_loss=True)
    fit = _fold_fit(xd, y, yd, fd, 3, 2, ["lasso"], **kw)
    keep = fid != 2
    _compare(fit, R.fit(x[keep], y[keep], penalty=["lasso"], **kw), ["lasso"])


@pytest.mark.parametrize("p,hessian", [(12, "upper.bound"), (200, "full")])
def test_leave_out_zero_is_the_dev_entry_bit_for_bit(p, hessian):
    import oem_amd
    x, y = _data(1500, p, 11)
    fid = np.random.default_rng(5).permutation(np.resize(np.arange(1, 6), 1500))
    xd, yd, fd = _dev(x, y, fid)
    pens = ["lasso", "mcp"]
    kw = dict(nlambda=10, lambda_min_ratio=0.01, compute_loss=True, hessian_type=hessian)
    _same(_fold_fit(xd, y, yd, fd, 5, 0, pens, **kw), oem_amd.oem_fit_logistic_dense(xd, y, penalty=pens, **kw), pens)


def test_fold_entry_is_repeatable():
    x, y, fid = _case_b()
    xd, yd, fd = _dev(x, y, fid)
    kw = dict(nlambda=25, irls_maxit=30, compute_loss=True, hessian_type="full")
    _same(_fold_fit(xd, y, yd, fd, 4, 3, ["lasso", "scad"], **kw), _fold_fit(xd, y, yd, fd, 4, 3, ["lasso", "scad"], **kw), ["lasso", "scad"])


def test_fold_entry_refusals_from_the_device():
    import oem_amd
    x, y = _data(40, 20, 32, k=2)
    fid = np.resize(np.arange(1, 4), 40)
    fid[:20] = 1                                                       # 14 rows stay outside fold 1: p + intercept = 21 >= 14
    xd, yd, fd = _dev(x, y, fid)
    with pytest.raises(oem_amd.OemgpuError, match="fold 1") as e:
        _fold_fit(xd, y, yd, fd, 3, 1, ["lasso"], nlambda=4)
    assert e.value.code == -4
    x, y, fid = _case_a()
    for bad in (0, 6):
        f2 = fid.copy()
        f2[777] = bad
        xd, yd, fd = _dev(x, y, f2)
        with pytest.raises(oem_amd.OemgpuError, match="fold ids") as e:
            _fold_fit(xd, y, yd, fd, 5, 1, ["lasso"], nlambda=4)
        assert e.value.code == -1


# ------------------------------------------------------------------------------------------------------------- the scoring entry
def _numpy_scores(x, y, fid, coef, over="warn"):
    """sums (nfolds x ncol x 8), counts, predmat (n x ncol) of a coefficient table nfolds x ncol x (p + 1), term by term as R forms them.
    over: numpy's errstate for an exp that overflows (a probability of exactly 0)"""
    nfolds, ncol = coef.shape[:2]
    n = x.shape[0]
    ymat = np.column_stack([(y == y.min()).astype(np.float64), (y == y.max()).astype(np.float64)])
    pred = np.full((n, ncol), np.nan)
    sums = np.zeros((nfolds, ncol, 8))
    counts = np.zeros(nfolds, dtype=np.int64)
    x1 = np.column_stack([np.ones(n), x])
    for f in range(nfolds):
        rows = fid == f + 1
        counts[f] = rows.sum()
        with np.errstate(over=over):
            pred[rows] = 1.0 / (1.0 + np.exp(-(x1[rows] @ coef[f].T)))
        for t, name in enumerate(("deviance", "class", "mse", "mae")):
            raw = CV.raw_errors(ymat[rows], pred[rows], name)
            sums[f, :, 2 * t] = raw.sum(axis=0)
            sums[f, :, 2 * t + 1] = (raw ** 2).sum(axis=0)
    return sums, counts, pred


def _check_scores(x, y, fid, coef, pad=0, over="warn"):
    """the scoring entry against numpy, twice for the same bits, and without predmat; pad: _dev's; over: _numpy_scores'.  Returns what the
    entry gave and what numpy gave: (sums, counts, predmat), (sums, counts, predmat)"""
    from oem_amd import api
    xd, yd, fd = _dev(x, y, fid, pad)
    nfolds = coef.shape[0]
    ref_sums, ref_counts, ref_pred = _numpy_scores(x, y, fid, coef, over)
    gap = np.abs(ref_pred - 0.5).min()
    print("min |prob - 0.5| =", gap)
    assert gap > 1e-7
    sums, counts, pred = api.logistic_cv_score(xd, yd, fd, nfolds, coef, predmat=True)
    print("predmat max diff", np.abs(pred - ref_pred).max(), "sums max rel diff", np.max(np.abs(sums - ref_sums) / np.maximum(np.abs(ref_sums), 1e-300)))
    assert np.array_equal(counts, ref_counts)
    assert np.array_equal(sums[:, :, 2:4], ref_sums[:, :, 2:4])                        # class: counts of 0 / 1
    for t in (0, 4, 6):
        np.testing.assert_allclose(sums[:, :, t:t + 2], ref_sums[:, :, t:t + 2], rtol=1e-10)
    assert np.abs(pred - ref_pred).max() <= 1e-12
    sums2, counts2, pred2 = api.logistic_cv_score(xd, yd, fd, nfolds, coef, predmat=True)
    assert sums.tobytes() == sums2.tobytes() and counts.tobytes() == counts2.tobytes() and pred.tobytes() == pred2.tobytes()
    sums3, counts3, none = api.logistic_cv_score(xd, yd, fd, nfolds, coef)              # without predmat: the same sums
    assert none is None and sums.tobytes() == sums3.tobytes() and counts.tobytes() == counts3.tobytes()
    return (sums, counts, pred), (ref_sums, ref_counts, ref_pred)


def _interpolated_table(x, y, fid, fitted=None, **kw):
    """the table cv.oem scores with: the restatement's fold fits interpolated onto its full fit's lambdas (fitted: CV.fits of the same
    arguments, where a test has them already)"""
    fit0, outlist = fitted if fitted is not None else CV.fits(x, y, fid, penalty=["lasso"], **kw)
    lam = np.asarray(fit0["lambda"][0])
    s = lam[lam >= max(np.min(o["lambda"][0]) for o in outlist)]
    coef = np.empty((len(outlist), len(s), x.shape[1] + 1))
    for i, o in enumerate(outlist):
        left, right, frac = CV.lambda_interp(o["lambda"][0], s)
        b = np.asarray(o["beta"][0])
        coef[i] = (b[:, left] * frac + b[:, right] * (1 - frac)).T
    return coef


@pytest.mark.parametrize("case", ["a", "b"])
def test_scoring_entry_on_the_cv_tables(case):
    if case == "a":
        x, y, fid = _case_a()
        coef = _interpolated_table(x, y, fid, nlambda=20)
    else:
        x, y, fid = _case_b()
        coef = _interpolated_table(x, y, fid, nlambda=25, irls_maxit=30)
    _check_scores(x, y, fid, coef)


def _case_c_rows(nrow):
    """the first nrow rows of case c (p = 200, three folds)"""
    x, y = _data(1500, 200, 31)
    fid = np.random.default_rng(6).permutation(np.resize(np.arange(1, 4), 1500))
    fid[640:768] = 2
    return np.asfortranarray(x[:nrow]), y[:nrow], fid[:nrow]


def _sparse_table(seed, nfolds, ncol, q, density=0.1):
    """a coefficient table with about `density` of its entries set, growing from column to column"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(nfolds, ncol, q)) * (rng.uniform(size=(nfolds, ncol, q)) < density) * np.linspace(0.02, 0.6, ncol)[None, :, None]


@pytest.mark.parametrize("nrow,ncol,seed", [(1500, 9, 8), (200, 2100, 9)])
def test_scoring_entry_table_in_lds_and_through_the_cache(nrow, ncol, seed):
    """p = 200: nine columns sit in LDS (with a last column group of one); 2100 columns (3.4 MB a fold) are read through the cache, in two
    launches of at most 2048 columns per fold.  The wide table is scored on the first 200 rows (four chunks, the last one short): of
    the 420 000 probabilities of this seed the nearest to 0.5 is 4.2e-7 away (checked on the CPU; the precondition asserts it)"""
    x, y, fid = _case_c_rows(nrow)
    _check_scores(x, y, fid, _sparse_table(seed, 3, ncol, 201))


# ------------------------------------------------------------------------------------------------------------- end to end
_E2E = {}


def _e2e_reference():
    if not _E2E:
        x, y, fid = _case_a()
        _E2E.update(x=x, y=y, fid=fid, fitted=CV.fits(x, y, fid, penalty=["lasso"], nlambda=20))
    return _E2E


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    return float(np.max(np.abs(a[ok] - b[ok]) / (1.0 + np.abs(b[ok])))) if ok.any() else 0.0


def _check_cv_oem(E, measure, grouped, **kw):
    """cv_oem(family="binomial") on E's x, y and foldid against the restatement, with its preconditions; kw: the fit's options, those of
    E["fitted"].  Returns the restatement's result"""
    import oem_amd
    nfolds = int(E["fid"].max())
    ref = CV.cv(E["x"], E["y"], E["fid"], penalty=["lasso"], type_measure=measure, grouped=grouped, fitted=E["fitted"], **kw)
    crit = np.sort(-ref["cvm"][0] if measure == "auc" else ref["cvm"][0])
    if measure == "class":
        crit = np.unique(crit)
    assert (crit[1] - crit[0]) > 1e-5 * abs(crit[0]), crit[:3]
    if measure == "auc":
        pv = ref["fit.preval"][0]
        for i in range(1, nfolds + 1):
            for j in range(pv.shape[1]):
                col = pv[E["fid"] == i, j]
                assert np.isnan(col).all() or len(np.unique(col)) == len(col)
    got = oem_amd.cv_oem(E["x"], E["y"], family="binomial", penalty="lasso", type_measure=measure, grouped=grouped, foldid=E["fid"], keep=True,
                         **kw)
    assert got["name"] == ref["name"] and got["penalty"] == ["lasso"] and got["best.model"] == "lasso"
    assert isinstance(got["oem.fit"], oem_amd.OemFitBinomial)
    lam_g, lam_r = np.asarray(got["lambda"][0]), np.asarray(ref["lambda"][0])
    assert lam_g.shape == lam_r.shape                                                   # the same columns survive the NA trimming
    assert np.array_equal(lam_g, np.asarray(got["oem.fit"]["lambda"][0])[:len(lam_g)])    # exactly the full fit's own
    print("lambda max rel diff to the restatement", np.max(np.abs(lam_g - lam_r) / lam_r))
    np.testing.assert_allclose(lam_g, lam_r, rtol=1e-12)
    assert np.array_equal(got["nzero"][0], ref["nzero"][0])
    d = {k: _rel(got[k][0], ref[k][0]) for k in ("cvm", "cvsd", "cvup", "cvlo", "fit.preval")}
    print("cv_oem", measure, "grouped" if grouped else "rows", "differences / (1 + |value|):", d)
    assert max(d.values()) <= CV_TOL, d
    assert np.array_equal(got["foldid"], E["fid"])
    for key in ("lambda.min", "lambda.1se"):                                            # the same element of the sequence
        assert got[key] == lam_g[int(np.nonzero(lam_r == ref[key])[0][0])], key
    assert got["model.min"] == ref["model.min"]
    return ref


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("measure", ["deviance", "class", "mse", "mae", "auc"])
def test_cv_oem_binomial_end_to_end(measure, grouped):
    _check_cv_oem(_e2e_reference(), measure, grouped, nlambda=20)


def test_cv_oem_binomial_consumers_and_a_device_x():
    """a device tensor is used as it is and gives the bits of the numpy x; predict_cv, summary_cv and plot_cv take the result"""
    import torch

    import oem_amd
    E = _e2e_reference()
    kw = dict(family="binomial", penalty=["lasso", "mcp"], nlambda=12, foldid=E["fid"], parallel=True)
    a = oem_amd.cv_oem(E["x"], E["y"], **kw)
    b = oem_amd.cv_oem(torch.as_tensor(E["x"], device="cuda:0"), E["y"], **kw)
    for m in range(2):
        assert np.array_equal(a["cvm"][m], b["cvm"][m]) and np.array_equal(a["cvsd"][m], b["cvsd"][m])
    assert a["name"] == "Binomial Deviance" and "fit.preval" not in a
    prob = oem_amd.predict_cv(a, E["x"][:50], type="response")
    cls = oem_amd.predict_cv(a, E["x"][:50], s="lambda.1se", type="class")
    assert prob.shape == (50, 1) and np.all((prob > 0) & (prob < 1)) and set(np.unique(cls)) <= {0, 1}
    s = oem_amd.summary_cv(a)
    assert s["model"] == "logistic" and s["type.measure"] == "Binomial Deviance" and s["n"] == 1500
    assert "logistic regression" in oem_amd.format_summary(s)
    drawn = oem_amd.plot_cv(a, which_model=1, show=False)
    assert drawn["ylab"] == "Binomial Deviance" and drawn["main"] == "mcp" and np.array_equal(drawn["cvm"], a["cvm"][1])


def test_cv_oem_binomial_small_fold_warnings():
    import oem_amd
    x, y = _data(60, 4, 33, k=2)
    fid = np.resize(np.arange(1, 8), 60)                               # 60 / 7 < 10
    with pytest.warns(UserWarning, match="Too few"):
        r = oem_amd.cv_oem(x, y, family="binomial", penalty="lasso", nlambda=5, type_measure="auc", foldid=fid)
    assert r["name"] == "Binomial Deviance"
    fid = np.resize(np.arange(1, 25), 60)                              # 60 / 24 < 3
    with pytest.warns(UserWarning, match="grouped=FALSE enforced"):
        oem_amd.cv_oem(x, y, family="binomial", penalty="lasso", nlambda=5, lambda_min_ratio=0.1, foldid=fid)
