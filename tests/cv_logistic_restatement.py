"""CPU restatement of cv.oem for family = "binomial" in numpy: cv.oem (ref R/cv_oem.R:56-221), cv.oemfit_binomial (:224-346),
cvcompute, lambda.interp, auc / auc.mat and getmin (R/utils.R), with tests/logistic_restatement.fit on x[keep], y[keep] as the fold fit.

TEST INFRASTRUCTURE ONLY: the tests hold oem_amd.cv_oem(family="binomial") and the two C entries under it to this, and this to
scikit-learn's metrics.  It shares no code with the library: it has its own interpolation and never imports oem_amd.api.  It follows
the R text line by line -- the n x nlambda matrices of predictions and raw errors are formed as R forms them -- so that the library's
route (sums per fold and column from the device) is checked against the definition and not against itself.
  * every fold is fitted on its own lambda sequence unless lambda_ is given; which_lam keeps the full fit's lambdas that no fold has to
    extrapolate below (:263-269); nlams[i] is the LAST model's count for every fold (:286);
  * auc.mat with unit weights; tied probabilities are ordered by row (the reference draws runif: any order is one of its draws).
"""
import warnings

import numpy as np

from tests import logistic_restatement as R

TYPENAMES = {"mse": "Mean-Squared Error", "mae": "Mean Absolute Error", "deviance": "Binomial Deviance", "auc": "AUC",
             "class": "Misclassification Error"}


def lambda_interp(lam, s):
    """lambda.interp (R/utils.R:64-87); 0-based left / right"""
    lam = np.asarray(lam, dtype=np.float64)
    s = np.array(s, dtype=np.float64)
    if len(lam) == 1:
        z = np.zeros(len(s), dtype=int)
        return z, z, np.ones(len(s))
    s[s > lam.max()] = lam.max()
    s[s < lam.min()] = lam.min()
    k = len(lam)
    sfrac = (lam[0] - s) / (lam[0] - lam[k - 1])
    lamn = (lam[0] - lam) / (lam[0] - lam[k - 1])
    coord = np.interp(sfrac, lamn, np.arange(k, dtype=np.float64))          # approx(lambda, seq(lambda), sfrac)$y
    left, right = np.floor(coord).astype(int), np.ceil(coord).astype(int)
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = (sfrac - lamn[right]) / (lamn[left] - lamn[right])
    frac[left == right] = 1.0
    return left, right, frac


def predict_response(fit, x, s, m):
    """predict.oemfit_binomial(type = "response") at the lambdas s (R/methods.R:48-109, :346-367)"""
    left, right, frac = lambda_interp(fit["lambda"][m], s)
    b = np.asarray(fit["beta"][m])
    nb = b[:, left] * frac + b[:, right] * (1 - frac)
    eta = np.column_stack([np.ones(x.shape[0]), x]) @ nb
    return 1.0 / (1.0 + np.exp(-eta))


def auc(y, prob, w, tie):
    """auc() with weights (R/utils.R:101-115); `tie` stands where the reference draws rprob = runif(): order(prob, tie)"""
    op = np.lexsort((tie, prob))
    y, w = y[op], w[op]
    cw = np.cumsum(w)
    w1 = w[y == 1]
    cw1 = np.cumsum(w1)
    with np.errstate(divide="ignore", invalid="ignore"):
        wauc = np.log(np.sum(w1 * (cw[y == 1] - cw1)))
        sumw1 = cw1[-1]
        sumw2 = cw[-1] - sumw1
        return float(np.exp(wauc - np.log(sumw1) - np.log(sumw2)))


def auc_mat(ymat, prob, weights=None):
    """auc.mat (R/utils.R:119-125): the rows twice, as class 0 with weight y[, 1] and as class 1 with weight y[, 2]"""
    ny = ymat.shape[0]
    weights = np.ones(ny) if weights is None else weights
    W = np.concatenate([weights * ymat[:, 0], weights * ymat[:, 1]])
    Y = np.concatenate([np.zeros(ny), np.ones(ny)])
    rows = np.arange(ny, dtype=np.float64)       # ties by row; a row's two copies tie again, and one of them has weight 0
    return auc(Y, np.concatenate([prob, prob]), W, np.concatenate([rows, rows]))


def raw_errors(ymat, pred, type_measure):
    """the switch of cv.oemfit_binomial (R/cv_oem.R:315-327); ymat: the n x 2 indicator matrix, pred: n x k (NaN where not predicted)"""
    y1, y2 = ymat[:, :1], ymat[:, 1:]
    if type_measure == "mse":
        return (y1 - (1 - pred)) ** 2 + (y2 - pred) ** 2
    if type_measure == "mae":
        return np.abs(y1 - (1 - pred)) + np.abs(y2 - pred)
    if type_measure == "deviance":
        pm = np.minimum(np.maximum(pred, 1e-5), 1 - 1e-5)
        pm = np.where(np.isnan(pred), np.nan, pm)
        lp = y1 * np.log(1 - pm) + y2 * np.log(pm)
        return 2 * (0.0 - lp)                                    # ly = 0 for 0/1 indicators
    if type_measure == "class":
        return np.where(np.isnan(pred), np.nan, y1 * (pred > 0.5) + y2 * (pred <= 0.5))
    raise ValueError(type_measure)


def cvcompute(mat, weights, foldid, nlams):
    """R/utils.R:128-144"""
    nfolds = int(foldid.max())
    wisum = np.array([weights[foldid == i].sum() for i in range(1, nfolds + 1)])
    out = np.full((nfolds, mat.shape[1]), np.nan)
    good = np.zeros((nfolds, mat.shape[1]))
    mat = np.where(np.isinf(mat), np.nan, mat)
    for i in range(nfolds):
        mi, wi = mat[foldid == i + 1], weights[foldid == i + 1]
        for j in range(mat.shape[1]):
            ok = ~np.isnan(mi[:, j])
            out[i, j] = np.sum(mi[ok, j] * wi[ok]) / np.sum(wi[ok]) if ok.any() else np.nan
        good[i, :int(nlams[i])] = 1
    return out, wisum, good.sum(axis=0)


def _wmean(a, w):
    out = np.full(a.shape[1], np.nan)
    for j in range(a.shape[1]):
        ok = ~np.isnan(a[:, j])
        if ok.any():
            out[j] = np.sum(a[ok, j] * w[ok]) / np.sum(w[ok])
    return out


def getmin(lam, cvm, cvsd):
    """R/utils.R:3-26"""
    lmin, l1se, cvs = [], [], []
    for m in range(len(cvm)):
        idmin = cvm[m] <= np.min(cvm[m])
        lmin.append(np.max(lam[m][idmin]))
        cvs.append(np.min(cvm[m][idmin]))
        i0 = int(np.nonzero(lam[m] == lmin[m])[0][0])
        semin = (cvm[m] + cvsd[m])[i0]
        l1se.append(np.max(lam[m][cvm[m] < semin]))
    mmin = int(np.argmin(cvs))
    return {"lambda.min": lmin[mmin], "model.min": mmin + 1, "lambda.1se": l1se[mmin]}


def fits(x, y, foldid, penalty=("lasso",), lambda_=None, stats=None, **kw):
    """the K + 1 fits of cv.oem (R/cv_oem.R:105-175): (the full fit, [the fit without fold i on x[keep], y[keep]]).  stats: a list that
    receives the step counts of every fold fit (logistic_restatement.fit's `stats`)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).ravel()
    foldid = np.asarray(foldid).ravel()
    penalty = list(penalty)
    lam_arg = None if lambda_ is None else [np.sort(np.asarray(lambda_, dtype=np.float64))[::-1] for _ in penalty]
    fit0 = R.fit(x, y, penalty=penalty, lambda_=lam_arg, **kw)
    outlist = []
    for i in range(1, int(foldid.max()) + 1):
        keep = foldid != i
        st = {}
        outlist.append(R.fit(x[keep], y[keep], penalty=penalty, lambda_=lam_arg, stats=st, **kw))
        if stats is not None:
            stats.append(st)
    return fit0, outlist


def cv(x, y, foldid, penalty=("lasso",), lambda_=None, type_measure="default", grouped=True, fitted=None, **kw):
    """cv.oem(family = "binomial", keep = TRUE).  kw: the options of logistic_restatement.fit; fitted: what fits() returned for the same
    arguments (the fits do not depend on type_measure / grouped).  Returns the cv.oem list as a dict, plus `outlist` (the fold fits),
    `which_lam` and `cvraw` (per model, before the means)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).ravel()
    foldid = np.asarray(foldid).ravel()
    n = x.shape[0]
    penalty = list(penalty)
    fit0, outlist = fitted if fitted is not None else fits(x, y, foldid, penalty=penalty, lambda_=lambda_, **kw)
    nmodels = len(penalty)
    nz = [(np.abs(np.asarray(b)[1:]) > 0).sum(axis=0) for b in fit0["beta"]]
    nfolds = int(foldid.max())
    assert nfolds >= 3
    # cv.oemfit_binomial
    if type_measure == "default":
        type_measure = "deviance"
    lev = np.unique(y)
    ymat = np.column_stack([(y == lev[0]).astype(np.float64), (y == lev[-1]).astype(np.float64)])
    if n / nfolds < 10 and type_measure == "auc":
        warnings.warn("Too few (< 10) observations per fold for type.measure='auc' in cv.lognet; changed to type.measure='deviance'. "
                      "Alternatively, use smaller value for nfolds")
        type_measure = "deviance"
    if n / nfolds < 3 and grouped:
        warnings.warn("Option grouped=FALSE enforced in cv.glmnet, since < 3 observations per fold")
        grouped = False
    lam = [np.asarray(l, dtype=np.float64) for l in fit0["lambda"]]
    nl = len(lam[0])
    which_lam = [lam[m] >= max(np.min(o["lambda"][m]) for o in outlist) for m in range(nmodels)]
    predlist = [np.full((n, nl), np.nan) for _ in range(nmodels)]
    nlams = np.zeros(nfolds)
    for i in range(nfolds):
        rows = foldid == i + 1
        for m in range(nmodels):
            nlami = int(which_lam[m].sum())
            predlist[m][rows, :nlami] = predict_response(outlist[i], x[rows], lam[m][which_lam[m]], m)
        nlams[i] = nlami
    weights = np.ones(n)
    if type_measure == "auc":
        cvraw, N, w = [], [], []
        for m in range(nmodels):
            raw = np.full((nfolds, nl), np.nan)
            good = np.zeros((nfolds, nl))
            for i in range(nfolds):
                good[i, :int(nlams[i])] = 1
                rows = foldid == i + 1
                for j in range(int(nlams[i])):
                    raw[i, j] = auc_mat(ymat[rows], predlist[m][rows, j], weights[rows])
            cvraw.append(raw); N.append(good.sum(axis=0))
            w.append(np.array([weights[foldid == i].sum() for i in range(1, nfolds + 1)]))
    else:
        N = [n - np.isnan(pm).sum(axis=0) for pm in predlist]
        cvraw = [raw_errors(ymat, pm, type_measure) for pm in predlist]
        if grouped:
            obs = [cvcompute(c, weights, foldid, nlams) for c in cvraw]
            cvraw, w, N = [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs]
        else:
            w = [weights for _ in range(nmodels)]
    cvm = [_wmean(cvraw[m], w[m]) for m in range(nmodels)]
    with np.errstate(invalid="ignore", divide="ignore"):
        cvsd = [np.sqrt(_wmean((cvraw[m] - cvm[m]) ** 2, w[m]) / (N[m] - 1)) for m in range(nmodels)]
    nas = np.zeros(nl, dtype=bool)
    for m in range(nmodels):
        nas |= np.isnan(cvsd[m])
    raw_untrimmed = cvraw
    if nas.any():
        cvm = [c[~nas] for c in cvm]; cvsd = [c[~nas] for c in cvsd]
        nz = [c[~nas] for c in nz]; lam = [l[~nas] for l in lam]
    name = TYPENAMES[type_measure]
    out = {"lambda": lam, "cvm": cvm, "cvsd": cvsd, "cvup": [a + b for a, b in zip(cvm, cvsd)], "cvlo": [a - b for a, b in zip(cvm, cvsd)],
           "nzero": nz, "name": name, "oem.fit": fit0, "fit.preval": predlist, "foldid": foldid, "outlist": outlist, "which_lam": which_lam,
           "cvraw": raw_untrimmed}
    out.update(getmin(lam, [-c for c in cvm] if name == "AUC" else cvm, cvsd))
    out["best.model"] = penalty[out["model.min"] - 1]
    out["penalty"] = penalty
    return out
