"""Test infrastructure: cv.oem(family = "gaussian") written out again from the reference's R (R/cv_oem.R:56-221 with
cv.oemfit_gaussian, :349-423; cvcompute, R/utils.R:128-144; lambda.interp, R/utils.R:64-98; getmin, R/utils.R:3-20), on the oracle's
oemDense (oracle.fit_dense) -- nothing here imports oem_amd.  K + 1 fits on gathered rows, every fold on its own lambda grid; the
held-out rows are predicted at the full fit's lambdas by linear interpolation of the fold's coefficients, only at the lambdas no
fold has to extrapolate to, packed into the leading columns; then fold means weighted by fold size (grouped) or plain means over
the rows (not grouped)."""
import numpy as np

from oracle import oracle as orc


def lambda_interp(lam, s):
    """lambda.interp (R/utils.R:64-98): left / right neighbours and the weight of the left one, for s on the sequence lam."""
    lam = np.asarray(lam, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    if len(lam) == 1:
        z = np.zeros(len(s), dtype=int)
        return z, z, np.ones(len(s))
    s = np.minimum(np.maximum(s, lam.min()), lam.max())          # s[s > max(lambda)] = max(lambda); s[s < min(lambda)] = min(lambda)
    k = len(lam)
    sfrac = (lam[0] - s) / (lam[0] - lam[k - 1])
    lamn = (lam[0] - lam) / (lam[0] - lam[k - 1])
    coord = np.interp(sfrac, lamn, np.arange(1, k + 1))          # approx(lambda, seq(lambda), sfrac)$y
    left, right = np.floor(coord).astype(int), np.ceil(coord).astype(int)
    frac = np.ones(len(s))
    d = left != right
    frac[d] = (sfrac[d] - lamn[right[d] - 1]) / (lamn[left[d] - 1] - lamn[right[d] - 1])
    return left - 1, right - 1, frac


def predict_at(fit, m, newx, s):
    """predict.oem(fit, newx, s = s, which.model = m) (R/methods.R:48-109): cbind(1, newx) %*% interpolated coefficients"""
    left, right, frac = lambda_interp(fit["lambda"][m], s)
    b = np.asarray(fit["beta"][m])
    nb = b[:, left] * frac + b[:, right] * (1.0 - frac)
    return nb[0] + newx @ nb[1:]


def cvcompute(mat, weights, foldid, nlams):
    """R/utils.R:128-144: the weighted mean of every fold's rows per column; a column is good for a fold up to nlams[fold]"""
    nfolds = int(foldid.max())
    out = np.full((nfolds, mat.shape[1]), np.nan)
    good = np.zeros((nfolds, mat.shape[1]))
    mat = np.where(np.isinf(mat), np.nan, mat)
    wisum = np.zeros(nfolds)
    for i in range(nfolds):
        rows = foldid == i + 1
        wi = weights[rows]
        mi = mat[rows]
        for j in range(mat.shape[1]):
            ok = ~np.isnan(mi[:, j])
            out[i, j] = np.sum(mi[ok, j] * wi[ok]) / np.sum(wi[ok]) if ok.any() else np.nan      # weighted.mean(..., na.rm = TRUE)
        good[i, :nlams[i]] = 1
        wisum[i] = wi.sum()
    return out, wisum, good.sum(axis=0)


def _wmean_cols(a, w):
    out = np.full(a.shape[1], np.nan)
    for j in range(a.shape[1]):
        ok = ~np.isnan(a[:, j])
        if ok.any():
            out[j] = np.sum(a[ok, j] * w[ok]) / np.sum(w[ok])
    return out


def cv_statistics(predmats, y, foldid, nlams, type_measure, grouped):
    """cv.oemfit_gaussian from predmat on (R/cv_oem.R:392-423): (cvm, cvsd) per model"""
    n = len(y)
    cvm, cvsd = [], []
    for pm in predmats:
        raw = (y[:, None] - pm) ** 2 if type_measure == "mse" else np.abs(y[:, None] - pm)
        N = n - np.isnan(pm).sum(axis=0)
        w = np.ones(n)
        if grouped:
            raw, w, N = cvcompute(raw, w, foldid, nlams)
        m = _wmean_cols(raw, w)
        with np.errstate(invalid="ignore", divide="ignore"):
            sd = np.sqrt(_wmean_cols((raw - m) ** 2, w) / (N - 1))
        cvm.append(m); cvsd.append(sd)
    return cvm, cvsd


def getmin(lam, cvm, cvsd):
    """getmin over several models (R/utils.R:3-20): the model and lambda of the smallest cvm; ties take the largest lambda"""
    mins = [np.nanmin(c) for c in cvm]
    which = int(np.argmin(mins))
    lam_min = float(np.max(lam[which][cvm[which] <= mins[which]]))
    return which, lam_min


def cv_oem(x, y, foldid, penalty, type_measure="mse", grouped=True, lambda_=None, standardize=True, intercept=True, fits=None, **kw):
    """The whole of cv.oem.  fits: (full fit, fold fits) of an earlier call on the same data and options, to skip the K + 1 fits.
    Returns a dict: lambda, cvm, cvsd (NaN columns trimmed as cv.oem trims them), predmat (fit.preval, untrimmed), which_lam,
    model_min (0-based), lambda_min, fits."""
    x = np.asarray(x, dtype=np.float64); y = np.asarray(y, dtype=np.float64).ravel()
    foldid = np.asarray(foldid).ravel()
    n, p = x.shape
    nfolds = int(foldid.max())
    penalty = [penalty] if isinstance(penalty, str) else list(penalty)
    if fits is None:
        opts = dict(penalty=penalty, standardize=standardize, intercept=intercept, lambda_=lambda_, **kw)
        opts.setdefault("lambda_min_ratio", 1e-4)                # R/oem.R: n >= p
        fit0 = orc.fit_dense(x, y, **opts)
        outlist = [orc.fit_dense(x[foldid != i], y[foldid != i], **opts) for i in range(1, nfolds + 1)]
        fits = (fit0, outlist)
    fit0, outlist = fits
    lam = [np.asarray(l, dtype=np.float64) for l in fit0["lambda"]]
    nmodels, nl = len(penalty), len(lam[0])
    which_lam = [lam[m] >= max(np.min(o["lambda"][m]) for o in outlist) for m in range(nmodels)]
    predmats = [np.full((n, nl), np.nan) for _ in range(nmodels)]
    nlams = np.zeros(nfolds, dtype=int)
    for i in range(nfolds):
        rows = foldid == i + 1
        nlami = 0
        for m in range(nmodels):
            nlami = int(which_lam[m].sum())
            if rows.any() and nlami > 0:
                predmats[m][rows, :nlami] = predict_at(outlist[i], m, x[rows], lam[m][which_lam[m]])
        nlams[i] = nlami                                          # of the last model (R/cv_oem.R:386-389)
    if n / nfolds < 3 and grouped:
        grouped = False
    cvm, cvsd = cv_statistics(predmats, y, foldid, nlams, type_measure, grouped)
    nas = np.zeros(nl, dtype=bool)
    for m in range(nmodels):
        nas |= np.isnan(cvsd[m])
    lam_t = [l[~nas] for l in lam]; cvm = [c[~nas] for c in cvm]; cvsd = [c[~nas] for c in cvsd]
    which, lam_min = getmin(lam_t, cvm, cvsd)
    return {"lambda": lam_t, "cvm": cvm, "cvsd": cvsd, "predmat": predmats, "which_lam": which_lam, "model_min": which,
            "lambda_min": lam_min, "fits": fits}
