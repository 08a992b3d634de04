"""CPU restatement of the sparse binomial fit (ref src/oem_logistic_sparse.cpp:30-313, src/oem_logistic_sparse.h) in numpy and
scipy.sparse.

TEST INFRASTRUCTURE ONLY: the tests hold liboemgpu's oemgpu_fit_logistic_sparse to this, and this to the dense restatement
(tests/logistic_restatement.py) and to the KKT conditions of the penalised logistic likelihood.  It is not oemLogisticDense on a
sparse matrix; the differences are kept as the reference has them:
  1. the single-thread branch of solve() (R's default ncores; cpp :88, 107-110; h :869-891);
  2. colsq = sum x^2 / (n - 1) over the stored values, 0 -> 1, s = 1 / sqrt(colsq), only with standardize (h :735-750); X not centred;
  3. eta = X (beta_tail o s) + beta_0 with an intercept (beta_0 as it is, no intval; h :874-877), X (beta o s) or X beta without one
     (h :885-890).  An intercept without standardize reads colsq_inv the reference never wrote (h :724, :880): refused;
  4. W = prob (1 - prob); the floor loop tests W(i) with i the IRLS index (h :963-969);
  5. the Hessian at every IRLS step but the skipped first step of a later lambda (h :866, :973); hessian.type is never read;
  6. with an intercept (h :456-528): XX[1:, 1:] = S X'WX S, colsums = (X'W) o s; at the first Hessian build xxdiag = mean diag
     XX[1:, 1:] and intval = sqrt((xxdiag / sum W) / n), recomputed only while xxdiag <= 0 (init_oem, once per call, is the only
     reset); XX[0, 1:] = intval colsums, XX[0, 0] = xxdiag; then XX /= n, d = 1.0005 lambda_max(XX), A = dI - XX;
  7. grad_tail = s o X'(y - prob) / n, grad_0 = sum (y - prob) / n (not scaled by intval), XY = XX beta + grad (h :981-1007);
  8. the first XY: XY_tail = s o X'y / n, XY_0 = sum y * intval = 0; lambda_0 over the non-intercept slots (h :752-811);
  9. get_beta (h :1040-1062) does beta_0 *= intval on the solver's own beta after every lambda (cpp :243), so the next lambda
     warm-starts from the rescaled intercept; it returns [beta_0, beta_tail o s];
 10. as the dense fit: the inner loop, the IRLS stop, niter = i + 1, the loss of the last prob, the last d, the intercept's penalty
     factor 0, "ols" with a single lambda;
 11. p + intercept >= n (the XWXt branch, h :497-502) is refused.
`stats` (optional dict) counts as the dense restatement's does; after the call stats["intval"] holds intval (0 when never computed).
"""
import numpy as np
import scipy.sparse as sp

from tests.logistic_restatement import _clamped, _loss, lambda_grid, next_beta, stop_rule


class Unsupported(ValueError):
    """a case the library refuses with OEMGPU_ERR_UNSUPPORTED"""


def fit(x, y, penalty=("lasso",), lambda_=None, nlambda=100, lambda_min_ratio=1e-4, alpha=1.0, gamma=3.0, tau=0.5,
        groups=None, unique_groups=None, group_weights=None, penalty_factor=None, standardize=True, intercept=True,
        compute_loss=False, maxit=500, tol=1e-7, irls_maxit=100, irls_tol=1e-3, stats=None):
    """Returns dict(beta=[(p + 1) x nl per penalty], lambda=[...], niter=[...], loss=[...], d=float, intval=float).
    x: any scipy.sparse matrix (or a dense array).  groups / unique_groups: as handed to the C entry (q entries with an intercept)."""
    x = sp.csc_matrix(x, dtype=np.float64)
    x.sum_duplicates()
    x.sort_indices()
    y = np.asarray(y, dtype=np.float64).ravel()
    n, p = x.shape
    o = 1 if intercept else 0
    q = p + o
    if intercept and not standardize:
        raise Unsupported("intercept without standardize")
    if q >= n:
        raise Unsupported("p + intercept >= n")
    if standardize:
        colsq = np.asarray(x.multiply(x).sum(axis=0)).ravel() / (n - 1.0)
        colsq[colsq == 0.0] = 1.0
        s = 1.0 / np.sqrt(colsq)
    else:
        s = np.ones(p)
    xt = x.T.tocsr()
    pf = np.ones(p) if penalty_factor is None else np.asarray(penalty_factor, dtype=np.float64)
    pf = np.concatenate([[0.0], pf]) if intercept else pf
    xy0 = np.zeros(q)
    xy0[o:] = (xt @ y) * s / n
    lmax = float(np.max(np.abs(xy0[o:])))
    provided = lambda_ is not None and len(lambda_) > 0
    nl = len(lambda_[0]) if provided else nlambda
    base = None if provided else lambda_grid(lmax, nlambda, lambda_min_ratio)
    grp = None
    if groups is not None and len(groups) > 0 and any("grp" in pn for pn in penalty):
        groups = np.asarray(groups)
        ug = np.asarray(unique_groups)
        gidx = [np.nonzero(groups == g)[0] for g in ug]
        gzero = [int(g) == 0 for g in ug]
        if group_weights is not None and len(group_weights) > 0:
            gw = np.asarray(group_weights, dtype=np.float64)
        else:
            gw = np.array([0.0 if gz else np.sqrt(len(ix)) for ix, gz in zip(gidx, gzero)])
        grp = (gidx, gw, gzero)
    out = dict(beta=[], **{"lambda": []}, niter=[], loss=[], d=0.0, intval=0.0)
    d = 0.0
    xxdiag, intval = 0.0, 0.0                                        # init_oem (h :731-732): once per call
    st = stats if stats is not None else {}
    for key in ("irls", "inner", "rows", "grams", "floored", "clamped"):
        st.setdefault(key, 0)
    for k, pen in enumerate(penalty):
        if provided:
            lam = np.asarray(lambda_[k], dtype=np.float64)
        else:
            lam = base.copy()
            if pen.endswith(".net"):
                lam = base / alpha
                if "mcp" in pen or "scad" in pen:
                    fact = 3.5 - min(3.5, gamma) * 5.71425 / 8.0
                    lam = fact * base / alpha ** 0.8
        nlk = 1 if pen == "ols" else nl
        B = np.zeros((p + 1, nl))
        NI = np.zeros(nl, dtype=np.int32)
        LO = np.full(nl, 1e99)
        beta = np.zeros(q)
        XX = A = XY = prob = None
        for li in range(nlk):
            i = 0
            while i < irls_maxit:
                beta_irls = beta.copy()
                if not (i == 0 and li > 0):
                    eta = x @ (beta[o:] * s) + (beta[0] if intercept else 0.0)
                    prob = 1.0 / (1.0 + np.exp(-eta))
                    W = prob * (1.0 - prob)
                    st["rows"] += 1
                    if i < n and W[i] < 1e-5:
                        W[i] = 1e-5
                        st["floored"] += 1
                    st["grams"] += 1
                    G = (xt @ sp.diags(W) @ x).toarray()
                    XX = np.zeros((q, q))
                    XX[o:, o:] = s[:, None] * G * s[None, :]
                    if intercept:
                        colsums = (xt @ W) * s
                        if xxdiag <= 0:
                            xxdiag = float(np.mean(np.diag(XX[1:, 1:])))
                            intval = np.sqrt((xxdiag / W.sum()) / n)
                        XX[0, 1:] = intval * colsums
                        XX[1:, 0] = intval * colsums
                        XX[0, 0] = xxdiag
                    XX /= n
                    d = float(np.linalg.eigvalsh(XX)[-1]) * 1.0005
                    A = -XX
                    A[np.diag_indices(q)] += d
                    r = y - prob
                    grad = np.zeros(q)
                    grad[o:] = ((xt @ r) / n) * s
                    if intercept:
                        grad[0] = r.sum() / n
                    XY = XX @ beta + grad
                for j in range(maxit):
                    bp = beta
                    u = A @ bp + XY
                    beta = next_beta(pen, u, lam[li], d, pf, alpha, gamma, tau, grp)
                    st["inner"] += 1
                    if stop_rule(beta, bp, tol):
                        break
                st["irls"] += 1
                if stop_rule(beta, beta_irls, irls_tol):
                    break
                i += 1
            NI[li] = i + 1
            if compute_loss:
                LO[li] = _loss(y, prob)
                st["clamped"] += _clamped(y, prob)
            if intercept:
                beta = beta.copy()
                beta[0] *= intval                                   # get_beta, in place (h :1040-1044)
            B[0, li] = beta[0] if intercept else 0.0
            B[1:, li] = beta[o:] * s
        if pen == "ols":
            out["beta"].append(B[:, :1]); out["niter"].append(int(NI[0])); out["loss"].append(float(LO[0]))
        else:
            out["beta"].append(B); out["niter"].append(NI); out["loss"].append(LO)
        out["lambda"].append(np.asarray(lam, dtype=np.float64))
    out["d"] = d
    out["intval"] = float(intval)
    st["intval"] = float(intval)
    return out
