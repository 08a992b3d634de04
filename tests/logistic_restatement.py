"""CPU restatement of the dense binomial fit (ref src/oem_logistic_dense.cpp:30-313, src/oem_logistic_dense.h:397-1094) in numpy.

TEST INFRASTRUCTURE ONLY: the tests hold liboemgpu's oemgpu_fit_logistic_dense to this, and this to independent solutions (the KKT
conditions of the penalised logistic likelihood, scikit-learn).  Quirks are kept as the reference has them:
  * colsq = sum x^2 / (n - 1), X not centred, 0 -> 1; s = 1 / sqrt(colsq) when standardize (h :727-738);
  * the intercept is coordinate 0 of q = p + 1 with penalty factor 0 (cpp :119-141); XX row / column 0 = [sum W, sum W x s] / n;
  * XY = s o X'Y / n with the raw 0/1 Y; lambda_0 = max |XY| over the non-intercept slots (h :762-805);
  * W floor: only element i (the IRLS index) is tested (h :953-959);
  * XX, d = 1.0005 lambda_max(XX), A only at (i == 0 and the first lambda) or for hessian "full" (h :964-965);
  * on a lambda after the first, the first IRLS step skips prob / XX / grad / XY (h :861);
  * niter = i + 1 (irls_maxit + 1 at the cap); loss = get_loss of the LAST prob computed (h :1057-1090); d = the last d.
`stats` (optional dict) counts what ran: irls (IRLS steps), inner (OEM iterations), rows (row passes: IRLS steps that are not the
skipped first step of a later lambda), grams (Hessian builds), floored (weights the W floor changed), clamped (terms of the reported
losses that took a 1e-5 clamp).
"""
import numpy as np

PENALTIES = ["elastic.net", "lasso", "ols", "mcp", "scad", "mcp.net", "scad.net",
             "grp.lasso", "grp.lasso.net", "grp.mcp", "grp.scad", "grp.mcp.net",
             "grp.scad.net", "sparse.grp.lasso"]


def stop_rule(cur, prev, tol):
    """ref src/utils.cpp:537-549: True = converged"""
    cn, pn = np.abs(cur) > 1e-13, np.abs(prev) > 1e-13
    if np.any(cn != pn):
        return False
    both = cn & pn
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs((cur[both] - prev[both]) / prev[both])
    return not np.any(rel > tol)


def _soft(u, tp, d):
    return np.where(u > tp, (u - tp) / d, np.where(u < -tp, (u + tp) / d, 0.0))


def _mcp(u, tp, d, gamma):
    gd, dmg = gamma * d, d - 1.0 / gamma
    return np.where(np.abs(u) > gd * tp, u / d, np.where(u > tp, (u - tp) / dmg, np.where(u < -tp, (u + tp) / dmg, 0.0)))


def _scad(u, tp, d, gamma):
    gd, g1d = gamma * d, (gamma - 1.0) * d
    gp, gq = (gamma - 1.0) * u, gamma * tp
    mid = np.where(gp > gq, (gp - gq) / (g1d - 1.0), np.where(gp < -gq, (gp + gq) / (g1d - 1.0), 0.0))
    low = np.where(u > tp, (u - tp) / d, np.where(u < -tp, (u + tp) / d, 0.0))
    return np.where(np.abs(u) > gd * tp, u / d, np.where(np.abs(u) > (d + 1.0) * tp, mid, low))


def _scad_norm(b, pen, d, gamma):
    gd, g1d = gamma * d, (gamma - 1.0) * d
    if abs(b) > gd * pen:
        return 1.0
    if abs(b) > (d + 1.0) * pen:
        gp, gq = gamma - 1.0, gamma * pen / b
        if gp > gq:
            return d * (gp - gq) / (g1d - 1.0)
        if gp < -gq:
            return d * (gp + gq) / (g1d - 1.0)
        return 0.0
    if b > pen:
        return 1.0 - pen / b
    if b < -pen:
        return 1.0 + pen / b
    return 0.0


def _mcp_norm(b, pen, d, gamma):
    if abs(b) > gamma * d * pen:
        return 1.0
    dmg = d - 1.0 / gamma
    if b > pen:
        return d * (1.0 - pen / b) / dmg
    if b < -pen:
        return d * (1.0 + pen / b) / dmg
    return 0.0


def _block(u, lam, d, kind, gamma, gidx, gw, gzero, q):
    out = np.zeros(q)
    for g, idx in enumerate(gidx):
        if gzero[g]:
            f = 1.0
        else:
            nrm = np.sqrt(float(np.sum(u[idx] * u[idx])))
            pen = lam * gw[g]
            if kind == "mcp":
                f = _mcp_norm(nrm, pen, d, gamma)
            elif kind == "scad":
                f = _scad_norm(nrm, pen, d, gamma)
            else:
                with np.errstate(divide="ignore", invalid="ignore"):
                    f = max(0.0, 1.0 - pen / nrm) if nrm > 0 or pen > 0 else 0.0
                if np.isnan(f):
                    f = 0.0
        if f != 0.0:
            out[idx] = u[idx] * f / d
    return out


def next_beta(pen, u, lam, d, pf, alpha, gamma, tau, grp):
    """ref h :569-672"""
    Ln, Dn = lam * alpha, d + (1.0 - alpha) * lam
    if pen == "lasso":
        return _soft(u, pf * lam, d)
    if pen == "ols":
        return u / d
    if pen == "elastic.net":
        return _soft(u, pf * Ln, Dn)
    if pen == "scad":
        return _scad(u, pf * lam, d, gamma)
    if pen == "scad.net":
        L, D = (0.0, d + lam) if alpha == 0 else (Ln, Dn)
        return _scad(u, pf * L, D, gamma)
    if pen == "mcp":
        return _mcp(u, pf * lam, d, gamma)
    if pen == "mcp.net":
        return _mcp(u, pf * Ln, Dn, gamma)
    gidx, gw, gzero = grp
    q = len(u)
    if pen == "sparse.grp.lasso":
        v = _soft(u, pf * (tau * lam), 1.0)
        return _block(v, (1.0 - tau) * lam, d, "lasso", gamma, gidx, gw, gzero, q)
    kind = "mcp" if "mcp" in pen else ("scad" if "scad" in pen else "lasso")
    L, D = (Ln, Dn) if pen.endswith(".net") else (lam, d)
    return _block(u, L, D, kind, gamma, gidx, gw, gzero, q)


def _clamped(y, prob):
    """terms of get_loss that take the log(1 / 1e-5) branch"""
    return int(np.sum(np.where(y == 1, prob <= 1e-5, prob > 1.0 - 1e-5)))


def _loss(y, prob):
    """get_loss, ref h :1057-1090"""
    l1 = np.where(prob > 1e-5, np.log(1.0 / np.maximum(prob, 1e-300)), np.log(1.0 / 1e-5))
    l0 = np.where(prob <= 1.0 - 1e-5, np.log(1.0 / np.maximum(1.0 - prob, 1e-300)), np.log(1.0 / 1e-5))
    return float(np.sum(np.where(y == 1, l1, l0)))


def lambda_grid(lmax, nlambda, lambda_min_ratio):
    """cpp :164-171"""
    lmin = lambda_min_ratio * lmax
    a, b = np.log(lmax), np.log(lmin)
    if nlambda == 1:
        return np.exp(np.array([a]))
    return np.exp(np.array([b if i == nlambda - 1 else a + (b - a) / (nlambda - 1) * i for i in range(nlambda)]))


def fit(x, y, penalty=("lasso",), lambda_=None, nlambda=100, lambda_min_ratio=1e-4, alpha=1.0, gamma=3.0, tau=0.5,
        groups=None, unique_groups=None, group_weights=None, penalty_factor=None, standardize=True, intercept=True,
        compute_loss=False, maxit=500, tol=1e-7, irls_maxit=100, irls_tol=1e-3, hessian_full=False, stats=None):
    """Returns dict(beta=[(p + 1) x nl per penalty], lambda=[...], niter=[...], loss=[...], d=float).
    groups / unique_groups: as handed to the C entry (with an intercept, groups has q = p + 1 entries with the intercept's first)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).ravel()
    n, p = x.shape
    o = 1 if intercept else 0
    q = p + o
    if standardize:
        colsq = np.sum(x * x, axis=0) / (n - 1.0)
        colsq[colsq == 0.0] = 1.0
        s = 1.0 / np.sqrt(colsq)
    else:
        s = np.ones(p)
    pf = np.ones(p) if penalty_factor is None else np.asarray(penalty_factor, dtype=np.float64)
    pf = np.concatenate([[0.0], pf]) if intercept else pf
    xy0 = np.zeros(q)
    xy0[o:] = ((x.T @ y) * s) / n
    if intercept:
        xy0[0] = y.sum() / n
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
    out = dict(beta=[], **{"lambda": []}, niter=[], loss=[], d=0.0)
    d = 0.0
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
        LO = np.full(nl, 1e99) if compute_loss else np.full(nl, 1e99)
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
                    if (i == 0 and li == 0) or hessian_full:
                        st["grams"] += 1
                        sw = np.sqrt(W)
                        Z = sw[:, None] * (x * s)
                        if intercept:
                            Z = np.column_stack([sw, Z])
                        XX = (Z.T @ Z) / n
                        d = float(np.linalg.eigvalsh(XX)[-1]) * 1.0005
                        A = -XX
                        A[np.diag_indices(q)] += d
                    r = y - prob
                    grad = np.zeros(q)
                    grad[o:] = ((x.T @ r) / n) * s
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
            B[0, li] = beta[0] if intercept else 0.0
            B[1:, li] = beta[o:] * s
        if pen == "ols":
            out["beta"].append(B[:, :1]); out["niter"].append(int(NI[0])); out["loss"].append(float(LO[0]))
        else:
            out["beta"].append(B); out["niter"].append(NI); out["loss"].append(LO)
        out["lambda"].append(np.asarray(lam, dtype=np.float64))
    out["d"] = d
    return out


def near_separable(n, p, seed, k=4):
    """Gaussian x whose rows 0-9 sit far out along the true beta (|eta| 20-40 under it); rows 0-6 are labelled as the true beta says,
    rows 7-9 against it.  Once a fit has grown, the W floor (row i at IRLS step i) and the loss clamps of the mislabelled rows fire."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, p))
    b = np.zeros(p)
    b[:k] = rng.choice([-1.0, 1.0], k) * rng.uniform(0.5, 1.0, k)
    sgn = rng.choice([-1.0, 1.0], 10)
    eta_far = sgn * rng.uniform(20.0, 40.0, 10)
    x[:10] = np.outer(eta_far / float(b @ b), b) + 0.1 * rng.normal(size=(10, p))
    eta = x @ b
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    y[:10] = (eta[:10] > 0).astype(np.float64)
    y[7:10] = 1.0 - y[7:10]
    return np.asfortranarray(x), y
