"""CPU restatement of the many-response binomial fit (oem_fit_logistic_dense_multi) in numpy.

TEST INFRASTRUCTURE ONLY.  The lock-step driver as the library runs it -- XX, d and A built ONCE at beta = 0 and shared, every
response's own lambda grid, one IRLS step for all live responses at a time, a response frozen from the step at which it meets the
IRLS stop, no row pass at (i = 0, li > 0) -- with the per-response arithmetic written exactly as tests/logistic_restatement.fit writes
it, so that the two agree to the byte when the driver is right.  `stats`: steps (lock-step IRLS steps), rows (row passes), grams.
Also the data of the tests: one x, m responses with a signal scale and an offset of their own (so that they stop at different steps).
"""
import numpy as np

from tests import logistic_restatement as R


def data(n, p, m, seed, k=5):
    """tests/test_gpu_logistic._data's x; response r draws from its own beta (scaled by 0.3 .. 2.5) and intercept (-1 .. 1)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, p)) * rng.uniform(0.5, 2.0, size=p) + rng.normal(size=p) * 0.2
    Y = np.zeros((n, m))
    for r in range(m):
        b = np.zeros(p)
        b[:k] = rng.uniform(-1.0, 1.0, k) * (0.3 + 2.2 * r / max(m - 1, 1))
        off = -1.0 + 2.0 * ((3 * r) % m) / max(m - 1, 1)
        prob = 1.0 / (1.0 + np.exp(-(x @ b + off)))
        Y[:, r] = (rng.uniform(size=n) < prob).astype(np.float64)
    return np.asfortranarray(x), Y


def fit_multi(x, Y, penalty=("lasso",), lambda_=None, nlambda=100, lambda_min_ratio=1e-4, alpha=1.0, gamma=3.0, tau=0.5,
              groups=None, unique_groups=None, group_weights=None, penalty_factor=None, standardize=True, intercept=True,
              compute_loss=False, maxit=500, tol=1e-7, irls_maxit=100, irls_tol=1e-3, stats=None):
    """Returns a list of m dicts, each as logistic_restatement.fit returns it."""
    x = np.asarray(x, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    n, p = x.shape
    m = Y.shape[1]
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
    provided = lambda_ is not None and len(lambda_) > 0
    nl = len(lambda_[0]) if provided else nlambda
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
    st = stats if stats is not None else {}
    for key in ("steps", "rows", "grams"):
        st.setdefault(key, 0)
    # ---- once per call: the Hessian at beta = 0 (every W is 0.25, no y in it), d, A
    prob0 = 1.0 / (1.0 + np.exp(-np.zeros(n)))
    W = prob0 * (1.0 - prob0)
    sw = np.sqrt(W)
    Z = sw[:, None] * (x * s)
    if intercept:
        Z = np.column_stack([sw, Z])
    XX = (Z.T @ Z) / n
    d = float(np.linalg.eigvalsh(XX)[-1]) * 1.0005
    A = -XX
    A[np.diag_indices(q)] += d
    st["grams"] += 1
    # ---- per response: XY = s o X'Y / n, its own base grid
    base = []
    for r in range(m):
        y = Y[:, r]
        xy0 = np.zeros(q)
        xy0[o:] = ((x.T @ y) * s) / n
        if intercept:
            xy0[0] = y.sum() / n
        lmax = float(np.max(np.abs(xy0[o:])))
        base.append(None if provided else R.lambda_grid(lmax, nlambda, lambda_min_ratio))
    outs = [dict(beta=[], **{"lambda": []}, niter=[], loss=[], d=d) for _ in range(m)]
    for k, pen in enumerate(penalty):
        lams = []
        for r in range(m):
            if provided:
                lam = np.asarray(lambda_[k], dtype=np.float64)
            else:
                lam = base[r].copy()
                if pen.endswith(".net"):
                    lam = base[r] / alpha
                    if "mcp" in pen or "scad" in pen:
                        fact = 3.5 - min(3.5, gamma) * 5.71425 / 8.0
                        lam = fact * base[r] / alpha ** 0.8
            lams.append(lam)
        nlk = 1 if pen == "ols" else nl
        B = [np.zeros((p + 1, nl)) for _ in range(m)]
        NI = [np.zeros(nl, dtype=np.int32) for _ in range(m)]
        LO = [np.full(nl, 1e99) for _ in range(m)]
        beta = [np.zeros(q) for _ in range(m)]
        XY = [None] * m
        prob = [None] * m
        for li in range(nlk):
            live = [True] * m
            nit = [irls_maxit + 1] * m
            i = 0
            while i < irls_maxit and any(live):
                beta_irls = [b.copy() for b in beta]
                if not (i == 0 and li > 0):
                    st["rows"] += 1
                    for r in range(m):
                        if not live[r]:
                            continue
                        y = Y[:, r]
                        eta = x @ (beta[r][o:] * s) + (beta[r][0] if intercept else 0.0)
                        prob[r] = 1.0 / (1.0 + np.exp(-eta))
                        rr = y - prob[r]
                        grad = np.zeros(q)
                        grad[o:] = ((x.T @ rr) / n) * s
                        if intercept:
                            grad[0] = rr.sum() / n
                        XY[r] = XX @ beta[r] + grad
                for r in range(m):
                    if not live[r]:
                        continue
                    for j in range(maxit):
                        bp = beta[r]
                        u = A @ bp + XY[r]
                        beta[r] = R.next_beta(pen, u, lams[r][li], d, pf, alpha, gamma, tau, grp)
                        if R.stop_rule(beta[r], bp, tol):
                            break
                st["steps"] += 1
                for r in range(m):
                    if live[r] and R.stop_rule(beta[r], beta_irls[r], irls_tol):
                        live[r] = False                          # frozen for the rest of this lambda
                        nit[r] = i + 1
                i += 1
            for r in range(m):
                NI[r][li] = nit[r]
                if compute_loss:
                    LO[r][li] = R._loss(Y[:, r], prob[r])
                B[r][0, li] = beta[r][0] if intercept else 0.0
                B[r][1:, li] = beta[r][o:] * s
        for r in range(m):
            if pen == "ols":
                outs[r]["beta"].append(B[r][:, :1]); outs[r]["niter"].append(int(NI[r][0])); outs[r]["loss"].append(float(LO[r][0]))
            else:
                outs[r]["beta"].append(B[r]); outs[r]["niter"].append(NI[r]); outs[r]["loss"].append(LO[r])
            outs[r]["lambda"].append(np.asarray(lams[r], dtype=np.float64))
    return outs
