"""A scipy / numpy restatement of cv.oem's fold fit on a sparse x with nobs <= nvars and no intercept, as
oemgpu_fit_sparse_wide_fold_res computes it (oem_amd/csrc/sparse_wide.hip with MASK; ref R/cv_oem.R:155-175 calls oem() on
x[!which, ], which reaches src/oem_sparse.h:607-612, 638-647, 932-941): tests/sparse_wide_restatement.py's iteration on the WHOLE
matrix with a row mask, and the kept-row count n_k wherever n enters.

    t = keep * (X beta)                  the row pass: a left-out row is not read, its t an exact 0
    g = X't / n_k                        the column pass, not masked: t is 0 in the left-out rows
    xy = X'(keep ? y : 0) / n_k          a select: y of a left-out row is never read (it may be NaN)
    colsq_j = sum over the kept rows of x_ij^2 / (n_k - 1), a column the fold empties -> 1
    d = 1.005 lambda_max(keep X X' keep / n_k), through the operator on n-vectors that are 0 in the left-out rows
    the lambda grid from the masked xy; the loss over the kept rows

Nothing is sliced.  Not a test module (no test_ prefix): tests/test_cv_sparse_wide_cpu.py holds it against the sliced restatement and
the oracle on every input of the GPU parity test of tests/test_gpu_cv_sparse_wide.py.

Also here, shared by both files: the shapes, seeds and fold ids of that parity test."""
import numpy as np
import scipy.sparse as sp

from tests import sparse_wide_restatement as R

# (n, p, density, folds): 63 / 64 / 65 rows (a wave of lanes) and the parity shape the library routes here by itself
PARITY_CASES = [(63, 300, 0.06, 3), (64, 300, 0.06, 3), (65, 300, 0.06, 3), (40, 1100, 0.02, 3)]
PARITY_KW = dict(nlambda=5, lambda_min_ratio=0.05, tol=1e-9, maxit=400)


def parity_input(n, p, dens, K):
    """(x, y, foldid) of a parity case: sparse_wide_restatement.parity_data and fold ids 1..K in a seeded order"""
    x, y = R.parity_data(n, p, dens)
    foldid = np.random.default_rng(7 * n + p).permutation(np.resize(np.arange(1, K + 1), n))
    return x, y, foldid


def d_of(x, keep):
    """1.005 lambda_max(keep X X' keep / n_k) through the masked operator alone (ARPACK on n-vectors)"""
    from scipy.sparse.linalg import LinearOperator, eigsh
    xr, xc = sp.csr_matrix(x), sp.csc_matrix(x)
    n = x.shape[0]
    m = np.asarray(keep, dtype=np.float64)
    nk = int(m.sum())
    mv = lambda v: m * (xr @ (xc.T @ (m * np.ravel(v)))) / nk
    if n <= 3:
        return 1.005 * float(np.linalg.eigvalsh(np.column_stack([mv(e) for e in np.eye(n)]))[-1])
    op = LinearOperator((n, n), matvec=mv, dtype=np.float64)
    v0 = m / np.sqrt(nk)                                            # a start vector in the kept rows' subspace
    return 1.005 * float(eigsh(op, k=1, which="LA", tol=1e-13, ncv=min(n - 1, 64), v0=v0)[0][0])


def fit(x, y, keep, penalty, standardize=True, nlambda=5, lambda_min_ratio=0.05, tol=1e-9, maxit=400, alpha=1.0, gamma=3.0,
        compute_loss=False, d_override=0.0):
    """the result layout of sparse_wide_restatement.fit, plus "kept" = n_k.  keep: n booleans, the rows with foldid != leave_out"""
    penalty = [penalty] if isinstance(penalty, str) else list(penalty)
    xc = sp.csc_matrix(x, dtype=np.float64); xc.sum_duplicates(); xc.sort_indices()
    xr = sp.csr_matrix(xc); xr.sort_indices()
    xct = xc.T
    n, p = xc.shape
    keep = np.asarray(keep, dtype=bool)
    m = keep.astype(np.float64)
    nk = int(keep.sum())
    ysel = np.where(keep, np.asarray(y, dtype=np.float64), 0.0)     # (a select, not a product: NaN in a left-out row stays out)
    ss = np.asarray(xc.multiply(xc).T @ m).ravel()
    cs = ss / (nk - 1.0); cs[cs == 0.0] = 1.0
    inv = 1.0 / np.sqrt(cs) if standardize else np.ones(p)
    xy = (xct @ ysel) / nk
    lmax = np.abs(xy * inv).max()
    d = d_override if d_override > 0 else d_of(xc, keep)
    out = {"beta": [], "lambda": [], "niter": [], "loss": [], "d": d, "penalty": penalty, "kept": nk}
    for pen in penalty:
        if pen not in ("lasso", "elastic.net", "mcp"):
            raise ValueError("the restatement covers lasso, elastic.net and mcp")
        lam = R.lambda_grid(lmax, nlambda, lambda_min_ratio)
        if pen == "elastic.net":
            lam = lam / alpha
        B = np.zeros((p + 1, nlambda)); nit = np.zeros(nlambda, dtype=np.int64); loss = np.full(nlambda, 1e99)
        beta = np.zeros(p)
        for i, l in enumerate(lam):
            it = 0
            for it in range(maxit):
                prev = beta
                t = m * (xr @ prev)                                 # masked row pass
                g = (xct @ t) * (1.0 / nk)                          # column pass, unmasked
                u = d * prev - g + xy
                if pen == "lasso":
                    beta = R._soft(u, l, d)
                elif pen == "elastic.net":
                    beta = R._soft(u, l * alpha, d + (1.0 - alpha) * l)
                else:
                    beta = R._mcp(u, l, d, gamma)
                if R._stop(beta, prev, tol):
                    break
            else:
                it = maxit
            nit[i] = it + 1
            B[1:, i] = beta * inv
            if compute_loss:
                r = ysel - m * (xr @ B[1:, i])
                loss[i] = float(r @ r)
        out["beta"].append(B); out["lambda"].append(lam); out["niter"].append(nit); out["loss"].append(loss)
    return out
