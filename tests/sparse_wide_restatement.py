"""A scipy / numpy restatement of oem() on a sparse x with nobs <= nvars and no intercept (ref src/oem_sparse.h:607-612, 638-647,
932-941; src/oem_big.h:537-541, 568-584, 743-764, 880-897), with its two products in the orders of the kernels of
oem_amd/csrc/sparse_wide.hip: X beta over the compressed ROWS (every row's entries in column order), X't over the compressed COLUMNS
(every column's entries in row order).  Nothing of n p entries is formed, so it also serves where the oracle's dense n x n eigen-solve
cannot run (n > 8192).

    u = X'(y - X beta) / n + d beta,   d = 1.005 lambda_max(X X'/n),   the data as they are;
    with standardize only lambda_zero (max |x_j'y| colsq_inv_j / n) and the returned coefficients (beta colsq_inv) carry the scales.

lasso, elastic.net and mcp.  Not a test module (no test_ prefix): tests/test_sparse_wide_cpu.py holds it against the oracle on every
input of the GPU parity test, tests/test_gpu_sparse_wide.py holds the GPU fit to it past the oracle's row limit.

Also here, shared by both files: the shapes and seeds of the GPU parity test and the generator of its inputs."""
import numpy as np
import scipy.sparse as sp

PARITY_SHAPES = [(40, 1100, 0.02), (64, 3000, 0.01), (200, 5000, 0.01), (300, 9000, 0.005)]      # (n, p, density)
PARITY_KW = dict(nlambda=5, lambda_min_ratio=0.05, tol=1e-9, maxit=400)


def parity_seed(n, p):
    return n + p


def parity_data(n, p, dens, seed=None):
    """a CSC matrix of about dens n p normal entries with column scales in [0.5, 3], an empty column (colsq falls back to 1) and
    y = X b + noise with six non-zero coefficients on well-filled columns; the structure is exactly 2 % / 1 % / .. or just below"""
    rng = np.random.default_rng(parity_seed(n, p) if seed is None else seed)
    nnz = int(dens * n * p)                                        # never above the route's 2 %
    flat = rng.choice(n * p, size=nnz, replace=False)
    rows, cols = flat % n, flat // n
    keep = cols != 5                                                # (a column of zeros)
    rows, cols = rows[keep], cols[keep]
    vals = rng.normal(size=rows.shape[0]) * rng.uniform(0.5, 3.0, p)[cols]
    x = sp.csc_matrix((vals, (rows, cols)), shape=(n, p))
    x.sum_duplicates(); x.sort_indices()
    fill = np.diff(x.indptr)
    top = np.argsort(-fill, kind="stable")[:6]
    b = np.zeros(p); b[top] = rng.uniform(1, 2, 6)
    y = x @ b + 0.5 * rng.normal(size=n)
    return x, y


def _stop(cur, prev, tol):
    c, q = np.abs(cur), np.abs(prev)
    if np.any((c > 1e-13) != (q > 1e-13)):
        return False
    both = (c > 1e-13) & (q > 1e-13)
    return not np.any(np.abs((cur[both] - prev[both]) / prev[both]) > tol)


def _soft(u, tp, d):
    return np.where(u > tp, (u - tp) / d, np.where(u < -tp, (u + tp) / d, 0.0))


def _mcp(u, tp, d, gamma):
    inner = np.where(u > tp, (u - tp) / (d - 1.0 / gamma), np.where(u < -tp, (u + tp) / (d - 1.0 / gamma), 0.0))
    return np.where(np.abs(u) > gamma * d * tp, u / d, inner)


def lambda_grid(lmax, nl, ratio):
    lo, hi = np.log(lmax), np.log(ratio * lmax)
    if nl == 1:
        return np.exp(np.array([hi]))
    step = (hi - lo) / (nl - 1)
    k = np.arange(nl, dtype=np.float64)
    if abs(hi) < abs(lo):
        v = hi - (nl - 1 - k) * step; v[0] = lo
    else:
        v = lo + k * step; v[-1] = hi
    return np.exp(v)


def d_of(x):
    """1.005 lambda_max(X X'/n) through the operator alone (ARPACK on n-vectors)"""
    from scipy.sparse.linalg import LinearOperator, eigsh
    xr, xc = sp.csr_matrix(x), sp.csc_matrix(x)
    n = x.shape[0]
    op = LinearOperator((n, n), matvec=lambda v: (xr @ (xc.T @ v)) / n, dtype=np.float64)
    if n <= 3:
        return 1.005 * float(np.linalg.eigvalsh((xr @ xr.T).toarray() / n)[-1])
    return 1.005 * float(eigsh(op, k=1, which="LA", tol=1e-13, ncv=min(n - 1, 64))[0][0])


def fit(x, y, penalty, standardize=True, nlambda=5, lambda_min_ratio=0.05, tol=1e-9, maxit=400, alpha=1.0, gamma=3.0,
        compute_loss=False, d_override=0.0):
    """the oracle's result layout: beta[k] (p + 1) x nlambda with row 0 the absent intercept, lambda[k], niter[k], loss[k], d"""
    penalty = [penalty] if isinstance(penalty, str) else list(penalty)
    xc = sp.csc_matrix(x, dtype=np.float64); xc.sum_duplicates(); xc.sort_indices()
    xr = sp.csr_matrix(xc); xr.sort_indices()                      # rows in column order
    xct = xc.T                                                      # CSR of X': the columns of X, each in row order
    n, p = xc.shape
    y = np.asarray(y, dtype=np.float64)
    ss = np.asarray(xc.multiply(xc).sum(axis=0)).ravel()
    cs = ss / (n - 1.0); cs[cs == 0.0] = 1.0
    inv = 1.0 / np.sqrt(cs) if standardize else np.ones(p)
    xy = (xct @ y) / n
    lmax = np.abs(xy * inv).max()
    d = d_override if d_override > 0 else d_of(xc)
    out = {"beta": [], "lambda": [], "niter": [], "loss": [], "d": d, "penalty": penalty}
    for pen in penalty:
        if pen not in ("lasso", "elastic.net", "mcp"):
            raise ValueError("the restatement covers lasso, elastic.net and mcp")
        lam = lambda_grid(lmax, nlambda, lambda_min_ratio)
        if pen == "elastic.net":
            lam = lam / alpha
        B = np.zeros((p + 1, nlambda)); nit = np.zeros(nlambda, dtype=np.int64); loss = np.full(nlambda, 1e99)
        beta = np.zeros(p)
        for i, l in enumerate(lam):
            it = 0
            for it in range(maxit):
                prev = beta
                t = xr @ prev                                       # row pass
                g = (xct @ t) * (1.0 / n)                           # column pass
                u = d * prev - g + xy
                if pen == "lasso":
                    beta = _soft(u, l, d)
                elif pen == "elastic.net":
                    beta = _soft(u, l * alpha, d + (1.0 - alpha) * l)
                else:
                    beta = _mcp(u, l, d, gamma)
                if _stop(beta, prev, tol):
                    break
            else:
                it = maxit                                          # (the loop ran out: maxit + 1, as the reference counts)
            nit[i] = it + 1
            B[1:, i] = beta * inv
            if compute_loss:
                r = y - xr @ B[1:, i]
                loss[i] = float(r @ r)
        out["beta"].append(B); out["lambda"].append(lam); out["niter"].append(nit); out["loss"].append(loss)
    return out
