"""Which region of its penalty operator every (coefficient, lambda) pair of a fitted path lies in, and how far from the nearest region
boundary.  TEST INFRASTRUCTURE, numpy only.

A test of a thresholding kernel on random data shows something about a branch of the operator only if some coefficient landed in that
branch -- and far enough from its edges that rounding on the device cannot have moved it into the neighbouring one.  census() answers both
for a Gram-form problem (xtx, xty, d) and a path fitted on it: it recomputes the operator's argument

    u = xty + (d I - xtx) beta                                              (ref src/oem_dense.h:512)

per lambda and classifies every pair with plain branches written from the operator DEFINITIONS (ref src/oem_dense.h:76-315, dispatch
:527-628), not from the device code or the oracle's.

Per-lambda constants, L the threshold multiplying penalty_factor / the group weight, D the denominator:

    lasso, mcp, scad, grp.lasso, grp.mcp, grp.scad     L = lambda                  D = d
    every .net penalty                                 L = alpha lambda            D = d + (1 - alpha) lambda
    scad.net at alpha == 0                             L = 0                       D = d + lambda
    sparse.grp.lasso                                   L = (1 - tau) lambda        D = d       L1 = tau lambda (inner soft threshold)

Regions (t = penalty_factor L for the element-wise operators, t = group_weight L and |u| = the group's norm s for the group factors):

    soft (lasso, elastic.net)   zero    |u| <= t                          shrunk  otherwise
    mcp(.net)                   zero    |u| <= t                          shrunk  t < |u| <= gamma D t   (denominator D - 1/gamma)
                                big     |u| > gamma D t
    scad(.net)                  zero    |u| <= t                          soft    t < |u| <= (D + 1) t
                                mid     (D + 1) t < |u| <= gamma D t      (denominator (gamma - 1) D - 1)
                                big     |u| > gamma D t
    grp.lasso(.net)             zero    s <= t                            shrunk  otherwise
    grp.mcp(.net)               zero, shrunk, one (f = 1) at the mcp bounds on s
    grp.scad(.net)              zero, soft, mid, one (f = 1) at the scad bounds on s
    sparse.grp.lasso            with v = soft(u, penalty_factor L1) and s = |v_g|:
                                inner_zero  s == 0: every member zeroed by the inner threshold
                                norm_zero   0 < s <= t: the group zeroed by its norm
                                alive_zero  s > t, this member zeroed by the inner threshold
                                alive       s > t, this member alive
    any group penalty           free    a member of the unpenalised group 0 (f = 1 whatever the norm); under the sparse group lasso
                                        the inner threshold still applies to it: free_zero where it zeroes the member (margin: the
                                        inner threshold's)

The margin of a pair is the relative distance |a - b| / max(a, b) of its |u| (or s) to the nearest boundary b of its operator (1 where
every boundary is 0); for the sparse group lasso the smaller of the group's margin and the inner threshold's margins that the pair's
region depends on."""
import numpy as np

NET = ("elastic.net", "mcp.net", "scad.net", "grp.lasso.net", "grp.mcp.net", "grp.scad.net")
KIND = {"lasso": "soft", "elastic.net": "soft", "mcp": "mcp", "mcp.net": "mcp", "scad": "scad", "scad.net": "scad",
        "grp.lasso": "grp.soft", "grp.lasso.net": "grp.soft", "grp.mcp": "grp.mcp", "grp.mcp.net": "grp.mcp",
        "grp.scad": "grp.scad", "grp.scad.net": "grp.scad", "sparse.grp.lasso": "sgl"}
REGIONS = {"soft": ("zero", "shrunk"), "mcp": ("zero", "shrunk", "big"), "scad": ("zero", "soft", "mid", "big"),
           "grp.soft": ("zero", "shrunk", "free"), "grp.mcp": ("zero", "shrunk", "one", "free"),
           "grp.scad": ("zero", "soft", "mid", "one", "free"), "sgl": ("inner_zero", "norm_zero", "alive_zero", "alive", "free", "free_zero")}


def constants(penalty, lam, d, alpha=1.0, tau=0.5):
    """(L, D, L1) of one lambda"""
    if penalty == "sparse.grp.lasso":
        return (1.0 - tau) * lam, d, tau * lam
    if penalty in NET:
        if penalty == "scad.net" and alpha == 0:
            return 0.0, d + lam, 0.0
        return alpha * lam, d + (1.0 - alpha) * lam, 0.0
    return lam, d, 0.0


def _rel(a, b):
    """|a - b| / max(a, b) for a, b >= 0; 1 where both are 0 (no boundary to cross)"""
    m = max(a, b)
    return abs(a - b) / m if m > 0 else 1.0


def _classify(kind, a, t, D, gamma):
    """(region, margin) of a magnitude a >= 0 under an operator of the family `kind` with threshold t"""
    if kind == "soft":
        bounds = [t]
        region = "zero" if a <= t else "shrunk"
    elif kind == "mcp":
        bounds = [t, gamma * D * t]
        if a > gamma * D * t:
            region = "big"
        elif a > t:
            region = "shrunk"
        else:
            region = "zero"
    else:
        bounds = [t, (D + 1.0) * t, gamma * D * t]
        if a > gamma * D * t:
            region = "big"
        elif a > (D + 1.0) * t:
            region = "mid" if (gamma - 1.0) * a > gamma * t else "mid_zero"
        elif a > t:
            region = "soft"
        else:
            region = "zero"
    return region, min(_rel(a, b) for b in bounds)


def census(penalty, xtx, xty, d, beta, lam, alpha=1.0, gamma=3.0, tau=0.5, penalty_factor=None, groups=None, unique_groups=None,
           group_weights=None):
    """beta: p x nlambda, the path in the coordinates of (xtx, xty); lam: the nlambda values the iteration ran with.
    Returns (region, margin): p x nlambda arrays of region names and relative margins."""
    xtx, xty, beta = np.asarray(xtx, dtype=np.float64), np.asarray(xty, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    p, nl = beta.shape
    pf = np.ones(p) if penalty_factor is None else np.asarray(penalty_factor, dtype=np.float64)
    kind = KIND[penalty]
    region = np.empty((p, nl), dtype=object)
    margin = np.zeros((p, nl))
    if kind.startswith("grp") or kind == "sgl":
        groups = np.asarray(groups)
        ug = np.unique(groups) if unique_groups is None else np.asarray(unique_groups)
        members = [np.flatnonzero(groups == g) for g in ug]
        gw = np.sqrt([float(len(m)) for m in members]) if group_weights is None else np.asarray(group_weights, dtype=np.float64)
    U = xty[:, None] + d * beta - xtx @ beta
    for l in range(nl):
        u = U[:, l]
        L, D, L1 = constants(penalty, float(lam[l]), d, alpha, tau)
        if kind in ("soft", "mcp", "scad"):
            for j in range(p):
                region[j, l], margin[j, l] = _classify(kind, abs(u[j]), pf[j] * L, D, gamma)
            continue
        for g, m, w in zip(ug, members, gw):
            if g == 0 and kind != "sgl":
                region[m, l], margin[m, l] = "free", 1.0
                continue
            if kind != "sgl":
                s = float(np.sqrt(np.sum(u[m] ** 2)))
                r, mg = _classify({"grp.soft": "soft", "grp.mcp": "mcp", "grp.scad": "scad"}[kind], s, w * L, D, gamma)
                region[m, l], margin[m, l] = {"big": "one"}.get(r, r), mg
                continue
            t1 = pf[m] * L1
            v = np.sign(u[m]) * np.maximum(np.abs(u[m]) - t1, 0.0)
            inner = np.array([_rel(abs(a), b) for a, b in zip(u[m], t1)])
            s = float(np.sqrt(np.sum(v ** 2)))
            if g == 0:                                    # f = 1, but the inner soft threshold has been applied (ref src/oem_dense.h:619)
                region[m, l], margin[m, l] = np.where(v != 0, "free", "free_zero"), inner
            elif s == 0.0:
                region[m, l], margin[m, l] = "inner_zero", inner.min()
            elif s <= w * L:
                region[m, l], margin[m, l] = "norm_zero", _rel(s, w * L)
            else:
                for i, j in enumerate(m):
                    region[j, l] = "alive" if v[i] != 0 else "alive_zero"
                    margin[j, l] = min(_rel(s, w * L), inner[i])
    return region, margin


def counts(region, margin, min_margin=1e-6):
    """{region name: number of (coefficient, lambda) pairs in it whose margin is at least min_margin}"""
    out = {}
    for r in np.unique(region.astype(str)):
        out[r] = int(np.sum((region == r) & (margin >= min_margin)))
    return out
