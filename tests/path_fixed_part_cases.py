"""Inputs of the recorded row-split path cases (tests/test_gpu_path_recorded.py, tools/record_path_outputs.py).

Every case is built from a fixed seed, so the fixtures under tests/golden/path_fixed_part/ hold outputs only: what the path kernel
gave at the commit that recorded them, and what the CPU oracle gives for the same call."""
import numpy as np


def problem(n, p, seed, nnz=None, sd=2.0, coef=(0.4, 1.6), dup=()):
    """x ~ N(0, sd^2), `nnz` true coefficients scattered over the columns (default p // 4), unit noise; dup: (to, from) column copies"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, p)) * sd
    for to, frm in dup:
        x[:, to] = x[:, frm]
    nnz = max(1, p // 4) if nnz is None else nnz
    b = np.zeros(p)
    b[rng.choice(p, nnz, replace=False)] = rng.uniform(coef[0], coef[1], nnz) * rng.choice([-1.0, 1.0], nnz)
    y = x @ b + rng.normal(size=n) + 0.3
    return np.asfortranarray(x), y


def lambda_max(x, y):
    """max |x_c' y_c| / n: the top of the grid of a fit with intercept and without standardisation"""
    n = x.shape[0]
    return float(np.abs((x - x.mean(axis=0)).T @ (y - y.mean())).max() / n)


def user_lambdas(x, y, nl, above=2, ratio=1e-2):
    """a decreasing sequence whose first `above` values lie over lambda_max (beta = 0 there)"""
    lm = lambda_max(x, y)
    head = lm * np.linspace(1.6, 1.1, above)
    tail = lm * np.exp(np.linspace(np.log(0.9), np.log(ratio), nl - above))
    return np.concatenate([head, tail])


def path_cost_problem(p=100, n=20000):
    """the problem of tools/path_cost.py and tools/path_round_segments.py"""
    rng = np.random.default_rng(123)
    b = np.concatenate([rng.uniform(size=p // 4), np.zeros(p - p // 4)])
    x = np.asfortranarray(rng.normal(size=(n, p)) * 3.0)
    y = x @ b + rng.normal(size=n)
    return x, y


def case(name):
    """(x, y, keyword arguments of oem() / the oracle's fit_dense)"""
    if name == "c1_p100_100lambda":
        x, y = path_cost_problem()
        return x, y, dict(penalty=["elastic.net"], intercept=True, standardize=False, nlambda=100, tol=1e-10)
    if name == "p8_lasso":
        x, y = problem(600, 8, 1, nnz=3)
        return x, y, dict(penalty=["lasso"], nlambda=10, tol=1e-9)
    if name == "p33_net_ridge_cap5":
        x, y = problem(600, 33, 2)
        return x, y, dict(penalty=["elastic.net"], alpha=0.5, nlambda=8, tol=1e-300, maxit=5)
    if name == "p100_lasso_cap3":
        x, y = problem(600, 100, 3)
        return x, y, dict(penalty=["lasso"], nlambda=12, tol=1e-300, maxit=3)
    if name == "p100_user_lambda_above_max":
        x, y = problem(600, 100, 4)
        return x, y, dict(penalty=["lasso"], standardize=False, lambda_=user_lambdas(x, y, 12), tol=1e-9)
    if name == "p100_short_to_full":
        x, y = problem(600, 100, 5, nnz=60, coef=(0.2, 2.0))
        return x, y, dict(penalty=["lasso"], nlambda=20, lambda_min_ratio=1e-3, tol=1e-10)
    if name == "p104_mcp":
        x, y = problem(600, 104, 6)
        return x, y, dict(penalty=["mcp"], gamma=3.0, nlambda=10, tol=1e-9)
    if name == "p105_scad":
        x, y = problem(600, 105, 7)
        return x, y, dict(penalty=["scad"], gamma=3.7, nlambda=10, tol=1e-9)
    if name == "p130_grp_lasso":
        x, y = problem(600, 130, 8)
        g = np.arange(130) // 5 + 1
        return x, y, dict(penalty=["grp.lasso"], groups=g, unique_groups=np.unique(g), nlambda=8, tol=1e-9)
    if name == "p177_lasso_accelerate":
        x, y = problem(600, 177, 9)
        return x, y, dict(penalty=["lasso"], accelerate=True, nlambda=10, tol=1e-9)
    if name == "p200_mcp_scad":
        x, y = problem(600, 200, 10)
        return x, y, dict(penalty=["mcp", "scad"], gamma=3.7, nlambda=10, tol=1e-9)
    if name == "p100_ols":
        x, y = problem(600, 100, 11)
        return x, y, dict(penalty=["ols"], tol=1e-9)
    if name == "p2_lasso":
        x, y = problem(600, 2, 12, nnz=1)
        return x, y, dict(penalty=["lasso"], nlambda=5, tol=1e-9)
    if name == "p40_duplicated_columns":
        x, y = problem(600, 40, 13, dup=[(k, k % 3) for k in range(3, 40)])
        return x, y, dict(penalty=["lasso"], nlambda=6, tol=1e-9)
    raise KeyError(name)


RECORDED = ["c1_p100_100lambda", "p8_lasso", "p33_net_ridge_cap5", "p100_lasso_cap3", "p100_user_lambda_above_max",
            "p100_short_to_full", "p104_mcp", "p105_scad", "p130_grp_lasso", "p177_lasso_accelerate", "p200_mcp_scad", "p100_ols",
            "p2_lasso", "p40_duplicated_columns"]


def device_kw(kw):
    """the same call for oem_amd.oem (which derives unique_groups itself)"""
    return {k: v for k, v in kw.items() if k != "unique_groups"}


def run_device(oa, name):
    """the case on the GPU, x resident on the device: (fit, Lanczos steps, cap reached)"""
    import ctypes as C
    import torch
    from oem_amd import _lib as L
    x, y, kw = case(name)
    xd = torch.as_tensor(np.ascontiguousarray(x.T), device="cuda").t()
    fit = oa.oem(xd, y, **device_kw(kw))
    steps, capped = C.c_int32(-1), C.c_int32(-1)
    assert L.lib().oemgpu_last_eigen_info(oa.context(), C.byref(steps), C.byref(capped)) == 0
    return fit, int(steps.value), int(capped.value)


def flat(fit, key):
    """one array over the penalties of a call"""
    return np.concatenate([np.ravel(np.asarray(v, dtype=np.float64)) for v in fit[key]])
