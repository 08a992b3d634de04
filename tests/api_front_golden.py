"""The cases behind tests/golden/api_front.json: what the entries of oem_amd/api.py refuse, the option blocks they build and the bytes
they return, recorded BEFORE their option prologues, cross-validation fronts and tails became one helper each.
tests/test_api_front_cpu.py and tests/test_gpu_api_front_bytes.py hold today's entries to the file.  Three sections:

    refusals     an entry called on host arrays with one invalid argument, or with two at once (the order of the checks):
                 [type(exc).__name__, str(exc)].  Every one is raised before a device or the library is looked for; a case that gets
                 as far as either is not written.
    options      api._Args replaced by a subclass that records its constructor arguments and stops the call: the option block of a grid
                 of valid option sets, with the warnings given on the way.  "options" holds the entries that take host arrays,
                 "options_gpu" those that demand a device tensor first.
    bytes_gpu    SHA-256 of everything in the result of one small seeded call per entry.

    python -m tests.api_front_golden OUT.json           (without a GPU: refusals and options)
    python -m tests.api_front_golden OUT.json gpu       (on a GPU: adds options_gpu and bytes_gpu to what OUT.json holds)
"""
import hashlib
import inspect
import json
import sys
import warnings

import numpy as np

N, P, M = 40, 5, 3


# ------------------------------------------------------------------------------------------ the entries and their inputs
def _host_inputs():
    rng = np.random.default_rng(20261)
    x = rng.normal(size=(N, P))
    Y = rng.normal(size=(N, M))
    return x, Y, (Y > 0).astype(np.float64)


def _entries(api):
    """name -> (callable, positional arguments on host arrays, binomial, fixed keyword arguments)"""
    import scipy.sparse as sp
    x, Y, Yb = _host_inputs()
    fold = np.resize(np.arange(1, 5), N)
    xtx, xty = x.T @ x, x.T @ Y[:, 0]
    return {
        "oem": (api.oem, dict(x=x, y=Y[:, 0]), False, {}),
        "oem_sparse": (api.oem, dict(x=sp.csc_matrix(x), y=Y[:, 0]), False, {}),
        "oem_multi": (api.oem_multi, dict(x=x, Y=Y), False, {}),
        "oem_fit_logistic_dense": (api.oem_fit_logistic_dense, dict(x=x, y=Yb[:, 0]), True, {}),
        "oem_fit_logistic_dense_multi": (api.oem_fit_logistic_dense_multi, dict(x=x, Y=Yb), True, {}),
        "oem_fit_logistic_dense_multi_folds": (api.oem_fit_logistic_dense_multi_folds, dict(x=x, Y=Yb, foldid=fold), True, {}),
        "oem_fit_logistic_sparse": (api.oem_fit_logistic_sparse, dict(x=sp.csc_matrix(x), y=Yb[:, 0]), True, {}),
        "oem_xtx": (api.oem_xtx, dict(xtx=xtx, xty=xty), False, {}),
        "big_oem": (api.big_oem, dict(x=x, y=Y[:, 0]), False, dict(penalty=["lasso"])),      # (its default is all fourteen: groups needed)
        "xval_oem": (api.xval_oem, dict(x=x, y=Y[:, 0]), False, {}),
        "xval_oem_multi": (api.xval_oem_multi, dict(x=x, Y=Y), False, {}),
        "cv_oem_gaussian": (api.cv_oem, dict(x=x, y=Y[:, 0]), False, {}),
        "cv_oem_binomial": (api.cv_oem, dict(x=x, y=Yb[:, 0]), True, dict(family="binomial")),
        "cv_oem_multi": (api.cv_oem_multi, dict(x=x, Y=Y), False, {}),
        "cv_oem_logistic_multi": (api.cv_oem_logistic_multi, dict(x=x, Y=Yb), True, {}),
    }


_XNAME = {"oem_xtx": "xtx"}
_YNAME = {"oem_xtx": "xty"}
_CV = ("cv_oem_gaussian", "cv_oem_binomial", "cv_oem_multi", "cv_oem_logistic_multi")
_FOLDS = _CV + ("xval_oem", "xval_oem_multi")
_BINOMIAL = ("oem_fit_logistic_dense", "oem_fit_logistic_dense_multi", "oem_fit_logistic_dense_multi_folds", "oem_fit_logistic_sparse",
             "cv_oem_binomial", "cv_oem_logistic_multi")
_MANY = ("oem_multi", "oem_fit_logistic_dense_multi", "oem_fit_logistic_dense_multi_folds", "xval_oem_multi", "cv_oem_multi",
         "cv_oem_logistic_multi")
_ALL = None


def _yname(entry):
    return _YNAME.get(entry, "Y" if entry in _MANY else "y")


def _one_column(entry, a):
    k = _XNAME.get(entry, "x")
    return {k: a[k][:1, :1] if entry == "oem_xtx" else a[k][:, :1]}


def _short_y(entry, a):
    k = _yname(entry)
    return {k: a[k][:-1]}


def _three_values(entry, a):
    k = _yname(entry)
    y = np.array(a[k], copy=True)
    y[:3] = 2.0
    return {k: y}


_GROUPS = np.array([1, 1, 2, 2, 3])

# the faults in the order of the issue's list: (name, entries that take it or None for all, the arguments it changes)
FAULTS = [
    ("penalty", _ALL, lambda e, a: dict(penalty="nope")),
    ("hessian_type", _BINOMIAL, lambda e, a: dict(hessian_type="nope")),
    ("family", ("oem", "oem_sparse", "oem_multi", "oem_xtx", "big_oem", "xval_oem", "xval_oem_multi", "cv_oem_gaussian", "cv_oem_multi"),
     lambda e, a: dict(family="binomial" if e in ("oem_xtx", "big_oem") else "poisson")),
    ("type_measure", _FOLDS, lambda e, a: dict(type_measure="rmse")),
    ("one_column", _ALL, _one_column),
    ("short_y", _ALL, _short_y),
    ("three_values", _BINOMIAL, _three_values),
    ("penalty_factor", _ALL, lambda e, a: dict(penalty_factor=np.ones(P + 1))),
    ("groups", _ALL, lambda e, a: dict(penalty=["grp.lasso"], groups=_GROUPS[:-1])),
    ("group_weights", _ALL, lambda e, a: dict(penalty=["grp.lasso"], groups=_GROUPS, group_weights=np.ones(7))),
    ("lambda_min_ratio_0", _ALL, lambda e, a: dict(lambda_min_ratio=0.0)),
    ("lambda_min_ratio_1", _ALL, lambda e, a: dict(lambda_min_ratio=1.0)),
    ("nlambda", _ALL, lambda e, a: dict(nlambda=0)),
    ("maxit", _ALL, lambda e, a: dict(maxit=0)),
    ("tol", _ALL, lambda e, a: dict(tol=-1.0)),
    ("irls_tol", _ALL, lambda e, a: dict(irls_tol=-1.0)),
    ("lambda_count", _ALL, lambda e, a: dict(lambda_=[[0.3, 0.2, 0.1], [0.3, 0.2, 0.1]])),
    ("lambda_lengths", _ALL, lambda e, a: dict(penalty=["lasso", "mcp"], lambda_=[[0.3, 0.2, 0.1], [0.3, 0.2]])),
    ("lambda_empty", _ALL, lambda e, a: dict(penalty=["lasso", "mcp"], lambda_=[[0.3, 0.2, 0.1], []])),
    ("lambda_one", _CV, lambda e, a: dict(lambda_=[0.1])),
    ("nfolds", _FOLDS, lambda e, a: dict(nfolds=2)),
    ("foldid", _FOLDS + ("oem_fit_logistic_dense_multi_folds",), lambda e, a: dict(foldid=np.resize(np.arange(1, 5), N - 1))),
    ("weights", tuple(e for e in ("oem", "oem_sparse", "oem_multi", "big_oem", "xval_oem_multi") + _BINOMIAL + _CV), lambda e, a: dict(weights=np.ones(N))),
    ("scale_factor", ("oem_xtx",), lambda e, a: dict(scale_factor=np.ones(P + 1))),
]


def refusal_cases(entry):
    """[(case name, the faults' names)]: every fault the entry takes alone, then every pair of neighbours in that list which do not set
    the same argument"""
    mine = [f for f in FAULTS if f[1] is None or entry in f[1]]
    if entry == "oem_fit_logistic_dense_multi_folds":                # (nfolds is what foldid holds)
        mine = [f for f in mine if f[0] != "nfolds"]
    cases = [(f[0], (f[0],)) for f in mine]
    probe = dict(x=np.zeros((2, 2)), xtx=np.zeros((2, 2)), y=np.zeros(2), Y=np.zeros((2, 2)), xty=np.zeros(2))
    for f, g in zip(mine, mine[1:]):
        if not set(f[2](entry, probe)) & set(g[2](entry, probe)):
            cases.append((f[0] + "+" + g[0], (f[0], g[0])))
    return cases


class _Reached(Exception):
    """the call got as far as the library or a device"""


def _no_library(api):
    """patches that turn every look for the library or a context into _Reached; returns the undo"""
    from oem_amd import _lib as L
    saved = (L.lib, api.context)

    def reached(*a, **k):
        raise _Reached()
    L.lib, api.context = reached, reached

    def undo():
        L.lib, api.context = saved
    return undo


def run_refusal(api, entry, faults):
    """[type name, message] of what the entry raises on this case, or None when it gets as far as the library or a device"""
    fn, args, _, fixed = _entries(api)[entry]
    kw = dict(args, **fixed)
    by_name = {f[0]: f for f in FAULTS}
    for name in faults:
        kw.update(by_name[name][2](entry, args))
    undo = _no_library(api)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fn(**kw)
    except _Reached:
        return None
    except (ValueError, TypeError, NotImplementedError, api.L.OemgpuError) as e:
        return [type(e).__name__, str(e)]
    except Exception:                                                 # (torch's own sentence for a machine without a device)
        return None
    finally:
        undo()
    return None


# ------------------------------------------------------------------------------------------ option blocks
class _Stop(Exception):
    pass


def _plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, (list, tuple)):
        return [_plain(u) for u in v]
    if callable(v):
        return "callable"
    return v


def _recording_args(api):
    real = api._Args
    sig = inspect.signature(real.__init__)
    seen = []

    class Recording(real):
        def __init__(self, *a, **k):
            b = sig.bind(self, *a, **k)
            b.apply_defaults()
            seen.append({name: _plain(v) for name, v in b.arguments.items() if name != "self"})
            raise _Stop()
    return real, Recording, seen


_LAM2 = [[0.4, 0.2, 0.1], [0.5, 0.25, 0.125]]
_G0 = np.array([0, 1, 1, 2, 2])
_G1 = np.array([1, 1, 2, 2, 3])


def option_grid(entry):
    """name -> keyword arguments of a valid option set, for this entry"""
    grid = {"default": {}, "two_penalties_lambda": dict(penalty=["lasso", "mcp"], lambda_=_LAM2), "lambda_min_ratio": dict(lambda_min_ratio=0.05),
            "compute_loss": dict(compute_loss=True)}
    for gname, g in (("g0", _G0), ("g1", _G1)):
        for gw in (False, True):
            for icpt in ((None,) if entry == "oem_xtx" else (True, False)):
                kw = dict(penalty=["grp.lasso", "lasso"], groups=g)
                if gw:
                    kw["group_weights"] = np.arange(1.0, len(np.unique(g)) + 1.0)
                if icpt is not None:
                    kw["intercept"] = icpt
                grid[f"group_{gname}_{'gw' if gw else 'nogw'}_{'x' if icpt is None else int(icpt)}"] = kw
    if entry == "oem_xtx":
        del grid["compute_loss"]
    if entry in ("oem", "oem_sparse", "oem_multi", "cv_oem_gaussian", "cv_oem_multi"):
        grid["accelerate"] = dict(accelerate=True)
    if entry in ("oem", "oem_sparse", "big_oem", "xval_oem", "cv_oem_gaussian"):
        grid["ngpus"] = dict(ngpus=2)
        grid["devices"] = dict(devices=[0])
        grid["upload_threads"] = dict(upload_threads=3)
    if entry in ("oem_multi", "cv_oem_multi"):
        grid["upload_threads"] = dict(upload_threads=3)
    if entry in ("oem", "oem_sparse", "oem_fit_logistic_dense", "oem_fit_logistic_sparse", "big_oem"):
        grid["n_less_than_p"] = dict(_wide=True)
    if entry == "big_oem":
        grid["every_penalty"] = dict(penalty=None, groups=_G1)
    if entry in _CV + ("xval_oem", "xval_oem_multi"):
        grid["type_measure_mae"] = dict(type_measure="mae")
    if entry in _FOLDS:
        grid = {k: dict(v, foldid=np.resize(np.arange(1, 5), N)) for k, v in grid.items()}
    return grid


HOST_OPTION_ENTRIES = ("oem", "oem_sparse", "oem_fit_logistic_dense", "oem_fit_logistic_sparse", "oem_xtx", "big_oem", "xval_oem",
                       "cv_oem_gaussian")
GPU_OPTION_ENTRIES = ("oem_multi", "oem_fit_logistic_dense_multi", "oem_fit_logistic_dense_multi_folds", "xval_oem_multi", "cv_oem_binomial",
                      "cv_oem_multi", "cv_oem_logistic_multi")


def _to_device(v):
    import torch
    return torch.as_tensor(np.ascontiguousarray(v), device="cuda")


def run_options(api, entry, name, gpu=False):
    """{"args": the constructor arguments of the first _Args the call builds, "warnings": the messages on the way there}"""
    import scipy.sparse as sp
    fn, args, _, fixed = _entries(api)[entry]
    kw = dict(option_grid(entry)[name])
    args = dict(args)
    if kw.pop("_wide", False):                                       # n < p: the first four rows
        for k in ("x", "y"):
            args[k] = args[k][:4]
    if gpu:
        for k in ("x", "Y"):
            if k in args and not sp.issparse(args[k]):
                args[k] = _to_device(args[k])
    real, Recording, seen = _recording_args(api)
    api._Args = Recording
    try:
        with warnings.catch_warnings(record=True) as ws:
            warnings.simplefilter("always")
            try:
                fn(**{**args, **fixed, **kw})
            except _Stop:
                pass
            else:
                raise AssertionError(f"{entry}/{name}: the call built no _Args")
    finally:
        api._Args = real
    return {"args": seen[0], "warnings": [str(w.message) for w in ws if issubclass(w.category, UserWarning)]}


# ------------------------------------------------------------------------------------------ result bytes
def digest(v):
    """SHA-256 over a canonical walk of a result: arrays as dtype, shape and bytes, containers in their order with their keys"""
    h = hashlib.sha256()

    def walk(u):
        if type(u).__module__.startswith("torch"):
            u = u.cpu().numpy()
        if isinstance(u, dict):
            h.update(b"{")
            for k, w in u.items():
                h.update(str(k).encode() + b":")
                walk(w)
            h.update(b"}")
        elif isinstance(u, (list, tuple)):
            h.update(b"[")
            for w in u:
                walk(w)
                h.update(b",")
            h.update(b"]")
        elif isinstance(u, (np.ndarray, np.generic)):
            a = np.ascontiguousarray(u)
            h.update(f"{a.dtype.str}{a.shape}".encode() + a.tobytes())
        elif isinstance(u, float):
            h.update(b"f" + np.float64(u).tobytes())
        else:
            h.update(repr(u).encode())
    walk(v)
    return h.hexdigest()


def _fit_digests(res):
    """a result (one fit or a list, lists of lists flattened) -> [{"keys": in order, "sha": key -> digest}]"""
    flat = []

    def gather(r):
        if isinstance(r, dict):
            flat.append(r)
        else:
            for q in r:
                gather(q)
    gather(res)
    return [{"keys": list(f), "sha": {k: digest(f[k]) for k in f}} for f in flat]


def _bytes_data():
    rng = np.random.default_rng(20262)
    n, p, m = 200, 6, 3
    x = rng.normal(size=(n, p)) + 0.5
    b = np.array([1.0, -0.7, 0.4, 0.0, 0.0, 0.0])
    Y = (x @ b)[:, None] * np.array([1.0, 0.5, -1.0]) + rng.normal(size=(n, m))
    Yb = (Y + 0.3 * rng.normal(size=(n, m)) > 0).astype(np.float64)
    fold = rng.permutation(np.resize(np.arange(1, 5), n))
    return x, Y, Yb, fold


_PEN = ["lasso", "mcp"]


def bytes_cases():
    """name -> function(oem_amd.api) -> result.  `seeded` cases draw their folds from a Generator and return its state with the result."""
    import scipy.sparse as sp
    x, Y, Yb, fold = _bytes_data()
    y, yb = Y[:, 0], Yb[:, 0]
    kw = dict(penalty=_PEN, nlambda=8)
    cm = lambda: _to_device(x.T).t()                                  # column-major on the device
    rm = lambda: _to_device(x)
    xs = sp.csc_matrix(np.where(np.abs(x) > 0.6, x, 0.0))

    def seeded(fn):
        def run(api):
            g = np.random.default_rng(77)
            res = fn(api, g)
            return [res, {"rng": g.bit_generator.state["state"]}]
        return run
    cases = {
        "oem_host": lambda api: api.oem(x, y, compute_loss=True, **kw),
        "oem_device": lambda api: api.oem(rm(), y, compute_loss=True, **kw),
        "oem_sparse": lambda api: api.oem(xs, y, **kw),
        "oem_multi": lambda api: api.oem_multi(rm(), Y, **kw),
        "oem_fit_logistic_dense": lambda api: api.oem_fit_logistic_dense(cm(), yb, compute_loss=True, **kw),
        "oem_fit_logistic_dense_host": lambda api: api.oem_fit_logistic_dense(x, yb, **kw),
        "oem_fit_logistic_dense_multi": lambda api: api.oem_fit_logistic_dense_multi(rm(), Yb, **kw),
        "oem_fit_logistic_dense_multi_folds": lambda api: api.oem_fit_logistic_dense_multi_folds(rm(), Yb, fold, **kw),
        "oem_fit_logistic_sparse": lambda api: api.oem_fit_logistic_sparse(xs, yb, **kw),
        "oem_xtx": lambda api: api.oem_xtx(x.T @ x / len(y), x.T @ y / len(y), **kw),
        "big_oem": lambda api: api.big_oem([x[:120], x[120:]], [y[:120], y[120:]], **kw),
        "xval_oem": lambda api: api.xval_oem(x, y, foldid=fold, **kw),
        "xval_oem_device": lambda api: api.xval_oem(rm(), y, foldid=fold, type_measure="mae", **kw),
        "xval_oem_multi": lambda api: api.xval_oem_multi(cm(), Y, foldid=fold, **kw),
        "cv_oem_gaussian_host": lambda api: api.cv_oem(x, y, foldid=fold, keep=True, **kw),
        "cv_oem_gaussian_device": lambda api: api.cv_oem(rm(), y, foldid=fold, keep=True, type_measure="mae", **kw),
        "cv_oem_gaussian_ungrouped": lambda api: api.cv_oem(cm(), y, foldid=fold, keep=True, grouped=False, **kw),
        "cv_oem_gaussian_sparsex": lambda api: _on_sparsex(api, xs, lambda sx: api.cv_oem(sx, y, foldid=fold, keep=True, **kw)),
        "cv_oem_binomial_mae": lambda api: api.cv_oem(cm(), yb, family="binomial", foldid=fold, keep=True, type_measure="mae", **kw),
        "cv_oem_binomial_auc": lambda api: api.cv_oem(x, yb, family="binomial", foldid=fold, keep=True, type_measure="auc", **kw),
        "cv_oem_binomial_ungrouped": lambda api: api.cv_oem(rm(), yb, family="binomial", foldid=fold, keep=True, grouped=False, **kw),
        "cv_oem_binomial_scipy": lambda api: api.cv_oem(xs, yb, family="binomial", foldid=fold, keep=True, **kw),
        "cv_oem_binomial_scipy_class": lambda api: api.cv_oem(xs, yb, family="binomial", foldid=fold, keep=True, type_measure="class", **kw),
        "cv_oem_multi": lambda api: api.cv_oem_multi(rm(), Y, foldid=fold, keep=True, **kw),
        "cv_oem_logistic_multi": lambda api: api.cv_oem_logistic_multi(rm(), Yb, foldid=fold, keep=True, **kw),
        "cv_oem_logistic_multi_auc": lambda api: api.cv_oem_logistic_multi(cm(), Yb, foldid=fold, keep=True, type_measure="auc", **kw),
        # the folds drawn from a seeded Generator: the draw, and what is left of the Generator
        "xval_oem_drawn": seeded(lambda api, g: api.xval_oem(x, y, nfolds=4, rng=g, **kw)),
        "xval_oem_multi_drawn": seeded(lambda api, g: api.xval_oem_multi(rm(), Y, nfolds=4, rng=g, **kw)),
        "cv_oem_gaussian_drawn": seeded(lambda api, g: api.cv_oem(rm(), y, nfolds=4, rng=g, keep=True, **kw)),
        "cv_oem_binomial_drawn": seeded(lambda api, g: api.cv_oem(rm(), yb, family="binomial", nfolds=4, rng=g, keep=True, **kw)),
        "cv_oem_multi_drawn": seeded(lambda api, g: api.cv_oem_multi(rm(), Y, nfolds=4, rng=g, keep=True, **kw)),
        "cv_oem_logistic_multi_drawn": seeded(lambda api, g: api.cv_oem_logistic_multi(rm(), Yb, nfolds=4, rng=g, keep=True, **kw)),
    }
    return cases


def _on_sparsex(api, xs, fn):
    with api.SparseX(xs) as sx:
        return fn(sx)


def run_bytes(api, name):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return _fit_digests(bytes_cases()[name](api))


# ------------------------------------------------------------------------------------------ the recording
def record_host(api):
    out = {"refusals": {}, "options": {}}
    for entry in _entries(api):
        for case, faults in refusal_cases(entry):
            got = run_refusal(api, entry, faults)
            if got is not None:
                out["refusals"][f"{entry}/{case}"] = got
    for entry in HOST_OPTION_ENTRIES:
        for name in option_grid(entry):
            out["options"][f"{entry}/{name}"] = run_options(api, entry, name)
    return out


def record_gpu(api):
    out = {"options_gpu": {}, "bytes_gpu": {}}
    for entry in GPU_OPTION_ENTRIES:
        for name in option_grid(entry):
            out["options_gpu"][f"{entry}/{name}"] = run_options(api, entry, name, gpu=True)
    for name in bytes_cases():
        out["bytes_gpu"][name] = run_bytes(api, name)
    return out


if __name__ == "__main__":
    from oem_amd import api as _api
    path = sys.argv[1]
    if len(sys.argv) > 2 and sys.argv[2] == "gpu":
        with open(path) as f:
            doc = json.load(f)
        doc.update(record_gpu(_api))
    else:
        doc = record_host(_api)
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
