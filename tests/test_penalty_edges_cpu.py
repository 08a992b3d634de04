"""The penalty operators at the edges of their parameters -- alpha in {0, 1}, tau in {0, 1}, gamma just above its lower limit, exact
zeros among the penalty factors and group weights -- with the oracle alone (no GPU): the table of edge cases that
tests/test_gpu_penalty_edges.py runs through every path engine, and the proof that each case is worth running there:

  * every path converges (no lambda reaches maxit) and stays finite,
  * every region of the operators that a case exists to reach holds at least MIN_PAIRS (coefficient, lambda) pairs whose relative
    margin to the nearest region boundary is at least MIN_MARGIN (tests/penalty_census.py), so that rounding on a device cannot move
    them into a neighbouring branch -- a copy of the operator with that branch wrong cannot pass,
  * three identities of the operators hold in the oracle bit for bit: sparse.grp.lasso at tau = 1 is the lasso, at tau = 0 it is
    grp.lasso, and every .net penalty at alpha = 1 is its plain penalty.

Data: standardised Gaussian columns, n = 50 p rows, coefficients of mixed sizes; the Gram
form (xtx, xty) of the same data serves the census and the oem.xtx engines.  Lambdas are always supplied (a generated grid is divided
by alpha: inf at alpha = 0, as in the reference)."""
import functools
import warnings
from dataclasses import dataclass

import numpy as np
import pytest

from oracle import oracle as orc
from tests import penalty_census as pc

MIN_PAIRS, MIN_MARGIN = 3, 1e-6
TOL, MAXIT = 1e-9, 2000
SHAPES = (40, 100, 150, 200, 230, 300, 640, 1030)     # the smallest p that selects each form of each Gram engine (RUNS below)
WIDE_SHAPES = ((40, 100), (130, 200))
# p >= n: the Gram is singular and the iteration slow.  Twelve lambdas down to 0.1 max |xty| on 20 true coefficients put >= 3 pairs into
# every needed region at both shapes; the oracle's longest lambda then takes 5,921 iterations at 1e-7 (zeros-group, whose unpenalised
# group makes it slower still, stops at 0.3 max |xty|)
WIDE_TOL, WIDE_MAXIT = 1e-7, 12000
WIDE_NLAMBDA, WIDE_LAM_LO, WIDE_NONZERO = 12, 0.1, 20

NETS = ["elastic.net", "mcp.net", "scad.net", "grp.lasso.net", "grp.mcp.net", "grp.scad.net"]
PLAIN = ["lasso", "mcp", "scad", "grp.lasso", "grp.mcp", "grp.scad"]
_FULL = {"lasso": ("zero", "shrunk"), "mcp": ("zero", "shrunk", "big"), "scad": ("zero", "soft", "mid", "big"),
         "grp.lasso": ("zero", "shrunk"), "grp.mcp": ("zero", "shrunk", "one"), "grp.scad": ("zero", "soft", "mid", "one")}


@dataclass(frozen=True)
class Case:
    name: str
    penalty: tuple
    need: tuple                      # per penalty: the regions the case exists to reach
    alpha: float = 1.0
    gamma: float = 3.0
    tau: float = 0.5
    pf: bool = False                 # penalty factors with exact zeros
    gw: str = ""                     # "": sqrt(group size); "random": uniform(0.5, 2); "zero": random with one exact 0
    compute_loss: bool = False
    lam_hi: float = 0.9              # the lambda grid, as fractions of max |xty|
    lam_lo: float = 0.02
    wide_lam_lo: float = 0.0         # p >= n: the grid's lower end where it is above WIDE_LAM_LO

    @property
    def has_groups(self):
        return any("grp" in q for q in self.penalty)

    def subset(self, which):
        """the case with its element-wise ("elem", "mixed-elem") or its group ("group") penalties only; "all": as it is"""
        if which == "all":
            return self
        keep = [k for k, q in enumerate(self.penalty) if ("grp" in q) == (which == "group")]
        return Case(**{**self.__dict__, "penalty": tuple(self.penalty[k] for k in keep), "need": tuple(self.need[k] for k in keep)})


CASES = [
    # alpha = 0: no threshold at all (L = 0), the ridge denominator D = d + lambda; scad.net's special case
    Case("net-alpha-0", tuple(NETS), (("shrunk",), ("big",), ("big",), ("shrunk",), ("one",), ("one",)), alpha=0.0),
    # alpha = 1: every .net penalty next to its plain penalty in one call (the device must give the same bits)
    Case("net-alpha-1", tuple(NETS + PLAIN), tuple(_FULL[q] for q in PLAIN + PLAIN), alpha=1.0),
    # tau = 0: the inner soft threshold is the identity;  tau = 1: the group threshold is 0 and a group the inner threshold zeroes
    # entirely has norm 0 (0 / 0 in the factor unless it is guarded)
    Case("tau-0", ("sparse.grp.lasso", "grp.lasso"), (("norm_zero", "alive"), ("zero", "shrunk")), tau=0.0, gw="random"),
    Case("tau-1", ("sparse.grp.lasso", "lasso"), (("inner_zero", "alive"), ("zero", "shrunk")), tau=1.0, gw="random", compute_loss=True),
    # gamma just above its lower limit: the denominators (gamma - 1) D - 1 and D - 1 / gamma are small
    Case("scad-gamma-2.05", ("scad", "scad.net"), (("zero", "big"),) * 2, alpha=0.5, gamma=2.05),
    Case("scad-gamma-2.5", ("scad", "scad.net"), (("zero", "soft", "mid", "big"),) * 2, alpha=0.5, gamma=2.5),
    Case("mcp-gamma-1.05", ("mcp", "mcp.net"), (("zero", "big"),) * 2, alpha=0.5, gamma=1.05),
    Case("mcp-gamma-1.5", ("mcp", "mcp.net"), (("zero", "shrunk", "big"),) * 2, alpha=0.5, gamma=1.5),
    Case("grp-scad-gamma-2.05", ("grp.scad",), (("zero", "one"),), gamma=2.05),
    Case("grp-scad-gamma-2.5", ("grp.scad",), (("zero", "mid", "one"),), gamma=2.5),
    Case("grp-mcp-gamma-1.05", ("grp.mcp",), (("zero", "one"),), gamma=1.05),
    Case("grp-mcp-gamma-1.5", ("grp.mcp",), (("zero", "shrunk", "one"),), gamma=1.5),
    # exact zeros: coordinates / a group that are not penalised at all
    Case("zeros-elem", ("lasso", "scad"), (("zero", "shrunk"), ("zero", "big")), pf=True),
    Case("zeros-group", ("grp.lasso", "grp.mcp"), (("zero", "shrunk"), ("zero", "one")), gw="zero", wide_lam_lo=0.3),
]
CASE_BY_NAME = {c.name: c for c in CASES}
ELEM_CASES = [c.name for c in CASES if any("grp" not in q for q in c.penalty)]
GROUP_CASES = [c.name for c in CASES if c.has_groups]
MIXED_CASES = [c.name for c in CASES if c.has_groups and c.name in ELEM_CASES]


@dataclass(frozen=True)
class Run:
    """one way to an engine: the entry ("oem" on the standardised data, "xtx" on its Gram form), the shape, the part of every case that
    is run ("all", "elem", "group"; "mixed-elem": the element-wise penalties of the cases that also hold group penalties), the switches that force the engine, and the engine's name (oem_amd.api.ENGINES)"""
    id: str
    entry: str
    p: int
    engine: str
    which: str = "all"
    env: tuple = ()
    n: int = 0                       # p >= n runs: the rows

    def engine_for(self, case):
        """p >= n: the register-resident and streamed forms take element-wise operators only"""
        if self.n and case.has_groups:
            return {"wres": "wcoop", "wstream": "wlaunches"}.get(self.engine, self.engine)
        return self.engine

    def cases(self):
        """(case name, group layout) of every run"""
        names = {"all": [c.name for c in CASES], "elem": ELEM_CASES, "group": GROUP_CASES, "mixed-elem": MIXED_CASES}[self.which]
        out = []
        for nm in names:
            lays = _layouts(CASE_BY_NAME[nm], self.p) if self.engine == "coop" else ("ragged",)
            out += [(nm, lay) for lay in lays]
        return out


# path_small.hip: four waves (p <= 128), eight (<= 160), eight with columns in LDS (<= 208), and the four-workgroup form (<= 288, where the
# cooperating engine is switched off); path_coop.hip at 300 and 640; path_symcoop.hip's two kernels at 1030; path_large.hip below and
# beyond 1024
RUNS = [Run("rows-40", "oem", 40, "rows"), Run("rows-100", "oem", 100, "rows"), Run("rows-150", "oem", 150, "rows"),
        Run("rows-200", "oem", 200, "rows"), Run("rows-230", "oem", 230, "rows", env=("OEM_NO_COOP",)),
        Run("coop-300", "oem", 300, "coop"), Run("coop-640", "xtx", 640, "coop"),
        Run("rowcoop-1030", "xtx", 1030, "rowcoop", which="elem"),
        Run("symcoop-1030-elem", "xtx", 1030, "symcoop", which="elem", env=("OEM_NO_ROWCOOP",)),
        Run("symcoop-1030-group", "xtx", 1030, "symcoop", which="group", env=("OEM_NO_ROWCOOP",)),
        Run("launches-300", "oem", 300, "launches", env=("OEM_NO_COOP",)),
        Run("launches-1030", "xtx", 1030, "launches", env=("OEM_NO_SYMCOOP", "OEM_NO_ROWCOOP"))]
# the forcing switches of test_wide_engine / _cooperating_engine / _resident_in_the_accumulator_file / _streamed_engine (test_gpu_parity.py)
_WIDE_ENV = {"wcoop": ("OEM_WIDE",), "wres": ("OEM_WIDE", "OEM_WRES"), "wstream": ("OEM_WIDE", "OEM_NO_WRES", "OEM_WSTREAM", "OEM_NO_WCOOP"),
             "wlaunches": ("OEM_WIDE", "OEM_NO_WCOOP")}
WIDE_RUNS = [Run(f"{e}-{n}x{p}", "oem", p, e, env=_WIDE_ENV[e], n=n) for (n, p) in WIDE_SHAPES for e in _WIDE_ENV]
# (the mixed cases once more with their element-wise penalties alone: alpha = 0 / 1 and tau = 1's lasso on the forms that take nothing else)
WIDE_ELEM_RUNS = [Run(f"{e}-{n}x{p}-elem", "oem", p, e, which="mixed-elem", env=_WIDE_ENV[e], n=n) for (n, p) in WIDE_SHAPES for e in ("wres", "wstream")]


@functools.lru_cache(maxsize=None)
def problem(p, n=None):
    """seeded standardised data (columns and y centred, variance 1 with divisor n) and its Gram form.  n = 50 p unless given: the
    non-convex operators at small gamma iterate to a fixed point only where the Gram's small eigenvalues exceed 1 / gamma.  Beyond
    p = 300 only the Gram form is kept (the engines for those sizes are run through oem.xtx)."""
    if n is None:
        n = 50 * p
    rng = np.random.default_rng(1000 * p + n)
    x = np.empty((n, p), order="F")
    for j0 in range(0, p, 64):
        x[:, j0:j0 + 64] = rng.standard_normal((n, min(64, p - j0)))
    m = max(12, p // 6) if n > p else WIDE_NONZERO
    b = np.zeros(p)
    b[rng.choice(p, m, replace=False)] = rng.choice([-1.0, 1.0], m) * np.geomspace(0.08, 1.5, m)
    y = x @ b + rng.normal(size=n)
    x -= x.mean(axis=0); x /= np.sqrt(np.einsum("ij,ij->j", x, x) / n)
    y = y - y.mean(); y = y / np.sqrt((y * y).mean())
    out = dict(n=n, p=p, y=y)
    xty = x.T @ y / n
    if n > p:
        out["xtx"], out["xty"] = x.T @ x / n, xty
    if p <= 300:
        out["x"] = x
    out["lmax"] = float(np.abs(xty).max())
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def layout(p, kind):
    """group labels: "ragged" -- runs of 1 .. 12 neighbouring columns, labels in no particular order, label 0 (unpenalised) among
    them;  "eights" -- runs of eight starting at label 0 (the cooperating engine's eight-lane form)"""
    if kind == "eights":
        g = np.arange(p) // 8
    else:
        rng = np.random.default_rng(77 + p)
        sizes = []
        while sum(sizes) < p:
            sizes.append(int(rng.integers(1, 13)))
        sizes[-1] -= sum(sizes) - p
        g = np.repeat(rng.permutation(len(sizes)), sizes)
    g = g.astype(np.int32)
    g.setflags(write=False)
    return g


def _layouts(case, p):
    """the layouts RUNS uses at this shape.  "eights" only at 640: path_coop.hip takes its eight-lane form where q is a multiple of 8 and
    every group is an aligned run of eight (at 300 the same labels would run the general form once more)"""
    return ("ragged", "eights") if case.has_groups and p == 640 else ("ragged",)


def nlambda(p):
    return 12 if p < 1030 else 6


def options(case, p, lay="ragged"):
    """(keywords of the oem_amd call that the case fixes whatever the problem -- penalties, alpha, gamma, tau, penalty factors, groups and
    their weights, compute_loss --, keywords the oracle takes on top of them)"""
    kw = dict(penalty=list(case.penalty), alpha=case.alpha, gamma=case.gamma, tau=case.tau)
    extra = {}
    rng = np.random.default_rng(5 * p + 1)
    if case.pf:
        pf = rng.uniform(0.5, 2.0, p); pf[rng.choice(p, 4, replace=False)] = 0.0
        kw["penalty_factor"] = pf
    if case.has_groups:
        g = layout(p, lay)
        kw["groups"] = g
        extra["unique_groups"] = np.unique(g)
        if case.gw:
            gw = rng.uniform(0.5, 2.0, len(extra["unique_groups"]))
            if case.gw == "zero":
                gw[len(gw) // 2] = 0.0
            kw["group_weights"] = gw
    if case.compute_loss:
        kw["compute_loss"] = True
    return kw, extra


def call_kwargs(case, p, lay="ragged", n=0):
    """options() with the lambda grid, tolerance and cap of problem(p) (n = 0) or of the p >= n problem(p, n)"""
    kw, extra = options(case, p, lay)
    if n:
        lam = np.geomspace(case.lam_hi, max(WIDE_LAM_LO, case.wide_lam_lo), WIDE_NLAMBDA) * problem(p, n)["lmax"]
        kw.update(lambda_=lam, tol=WIDE_TOL, maxit=WIDE_MAXIT)
    else:
        kw.update(lambda_=np.geomspace(case.lam_hi, case.lam_lo, nlambda(p)) * problem(p)["lmax"], tol=TOL, maxit=MAXIT)
    return kw, extra


_FITS = {}


def oracle_xtx(name, p, lay="ragged", which="all", d=0.0):
    """the oracle's path on the Gram form of problem(p), computed once per (case, shape, layout, subset, d)"""
    key = (name, p, lay, which, d)
    if key not in _FITS:
        case = CASE_BY_NAME[name].subset(which)
        kw, extra = call_kwargs(case, p, lay)
        kw.pop("compute_loss", None)                       # (oem.xtx has no loss)
        pr = problem(p)
        _FITS[key] = _frozen(orc.fit_xtx(pr["xtx"], pr["xty"], native=True, d_override=d, **kw, **extra))
    return _FITS[key]


def oracle_dense(name, p, lay="ragged", which="all"):
    """the oracle's oem() on the standardised data of problem(p), p <= 300, computed once"""
    key = ("dense", name, p, lay, which)
    if key not in _FITS:
        kw, extra = call_kwargs(CASE_BY_NAME[name].subset(which), p, lay)
        pr = problem(p)
        _FITS[key] = _frozen(orc.fit_dense(pr["x"], pr["y"], native=True, **kw, **extra))
    return _FITS[key]


def oracle_wide(name, n, p, which="all"):
    key = (name, n, p, which)
    if key not in _FITS:
        case = CASE_BY_NAME[name].subset(which)
        pr = problem(p, n)
        kw, extra = call_kwargs(case, p, "ragged", n=n)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _FITS[key] = _frozen(orc.fit_dense(pr["x"], pr["y"], native=True, **kw, **extra))
    return _FITS[key]


def _frozen(r):
    for k in ("beta", "niter", "lambda", "loss"):
        for a in r[k]:
            a.setflags(write=False)
    return r


def _census(case, p, lay, r, k, n=0):
    """the census of penalty k of a fit r of the oracle: on the Gram form of problem(p), or (n > 0) on x'x / n, x'y / n of the p >= n
    problem -- standardised data, so the coefficients below the intercept's row are those the iteration ran on"""
    kw, extra = options(case, p, lay)
    pr = problem(p, n) if n else problem(p)
    beta = r["beta"][k][1:] if n else r["beta"][k]
    xtx = pr["x"].T @ pr["x"] / n if n else pr["xtx"]
    xty = pr["x"].T @ pr["y"] / n if n else pr["xty"]
    return pc.census(case.penalty[k], xtx, xty, r["d"], beta, r["lambda"][k], alpha=case.alpha, gamma=case.gamma,
                     tau=case.tau, penalty_factor=kw.get("penalty_factor"), groups=kw.get("groups"), unique_groups=extra.get("unique_groups"),
                     group_weights=kw.get("group_weights"))


@pytest.mark.parametrize("p", SHAPES)
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_every_case_converges_and_reaches_its_regions(name, p):
    case = CASE_BY_NAME[name]
    for lay in _layouts(case, p):
        r = oracle_xtx(name, p, lay)
        for k, pen in enumerate(case.penalty):
            assert np.isfinite(r["beta"][k]).all(), (pen, lay)
            assert r["niter"][k].max() <= MAXIT // 2, (pen, lay, r["niter"][k])          # far from the cap: a device one iteration off is not at it either
            region, margin = _census(case, p, lay, r, k)
            got = pc.counts(region, margin, MIN_MARGIN)
            assert "mid_zero" not in got
            for need in case.need[k]:
                assert got.get(need, 0) >= MIN_PAIRS, (pen, lay, need, got)
            kw, _ = call_kwargs(case, p, lay)
            if case.pf:                                    # the unpenalised coordinates: never thresholded
                free = kw["penalty_factor"] == 0
                assert np.all(region[free] == ("shrunk" if pen == "lasso" else "big")) and np.all(margin[free] == 1.0)
            if case.gw == "zero":                          # the group of weight 0: its factor is 1 (grp.lasso: 1 - 0 / s)
                ug = np.unique(kw["groups"])
                g0 = ug[np.flatnonzero(kw["group_weights"] == 0)[0]]
                if g0 != 0:
                    assert np.all(region[kw["groups"] == g0] == ("shrunk" if pen == "grp.lasso" else "one"))


@pytest.mark.parametrize("p", SHAPES)
def test_tau_edges_contain_whole_groups(p):
    """tau = 1: at least one group with s = 0 exactly and one living group at some lambda; tau = 0: zeroed and shrunk groups"""
    for name, a, b in (("tau-1", "inner_zero", "alive"), ("tau-0", "norm_zero", "alive")):
        case = CASE_BY_NAME[name]
        for lay in _layouts(case, p):
            r = oracle_xtx(name, p, lay)
            region, margin = _census(case, p, lay, r, 0)
            g = layout(p, lay)
            for want in (a, b):
                hit = (region == want) & (margin >= MIN_MARGIN)
                assert any(hit[g == lab].any() for lab in np.unique(g) if lab != 0), (name, lay, want)


@pytest.mark.parametrize("p", SHAPES)
def test_operator_identities_hold_bit_for_bit_in_the_oracle(p):
    """sparse.grp.lasso at tau = 1 is the lasso and at tau = 0 grp.lasso; every .net penalty at alpha = 1 is its plain penalty"""
    for lay in _layouts(CASE_BY_NAME["tau-0"], p):
        for name in ("tau-1", "tau-0"):
            r = oracle_xtx(name, p, lay)
            assert np.array_equal(r["beta"][0], r["beta"][1]) and np.array_equal(r["niter"][0], r["niter"][1]), (name, lay)
        r = oracle_xtx("net-alpha-1", p, lay)
        for k in range(6):
            assert np.array_equal(r["beta"][k], r["beta"][k + 6]) and np.array_equal(r["niter"][k], r["niter"][k + 6]), (NETS[k], lay)


def test_the_census_classifies_as_the_operator_thresholds():
    """the census against the oracle's operator itself (orc.threshold): a pair it calls zero is a zero of the operator and the others
    are not, on arguments spread over every region and at every edge parameter of the table"""
    rng = np.random.default_rng(3)
    p = 60
    g = layout(p, "ragged")
    ug = np.unique(g)
    gw = rng.uniform(0.5, 2.0, len(ug))
    pf = rng.uniform(0.5, 2.0, p); pf[:3] = 0.0
    u = rng.normal(size=p) * np.geomspace(0.05, 8.0, p)
    g0 = np.flatnonzero(g == 0)
    u[g0[0]], u[g0[1:]] = 0.01, 5.0                        # the unpenalised group: a member below the inner threshold, the others above
    xtx, d, lam = np.eye(p), 1.3, 0.7                       # u = xty + (d I - xtx) beta: with beta = 0, u = xty
    for pen in NETS + PLAIN + ["sparse.grp.lasso"]:
        for alpha, gamma, tau in ((0.0, 3.0, 0.0), (1.0, 2.05, 1.0), (0.5, 2.5, 0.4), (0.5, 1.5, 0.4), (0.5, 1.05, 0.4)):
            if "scad" in pen and gamma < 2:
                continue
            out = orc.threshold(pen, u, lam, d, alpha=alpha, gamma=gamma, tau=tau, penalty_factor=pf, groups=g, unique_groups=ug, group_weights=gw)
            region, margin = pc.census(pen, xtx, u, d, np.zeros((p, 1)), [lam], alpha=alpha, gamma=gamma, tau=tau, penalty_factor=pf, groups=g,
                                       unique_groups=ug, group_weights=gw)
            zero = np.isin(region[:, 0], ("zero", "inner_zero", "norm_zero", "alive_zero", "free_zero"))
            assert np.array_equal(out == 0, zero), (pen, alpha, gamma, tau)
            if pen == "sparse.grp.lasso" and tau > 0:
                assert region[g0[0], 0] == "free_zero" and np.all(region[g0[1:], 0] == "free")
            L, D, L1 = pc.constants(pen, lam, d, alpha, tau)
            if pc.KIND[pen] in ("mcp", "scad"):           # the untouched region: u / D
                big = region[:, 0] == "big"
                assert np.array_equal(out[big], u[big] / D)
            if pc.KIND[pen] in ("grp.mcp", "grp.scad"):
                one = np.isin(region[:, 0], ("one", "free"))
                assert np.array_equal(out[one], u[one] * 1.0 / D)


@pytest.mark.parametrize("n,p", WIDE_SHAPES)
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_wide_cases_converge_and_reach_their_regions(name, n, p):
    """the p >= n runs: tolerance, cap and lambda grid are such that the oracle alone stops by its rule at every lambda, far from the cap,
    and every region the case is meant for holds its pairs with margin here too (the p >= n engines carry operator copies of their own)"""
    case = CASE_BY_NAME[name]
    r = oracle_wide(name, n, p)
    for k, pen in enumerate(case.penalty):
        assert np.isfinite(r["beta"][k]).all()
        assert r["niter"][k].max() <= WIDE_MAXIT // 2, (pen, r["niter"][k])
        got = pc.counts(*_census(case, p, "ragged", r, k, n=n), MIN_MARGIN)
        assert "mid_zero" not in got
        for need in case.need[k]:
            assert got.get(need, 0) >= MIN_PAIRS, (pen, need, got)


def planned_engine(run, name, lay="ragged", num_cu=256):
    """the engine the library's plan (oemgpu_selftest_plan through tests/test_host_api.py's _plan: host arithmetic, no GPU) gives a run of a
    case under the run's switches"""
    import os
    from oem_amd import _lib as L
    from tests.test_host_api import _SEM_DENSE, _SEM_XTX, _plan
    case = CASE_BY_NAME[name].subset(run.which)
    dense = run.entry == "oem"
    old = {e: os.environ.get(e) for e in run.env}
    try:
        for e in run.env:
            os.environ[e] = "1"
        L.reload_switches()
        return _plan(run.p, list(case.penalty), sem=_SEM_DENSE if dense else _SEM_XTX, intercept=int(dense),
                     groups=(lambda q: layout(run.p, lay)) if case.has_groups else None, wide_n=run.n, num_cu=num_cu,
                     compute_loss=dense and case.compute_loss, user_lambda=True)[0]
    finally:
        for e, v in old.items():
            if v is None:
                del os.environ[e]
            else:
                os.environ[e] = v
        L.reload_switches()


@pytest.mark.parametrize("run", RUNS + WIDE_RUNS + WIDE_ELEM_RUNS, ids=lambda r: r.id)
def test_every_run_is_planned_onto_its_engine(run):
    """on a 256-CU device, under its switches, every (case, layout) of a run goes to the engine the run is named after -- the GPU file
    asserts the same of the engine that ran"""
    assert run.cases()
    for name, lay in run.cases():
        assert planned_engine(run, name, lay) == run.engine_for(CASE_BY_NAME[name].subset(run.which)), (run.id, name, lay)
