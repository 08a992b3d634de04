"""predict() on the device (oemgpu_predict_dev, oemgpu_predict_rm_dev, oemgpu_predict_sparse_res), the part that needs no GPU: the
exports, the launch plan (oemgpu_selftest_predict_plan) swept over n, p, ncol for the three layouts, the refusals that come back before
a device is looked for, and the host inputs of predict() (numpy, scipy, CPU torch), which take the path they took before."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ["oemgpu_predict_dev", "oemgpu_predict_rm_dev", "oemgpu_predict_sparse_res", "oemgpu_selftest_predict_plan"]
ERR_ARG = -1
LDS_BYTES = 160 << 10          # LDS of a gfx950 CU
LDS_TABLE = 140 << 10          # the coefficient tile of a pass stays in LDS up to here
LDS_TURN = 8 * 8 * 16 * 17     # the eight waves' transposing tiles
KCH = 112                      # coefficient rows per LDS chunk
LAYOUTS = [-1, 0, 1]           # column-major, OEMGPU_F64, OEMGPU_F32


def _lib():
    import oem_amd
    return oem_amd.lib()


def test_entries_are_declared_exported_and_listed():
    import oem_amd
    from oem_amd import _lib as L
    header = (ROOT / "include" / "oemgpu.h").read_text()
    dyn = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert re.search(r" T " + name + r"$", dyn, re.M), name
        assert name in oem_amd.EXPORTS
        assert getattr(_lib(), name).argtypes is not None
    # every declaration says what it restates
    for name in ENTRIES:
        comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "R/methods.R:48-109, 346-367" in comment, name


def _plan(n, p, ncol, layout, num_cu):
    out = (C.c_int64 * 8)()
    rc = _lib().oemgpu_selftest_predict_plan(n, p, ncol, layout, num_cu, out)
    return rc, list(out)


NS = [1, 2, 15, 16, 17, 127, 128, 129, 255, 256, 257, 4099, 32767, 32768, 32769, 65537, 262143, 262144, 262145, 10 ** 6, 3_000_017, 10 ** 7]
PS = [1, 2, 3, 4, 5, 55, 56, 57, 100, 113, 158, 159, 160, 161, 300, 512, 1115, 1116, 1117, 1118, 1119, 1120, 1121, 8191, 19999, 20000]
NCOLS = [1, 2, 15, 16, 17, 31, 32, 33, 100, 111, 112, 113, 128, 129, 200, 224, 225, 299, 300]


@pytest.mark.parametrize("num_cu", [256, 1])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_plan_sweep(layout, num_cu):
    """for every (n, p, ncol): the workgroups' row ranges cover [0, n) without gaps and none is empty, the passes cover every 16-column
    tile with at most 7 per pass (x is read once while ncol <= 112, and never more often than ceil(tiles / 7) times), the LDS asked for
    fits a CU, and the table goes through LDS in chunks exactly when its pass tile exceeds 140 KiB"""
    seen = set()
    for n in NS:
        for p in PS:
            for ncol in NCOLS:
                rc, (rpw, nwg, lt, passes, chunk, krows, lds, nchunks) = _plan(n, p, ncol, layout, num_cu)
                assert rc == 0
                assert rpw >= 128 and rpw % 128 == 0
                assert nwg >= 1 and (nwg - 1) * rpw < n <= nwg * rpw          # ranges [g rpw, min(n, (g + 1) rpw)): no gap, none empty
                assert nwg <= 2 * num_cu
                ntile = -(-ncol // 16)
                assert 1 <= lt <= 7 and passes * lt >= ntile and (passes - 1) * lt < ntile
                assert passes == -(-ntile // 7)
                if ncol <= 112:
                    assert passes == 1 and lt == ntile
                K4 = (p + 1 + 3) // 4 * 4
                want_chunk = K4 * 16 * lt * 8 > LDS_TABLE
                assert chunk == int(want_chunk)
                assert krows == (KCH if want_chunk else K4)
                assert nchunks == (-(-K4 // KCH) if want_chunk else 1)
                assert nchunks * krows >= K4 and (nchunks - 1) * krows < K4
                assert lds == krows * 16 * lt * 8 + LDS_TURN and lds <= LDS_BYTES
                if 2 * lds > LDS_BYTES:
                    assert nwg <= num_cu                                      # one workgroup fills a CU: one round of them
                seen.add((chunk, passes > 1))
    assert seen == {(0, False), (0, True), (1, False), (1, True)}


def test_the_three_layouts_share_one_plan():
    for n, p, ncol in [(1, 1, 1), (4099, 300, 113), (10 ** 6, 512, 100), (64, 20000, 1)]:
        plans = [_plan(n, p, ncol, layout, 256) for layout in LAYOUTS]
        assert plans[0][0] == 0 and plans[0] == plans[1] == plans[2]


def test_the_switch_between_lds_and_chunks_is_where_the_formula_puts_it():
    """one column tile: 128 bytes per coefficient row, so K4 = 1120 rows (p + 1 in 1117..1120) is the last table that stays; seven
    tiles: 896 bytes per row, K4 = 160"""
    assert _plan(1000, 1119, 1, -1, 256)[1][4:8] == [0, 1120, 1120 * 128 + LDS_TURN, 1]
    assert _plan(1000, 1120, 1, -1, 256)[1][4:8] == [1, KCH, KCH * 128 + LDS_TURN, -(-1124 // KCH)]
    assert _plan(1000, 159, 112, -1, 256)[1][4:8] == [0, 160, 160 * 896 + LDS_TURN, 1]
    assert _plan(1000, 160, 112, -1, 256)[1][4:8] == [1, KCH, KCH * 896 + LDS_TURN, 2]


def test_plan_refusals():
    assert _plan(0, 4, 1, -1, 256)[0] == ERR_ARG and _plan(4, 0, 1, -1, 256)[0] == ERR_ARG and _plan(4, 4, 0, -1, 256)[0] == ERR_ARG
    assert _plan(4, 4, 1, -1, 0)[0] == ERR_ARG
    assert _plan(4, 4, 1, 2, 256)[0] == ERR_ARG and _plan(4, 4, 1, -2, 256)[0] == ERR_ARG
    assert _lib().oemgpu_selftest_predict_plan(4, 4, 1, -1, 256, None) == ERR_ARG


# a context, a handle and device pointers that are never dereferenced: every refusal below comes back before the device is touched
CTX, PTR = C.c_void_p(0x1000), C.c_void_p(0x2000)


def _coef(ncol, p):
    return np.zeros(max(ncol, 1) * (p + 1)).ctypes.data_as(C.POINTER(C.c_double))


def _cm(ctx=CTX, x=PTR, n=50, ld=None, p=5, coef=True, ncol=3, type=0, out=PTR):
    return _lib().oemgpu_predict_dev(ctx, x, n, n if ld is None else ld, p, _coef(ncol, p) if coef else None, ncol, type, out)


def _rm(ctx=CTX, x=PTR, dtype=0, n=50, ldr=None, p=5, coef=True, ncol=3, type=0, out=PTR):
    return _lib().oemgpu_predict_rm_dev(ctx, x, dtype, n, p if ldr is None else ldr, p, _coef(ncol, p) if coef else None, ncol, type, out)


def _sp(ctx=CTX, x=PTR, p=5, coef=True, ncol=3, type=0, out=PTR):
    return _lib().oemgpu_predict_sparse_res(ctx, x, _coef(ncol, p) if coef else None, ncol, type, out)


SHARED_BAD = {
    "NULL ctx": dict(ctx=None),
    "NULL x": dict(x=None),
    "NULL coef": dict(coef=False),
    "NULL out": dict(out=None),
    "ncol = 0": dict(ncol=0),
    "type -1": dict(type=-1),
    "type 3": dict(type=3),
}
DENSE_BAD = {"n = 0": dict(n=0), "p = 0": dict(p=0)}
CM_BAD = {"ld < n": dict(ld=49), "x on a 4-byte boundary": dict(x=C.c_void_p(0x2004))}
RM_BAD = {
    "ldr < p": dict(ldr=4),
    "dtype 2": dict(dtype=2),
    "dtype -1": dict(dtype=-1),
    "float64 x on a 4-byte boundary": dict(x=C.c_void_p(0x2004), dtype=0),
    "float32 x on a 2-byte boundary": dict(x=C.c_void_p(0x2002), dtype=1),
}
CASES = ([(_cm, "predict", w, kw) for w, kw in {**SHARED_BAD, **DENSE_BAD, **CM_BAD}.items()] +
         [(_rm, "predict_rm", w, kw) for w, kw in {**SHARED_BAD, **DENSE_BAD, **RM_BAD}.items()] +
         [(_sp, "predict_sparse", w, kw) for w, kw in SHARED_BAD.items()])


@pytest.mark.parametrize("call,name,what,kw", CASES, ids=[f"{n}-{w}" for _, n, w, _ in CASES])
def test_argument_errors_come_back_before_any_device_work(call, name, what, kw):
    assert call(**kw) == ERR_ARG, what
    msg = _lib().oemgpu_last_error().decode()
    assert msg.startswith(name + ":"), msg
    if what.startswith("type"):
        assert "type" in msg
    if what.startswith("dtype"):
        assert "OEMGPU_F64" in msg
    if what in ("ld < n", "ldr < p"):
        assert what in msg
    if "boundary" in what:
        assert "aligned" in msg


# ------------------------------------------------------------------------------------------ predict() on host inputs: as before
def _fit(family, p=6, nlam=7, seed=3):
    from oem_amd import api
    rng = np.random.default_rng(seed)
    fit = api.OemFit()
    fit["beta"] = [rng.standard_normal((p + 1, nlam)), rng.standard_normal((p + 1, nlam))]
    fit["lambda"] = [np.geomspace(1.0, 0.01, nlam), np.geomspace(2.0, 0.05, nlam)]
    fit["penalty"] = ["lasso", "mcp"]
    fit["family"] = family
    return fit


def _as_before(fit, newx, s, which_model, type):
    """the expression of predict()'s host path as it stood before the device path was added"""
    from oem_amd import api
    nbeta = np.array(fit["beta"][which_model])
    if s is not None:
        lam = np.asarray(fit["lambda"][which_model], dtype=np.float64)
        left, right, frac = api._lambda_interp(lam, np.atleast_1d(np.asarray(s, dtype=np.float64)))
        nbeta = nbeta[:, left] * frac + nbeta[:, right] * (1 - frac)
    if hasattr(newx, "tocsc"):
        import scipy.sparse as sp
        newx = sp.csc_matrix(newx, dtype=np.float64)
        if newx.shape[1] < nbeta.shape[0]:
            newx = sp.hstack([sp.csc_matrix(np.ones((newx.shape[0], 1))), newx], format="csc")
        nfit = np.asarray(newx @ nbeta)
    else:
        newx = np.asarray(newx, dtype=np.float64)
        if newx.shape[1] < nbeta.shape[0]:
            newx = np.column_stack([np.ones(newx.shape[0]), newx])
        nfit = newx @ nbeta
    if fit.get("family") == "binomial":
        if type == "response":
            return 1.0 / (1.0 + np.exp(-nfit))
        if type == "class":
            return np.where(nfit > 0, 1, 0)
    return nfit


@pytest.mark.parametrize("family", ["gaussian", "binomial"])
@pytest.mark.parametrize("kind", ["numpy", "numpy float32", "numpy with the intercept's column", "scipy", "cpu torch"])
def test_host_inputs_take_the_path_they_took(kind, family):
    import scipy.sparse as sp
    import torch
    from oem_amd import api
    rng = np.random.default_rng(11)
    x = rng.standard_normal((23, 6))
    x[rng.random(x.shape) < 0.5] = 0.0
    newx = {"numpy": x, "numpy float32": x.astype(np.float32), "numpy with the intercept's column": np.column_stack([np.ones(23), x]),
            "scipy": sp.csr_matrix(x), "cpu torch": torch.from_numpy(x.copy())}[kind]
    fit = _fit(family)
    for s in (None, 0.3, [0.5, 0.02, 0.0123, 5.0]):
        for which_model in (0, 1, "mcp"):
            for type in ("link", "response", "class"):
                got = api.predict(fit, newx, s=s, which_model=which_model, type=type)
                want = _as_before(fit, newx, s, 1 if which_model == "mcp" else which_model, type)
                assert isinstance(got, np.ndarray) and got.dtype == want.dtype and np.array_equal(got, want)


def test_the_policy_says_which_tensors_predict_reads_in_place():
    """_predict_rowmajor_in_place reads only dtype, shape and strides: CPU tensors pin it"""
    import torch
    from oem_amd import api
    from oem_amd import _lib as L
    x = torch.zeros((6, 4), dtype=torch.float64)
    assert api._predict_rowmajor_in_place(x) == L.OEMGPU_F64 and api._predict_rowmajor_in_place(x.float()) == L.OEMGPU_F32
    assert api._predict_rowmajor_in_place(torch.zeros((6, 9), dtype=torch.float32)[:, 1:5]) == L.OEMGPU_F32      # a row stride beyond p, an odd offset
    assert api._predict_rowmajor_in_place(torch.zeros((40, 30000))) == L.OEMGPU_F32                               # no limit on p, p > n
    assert api._predict_rowmajor_in_place(x.half()) is None
    assert api._predict_rowmajor_in_place(torch.zeros((4, 6), dtype=torch.float64).t()) is None                   # already column-major
    assert api._predict_rowmajor_in_place(torch.zeros((6, 8), dtype=torch.float64)[:, ::2]) is None               # strided in its columns
