"""The row-major binomial entries (oemgpu_fit_logistic_dense_rm_dev, oemgpu_fit_logistic_dense_fold_rm_dev,
oemgpu_logistic_cv_score_rm_dev), the part that needs no GPU: the exports, the refusals that come back before any device work, and
the band plan of the row pass (oemgpu_selftest_logistic_rm_plan) swept over every p the fit serves."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ["oemgpu_fit_logistic_dense_rm_dev", "oemgpu_fit_logistic_dense_fold_rm_dev", "oemgpu_logistic_cv_score_rm_dev"]
ERR_ARG, ERR_UNSUPPORTED = -1, -4
LDS_BYTES = 160 << 10          # LDS of a gfx950 CU
P_MAX = 8191


def _lib():
    import oem_amd
    return oem_amd.lib()


def test_entries_are_declared_exported_and_listed():
    import oem_amd
    from oem_amd import _lib as L
    header = (ROOT / "include" / "oemgpu.h").read_text()
    dyn = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES + ["oemgpu_selftest_logistic_rm_plan"]:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert re.search(r" T " + name + r"$", dyn, re.M), name
        assert name in oem_amd.EXPORTS
        assert getattr(_lib(), name).argtypes is not None


def _opts(p):
    from oem_amd import api
    return api._Args(["lasso"], [np.zeros(0)], 5, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(p), np.zeros(0, np.int32),
                     np.zeros(0, np.int32), np.zeros(0))


# a context and device pointers that are never dereferenced: every refusal below comes back before the device is touched
CTX, PTR = C.c_void_p(0x1000), C.c_void_p(0x2000)


def _fit(ctx=CTX, x=PTR, dtype=0, n=50, ldr=None, p=5, y=PTR, intercept=1, hf=0, irls_maxit=10, irls_tol=1e-3):
    a = _opts(p)
    return _lib().oemgpu_fit_logistic_dense_rm_dev(ctx, x, dtype, n, p if ldr is None else ldr, p, y, 1, intercept, hf, irls_maxit, irls_tol,
                                                   C.byref(a.c), *a.outputs(p + 1))


def _fold(ctx=CTX, x=PTR, dtype=0, n=50, ldr=None, p=5, y=PTR, foldid=PTR, nfolds=5, leave_out=1, intercept=1, hf=0, irls_maxit=10,
          irls_tol=1e-3):
    a = _opts(p)
    return _lib().oemgpu_fit_logistic_dense_fold_rm_dev(ctx, x, dtype, n, p if ldr is None else ldr, p, y, foldid, nfolds, leave_out, 1, intercept,
                                                        hf, irls_maxit, irls_tol, C.byref(a.c), *a.outputs(p + 1))


def _score(ctx=CTX, x=PTR, dtype=0, n=50, ldr=None, p=5, y=PTR, foldid=PTR, nfolds=5, ncol=3, coef=True, sums=True, counts=True):
    cf = np.zeros(nfolds * ncol * (p + 1)) if coef else None
    sm = np.zeros(nfolds * ncol * 8) if sums else None
    ct = np.zeros(nfolds, dtype=np.int64) if counts else None
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    return _lib().oemgpu_logistic_cv_score_rm_dev(ctx, x, dtype, n, p if ldr is None else ldr, p, y, 1.0, foldid, nfolds,
                                                  None if cf is None else cf.ctypes.data_as(dp), ncol, None if sm is None else sm.ctypes.data_as(dp),
                                                  None if ct is None else ct.ctypes.data_as(ip), None)


CALLS = [(_fit, "fit_logistic_dense_rm"), (_fold, "fit_logistic_dense_fold_rm"), (_score, "logistic_cv_score_rm")]

# what is wrong -> the arguments that say it; every one an OEMGPU_ERR_ARG of all three entries
BAD = {
    "NULL ctx": dict(ctx=None),
    "NULL x": dict(x=None),
    "NULL y": dict(y=None),
    "dtype 2": dict(dtype=2),
    "dtype -1": dict(dtype=-1),
    "ldr < p": dict(ldr=4),
    "float64 x on a 4-byte boundary": dict(x=C.c_void_p(0x2004), dtype=0),
    "float32 x on a 2-byte boundary": dict(x=C.c_void_p(0x2002), dtype=1),
    "n = 0": dict(n=0),
}


@pytest.mark.parametrize("what", list(BAD))
@pytest.mark.parametrize("call,name", CALLS, ids=[n for _, n in CALLS])
def test_argument_errors_come_back_before_any_device_work(call, name, what):
    assert call(**BAD[what]) == ERR_ARG, what
    msg = _lib().oemgpu_last_error().decode()
    assert name in msg or "fit_logistic_dense" in msg, msg      # (the shared checks speak in the column-major entry's name)
    if what.startswith("dtype"):
        assert "OEMGPU_F64" in msg
    if what == "ldr < p":
        assert "ldr < p" in msg
    if "boundary" in what:
        assert "aligned" in msg


def test_a_float32_x_on_a_4_byte_boundary_is_not_an_alignment_error():
    """element alignment is all that is asked: the same pointer passes the alignment check as float32 (and is then refused for its shape,
    so that the fake context is never used)"""
    assert _fit(x=C.c_void_p(0x2004), dtype=1, n=6, p=5) == ERR_UNSUPPORTED
    assert _fit(x=C.c_void_p(0x2004), dtype=0, n=50, p=5) == ERR_ARG


def test_the_fold_and_scoring_entries_keep_their_own_refusals():
    assert _fold(foldid=None) == ERR_ARG
    assert _fold(nfolds=2) == ERR_ARG and "nfolds must be bigger than 3" in _lib().oemgpu_last_error().decode()
    assert _fold(leave_out=6) == ERR_ARG and _fold(leave_out=-1) == ERR_ARG
    assert _score(foldid=None) == ERR_ARG and _score(coef=False) == ERR_ARG and _score(sums=False) == ERR_ARG and _score(counts=False) == ERR_ARG
    assert _score(nfolds=2) == ERR_ARG and _score(ncol=0) == ERR_ARG
    for call in (_fit, _fold):
        assert call(hf=2) == ERR_ARG and call(irls_maxit=0) == ERR_ARG and call(irls_tol=-1.0) == ERR_ARG


def test_null_outputs_are_argument_errors():
    lib = _lib()
    a = _opts(5)
    out = list(a.outputs(6))
    for k in range(len(out)):
        bad = list(out)
        bad[k] = None
        assert lib.oemgpu_fit_logistic_dense_rm_dev(CTX, PTR, 0, 50, 5, 5, PTR, 1, 1, 0, 10, 1e-3, C.byref(a.c), *bad) == ERR_ARG
        assert lib.oemgpu_fit_logistic_dense_fold_rm_dev(CTX, PTR, 0, 50, 5, 5, PTR, PTR, 5, 1, 1, 1, 0, 10, 1e-3, C.byref(a.c), *bad) == ERR_ARG
    assert lib.oemgpu_fit_logistic_dense_rm_dev(CTX, PTR, 0, 50, 5, 5, PTR, 1, 1, 0, 10, 1e-3, None, *out) == ERR_ARG


@pytest.mark.parametrize("dtype", [0, 1])
def test_shapes_the_fit_does_not_serve_are_refused_before_any_device_work(dtype):
    lib = _lib()
    for call in (_fit, _fold):
        assert call(dtype=dtype, n=6, p=5, intercept=1) == ERR_UNSUPPORTED        # p + intercept >= n: the reference's XWXt branch
        assert "XWXt" in lib.oemgpu_last_error().decode()
        assert call(dtype=dtype, n=5, p=5, intercept=0) == ERR_UNSUPPORTED
        assert call(dtype=dtype, n=10 * (P_MAX + 1), p=P_MAX + 1) == ERR_UNSUPPORTED
        assert str(P_MAX) in lib.oemgpu_last_error().decode()
    assert _score(dtype=dtype, n=10 * (P_MAX + 1), p=P_MAX + 1) == ERR_UNSUPPORTED
    assert str(P_MAX) in lib.oemgpu_last_error().decode()


def test_the_helper_says_which_tensors_the_binomial_entries_read_in_place():
    """_logistic_rowmajor_in_place reads only dtype, shape and strides: CPU tensors pin it"""
    import torch
    from oem_amd import api
    from oem_amd import _lib as L
    x = torch.zeros((6, 4), dtype=torch.float64)
    assert api._logistic_rowmajor_in_place(x) == L.OEMGPU_F64 and api._logistic_rowmajor_in_place(x.float()) == L.OEMGPU_F32
    assert api._logistic_rowmajor_in_place(torch.zeros((6, 9), dtype=torch.float32)[:, :4]) == L.OEMGPU_F32          # a row stride beyond p
    assert api._logistic_rowmajor_in_place(torch.zeros((4000, 2000))) == L.OEMGPU_F32                                 # no limit on p
    assert api._logistic_rowmajor_in_place(x.half()) is None
    assert api._logistic_rowmajor_in_place(torch.zeros((4, 6), dtype=torch.float64).t()) is None                      # already column-major
    assert api._logistic_rowmajor_in_place(torch.zeros((6, 8), dtype=torch.float64)[:, ::2]) is None                  # strided in its columns


def _plan(n, p, dtype, intercept, num_cu):
    out = (C.c_int64 * 8)()
    rc = _lib().oemgpu_selftest_logistic_rm_plan(n, p, dtype, intercept, num_cu, out)
    return rc, list(out)


@pytest.mark.parametrize("dtype", [0, 1])
def test_band_plan_sweep(dtype):
    """for EVERY p the fit serves: every column is in exactly one band, every band but the last is a multiple of 4 wide (the four eta
    partials carry across bands in their order), the p accumulators and the tile of the widest band fit the LDS of a CU, one band
    whenever that fits, and the band width falls as p grows"""
    widths = []
    for p in range(1, P_MAX + 1):
        rc, (nband, bw, last, lds, ch, nchunk, rbz, nzblk) = _plan(10 * P_MAX, p, dtype, 1, 256)
        assert rc == 0
        assert nband >= 1 and 1 <= last <= bw
        assert (nband - 1) * bw + last == p                      # bands [b bw, min(p, (b + 1) bw)) cover 0 .. p - 1 once each
        assert nband == 1 or bw % 4 == 0
        assert 8 * p + 8 * 65 * bw < lds <= LDS_BYTES
        if 8 * p + 8 * 65 * p + 4096 <= LDS_BYTES:
            assert nband == 1 and bw == p
        else:
            assert nband > 1 and 8 * p + 8 * 65 * (bw + 4) + 4096 > LDS_BYTES    # the widest band that fits
        widths.append(bw if nband > 1 else None)
    multi = [w for w in widths if w is not None]
    assert multi and all(a >= b for a, b in zip(multi, multi[1:])) and multi[-1] >= 64
    assert widths[:256] == [None] * 256                           # p <= 256 (a workgroup's threads): one band


@pytest.mark.parametrize("intercept", [0, 1])
def test_chunks_and_z_blocks_are_the_column_major_plans(intercept):
    lib = _lib()
    cm = (C.c_int64 * 8)()
    for n in (63, 64, 65, 129, 4097, 70001, 1_000_000, 3_000_017):
        for p in (2, 50, 192, 193, 480, 1024, 8191):
            if p + intercept >= n:
                continue
            for num_cu in (1, 80, 256):
                rc, out = _plan(n, p, 1, intercept, num_cu)
                assert rc == 0 and lib.oemgpu_selftest_logistic_plan(n, p, intercept, 0, num_cu, cm) == 0
                assert out[4:8] == list(cm)[0:4]


def test_plan_refusals():
    assert _plan(0, 4, 0, 1, 256)[0] == ERR_ARG and _plan(4, 0, 0, 1, 256)[0] == ERR_ARG and _plan(4, 4, 0, 1, 0)[0] == ERR_ARG
    assert _plan(100, 4, 2, 1, 256)[0] == ERR_ARG
    assert _lib().oemgpu_selftest_logistic_rm_plan(100, 4, 0, 1, 256, None) == ERR_ARG
    assert _plan(10 ** 6, P_MAX + 1, 0, 1, 256)[0] == ERR_UNSUPPORTED
