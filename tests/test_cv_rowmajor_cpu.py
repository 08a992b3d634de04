"""The row-major entries of xval.oem and Gaussian cv.oem (oemgpu_xval_dense_rm_dev, oemgpu_cv_fold_fits_rm_dev,
oemgpu_selftest_fold_gather_rm_dev), the part that needs no GPU: the exports, and the refusals that come back before any device work --
the column-major counterparts' own, and a dtype that is no code, ldr < p and an x that is not aligned to its element."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ["oemgpu_xval_dense_rm_dev", "oemgpu_cv_fold_fits_rm_dev", "oemgpu_selftest_fold_gather_rm_dev"]
ERR_ARG, ERR_UNSUPPORTED = -1, -4
I64 = C.POINTER(C.c_int64)


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
    from oem_amd import api
    assert callable(api.rowmajor_fold_order) and callable(api._xval_rowmajor_in_place)


def _opts(p):
    from oem_amd import api
    return api._Args(["lasso"], [np.zeros(0)], 5, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(p), np.zeros(0, np.int32),
                     np.zeros(0, np.int32), np.zeros(0))


# a context and device pointers that are never dereferenced: every refusal below comes back before the device is touched
CTX, PTR = C.c_void_p(0x1000), C.c_void_p(0x2000)


class Call:
    """one call of each entry on (ctx, x, dtype, n, ldr, p, y, foldid, nfolds); `drop`: the index of an output pointer passed as NULL"""

    def __init__(self, p):
        self.p = max(p, 2)
        self.a = _opts(self.p)
        self.cv = np.zeros((2, 1, 5))
        self.fn = np.zeros(512, dtype=np.int64)

    def xval(self, ctx, x, dt, n, ldr, p, y, fid, K, drop=None, opts=True):
        out = list(self.a.outputs(self.p + 1)) + [self.cv[0].ctypes.data_as(C.POINTER(C.c_double)), self.cv[1].ctypes.data_as(C.POINTER(C.c_double))]
        if drop is not None:
            out[drop] = None
        rc = _lib().oemgpu_xval_dense_rm_dev(ctx, x, dt, n, ldr, p, y, None, fid, K, 1, 1, 0, C.byref(self.a.c) if opts else None, *out)
        return rc, _lib().oemgpu_last_error().decode()

    def fits(self, ctx, x, dt, n, ldr, p, y, fid, K, drop=None, opts=True):
        out = list(self.a.outputs(self.p + 1)) + [self.fn.ctypes.data_as(I64)]
        if drop is not None:
            out[drop] = None
        rc = _lib().oemgpu_cv_fold_fits_rm_dev(ctx, x, dt, n, ldr, p, y, fid, K, 1, 1, C.byref(self.a.c) if opts else None, *out)
        return rc, _lib().oemgpu_last_error().decode()

    def gather(self, ctx, x, dt, n, ldr, p, y, fid, K, drop=None, ldo=None):
        out = [PTR, (n + 16 * K + 15) // 16 * 16 if ldo is None else ldo, PTR, self.fn.ctypes.data_as(I64), self.fn[256:].ctypes.data_as(I64)]
        if drop is not None:
            out[drop] = None
        rc = _lib().oemgpu_selftest_fold_gather_rm_dev(ctx, x, dt, n, ldr, p, y, fid, K, *out)
        return rc, _lib().oemgpu_last_error().decode()


# (ctx, x, dtype, n, ldr, p, y, foldid, nfolds): what is wrong, and a word of the message
BAD = [
    ((None, PTR, 0, 100, 4, 4, PTR, PTR, 5), "NULL ctx", "NULL argument"),
    ((CTX, None, 0, 100, 4, 4, PTR, PTR, 5), "NULL x", "NULL argument"),
    ((CTX, PTR, 0, 100, 4, 4, None, PTR, 5), "NULL y", "NULL argument"),
    ((CTX, PTR, 0, 100, 4, 4, PTR, None, 5), "NULL foldid", "NULL argument"),
    ((CTX, PTR, 2, 100, 4, 4, PTR, PTR, 5), "dtype 2", "neither OEMGPU_F64 nor OEMGPU_F32"),
    ((CTX, PTR, -1, 100, 4, 4, PTR, PTR, 5), "dtype -1", "neither OEMGPU_F64 nor OEMGPU_F32"),
    ((CTX, PTR, 1, 100, 3, 4, PTR, PTR, 5), "ldr = p - 1", "ldr"),
    ((CTX, C.c_void_p(0x2004), 0, 100, 4, 4, PTR, PTR, 5), "a float64 x at an odd multiple of 4", "not aligned"),
    ((CTX, C.c_void_p(0x2002), 1, 100, 4, 4, PTR, PTR, 5), "a float32 x at an odd multiple of 2", "not aligned"),
    ((CTX, PTR, 0, 100, 4, 4, PTR, PTR, 1), "nfolds 1", "nfolds must be in 2..512"),
    ((CTX, PTR, 1, 100000, 4, 4, PTR, PTR, 513), "nfolds 513", "nfolds must be in 2..512"),
    ((CTX, PTR, 0, 0, 4, 4, PTR, PTR, 5), "n = 0", "bad n"),
    ((CTX, PTR, 0, 2 ** 31 - 80, 4, 4, PTR, PTR, 5), "n + 16 nfolds = 2^31", "32-bit row positions"),
]


@pytest.mark.parametrize("args,what,word", BAD, ids=[w for _, w, _ in BAD])
def test_argument_errors_come_back_before_any_device_work(args, what, word):
    k = Call(args[5])
    for call in (k.xval, k.fits, k.gather):
        rc, msg = call(*args)
        assert rc == (ERR_UNSUPPORTED if "32-bit" in word else ERR_ARG), (what, call.__name__, rc, msg)
        assert word in msg, (what, call.__name__, msg)


def test_a_float32_pointer_on_a_4_byte_boundary_is_not_an_alignment_error():
    """the call goes on to the next check (here: nfolds), which a misaligned x never reaches"""
    k = Call(4)
    x4 = C.c_void_p(0x2004)
    for call in (k.xval, k.fits, k.gather):
        rc, msg = call(CTX, x4, 1, 100, 4, 4, PTR, PTR, 1)
        assert rc == ERR_ARG and "nfolds must be in 2..512" in msg and "aligned" not in msg, (call.__name__, msg)
        rc, msg = call(CTX, x4, 0, 100, 4, 4, PTR, PTR, 1)
        assert rc == ERR_ARG and "not aligned" in msg, (call.__name__, msg)


def test_null_outputs_and_options_are_argument_errors():
    k = Call(4)
    ok = (CTX, PTR, 0, 100, 4, 4, PTR, PTR, 5)
    for drop in range(7):
        rc, msg = k.xval(*ok, drop=drop)
        assert rc == ERR_ARG and "NULL argument" in msg, (drop, msg)
    for drop in range(6):
        rc, msg = k.fits(*ok, drop=drop)
        assert rc == ERR_ARG and "NULL argument" in msg, (drop, msg)
    for drop in (0, 2, 3, 4):
        rc, msg = k.gather(*ok, drop=drop)
        assert rc == ERR_ARG and "NULL argument" in msg, (drop, msg)
    assert k.xval(*ok, opts=False)[0] == ERR_ARG
    assert k.fits(*ok, opts=False)[0] == ERR_ARG
    rc, msg = k.gather(*ok, ldo=(100 + 16 * 5 + 15) // 16 * 16 - 16)
    assert rc == ERR_ARG and "ldo" in msg


def test_too_few_rows_are_refused_as_by_the_column_major_entries():
    """xval.oem: n <= p; the fold fits: n - ceil(n / K) <= p, the largest fold then leaves no more rows than columns whatever the ids are.
    The codes and messages are the column-major entries' own.  (A shape that passes these checks goes on to the device, so the serving
    side of the boundary is in tests/test_gpu_cv_rowmajor.py.)"""
    k = Call(40)
    rc, msg = k.xval(CTX, PTR, 1, 40, 40, 40, PTR, PTR, 5)
    assert rc == ERR_UNSUPPORTED and msg == "dimension of x larger than number of observations"
    lib = _lib()
    a = _opts(40)
    cv = np.zeros((2, 1, 5))
    ref = lib.oemgpu_xval_dense_dev(CTX, PTR, 40, 40, 40, PTR, None, PTR, 5, 1, 1, 0, C.byref(a.c), *a.outputs(41),
                                    cv[0].ctypes.data_as(C.POINTER(C.c_double)), cv[1].ctypes.data_as(C.POINTER(C.c_double)))
    assert ref == rc and lib.oemgpu_last_error().decode() == msg
    # 50 rows in 5 folds: 50 - 10 = 40 <= p
    rc, msg = k.fits(CTX, PTR, 0, 50, 47, 40, PTR, PTR, 5)
    assert rc == ERR_UNSUPPORTED and "50 rows in 5 folds leave some fold no more rows than the 40 columns" in msg
    a = _opts(40)
    fn = np.zeros(5, dtype=np.int64)
    ref = lib.oemgpu_cv_fold_fits_dev(CTX, PTR, 50, 50, 40, PTR, PTR, 5, 1, 1, C.byref(a.c), *a.outputs(41), fn.ctypes.data_as(I64))
    assert ref == rc and lib.oemgpu_last_error().decode() == msg
    # 51 rows in 5 folds: 51 - 11 = 40 <= p still; 52 - 11 = 41 > p passes this check (and would go on to the device: not called here)
    assert k.fits(CTX, PTR, 0, 51, 47, 40, PTR, PTR, 5)[0] == ERR_UNSUPPORTED


def test_the_helper_takes_what_the_binomial_helper_takes():
    import torch
    from oem_amd import api
    from oem_amd import _lib as L
    x = torch.zeros((6, 4), dtype=torch.float64)
    assert api._xval_rowmajor_in_place(x) == L.OEMGPU_F64 and api._xval_rowmajor_in_place(x.float()) == L.OEMGPU_F32
    assert api._xval_rowmajor_in_place(torch.zeros((6, 9), dtype=torch.float32)[:, :4]) == L.OEMGPU_F32          # a row stride beyond p
    assert api._xval_rowmajor_in_place(torch.zeros((4000, 2000))) == L.OEMGPU_F32                                 # no limit on p
    assert api._xval_rowmajor_in_place(x.half()) is None
    assert api._xval_rowmajor_in_place(torch.zeros((4, 6), dtype=torch.float64).t()) is None                      # already column-major
    assert api._xval_rowmajor_in_place(torch.zeros((6, 8), dtype=torch.float64)[:, ::2]) is None                  # strided in its columns
