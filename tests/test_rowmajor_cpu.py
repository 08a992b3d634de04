"""The row-major entries (oemgpu_shift_sums_rm_dev, oemgpu_moments_rm_dev, oemgpu_fit_dense_rm_dev), the part that needs no GPU: the
exports, the refusals that come back before any device work, and the launch plan of the moment pass across its boundaries."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ["oemgpu_shift_sums_rm_dev", "oemgpu_moments_rm_dev", "oemgpu_fit_dense_rm_dev"]
ERR_ARG, ERR_UNSUPPORTED = -1, -4


def _lib():
    import oem_amd
    return oem_amd.lib()


def test_entries_are_declared_exported_and_listed():
    import oem_amd
    from oem_amd import _lib as L
    header = (ROOT / "include" / "oemgpu.h").read_text()
    dyn = subprocess.run(["nm", "-D", "--defined-only", str(L.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES + ["oemgpu_selftest_gram_rm_plan"]:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert re.search(r" T " + name + r"$", dyn, re.M), name
        assert name in oem_amd.EXPORTS
        assert getattr(_lib(), name).argtypes is not None
    assert re.search(r"#define OEMGPU_F64 0\b", header) and re.search(r"#define OEMGPU_F32 1\b", header)
    assert (L.OEMGPU_F64, L.OEMGPU_F32) == (0, 1)
    assert int(re.search(r"#define OEMGPU_RM_P_MAX (\d+)", header).group(1)) == L.RM_P_MAX >= 512


def _opts(p):
    """(struct, keepalive) of a one-penalty lasso call on p columns"""
    from oem_amd import api
    a = api._Args(["lasso"], [np.zeros(0)], 5, 1e-3, 1.0, 3.0, 0.5, 1e-7, 100, False, False, np.ones(p), np.zeros(0, np.int32),
                  np.zeros(0, np.int32), np.zeros(0))
    return a


# a context and device pointers that are never dereferenced: every refusal below comes back before the device is touched
CTX, PTR = C.c_void_p(0x1000), C.c_void_p(0x2000)

# (ctx, x, dtype, n, ldr, p, y): what is wrong
BAD = [
    ((None, PTR, 0, 10, 4, 4, PTR), "NULL ctx"),
    ((CTX, None, 0, 10, 4, 4, PTR), "NULL x"),
    ((CTX, PTR, 0, 10, 4, 4, None), "NULL y"),
    ((CTX, PTR, 2, 10, 4, 4, PTR), "dtype 2"),
    ((CTX, PTR, -1, 10, 4, 4, PTR), "dtype -1"),
    ((CTX, PTR, 1, 0, 4, 4, PTR), "n = 0"),
    ((CTX, PTR, 0, 10, 4, 0, PTR), "p = 0"),
    ((CTX, PTR, 1, 10, 3, 4, PTR), "ldr < p"),
    ((CTX, C.c_void_p(0x2004), 0, 10, 4, 4, PTR), "a float64 x at an odd multiple of 4"),
    ((CTX, C.c_void_p(0x2002), 1, 10, 4, 4, PTR), "a float32 x at an odd multiple of 2"),
]


@pytest.mark.parametrize("args,what", BAD, ids=[w for _, w in BAD])
def test_argument_errors_come_back_before_any_device_work(args, what):
    lib = _lib()
    ctx, x, dt, n, ldr, p, y = args
    assert lib.oemgpu_shift_sums_rm_dev(ctx, x, dt, n, ldr, p, y, PTR) == ERR_ARG, what
    assert "shift_sums_rm" in lib.oemgpu_last_error().decode()
    assert lib.oemgpu_moments_rm_dev(ctx, x, dt, n, ldr, p, y, None, PTR) == ERR_ARG, what
    assert "moments_rm" in lib.oemgpu_last_error().decode()
    a = _opts(max(p, 2))
    assert lib.oemgpu_fit_dense_rm_dev(ctx, x, dt, n, ldr, p, y, 1, 1, C.byref(a.c), *a.outputs(max(p, 2) + 1)) == ERR_ARG, what
    assert "fit_dense_rm" in lib.oemgpu_last_error().decode()


def test_null_outputs_are_argument_errors():
    lib = _lib()
    assert lib.oemgpu_shift_sums_rm_dev(CTX, PTR, 0, 10, 4, 4, PTR, None) == ERR_ARG
    assert lib.oemgpu_moments_rm_dev(CTX, PTR, 0, 10, 4, 4, PTR, None, None) == ERR_ARG
    a = _opts(4)
    out = list(a.outputs(5))
    for k in range(len(out)):
        bad = list(out); bad[k] = None
        assert lib.oemgpu_fit_dense_rm_dev(CTX, PTR, 0, 10, 4, 4, PTR, 1, 1, C.byref(a.c), *bad) == ERR_ARG
    assert lib.oemgpu_fit_dense_rm_dev(CTX, PTR, 0, 10, 4, 4, PTR, 1, 1, None, *out) == ERR_ARG


def test_shapes_of_the_column_major_entry_are_refused_by_name():
    """p above the limit, and a p >= n shape of the wide engine (500 x 2500): OEMGPU_ERR_UNSUPPORTED before any device work, and the
    message says where such a matrix goes"""
    from oem_amd import _lib as L
    lib = _lib()
    p = L.RM_P_MAX + 1
    a = _opts(p)
    assert lib.oemgpu_fit_dense_rm_dev(CTX, PTR, 0, 10 * p, p, p, PTR, 1, 1, C.byref(a.c), *a.outputs(p + 1)) == ERR_UNSUPPORTED
    assert "column-major entry" in lib.oemgpu_last_error().decode()
    assert lib.oemgpu_moments_rm_dev(CTX, PTR, 0, 10 * p, p, p, PTR, None, PTR) == ERR_UNSUPPORTED
    assert "column-major entry" in lib.oemgpu_last_error().decode()
    a = _opts(2500)
    assert lib.oemgpu_fit_dense_rm_dev(CTX, PTR, 1, 500, 2500, 2500, PTR, 1, 1, C.byref(a.c), *a.outputs(2501)) == ERR_UNSUPPORTED
    msg = lib.oemgpu_last_error().decode()
    assert "p >= n" in msg and "oemgpu_fit_dense_dev" in msg


def test_the_helper_says_which_tensors_oem_reads_in_place():
    """_rowmajor_in_place reads only dtype, shape and strides: CPU tensors pin it"""
    import torch
    from oem_amd import api
    from oem_amd import _lib as L
    x = torch.zeros((6, 4), dtype=torch.float64)
    assert api._rowmajor_in_place(x) == L.OEMGPU_F64 and api._rowmajor_in_place(x.float()) == L.OEMGPU_F32
    assert api._rowmajor_in_place(torch.zeros((6, 9), dtype=torch.float32)[:, :4]) == L.OEMGPU_F32          # a row stride beyond p
    assert api._rowmajor_in_place(x.half()) is None
    assert api._rowmajor_in_place(torch.zeros((4, 6), dtype=torch.float64).t()) is None                      # already column-major
    assert api._rowmajor_in_place(torch.zeros((6, 8), dtype=torch.float64)[:, ::2]) is None                  # strided in its columns
    assert api._rowmajor_in_place(torch.zeros((4, 4), dtype=torch.float64)) is None                          # n <= p: the p >= n engines
    assert api._rowmajor_in_place(torch.zeros((4, 6), dtype=torch.float32)) is None
    assert api._rowmajor_in_place(torch.zeros((L.RM_P_MAX + 1, L.RM_P_MAX), dtype=torch.float32)) == L.OEMGPU_F32
    assert api._rowmajor_in_place(torch.zeros((L.RM_P_MAX + 2, L.RM_P_MAX + 1), dtype=torch.float32)) is None   # p beyond the row-major pass


def test_a_float32_x_on_a_4_byte_boundary_is_not_an_alignment_error():
    """element alignment is all that is asked: the same pointer passes as float32 (and is then refused for its shape, so that the fake
    context is never used)"""
    lib = _lib()
    from oem_amd import _lib as L
    x4 = C.c_void_p(0x2004)
    p = L.RM_P_MAX + 1
    assert lib.oemgpu_moments_rm_dev(CTX, x4, 1, 10 * p, p, p, PTR, None, PTR) == ERR_UNSUPPORTED
    assert lib.oemgpu_moments_rm_dev(CTX, x4, 0, 10 * p, p, p, PTR, None, PTR) == ERR_ARG
    assert "aligned" in lib.oemgpu_last_error().decode()


def _plan(n, p, num_cu):
    out = (C.c_int64 * 8)()
    rc = _lib().oemgpu_selftest_gram_rm_plan(n, p, num_cu, out)
    return rc, list(out)


NS = [1, 3, 15, 16, 17, 63, 64, 65, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4099, 70001, 10 ** 6, 10 ** 6 + 1, 12_500_000, 2 ** 31 + 5, 2 ** 36]
PS = [1, 2, 13, 14, 15, 30, 31, 62, 63, 64, 100, 126, 127, 130, 257, 510, 511, 512, 1022, 1023, 1024]


@pytest.mark.parametrize("num_cu", [1, 8, 256, 304])
def test_plan_sweep(num_cu):
    """every row is in exactly one chunk, no chunk is empty, a chunk is whole 16-row steps, the workgroups stay near four per CU, a
    chunk is no shorter than 1024 rows unless the matrix is, and the tile / block counts are those of [X | y | 1]"""
    for n in NS:
        for p in PS:
            rc, (ntc, nblk, nchunk, steps, nwg, tpart, last_row, pmax) = _plan(n, p, num_cu)
            assert rc == 0
            assert ntc == -(-(p + 2) // 16)
            nb = -(-ntc // 4)
            assert nblk == nb * (nb + 1) // 2
            nstep = -(-n // 16)
            assert nchunk >= 1 and steps >= 1
            assert nchunk * steps >= nstep > (nchunk - 1) * steps            # covers every row; the last chunk is not empty
            assert last_row == (nchunk - 1) * steps * 16 < n
            assert nwg == nchunk * nblk
            assert tpart == nwg * 16 * 256
            # about four workgroups per CU; more only to keep a chunk under 16 MiB of float64 rows, and then the partials under 512 MiB
            cap = max(1024, (16 << 20) // (8 * (p + 2)))
            target = -(-4 * num_cu // nblk)
            assert nchunk <= max(1, target, min(-(-n // cap), (512 << 20) // (nblk * 32768)))
            assert tpart * 8 <= max(512 << 20, target * nblk * 32768)
            assert nchunk == 1 or steps * 16 >= 1024
            assert nwg < 2 ** 31 and pmax == 1024
    # the plan's boundaries in n: one chunk below 2048 rows, then two
    assert _plan(2047, 100, 256)[1][2] == 1 and _plan(2048, 100, 256)[1][2] == 2
    # the three shapes of tools/time_rowmajor.py on 256 CUs: (blocks, chunks, 16-row steps per chunk)
    assert [_plan(n, p, 256)[1][1:4] for n, p in ((10 ** 6, 100), (10 ** 6, 512), (12_500_000, 256))] == [[3, 342, 183], [45, 246, 255], [15, 1092, 716]]
    # ... and in p: the block grid grows at p + 2 = 64 k + 1
    assert [_plan(10 ** 6, p, 256)[1][1] for p in (62, 63, 126, 127)] == [1, 3, 3, 6]


def test_plan_refusals():
    assert _plan(0, 4, 256)[0] == ERR_ARG and _plan(4, 0, 256)[0] == ERR_ARG and _plan(4, 4, 0)[0] == ERR_ARG
    assert _lib().oemgpu_selftest_gram_rm_plan(4, 4, 256, None) == ERR_ARG
    assert _plan(10 ** 6, 1025, 256)[0] == ERR_UNSUPPORTED
