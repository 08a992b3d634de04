"""The launch plan of xval.oem's CV-error kernel (oem_amd/csrc/xval.hip: cv_error_plan, reported by oemgpu_selftest_xval_cv_plan), the
part that needs no GPU: its invariants over p, the number of lambdas, the folds, the penalties and the CU count; the shapes that
tests/test_gpu_xval_bounds.py runs, pinned to the branch each is named for; and the argument errors of the plan entry and of
oemgpu_selftest_xval_cv_error_dev, which come back before a device is looked for."""
import ctypes as C

import numpy as np
import pytest

LDS_MAX = 140 * 1024           # the coefficient tile of a pass stays in LDS up to here
KCH = 112                      # coefficient rows per LDS chunk
SINGLE, MULTI, CHUNK = 0, 1, 2

# (p, nlambda) -> (form, lt, passes, chunks, columns of the last chunk): the cases of tests/test_gpu_xval_bounds.py
PINNED = {
    (3, 1): (SINGLE, 1, 1, 1, 4),
    (55, 112): (SINGLE, 7, 1, 1, 56),
    (56, 113): (MULTI, 4, 2, 1, 60),
    (159, 112): (MULTI, 7, 1, 1, 160),         # LDS = 143 360, the limit itself
    (160, 112): (CHUNK, 7, 1, 2, 52),
    (223, 112): (CHUNK, 7, 1, 2, 112),
    (224, 100): (CHUNK, 7, 1, 3, 4),
    (280, 64): (CHUNK, 4, 1, 3, 60),
    (230, 224): (CHUNK, 7, 2, 3, 8),
    (1119, 16): (MULTI, 1, 1, 1, 1120),        # LDS at the limit
    (1120, 16): (CHUNK, 1, 1, 11, 4),
    (20, 225): (SINGLE, 5, 3, 1, 24),
    (20, 250): (SINGLE, 6, 3, 1, 24),          # 16 tiles: the last pass holds 2 tiles beyond them
    (40, 129): (SINGLE, 5, 2, 1, 44),          # 9 tiles: the last pass is one tile short
    (7, 32): (SINGLE, 2, 1, 1, 8),             # p + 1 = 8 fills a k-step
    (8, 48): (SINGLE, 3, 1, 1, 12),            # p + 1 = 9 opens one for the intercept alone
}


def _lib():
    import oem_amd
    return oem_amd.lib()


def _plan(L, n, p, K, npen, nl, num_cu, out=None):
    out = (C.c_int64 * 7)() if out is None else out
    assert L.oemgpu_selftest_xval_cv_plan(n, p, K, npen, nl, num_cu, out) == 0, (n, p, K, npen, nl, num_cu)
    return tuple(out)


def _ps():
    return list(range(1, 601)) + sorted(set(range(600, 5001, 37)) | {1119, 1120, 1183, 1184, 4999, 5000})


def _nls():
    return sorted(set(range(1, 131)) | {16 * k + d for k in range(8, 38) for d in (-1, 0, 1) if 16 * k + d <= 600})


@pytest.mark.parametrize("grid", ["every p", "every nlambda"])
def test_plan_over_p_and_nlambda(grid):
    """every p to 600 (then strided to 5000) against every nlambda to 130 and the neighbours of every multiple of 16 to 600; every nlambda
    from 1 to 600 against the p on either side of a k-step, of SINGLE's 56 columns, of a chunk and of the LDS limit at every lt"""
    L = _lib()
    out = (C.c_int64 * 7)()
    if grid == "every p":
        ps, nls = _ps(), _nls()
    else:
        edge = {LDS_MAX // (128 * lt) - 1 + d for lt in range(1, 8) for d in (-4, -1, 0, 1, 4)}      # K4 = 1120 / lt
        ps, nls = sorted({1, 2, 3, 4, 7, 8, 54, 55, 56, 57, 110, 111, 112, 222, 223, 224, 5000} | edge), list(range(1, 601))
    P = np.empty((len(ps), len(nls), 7), dtype=np.int64)
    for i, p in enumerate(ps):
        for j, nl in enumerate(nls):
            assert L.oemgpu_selftest_xval_cv_plan(700, p, 3, 1, nl, 256, out) == 0
            P[i, j] = out
    lt, passes, form, lds, chunks, last, nwg = (P[..., k] for k in range(7))
    K4 = ((np.array(ps) + 4) // 4 * 4)[:, None] + 0 * lt
    nl = np.array(nls)[None, :] + 0 * lt
    ntile = (nl + 15) // 16
    assert lt.min() >= 1 and lt.max() <= 7
    assert np.all(passes * lt >= ntile) and np.all(ntile > (passes - 1) * lt)
    assert np.all(passes[nl <= 112] == 1) and np.all(lt[nl <= 112] == ntile[nl <= 112])
    assert np.all(passes == -(-ntile // 7))                       # the fewest passes of at most 7 tiles ...
    assert np.all(lt == -(-ntile // passes))                      # ... made even
    assert lds.max() <= LDS_MAX and lds.min() > 0
    chunk = K4 * 16 * lt * 8 > LDS_MAX
    assert np.array_equal(form == CHUNK, chunk)
    assert np.array_equal(form == SINGLE, ~chunk & (K4 <= 56))
    assert np.all((form == SINGLE) | (form == MULTI) | (form == CHUNK))
    assert np.all(lds[~chunk] == (K4 * 16 * lt * 8)[~chunk]) and np.all(lds[chunk] == (KCH * 16 * lt * 8)[chunk])
    assert np.all(chunks[~chunk] == 1) and np.all(last[~chunk] == K4[~chunk])
    assert np.all(chunks[chunk] == -(-K4[chunk] // KCH))
    assert np.all((chunks - 1) * KCH + last == K4)
    assert np.all(last[chunk] >= 4) and np.all(last[chunk] <= KCH) and np.all(last % 4 == 0)
    assert {SINGLE, MULTI, CHUNK} == set(np.unique(form)) and set(np.unique(lt)) == set(range(1, 8))
    assert chunk[:, nl[0] == 100].any() and (chunks[chunk].max() > 40)
    if grid == "every nlambda":
        assert passes.max() == 6 and all(np.any(chunk & (lt == t)) and np.any(~chunk & (lt == t)) for t in range(1, 8))
    assert np.all(nwg >= 1)


@pytest.mark.parametrize("num_cu", [1, 64, 256, 304])
def test_plan_grid(num_cu):
    """workgroups per (fold, penalty): never more than the CUs hold at once unless one per (fold, penalty) already is, never more than
    the row tiles of an average fold; and the folds, penalties, rows and CUs do not touch the lambda / coefficient side of the plan"""
    L = _lib()
    out = (C.c_int64 * 7)()
    seen = set()
    for K in (2, 3, 10, 130, 512):
        for npen in (1, 2, 3, 4):
            for n in (1, 2, 100, 127 * K, 128 * K, 128 * K + 1, 700, 3000, 4000, 10 ** 6, 2 ** 31 - 16 * 512 - 1):
                for p, nl in ((20, 40), (160, 112), (1120, 16), (20, 250)):
                    P = _plan(L, n, p, K, npen, nl, num_cu, out)
                    nwg = P[6]
                    assert nwg >= 1 and nwg * K * npen <= max(num_cu, K * npen), (P, n, K, npen)
                    tiles = -(-(n // K) // 128)
                    assert nwg == max(1, min(num_cu // (K * npen), tiles)), (P, n, K, npen)
                    assert P[:6] == _plan(L, 700, p, 3, 1, nl, 256)[:6]
                    seen.add(nwg)
    assert 1 in seen and (num_cu == 1 or max(seen) > 1)


def test_pinned_shapes():
    L = _lib()
    for (p, nl), (form, lt, passes, chunks, last) in PINNED.items():
        P = _plan(L, 700, p, 3, 1, nl, 256)
        assert (P[2], P[0], P[1], P[4], P[5]) == (form, lt, passes, chunks, last), (p, nl, P)
    assert _plan(L, 700, 159, 3, 1, 112, 256)[3] == 143360 == LDS_MAX
    assert _plan(L, 400, 1119, 3, 1, 16, 256)[3] == 143360
    assert _plan(L, 700, 160, 3, 1, 112, 256)[3] == KCH * 16 * 7 * 8
    lt, passes = _plan(L, 700, 20, 3, 1, 250, 256)[:2]
    assert passes * lt - 16 == 2                                 # two tiles of the last pass lie beyond the 16 there are
    lt, passes = _plan(L, 700, 40, 3, 1, 129, 256)[:2]
    assert passes * lt - 9 == 1                                  # the last pass is one tile short


def test_plan_argument_errors():
    L = _lib()
    out = (C.c_int64 * 7)()
    for n, p, K, npen, nl, cu in ((0, 5, 3, 1, 10, 256), (-1, 5, 3, 1, 10, 256), (100, 0, 3, 1, 10, 256), (100, 5, 3, 0, 10, 256),
                                  (100, 5, 3, 1, 0, 256), (100, 5, 3, 1, 10, 0), (100, 5, 1, 1, 10, 256), (100, 5, 513, 1, 10, 256),
                                  (100, 5, 0, 1, 10, 256), (100, 5, -3, 1, 10, 256)):
        assert L.oemgpu_selftest_xval_cv_plan(n, p, K, npen, nl, cu, out) == -1, (n, p, K, npen, nl, cu)
        assert L.oemgpu_last_error()
    assert L.oemgpu_selftest_xval_cv_plan(100, 5, 513, 1, 10, 256, out) == -1 and b"nfolds" in L.oemgpu_last_error()
    assert L.oemgpu_selftest_xval_cv_plan(100, 5, 3, 1, 10, 256, None) == -1
    assert L.oemgpu_selftest_xval_cv_plan(100, 5, 2, 1, 10, 256, out) == 0 and L.oemgpu_selftest_xval_cv_plan(100, 5, 512, 1, 10, 256, out) == 0


def test_cv_error_entry_argument_errors_before_any_device():
    """a NULL context or pointer, non-positive sizes, nfolds outside 2..512, a type_measure that is neither, ld < n: -1 whatever else is
    handed over -- the context and the device pointers are never looked at (they point at host scratch here)"""
    L = _lib()
    scratch = (C.c_double * 64)()
    ptr = C.addressof(scratch)
    dp = C.cast(scratch, C.POINTER(C.c_double))

    def call(ctx=ptr, x=ptr, n=50, ld=50, p=4, y=ptr, w=None, fid=ptr, K=5, coef=dp, npen=1, nl=3, tm=0, cvm=dp, cvsd=dp, tri=None):
        return L.oemgpu_selftest_xval_cv_error_dev(ctx, x, n, ld, p, y, w, fid, K, coef, npen, nl, tm, cvm, cvsd, tri)
    for kw in (dict(ctx=None), dict(x=None), dict(y=None), dict(fid=None), dict(coef=None), dict(cvm=None), dict(cvsd=None)):
        assert call(**kw) == -1, kw
        assert b"NULL" in L.oemgpu_last_error()
    for kw in (dict(p=0), dict(npen=0), dict(nl=0), dict(n=0), dict(ld=49), dict(tm=2), dict(tm=-1)):
        assert call(**kw) == -1, kw
    for K in (1, 513, 0, -2):
        assert call(K=K) == -1
        assert b"nfolds" in L.oemgpu_last_error()
    assert call(n=2 ** 31 - 80, ld=2 ** 31 - 80) == -4          # 32-bit row positions, as in oemgpu_xval_dense_dev
