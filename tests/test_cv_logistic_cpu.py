"""cv.oem for binomial fits, the part that needs no GPU: the C entries are declared, exported and bound; their argument errors
come back before a device is looked for; the scoring entry's launch plan (oemgpu_selftest_cv_score_plan) holds its invariants over
n, p, ncol and the CU count; the restatement's error terms (tests/cv_logistic_restatement.py) are scikit-learn's; and
cv_oem(family="binomial") makes oem()'s check of y."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import cv_logistic_restatement as CV

ROOT = Path(__file__).resolve().parent.parent
NEW = ("oemgpu_fit_logistic_dense_fold_dev", "oemgpu_logistic_cv_score_dev", "oemgpu_selftest_cv_score_plan")
LDS_BYTES = 160 << 10          # LDS of a gfx950 CU


def test_new_symbols_are_declared_exported_and_bound():
    import oem_amd
    h = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "oemgpu.h").read_text(), flags=re.S)
    L = oem_amd.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, h), name
        assert hasattr(L, name), name
        assert name in oem_amd.EXPORTS, name


def _opts(p, nlambda=5):
    from oem_amd import api
    return api._Args(["lasso"], [], nlambda, 1e-4, 1.0, 3.0, 0.5, 1e-7, 500, False, False, np.ones(p), np.zeros(0, np.int32),
                     np.zeros(0, np.int32), np.zeros(0))


def test_fold_entry_argument_errors_before_any_device():
    """a NULL foldid, nfolds < 3 and leave_out outside [0, nfolds] are -1 whatever else is handed over: the context and the device
    pointers are never looked at (they point at host scratch here)"""
    import oem_amd
    L = oem_amd.lib()
    n, p = 50, 4
    a = _opts(p)
    out = a.outputs(p + 1)
    scratch = (C.c_double * 64)()
    ptr = C.addressof(scratch)

    def call(foldid, nfolds, leave_out):
        return L.oemgpu_fit_logistic_dense_fold_dev(ptr, ptr, n, n, p, ptr, foldid, nfolds, leave_out, 1, 1, 0, 100, 1e-3, C.byref(a.c), *out)
    assert call(None, 5, 1) == -1
    assert b"NULL" in L.oemgpu_last_error()
    assert call(ptr, 2, 1) == -1
    assert b"nfolds" in L.oemgpu_last_error()
    assert call(ptr, 5, -1) == -1
    assert call(ptr, 5, 6) == -1
    assert b"leave_out" in L.oemgpu_last_error()
    # then the fit's own host-side checks, still without a device: p + intercept >= n is -4
    assert L.oemgpu_fit_logistic_dense_fold_dev(ptr, ptr, 5, 5, p, ptr, ptr, 5, 1, 1, 1, 0, 100, 1e-3, C.byref(a.c), *out) == -4


def test_score_entry_argument_errors_before_any_device():
    import oem_amd
    L = oem_amd.lib()
    scratch = (C.c_double * 64)()
    ptr = C.addressof(scratch)
    dp = C.cast(scratch, C.POINTER(C.c_double))
    cnt = (C.c_int64 * 8)()
    assert L.oemgpu_logistic_cv_score_dev(ptr, ptr, 50, 50, 4, ptr, 1.0, None, 5, dp, 3, dp, cnt, None) == -1
    assert L.oemgpu_logistic_cv_score_dev(ptr, ptr, 50, 50, 4, ptr, 1.0, ptr, 2, dp, 3, dp, cnt, None) == -1
    assert L.oemgpu_logistic_cv_score_dev(ptr, ptr, 50, 50, 4, ptr, 1.0, ptr, 5, dp, 0, dp, cnt, None) == -1
    assert L.oemgpu_logistic_cv_score_dev(ptr, ptr, 50, 40, 4, ptr, 1.0, ptr, 5, dp, 3, dp, cnt, None) == -1
    assert L.oemgpu_logistic_cv_score_dev(ptr, ptr, 10000, 10000, 8192, ptr, 1.0, ptr, 5, dp, 3, dp, cnt, None) == -4


def _score_plan(L, n, p, ncol, num_cu, out=None):
    out = (C.c_int64 * 6)() if out is None else out
    assert L.oemgpu_selftest_cv_score_plan(n, p, ncol, num_cu, out) == 0, (n, p, ncol, num_cu)
    return tuple(out)


def _check_score_plan(P, n, p, ncol, num_cu):
    ch, nchunk, tlds, cb, nlaunch, lds = P
    assert ch >= 64 and ch % 64 == 0, (P, n, num_cu)
    assert (nchunk - 1) * ch < n <= nchunk * ch, (P, n, num_cu)
    assert nchunk <= 4 * num_cu, (P, n, num_cu)
    assert tlds == (1 if 8 * (ncol * (p + 9) + 1) <= LDS_BYTES else 0), (P, p, ncol)
    assert 0 < lds <= LDS_BYTES, (P, p, ncol)
    assert cb >= 1 and cb * nlaunch >= ncol and cb * nlaunch < ncol + cb, (P, p, ncol)
    if tlds:                                                # the whole table and its accumulators, in one launch
        assert (cb, nlaunch, lds) == (ncol, 1, 8 * (ncol * (p + 9) + 1)), (P, p, ncol)
    else:                                                   # the accumulators of a launch's columns alone
        assert lds == 8 * (8 * cb + 1), (P, p, ncol)


@pytest.mark.parametrize("num_cu", [64, 256, 304])
def test_score_plan_rows(num_cu):
    """n from 1 to 3e6: the neighbours of every multiple of 64 * 4 * num_cu (where the rows per workgroup grow by a tile), the small n
    where a workgroup has one tile, and a seeded draw in between"""
    import oem_amd
    L = oem_amd.lib()
    out = (C.c_int64 * 6)()
    step = 64 * 4 * num_cu
    ns = set(range(1, 300)) | {3 * 10 ** 6}
    for m in range(step, 3 * 10 ** 6 + step, step):
        ns |= {m - 1, m, m + 1, m - 64, m + 64, m + 65}
    ns |= {int(v) for v in np.random.default_rng(num_cu).integers(1, 3 * 10 ** 6, 3000)}
    seen = set()
    for n in sorted(v for v in ns if 1 <= v <= 3 * 10 ** 6):
        P = _score_plan(L, n, 5, 9, num_cu, out)
        _check_score_plan(P, n, 5, 9, num_cu)
        assert P[0] == max(64, -(-(-(-n // (4 * num_cu))) // 64) * 64), (P, n)
        seen.add(P[0])
    assert {64, 128, 192} <= seen                           # one tile and several tiles per workgroup were both looked at
    for n, p, ncol in ((1, 8191, 5000), (3 * 10 ** 6, 1, 1), (step + 1, 200, 98), (step, 200, 97)):      # n and the table do not interact
        P, Q = _score_plan(L, n, p, ncol, num_cu), _score_plan(L, n, 5, 9, num_cu)
        _check_score_plan(P, n, p, ncol, num_cu)
        assert P[:2] == Q[:2]


def test_score_plan_table():
    """p from 1 to 8191 against every ncol from 1 to 5000 (a set of p that holds the ends, the fits' own limits and a seeded draw), and
    for EVERY p the two ncol on either side of the LDS limit"""
    import oem_amd
    L = oem_amd.lib()
    out = (C.c_int64 * 6)()
    rng = np.random.default_rng(12)
    ps = sorted({1, 2, 7, 8, 9, 55, 56, 57, 110, 192, 193, 200, 1023, 1024, 2047, 2048, 2049, 4095, 4096, 6826, 8190, 8191} |
                {int(v) for v in rng.integers(1, 8192, 24)})
    for p in ps:
        for ncol in range(1, 5001):
            _check_score_plan(_score_plan(L, 1000, p, ncol, 256, out), 1000, p, ncol, 256)
    both = set()
    for p in range(1, 8192):
        edge = (LDS_BYTES // 8 - 1) // (p + 9)              # the most columns whose table fits
        for ncol in (edge, edge + 1):
            if 1 <= ncol <= 5000:
                P = _score_plan(L, 77, p, ncol, 64, out)
                _check_score_plan(P, 77, p, ncol, 64)
                assert P[2] == (1 if ncol == edge else 0), (P, p, ncol)
                both.add(P[2])
    assert both == {0, 1}
    assert _score_plan(L, 200, 200, 97, 256)[2:] == (1, 97, 1, 162192)
    assert _score_plan(L, 200, 200, 98, 256)[2:] == (0, 98, 1, 8 * (8 * 98 + 1))
    assert _score_plan(L, 130, 8191, 2, 256)[2:] == (1, 2, 1, 8 * (2 * 8200 + 1))
    assert _score_plan(L, 130, 8191, 3, 256)[2:] == (0, 3, 1, 8 * 25)
    assert _score_plan(L, 200, 200, 2100, 256)[2:] == (0, 2048, 2, 8 * (8 * 2048 + 1))
    assert _score_plan(L, 200, 1, 5000, 256)[2:] == (0, 2048, 3, 8 * (8 * 2048 + 1))


def test_score_plan_argument_errors():
    import oem_amd
    L = oem_amd.lib()
    out = (C.c_int64 * 6)()
    for n, p, ncol, num_cu in ((0, 5, 9, 256), (100, 0, 9, 256), (100, 8192, 9, 256), (100, 5, 0, 256), (100, 5, 9, 0)):
        assert L.oemgpu_selftest_cv_score_plan(n, p, ncol, num_cu, out) == -1
    assert L.oemgpu_selftest_cv_score_plan(100, 5, 9, 256, None) == -1


def _table(seed=0, n=400, p=6, k=7):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, p))
    y = (rng.uniform(size=n) < 0.5).astype(np.float64)
    coef = rng.normal(size=(p + 1, k)) * np.linspace(0.1, 3.0, k)          # the last columns reach the 1e-5 clamp
    prob = 1.0 / (1.0 + np.exp(-(np.column_stack([np.ones(n), x]) @ coef)))
    return y, prob


def test_restatement_deviance_and_class_are_sklearns():
    pytest.importorskip("sklearn")
    from sklearn.metrics import log_loss, zero_one_loss
    y, prob = _table()
    prob[:3, -1] = [1e-9, 1.0 - 1e-9, 0.5]                                  # both clamps and the class rule's boundary
    ymat = np.column_stack([1.0 - y, y])
    dev = CV.raw_errors(ymat, prob, "deviance")
    cls = CV.raw_errors(ymat, prob, "class")
    for j in range(prob.shape[1]):
        pc = np.clip(prob[:, j], 1e-5, 1 - 1e-5)
        ll = log_loss(y, np.column_stack([1 - pc, pc]), labels=[0.0, 1.0])
        assert abs(dev[:, j].mean() - 2.0 * ll) <= 1e-12 * (1 + 2.0 * ll)
        assert cls[:, j].mean() == pytest.approx(zero_one_loss(y, (prob[:, j] > 0.5).astype(np.float64)), abs=1e-15)
    # mse / mae count both columns of the indicator matrix (1 - pred is rounded to 1.1e-16 absolute: terms of order 1, atol 1e-15)
    np.testing.assert_allclose(CV.raw_errors(ymat, prob, "mse"), 2 * (y[:, None] - prob) ** 2, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(CV.raw_errors(ymat, prob, "mae"), 2 * np.abs(y[:, None] - prob), rtol=1e-13, atol=1e-15)


def test_restatement_auc_is_sklearns_without_ties():
    pytest.importorskip("sklearn")
    from sklearn.metrics import roc_auc_score
    y, prob = _table(seed=1)
    ymat = np.column_stack([1.0 - y, y])
    for j in range(prob.shape[1]):
        assert len(np.unique(prob[:, j])) == len(y)
        assert CV.auc_mat(ymat, prob[:, j]) == pytest.approx(roc_auc_score(y, prob[:, j]), rel=1e-12)


def test_library_auc_is_the_restatements():
    """the host-side AUC of cv_oem (no GPU in it) against auc.mat's doubled-rows form, ties included"""
    from oem_amd import api
    y, prob = _table(seed=2)
    prob[:50, 0] = prob[50:100, 0]                                          # ties, broken by row order in both
    ymat = np.column_stack([1.0 - y, y])
    for j in range(prob.shape[1]):
        assert api._auc_rows(y, prob[:, j]) == pytest.approx(CV.auc_mat(ymat, prob[:, j]), rel=1e-13)


def test_cv_oem_binomial_checks_y_like_oem():
    import oem_amd
    rng = np.random.default_rng(3)
    x = rng.normal(size=(60, 4))
    y = rng.integers(0, 3, size=60).astype(np.float64)
    with pytest.raises(ValueError, match="y must be a binary outcome"):
        oem_amd.cv_oem(x, y, family="binomial", penalty="lasso", nfolds=5)
    with pytest.raises(oem_amd.OemgpuError, match="weights not implemented yet."):
        oem_amd.cv_oem(x, (y > 0).astype(np.float64), family="binomial", weights=np.ones(60))
    with pytest.raises(ValueError, match="should be one of"):
        oem_amd.cv_oem(x, y, family="poisson")
