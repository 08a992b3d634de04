"""cv.oem for binomial fits, the part that needs no GPU: the two C entries are declared, exported and bound; their argument errors
come back before a device is looked for; the restatement's error terms (tests/cv_logistic_restatement.py) are scikit-learn's; and
cv_oem(family="binomial") makes oem()'s check of y."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import cv_logistic_restatement as CV

ROOT = Path(__file__).resolve().parent.parent
NEW = ("oemgpu_fit_logistic_dense_fold_dev", "oemgpu_logistic_cv_score_dev")


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
