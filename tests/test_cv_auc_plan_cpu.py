"""The host side of cv.oem's device AUC, without a GPU: the two entries are exported and refuse bad arguments before a device is looked
for; the launch plan of oemgpu_logistic_cv_auc_dev (oemgpu_selftest_cv_auc_plan, the one function the launch code reads) holds its
invariants over n in 1 .. 10^7, K in {3, 10}, ncol in {1, 100, 1400} and 1, 64 and 256 CUs; and the closing formula that
api._cv_oem_binomial_on applies to the device's integers (api._auc_from_counts, factored out of api._auc_rows) is the one _auc_rows
applies, bit for bit."""
import ctypes as C

import numpy as np
import pytest

LDS_BYTES = 160 << 10
WS_BOUND = 256 << 20


def _plan(n, K, ncol, num_cu, longest):
    from oem_amd import api
    return api.cv_auc_plan(n, K, ncol, num_cu, longest)


def test_entries_are_exported_and_check_their_arguments():
    import oem_amd
    L = oem_amd.lib()
    assert "oemgpu_logistic_cv_auc_dev" in oem_amd.EXPORTS and "oemgpu_selftest_cv_auc_plan" in oem_amd.EXPORTS
    ptr = C.c_void_p(64)                                               # never dereferenced: the checks come first
    out = (C.c_int64 * 4)()
    a = C.cast(out, C.POINTER(C.c_int64))
    assert L.oemgpu_logistic_cv_auc_dev(None, ptr, 50, 3, ptr, 1.0, ptr, 5, a, a, a) == -1
    assert L.oemgpu_logistic_cv_auc_dev(ptr, None, 50, 3, ptr, 1.0, ptr, 5, a, a, a) == -1
    assert L.oemgpu_logistic_cv_auc_dev(ptr, ptr, 50, 3, None, 1.0, ptr, 5, a, a, a) == -1
    assert L.oemgpu_logistic_cv_auc_dev(ptr, ptr, 50, 3, ptr, 1.0, None, 5, a, a, a) == -1
    assert L.oemgpu_logistic_cv_auc_dev(ptr, ptr, 50, 3, ptr, 1.0, ptr, 5, None, a, a) == -1
    assert L.oemgpu_logistic_cv_auc_dev(ptr, ptr, 50, 3, ptr, 1.0, ptr, 5, a, None, a) == -1
    assert L.oemgpu_logistic_cv_auc_dev(ptr, ptr, 50, 3, ptr, 1.0, ptr, 5, a, a, None) == -1
    assert L.oemgpu_logistic_cv_auc_dev(ptr, ptr, 0, 3, ptr, 1.0, ptr, 5, a, a, a) == -1
    assert L.oemgpu_logistic_cv_auc_dev(ptr, ptr, 50, 0, ptr, 1.0, ptr, 5, a, a, a) == -1
    assert L.oemgpu_logistic_cv_auc_dev(ptr, ptr, 50, 3, ptr, 1.0, ptr, 0, a, a, a) == -1
    assert b"nfolds" in L.oemgpu_last_error()
    assert L.oemgpu_logistic_cv_auc_dev(ptr, ptr, 50000, 3, ptr, 1.0, ptr, 4097, a, a, a) == -4
    assert L.oemgpu_logistic_cv_auc_dev(ptr, ptr, 2 ** 31, 3, ptr, 1.0, ptr, 5, a, a, a) == -4
    big = (C.c_int64 * 9)()
    for bad in ((0, 3, 1, 256, 0), (10, 0, 1, 256, 5), (10, 4097, 1, 256, 5), (10, 3, 0, 256, 5), (10, 3, 1, 0, 5), (10, 3, 1, 256, 11),
                (10, 3, 1, 256, -1)):
        assert L.oemgpu_selftest_cv_auc_plan(*bad, big) == -1, bad
    assert L.oemgpu_selftest_cv_auc_plan(10, 3, 1, 256, 5, None) == -1


N_SWEEP = sorted({int(round(10 ** e)) for e in np.linspace(0.0, 7.0, 29)} | {1, 10 ** 7})


@pytest.mark.parametrize("num_cu", [1, 64, 256])
@pytest.mark.parametrize("ncol", [1, 100, 1400])
@pytest.mark.parametrize("K", [3, 10])
def test_plan_invariants(K, ncol, num_cu):
    for n in N_SWEEP:
        longest_even = (n + K - 1) // K
        seen_hbm = False
        for longest in sorted({0, 1, longest_even // 2, longest_even, min(n, 2 * longest_even), n}):
            P = _plan(n, K, ncol, num_cu, longest)
            tag = (n, K, ncol, num_cu, longest, P)
            assert P["tile"] >= 64 and P["tile"] % 64 == 0 and P["lmax"] >= P["tile"], tag
            assert P["lds"] <= LDS_BYTES, tag
            assert P["lds"] >= 16 * min(longest, P["lmax"]), tag       # two key buffers of the longest LDS segment fit in what is asked for
            assert 1 <= P["cb"] <= ncol and P["batches"] * P["cb"] >= ncol and (P["batches"] - 1) * P["cb"] < ncol, tag
            assert P["ws"] <= WS_BOUND + 16 * n, tag                   # the bound plus one column's share
            if P["form"] == "hbm":
                assert P["ws"] >= 16 * n * P["cb"] + 4 * n, tag        # the key buffers of a batch and perm are in it
                assert P["cb"] == ncol or P["ws"] + 16 * n + 8 * K > WS_BOUND, tag   # a batch is as wide as the bound lets it be (a column: keys + K results)
                assert P["cb"] == min(ncol, _plan(n, K, 10 ** 6, num_cu, longest)["cb"]), tag   # and as wide whatever ncol is
            else:
                assert P["batches"] == 1, tag                          # nothing to keep under a bound: one launch takes every column
            assert P["chunk"] % 64 == 0 and P["chunks"] * P["chunk"] >= n > (P["chunks"] - 1) * P["chunk"] and P["chunks"] <= 1024, tag
            # the choice is monotone in the segment length: LDS up to lmax, the workspace beyond, and lmax does not depend on the call
            assert (P["form"] == "hbm") == (longest > P["lmax"]), tag
            assert not (seen_hbm and P["form"] == "lds"), tag
            seen_hbm = seen_hbm or P["form"] == "hbm"
            assert P["lmax"] == _plan(1, 3, 1, 1, 0)["lmax"], tag


def test_form_switches_once_along_the_segment_length():
    L = _plan(100000, 3, 5, 256, 10)["lmax"]
    forms = [_plan(100000, 3, 5, 256, ln)["form"] for ln in range(L - 3, L + 4)]
    assert forms == ["lds"] * 4 + ["hbm"] * 3


def test_closing_formula_is_auc_rows():
    from oem_amd import api
    rng = np.random.default_rng(5)
    for k in range(300):
        m = int(rng.integers(1, 60))
        if k % 7 == 0:
            y2 = np.ones(m)                                            # n0 = 0
        elif k % 7 == 1:
            y2 = np.zeros(m)                                           # n1 = 0, u = 0
        else:
            y2 = (rng.random(m) < 0.5).astype(np.float64)
        prob = np.round(rng.random(m), 1) if k % 2 else rng.random(m)
        if k % 7 == 2:                                                 # every y2 = 1 row in front: u = 0 with n1, n0 > 0
            prob = np.where(y2 == 1, 0.1, 0.9)
        ys = y2[np.argsort(prob, kind="stable")] == 1
        u, n1, n0 = int(np.cumsum(~ys)[ys].sum()), int(ys.sum()), int((~ys).sum())
        a, b = api._auc_rows(y2, prob), api._auc_from_counts(float(u), float(n1), float(n0))
        assert np.float64(a).tobytes() == np.float64(b).tobytes() or (np.isnan(a) and np.isnan(b)), (k, u, n1, n0, a, b)
    for u, n1, n0 in ((0, 0, 5), (0, 5, 0), (0, 3, 4), (12, 3, 4), (10 ** 15, 10 ** 8, 10 ** 8)):
        got = api._auc_from_counts(float(u), float(n1), float(n0))
        with np.errstate(divide="ignore", invalid="ignore"):
            want = float(np.exp(np.log(float(u)) - np.log(float(n1)) - np.log(float(n0))))
        assert (np.isnan(got) and np.isnan(want)) or got == want, (u, n1, n0)
    assert api._auc_from_counts(12.0, 3.0, 4.0) == pytest.approx(1.0, abs=1e-15) and api._auc_from_counts(0.0, 3.0, 4.0) == 0.0
