"""ONE pass of the sparse wide engine (oem_amd/csrc/sparse_wide.hip) through oemgpu_selftest_sparse_wide_pass, at every lane count the
gather kernel is instantiated for, held to exact sums.  No path is fitted here.

The fits of tests/test_gpu_sparse_wide.py and tests/test_gpu_cv_sparse_wide.py reach, on a 256-CU device, rows at 64 (or 4) lanes and
columns at 4 .. 64, never 1 or 2; this file forces the lanes.  On the dyadic inputs of tests/sparse_wide_pass_cases.py every sum is
exact in float64 whatever its order, so every output is compared BIT FOR BIT with an integer computation:

  spw_gather_kernel<L, false, false>   test_rows_exact[L-0] (rows) and test_cols_exact[L-*] (columns), L = 1 .. 64
  spw_gather_kernel<L, false, true>    test_rows_exact[L-1], [L-2]: a left-out row is +0.0 whether short, long or empty
  spw_gather_kernel<L, true, false>    test_stats_exact[L-0]
  spw_gather_kernel<L, true, true>     test_stats_exact[L-1], [L-2]
  spw_long_kernel<STATS, MASK>         the same four tests: at every L the structured case has rows and columns of more than 32 L entries
  spw_scan_kernel                      test_rows_exact: the lists of long lines and the longest lines against numpy, per L
  spw_y_kernel<MASK>                   test_stats_exact: stats[0 .. 3] and the shift flags
  spw_resid_sq_kernel<MASK>, spw_loss_sum_kernel    test_loss_exact at n = 2047, 2048, 2049, 4097 and on the structured case

The outputs are filled with NaN before a call, so a slot the pass leaves unwritten shows.  The real-valued twin holds the same kernels,
at every L, to the derived bound of sparse_wide_pass_cases.line_bound around math.fsum."""
import ctypes as C

import numpy as np
import pytest

from tests import sparse_wide_pass_cases as S

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -4
MASKS = (0, 1, 2)                  # leave_out: 0 unmasked; fold 1 holds the full row and empties a column; fold 2 an empty row


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available()
    from oem_amd import api
    return api


@pytest.fixture(scope="module")
def dev(api):
    """case -> (case, SparseX, device tensors), every handle built once for the module"""
    import torch
    made = {}

    def get(c):
        if c.name not in made:
            t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")
            d = dict(v=t(c.v), w=t(c.w), y=t(c.y), fid=None if c.fid is None else t(c.fid, torch.int32))
            if not c.real:
                d["coef"] = t(c.coef)
            made[c.name] = (c, api.SparseX(c.csc), d)
        return made[c.name]
    yield get
    for _, sx, _ in made.values():
        sx.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b, label):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    bad = np.nonzero(_bits(a) != _bits(b))[0]
    assert bad.size == 0, (label, bad.size, bad[:5], a[bad[:5]], b[bad[:5]])


def _within_ulps(a, b, k, label):
    """|a - b| <= k ulps of b; b finite"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.all(np.isfinite(a)), label
    bad = np.nonzero(np.abs(a - b) > k * np.spacing(np.abs(b)))[0]
    assert bad.size == 0, (label, bad.size, bad[:5], a[bad[:5]], b[bad[:5]])


def _mask_kw(d, leave_out):
    return dict(foldid=d["fid"], nfolds=S.K_FOLDS, leave_out=leave_out) if leave_out else {}


def _scales(n):
    return (1.0, 0.5, 1.0 / n)


def _check_info(c, r, L, leave_out, label):
    i = r["info"]
    assert (i["row_lanes"], i["col_lanes"]) == (L, L), label
    lr, lc = S.long_lines(c.row_len, L), S.long_lines(c.col_len, L)
    assert (i["long_rows"], i["long_cols"]) == (lr.size, lc.size), label
    assert (i["longest_row"], i["longest_col"]) == (c.row_len.max(), c.col_len.max()), label
    assert np.array_equal(r["long_row_list"], lr) and np.array_equal(r["long_col_list"], lc), label    # as sets: both sorted
    keep = S.keep_rows(c, leave_out)
    assert i["kept"] == keep.sum() and i["masked"] == (1 if leave_out else 0), label


# ------------------------------------------------------------------------------------------------- dyadic data: bit for bit
@pytest.mark.parametrize("leave_out", MASKS)
@pytest.mark.parametrize("L", S.LANES)
def test_rows_exact(api, dev, L, leave_out):
    c, sx, d = dev(S.structured())
    keep = S.keep_rows(c, leave_out)
    exact = S.exact_rows(c) / 64.0
    assert np.any(~keep[S.long_lines(c.row_len, L)]) or not leave_out          # a long row is left out, another kept
    for scale in _scales(c.n):
        r = api.sparse_wide_pass(sx, "rows", d["v"], L, L, scale=scale, **_mask_kw(d, leave_out))
        _check_info(c, r, L, leave_out, (L, leave_out))
        want = np.where(keep, exact * scale, 0.0)                   # a kept row: the unmasked bits; a left-out row, an empty one: +0.0
        _same(r["out"], want, ("rows", L, leave_out, scale))
    assert not np.any(np.signbit(r["out"][~keep])) and not np.any(np.signbit(r["out"][c.row_len == 0]))


@pytest.mark.parametrize("leave_out", MASKS)
@pytest.mark.parametrize("L", S.LANES)
def test_cols_exact(api, dev, L, leave_out):
    import torch
    c, sx, d = dev(S.structured())
    keep = S.keep_rows(c, leave_out)
    w = d["w"] * torch.as_tensor(keep, device="cuda:0")             # a fit's input is exactly zero in the left-out rows
    exact = S.exact_cols(c, keep) / 64.0
    for scale in _scales(c.n):
        r = api.sparse_wide_pass(sx, "cols", w, L, L, scale=scale, **_mask_kw(d, leave_out))
        _check_info(c, r, L, leave_out, (L, leave_out))
        _same(r["out"], exact * scale, ("cols", L, leave_out, scale))
    assert not np.any(np.signbit(r["out"][c.col_len == 0]))
    if leave_out:                                                   # the column pass itself is never masked
        r = api.sparse_wide_pass(sx, "cols", d["w"], L, L, **_mask_kw(d, leave_out))
        _same(r["out"], S.exact_cols(c) / 64.0, ("cols, full w", L, leave_out))
        if leave_out == 1:
            assert exact[c.role.inside_col] == 0.0 and np.array_equal(exact[c.role.outside_col], S.exact_cols(c)[c.role.outside_col] / 64.0)


def _stats_want(c, keep, standardize):
    dot, ss, yy, nk = S.exact_stats(c, keep)
    xy = (dot / 64.0) / float(nk)
    cs = (ss / 64.0) / (float(nk) - 1.0)
    cs[cs == 0.0] = 1.0
    inv = 1.0 / np.sqrt(cs) if standardize else np.ones(c.p)
    return xy, inv, xy * inv, yy / 64.0, nk


@pytest.mark.parametrize("leave_out", MASKS)
@pytest.mark.parametrize("L", S.LANES)
def test_stats_exact(api, dev, L, leave_out):
    import torch
    c, sx, d = dev(S.structured())
    keep = S.keep_rows(c, leave_out)
    p = c.p
    for standardize in (0, 1):
        xy, inv, xy_std, yy, nk = _stats_want(c, keep, standardize)
        r = api.sparse_wide_pass(sx, "stats", d["y"], L, L, standardize=standardize, **_mask_kw(d, leave_out))
        label = ("stats", L, leave_out, standardize)
        _check_info(c, r, L, leave_out, label)
        st = r["stats"]
        _within_ulps(r["out"], xy, 2, label + ("xy",))
        _within_ulps(st[4 + p:4 + 2 * p], inv, 2, label + ("scale",))
        _within_ulps(r["xy_std"], xy_std, 2, label + ("xy_std",))
        _same(st[4:4 + p], np.zeros(p), label + ("stats[4 + j]",))
        _same(st[:4], [0.0, 1.0, yy, float(nk)], label + ("stats[0 .. 3]",))
        _same(st[4 + 2 * p:], [0.0, 0.0], label + ("shift flags",))
        if not standardize:
            _same(st[4 + p:4 + 2 * p], np.ones(p), label + ("scale without standardize",))
        for j in np.nonzero(c.col_len == 0)[0]:                     # a zero column: xy = +0.0, scale 1
            assert _bits(r["out"][j]) == 0 and st[4 + p + j] == 1.0, label
        if leave_out == 1:                                          # the column the fold empties: xy = 0, scale 1
            j = c.role.inside_col
            assert c.col_len[j] > 5 and _bits(r["out"][j]) == 0 and st[4 + p + j] == 1.0 and _bits(r["xy_std"][j]) == 0, label
        if leave_out:                                               # y of a left-out row is never read
            ynan = torch.where(torch.as_tensor(keep, device="cuda:0"), d["y"], torch.full_like(d["y"], float("nan")))
            g = api.sparse_wide_pass(sx, "stats", ynan, L, L, standardize=standardize, **_mask_kw(d, leave_out))
            for key in ("out", "xy_std", "stats"):
                _same(g[key], r[key], label + ("NaN in the left-out rows", key))


LOSS_CASES = [("chunk", n) for n in S.CHUNK_NS] + [("structured", 0)]


@pytest.mark.parametrize("leave_out", MASKS)
@pytest.mark.parametrize("L", (1, 8, 64))
@pytest.mark.parametrize("kind,n", LOSS_CASES, ids=[k + (str(n) if n else "") for k, n in LOSS_CASES])
def test_loss_exact(api, dev, kind, n, L, leave_out):
    c, sx, d = dev(S.chunk(n) if kind == "chunk" else S.structured())
    keep = S.keep_rows(c, leave_out)
    total, chunks = S.exact_loss(c, keep)
    assert len(chunks[0]) == (c.n + 2047) // 2048
    r = api.sparse_wide_pass(sx, "loss", d["y"], L, L, coef=d["coef"], **_mask_kw(d, leave_out))
    assert r["info"]["row_lanes"] == L and r["info"]["kept"] == keep.sum()
    _same(r["out"], [t / 4096.0 for t in total], ("loss", c.name, L, leave_out))
    assert len(set(total)) == len(total) and min(total) > 0         # the tables differ, so a loss in the wrong slot shows


@pytest.mark.parametrize("L", S.LANES)
@pytest.mark.parametrize("shape", [(2, 3), (2, 2)], ids=["2x3", "2x2"])
def test_tiny_cases(api, dev, shape, L):
    c, sx, d = dev(S.tiny(shape))
    for scale in _scales(c.n):
        _same(api.sparse_wide_pass(sx, "rows", d["v"], L, L, scale=scale)["out"], S.exact_rows(c) / 64.0 * scale, ("rows", shape, L))
        _same(api.sparse_wide_pass(sx, "cols", d["w"], L, L, scale=scale)["out"], S.exact_cols(c) / 64.0 * scale, ("cols", shape, L))
    keep = np.ones(c.n, dtype=bool)
    for standardize in (0, 1):
        xy, inv, xy_std, yy, nk = _stats_want(c, keep, standardize)
        r = api.sparse_wide_pass(sx, "stats", d["y"], L, L, standardize=standardize)
        _within_ulps(r["out"], xy, 2, (shape, L)); _within_ulps(r["stats"][4 + c.p:4 + 2 * c.p], inv, 2, (shape, L))
        _within_ulps(r["xy_std"], xy_std, 2, (shape, L))
        _same(r["stats"][:4], [0.0, 1.0, yy, float(nk)], (shape, L)); _same(r["stats"][4 + 2 * c.p:], [0.0, 0.0], (shape, L))
    r = api.sparse_wide_pass(sx, "loss", d["y"], L, L, coef=d["coef"])
    _same(r["out"], [t / 4096.0 for t in S.exact_loss(c)[0]], ("loss", shape, L))
    assert r["info"]["long_rows"] == 0 and r["info"]["long_cols"] == 0 and len(r["long_row_list"]) == 0


def test_no_long_lines_where_none_is_long(api, dev):
    c, sx, d = dev(S.chunk(2049))
    for L in S.LANES:
        r = api.sparse_wide_pass(sx, "rows", d["v"], L, L)
        i = r["info"]
        assert (i["long_rows"], i["long_cols"], i["longest_row"], i["longest_col"]) == (0, 0, c.row_len.max(), c.col_len.max())
        assert r["long_row_list"].size == 0 and r["long_col_list"].size == 0
        _same(r["out"], S.exact_rows(c) / 64.0, ("chunk rows", L))


# ---------------------------------------------------------------------------------------------------------- planned lanes
@pytest.mark.parametrize("leave_out", (0, 1))
def test_planned_lanes_are_the_plans_and_give_the_forced_bits(api, dev, leave_out):
    import torch
    from oem_amd import _lib
    c, sx, d = dev(S.structured())
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    out = (C.c_int64 * 8)()
    _lib.check(_lib.lib().oemgpu_selftest_sparse_wide_plan(c.n, c.p, c.nnz, int(c.row_len.max()), int(c.col_len.max()), cu, out))
    Lr, Lc = 64 // out[1], 64 // out[2]
    assert (Lr, Lc) == (S.lanes_plan(c.n, c.nnz, cu), S.lanes_plan(c.p, c.nnz, cu)) and out[3] == 1 and out[4] == 1
    kw = _mask_kw(d, leave_out)
    for kind, vec, extra in (("rows", d["v"], dict(scale=0.5)), ("cols", d["w"], dict(scale=0.5)), ("stats", d["y"], dict(standardize=1)),
                             ("loss", d["y"], dict(coef=d["coef"]))):
        a = api.sparse_wide_pass(sx, kind, vec, 0, 0, **extra, **kw)
        b = api.sparse_wide_pass(sx, kind, vec, Lr, Lc, **extra, **kw)
        assert (a["info"]["row_lanes"], a["info"]["col_lanes"]) == (Lr, Lc), kind
        assert a["info"] == b["info"], kind
        for key in a:
            if key != "info":
                _same(a[key], b[key], (kind, key))
    # the lanes of the two orientations are forced apart: rows at 1, columns at 64 and the other way round
    for Lr2, Lc2 in ((1, 64), (64, 1)):
        r = api.sparse_wide_pass(sx, "rows", d["v"], Lr2, Lc2)
        i = r["info"]
        assert (i["row_lanes"], i["col_lanes"]) == (Lr2, Lc2)
        assert (i["long_rows"], i["long_cols"]) == (S.long_lines(c.row_len, Lr2).size, S.long_lines(c.col_len, Lc2).size)
        _same(r["out"], S.exact_rows(c) / 64.0, ("rows", Lr2, Lc2))


# ------------------------------------------------------------------------------------------------------- the real-valued twin
def test_real_twin_within_the_derived_bound_at_every_lane_count(api, dev):
    t, sx, d = dev(S.real_twin())
    for kind, m, vec, key, lens in (("rows", t.csr, t.v, "v", t.row_len), ("cols", t.csc, t.w, "w", t.col_len)):
        ref, a = S.fsum_lines(m, vec)
        got = {}
        for scale in (1.0, 0.37):
            bound = S.line_bound(lens, a, scale)
            for L in S.LANES:
                r = api.sparse_wide_pass(sx, kind, d[key], L, L, scale=scale)["out"]
                r2 = api.sparse_wide_pass(sx, kind, d[key], L, L, scale=scale)["out"]
                _same(r, r2, (kind, L, "two calls"))
                err = np.abs(r - ref * scale)
                assert np.all(np.isfinite(r)) and np.all(err <= bound), (kind, L, scale, float((err - bound).max()))
                assert np.all(_bits(r[lens == 0]) == 0)
                got[(scale, L)] = r
        bound = S.line_bound(lens, a, 1.0)
        moved = 0
        for i, L1 in enumerate(S.LANES):
            for L2 in S.LANES[i + 1:]:
                short = lens <= S.LONG_PER_LANE * L1                # the short form takes the line at both lane counts
                diff = np.abs(got[(1.0, L1)] - got[(1.0, L2)])
                assert np.all(diff[short] <= 2 * bound[short]), (kind, L1, L2)
                moved += int(np.count_nonzero(diff[short]))
                one = lens <= 1                                     # nothing to reorder: the same bits at every L
                _same(got[(1.0, L1)][one], got[(1.0, L2)][one], (kind, L1, L2, "one entry"))
        assert moved > 0                                            # the order does change with L -- and nothing else does


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(api, dev):
    import scipy.sparse as sp
    import torch
    from oem_amd import _lib as L
    c, sx, d = dev(S.chunk(2047))

    def refused(code, match, *a, **kw):
        with pytest.raises(L.OemgpuError, match=match) as e:
            api.sparse_wide_pass(sx, *a, **kw)
        assert e.value.code == code
    for bad in (3, 65, -2, 128):
        refused(ERR_ARG, "lanes must be", "rows", d["v"], bad, 1)
        refused(ERR_ARG, "lanes must be", "rows", d["v"], 1, bad)
    refused(ERR_ARG, "3..512", "rows", d["v"], foldid=d["fid"], nfolds=2, leave_out=1)
    refused(ERR_ARG, "leave_out", "rows", d["v"], foldid=d["fid"], nfolds=3, leave_out=4)
    refused(ERR_ARG, "NULL foldid", "rows", d["v"], foldid=None, nfolds=3, leave_out=1)
    refused(ERR_ARG, "NULL argument", "loss", d["y"])               # no tables
    refused(ERR_ARG, "NULL argument", "rows", None)
    stray = d["fid"].clone(); stray[5] = 7
    for k in (0, 1):                                                # the ids' range whatever is left out
        refused(ERR_ARG, "fold ids are outside", "rows", d["v"], foldid=stray, nfolds=3, leave_out=k)
    one = torch.full_like(d["fid"], 2); one[9] = 1
    refused(ERR_ARG, "keeps 1 of", "rows", d["v"], foldid=one, nfolds=3, leave_out=2)
    info = (C.c_int64 * 8)()
    rc = L.lib().oemgpu_selftest_sparse_wide_pass(api.context(0), sx.handle, 4, 0, 0, None, 3, 0, 0, 1.0, d["v"].data_ptr(), None, 0,
                                                  d["v"].data_ptr(), None, None, info, None, None)
    assert rc == ERR_ARG and b"pass must be" in L.lib().oemgpu_last_error()
    tall = sp.random(9, 4, density=0.5, format="csc", random_state=np.random.default_rng(1))
    with api.SparseX(tall) as st:
        with pytest.raises(L.OemgpuError, match="n > p") as e:
            api.sparse_wide_pass(st, "rows", torch.zeros(4, dtype=torch.float64, device="cuda:0"))
        assert e.value.code == ERR_UNSUPPORTED
    r = api.sparse_wide_pass(sx, "rows", d["v"], 2, 2)              # the handle and the context serve on
    _same(r["out"], S.exact_rows(c) / 64.0, "after the refusals")
