"""tests/sparse_wide_pass_cases.py on its own, without a GPU: the structure it claims, the 2^53 conditions that make its integer
references exact, those references against a second derivation (plain float64 numpy sums, exact on the same data), the number of long
lines per lane count against the library's own plan arithmetic, the real-valued twin's bound on the reference side alone -- and the
refusals of oemgpu_selftest_sparse_wide_pass that come back before any device work."""
import ctypes as C

import numpy as np
import pytest

from tests import sparse_wide_pass_cases as S

ERR_ARG, ERR_UNSUPPORTED = -1, -4
DYADIC = [S.structured, lambda: S.tiny((2, 3)), lambda: S.tiny((2, 2))] + [lambda n=n: S.chunk(n) for n in S.CHUNK_NS]
IDS = ["structured", "2x3", "2x2"] + ["chunk%d" % n for n in S.CHUNK_NS]


def test_the_module_needs_neither_torch_nor_the_oracle():
    src = open(S.__file__).read()
    assert "import torch" not in src and "oracle import" not in src and "import oracle" not in src


# ------------------------------------------------------------------------------------------------------------------ structure
def test_structured_case_has_every_crafted_length_among_rows_and_columns():
    c = S.structured()
    assert (c.n, c.p) == (S.N_STRUCT, S.P_STRUCT) and c.n <= c.p and 90000 < c.nnz < 115000
    rows, cols = set(c.row_len.tolist()), set(c.col_len.tolist())    # read from indptr of the CSR and CSC forms
    for L in S.LANES:
        for t in S.crafted_lengths(L):
            assert t in rows, ("row", L, t)
            assert t in cols, ("column", L, t)
        assert (c.n * L) % 256 != 0 and (c.p * L) % 256 != 0         # the last workgroup is ragged
    assert 32 * 64 + 1 == 2049 and 2049 in rows and 2049 in cols
    r = c.role
    for (t, f), i in r.crafted_rows.items():                         # every length in every fold
        assert c.row_len[i] == t and c.fid[i] == f + 1
    for t, j in r.crafted_cols.items():
        assert c.col_len[j] == t
    assert c.row_len[0] == 0 and c.row_len[-1] == 0 and c.col_len[0] == 0 and c.col_len[-1] == 0
    assert np.all(c.row_len[r.empty_rows] == 0) and np.all(c.col_len[r.empty_cols] == 0)
    assert c.row_len[r.full_row] == c.p - 4 == c.row_len.max()       # every column but the three empty ones and the one outside fold 1
    assert c.col_len[r.full_col] == c.n - 3 == c.col_len.max()
    assert c.row_len[r.full_row] > 32 * 64 and c.col_len[r.full_col] > 32 * 64


def test_structured_folds():
    c = S.structured()
    r = c.role
    assert set(np.unique(c.fid)) == {1, 2, 3} and c.K == 3
    assert c.fid[r.full_row] == 1
    assert any(c.fid[i] == 2 for i in r.empty_rows)
    for L in S.LANES:                                                # fold 1 both contains and omits long rows (and 32 L exactly)
        lr = S.long_lines(c.row_len, L)
        assert np.any(c.fid[lr] == 1) and np.any(c.fid[lr] != 1)
        at = np.nonzero(c.row_len == 32 * L)[0]
        assert np.any(c.fid[at] == 1) and np.any(c.fid[at] != 1)
    ins = c.csc[:, r.inside_col].indices
    out = c.csc[:, r.outside_col].indices
    assert ins.size > 5 and np.all(c.fid[ins] == 1)                  # wholly inside fold 1: emptied when fold 1 is left out
    assert out.size > 5 and np.all(c.fid[out] != 1)                  # wholly outside
    for k in (1, 2, 3):
        assert (c.fid != k).sum() >= 2


def test_stored_zeros_and_value_ranges():
    c = S.structured()
    d = c.csc.data
    assert np.array_equal(d * 8, np.round(d * 8)) and np.abs(d * 8).max() <= 32
    neg0 = (d == 0) & np.signbit(d)
    pos0 = (d == 0) & ~np.signbit(d)
    assert neg0.sum() == 12 and pos0.sum() == 12
    assert np.array_equal(c.kcsc.data, (d * 8).astype(np.int64)) and np.array_equal(c.kcsc.indices, c.csc.indices)
    assert np.array_equal(c.kcsr.indptr, c.csr.indptr) and np.array_equal(c.kcsr.indices, c.csr.indices)
    for v in (c.vi, c.wi, c.yi):
        assert np.abs(v).max() <= 32 and np.abs(v).min() >= 1
    assert np.all(np.isnan(c.coef[:, 0])) and np.abs(c.bi).max() <= 8 and np.all((c.bi != 0).sum(axis=1) == 12)
    t = S.real_twin()
    assert np.array_equal(t.csc.indptr, c.csc.indptr) and np.array_equal(t.csc.indices, c.csc.indices)
    assert 1.4 < t.csc.data.std() < 1.6


def test_edge_cases():
    assert (S.tiny((2, 3)).n, S.tiny((2, 3)).p) == (2, 3)
    assert (S.tiny((2, 2)).n, S.tiny((2, 2)).p) == (2, 2)
    assert S.CHUNK_NS == (2047, 2048, 2049, 4097)
    for n in S.CHUNK_NS:
        c = S.chunk(n)
        assert c.n == c.p == n and 1 <= c.row_len.min() and c.row_len.max() <= 5
        assert len(S.exact_loss(c)[1][0]) == (n + 2047) // 2048


# ------------------------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("make", DYADIC, ids=IDS)
def test_the_2_53_conditions_hold(make):
    assert S.check_exact(make()) < 2 ** 53


@pytest.mark.parametrize("make,leave_out", [(m, k) for m, i in zip(DYADIC, IDS) for k in ((0,) if "x" in i else (0, 1, 2))],
                         ids=["%s-%d" % (i, k) for i in IDS for k in ((0,) if "x" in i else (0, 1, 2))])
def test_integer_references_equal_plain_float64_sums(make, leave_out):
    """np.bincount adds float64 terms one after the other in storage order; on this data that is exact too (the tiny cases carry no folds)"""
    c = make()
    keep = S.keep_rows(c, leave_out)
    m = c.csc.tocoo()
    kf = keep[m.row]
    rows = np.bincount(m.row, weights=m.data * c.v[m.col], minlength=c.n)
    assert np.array_equal(S.exact_rows(c, keep) / 64.0, np.where(keep, rows, 0.0))
    assert np.array_equal(S.exact_cols(c, keep) / 64.0, np.bincount(m.col, weights=m.data * c.w[m.row] * kf, minlength=c.p))
    dot, ss, yy, nk = S.exact_stats(c, keep)
    assert np.array_equal(dot / 64.0, np.bincount(m.col, weights=m.data * c.y[m.row] * kf, minlength=c.p))
    assert np.array_equal(ss / 64.0, np.bincount(m.col, weights=m.data * m.data * kf, minlength=c.p))
    assert yy / 64.0 == float(np.sum(c.y[keep] ** 2)) and nk == int(keep.sum())
    total, chunks = S.exact_loss(c, keep)
    for b, tot, per in zip(c.coef, total, chunks):
        r = c.y - np.bincount(m.row, weights=m.data * b[1:][m.col], minlength=c.n)
        assert tot / 4096.0 == float(np.sum(r[keep] ** 2)) and sum(per) == tot


# ------------------------------------------------------------------------------------------------------------------ long lines
def test_long_line_counts_follow_the_plan_arithmetic():
    """for each forced L: the lines of more than 32 L entries, and the library's plan (its lanes for a CU count that yields L) says the
    long form is used exactly when there are any"""
    import oem_amd
    lib = oem_amd.lib()
    c = S.structured()

    def plan(n, p, nnz, lr, lc, cu):
        out = (C.c_int64 * 8)()
        assert lib.oemgpu_selftest_sparse_wide_plan(n, p, nnz, lr, lc, cu, out) == 0
        return list(out)
    for cu in (1, 8, 64, 256, 304, 1024):                            # the restated lane rule is the library's
        o = plan(c.n, c.p, c.nnz, 0, 0, cu)
        assert (64 // o[1], 64 // o[2]) == (S.lanes_plan(c.n, c.nnz, cu), S.lanes_plan(c.p, c.nnz, cu)), cu
    assert (S.lanes_plan(c.n, c.nnz, 256), S.lanes_plan(c.p, c.nnz, 256)) == (32, 32)
    want = {1: 32, 2: 64, 4: 128, 8: 256, 16: 512, 32: 1024, 64: 2048}
    for L in S.LANES:
        lr, lc = S.long_lines(c.row_len, L), S.long_lines(c.col_len, L)
        assert np.all(c.row_len[lr] > want[L]) and lr.size == (c.row_len > want[L]).sum() and lr.size >= 4
        assert lc.size >= 2 and c.role.full_row in lr and c.role.full_col in lc
        assert not np.any(np.isin(np.nonzero(c.row_len == want[L])[0], lr))        # exactly 32 L: the short form's
        assert np.all(np.isin(np.nonzero(c.row_len == want[L] + 1)[0], lr))
    # the plan's long flags switch between a longest line of 32 L and 32 L + 1, at the lanes it chooses
    for cu in (8, 256):
        o = plan(c.n, c.p, c.nnz, 0, 0, cu)
        Lr, Lc = 64 // o[1], 64 // o[2]
        assert plan(c.n, c.p, c.nnz, 32 * Lr, 32 * Lc, cu)[3:5] == [0, 0]
        assert plan(c.n, c.p, c.nnz, 32 * Lr + 1, 32 * Lc, cu)[3:5] == [1, 0]
        assert plan(c.n, c.p, c.nnz, 32 * Lr, 32 * Lc + 1, cu)[3:5] == [0, 1]
    for n in S.CHUNK_NS:                                             # no long line at any L
        assert S.long_lines(S.chunk(n).row_len, 1).size == 0 and S.long_lines(S.chunk(n).col_len, 1).size == 0


# ------------------------------------------------------------------------------------------------------------ the real twin
def test_real_twin_bound_holds_on_the_reference_side():
    """math.fsum against a plain left-to-right float64 sum of the same products: one of the summation trees the bound covers"""
    t = S.real_twin()
    for m, vec, lens in ((t.csr, t.v, t.row_len), (t.csc, t.w, t.col_len)):
        ref, a = S.fsum_lines(m, vec)
        prod = m.data * vec[m.indices]
        seq = np.array([np.cumsum(prod[m.indptr[i]:m.indptr[i + 1]])[-1] if lens[i] else 0.0 for i in range(lens.size)])
        b = S.line_bound(lens, a)
        assert np.all(np.abs(seq - ref) <= b)
        assert np.all(b[lens > 0] > 0) and np.all(b[lens == 0] == 0)
        assert np.all(b <= 2.0 ** -41 * np.maximum(a, 1e-300))       # (2049 + 2) 2^-53 < 2^-41: the bound is tight, not generous
        assert np.any(seq != ref)                                    # and real data does round: the twin is no second dyadic case


# ------------------------------------------------------------------------------------------------------------------ refusals
class _Handle(C.Structure):
    """the leading fields of oemgpu_sparse_x (oem_amd/csrc/logistic.hpp) that the entry's checks read"""
    _fields_ = [("device", C.c_int), ("n", C.c_int64), ("nnz", C.c_int64), ("maxcol", C.c_int64), ("p", C.c_int32), ("rest", C.c_char * 256)]


def test_pass_entry_refuses_before_any_device_work():
    import oem_amd
    lib = oem_amd.lib()
    scratch = (C.c_double * 64)()                                    # a zeroed "context": device 0, never followed further
    ptr = C.addressof(scratch)
    h = _Handle(); h.device = 0; h.n = 5; h.p = 8
    info = (C.c_int64 * 8)(*([-7] * 8))

    def call(ctx=ptr, x=C.addressof(h), kind=0, rl=0, cl=0, fid=ptr, nfolds=3, leave=1, vec=ptr, coef=None, ncoef=0, out=ptr, out2=None,
             st=None, inf=info):
        rc = lib.oemgpu_selftest_sparse_wide_pass(ctx, x, kind, rl, cl, fid, nfolds, leave, 1, 1.0, vec, coef, ncoef, out, out2, st, inf, None, None)
        return rc, lib.oemgpu_last_error().decode()
    for kw in (dict(ctx=None), dict(x=None), dict(vec=None), dict(out=None), dict(inf=None), dict(kind=2), dict(kind=2, out2=ptr),
               dict(kind=2, st=ptr), dict(kind=3), dict(kind=3, coef=ptr, ncoef=0)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "NULL argument" in msg, kw
    for kind in (-1, 4, 99):
        rc, msg = call(kind=kind)
        assert rc == ERR_ARG and "pass must be" in msg, kind
    for bad in (-1, 3, 5, 6, 12, 48, 65, 128):
        for kw in (dict(rl=bad), dict(cl=bad)):
            rc, msg = call(**kw)
            assert rc == ERR_ARG and "lanes must be" in msg, kw
    h.device = 1                                                     # every allowed lane count passes on to the next refusal
    for L in (0,) + S.LANES:
        rc, msg = call(rl=L, cl=L)
        assert rc == ERR_ARG and "different devices" in msg, L
    h.device = 0
    for nf in (2, 513, 0, -1):
        rc, msg = call(nfolds=nf, leave=0)
        assert rc == ERR_ARG and "3..512" in msg, nf
    for lo in (-1, 4):
        rc, msg = call(leave=lo)
        assert rc == ERR_ARG and "leave_out" in msg, lo
    rc, msg = call(fid=None, leave=2)
    assert rc == ERR_ARG and "NULL foldid" in msg
    h.n = 1
    rc, msg = call()
    assert rc == ERR_ARG and "two rows" in msg
    h.n = 9
    rc, msg = call()
    assert rc == ERR_UNSUPPORTED and "n > p" in msg
    assert list(info) == [-7] * 8                                    # nothing was written
    assert len(lib.oemgpu_switch_names().split()) == 34              # forcing lanes is an argument, not a switch
