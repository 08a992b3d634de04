"""The kernel form of the column-major moment pass (gram.hip: gram_form, exported as oemgpu_selftest_gram_form) against an independent
restatement of its rule, and the 32-bit lane offsets of every scalar-base form recomputed in Python integers from the kernels' own
formulas: each in [0, 2^32) before the cast to unsigned, each inside the column it names.  Pure host arithmetic, no GPU."""
import ctypes as C

import numpy as np
import pytest

TRI, RING_SADDR, RING_LANE, SB, WD3, WD4, WD_UNITS, BLK = range(8)
TWO32 = 1 << 32

P_SWEEP = sorted(set(range(2, 161)) | set(range(161, 193)) | set(range(225, 257)) | set(range(481, 513)))
N_SWEEP = (1, 63, 64, 4099, 40002)


def ld_max(p):
    """the largest even ld with p ld 8 + 65536 < 2^32"""
    m = (TWO32 - 65536 - 1) // (8 * p)
    return m - (m & 1)


def ld_sweep(n, p):
    base = (n, 8, 1 << 24, (1 << 31) // (8 * 15), ld_max(p), (1 << 25) - 2, 1 << 25, 1 << 28)
    return sorted({b + d for b in base for d in (-2, -1, 0, 1, 2) if b + d >= max(n, 1)})      # (the entry points refuse ld < n)


def rule(n, ld, p, aligned):
    """the form rule, restated: (form, strips)"""
    nt = (p + 2 + 15) // 16                                     # tile columns of Z = [X | y | 1]
    if nt <= 7:                                                 # one wave holds the triangle
        if not aligned or nt < 4 or n < 64:
            return TRI, 0
        if p >= 16 * (nt - 1) and p * ld * 8 + 65536 < TWO32:   # fragments 0 .. nt - 2 are whole columns of X, offsets fit 32 bits
            rem = p + 2 - 16 * (nt - 1)
            return RING_SADDR, (1 if rem <= 4 else 2 if rem <= 8 else 0)
        return RING_LANE, 0
    ntc = (p + 15) // 16
    if not aligned or n < 64 or ld * 16 * 8 >= TWO32:
        return BLK, 0
    if ntc in (11, 12):
        return WD3, 0
    if ntc in (15, 16):
        return WD4, 0
    if ntc >= 31 and ntc % 16 in (0, 15):
        return WD_UNITS, 0
    return SB, 0


@pytest.fixture(scope="module")
def L():
    import oem_amd
    return oem_amd.lib()


def test_ld_max_and_the_first_ld_past_2_to_the_31():
    assert (ld_max(62), ld_max(100), ld_max(110)) == (8_659_076, 5_368_626, 4_880_570)
    for p in (62, 78, 94, 98, 100, 110):
        assert p * ld_max(p) * 8 + 65536 < TWO32 <= p * (ld_max(p) + 2) * 8 + 65536
    # the first even ld at which lane 15 of a shared-slab / one-read fragment passes 2^31 bytes
    assert 15 * 17_895_698 * 8 >= 1 << 31 > 15 * 17_895_696 * 8


def _ring_offsets(p, ld):
    """voff[f] of gram_tri_ring_body for the scalar-base fragments f < NT - 1, all lanes: (offsets before the cast, instruction offsets,
    columns)"""
    nt = (p + 2 + 15) // 16
    cen = nt // 2
    f, i, q = np.meshgrid(np.arange(nt - 1, dtype=np.int64), np.arange(16, dtype=np.int64), np.arange(4, dtype=np.int64), indexing="ij")
    col = 16 * f + i
    assert int(col.max()) < p                                   # whole columns of X: the kernel's `col < p ? col : 0` never takes the 0
    inst = (f - cen) * 1024
    return (col * ld + 2 * q) * 8 - inst, inst, col, q


def _tile_offsets(p, ld):
    """doff[k] of gram_sb_body / gram_wd_body / gram_od_body for every tile column a super-block or unit may name (up to three of padding
    behind the last real one in a deal of eights, a six and a four; up to fifteen in a unit of sixteen), all lanes"""
    ntc = (p + 15) // 16
    T, i, q = np.meshgrid(np.arange(ntc + 16, dtype=np.int64), np.arange(16, dtype=np.int64), np.arange(4, dtype=np.int64), indexing="ij")
    t0 = np.minimum(16 * T, p - 1)
    col = np.minimum(16 * T + i, p - 1)
    return ((col - t0) * ld + 2 * q) * 8, t0, col, q


def test_form_rule_and_lane_offsets(L):
    out = (C.c_int64 * 2)()
    seen = {}
    checked = set()
    edge = {"ring_hi": 0, "tile_hi": 0}
    for p in P_SWEEP:
        for n in N_SWEEP:                                       # (n, p) outermost: the library keeps the last plans
            for ld in ld_sweep(n, p):
                for aligned in ((1, 0) if ld % 2 == 0 else (0,)):       # an odd ld is never 16-byte aligned in every column
                    assert L.oemgpu_selftest_gram_form(n, ld, p, aligned, 256, out) == 0, L.oemgpu_last_error().decode()
                    got = (int(out[0]), int(out[1]))
                    assert got == rule(n, ld, p, bool(aligned)), (n, ld, p, aligned, got)
                    seen[got] = seen.get(got, 0) + 1
                    form = got[0]
                    if form in (TRI, RING_LANE, BLK) or (form, p, ld, n) in checked:
                        continue
                    checked.add((form, p, ld, n))
                    assert n >= 64 and ld >= n                  # so a slab's rows w0 + 2 q, w0 + 2 q + 1 (w0 + 8 <= n) exist in every column
                    if form == RING_SADDR:
                        off, inst, col, q = _ring_offsets(p, ld)
                        base = 0                                # the scalar base is x + w0
                    else:
                        off, t0, col, q = _tile_offsets(p, ld)
                        inst, base = 0, t0 * ld * 8             # the scalar base is x + t0 ld + row_begin
                    assert int(off.min()) >= 0 and int(off.max()) < TWO32, (form, p, ld, int(off.min()), int(off.max()))
                    # the 16 bytes a lane reads in the LAST slab (first row n - 8: a slab is eight rows that all exist) end inside the
                    # n rows of column `col`, and so inside its ld elements; in the first slab they start at or behind its first row
                    first = base + off + inst                   # bytes from x, the slab's first row 0
                    last_end = first + (n - 8) * 8 + 16
                    assert np.all(first >= col * ld * 8) and np.all(last_end <= (col * ld + n) * 8) and 8 <= n <= ld
                    if int(off.max()) >= 1 << 31:
                        edge["ring_hi" if form == RING_SADDR else "tile_hi"] += 1
    # every form, every strip count and both halves of the offset range were reached
    assert {k[0] for k in seen} == set(range(8)), seen
    assert {k[1] for k in seen if k[0] == RING_SADDR} == {0, 1, 2}
    assert edge["ring_hi"] > 0 and edge["tile_hi"] > 0, edge


def test_guards_are_tight(L):
    """at the guards themselves: the ring's largest offset at ld_max(p) stays below p ld 8 + 65,536 (the slack covers the pre-decrement of
    at most three KiB), ld >= 8 keeps the pre-decremented offsets at or above zero, and the shared-slab / one-read forms end at 2^25"""
    # ring: the largest offset is ((16 (nt - 1) - 1) ld + 6) 8 + CEN 1024 <= p ld 8 + 65536 - 1 whenever the guard holds
    for p in P_SWEEP:
        nt = (p + 2 + 15) // 16
        if nt > 7 or nt < 4 or p < 16 * (nt - 1):
            continue
        ld = ld_max(p)
        off, inst, col, q = _ring_offsets(p, ld)
        assert 0 <= int(off.min()) and int(off.max()) < p * ld * 8 + 65536 < TWO32
        assert int(-inst.min()) <= 3 * 1024 < 65536             # the pre-decrement adds at most CEN KiB
        # ld >= 8 keeps every pre-decremented offset at or above zero: 16 ld 8 bytes per fragment against 1 KiB
        assert int(_ring_offsets(p, 8)[0].min()) >= 0
    assert int(_ring_offsets(100, 2)[0].min()) < 0              # the 1-row shard with ld = 2 that once read 4 GB away (seven tile columns)
    # shared-slab / one-read: lane 15 of a tile at ld = 2^25 is 15 2^25 8 + 48 < 2^32 still, but the guard is stated on the tile (16 ld 8)
    off, _, _, _ = _tile_offsets(130, (1 << 25) - 2)
    assert int(off.max()) == (15 * ((1 << 25) - 2) + 6) * 8 < TWO32
    out = (C.c_int64 * 2)()
    for p, inside in ((130, SB), (161, WD3), (225, WD4), (500, WD_UNITS)):
        assert L.oemgpu_selftest_gram_form(4099, (1 << 25) - 2, p, 1, 256, out) == 0 and out[0] == inside
        assert L.oemgpu_selftest_gram_form(4099, 1 << 25, p, 1, 256, out) == 0 and out[0] == BLK


def test_bad_arguments_are_refused(L):
    out = (C.c_int64 * 2)()
    for args in ((0, 8, 4, 1, 256), (8, 0, 4, 1, 256), (8, 8, 0, 1, 256), (8, 8, 4, 1, 0)):
        assert L.oemgpu_selftest_gram_form(*args, out) != 0
    assert L.oemgpu_selftest_gram_form(8, 8, 4, 1, 256, None) != 0


def test_the_exact_reference_of_the_large_ld_tests_is_exact():
    """tests/test_gpu_large_ld.py holds the moment kernels to array_equal on entries k / 8, |k| <= 32, against the int64 product of 8 z:
    every product is a multiple of 1 / 64 below 16 in magnitude and every sum of 40,002 of them is below 2^53 / 64, so float64 holds every
    partial sum exactly in any order; and the blocked product the GPU tests use is numpy's int64 product"""
    from tests.exact_gram import exact_gram
    assert 40002 * 32 * 32 < 2 ** 53
    rng = np.random.default_rng(5)
    k = rng.integers(-32, 33, size=(4099, 60))
    k[:, -1] = 8
    k[:7] = 32                                                 # the bound itself in a few rows
    g = exact_gram(k)
    assert g.dtype == np.int64 and np.array_equal(g, k.T @ k)
    z = k / 8.0                                                # the values the kernels read: float64 sums in two different orders are the same bits
    ref = g / 64.0
    assert np.array_equal(z.T @ z, ref) and np.array_equal(z[::-1].T @ z[::-1], ref) and np.array_equal(np.einsum("ij,ik->jk", z, z), ref)
    worst = np.full((40002, 2), 32, dtype=np.int64)
    assert np.array_equal(exact_gram(worst), np.full((2, 2), 40002 * 1024))
