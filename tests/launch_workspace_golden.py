"""Produces tests/golden/launch_workspace.json: where the launch-per-iteration drivers kept every region of their workspaces BEFORE
oem_amd/csrc/path_large_layout.hpp named them, as a plain restatement of the hand arithmetic of commit 7dbe463 (each expression with the
file:line it was read from), and what oemgpu_selftest_plan returned at that commit.  tests/test_launch_workspace_cpu.py holds the
header (compiled by the host compiler alone) and today's plan to this file.

    python -m tests.launch_workspace_golden OUT.json            the restatement; the "plan" section is carried over from the file as it is
    python -m tests.launch_workspace_golden OUT.json --plan     ... and the "plan" section recorded from the library of THIS tree
                                                                (done once, on a build of commit 7dbe463)

All offsets and sizes are counted in doubles.  A region is [offset, length].
"""
import json
import sys
from pathlib import Path

COMMIT = "7dbe463"
# path_large.hip:33-34, 738, 851, 1108, 1193 and common.hpp:445 at that commit
STATE_DBL, MAXL, FMAXB, SYM_TB, SPK_HC, SPW_T_DOUBLES = 16, 512, 1024, 128, 32, 1024
SPK_TILE = SYM_TB * SYM_TB

QS = [2, 100, 288, 289, 511, 512, 513, 1024, 1025, 2047, 2048, 2049, 3000, 4095, 4096, 4097, 6145, 8192, 12289, 20000]
WIDE_NS = [3, 64, 65, 200, 1000, 2048, 2049, 2100, 5000]
SPW_NS = [1, 40, 1000, 65537]


def wide_ps(n):
    return sorted({p for p in (n, 2 * n + 3, 1100, 20000) if p >= n})


def _regions(pairs):
    """[(name, length), ...] laid end to end -> {name: [offset, length], ..., "total": end}"""
    out, at = {}, 0
    for name, length in pairs:
        out[name] = [at, length]
        at += length
    out["total"] = at
    return out


def large_work(q):
    """PathArgs::work of run_path_large (and the state | beta | g head of it that the p >= n drivers use)"""
    v = q + 8
    sym_part = 2 * (q // SYM_TB) * q + 16 if q == 4096 else 0                     # path_large.hip:1703 sym_part_doubles
    uf = 2 * (q + 8)                                                               # path_large.hip:1702 update_uf_doubles
    total = STATE_DBL + 5 * (q + 8) + 2 * MAXL + 64 + 16 + 2 * (q + 8) + FMAXB + 16 + 2 * (q + 8) + 6 * (q + 8) + sym_part + uf    # path_large.hip:1712-1713
    beta = STATE_DBL                                                               # path_large.hip:1779
    g, vv, vp, w = beta + v, beta + 2 * v, beta + 3 * v, beta + 4 * v              # path_large.hip:1779
    T = w + v                                                                      # path_large.hip:1780
    fbase = T + 2 * MAXL + 64                                                      # path_large.hip:1887, 1946
    fdone, Bv = fbase + 8, fbase + 16                                              # path_large.hip:1889-1890, 1947-1948
    flags = Bv + 2 * (q + 8)                                                       # path_large.hip:1891
    gbase = Bv + 2 * (q + 8) + FMAXB                                               # path_large.hip:1949
    Uv = gbase + 16                                                                # path_large.hip:1951
    LZ = T + 2 * MAXL + 64 + 16 + 2 * (q + 8) + FMAXB + 16 + 2 * (q + 8)           # path_large.hip:1795
    Vc, Vp, Wb = LZ, LZ + 2 * (q + 8), LZ + 4 * (q + 8)                            # path_large.hip:1796
    SP = LZ + 6 * (q + 8)                                                          # path_large.hip:1797
    SS = SP + 2 * (q // SYM_TB) * q                                                # path_large.hip:1896 (used at q = 4096 only)
    ufo = total - uf                                                               # path_large.hip:1716 update_uf
    sym = q == 4096
    return {"state": [0, STATE_DBL], "beta": [beta, v], "g": [g, v], "v": [vv, v], "vp": [vp, v], "w": [w, v], "T": [T, 2 * MAXL + 64],
            "fstate": [fbase, 8], "fdone": [fdone, 8], "Bv": [Bv, 2 * v], "flags": [flags, FMAXB], "gstate": [gbase, 16], "Uv": [Uv, 2 * v],
            "Vc": [Vc, 2 * v], "Vp": [Vp, 2 * v], "Wb": [Wb, 2 * v], "sym_part": [SP, SS - SP if sym else 0], "sym_state": [SS if sym else SP, 16 if sym else 0],
            "uf": [ufo, uf], "total": total}


def spk_work(q):
    """PathArgs::sympk: the packed lower triangle and what the (head, product) pairs keep behind it"""
    if q <= 1024:                                                                  # path_large.hip:1476
        return _regions([(k, 0) for k in ("blocks", "P", "B", "flags", "sstate", "done", "nz32", "gen")]) | {"zero_from": 0, "zero_doubles": 0}
    nblk = (q + SYM_TB - 1) // SYM_TB                                              # path_large.hip:1109 spk_nblk
    ntile = nblk * (nblk + 1) // 2                                                 # path_large.hip:1110 spk_ntile
    qpad = nblk * SYM_TB                                                           # path_large.hip:1477, 1805
    total = ntile * SPK_TILE + nblk * qpad + 2 * qpad + FMAXB + 16 + 8 + qpad // 32 + 8 + 4 * FMAXB + 16      # path_large.hip:1480
    P = ntile * SPK_TILE                                                           # path_large.hip:1455, 1806
    B = P + nblk * qpad                                                            # path_large.hip:1806
    flags = B + 2 * qpad                                                           # path_large.hip:1920
    SS = B + 2 * qpad + FMAXB                                                      # path_large.hip:1921
    fdone = B + 2 * qpad + FMAXB + 16                                              # path_large.hip:1922
    nz32 = B + 2 * qpad + FMAXB + 16 + 8                                           # path_large.hip:1814, 1923
    gen = B + 2 * qpad + FMAXB + 16 + 8 + qpad // 32 + 8                           # path_large.hip:1924
    zero = 2 * qpad + FMAXB + 16 + 8 + qpad // 32 + 8 + 4 * FMAXB + 16             # path_large.hip:1810 (from B on)
    return {"blocks": [0, P], "P": [P, nblk * qpad], "B": [B, 2 * qpad], "flags": [flags, FMAXB], "sstate": [SS, 16], "done": [fdone, 8],
            "nz32": [nz32, qpad // 32 + 8], "gen": [gen, 4 * FMAXB + 16], "total": total, "zero_from": B, "zero_doubles": zero}


def wide_nr(n):                                                                    # path_large.hip:2012-2018
    need = (n + 63) // 64
    return next((v for v in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32) if v >= need), 0)


def wide_layout(n):                                                                # path_large.hip:2023-2030 -> (nb, rb, nr)
    nb = 1 if n <= 2048 else (n + 2047) // 2048
    rb = (n + nb - 1) // nb
    return nb, rb, wide_nr(rb)


def wide_workgroups(n, p):                                                         # path_large.hip:2022, 2031-2037
    nr = wide_layout(n)[2]
    nw = 16 if nr <= 8 else (8 if nr <= 16 else 4)
    return max(1, min(256, (p + nw - 1) // nw))


def wide_scratch(n, p):
    """WideArgs::scratch as run_path_wide_nr (one row block) and run_path_wide_blocks lay it out: the engine's own part"""
    nb, _, nr = wide_layout(n)
    W, npad, rows = wide_workgroups(n, p), 64 * nr, nb * 64 * nr                   # common.hpp:419-420
    own = W * npad + 5 * rows + 2 * MAXL + 64 + 16 + 2 + FMAXB + 64 + nb * (p + 8)      # path_large.hip:2042
    r = W * npad                                                                   # path_large.hip:2582 (2497: the blocks form skips it)
    t, v, vp, w = r + rows, r + 2 * rows, r + 3 * rows, r + 4 * rows               # path_large.hip:2582, 2497
    T = w + rows                                                                   # path_large.hip:2583, 2498
    SS, fdone, flags = T + 2 * MAXL + 64, T + 2 * MAXL + 64 + 16, T + 2 * MAXL + 64 + 16 + 2      # path_large.hip:2584-2586
    gb = T + 2 * MAXL + 64 + 16 + 2 + FMAXB + 64                                   # path_large.hip:2499
    return {"W": W, "nb": nb, "nr": nr, "P": [0, W * npad], "r": [r, rows], "t": [t, rows], "v": [v, rows], "vp": [vp, rows], "w": [w, rows],
            "T": [T, 2 * MAXL + 64], "sstate": [SS, 16], "done": [fdone, 2], "flags": [flags, FMAXB + 64], "gb": [gb, nb * (p + 8)], "own_total": own}


def spw_vec(n):
    """SpwArgs::vec of run_path_sparse_wide"""
    return {"t": [0, n], "v": [n, n], "vp": [2 * n, n], "w": [3 * n, n], "T": [4 * n, SPW_T_DOUBLES],      # path_large.hip:2718
            "total": 4 * n + SPW_T_DOUBLES}                                        # path_large.hip:2723, sparse_wide.hip:251, api.hip:3143


def restatement():
    return {"large": {str(q): large_work(q) for q in QS}, "spk": {str(q): spk_work(q) for q in QS},
            "wide": {"%dx%d" % (n, p): wide_scratch(n, p) for n in WIDE_NS for p in wide_ps(n)},
            "spw": {str(n): spw_vec(n) for n in SPW_NS}}


# ---- oemgpu_selftest_plan over the grids of tests/test_host_api.py (its two plan tests), every penalty set, default options
PLAN_QS = sorted(set(list(range(2, 301)) + [q + d for q in (512, 1024, 2048, 3457, 4096, 8192) for d in (-1, 0, 1)] + list(range(320, 4200, 97)) + [5000, 12000, 20000]))
PLAN_NS = (3, 40, 64, 100, 128, 192, 200, 256, 500, 700, 960, 1000, 1024, 1500, 2048, 2100, 5000)


def plan_ps(n):
    return sorted(p for p in {n, n + 1, 2 * n + 3, 1100, 1500, 2500, 2912, 6300, 9000, 12200, 20000, 30000, 100000} if p >= n)


def plan_values():
    """{"gram": {q: [reserved_bytes per penalty set]}, "wide": {"nxp": [[reserved_bytes, scratch_have_doubles] per penalty set]}}"""
    from tests.test_host_api import _PEN_SETS, _plan
    gram = {str(q): [_plan(q, pens, groups=grp)[2] for pens, grp in _PEN_SETS] for q in PLAN_QS}
    wide = {"%dx%d" % (n, p): [list(_plan(p, pens, groups=grp, wide_n=n)[2::2]) for pens, grp in _PEN_SETS] for n in PLAN_NS for p in plan_ps(n)}
    return {"gram": gram, "wide": wide}


if __name__ == "__main__":
    out = Path(sys.argv[1])
    doc = restatement()
    doc["header"] = ("Offsets and sizes in doubles, restated by tests/launch_workspace_golden.py from the expressions of commit %s; "
                     "\"plan\": oemgpu_selftest_plan's reserved_bytes and scratch_have_doubles, recorded once from a build of commit %s." % (COMMIT, COMMIT))
    doc["plan"] = plan_values() if "--plan" in sys.argv[2:] else json.loads(out.read_text())["plan"]
    out.write_text(json.dumps(doc, separators=(",", ":"), sort_keys=True) + "\n")
