"""The workspaces of the launch-per-iteration drivers (oem_amd/csrc/path_large.hip) are laid out in ONE place,
oem_amd/csrc/path_large_layout.hpp, which a host compiler reads without HIP.  This file compiles a small program against that header,
prints every region, and holds the output to tests/golden/launch_workspace.json: the offsets the drivers used when they were hand
arithmetic (tests/launch_workspace_golden.py restates those expressions line by line), so that naming the regions moved none of them.
The same golden file holds what oemgpu_selftest_plan returned for the workspace sizes before the header existed.
"""
import json
import subprocess
from pathlib import Path

import pytest

from tests import launch_workspace_golden as G

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / "tests" / "golden" / "launch_workspace.json").read_text())

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "path_large_layout.hpp"
using namespace oemgpu;
#define R(S, f) printf(" " #f "=%zu,%zu", S.f.off, S.f.len)
int main(int argc, char **argv)
{
    for (int k = 1; k + 2 < argc; k += 3) {
        const char kind = argv[k][0];
        const int a = atoi(argv[k + 1]), b = atoi(argv[k + 2]);
        if (kind == 'l') { const LargeWork L = large_work(a); printf("large %d", a); R(L, state); R(L, beta); R(L, g); R(L, v); R(L, vp); R(L, w); R(L, T); R(L, fstate); R(L, fdone); R(L, Bv);
                           R(L, flags); R(L, gstate); R(L, Uv); R(L, Vc); R(L, Vp); R(L, Wb); R(L, sym_part); R(L, sym_state); R(L, uf); printf(" total=%zu\n", L.total); }
        if (kind == 's') { const SpkWork S = spk_work(a); printf("spk %d", a); R(S, blocks); R(S, P); R(S, B); R(S, flags); R(S, sstate); R(S, done); R(S, nz32); R(S, gen);
                           printf(" total=%zu zero_from=%zu zero_doubles=%zu\n", S.total, S.zero_from, S.zero_doubles); }
        if (kind == 'w') { const WideLayout lay = wide_layout(a); const int W = wide_workgroups(a, b); const WideScratch S = wide_scratch(a, b, W, lay); printf("wide %dx%d W=%d nb=%d nr=%d", a, b, W, lay.nb, lay.nr);
                           R(S, P); R(S, r); R(S, t); R(S, v); R(S, vp); R(S, w); R(S, T); R(S, sstate); R(S, done); R(S, flags); R(S, gb); printf(" own_total=%zu\n", S.own_total); }
        if (kind == 'v') { const SpwVec V = spw_vec(a); printf("spw %d", a); R(V, t); R(V, v); R(V, vp); R(V, w); R(V, T); printf(" total=%zu\n", V.total);
                           if (spw_vec_doubles(a) != V.total || V.T.len != 2 * MAXL) return 2; }
    }
    return 0;
}
"""

LARGE_ORDER = ["state", "beta", "g", "v", "vp", "w", "T", "fstate", "fdone", "Bv", "flags", "gstate", "Uv", "Vc", "Vp", "Wb", "sym_part", "sym_state", "uf"]
SPK_ORDER = ["blocks", "P", "B", "flags", "sstate", "done", "nz32", "gen"]
WIDE_ORDER = ["P", "r", "t", "v", "vp", "w", "T", "sstate", "done", "flags", "gb"]
SPW_ORDER = ["t", "v", "vp", "w", "T"]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """the header's tables as the compiled program prints them: {"large": {"q": {...}}, "spk": ..., "wide": {"nxp": ...}, "spw": ...}"""
    tmp = tmp_path_factory.mktemp("launch_workspace")
    src, exe = tmp / "print_layout.cpp", tmp / "print_layout"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "oem_amd" / "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    args = []
    for q in G.QS:
        args += ["l", str(q), "0", "s", str(q), "0"]
    for n in G.WIDE_NS:
        for p in G.wide_ps(n):
            args += ["w", str(n), str(p)]
    for n in G.SPW_NS:
        args += ["v", str(n), "0"]
    r = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True, timeout=60)
    out = {"large": {}, "spk": {}, "wide": {}, "spw": {}}
    for line in r.stdout.splitlines():
        kind, key, *fields = line.split()
        rec = {}
        for f in fields:
            name, val = f.split("=")
            rec[name] = [int(x) for x in val.split(",")] if "," in val else int(val)
        out[kind][key] = rec
    return out


@pytest.mark.parametrize("kind", ["large", "spk", "wide", "spw"])
def test_every_region_is_where_the_hand_arithmetic_had_it(printed, kind):
    assert set(printed[kind]) == set(GOLDEN[kind]) and len(printed[kind]) >= 4
    for key, want in GOLDEN[kind].items():
        assert printed[kind][key] == want, (kind, key)


def test_the_golden_file_is_the_restatement_of_the_parent_expressions():
    """tests/golden/launch_workspace.json is what tests/launch_workspace_golden.py writes (its layout sections: pure Python)"""
    again = json.loads(json.dumps(G.restatement()))
    for kind in ("large", "spk", "wide", "spw"):
        assert again[kind] == GOLDEN[kind], kind


@pytest.mark.parametrize("kind,order,total", [("large", LARGE_ORDER, "total"), ("spk", SPK_ORDER, "total"), ("wide", WIDE_ORDER, "own_total"),
                                              ("spw", SPW_ORDER, "total")])
def test_regions_follow_each_other_and_end_at_the_total(printed, kind, order, total):
    for key, rec in printed[kind].items():
        at = 0
        for name in order:
            off, length = rec[name]
            assert off >= at, (kind, key, name, off, at)              # no overlap with the region in front
            assert off == at, (kind, key, name, off, at)              # ... and no gap either: spare doubles belong to a region
            at = off + length
        assert at == rec[total], (kind, key, at, rec[total])
    for key, rec in printed["spk"].items():
        assert rec["zero_from"] == rec["B"][0] and rec["zero_from"] + rec["zero_doubles"] == rec["total"], key


def test_the_plan_reserves_what_it_reserved_before_the_header():
    """oemgpu_selftest_plan over the grids of tests/test_host_api.py's two plan tests: reserved_bytes (the Gram engines' workspace is
    path_large_work_doubles) and scratch_have_doubles (wide_scratch_doubles) as the build of the parent commit returned them"""
    now = G.plan_values()
    want = GOLDEN["plan"]
    assert set(now["gram"]) == set(want["gram"]) and set(now["wide"]) == set(want["wide"])
    for q, v in want["gram"].items():
        assert now["gram"][q] == v, q
    for key, v in want["wide"].items():
        assert now["wide"][key] == v, key
