"""The launch-per-iteration host drivers of oem_amd/csrc/path_large.hip (run_path_large, run_path_wide_nr, run_path_wide_blocks,
run_path_sparse_wide) enqueue exactly what they enqueued before their workspaces were named in path_large_layout.hpp and their batch
loops, Lanczos looks and engine choice became one function each: on the seeded problems of tests/launch_drivers_golden.py -- one per
branch of the drivers -- today's tree returns the bytes recorded from the tree before (tests/golden/launch_drivers_bytes.json:
beta, lambda, niter, d, and the loss where the case computes one)."""
import json
from pathlib import Path

import pytest

from tests import launch_drivers_golden as G

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "launch_drivers_bytes.json").read_text())


@pytest.fixture(scope="module")
def oa():
    import torch
    assert torch.cuda.is_available()
    import oem_amd
    oem_amd.lib()
    return oem_amd


def test_the_golden_file_has_every_case():
    assert set(GOLDEN) == set(G.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_same_bytes_as_before_the_drivers_were_refactored(oa, name, monkeypatch):
    for s in G.SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for s in G.CASES[name]["env"]:
        monkeypatch.setenv(s, "1")
    rec, engine = G.run(oa, name)
    assert engine == G.CASES[name]["engine"], (name, engine)
    want = GOLDEN[name]
    assert set(rec) == set(want), name
    for key in sorted(want):
        assert rec[key] == want[key], (name, key)
