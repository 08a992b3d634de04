"""oem_fit_logistic_dense_multi returns the bytes it returned before its driver learned fold instances and its row pass a fold mask:
tests/golden/logistic_multi_bytes.json holds the SHA-256 hashes that tests/logistic_multi_golden.py wrote on that earlier build."""
import json
from pathlib import Path

import pytest

from tests import logistic_multi_golden as G

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "logistic_multi_bytes.json").read_text())


def test_the_golden_file_covers_the_problems():
    assert sorted(GOLDEN) == sorted(G.PROBLEMS)


@pytest.mark.parametrize("name", sorted(G.PROBLEMS))
def test_plain_call_keeps_its_bytes(name):
    import oem_amd
    got = G.run(oem_amd, name)
    assert got == GOLDEN[name], {k: (got[k][:12], GOLDEN[name][k][:12]) for k in got if got[k] != GOLDEN[name][k]}
