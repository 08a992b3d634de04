"""The entries of oem_amd/api.py that demand a device tensor build the option blocks they built, and every entry returns the bytes it
returned, before the option prologues, the cross-validation fronts and tails and the many-response outputs became one helper each:
tests/golden/api_front.json holds what tests/api_front_golden.py wrote on that earlier tree ("options_gpu" and "bytes_gpu")."""
import json
from pathlib import Path

import pytest

from tests import api_front_golden as G

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "api_front.json").read_text())


@pytest.fixture(scope="module")
def api():
    from oem_amd import api
    return api


def test_the_golden_file_covers_the_cases():
    assert sorted(GOLDEN["options_gpu"]) == sorted(f"{e}/{name}" for e in G.GPU_OPTION_ENTRIES for name in G.option_grid(e))
    assert sorted(GOLDEN["bytes_gpu"]) == sorted(G.bytes_cases())


@pytest.mark.parametrize("key", sorted(GOLDEN["options_gpu"]))
def test_option_block_keeps_its_arguments(api, key):
    entry, name = key.split("/")
    got = json.loads(json.dumps(G.run_options(api, entry, name, gpu=True)))
    assert got == GOLDEN["options_gpu"][key], {k: (v, GOLDEN["options_gpu"][key]["args"].get(k)) for k, v in got["args"].items()
                                               if v != GOLDEN["options_gpu"][key]["args"].get(k)}


@pytest.mark.parametrize("name", sorted(GOLDEN["bytes_gpu"]))
def test_result_keeps_its_keys_and_bytes(api, name):
    got, want = G.run_bytes(api, name), GOLDEN["bytes_gpu"][name]
    assert [f["keys"] for f in got] == [f["keys"] for f in want]
    diff = [(i, k) for i, (f, g) in enumerate(zip(got, want)) for k in f["sha"] if f["sha"][k] != g["sha"][k]]
    assert not diff, diff
