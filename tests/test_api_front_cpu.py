"""The entries of oem_amd/api.py refuse what they refused, in the same words and the same order, and build the option blocks they built,
before their option prologues and cross-validation fronts became one helper each: tests/golden/api_front.json holds what
tests/api_front_golden.py wrote on that earlier tree (its "refusals" and "options" sections need no GPU)."""
import json
from collections import Counter
from pathlib import Path

import pytest

from tests import api_front_golden as G

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "api_front.json").read_text())


@pytest.fixture(scope="module")
def api():
    from oem_amd import api
    return api


def _defined_refusals(api):
    return [f"{entry}/{case}" for entry in G._entries(api) for case, _ in G.refusal_cases(entry)]


def test_the_golden_file_holds_the_cases(api):
    """every recorded case is one the module defines; at most one defined refusal in ten is missing (it reached the library when the file
    was written) and every entry keeps at least five; every option set of the host entries is there"""
    defined = _defined_refusals(api)
    assert set(GOLDEN["refusals"]) <= set(defined)
    assert 10 * (len(defined) - len(GOLDEN["refusals"])) <= len(defined), (len(defined), len(GOLDEN["refusals"]))
    per_entry = Counter(k.split("/")[0] for k in GOLDEN["refusals"])
    assert all(per_entry[entry] >= 5 for entry in G._entries(api)), per_entry
    assert sorted(GOLDEN["options"]) == sorted(f"{e}/{name}" for e in G.HOST_OPTION_ENTRIES for name in G.option_grid(e))


@pytest.mark.parametrize("key", sorted(GOLDEN["refusals"]))
def test_refusal_keeps_its_type_and_words(api, key):
    entry, case = key.split("/")
    assert G.run_refusal(api, entry, tuple(case.split("+"))) == GOLDEN["refusals"][key]


@pytest.mark.parametrize("key", sorted(GOLDEN["options"]))
def test_option_block_keeps_its_arguments(api, key):
    entry, name = key.split("/")
    got = json.loads(json.dumps(G.run_options(api, entry, name)))
    assert got == GOLDEN["options"][key], {k: (v, GOLDEN["options"][key]["args"].get(k)) for k, v in got["args"].items()
                                           if v != GOLDEN["options"][key]["args"].get(k)}


def test_n_less_than_p_warns(api):
    assert any("may be very slow when p > n" in w for w in GOLDEN["options"]["oem/n_less_than_p"]["warnings"])
