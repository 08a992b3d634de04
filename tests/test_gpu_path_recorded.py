"""The row-split path kernel (path_small.hip, p <= 208) against its own recorded outputs.

tests/golden/path_fixed_part/<case>.npz holds, for each case of tests/path_fixed_part_cases.py, what the kernel gave at the commit
before its cycles outside the OEM rounds were cut (tools/record_path_outputs.py) and what the CPU oracle gives.  A change there
(loop structure, Lanczos step, Ritz looks, prologue) must leave
  1. lambda, niter and the number of Lanczos steps IDENTICAL, and
  2. beta and d within last bits: |new - recorded| <= |recorded - oracle|, the recorded kernel's own distance from the oracle on that
     case, which the fixture stores as dist_beta / dist_d.
The inputs come from fixed seeds; nothing outside the repository is read."""
from pathlib import Path

import numpy as np
import pytest

from tests import path_fixed_part_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "path_fixed_part"


@pytest.fixture(scope="module")
def oa():
    import torch
    assert torch.cuda.is_available()
    import oem_amd
    oem_amd.lib()
    return oem_amd


@pytest.mark.parametrize("name", cases.RECORDED)
def test_recorded_case(oa, name):
    rec = np.load(GOLDEN / f"{name}.npz")
    fit, steps, capped = cases.run_device(oa, name)
    beta, lam, niter = cases.flat(fit, "beta"), cases.flat(fit, "lambda"), cases.flat(fit, "niter").astype(np.int32)
    db, dd = float(np.abs(beta - rec["beta"]).max()), abs(float(fit["d"]) - float(rec["d"]))
    print(f"{name}: |beta - recorded| {db:.3g} (bound {float(rec['dist_beta']):.3g}), |d - recorded| {dd:.3g} "
          f"(bound {float(rec['dist_d']):.3g}), steps {steps} (recorded {int(rec['steps'])})")
    assert np.array_equal(lam, rec["lam"]), name
    assert np.array_equal(niter, rec["niter"]), (name, niter, rec["niter"])
    assert steps == int(rec["steps"]) and capped == int(rec["capped"]), (name, steps, capped)
    # the stored distances are what they say (the bound is read from data, and the data is checked)
    assert float(rec["dist_beta"]) == float(np.abs(rec["beta"] - rec["oracle_beta"]).max())
    assert float(rec["dist_d"]) == abs(float(rec["d"]) - float(rec["oracle_d"]))
    assert db <= float(rec["dist_beta"]), (name, db, float(rec["dist_beta"]))
    assert dd <= float(rec["dist_d"]), (name, dd, float(rec["dist_d"]))
