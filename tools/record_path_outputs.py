#!/usr/bin/env python3
"""Record what the row-split path kernel gives for the cases of tests/path_fixed_part_cases.py, beside the CPU oracle's outputs:

    python tools/record_path_outputs.py            # writes tests/golden/path_fixed_part/<case>.npz

Run it on the commit whose outputs are to be kept (the parent of a change that may move last bits); the change is then held to
|new - recorded| <= |recorded - oracle| by tests/test_gpu_path_recorded.py.  Inputs come from fixed seeds and are not stored."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import oem_amd as oa  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import path_fixed_part_cases as cases  # noqa: E402

out = ROOT / "tests" / "golden" / "path_fixed_part"
out.mkdir(parents=True, exist_ok=True)
for name in cases.RECORDED:
    x, y, kw = cases.case(name)
    fit, steps, capped = cases.run_device(oa, name)
    ref = orc.fit_dense(x, y, **kw)
    rec = dict(beta=cases.flat(fit, "beta"), lam=cases.flat(fit, "lambda"), niter=cases.flat(fit, "niter").astype(np.int32),
               d=np.float64(fit["d"]), steps=np.int32(steps), capped=np.int32(capped),
               oracle_beta=cases.flat(ref, "beta"), oracle_lam=cases.flat(ref, "lambda"),
               oracle_niter=cases.flat(ref, "niter").astype(np.int32), oracle_d=np.float64(ref["d"]))
    rec["dist_beta"] = np.float64(np.abs(rec["beta"] - rec["oracle_beta"]).max())
    rec["dist_d"] = np.float64(abs(rec["d"] - rec["oracle_d"]))
    np.savez_compressed(out / f"{name}.npz", **rec)
    same = np.array_equal(rec["niter"], rec["oracle_niter"])
    print(f"{name:30s} steps {steps:3d} d {fit['d']:.17g} |beta - oracle| {rec['dist_beta']:.3g} |d - oracle| {rec['dist_d']:.3g} "
          f"niter {'equal' if same else 'DIFFER'} ({(out / (name + '.npz')).stat().st_size} bytes)")
