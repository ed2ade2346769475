"""One process = one setting of the tuning knobs of the run-time built one-level sweeps (``PDEHIP_JIT_RY`` / ``_CZ`` / ``_WY`` / ``_BLOCKS`` are read
once per process): a handful of the cases of tests/jit_cases.py - slope and stage sweeps, walls, tails, 3-D - with the instance names and the
bit comparisons reported as one JSON line.  Launched by tests/test_hip_jit_instances.py::test_tuning_knobs_give_the_same_bits."""
from __future__ import annotations

import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "py-pde_amd", ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import jit_cases as J  # noqa: E402
from jit_device import Runner  # noqa: E402

import pde_hip  # noqa: E402


def main() -> int:
    knobs = {key: int(os.environ.get(f"PDEHIP_JIT_{key.upper()}", "0") or 0) for key in ("ry", "cz", "wy", "blocks")}
    runner = Runner(pde_hip.get_backend("hip")._lib, knobs)
    report = {"knobs": knobs, "cases": {}}
    for c in J.worker_cases():
        name, bad = runner.run(c)
        report["cases"][c.id] = {"name": name, "differences": bad}
    print("JITKNOBS " + json.dumps(report), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
