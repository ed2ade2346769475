"""One process with ``PDEHIP_JIT_GRAPH=1 PDEHIP_TILE2D=0`` (read once per process): the fixed-step Euler loop of a one-pass expression without explicit
time replays a captured block of 16 steps from the third step on (``replay_blocks``, csrc/pdehip_jit.hip).  Runs `RUNS` through ``eq.solve``, the
71-step ones also as two identical calls of the C loop (`same_call_twice`: the second finds the first one's graph in the cache), writes the final
states to the ``.npz`` file named on the command line and reports the kernel names as one JSON line.  Launched by tests/test_hip_jit_replay.py, which computes the same runs without the two variables."""
from __future__ import annotations

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "py-pde_amd", ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import tile2d_cases as T  # noqa: E402

import pde_hip  # noqa: E402
from pde_hip.device import DeviceArray  # noqa: E402

EXPR = T.EXPRESSIONS[2]["allen_cahn"]
DT = T.DT[2]
# 2 plain steps, then whole blocks of 16 from four blocks on: 66 = head + four blocks and nothing left, 71 = an odd remainder of 5 (the parity
# of the buffer the result is in), 65 = one short (no replay)
STEPS = (66, 71, 65)
RUNS = [(shape, dtype, steps) for shape, dtype in (((24, 40), "float64"), ((6, 8, 16), "float64"), ((24, 40), "float32")) for steps in STEPS]


def run_id(shape, dtype, steps) -> str:
    return f"{'x'.join(map(str, shape))}-{dtype}-{steps}"


def problem(shape, dtype):
    """(equation, state): walls along the first axis, periodic along the second (2-D); walls, periodic, walls (3-D)"""
    if len(shape) == 2:
        return T.jit_eq(2, "allen_cahn", "lp"), T.state_of(2, shape, "lp", dtype)
    grid = pde_hip.CartesianGrid([[0, 1.0 * shape[0]], [0, 0.9 * shape[1]], [0, 1.1 * shape[2]]], shape, periodic=[False, True, False])
    return pde_hip.PDE(EXPR, bc="auto_periodic_neumann"), pde_hip.ScalarField(grid, T.field_data(shape, dtype), dtype=np.dtype(dtype))


def same_call_twice(backend, eq, state, steps: int):
    """``pdehip_jit_euler_run`` twice with the same handles, face tables, buffers and dt (``eq.solve`` makes new ones per call): everything the
    key of a captured block holds, so the second call finds the graph the first one captured.  The final states of both calls."""
    rhs = backend.make_expression_rhs(eq, state)
    a, b = DeviceArray(rhs.info), DeviceArray(rhs.info)
    out = []
    for _ in range(2):
        a.set_valid(state.data, stream=backend.stream)
        res = rhs.euler_loop(a, b, DT, 0.0, steps)
        assert res is not None
        out.append(np.array(res.get_valid(stream=backend.stream)))
    return out


def main() -> int:
    backend = pde_hip.get_backend("hip")
    lib = backend._lib
    states, names = {}, {}
    for shape, dtype, steps in RUNS:
        rid = run_id(shape, dtype, steps)
        eq, state = problem(shape, dtype)
        states[rid] = T.solve(eq, state, 0.0, DT, steps)
        names[rid] = lib.last_kernel_name().decode()
        if steps == 71:
            states[rid + "-first"], states[rid + "-second"] = same_call_twice(backend, eq, state, steps)
            names[rid + "-second"] = lib.last_kernel_name().decode()
    np.savez(sys.argv[1], **states)
    print("JITREPLAY " + json.dumps(names), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
