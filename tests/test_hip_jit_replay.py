"""The replay route of ``pdehip_jit_euler_run`` (``PDEHIP_JIT_GRAPH=1``): two plain steps, then a captured block of 16 steps replayed while whole
blocks remain, the rest as plain steps.  The knobs are read once per process, so tests/jit_replay_worker.py runs in a child with
``PDEHIP_JIT_GRAPH=1 PDEHIP_TILE2D=0``; this process computes the same runs by the default route.  The replayed launches are the launches of the
plain loop (and the tile kernel of the default route gives the bits of the one-level kernels: tests/test_hip_tile2d_instances.py), so the states
must be equal byte for byte; fp64 also equals the host shim byte for byte.

What this can and cannot show: the library exports nothing that says whether a graph was launched, and a capture that cannot be instantiated
leaves its steps to the plain loop, with the same bytes and the same last kernel name.  Equal bytes prove that the route taken under
``PDEHIP_JIT_GRAPH=1`` - the head, the replayed blocks with their buffer parity, the remainder - agrees with the plain launches, not that a graph
ran; likewise the 65-step runs only show that one step short of a replay gives the right result.  Which step counts replay is pinned on the CPU
(tests/test_tile2d_cases_cpu.py::test_when_the_captured_block_is_replayed).

fp32 against the shim (which rounds the stencil values to fp32 before the epilogue, the kernels keep them in fp64 registers) within a bound that is
derived, not measured.  One Euler step u -> u + dt (u - u^3 + lap u) with dt = 0.01 on this grid (dx = 1 and 0.9: the stencil weights sum to
4 + 4 / 0.81 < 8.94 in absolute value, dt * 8.94 < 1) has non-negative weights whose sum is 1 + dt (1 - 3 xi^2) <= 1.01, the conditions copy or
reflect cells with factors of modulus <= 1: a difference between two states grows by at most 1.01 per step in the maximum norm.  A step adds at
most one fp32 spacing below 1, 2^-24 (two roundings of results that differ), plus dt * 2^-24 * |lap u| < 0.09 * 2^-24 for the rounded stencil value
while |u| < 1.  After n steps: n * 1.01^n * 1.09 * 2^-24 (9.4e-6 for n = 71)."""

from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import jit_cases as J
import jit_replay_worker as W
import numpy as np
import pytest
import tile2d_cases as T

pytestmark = pytest.mark.gpu

WORKER = Path(__file__).resolve().parent / "jit_replay_worker.py"


def fp32_bound(steps: int) -> float:
    return steps * 1.01 ** steps * 1.09 * 2.0 ** -24


@pytest.fixture(scope="module")
def replayed(tmp_path_factory):
    """(states, kernel names) of the worker's runs"""
    out = tmp_path_factory.mktemp("replay") / "states.npz"
    env = dict(os.environ)
    env.update(PDEHIP_JIT_GRAPH="1", PDEHIP_TILE2D="0")
    proc = subprocess.run([sys.executable, str(WORKER), str(out)], capture_output=True, text=True, timeout=300, env=env)
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("JITREPLAY ")]
    assert proc.returncode == 0 and lines, (proc.stdout[-2000:], proc.stderr[-2000:])
    with np.load(out) as data:
        return {k: data[k] for k in data.files}, json.loads(lines[-1][len("JITREPLAY "):])


@pytest.mark.parametrize("run", W.RUNS, ids=lambda r: W.run_id(*r))
def test_replayed_blocks_give_the_bytes_of_the_default_route(replayed, run):
    shape, dtype, steps = run
    states, names = replayed
    rid = W.run_id(*run)
    got = states[rid]
    # the one-level instance of the grid, faces on the fly: neither the tile kernel nor the generic one
    assert names[rid] == J.kernel_name(J.plan(tuple(shape), np.dtype(dtype), fused=True)), names[rid]
    eq, state = W.problem(shape, dtype)
    here = T.solve(eq, state, 0.0, W.DT, steps)
    assert got.dtype == here.dtype == np.dtype(dtype) and got.shape == tuple(shape)
    assert np.isfinite(got).all() and not np.array_equal(got, state.data)
    assert got.tobytes() == here.tobytes(), f"{rid}: max abs {np.abs(got - here).max():.3e} against the default route"
    if steps == 71:      # the C loop called twice with one set of handles, tables and buffers: the second call's key is the first one's
        assert names[rid + "-second"] == names[rid], rid
        assert states[rid + "-first"].tobytes() == got.tobytes() and states[rid + "-second"].tobytes() == got.tobytes(), rid
    ref = T.shim_solve(eq, state, 0.0, W.DT, steps)
    if dtype == "float64":
        assert got.tobytes() == ref.tobytes(), f"{rid}: max abs {np.abs(got - ref).max():.3e} against the host shim"
    else:
        err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
        print(f"{rid}: fp32 max abs against the shim {err:.3e}, bound {fp32_bound(steps):.3e}")
        assert np.abs(ref).max() < 1 and err <= fp32_bound(steps), rid


def test_the_runs_are_what_they_claim_to_be():
    assert {s for _, _, s in W.RUNS} == {65, 66, 71} and len(W.RUNS) == 9
    # 66: the head and four blocks; 71: an odd remainder; 65: one step short of a replay
    assert (66 - 2) % 16 == 0 and (66 - 2) // 16 == 4 and (71 - 2) % 16 == 5 and (65 - 2) < 4 * 16
