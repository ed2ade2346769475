"""The run-time built one-level kernels (csrc/pdehip_jit.hip) instance by instance: every case of tests/jit_cases.py through the C ABI
(tests/jit_device.py; tests/test_jit_cases_cpu.py pins the table to the planner header and keeps its cases from being vacuous).

Per case: the recorded name is the restated instance (RY, CZ, WY, 2-D / 3-D, faces on the fly, stage epilogue, tails code, planes per workgroup
and x-chunks), the slope, the stage result and the error cell have the reference's bits - fp64: the host shim, fp32: the fp64 twin rounded once -
and the WHOLE allocation of every array of the call is otherwise what was uploaded: ghost cells, the row padding behind a row that ends inside a
vector, the slack, the input, the earlier slopes.  NaNs by position.

The generic kernel runs the same grids from misaligned buffers; the stage entry point must refuse them and launch nothing.  The fixed-point
epilogue (kind 5) is reached through ``eq.solve``.  The two-level kernels (``pdehip_jit_euler2``, ``pdehip_jit_fused2``) run once per tile the two-step
planner gives them, against two passes of the same reference.  The tuning knobs are read once per process: one child process runs a handful of the cases with
``PDEHIP_JIT_RY=4 PDEHIP_JIT_WY=2 PDEHIP_JIT_BLOCKS=64``.
"""

from __future__ import annotations

import json
import os
import subprocess
import sys
import time
from pathlib import Path

import jit_cases as J
import numpy as np
import pytest
from implicit_cases import fixedpoint_run, oracle_rhs
from jit_device import Runner

import pde_hip

pytestmark = pytest.mark.gpu

REPORT = {"slope": set(), "stage": set(), "generic": set(), "fixed-point": set(), "two-level": set(), "knobs": set(), "cases": 0, "seconds": 0.0}


@pytest.fixture(scope="module")
def runner():
    return Runner(pde_hip.get_backend("hip")._lib)


@pytest.fixture(scope="module", autouse=True)
def _report(runner):
    start = time.perf_counter()
    yield
    REPORT["seconds"] = round(time.perf_counter() - start, 2)
    print("\nrun-time built one-level kernels, instances reached:")
    for key, v in REPORT.items():
        print(f"  {key}: " + ("".join(f"\n    {n}" for n in sorted(v)) if isinstance(v, set) else str(v)))


def _groups():
    """One item per (row of the table, type): its cases run in a loop"""
    out = {}
    for c in J.cases():
        out.setdefault(f"{c.what}-{c.dtype.name}", []).append(c)
    return out


GROUPS = _groups()


@pytest.mark.parametrize("group", list(GROUPS))
def test_instance(runner, group):
    bad = []
    for c in GROUPS[group]:
        with np.errstate(all="ignore"):
            name, diffs = runner.run(c)
        print(f"{c.id}: {name}" + "".join(f"\n    {d}" for d in diffs))
        bad += [f"{c.id}: {d}" for d in diffs]
        REPORT["stage" if c.stage else "slope"].add(name)
        REPORT["cases"] += 1
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c", J.generic_cases(), ids=[c.id for c in J.generic_cases()])
def test_misaligned_arrays_take_the_generic_kernel(runner, c):
    name, diffs = runner.run(c)
    assert name == f"pde_kernel<generic,{'double' if c.dtype == np.float64 else 'float'}> (run-time built)"
    assert not diffs, "\n".join(diffs)
    _, diffs = runner.run(c, stage_on_generic=True)        # *done = 0, nothing launched, nothing written, the mark's name left
    assert not diffs, "\n".join(diffs)
    REPORT["generic"].add(name)
    REPORT["cases"] += 2


@pytest.mark.parametrize("expr", ["0.7 * laplace(c)", "0.7 * laplace(c) - 0.5 * c"], ids=["diffusion", "decay"])
@pytest.mark.parametrize("shape", [(16, 32, 130), (16, 32, 131)], ids=["cz2", "cz2-tails"])
def test_fixed_point_epilogue(runner, shape, expr):
    """Kind 5 (``pdehip_jit_fixedpoint_run``): one implicit and one Crank-Nicolson solve against the numpy restatement of the reference's loops around
    the oracle's right-hand side.  ``0.7 * laplace(c)`` is recognised as the diffusion equation by the host and runs on the BUILT-IN stage sweep
    (``lap_march_kernel<..., mode=10, ...>``): the name says so.  The same equation with a decay term is what reaches the run-time built sweep;
    its reference is the oracle's diffusion rate minus ``0.5 * c`` (one rounding each for the product, the exact halving and the difference, in
    any order of the two terms)."""
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.UnitGrid(list(shape), periodic=[True, False, True])
    bc = ["periodic", {"value": 0.4}, "periodic"]
    eq = pde_hip.PDE({"c": expr}, bc=bc)
    diffusion = oracle_rhs(grid, pde_hip.DiffusionPDE(0.7, bc=bc))
    rhs = diffusion if "0.5" not in expr else (lambda valid, t: diffusion(valid, t) - 0.5 * valid)
    state = pde_hip.ScalarField(grid, np.random.default_rng(2).uniform(-1, 1, grid.shape))
    sweep = J.kernel_name(J.plan(shape, np.float64, stage=True, kind=5, nk=2, fused=True))
    assert "RY=1,CZ=2" in sweep and ("tails" in sweep) == (shape[-1] % 2 == 1)
    tail = " + fixed-point epilogue (st_kind 5: update and convergence norm in the sweep)"
    for solver, kw in (("implicit", {}), ("crank-nicolson", {"explicit_fraction": 0.3})):
        runner.mark()
        sol = pde_hip.solvers.SolverBase.from_name(solver, pde=eq, backend=backend, **kw)
        res = pde_hip.Controller(sol, t_range=0.05 * 2, tracker=None).run(state.copy(), 0.05)
        name = runner.lib.last_kernel_name().decode()
        print(f"{expr!r}, {solver}: {name}")
        want, evals, counts = fixedpoint_run(rhs, state.data, 0.05, 2, scheme=solver, **kw)
        assert sol.info["iterations"] == counts and sol.info["function_evaluations"] == evals
        assert np.array_equal(res.data, want), f"{expr!r}, {solver}: max abs {np.abs(res.data - want).max():.3e}"
        if "0.5" in expr:
            assert name == sweep + tail, name
        else:
            assert name.startswith("lap_march_kernel<double,2,") and "mode=10" in name and name.endswith(tail), name
        REPORT["fixed-point"].add(name)


@pytest.mark.parametrize("mode", ["two", "fused2"])
@pytest.mark.parametrize("dtype,shape,ry", J.TWO_LEVEL, ids=[f"{d}-{'x'.join(map(str, s))}" for d, s, _ in J.TWO_LEVEL])
def test_two_level_kernels(runner, mode, dtype, shape, ry):
    """``pdehip_jit_euler2`` / ``pdehip_jit_fused2`` on one shape per (type, rows per tile, 2-D / 3-D) the two-step planner answers for them: the
    recorded name, the bits of two passes of the reference, input and output as whole allocations."""
    with np.errstate(all="ignore"):
        name, diffs = runner.run_two_level(mode, dtype, shape, ry)
    print(f"{mode}-{dtype}-{shape}: {name}")
    assert not diffs, "\n".join(diffs)
    REPORT["two-level"].add(name)


def test_tuning_knobs_give_the_same_bits():
    """"any value works".  Four rows per tile, two waves per workgroup in the stage sweeps, 64 wave tiles per sweep: other
    instances, other seams, the same bits (tests/jit_knob_worker.py in a process of its own)."""
    env = dict(os.environ)
    env.pop("PDEHIP_JIT_CZ", None)
    env.update(PDEHIP_JIT_RY="4", PDEHIP_JIT_WY="2", PDEHIP_JIT_BLOCKS="64")
    worker = Path(__file__).resolve().parent / "jit_knob_worker.py"
    proc = subprocess.run([sys.executable, str(worker)], capture_output=True, text=True, timeout=300, env=env)
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("JITKNOBS ")]
    assert proc.returncode == 0 and lines, (proc.stdout[-2000:], proc.stderr[-2000:])
    report = json.loads(lines[-1][len("JITKNOBS "):])
    assert report["knobs"] == J.WORKER_KNOBS
    cases = {c.id: c for c in J.worker_cases()}
    assert set(report["cases"]) == set(cases) and len(cases) >= 8
    bad = []
    for cid, r in report["cases"].items():
        p = J.case_plan(cases[cid], J.WORKER_KNOBS)
        assert p.ry == 4 and p.wy == (2 if p.stage else 1)
        if r["name"] != J.kernel_name(p):
            bad.append(f"{cid}: name {r['name']!r}, expected {J.kernel_name(p)!r}")
        bad += [f"{cid}: {d}" for d in r["differences"]]
        REPORT["knobs"].add(r["name"])
    assert not bad, "\n".join(bad)
