"""GPU tests of the implicit Euler and Crank-Nicolson solvers (``solver="implicit"`` / ``"crank-nicolson"``): bit-equality with the
numpy restatement of the reference's loops (tests/implicit_cases.py), iteration counts, determinism, batching, non-convergence,
hooks, the kernel instance that ran."""

from __future__ import annotations

import numpy as np
import pytest

import pde_hip
from implicit_cases import NotConverged, fixedpoint_run, oracle_rhs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    return pde_hip.get_backend("hip")


def smooth(grid, dtype=np.float64, seed=0):
    rng = np.random.default_rng(seed)
    data = rng.uniform(-1, 1, grid.shape)
    return pde_hip.ScalarField(grid, data.astype(dtype), dtype=dtype)


def solve(eq, state, dt, steps, solver, backend, **kw):
    sol = pde_hip.solvers.SolverBase.from_name(solver, pde=eq, backend=backend, **kw)
    ctl = pde_hip.Controller(sol, t_range=dt * steps, tracker=None)
    res = ctl.run(state, dt)
    return res, sol


CLASS_CASES = {
    # id: (shape, periodic, bounds, pde, bc, dtype, dt, steps, solver, kwargs)
    "diff-3d-per-implicit": ((16, 12, 40), True, None, "diffusion", None, "f8", 0.05, 3, "implicit", {}),
    "diff-3d-walls-cn": ((10, 14, 36), [True, False, False], None, "diffusion", [None, {"value": 1.0}, {"derivative": 0.5}], "f8", 0.05, 3, "crank-nicolson", {}),
    "diff-3d-cn-alpha": ((10, 14, 36), True, None, "diffusion", None, "f8", 0.05, 3, "crank-nicolson", {"explicit_fraction": 0.3}),
    "diff-2d-dx": ((24, 50), [False, True], [(0, 6.0), (0, 25.0)], "diffusion", [{"value": 0.2}, None], "f8", 0.01, 4, "implicit", {}),
    "diff-2d-f32": ((32, 64), True, None, "diffusion", None, "f4", 0.05, 3, "crank-nicolson", {"maxerror": 1e-3}),
    "diff-1d": ((65,), False, None, "diffusion", {"value": 0.0}, "f8", 0.05, 3, "implicit", {}),
    "diff-3d-odd": ((7, 9, 33), True, None, "diffusion", None, "f8", 0.05, 2, "implicit", {}),
    "ch-3d-implicit": ((12, 12, 32), True, None, "ch", None, "f8", 0.005, 3, "implicit", {}),
    "ch-2d-cn": ((24, 40), [True, False], None, "ch", None, "f8", 0.005, 3, "crank-nicolson", {"explicit_fraction": 0.3}),
}


def make_case(cid):
    shape, periodic, bounds, kind, bc, dtype, dt, steps, solver, kw = CLASS_CASES[cid]
    grid = pde_hip.UnitGrid(list(shape), periodic=periodic) if bounds is None else pde_hip.CartesianGrid(bounds, list(shape), periodic=periodic)
    if bc is not None and isinstance(bc, list):
        bc = ["periodic" if b is None else b for b in bc]
    if kind == "diffusion":
        eq = pde_hip.DiffusionPDE(0.7, **({} if bc is None else {"bc": bc}))
    else:
        eq = pde_hip.CahnHilliardPDE(interface_width=1.1)
    return grid, eq, np.dtype(dtype), dt, steps, solver, kw


@pytest.mark.parametrize("cid", sorted(CLASS_CASES))
def test_class_pde_bit_equal_to_the_restatement(cid, backend):
    grid, eq, dtype, dt, steps, solver, kw = make_case(cid)
    state = smooth(grid, dtype)
    res, sol = solve(eq, state.copy(), dt, steps, solver, backend, **kw)
    want, evals, counts = fixedpoint_run(oracle_rhs(grid, eq, dtype), state.data, dt, steps, scheme=solver, **kw)
    assert sol.info["iterations"] == counts
    assert sol.info["function_evaluations"] == evals
    assert sol.info["steps"] == steps
    assert res.data.dtype == dtype
    assert np.array_equal(res.data, want), f"max abs {np.abs(res.data - want).max():.3e}"


@pytest.mark.parametrize("solver", ["implicit", "crank-nicolson"])
def test_kernel_name_names_the_fixed_point_instance(solver, backend):
    from pde_hip import _lib

    grid = pde_hip.UnitGrid([16, 16, 128], periodic=True)
    solve(pde_hip.DiffusionPDE(0.5), smooth(grid), 0.05, 2, solver, backend)
    name = _lib.get_lib().last_kernel_name().decode()
    assert "lap_march_kernel" in name and "fixed-point epilogue" in name, name


def test_iteration_counts_change_and_repeat(backend):
    """A decaying initial condition with a tight tolerance: the iteration count falls from step to step - the same counts as the
    restatement and the same counts twice in a row."""
    grid = pde_hip.UnitGrid([8, 16, 64], periodic=True)
    x = np.indices(grid.shape)
    data = np.sin(2 * np.pi * x[2] / 64) + 0.5 * np.sin(2 * np.pi * x[1] / 16 * 3) * np.cos(2 * np.pi * x[0] / 8 * 2)
    state = pde_hip.ScalarField(grid, data)
    eq = pde_hip.DiffusionPDE(1.0)
    kw = {"maxerror": 1e-9, "maxiter": 200}
    runs = [solve(eq, state.copy(), 0.07, 12, "implicit", backend, **kw) for _ in range(2)]
    want, evals, counts = fixedpoint_run(oracle_rhs(grid, eq), state.data, 0.07, 12, **kw)
    assert len(set(counts)) > 1, counts
    for res, sol in runs:
        assert sol.info["iterations"] == counts
        assert np.array_equal(res.data, want)


@pytest.mark.parametrize("solver", ["implicit", "crank-nicolson"])
def test_batch_size_does_not_change_results(solver, backend, monkeypatch):
    grid = pde_hip.UnitGrid([12, 10, 48], periodic=[True, False, True])
    eq = pde_hip.DiffusionPDE(0.9)
    state = smooth(grid, seed=3)
    out = []
    for batch in ("0", "1", "100"):
        monkeypatch.setenv("PDEHIP_FIXEDPOINT_BATCH", batch)
        res, sol = solve(eq, state.copy(), 0.05, 5, solver, backend)
        out.append((res.data.copy(), list(sol.info["iterations"]), sol.info["function_evaluations"]))
    for data, counts, evals in out[1:]:
        assert np.array_equal(data, out[0][0]) and counts == out[0][1] and evals == out[0][2]


def test_pointwise_form_names_itself(backend):
    """Class Cahn-Hilliard: two-level slope sweep + the pointwise kernel for update and norm - the same bits as the restatement, and
    `pdehip_last_kernel_name` says which form ran."""
    from pde_hip import _lib

    grid = pde_hip.UnitGrid([16, 16, 64], periodic=True)
    eq = pde_hip.CahnHilliardPDE()
    state = smooth(grid, seed=5)
    state.data *= 0.3
    res, sol = solve(eq, state.copy(), 0.002, 3, "crank-nicolson", backend)
    name = _lib.get_lib().last_kernel_name().decode()
    want, evals, counts = fixedpoint_run(oracle_rhs(grid, eq), state.data, 0.002, 3, scheme="crank-nicolson")
    assert np.array_equal(res.data, want) and sol.info["iterations"] == counts
    assert "fixedpoint_combine_kernel" in name, name


def test_non_convergence_raises_and_the_backend_survives(backend):
    grid = pde_hip.UnitGrid([8, 8, 32], periodic=True)
    eq = pde_hip.DiffusionPDE(1.0)
    state = smooth(grid)
    with pytest.raises(pde_hip.ConvergenceError, match="Implicit Euler step did not converge."):
        solve(eq, state.copy(), 1.0, 3, "implicit", backend, maxiter=5)       # dt far beyond the fixed-point limit
    with pytest.raises(pde_hip.ConvergenceError, match="Crank-Nicolson step did not converge."):
        solve(eq, state.copy(), 2.0, 3, "crank-nicolson", backend, maxiter=5)
    with pytest.raises(NotConverged):
        fixedpoint_run(oracle_rhs(grid, eq), state.data, 1.0, 3, maxiter=5)
    res, sol = solve(eq, state.copy(), 0.05, 2, "implicit", backend)
    want, _, counts = fixedpoint_run(oracle_rhs(grid, eq), state.data, 0.05, 2)
    assert np.array_equal(res.data, want) and sol.info["iterations"] == counts


def test_host_hook_runs_after_every_step(backend):
    grid = pde_hip.UnitGrid([8, 8, 32], periodic=True)
    calls = []

    class Clipped(pde_hip.DiffusionPDE):
        def make_post_step_hook(self, state, backend="numpy"):
            def hook(data, t, post_step_data):
                calls.append(t)
                np.clip(data, -0.5, 0.5, out=data)
                return data, post_step_data

            return hook, None

    state = smooth(grid)
    res, sol = solve(Clipped(0.8), state.copy(), 0.05, 4, "crank-nicolson", backend)
    want, evals, counts = fixedpoint_run(oracle_rhs(grid, pde_hip.DiffusionPDE(0.8)), state.data, 0.05, 4, scheme="crank-nicolson",
                                         hook=lambda s, t: np.clip(s, -0.5, 0.5))
    assert len(calls) == 4 and np.allclose(calls, [0, 0.05, 0.1, 0.15])
    assert np.array_equal(res.data, want) and sol.info["iterations"] == counts and sol.info["function_evaluations"] == evals


@pytest.mark.parametrize("shape,dtype,kind,steps", [
    ((256, 256, 256), "f8", "diffusion", 5),
    ((256, 256, 256), "f4", "diffusion", 3),
    ((160, 130, 200), "f8", "walls", 3),
    ((1024, 1024), "f8", "diffusion", 3),
    ((128, 128, 128), "f8", "ch", 2),
])
def test_production_sizes_bit_equal(shape, dtype, kind, steps, backend):
    dtype = np.dtype(dtype)
    if kind == "walls":
        grid = pde_hip.UnitGrid(list(shape), periodic=[False, True, False])
        eq = pde_hip.DiffusionPDE(0.6, bc=[{"value": 0.3}, "periodic", {"derivative": -0.2}])
    else:
        grid = pde_hip.UnitGrid(list(shape), periodic=True)
        eq = pde_hip.DiffusionPDE(0.6) if kind == "diffusion" else pde_hip.CahnHilliardPDE()
    state = smooth(grid, dtype, seed=11)
    dt = 0.05 if kind != "ch" else 0.002
    kw = {"maxerror": 1e-3} if dtype == np.float32 else {}
    for solver in ("implicit", "crank-nicolson"):
        res, sol = solve(eq, state.copy(), dt, steps, solver, backend, **kw)
        want, evals, counts = fixedpoint_run(oracle_rhs(grid, eq, dtype), state.data, dt, steps, scheme=solver, **kw)
        assert sol.info["iterations"] == counts and sol.info["function_evaluations"] == evals
        assert np.array_equal(res.data, want), f"{solver}: max abs {np.abs(res.data.astype(float) - want).max():.3e}"


# ---- expression PDEs: the run-time compiled passes (pdehip_jit_fixedpoint_run) ------------------------------------------------------
def test_expression_diffusion_takes_the_epilogue_in_its_pass(backend):
    from pde_hip import _lib

    grid = pde_hip.UnitGrid([12, 10, 64], periodic=[True, False, True])
    eq = pde_hip.PDE({"c": "0.7 * laplace(c)"}, bc=["periodic", {"value": 0.4}, "periodic"])
    twin = pde_hip.DiffusionPDE(0.7, bc=["periodic", {"value": 0.4}, "periodic"])
    state = smooth(grid, seed=2)
    for solver, kw in (("implicit", {}), ("crank-nicolson", {"explicit_fraction": 0.3})):
        res, sol = solve(eq, state.copy(), 0.05, 3, solver, backend, **kw)
        name = _lib.get_lib().last_kernel_name().decode()
        want, evals, counts = fixedpoint_run(oracle_rhs(grid, twin), state.data, 0.05, 3, scheme=solver, **kw)
        assert sol.info["iterations"] == counts and sol.info["function_evaluations"] == evals
        assert np.array_equal(res.data, want)
        assert "fixed-point epilogue" in name, name
        # the host recognises ``D * laplace(c)`` as the diffusion equation: the iterations ran on the built-in stage sweep
        assert name.startswith("lap_march_kernel<double,2,") and "mode=10" in name, name
        # with a decay term the expression compiler takes it: the run-time built stage instance of this grid (one row per tile, the wall
        # applied on the fly), the same epilogue in its pass, the same bits as the restatement
        decay = pde_hip.PDE({"c": "0.7 * laplace(c) - 0.5 * c"}, bc=["periodic", {"value": 0.4}, "periodic"])
        res, sol = solve(decay, state.copy(), 0.05, 3, solver, backend, **kw)
        name = _lib.get_lib().last_kernel_name().decode()
        diffusion = oracle_rhs(grid, twin)
        want, evals, counts = fixedpoint_run(lambda valid, t: diffusion(valid, t) - 0.5 * valid, state.data, 0.05, 3, scheme=solver, **kw)
        assert sol.info["iterations"] == counts and sol.info["function_evaluations"] == evals
        assert np.array_equal(res.data, want)
        assert name.startswith("pde_kernel<double,2,RY=1,CZ=1,WY=1,3-D,ibc,stage,-> (lx=1, 12 x-chunks; run-time built) + fixed-point epilogue"), name


@pytest.mark.parametrize("shape", [(12, 12, 32), (128, 128, 128), (40, 64), (96,)])
def test_two_pass_expression_equals_the_class_pde(shape, backend):
    """``laplace(c**3 - c - laplace(c))`` (two passes: the last one carries update and norm) against the Cahn-Hilliard restatement."""
    grid = pde_hip.UnitGrid(list(shape), periodic=True)
    eq = pde_hip.PDE({"c": "laplace(c**3 - c - laplace(c))"})
    state = smooth(grid, seed=4)
    state.data *= 0.3
    res, sol = solve(eq, state.copy(), 0.002, 2, "crank-nicolson", backend)
    want, evals, counts = fixedpoint_run(oracle_rhs(grid, pde_hip.CahnHilliardPDE(interface_width=1.0)), state.data, 0.002, 2, scheme="crank-nicolson")
    assert sol.info["iterations"] == counts and sol.info["function_evaluations"] == evals
    assert np.array_equal(res.data, want), f"max abs {np.abs(res.data - want).max():.3e}"


def test_time_dependent_face_sees_the_right_times(backend):
    """A face that is an expression of time: the first estimate of implicit Euler sees it at t, every iteration at t + dt."""
    from helpers import host_faces, oracle_grid, to_full
    from oracle import pde_oracle as O
    from pde_hip import _abi

    grid = pde_hip.UnitGrid([16, 64], periodic=[False, True])
    eq = pde_hip.DiffusionPDE(0.7, bc=[{"value_expression": "1 + 2 * t"}, "periodic"])
    state = smooth(grid, seed=6)
    g = oracle_grid(grid)

    def rhs(valid, t):
        faces = host_faces(grid.get_boundary_conditions([{"value": 1 + 2 * t}, "periodic"]))
        spec = O.make_rhs(_abi.RHS_DIFFUSION, 0.7, faces.c)
        return np.ascontiguousarray(O.rhs_scaled(g, spec, to_full(grid, np.ascontiguousarray(valid)), 1.0)[1:-1, 1:-1])

    for solver in ("implicit", "crank-nicolson"):
        res, sol = solve(eq, state.copy(), 0.05, 3, solver, backend)
        want, evals, counts = fixedpoint_run(rhs, state.data, 0.05, 3, scheme=solver)
        assert sol.info["iterations"] == counts and sol.info["function_evaluations"] == evals
        np.testing.assert_allclose(res.data, want, rtol=1e-13, atol=1e-15)


def test_complex_field_and_two_field_system(backend):
    from helpers import oracle_grid
    from oracle import pde_oracle as O

    grid = pde_hip.UnitGrid([16, 32], periodic=True)
    g = oracle_grid(grid)

    def lap(a):
        return O.laplace(g, np.ascontiguousarray(np.pad(a, 1, mode="wrap"), dtype=np.float64))   # periodic ghost cells

    rng = np.random.default_rng(8)
    data = rng.uniform(-1, 1, grid.shape) + 1j * rng.uniform(-1, 1, grid.shape)
    state = pde_hip.ScalarField(grid, data, dtype=complex)
    eq = pde_hip.PDE({"c": "-I * laplace(c)"})
    res, sol = solve(eq, state.copy(), 0.02, 3, "crank-nicolson", backend)
    want, evals, counts = fixedpoint_run(lambda c, t: -1j * (lap(c.real) + 1j * lap(c.imag)), data, 0.02, 3, scheme="crank-nicolson")
    assert sol.info["iterations"] == counts and sol.info["function_evaluations"] == evals
    np.testing.assert_allclose(res.data, want, rtol=1e-13, atol=1e-15)

    u = pde_hip.ScalarField(grid, rng.uniform(0, 1, grid.shape))
    v = pde_hip.ScalarField(grid, rng.uniform(0, 1, grid.shape))
    both = pde_hip.FieldCollection([u, v])
    eq2 = pde_hip.PDE({"u": "0.5 * laplace(u) + v - u", "v": "0.2 * laplace(v) - v"})
    res2, sol2 = solve(eq2, both.copy(), 0.05, 3, "implicit", backend)

    def rhs2(s, t):
        return np.stack([0.5 * lap(s[0]) + s[1] - s[0], 0.2 * lap(s[1]) - s[1]])

    want2, evals2, counts2 = fixedpoint_run(rhs2, both.data, 0.05, 3)
    assert sol2.info["iterations"] == counts2 and sol2.info["function_evaluations"] == evals2
    np.testing.assert_allclose(res2.data, want2, rtol=1e-13, atol=1e-15)


def test_traced_hook_runs_on_the_device_after_every_step(backend):
    grid = pde_hip.UnitGrid([8, 8, 32], periodic=True)

    def hook(state_data, t):
        return np.clip(state_data, -0.4, 0.4)

    eq = pde_hip.PDE({"c": "0.8 * laplace(c)"}, post_step_hook=hook)
    state = smooth(grid, seed=9)
    res, sol = solve(eq, state.copy(), 0.05, 3, "implicit", backend)
    assert getattr(backend.make_inner_stepper.__self__._make_host_post_step(sol, state), "on_device", False), "the hook was not traced"
    want, evals, counts = fixedpoint_run(oracle_rhs(grid, pde_hip.DiffusionPDE(0.8)), state.data, 0.05, 3, hook=lambda s, t: np.clip(s, -0.4, 0.4))
    assert sol.info["iterations"] == counts and sol.info["function_evaluations"] == evals
    assert np.array_equal(res.data, want)


def test_refusals_name_their_reason(backend):
    grid = pde_hip.UnitGrid([8, 16], periodic=[False, True])
    state = smooth(grid)
    with pytest.raises(NotImplementedError, match="stochastic"):
        solve(pde_hip.DiffusionPDE(1.0, noise=0.1), state.copy(), 0.01, 2, "implicit", backend)
    eq = pde_hip.DiffusionPDE(1.0, bc=[{"value_expression": "1 + t"}, "periodic"])
    solve(eq, state.copy(), 0.01, 2, "crank-nicolson", backend)     # expressions of time are supported


# ---- the reference's golden runs -----------------------------------------------------------------------------------------------------
def _golden():
    from helpers import GOLDEN, load_cases

    npz = np.load(GOLDEN / "implicit.npz", allow_pickle=False)
    return npz, load_cases(npz)


@pytest.mark.parametrize("cid", [c["id"] for c in _golden()[1]])
def test_golden_runs_of_the_reference(cid, backend):
    from helpers import get_case

    npz, _ = _golden()
    case = get_case(npz, cid)
    grid = pde_hip.CartesianGrid(case["bounds"], case["shape"], periodic=case["periodic"])
    if case["eq"] == "diffusion":
        eq = pde_hip.DiffusionPDE(case["param"], **({} if case["bc"] is None else {"bc": case["bc"]}))
    else:
        eq = pde_hip.CahnHilliardPDE(interface_width=case["param"])
    dtype = np.dtype(case["dtype"])
    init = npz[f"{cid}/input"]
    state = pde_hip.ScalarField(grid, init.copy(), dtype=dtype)
    if not case.get("converges", True):
        with pytest.raises(pde_hip.ConvergenceError) as err:
            solve(eq, state, case["dt"], case["steps"], case["solver"], backend, **case["kw"])
        assert str(err.value) == str(npz[f"{cid}/message"])
        return
    res, sol = solve(eq, state, case["dt"], case["steps"], case["solver"], backend, **case["kw"])
    want, evals, counts = fixedpoint_run(oracle_rhs(grid, eq, dtype), init, case["dt"], case["steps"], scheme=case["solver"], **case["kw"])
    assert np.array_equal(res.data, want)
    assert sol.info["function_evaluations"] == int(npz[f"{cid}/evaluations"]) == evals
    assert sol.info["iterations"] == list(npz[f"{cid}/iterations"])
    np.testing.assert_allclose(res.data, npz[f"{cid}/final"], rtol=1e-5 if dtype == np.float32 else 1e-12, atol=1e-6 if dtype == np.float32 else 1e-14)
