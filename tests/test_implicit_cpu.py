"""CPU checks of the implicit Euler / Crank-Nicolson feature: the numpy restatement (tests/implicit_cases.py) reproduces the reference's
golden runs; a library without the new entry points (the host shim) refuses the two solvers as before; the ABI table lists them."""

from __future__ import annotations

import numpy as np
import pytest

import pde_hip
import refpath
import shimlib
from helpers import GOLDEN, get_case, load_cases
from implicit_cases import NotConverged, fixedpoint_run, oracle_rhs
from pde_hip import _abi

NPZ = np.load(GOLDEN / "implicit.npz", allow_pickle=False)
NEW = ["fixedpoint_ctl_bytes", "fixedpoint_run", "jit_fixedpoint_run"]


def build(case):
    grid = pde_hip.CartesianGrid(case["bounds"], case["shape"], periodic=case["periodic"])
    if case["eq"] == "diffusion":
        eq = pde_hip.DiffusionPDE(case["param"], **({} if case["bc"] is None else {"bc": case["bc"]}))
    else:
        eq = pde_hip.CahnHilliardPDE(interface_width=case["param"])
    return grid, eq


@pytest.mark.parametrize("cid", [c["id"] for c in load_cases(NPZ)])
def test_restatement_reproduces_the_reference(cid):
    case = get_case(NPZ, cid)
    grid, eq = build(case)
    dtype = np.dtype(case["dtype"])
    init = NPZ[f"{cid}/input"]
    rhs = oracle_rhs(grid, eq, dtype)
    if not case.get("converges", True):
        with pytest.raises(NotConverged) as err:
            fixedpoint_run(rhs, init, case["dt"], case["steps"], scheme=case["solver"], **case["kw"])
        assert str(err.value) == str(NPZ[f"{cid}/message"])
        return
    got, evals, counts = fixedpoint_run(rhs, init, case["dt"], case["steps"], scheme=case["solver"], **case["kw"])
    assert evals == int(NPZ[f"{cid}/evaluations"])
    assert counts == list(NPZ[f"{cid}/iterations"])
    want = NPZ[f"{cid}/final"]
    assert got.dtype == want.dtype
    np.testing.assert_allclose(got, want, rtol=1e-5 if dtype == np.float32 else 1e-12, atol=1e-6 if dtype == np.float32 else 1e-14)


def test_abi_table_lists_the_new_entry_points():
    assert _abi.ABI_VERSION == 8
    for name in NEW:
        assert "pdehip_" + name in _abi.exported_symbols()
        assert name in _abi.OPTIONAL_PROTOTYPES
        assert name not in _abi.COMPUTE_PROTOTYPES and name not in _abi.COMM_PROTOTYPES and name not in _abi.RUNTIME_PROTOTYPES


def test_product_library_exports_them():
    from pde_hip import _lib

    assert _lib.get_lib().missing == set()


@pytest.mark.parametrize("solver", ["implicit", "crank-nicolson"])
def test_host_shim_still_refuses_the_solvers(solver):
    """Mirror classes on the tests-only host library, which lacks the new entry points: refused as before the feature."""
    with shimlib.use_shim() as lib:
        if not refpath.REAL:
            assert set(NEW) <= lib.missing and not lib.has("fixedpoint_run")
        grid = pde_hip.UnitGrid([8, 8], periodic=True)
        state = pde_hip.ScalarField(grid, np.random.default_rng(0).uniform(size=grid.shape))
        if refpath.REAL:
            pytest.skip("the real library has the entry points")
        with pytest.raises(NotImplementedError, match="does not support solver"):
            pde_hip.DiffusionPDE().solve(state, t_range=0.1, dt=0.05, solver=solver, backend="hip", tracker=None)


@pytest.mark.parametrize("solver", ["implicit", "crank-nicolson"])
def test_host_shim_refuses_them_under_the_real_pypde(solver):
    pde = refpath.import_reference()
    if pde is None or refpath.REAL:
        pytest.skip("needs the reference py-pde and the host shim")
    with shimlib.use_shim():
        import pde_hip.pypde_plugin  # noqa: F401

        grid = pde.UnitGrid([8, 8], periodic=True)
        state = pde.ScalarField(grid, np.random.default_rng(0).uniform(size=grid.shape))
        with pytest.raises(NotImplementedError, match="does not support solver"):
            pde.DiffusionPDE().solve(state, t_range=0.1, dt=0.05, solver=solver, backend="hip", tracker=None)


def test_solver_classes_and_registration():
    assert pde_hip.ImplicitSolver.name == "implicit" and pde_hip.CrankNicolsonSolver.name == "crank-nicolson"
    assert issubclass(pde_hip.ConvergenceError, RuntimeError)
    from pde_hip.steppers import _fixedpoint_scheme

    class ImplicitSolver:      # an unrelated class of that name is not the reference's solver
        name = "implicit-test"
        maxiter, maxerror = 1, 1.0

    assert _fixedpoint_scheme(ImplicitSolver()) is None
