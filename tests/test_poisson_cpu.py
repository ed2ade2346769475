"""CPU checks of the Poisson solver: a dense numpy restatement (tests/poisson_cases.py) reproduces the reference's golden solutions;
the decisions taken on the host - singular systems, refused conditions, the `method` argument, the operator without conditions - are
tested on the face tables without a device; a library without the entry points (the host shim) refuses the operator and names them.
The restated loop (`cg`) reproduces the dense solutions, ends in breakdown on an indefinite system, and keeps the tolerances of the
device tests (tests/test_hip_poisson_trajectory.py) with its own two summation modes."""

from __future__ import annotations

import numpy as np
import pytest

import pde_hip
import refpath
import shimlib
from helpers import GOLDEN, get_case, host_faces, load_cases
from pde_hip import _abi, poisson
from poisson_cases import BREAKDOWN, CONVERGED, INDEFINITE, NotSolved, cg, dense_solve, laplace_with_bcs, make_grid

NPZ = np.load(GOLDEN / "poisson.npz", allow_pickle=False)
NEW = ["poisson_create", "poisson_solve", "poisson_destroy"]
DENSE = [c["id"] for c in load_cases(NPZ) if int(np.prod(c["shape"])) <= 2000]
ALL = [c["id"] for c in load_cases(NPZ)]


@pytest.mark.parametrize("cid", DENSE)
def test_restatement_reproduces_the_reference(cid):
    case = get_case(NPZ, cid)
    grid = make_grid(case)
    rhs = NPZ[f"{cid}/rhs"]
    if case.get("raises"):
        with pytest.raises(NotSolved, match="could not be solved"):
            dense_solve(grid, case["bc"], rhs)
        assert "only periodic or Neumann conditions" in str(NPZ[f"{cid}/message"])
        return
    want = NPZ[f"{cid}/solution"]
    got = dense_solve(grid, case["bc"], rhs)
    if poisson.is_singular(host_faces(grid.get_boundary_conditions(case["bc"])).c, grid.num_axes):
        # solutions of a singular system differ by constants, and which one the reference returns depends on whether its direct solver
        # noticed the rank (then lsmr: mean zero) or not (then any member of the family): compared up to the constant
        assert abs(got.mean()) < 1e-9
        want = want - want.mean()
    assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("cid", [c for c in ALL if c not in DENSE])
def test_golden_solutions_satisfy_the_split_system(cid):
    """The larger cases: L(u) = A u + v applied to the recorded solution gives the right-hand side back."""
    case = get_case(NPZ, cid)
    grid = make_grid(case)
    rhs, want = NPZ[f"{cid}/rhs"], NPZ[f"{cid}/solution"]
    assert np.abs(laplace_with_bcs(grid, case["bc"], want) - rhs).max() <= 1e-9 * max(1.0, np.abs(want).max())
    faces = host_faces(grid.get_boundary_conditions(case["bc"]))
    assert poisson.is_singular(faces.c, grid.num_axes) == (cid == "3d-neumann-zero-mean")


def test_singular_systems_are_recognised_on_the_face_table():
    flags = {}
    for case in load_cases(NPZ):
        grid = make_grid(case)
        faces = host_faces(grid.get_boundary_conditions(case["bc"]))
        poisson.check_faces(faces.c, grid.shape)
        flags[case["id"]] = poisson.is_singular(faces.c, grid.num_axes)
    assert {k for k, v in flags.items() if v} == {"2d-periodic-zero-mean", "3d-neumann-zero-mean", "2d-periodic-nonzero-mean"}
    # coefficient arrays: singular only when every factor is one
    grid = pde_hip.UnitGrid([6, 5])
    bcs = grid.get_boundary_conditions([{"derivative": "sin(y)"} if False else {"derivative": np.linspace(0, 1, 5)}, {"derivative": 0.0}])
    faces = host_faces(bcs)
    arrays = {q: np.ones(5) for q in range(4) if faces.c[q].flags & _abi.BCF_ARRAYS}
    assert arrays and poisson.is_singular(faces.c, 2, arrays)
    assert not poisson.is_singular(faces.c, 2)                               # unknown arrays: not assumed
    assert not poisson.is_singular(faces.c, 2, {q: np.full(5, 0.5) for q in arrays})


def test_refused_conditions_name_the_face():
    grid = pde_hip.UnitGrid([8, 8])
    faces = host_faces(grid.get_boundary_conditions([{"curvature": 0.3}, {"value": 0.0}]))
    with pytest.raises(NotImplementedError, match=r"lower face of axis 0 is a second-order condition"):
        poisson.check_faces(faces.c, grid.shape)
    faces = host_faces(grid.get_boundary_conditions([{"value": 0.0}, [{"value": 0.0}, {"curvature": 1.0}]]))
    with pytest.raises(NotImplementedError, match=r"upper face of axis 1 is a second-order condition"):
        poisson.check_faces(faces.c, grid.shape)
    table = host_faces(grid.get_boundary_conditions({"value": 0.0}))
    table.c[0].index1 = 3
    with pytest.raises(NotImplementedError, match="neither adjacent nor periodic"):
        poisson.check_faces(table.c, grid.shape)
    table = host_faces(grid.get_boundary_conditions({"value": 0.0}))
    table.c[0].index1 = 7                                                    # a one-sided link to the other end
    with pytest.raises(NotImplementedError, match="without being periodic"):
        poisson.check_faces(table.c, grid.shape)
    with pytest.raises(NotImplementedError, match="complex factor"):
        poisson.check_conditions(grid.get_boundary_conditions({"type": "mixed", "value": 1 + 2j, "const": 0.0}))


def test_method_and_defaults():
    poisson.check_method("auto")
    poisson.check_method("cg")
    with pytest.raises(ValueError, match="Method scipy is not available"):
        poisson.check_method("scipy")
    assert poisson.default_maxiter([16, 8]) == 1000 and poisson.default_maxiter([512, 512, 512]) == 25600
    assert poisson.DEFAULT_RTOL == 1e-10 and poisson.DEFAULT_BATCH == 32


def test_status_becomes_the_references_exceptions():
    info = {"iterations": 3, "residual": 0.5, "rhs_norm": 2.0, "check_residual": 0.25, "status": _abi.POISSON_CONVERGED}
    poisson.raise_for_status(info, 3)
    with pytest.raises(pde_hip.ConvergenceError, match="within 3 iterations"):
        poisson.raise_for_status(dict(info, status=_abi.POISSON_MAXITER), 3)
    with pytest.raises(RuntimeError, match=r"Poisson problem could not be solved \(Residual: 0.25\)"):
        poisson.raise_for_status(dict(info, status=_abi.POISSON_INCONSISTENT), 3)
    with pytest.raises(RuntimeError, match="not negative definite"):
        poisson.raise_for_status(dict(info, status=_abi.POISSON_BREAKDOWN), 3)


def test_abi_table_lists_the_entry_points():
    for name in NEW:
        assert "pdehip_" + name in _abi.exported_symbols()
        assert name in _abi.OPTIONAL_PROTOTYPES
        assert name not in _abi.COMPUTE_PROTOTYPES and name not in _abi.COMM_PROTOTYPES and name not in _abi.RUNTIME_PROTOTYPES
    import ctypes as C

    assert C.sizeof(_abi.Poisson) == 2 * 8 + 4 * 4 + 3 * 8 + 2 * 4
    from pde_hip import _lib

    assert not (set(NEW) & _lib.get_lib().missing)


def test_operator_is_registered_and_needs_conditions():
    grid = pde_hip.UnitGrid([8, 8])
    backend = pde_hip.get_backend("hip")
    info = backend.get_operator_info(grid, "poisson_solver")
    assert (info.rank_in, info.rank_out) == (0, 0) and "poisson_solver" in backend.get_registered_operators(grid)
    with pytest.raises(ValueError, match="built from the boundary conditions"):
        info.factory(grid, backend=backend)
    with pytest.raises(ValueError, match="Method scipy is not available"):       # (before anything touches a device)
        info.factory(grid, backend=backend, bcs=grid.get_boundary_conditions({"value": 0}), method="scipy")


def test_host_shim_refuses_the_operator_and_names_the_entry_points():
    if refpath.REAL:
        pytest.skip("the real library has the entry points")
    with shimlib.use_shim() as lib:
        assert set(NEW) <= lib.missing and not lib.has("poisson_solve")
        grid = pde_hip.UnitGrid([8, 8])
        with pytest.raises(NotImplementedError, match="pdehip_poisson_create, pdehip_poisson_destroy, pdehip_poisson_solve"):
            grid.make_operator("poisson_solver", {"value": 0.0}, backend="hip")
        with pytest.raises(NotImplementedError, match="pdehip_poisson_solve"):
            pde_hip.solve_poisson_equation(pde_hip.ScalarField(grid, 1.0), {"value": 0.0})
        with pytest.raises(ValueError, match="built from the boundary conditions"):
            grid.make_operator_no_bc("poisson_solver", backend="hip")
        with pytest.raises(NotImplementedError):                                  # inside expressions it stays refused
            pde_hip.PDE({"c": "poisson_solver(c)"}).evolution_rate(pde_hip.ScalarField(grid, 1.0))


# ---- the restated loop behind the device tests that compare iteration by iteration ------------------------------------------------
def indefinite_case():
    grid = pde_hip.UnitGrid(INDEFINITE["shape"])
    return grid, INDEFINITE["bc"], np.random.default_rng(INDEFINITE["seed"]).uniform(-1, 1, grid.shape)


@pytest.mark.parametrize("cid", [c for c in DENSE if not get_case(NPZ, c).get("raises")])
def test_restated_cg_reproduces_the_dense_solutions(cid):
    case = get_case(NPZ, cid)
    grid = make_grid(case)
    singular = poisson.is_singular(host_faces(grid.get_boundary_conditions(case["bc"])).c, grid.num_axes)
    want = dense_solve(grid, case["bc"], NPZ[f"{cid}/rhs"])
    for sums in ("exact", "numpy"):
        traj = cg(grid, case["bc"], NPZ[f"{cid}/rhs"], rtol=1e-12, maxiter=poisson.default_maxiter(grid.shape), singular=singular, sums=sums, keep=())
        assert traj.status == CONVERGED and 0 < traj.iterations == len(traj.scalars)
        assert np.abs(traj.x - want).max() <= 1e-8 * max(1.0, np.abs(want).max())
        assert np.abs(traj.x - NPZ[f"{cid}/solution"] + (NPZ[f"{cid}/solution"].mean() if singular else 0.0)).max() <= 1e-8 * max(1.0, np.abs(want).max())


def test_restated_cg_breaks_down_on_an_indefinite_system():
    from poisson_cases import matrix_and_vector

    grid, bc, f = indefinite_case()
    assert host_faces(grid.get_boundary_conditions(bc)).c[0].factor1 > 2
    assert np.linalg.eigvalsh(-matrix_and_vector(grid, bc)[0]).min() < 0
    for sums in ("exact", "numpy"):
        traj = cg(grid, bc, f, rtol=1e-10, maxiter=100, sums=sums)
        assert traj.status == BREAKDOWN and traj.iterations == 1 and len(traj.iterates) == 1


def test_trajectory_tolerances_hold_for_the_restatement_itself():
    import poisson_trajectory_cases as T

    assert set(T.TOL) == {c["id"] for c in T.CASES}
    T.check_tolerances("cg")      # (the preconditioned cases: tests/test_poisson_mg_cpu.py)


def test_both_summation_modes_need_the_same_iterations():
    import poisson_trajectory_cases as T

    T.check_equal_iteration_counts("cg")
