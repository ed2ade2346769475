"""CPU checks of the multigrid-preconditioned Poisson solver (method "mgcg"): the arguments are validated before anything touches a
device; the hierarchy rule; the numpy restatement of the V-cycle (tests/poisson_mg_cases.py) is a symmetric positive operator whose
diagonal is the matrix's, and conjugate gradients around it reproduce the reference's golden solutions; the new entry points are in
the ABI table and in the built library; the host shim, which lacks them, refuses the method and names them."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import pde_hip
import refpath
import shimlib
from helpers import GOLDEN, get_case, host_faces, load_cases
from pde_hip import _abi, poisson
from poisson_cases import make_grid, matrix_and_vector
from poisson_mg_cases import Cycle, hierarchy, mgcg

NPZ = np.load(GOLDEN / "poisson.npz", allow_pickle=False)
NEW = ["poisson_set_multigrid", "poisson_precondition"]
DENSE = [c["id"] for c in load_cases(NPZ) if int(np.prod(c["shape"])) <= 2000 and not c.get("raises")]
MIXED = {"type": "mixed", "value": 0.8, "const": 0.3}
SMALL = [
    ("1d-dirichlet", [12], [False], {"value": 0.3}),
    ("1d-periodic", [8], [True], "periodic"),
    ("1d-one-cell", [1], [False], [[{"value": 1.0}, {"derivative": 0.5}]]),
    ("2d-mixed", [8, 6], [False, False], [[{"value": 0.5}, MIXED], [{"derivative": -0.2}, {"value": 2.0}]]),
    ("2d-neumann-periodic", [6, 8], [False, True], [{"derivative": 0.0}, "periodic"]),
    ("2d-two-cells", [2, 5], [True, False], ["periodic", {"value": 0.0}]),
    ("2d-array-face", [6, 8], [False, False], [[{"value": np.linspace(0, 1, 8)}, {"type": "mixed", "value": np.linspace(0.2, 1.5, 8), "const": 0.1}], {"value": 0.0}]),
    ("3d-faces", [4, 6, 4], [False, True, False], [[{"value": 1.0}, MIXED], "periodic", {"derivative": 0.1}]),
]


def small_grid(shape, periodic):
    return pde_hip.CartesianGrid([[0, 0.7 * n + 0.5] for n in shape], shape, periodic=periodic)


def test_method_is_accepted_and_scipy_still_refused():
    poisson.check_method("mgcg")
    assert poisson.METHODS == ("auto", "cg", "mgcg")
    with pytest.raises(ValueError, match="Method scipy is not available"):
        poisson.check_method("scipy")


def test_arguments_are_validated_before_a_device_is_touched():
    grid = pde_hip.UnitGrid([8, 8])
    bcs = grid.get_boundary_conditions({"value": 0})
    backend = pde_hip.get_backend("hip")
    info = backend.get_operator_info(grid, "poisson_solver")
    for method in ("cg", "auto"):
        with pytest.raises(TypeError, match="mg_smooth.*need method=\"mgcg\""):
            info.factory(grid, backend=backend, bcs=bcs, method=method, mg_smooth=2)
    with pytest.raises(TypeError, match="unknown argument"):
        info.factory(grid, backend=backend, bcs=bcs, method="mgcg", mg_cycles=2)
    for name in ("mg_smooth", "mg_coarse", "mg_levels"):
        for bad in (0, -1, 1.5):
            with pytest.raises(ValueError, match=f"{name} must be a positive integer"):
                info.factory(grid, backend=backend, bcs=bcs, method="mgcg", **{name: bad})
    assert poisson.mg_options("mgcg", {}) == {"mg_smooth": 2, "mg_coarse": 32, "mg_levels": None}
    assert poisson.mg_options("cg", {}) == {} and poisson.MG_MAXITER == 200
    assert poisson.default_maxiter([512, 512, 512]) == 25600            # the plain loop keeps its default


def test_hierarchy_rule():
    assert hierarchy([512, 512, 512]) == [(512,) * 3, (256,) * 3, (128,) * 3, (64,) * 3, (32,) * 3, (16,) * 3, (8,) * 3]
    assert hierarchy([513, 513, 513]) == [(513, 513, 513)]
    assert hierarchy([500, 500, 300]) == [(500, 500, 300), (250, 250, 150), (125, 125, 75)]
    assert hierarchy([128, 128, 126]) == [(128, 128, 126), (64, 64, 63), (32, 32, 63), (16, 16, 63), (8, 8, 63), (4, 4, 63), (2, 2, 63)]
    assert hierarchy([256, 256]) == [(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)]
    assert hierarchy([1]) == [(1,)] and hierarchy([2, 3]) == [(2, 3)] and hierarchy([3, 3, 3]) == [(3, 3, 3)]
    assert hierarchy([2, 2, 1024]) == [(2, 2, 1024), (2, 2, 512), (2, 2, 256), (2, 2, 128)]
    assert hierarchy([512, 512, 512], max_levels=3) == [(512,) * 3, (256,) * 3, (128,) * 3]
    assert hierarchy([4096]) == [(4096,), (2048,), (1024,), (512,)]


@pytest.mark.parametrize("name,shape,periodic,bc", SMALL, ids=[s[0] for s in SMALL])
def test_diagonal_equals_the_matrix_diagonal(name, shape, periodic, bc):
    grid = small_grid(shape, periodic)
    matrix, _ = matrix_and_vector(grid, bc)
    cyc = Cycle(grid, bc, max_levels=1)
    assert np.abs(cyc.levels[0].diagonal().ravel() + np.diag(matrix)).max() <= 1e-13 * np.abs(np.diag(matrix)).max()
    assert np.abs((cyc.levels[0].minus_a(np.ones(shape)) + (matrix @ np.ones(matrix.shape[0])).reshape(shape))).max() < 1e-12


@pytest.mark.parametrize("name,shape,periodic,bc", [s for s in SMALL if int(np.prod(s[1])) > 1], ids=[s[0] for s in SMALL if int(np.prod(s[1])) > 1])
def test_restated_cycle_is_symmetric_and_positive(name, shape, periodic, bc):
    grid = small_grid([2 * n for n in shape], periodic)      # two levels at least
    if name == "2d-array-face":
        bc = [[{"value": np.linspace(0, 1, 16)}, {"type": "mixed", "value": np.linspace(0.2, 1.5, 16), "const": 0.1}], {"value": 0.0}]
    cyc = Cycle(grid, bc, smooth=2, coarse=8, stop_cells=8)
    assert len(cyc.levels) >= 2
    m = cyc.matrix()
    assert np.abs(m - m.T).max() <= 1e-13 * np.abs(m).max()
    assert np.linalg.eigvalsh(0.5 * (m + m.T)).min() > 0


@pytest.mark.parametrize("cid", DENSE)
def test_restated_mgcg_reproduces_the_dense_solutions(cid):
    case = get_case(NPZ, cid)
    grid = make_grid(case)
    rhs = NPZ[f"{cid}/rhs"]
    singular = poisson.is_singular(host_faces(grid.get_boundary_conditions(case["bc"])).c, grid.num_axes)
    got, iters = mgcg(grid, case["bc"], rhs, rtol=1e-12, singular=singular, stop_cells=32)
    want = NPZ[f"{cid}/solution"]
    if singular:
        want = want - want.mean()
    assert np.abs(got - want).max() <= 1e-8 * max(1.0, np.abs(want).max())
    assert 0 < iters <= 60


def test_abi_table_lists_the_entry_points_and_the_library_exports_them():
    for name in NEW:
        assert "pdehip_" + name in _abi.exported_symbols()
        assert name in _abi.OPTIONAL_PROTOTYPES
        assert name not in _abi.COMPUTE_PROTOTYPES and name not in _abi.COMM_PROTOTYPES and name not in _abi.RUNTIME_PROTOTYPES
    assert C.sizeof(_abi.Poisson) == 64
    assert C.sizeof(_abi.PoissonMg) == 4 * 4 + 8 + _abi.MG_MAX_LEVELS * 3 * 8 + 8
    from pde_hip import _lib

    assert not (set(NEW) & _lib.get_lib().missing)


def test_host_shim_refuses_the_method_and_names_the_entry_points():
    if refpath.REAL:
        pytest.skip("the real library has the entry points")
    with shimlib.use_shim() as lib:
        assert set(NEW) <= lib.missing
        grid = pde_hip.UnitGrid([8, 8])
        with pytest.raises(NotImplementedError, match="pdehip_poisson_create"):      # the shim has no Poisson solver at all: named first
            grid.make_operator("poisson_solver", {"value": 0.0}, backend="hip", method="mgcg")
        # a library with the plain solver but without the multigrid entry points: the two new ones are named
        plain = set(poisson.ENTRY_POINTS) & lib.missing
        lib.missing -= plain
        try:
            with pytest.raises(NotImplementedError, match="pdehip_poisson_precondition, pdehip_poisson_set_multigrid"):
                grid.make_operator("poisson_solver", {"value": 0.0}, backend="hip", method="mgcg")
        finally:
            lib.missing |= plain


def test_trajectory_tolerances_hold_for_the_restated_mgcg():
    """The preconditioned cases of tests/test_hip_poisson_trajectory.py (the checks: tests/poisson_trajectory_cases.py)."""
    import poisson_trajectory_cases as T

    T.check_tolerances("mgcg")


def test_both_summation_modes_need_the_same_mgcg_iterations():
    import poisson_trajectory_cases as T

    T.check_equal_iteration_counts("mgcg")


def test_mgcg_returns_a_trajectory_like_cg():
    grid = small_grid([8, 6], [False, False])
    bc = SMALL[3][3]
    f = np.random.default_rng(2).uniform(-1, 1, grid.shape)
    u, iters = mgcg(grid, bc, f, rtol=1e-10, stop_cells=8)
    traj = mgcg(grid, bc, f, rtol=1e-10, stop_cells=8, sums="numpy")
    assert traj.status == 0 and traj.iterations == iters == len(traj.scalars) == len(traj.iterates)
    assert np.array_equal(traj.x, u) and np.array_equal(traj.iterates[-1], u)
    short = mgcg(grid, bc, f, rtol=1e-10, maxiter=2, stop_cells=8, sums="exact")
    assert short.status == 1 and short.iterations == 2 and np.abs(short.iterates[1] - traj.iterates[1]).max() <= 1e-12 * np.abs(u).max()
    with pytest.raises(RuntimeError, match="did not converge within 2"):
        mgcg(grid, bc, f, rtol=1e-10, maxiter=2, stop_cells=8)
    with pytest.raises(RuntimeError, match="ended with a non-finite scalar after 0 iterations"):      # other statuses keep their name
        mgcg(grid, bc, np.where(f > 0.9, np.nan, f), rtol=1e-10, stop_cells=8)
