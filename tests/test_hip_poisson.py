"""GPU tests of the Poisson solver on the mirror classes: the reference's golden solutions, residuals of large grids measured with the
existing device Laplacian, fp32 and complex fields, determinism, independence of the batch size, iteration counts, the failure modes
and the refusals; the stop rule and the return statuses (tests/poisson_stop_cases.py); conditions given as expressions of the
coordinates and of time.  On a library without the operator every test here fails."""

from __future__ import annotations

import numpy as np
import pytest

import pde_hip
import poisson_stop_cases as stop
from helpers import GOLDEN, get_case, load_cases

pytestmark = pytest.mark.gpu

NPZ = np.load(GOLDEN / "poisson.npz", allow_pickle=False)
MIXED = {"type": "mixed", "value": 0.8, "const": 0.3}


@pytest.fixture(scope="module")
def backend():
    return pde_hip.get_backend("hip")


def make_grid(case):
    return pde_hip.CartesianGrid(case["bounds"], case["shape"], periodic=case["periodic"])


def rel_max(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


@pytest.mark.parametrize("cid", [c["id"] for c in load_cases(NPZ) if not c.get("raises") and c["rhs"] != "laplace"])
def test_golden_solutions(cid, backend):
    case = get_case(NPZ, cid)
    grid = make_grid(case)
    op = grid.make_operator("poisson_solver", case["bc"], backend=backend)
    got = op(NPZ[f"{cid}/rhs"])
    assert op.info["converged"] and op.info["iterations"] > 0
    want = NPZ[f"{cid}/solution"]
    if "zero-mean" in cid:
        # singular systems: the solver returns the solution of minimum norm (mean zero); the reference returns that one (lsmr) or, when
        # its direct solver did not notice the rank, another member of the family - compared up to the constant
        assert abs(got.mean()) < 1e-10
        want = want - want.mean()
    assert rel_max(got, want) < 1e-8
    res = pde_hip.solve_poisson_equation(pde_hip.ScalarField(grid, NPZ[f"{cid}/rhs"]), case["bc"])
    assert res.label == str(NPZ[f"{cid}/label"]) and np.array_equal(res.data, got)


def test_solve_laplace_equation_equals_its_golden(backend):
    case = get_case(NPZ, "2d-laplace")
    res = pde_hip.solve_laplace_equation(make_grid(case), case["bc"])
    assert res.label == str(NPZ["2d-laplace/label"]) == "Solution to Laplace's equation"
    assert rel_max(res.data, NPZ["2d-laplace/solution"]) < 1e-8


def test_singular_inconsistent_raises_like_the_reference(backend):
    case = get_case(NPZ, "2d-periodic-nonzero-mean")
    grid = make_grid(case)
    rhs = pde_hip.ScalarField(grid, NPZ["2d-periodic-nonzero-mean/rhs"])
    with pytest.raises(RuntimeError) as err:
        pde_hip.solve_poisson_equation(rhs, case["bc"])
    want = str(NPZ["2d-periodic-nonzero-mean/message"])
    assert str(err.value).split("magnitude")[0] == want.split("magnitude")[0]
    assert "Poisson problem could not be solved (Residual:" in str(err.value.__cause__)
    op = grid.make_operator("poisson_solver", case["bc"], backend=backend)
    with pytest.raises(RuntimeError, match=r"could not be solved \(Residual"):
        op(rhs.data)
    # the same operator, a consistent right-hand side: solved
    got = op(rhs.data - rhs.data.mean())
    assert op.info["converged"] and abs(got.mean()) < 1e-12


@pytest.mark.parametrize("n,bc", [(128, {"value": 0.0}), (128, [[{"value": 0.5}, MIXED], [{"derivative": -0.2}, {"value": 2.0}], "periodic"]),
                                  (256, {"value": 0.0}), (256, [[{"value": 0.5}, MIXED], [{"derivative": -0.2}, {"value": 2.0}], "periodic"])])
def test_residual_on_large_grids(n, bc, backend):
    """||L u - f||_2 <= 10 rtol ||f - v||_2 with L the existing device Laplacian (conditions included), v = L(0)."""
    periodic = [False, False, isinstance(bc, list)]
    grid = pde_hip.CartesianGrid([[0, 1.0 * n], [0, 0.5 * n], [0, 2.0 * n]], [n, n, n], periodic=periodic)
    rng = np.random.default_rng(n)
    f = pde_hip.ScalarField(grid, rng.uniform(-1, 1, grid.shape))
    rtol = 1e-8
    op = grid.make_operator("poisson_solver", bc, backend=backend, rtol=rtol)
    u = pde_hip.ScalarField(grid, op(f.data))
    assert op.info["converged"]
    v = pde_hip.ScalarField(grid, 0.0).laplace(bc).data
    resid = np.linalg.norm((u.laplace(bc).data - f.data).ravel())
    assert resid <= 10 * rtol * np.linalg.norm((f.data - v).ravel()), (resid, op.info)
    assert abs(op.info["rhs_norm"] - np.linalg.norm((f.data - v).ravel())) <= 1e-9 * op.info["rhs_norm"]


def test_fp32_fields(backend):
    case = get_case(NPZ, "3d-faces")
    grid = make_grid(case)
    rhs = NPZ["3d-faces/rhs"].astype(np.float32)
    got = grid.make_operator("poisson_solver", case["bc"], backend=backend)(rhs)
    assert got.dtype == np.float32 and rel_max(got, NPZ["3d-faces/solution"]) < 1e-5
    res = pde_hip.solve_poisson_equation(pde_hip.ScalarField(grid, rhs, dtype=np.float32), case["bc"])
    assert res.data.dtype == np.float32 and np.array_equal(res.data, got)


def test_complex_fields(backend):
    case = get_case(NPZ, "2d-dx-walls")
    grid = make_grid(case)
    re, im = NPZ["2d-dx-walls/rhs"], NPZ["2d-dx-periodic-mixed/rhs"]
    bc = [[{"value": 0.7 + 0.2j}, {"derivative": 0.25}], [{"value": 1j}, {"value": -1.0}]]
    got = grid.make_operator("poisson_solver", bc, backend=backend, dtype=complex)(re + 1j * im)
    assert np.iscomplexobj(got)
    bc_re = [[{"value": 0.7}, {"derivative": 0.25}], [{"value": 0.0}, {"value": -1.0}]]
    bc_im = [[{"value": 0.2}, {"derivative": 0.0}], [{"value": 1.0}, {"value": 0.0}]]
    want_re = grid.make_operator("poisson_solver", bc_re, backend=backend)(re)
    want_im = grid.make_operator("poisson_solver", bc_im, backend=backend)(im)
    assert np.array_equal(got.real, want_re) and np.array_equal(got.imag, want_im)


def test_two_runs_and_batch_sizes_give_equal_bits(backend):
    grid = pde_hip.CartesianGrid([[0, 40], [0, 20], [0, 64]], [40, 36, 128], periodic=[False, True, False])
    bc = [[{"value": 1.0}, MIXED], "periodic", {"derivative": 0.1}]
    f = np.random.default_rng(3).uniform(-1, 1, grid.shape)
    runs = []
    for batch in (32, 32, 1, 7):
        op = grid.make_operator("poisson_solver", bc, backend=backend, batch=batch)
        runs.append((op(f), op.info["iterations"], op.info["residual"]))
    for data, iters, res in runs[1:]:
        assert np.array_equal(data, runs[0][0]) and iters == runs[0][1] and res == runs[0][2]


def test_1d_dirichlet_needs_at_most_n_iterations(backend):
    n = 96
    grid = pde_hip.UnitGrid([n])
    op = grid.make_operator("poisson_solver", {"value": 0.0}, backend=backend, rtol=1e-9)
    f = np.random.default_rng(5).uniform(-1, 1, grid.shape)
    u = op(f)
    assert op.info["converged"] and op.info["iterations"] <= n
    lap = pde_hip.ScalarField(grid, u).laplace({"value": 0.0}).data
    assert np.linalg.norm(lap - f) <= 1e-7 * np.linalg.norm(f)
    # odd row length: the one-cell-per-thread instances
    grid = pde_hip.UnitGrid([33, 31])
    op = grid.make_operator("poisson_solver", {"value": 0.0}, backend=backend)
    f = np.random.default_rng(6).uniform(-1, 1, grid.shape)
    lap = pde_hip.ScalarField(grid, op(f)).laplace({"value": 0.0}).data
    assert np.linalg.norm(lap - f) <= 1e-8 * np.linalg.norm(f)


def test_maxiter_raises_convergence_error_and_the_operator_survives(backend):
    grid = pde_hip.UnitGrid([32, 32])
    f = np.random.default_rng(7).uniform(-1, 1, grid.shape)
    op = grid.make_operator("poisson_solver", {"value": 0.0}, backend=backend, maxiter=3)
    with pytest.raises(pde_hip.ConvergenceError, match="within 3 iterations"):
        op(f)
    assert op.info["iterations"] == 3 and not op.info["converged"]
    with pytest.raises(pde_hip.ConvergenceError):
        pde_hip.solve_poisson_equation(pde_hip.ScalarField(grid, f), {"value": 0.0}, maxiter=3)
    ok = grid.make_operator("poisson_solver", {"value": 0.0}, backend=backend)(f)
    assert np.isfinite(ok).all()


def test_second_right_hand_side_on_the_same_operator(backend):
    case = get_case(NPZ, "3d-faces")
    grid = make_grid(case)
    op = grid.make_operator("poisson_solver", case["bc"], backend=backend)
    first = op(NPZ["3d-faces/rhs"])
    other = op(2.0 * NPZ["3d-faces/rhs"] + 0.3)
    again = op(NPZ["3d-faces/rhs"])
    assert np.array_equal(first, again) and not np.array_equal(first, other)
    fresh = grid.make_operator("poisson_solver", case["bc"], backend=backend)(2.0 * NPZ["3d-faces/rhs"] + 0.3)
    assert np.array_equal(other, fresh)


def test_device_arrays_in_device_arrays_out(backend):
    from pde_hip.device import DeviceArray

    case = get_case(NPZ, "2d-dx-walls")
    grid = make_grid(case)
    op = grid.make_operator("poisson_solver", case["bc"], backend=backend)
    native = DeviceArray(backend.grid_info(grid, np.float64)).set_valid(NPZ["2d-dx-walls/rhs"], backend.stream)
    out = op(native)
    assert isinstance(out, DeviceArray) and np.array_equal(out.get_valid(stream=backend.stream), op(NPZ["2d-dx-walls/rhs"]))


def test_coefficient_arrays_on_a_face(backend):
    """A Dirichlet value that varies along the wall (PDEHIP_BCF_ARRAYS): residual with the device Laplacian."""
    grid = pde_hip.CartesianGrid([[0, 4.0], [0, 6.0]], [32, 48])
    bc = [[{"value": np.linspace(0, 1, 48)}, {"derivative": 0.2}], {"value": 0.0}]
    f = np.random.default_rng(8).uniform(-1, 1, grid.shape)
    op = grid.make_operator("poisson_solver", bc, backend=backend)
    u = pde_hip.ScalarField(grid, op(f))
    assert op.info["converged"]
    assert np.linalg.norm(u.laplace(bc).data - f) <= 1e-8 * np.linalg.norm(f)


def test_curvature_face_is_refused(backend):
    grid = pde_hip.UnitGrid([16, 16])
    with pytest.raises(NotImplementedError, match="lower face of axis 0 is a second-order condition"):
        grid.make_operator("poisson_solver", [{"curvature": 0.5}, {"value": 0.0}], backend=backend)
    with pytest.raises(ValueError, match="Method scipy is not available"):
        grid.make_operator("poisson_solver", {"value": 0.0}, backend=backend, method="scipy")
    with pytest.raises(ValueError, match="built from the boundary conditions"):
        grid.make_operator_no_bc("poisson_solver", backend=backend)


def test_last_kernel_name_names_the_fused_sweep(backend):
    from pde_hip import _lib

    grid = pde_hip.UnitGrid([16, 16, 64])
    grid.make_operator("poisson_solver", {"value": 0.0}, backend=backend)(np.ones(grid.shape))
    name = _lib.get_lib().last_kernel_name().decode()
    assert "poisson_apply_kernel" in name and "r.r and r.w" in name, name


# ---- stop rule and statuses (the preconditioned twins: tests/test_hip_poisson_mg.py) ------------------------------------------------
def test_atol_stops_at_the_restatements_iteration(backend):
    stop.check_atol(backend, "cg")


def test_right_hand_side_of_the_zero_field_needs_no_iteration(backend):
    stop.check_zero_iterations(backend, "cg")


def test_nan_and_inf_are_a_status_and_the_operator_survives(backend):
    stop.check_nonfinite(backend, "cg")


def test_indefinite_system_breaks_down_at_the_restatements_iteration(backend):
    stop.check_breakdown(backend, "cg")


# ---- conditions given as expressions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["cg", "mgcg"])
def test_expression_conditions_equal_the_same_values_as_arrays(method, backend):
    """Coefficients that are powers of two: the expression and the array hold the same bits whatever the order of the products."""
    grid = pde_hip.CartesianGrid([[0, 4.0], [0, 6.0]], [32, 48])
    y = np.asarray(grid.axes_coords[1])
    as_expr = [[{"value_expression": "0.5 + 0.25*y"}, {"derivative_expression": "0.125*y"}], {"value": 0.0}]
    as_arrays = [[{"value": 0.5 + 0.25 * y}, {"derivative": 0.125 * y}], {"value": 0.0}]
    f = np.random.default_rng(31).uniform(-1, 1, grid.shape)
    a = grid.make_operator("poisson_solver", as_expr, backend=backend, method=method)
    b = grid.make_operator("poisson_solver", as_arrays, backend=backend, method=method)
    assert np.array_equal(a(f), b(f)) and a.info == b.info and a.info["iterations"] > 0
    u = pde_hip.ScalarField(grid, a(f))
    assert np.linalg.norm(u.laplace(as_arrays).data - f) <= 1e-8 * np.linalg.norm(f)


@pytest.mark.parametrize("method", ["cg", "mgcg"])
def test_time_dependent_condition_is_refreshed_on_every_solve(method, backend):
    """One operator, two times: each solve equals a fresh operator with the value of that time as a constant (the handle is rebuilt on
    every solve, because the coefficient arrays - and with them whether the system is singular - may have changed)."""
    grid = pde_hip.CartesianGrid([[0, 4.0], [0, 6.0]], [32, 48])
    f = np.random.default_rng(32).uniform(-1, 1, grid.shape)
    op = grid.make_operator("poisson_solver", [[{"value_expression": "0.5 + 0.25*t"}, {"derivative": 0.2}], {"value": 0.0}], backend=backend, method=method)
    got = {t: op(f, args={"t": t}).copy() for t in (1.0, 3.0, 1.0)}
    for t, value in ((1.0, 0.75), (3.0, 1.25)):
        fresh = grid.make_operator("poisson_solver", [[{"value": value}, {"derivative": 0.2}], {"value": 0.0}], backend=backend, method=method)
        assert np.array_equal(got[t], fresh(f)), t
    assert not np.array_equal(got[1.0], got[3.0])
    with pytest.raises(RuntimeError, match="Require value for `t`"):
        op(f)


def test_expression_that_reads_the_value_is_refused(backend):
    """(No CPU twin: the refusal is made by `_Solver` after the expression table has uploaded its coefficient arrays, and the host shim
    of the CPU tests has no Poisson entry points, so the operator is refused there before it gets that far.)"""
    grid = pde_hip.UnitGrid([16, 16])
    for bc in ({"value_expression": "value**2"}, {"derivative_expression": "0.1 - 0.3 * value**3"}):
        with pytest.raises(NotImplementedError, match="not affine in the adjacent value: the problem is not linear"):
            grid.make_operator("poisson_solver", [[bc, {"value": 0.0}], {"value": 0.0}], backend=backend)
