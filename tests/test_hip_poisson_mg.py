"""GPU tests of the multigrid-preconditioned Poisson solver (method "mgcg"): the reference's golden solutions, the V-cycle on its own
against the numpy restatement (tests/poisson_mg_cases.py) with its symmetry and positivity, iteration counts that do not grow with
the grid - the point of the method -, grids that coarsen badly or not at all, fp32 / complex / device arrays, failure modes and
determinism.  On a library without the method every test here fails."""

from __future__ import annotations

import numpy as np
import pytest

import pde_hip
import poisson_stop_cases as stop
from helpers import GOLDEN, get_case, load_cases
from poisson_mg_cases import Cycle, hierarchy

pytestmark = pytest.mark.gpu

NPZ = np.load(GOLDEN / "poisson.npz", allow_pickle=False)
MIXED = {"type": "mixed", "value": 0.8, "const": 0.3}
FACES3 = [[{"value": 0.5}, MIXED], [{"derivative": -0.2}, {"value": 2.0}], "periodic"]


@pytest.fixture(scope="module")
def backend():
    return pde_hip.get_backend("hip")


def make_grid(case):
    return pde_hip.CartesianGrid(case["bounds"], case["shape"], periodic=case["periodic"])


def rel_max(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


def apply_cycle(backend, grid, bc, r, **kwargs):
    """z = M r through pdehip_poisson_precondition."""
    from pde_hip.device import DeviceArray

    op = grid.make_operator("poisson_solver", bc, backend=backend, method="mgcg", **kwargs)
    info = backend.grid_info(grid, np.float64)
    r_dev = DeviceArray(info).set_valid(np.ascontiguousarray(r, dtype=np.float64), backend.stream)
    z_dev = op.solver_for(None).precondition(r_dev, DeviceArray(info))
    return z_dev.get_valid(stream=backend.stream), op


@pytest.mark.parametrize("cid", [c["id"] for c in load_cases(NPZ) if not c.get("raises") and c["rhs"] != "laplace"])
def test_golden_solutions(cid, backend):
    case = get_case(NPZ, cid)
    grid = make_grid(case)
    op = grid.make_operator("poisson_solver", case["bc"], backend=backend, method="mgcg")
    got = op(NPZ[f"{cid}/rhs"])
    assert op.info["converged"] and op.info["iterations"] > 0 and op.info["method"] == "mgcg"
    assert op.info["level_shapes"] == hierarchy(grid.shape) and op.info["levels"] == len(op.info["level_shapes"])
    want = NPZ[f"{cid}/solution"]
    if "zero-mean" in cid:
        assert abs(got.mean()) < 1e-10
        want = want - want.mean()
    assert rel_max(got, want) < 1e-8
    res = pde_hip.solve_poisson_equation(pde_hip.ScalarField(grid, NPZ[f"{cid}/rhs"]), case["bc"], method="mgcg")
    assert res.label == str(NPZ[f"{cid}/label"]) and np.array_equal(res.data, got)


def test_laplace_golden_and_the_inconsistent_singular_case(backend):
    case = get_case(NPZ, "2d-laplace")
    grid = make_grid(case)
    got = grid.make_operator("poisson_solver", case["bc"], backend=backend, method="mgcg")(np.zeros(grid.shape))
    assert rel_max(got, NPZ["2d-laplace/solution"]) < 1e-8
    case = get_case(NPZ, "2d-periodic-nonzero-mean")
    grid = make_grid(case)
    rhs = pde_hip.ScalarField(grid, NPZ["2d-periodic-nonzero-mean/rhs"])
    with pytest.raises(RuntimeError) as err:
        pde_hip.solve_poisson_equation(rhs, case["bc"], method="mgcg")
    want = str(NPZ["2d-periodic-nonzero-mean/message"])
    assert str(err.value).split("magnitude")[0] == want.split("magnitude")[0]
    assert "Poisson problem could not be solved (Residual:" in str(err.value.__cause__)


def ramp(m1, m2, a, b, c=0.0):
    return a * np.linspace(0, 1, m1)[:, None] + b * np.linspace(0, 1, m2)[None, :] + c


ARRAY_FACES3 = [[{"value": ramp(10, 36, 1.0, 0.5)}, {"type": "mixed", "value": ramp(10, 36, 0.3, 1.1, 0.2), "const": 0.1}],
                [{"type": "mixed", "value": ramp(40, 36, 0.7, 0.2, 0.1), "const": ramp(40, 36, 0.1, 0.1)}, {"value": ramp(40, 36, 0.2, 0.9)}],
                [{"derivative": ramp(40, 10, 0.4, 0.3)}, {"type": "mixed", "value": ramp(40, 10, 0.25, 1.3, 0.4), "const": 0.0}]]

CYCLES = [
    ("1d-even", [[0, 3.0]], [1024], [False], [[{"value": 0.2}, {"derivative": 0.1}]], {}),
    ("1d-odd-no-coarsening", [[0, 3.0]], [777], [True], "periodic", {"mg_coarse": 5}),
    ("2d-mixed-even", [[0, 2.0], [0, 3.0]], [48, 64], [False, False], [[{"value": 0.5}, MIXED], [{"derivative": -0.2}, {"value": 2.0}]], {}),
    ("2d-odd-rows", [[0, 2.0], [0, 3.0]], [40, 51], [True, False], ["periodic", {"value": 0.0}], {"mg_smooth": 3}),
    ("2d-array-face", [[0, 4.0], [0, 6.0]], [32, 48], [False, False],
     [[{"value": np.linspace(0, 1, 48)}, {"type": "mixed", "value": np.linspace(0.2, 1.5, 48), "const": 0.1}], [{"derivative": 0.2}, {"value": 0.0}]], {}),
    ("3d-faces", [[0, 1.0], [0, 0.5], [0, 2.0]], [24, 20, 32], [False, False, True], FACES3, {}),
    ("3d-one-sweep", [[0, 1.0], [0, 1.0], [0, 1.0]], [16, 16, 18], [False, True, False], [{"derivative": 0.0}, "periodic", {"value": 1.0}], {"mg_smooth": 1, "mg_coarse": 1}),
    ("3d-two-levels", [[0, 1.0], [0, 1.0], [0, 1.0]], [32, 32, 32], [False, False, False], {"value": 0.0}, {"mg_levels": 2, "mg_coarse": 3}),
    # coefficient arrays on the faces of all three axes, every factor array from two different ramps (a transposed or mis-strided face
    # shows); 40 x 10 x 36 -> 20 x 5 x 18 -> 10 x 5 x 9: the first transfer halves both axes of the faces of axis 1, the second only one
    # axis of the faces of axes 0 and 2
    ("3d-array-faces", [[0, 1.0], [0, 0.5], [0, 2.0]], [40, 10, 36], [False, False, False], ARRAY_FACES3, {}),
    ("3d-array-faces-one-transfer", [[0, 1.0], [0, 0.5], [0, 2.0]], [40, 10, 36], [False, False, False], ARRAY_FACES3, {"mg_levels": 2, "mg_coarse": 4}),
    # the last level 8 x 8 x 9 = 576 cells in LDS, every axis wrapping inside the one-workgroup kernel
    ("3d-lds-periodic", [[0, 1.0], [0, 0.5], [0, 2.0]], [16, 16, 18], [True, True, True], "periodic", {"mg_levels": 2}),
    ("3d-lds-mixed-periodic", [[0, 1.0], [0, 0.5], [0, 2.0]], [16, 16, 18], [True, False, True], ["periodic", [{"value": 0.5}, MIXED], "periodic"], {"mg_levels": 2, "mg_coarse": 7}),
    # an axis of extent 2: periodic (both neighbours are the same cell) and between walls
    ("3d-extent-2-periodic", [[0, 1.0], [0, 0.5], [0, 2.0]], [64, 2, 64], [False, True, False], [{"value": 0.5}, "periodic", {"derivative": 0.1}], {}),
    ("3d-extent-2-walls", [[0, 1.0], [0, 0.5], [0, 2.0]], [64, 2, 64], [False, False, False], [{"value": 0.5}, [{"derivative": -0.2}, MIXED], {"derivative": 0.1}], {}),
    ("2d-extent-2-periodic", [[0, 1.0], [0, 8.0]], [2, 64], [True, False], ["periodic", [{"value": 0.5}, MIXED]], {}),
    ("2d-extent-2-periodic-fastest", [[0, 8.0], [0, 1.0]], [64, 2], [False, True], [[{"value": 0.5}, MIXED], "periodic"], {"mg_coarse": 6}),
    # a 3-D last level above 1024 cells (12 x 10 x 16) with faces: one launch per sweep
    ("3d-large-last-level", [[0, 1.0], [0, 0.5], [0, 2.0]], [24, 20, 32], [False, False, True], FACES3, {"mg_levels": 2, "mg_coarse": 5}),
    # one sweep on a level in LDS: the loop over further sweeps runs zero times
    ("2d-lds-one-sweep", [[0, 2.0], [0, 3.0]], [32, 24], [False, False], [[{"value": 0.5}, MIXED], [{"derivative": -0.2}, {"value": 2.0}]], {"mg_coarse": 1}),
    ("1d-lds-one-sweep-one-level", [[0, 3.0]], [777], [True], "periodic", {"mg_coarse": 1}),
]


@pytest.mark.parametrize("name,bounds,shape,periodic,bc,opts", CYCLES, ids=[c[0] for c in CYCLES])
def test_cycle_equals_the_restatement(name, bounds, shape, periodic, bc, opts, backend):
    grid = pde_hip.CartesianGrid(bounds, shape, periodic=periodic)
    r = np.random.default_rng(len(name)).uniform(-1, 1, grid.shape)
    got, op = apply_cycle(backend, grid, bc, r, **opts)
    want = Cycle(grid, bc, smooth=opts.get("mg_smooth", 2), coarse=opts.get("mg_coarse", 32), max_levels=opts.get("mg_levels"))(r)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    again, _ = apply_cycle(backend, grid, bc, r, **opts)
    assert np.array_equal(got, again)


def test_cycle_is_symmetric_and_positive_at_64_cubed(backend):
    grid = pde_hip.CartesianGrid([[0, 1.0], [0, 0.5], [0, 2.0]], [64, 64, 64], periodic=[False, False, True])
    rng = np.random.default_rng(11)
    a, b = rng.uniform(-1, 1, grid.shape), rng.uniform(-1, 1, grid.shape)
    ma, _ = apply_cycle(backend, grid, FACES3, a)
    mb, _ = apply_cycle(backend, grid, FACES3, b)
    lhs, rhs = float((ma * b).sum()), float((a * mb).sum())
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(ma) * np.linalg.norm(b)
    assert float((a * ma).sum()) > 0 and float((b * mb).sum()) > 0


def solve_and_check(grid, bc, backend, seed, rtol=1e-8, singular=False, **kwargs):
    f = np.random.default_rng(seed).uniform(-1, 1, grid.shape)
    if singular:
        f -= f.mean()
    op = grid.make_operator("poisson_solver", bc, backend=backend, method="mgcg", rtol=rtol, **kwargs)
    u = pde_hip.ScalarField(grid, op(f))
    assert op.info["converged"]
    v = pde_hip.ScalarField(grid, 0.0).laplace(bc).data
    resid = np.linalg.norm((u.laplace(bc).data - f).ravel())
    assert resid <= 10 * rtol * np.linalg.norm((f - v).ravel()), (resid, op.info)
    return op.info, f


def test_iteration_count_does_not_grow_with_the_grid(backend):
    """The point of the method: all-Dirichlet unit grids, random right-hand side, rtol 1e-8."""
    counts = {}
    for n in (64, 128, 256):
        info, f = solve_and_check(pde_hip.UnitGrid([n, n, n]), {"value": 0.0}, backend, n)
        counts[n] = info["iterations"]
        assert info["iterations"] <= 25, counts
        assert info["levels"] == len(hierarchy([n, n, n]))
        if n == 128:
            plain = pde_hip.UnitGrid([n, n, n]).make_operator("poisson_solver", {"value": 0.0}, backend=backend, method="cg", rtol=1e-8)
            plain(f)
            assert plain.info["iterations"] > 10 * info["iterations"], (plain.info, info)
    assert counts[256] - counts[64] <= 4, counts


def test_mixed_faces_and_a_singular_system(backend):
    for n in (128, 256):
        grid = pde_hip.CartesianGrid([[0, 1.0 * n], [0, 0.5 * n], [0, 2.0 * n]], [n, n, n], periodic=[False, False, True])
        info, _ = solve_and_check(grid, FACES3, backend, n)
        assert info["iterations"] <= 100, info        # (spacings 1 : 0.5 : 2, i.e. stencil weights 1 : 4 : 1/4: a point smoother loses much of its grip)
    grid = pde_hip.UnitGrid([256, 256], periodic=[False, True])
    info, _ = solve_and_check(grid, [{"derivative": 0.0}, "periodic"], backend, 3, singular=True)
    assert info["iterations"] <= 30, info


def test_grids_that_coarsen_badly_still_converge(backend):
    info, _ = solve_and_check(pde_hip.UnitGrid([128, 128, 126]), {"value": 0.0}, backend, 5)
    assert info["level_shapes"][-1] == (2, 2, 63) and info["levels"] == 7 and info["iterations"] <= 100
    info, _ = solve_and_check(pde_hip.UnitGrid([33, 31]), {"value": 0.0}, backend, 6)
    assert info["levels"] == 1 and info["level_shapes"] == [(33, 31)]


def test_fp32_and_complex_fields(backend):
    case = get_case(NPZ, "3d-faces")
    grid = make_grid(case)
    rhs = NPZ["3d-faces/rhs"].astype(np.float32)
    got = grid.make_operator("poisson_solver", case["bc"], backend=backend, method="mgcg")(rhs)
    assert got.dtype == np.float32 and rel_max(got, NPZ["3d-faces/solution"]) < 1e-5
    case = get_case(NPZ, "2d-dx-walls")
    grid = make_grid(case)
    re, im = NPZ["2d-dx-walls/rhs"], NPZ["2d-dx-periodic-mixed/rhs"]
    bc = [[{"value": 0.7 + 0.2j}, {"derivative": 0.25}], [{"value": 1j}, {"value": -1.0}]]
    got = grid.make_operator("poisson_solver", bc, backend=backend, dtype=complex, method="mgcg")(re + 1j * im)
    bc_re = [[{"value": 0.7}, {"derivative": 0.25}], [{"value": 0.0}, {"value": -1.0}]]
    bc_im = [[{"value": 0.2}, {"derivative": 0.0}], [{"value": 1.0}, {"value": 0.0}]]
    want_re = grid.make_operator("poisson_solver", bc_re, backend=backend, method="mgcg")(re)
    want_im = grid.make_operator("poisson_solver", bc_im, backend=backend, method="mgcg")(im)
    assert np.iscomplexobj(got) and np.array_equal(got.real, want_re) and np.array_equal(got.imag, want_im)


def test_device_arrays_and_a_second_right_hand_side(backend):
    from pde_hip.device import DeviceArray

    case = get_case(NPZ, "3d-faces")
    grid = make_grid(case)
    op = grid.make_operator("poisson_solver", case["bc"], backend=backend, method="mgcg")
    first = op(NPZ["3d-faces/rhs"])
    other = op(2.0 * NPZ["3d-faces/rhs"] + 0.3)
    again = op(NPZ["3d-faces/rhs"])
    assert np.array_equal(first, again) and not np.array_equal(first, other)
    native = DeviceArray(backend.grid_info(grid, np.float64)).set_valid(NPZ["3d-faces/rhs"], backend.stream)
    out = op(native)
    assert isinstance(out, DeviceArray) and np.array_equal(out.get_valid(stream=backend.stream), first)


def test_maxiter_raises_and_the_operator_survives(backend):
    grid = pde_hip.UnitGrid([64, 64])
    f = np.random.default_rng(7).uniform(-1, 1, grid.shape)
    op = grid.make_operator("poisson_solver", {"value": 0.0}, backend=backend, method="mgcg", maxiter=2)
    with pytest.raises(pde_hip.ConvergenceError, match=r"mgcg\) did not converge within 2 iterations"):
        op(f)
    assert op.info["iterations"] == 2 and not op.info["converged"]
    ok = grid.make_operator("poisson_solver", {"value": 0.0}, backend=backend, method="mgcg")(f)
    assert np.isfinite(ok).all()


def test_runs_and_batch_sizes_give_equal_bits_and_the_plain_path_is_unchanged(backend):
    from pde_hip import _lib

    grid = pde_hip.CartesianGrid([[0, 40], [0, 20], [0, 64]], [40, 36, 128], periodic=[False, True, False])
    bc = [[{"value": 1.0}, MIXED], "periodic", {"derivative": 0.1}]
    f = np.random.default_rng(3).uniform(-1, 1, grid.shape)
    runs = []
    for batch in (32, 32, 1, 7):
        op = grid.make_operator("poisson_solver", bc, backend=backend, method="mgcg", batch=batch)
        runs.append((op(f), op.info["iterations"], op.info["residual"]))
    for data, iters, res in runs[1:]:
        assert np.array_equal(data, runs[0][0]) and iters == runs[0][1] and res == runs[0][2]
    name = _lib.get_lib().last_kernel_name().decode()
    assert "poisson_mg_apply_kernel" in name and "r.z, z.w and r.r" in name, name
    auto = grid.make_operator("poisson_solver", bc, backend=backend)
    plain = grid.make_operator("poisson_solver", bc, backend=backend, method="cg")
    a, c = auto(f), plain(f)
    assert np.array_equal(a, c) and auto.info["iterations"] == plain.info["iterations"] > runs[0][1]
    assert "poisson_apply_kernel" in _lib.get_lib().last_kernel_name().decode()
    assert rel_max(runs[0][0], a) < 1e-8


@pytest.mark.parametrize("method", ["mgcg", "cg"])
def test_factor_arrays_of_exact_ones_make_the_system_singular(method, backend):
    """Neumann conditions given as arrays on every face: the library reads the factor arrays (all ones) from the device, finds the
    system singular and returns the solution of mean zero."""
    from pde_hip.device import DeviceArray

    grid = pde_hip.CartesianGrid([[0, 1.0], [0, 0.5], [0, 2.0]], [40, 10, 36])
    centred = lambda m1, m2, a, b: ramp(m1, m2, a, b) - ramp(m1, m2, a, b).mean()      # noqa: E731  (no net flux through a face)
    bc = [[{"derivative": centred(10, 36, 0.4, 0.3)}, {"derivative": centred(10, 36, 0.1, -0.3)}], [{"derivative": centred(40, 36, 0.2, 0.1)}, {"derivative": np.zeros((40, 36))}],
          [{"derivative": centred(40, 10, -0.2, 0.3)}, {"derivative": centred(40, 10, 0.5, 0.5)}]]
    f = np.random.default_rng(12).uniform(-1, 1, grid.shape)
    f -= f.mean()
    op = grid.make_operator("poisson_solver", bc, backend=backend, method=method, rtol=1e-9)
    info = backend.grid_info(grid, np.float64)
    out = DeviceArray(info)
    status = op.solver_for(None).solve(DeviceArray(info).set_valid(f, backend.stream), out)
    assert status["singular"] and status["status"] == 0 and status["iterations"] > 0, status
    got = out.get_valid(stream=backend.stream)
    assert abs(got.mean()) < 1e-10
    u = pde_hip.ScalarField(grid, got)
    assert np.linalg.norm(u.laplace(bc).data - f) <= 1e-7 * np.linalg.norm(f)
    # one factor that is not one: regular
    bc[1][1] = {"type": "mixed", "value": np.where(np.arange(40 * 36).reshape(40, 36) == 777, 0.5, 0.0), "const": 0.0}
    op = grid.make_operator("poisson_solver", bc, backend=backend, method=method, rtol=1e-9)
    status = op.solver_for(None).solve(DeviceArray(info).set_valid(f, backend.stream), out)
    assert not status["singular"], status


# ---- stop rule and statuses: the twins of tests/test_hip_poisson.py ----------------------------------------------------------------------
def test_atol_stops_at_the_restatements_iteration(backend):
    stop.check_atol(backend, "mgcg")


def test_right_hand_side_of_the_zero_field_needs_no_iteration(backend):
    stop.check_zero_iterations(backend, "mgcg")


def test_nan_and_inf_are_a_status_and_the_operator_survives(backend):
    stop.check_nonfinite(backend, "mgcg")


def test_indefinite_system_breaks_down_near_the_restatements_iteration(backend):
    stop.check_breakdown(backend, "mgcg")
