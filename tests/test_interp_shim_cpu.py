"""The Python side of interpolation without a GPU: the host shim with the interpolation entry points (tests/interp_shimlib.py) stands in
for the library, so ``pde_hip/interpolation.py`` runs end to end - through the mirror classes and, where py-pde is importable, through the
plugin on REAL py-pde fields: ``field.make_interpolator(backend="hip")``, ``pde_hip.interpolate_to_grid``, py-pde's own ``DomainError`` and
the class of the result.  Values are compared with the restatement (tests/interp_cases.py) with ``np.array_equal``: the shim's plain C is the
same fp64 expressions in the same order.  The device kernels are tested on the GPU (tests/test_hip_interp.py)."""

from __future__ import annotations

import sys

import numpy as np
import pytest

import interp_cases as IC
import interp_shimlib
import pde_hip
import refpath
import shimlib
from helpers import GOLDEN
from pde_hip.interpolation import DomainError, error_classes

BOUNDS = [(-1.0, 2.0), (0.5, 3.0), (0.0, 1.0)]


def same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    np.testing.assert_array_equal(a, b)


@pytest.fixture
def shim():
    with interp_shimlib.use_shim() as lib:
        yield lib


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "interp.npz", allow_pickle=False)


def wall_points(grid):
    per_axis = [[lo, lo + 0.1 * dx, 0.5 * (lo + hi), hi - 0.3 * dx, hi] for (lo, hi), dx in zip(grid.axes_bounds, grid.discretization)]
    return np.array(np.meshgrid(*per_axis, indexing="ij")).reshape(len(per_axis), -1).T


@pytest.mark.parametrize("cid,shape,periodic,bc", IC.GOLDEN_CASES, ids=[c[0] for c in IC.GOLDEN_CASES])
def test_mirror_fields_with_conditions(shim, golden, cid, shape, periodic, bc):
    """``interpolate(bc=...)`` and ``interpolate_to_grid(bc=...)``: edges and corners as in the reference's full arrays (the golden)."""
    nd = len(shape)
    grid = pde_hip.CartesianGrid(IC.GOLDEN_BOUNDS[nd], shape, periodic=list(periodic))
    full, valid = golden[cid + "/full"], golden[cid + "/valid"]
    field = pde_hip.ScalarField(grid, valid)
    field.set_ghost_cells(bc, set_corners=True)
    np.testing.assert_array_equal(field._data_full, full)
    points = wall_points(grid)
    same(pde_hip.ScalarField(grid, valid).interpolate(points, bc=bc), IC.interpolate(grid, full, points, with_ghost_cells=True))
    dst = pde_hip.CartesianGrid(IC.GOLDEN_BOUNDS[nd], tuple(2 * n + 1 for n in shape))
    same(field.interpolate_to_grid(dst, bc=bc).data, IC.interpolate(grid, full, dst.cell_coords, with_ghost_cells=True))


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.complex128])
def test_mirror_fields_types_fill_and_errors(shim, dtype, rng):
    grid = pde_hip.CartesianGrid(BOUNDS[:2], (3, 4), periodic=[False, True])
    data = IC.field_data(grid.shape, (2,), dtype, seed=1)
    field = pde_hip.VectorField(grid, data)
    lo, hi = np.array(BOUNDS[:2]).T
    points = lo + (hi - lo) * rng.uniform(-0.1, 1.1, (7, 5, 2))
    same(field.make_interpolator(fill=[1.0, -2.0])(points), IC.interpolate(grid, data, points, fill=[1.0, -2.0]))
    interp = field.make_interpolator()
    inside = lo + (hi - lo) * rng.uniform(0, 1, (300, 2))
    for count in (1, 300, 7):                                # the buffers kept between calls grow and are reused
        same(interp(inside[:count]), IC.interpolate(grid, data, inside[:count]))
    with pytest.raises(DomainError if "pde" not in sys.modules else error_classes()[0], match="Point lies outside the grid domain"):
        interp(points)
    same(interp(inside[:3]), IC.interpolate(grid, data, inside[:3]))      # the counter starts from zero again
    dst = pde_hip.CartesianGrid(BOUNDS[:2], (5, 9), periodic=[False, True])
    res = field.interpolate_to_grid(dst)
    assert type(res) is pde_hip.VectorField
    same(res.data, IC.interpolate(grid, data, dst.cell_coords))


def test_a_subclass_of_the_cartesian_grid_is_cartesian(shim):
    class MyGrid(pde_hip.CartesianGrid):
        pass

    grid = MyGrid([(0.0, 2.0)], (4,))
    data = IC.field_data(grid.shape)
    points = np.array([[0.3], [1.9]])
    same(pde_hip.ScalarField(grid, data).make_interpolator()(points), IC.interpolate(grid, data, points))


def test_a_library_without_the_entry_points_is_refused():
    if refpath.REAL:
        pytest.skip("the real library has the entry points")
    with shimlib.use_shim() as lib:
        assert not lib.has("interpolate_points") and not lib.has("set_ghost_corners")
        grid = pde_hip.UnitGrid([4, 4])
        field = pde_hip.ScalarField(grid, 1.0)
        with pytest.raises(NotImplementedError, match="no interpolation kernels"):
            field.make_interpolator()(np.array([[1.0, 1.0]]))
        with pytest.raises(NotImplementedError, match="no interpolation kernels"):
            field.interpolate_to_grid(pde_hip.UnitGrid([4, 4]))
        with pytest.raises(NotImplementedError, match="no interpolation kernels"):
            field.set_ghost_cells({"value": 0.0}, set_corners=True)


# ---- the plugin on REAL py-pde fields ---------------------------------------------------------------------------------------------
@pytest.fixture
def pde():
    mod = refpath.import_reference()
    if mod is None:
        pytest.skip("py-pde (reference) not available")
    import pde_hip.pypde_plugin  # noqa: F401  (registers "hip")

    return mod


def test_plugin_interpolator_on_pypde_fields(pde, shim, rng):
    grid = pde.CartesianGrid(BOUNDS[:2], (5, 6), periodic=[True, False])
    mirror = pde_hip.CartesianGrid(BOUNDS[:2], (5, 6), periodic=[True, False])
    lo, hi = np.array(BOUNDS[:2]).T
    points = lo + (hi - lo) * rng.uniform(0, 1, (50, 2))
    for cls, rank, dtype in ((pde.ScalarField, 0, np.float64), (pde.VectorField, 1, np.float64), (pde.Tensor2Field, 2, np.complex128)):
        data = IC.field_data(grid.shape, (2,) * rank, dtype, seed=11 + rank)
        field = cls(grid, data, dtype=dtype)
        same(field.make_interpolator(backend="hip")(points), IC.interpolate(mirror, data, points))
        same(field.make_interpolator(backend="hip", fill=0.5)(points + 1.0), IC.interpolate(mirror, data, points + 1.0, fill=0.5))
    field = pde.ScalarField(grid, IC.field_data(grid.shape, seed=11))
    with pytest.raises(pde.grids.base.DomainError, match="Point lies outside the grid domain"):
        field.make_interpolator(backend="hip")(np.array([[0.0, 9.0]]))
    with pytest.raises(pde.grids.base.DimensionError):
        field.make_interpolator(backend="hip")(np.zeros((4, 3)))
    full = IC.field_data((7, 8), seed=12)
    near_walls = wall_points(mirror)
    same(field.make_interpolator(backend="hip", with_ghost_cells=True)(near_walls, full),
         IC.interpolate(mirror, full, near_walls, with_ghost_cells=True))


def test_plugin_regridding_of_pypde_fields(pde, shim, golden):
    grid = pde.CartesianGrid(BOUNDS[:2], (5, 6), periodic=[True, False])
    mirror = pde_hip.CartesianGrid(BOUNDS[:2], (5, 6), periodic=[True, False])
    target = pde.CartesianGrid(BOUNDS[:2], (9, 11), periodic=[True, False])
    for cls, rank in ((pde.ScalarField, 0), (pde.VectorField, 1)):
        data = IC.field_data(grid.shape, (2,) * rank, seed=21 + rank)
        res = pde_hip.interpolate_to_grid(cls(grid, data), target, label="fine")
        assert type(res) is cls and res.grid is target and res.label == "fine"
        same(res.data, IC.interpolate(mirror, data, target.cell_coords))
    # conditions of py-pde's own BoundariesList, edges and corners included: the reference's full array is the golden
    cid, shape, periodic, bc = IC.GOLDEN_CASES[6]                       # 3d-mixed
    src = pde.CartesianGrid(IC.GOLDEN_BOUNDS[3], shape, periodic=list(periodic))
    src_mirror = pde_hip.CartesianGrid(IC.GOLDEN_BOUNDS[3], shape, periodic=list(periodic))
    dst = pde.CartesianGrid(IC.GOLDEN_BOUNDS[3], (5, 7, 9))
    field = pde.ScalarField(src, golden[cid + "/valid"])
    same(pde_hip.interpolate_to_grid(field, dst, bc=bc).data,
         IC.interpolate(src_mirror, golden[cid + "/full"], dst.cell_coords, with_ghost_cells=True))
    larger = pde.CartesianGrid([(-0.5, 2.0), (-1.0, 1.0), (2.0, 5.0)], (5, 4, 6))
    same(pde_hip.interpolate_to_grid(field, larger, fill=-1.0).data, IC.interpolate(src_mirror, field.data, larger.cell_coords, fill=-1.0))
    with pytest.raises(pde.grids.base.DomainError):
        pde_hip.interpolate_to_grid(field, larger)
    with pytest.raises(NotImplementedError, match="Cartesian grids only"):
        pde_hip.interpolate_to_grid(field, pde.SphericalSymGrid(2.0, 8))
    with pytest.raises(pde.grids.base.DimensionError):
        pde_hip.interpolate_to_grid(field, target)


def test_plugin_reads_a_resident_state_where_it_is(pde, shim, rng, monkeypatch):
    """After ``eq.solve(..., backend="hip")`` of py-pde the result is resident: interpolation reads the device copy, nothing is pulled,
    and the regridded field has py-pde's own class, not the intercepting subclass."""
    from pde_hip.resident import ResidentState

    grid = pde.UnitGrid([8, 6], periodic=[True, False])
    state = pde.ScalarField(grid, rng.uniform(0, 1, grid.shape))
    res = pde.DiffusionPDE().solve(state, t_range=0.2, dt=0.05, backend="hip", solver="euler", tracker=None)
    link = res.__dict__["_hip_link"]
    assert link.host_stale and link.downloads == 0
    points = rng.uniform(0, 1, (40, 2)) * np.array(grid.shape)
    with monkeypatch.context() as m:
        m.setattr(ResidentState, "pull", lambda self, field=None: pytest.fail("the resident state was pulled"))
        got = res.make_interpolator(backend="hip")(points)
        same_grid = pde_hip.interpolate_to_grid(res, pde.UnitGrid([8, 6], periodic=[True, False]))
    assert link.downloads == 0 and type(same_grid) is pde.ScalarField
    advanced = np.array(res.data)
    mirror = pde_hip.UnitGrid([8, 6], periodic=[True, False])
    same(got, IC.interpolate(mirror, advanced, points))
    same(same_grid.data, advanced)
