"""CPU checks of the interpolation yardstick (tests/interp_cases.py) and of the argument checking that needs no device."""

from __future__ import annotations

import numpy as np
import pytest

import interp_cases as IC
import pde_hip
from helpers import GOLDEN


@pytest.mark.parametrize("cid,shape,periodic,bc", IC.GOLDEN_CASES, ids=[c[0] for c in IC.GOLDEN_CASES])
def test_restated_corners_match_the_reference_golden(cid, shape, periodic, bc):
    """The golden holds the reference's own ``set_ghost_cells(set_corners=True)`` output; from its face ghost cells the restatement must
    rebuild every edge and corner cell, bit for bit."""
    npz = np.load(GOLDEN / "interp.npz", allow_pickle=False)
    full = npz[cid + "/full"]
    nd = len(shape)
    assert full.shape == tuple(n + 2 for n in shape)
    np.testing.assert_array_equal(full[(slice(1, -1),) * nd], npz[cid + "/valid"])
    idx = np.indices(full.shape)
    n_ghost = sum(((idx[a] == 0) | (idx[a] == full.shape[a] - 1)).astype(int) for a in range(nd))
    work = np.where(n_ghost >= 2, np.nan, full)
    IC.set_corners(work, nd)
    np.testing.assert_array_equal(work, full)
    assert np.isfinite(full).all()


@pytest.mark.parametrize("shape", [(7,), (5, 6), (4, 5, 6)])
def test_restatement_matches_scipy_on_interior_points(shape, rng):
    from scipy.interpolate import RegularGridInterpolator

    bounds = [(-1.0, 2.0), (0.5, 3.0), (0.0, 1.0)][: len(shape)]
    grid = pde_hip.CartesianGrid(bounds, shape)
    data = rng.uniform(-1, 1, shape)
    lo = np.array([c[0] for c in grid.axes_coords])
    hi = np.array([c[-1] for c in grid.axes_coords])
    points = lo + (hi - lo) * rng.uniform(0, 1, (200, len(shape)))
    expect = RegularGridInterpolator(grid.axes_coords, data, method="linear")(points)
    got = IC.interpolate(grid, data, points)
    assert np.abs(got - expect).max() <= 1e-13 * np.abs(expect).max()


def test_one_sided_and_periodic_branches_by_hand():
    # UnitGrid of 4 cells: centres 0.5, 1.5, 2.5, 3.5
    data = np.array([1.0, 2.0, 4.0, 8.0])
    wall = pde_hip.UnitGrid([4])
    assert IC.axis_data(4, False, 0.0, 1.0, 0.25) == (0, 0, 0.25, 0.75)          # close to the lower wall: both support points cell 0
    assert IC.axis_data(4, False, 0.0, 1.0, 3.75) == (3, 3, 0.75, 0.25)          # close to the upper wall
    assert IC.axis_data(4, False, 0.0, 1.0, 1.75) == (1, 2, 0.75, 0.25)          # bulk
    assert IC.axis_data(4, False, 0.0, 1.0, 4.0 + 1e-9)[0] == -42 and IC.axis_data(4, False, 0.0, 1.0, -1e-9)[0] == -42
    assert IC.axis_data(4, True, 0.0, 1.0, 3.75) == (3, 0, 0.75, 0.25)           # periodic: wraps
    assert IC.axis_data(4, True, 0.0, 1.0, -0.25) == (3, 0, 0.75, 0.25)          # 0.25 to the right of centre -0.5 = cell 3
    assert IC.axis_data(4, True, 0.0, 1.0, 9.0) == (0, 1, 0.5, 0.5)
    assert IC.axis_data(4, False, 0.0, 1.0, 0.25, True) == (0, 1, 0.25, 0.75)    # ghost cells: the bulk rule, shifted by one
    assert IC.axis_data(4, False, 0.0, 1.0, -1e-9, True)[0] == -42
    # the fix-up of the float divmod: a tiny negative quotient is (-1.0, 1.0), not (-1.0, 1 - 1e-17)
    assert divmod(-1e-17, 1.0) == (-1.0, 1.0)
    assert IC.axis_data(4, False, 0.0, 1.0, 0.5 - 1e-17) == IC.axis_data(4, False, 0.0, 1.0, 0.5)        # (0.5 - 1e-17 rounds to 0.5)
    below = float(np.nextafter(0.5, 0.0))                                        # quotient -2**-54: (-1.0, 1.0) after the fix-up
    assert divmod(below - 0.5, 1.0) == (-1.0, 1.0)
    assert IC.axis_data(4, False, 0.0, 1.0, below) == (-1, 0, 0, 1.0)           # data[..., -1], the last cell, with weight 0
    np.testing.assert_array_equal(IC.interpolate(wall, data, [[0.25], [1.75], [3.75], [4.0]]), [1.0, 0.75 * 2 + 0.25 * 4, 8.0, 8.0])
    np.testing.assert_array_equal(IC.interpolate(pde_hip.UnitGrid([4], periodic=True), data, [[3.75], [-0.25]]), [0.75 * 8 + 0.25 * 1, 0.75 * 8 + 0.25 * 1])
    with pytest.raises(IC.DomainError):
        IC.interpolate(wall, data, [[4.5]])
    np.testing.assert_array_equal(IC.interpolate(wall, data, [[4.5]], fill=-3), [-3.0])
    # fp32 data: fp64 weights and sum, one rounding at the store
    d32 = np.array([0.1, 0.7, 0.3, 0.9], np.float32)
    got = IC.interpolate(wall, d32, [[1.3]])
    assert got.dtype == np.float32 and got[0] == np.float32(0.2 * np.float64(d32[0]) + 0.8 * np.float64(d32[1]))


def test_make_interpolator_checks_its_arguments_without_a_device():
    from pde_hip.interpolation import DimensionError, DomainError, _convert_fill, error_classes

    grid = pde_hip.UnitGrid([4, 5])
    field = pde_hip.VectorField(grid, 1.0)
    interp = field.make_interpolator(fill=[1, 2])
    with pytest.raises(ValueError, match="Dimension of point does not match axes count 2"):
        interp(np.zeros((3, 3)))
    with pytest.raises(ValueError):                       # a fill that does not broadcast to the data shape
        field.make_interpolator(fill=[1, 2, 3])
    dom, dim = error_classes()
    assert issubclass(dom, ValueError) and issubclass(dim, ValueError)
    assert dom.__name__ == "DomainError" and dim.__name__ == "DimensionError"
    assert issubclass(DomainError, ValueError) and issubclass(DimensionError, ValueError)
    np.testing.assert_array_equal(_convert_fill(1 + 2j, (), np.dtype(np.complex128)), [1.0, 2.0])
    np.testing.assert_array_equal(_convert_fill([1, 2], (2,), np.dtype(np.float32)), [1.0, 2.0])
    assert _convert_fill(None, (), np.dtype(np.float64)) is None

    class PolarSymGrid:                                   # anything that is not Cartesian is refused before a device is needed
        shape, dim, num_axes, periodic, discretization, axes_bounds = (4,), 2, 1, [False], np.array([1.0]), ((0.0, 4.0),)

    class Probe:
        grid, rank, dtype = PolarSymGrid(), 0, np.dtype(np.float64)

    with pytest.raises(NotImplementedError, match="Cartesian"):
        pde_hip.get_backend("hip").make_interpolator(Probe())
    with pytest.raises(NotImplementedError, match="Cartesian"):
        pde_hip.get_backend("hip").interpolate_to_grid(pde_hip.ScalarField(grid, 1.0), PolarSymGrid())
    with pytest.raises(ValueError, match="Incompatible grid dimensions"):
        pde_hip.interpolate_to_grid(pde_hip.ScalarField(grid, 1.0), pde_hip.UnitGrid([4]))
    assert callable(pde_hip.interpolate_to_grid)
