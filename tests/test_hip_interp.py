"""Interpolation on the device against the restatement of the reference (tests/interp_cases.py), bit for bit: the default build
evaluates the same fp64 expressions in the same order, so every comparison is ``np.array_equal`` - a tolerance would hide a wrong branch."""

from __future__ import annotations

import itertools

import numpy as np
import pytest

import interp_cases as IC
import pde_hip
from helpers import GOLDEN
from pde_hip.interpolation import error_classes

pytestmark = pytest.mark.gpu

FIELDS = {0: pde_hip.ScalarField, 1: pde_hip.VectorField, 2: pde_hip.Tensor2Field}
BOUNDS = [(-1.0, 2.0), (0.5, 3.0), (0.0, 1.0)]


def make_field(grid, data):
    return FIELDS[data.ndim - grid.num_axes](grid, data)


def same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    np.testing.assert_array_equal(a, b)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "interp.npz", allow_pickle=False)


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("ndim", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_branches_of_every_axis(n, ndim, periodic):
    """Walls, half a cell inside, cell centres, one ulp either side of each (one ulp below ``lo + dx/2`` is the quotient the ``divmod``
    fix-up turns into (-1.0, 1.0)) and ``lo - 1e-17 dx``; along one axis at a time while the other axes cycle through the same marks."""
    grid = pde_hip.CartesianGrid(BOUNDS[:ndim], (n,) * ndim, periodic=periodic)
    data = IC.field_data(grid.shape, seed=n)
    marks = [IC.axis_probe_coords(*BOUNDS[a], n) for a in range(ndim)]
    points = []
    for a in range(ndim):
        for i, c in enumerate(marks[a]):
            p = [marks[b][(7 * i + 3 * b) % len(marks[b])] for b in range(ndim)]
            p[a] = c
            points.append(p)
    points = np.array(points)
    for ghost in (False, True):
        src = IC.field_data(tuple(s + 2 for s in grid.shape), seed=n + 1) if ghost else data
        interp = make_field(grid, data).make_interpolator(fill=-7.0, with_ghost_cells=ghost)
        same(interp(points, src), IC.interpolate(grid, src, points, fill=-7.0, with_ghost_cells=ghost))


def test_small_weights_are_dropped():
    """1e-15 itself is no attainable weight (the quotient minus 0.5 is a multiple of 2**-54 there); the two neighbours of 1e-15 are:
    9 * 2**-53 < 1e-15 must become exactly 0 - the 1e300 in that cell leaves no trace -, 10 * 2**-53 stays."""
    grid = pde_hip.UnitGrid([4])
    data = np.array([3.0, 1e300, 5.0, 7.0])
    points = np.array([[0.5 + 9 * 2.0**-53], [0.5 + 10 * 2.0**-53], [1.5 - 4 * 2.0**-52], [1.5 - 5 * 2.0**-52]])
    assert [IC.axis_data(4, False, 0.0, 1.0, float(p))[3] for p in points[:2, 0]] == [0, 10 * 2.0**-53]
    expect = IC.interpolate(grid, data, points)
    assert expect[0] == (1 - 9 * 2.0**-53) * 3.0 and expect[1] > 1e284
    same(pde_hip.ScalarField(grid, data).make_interpolator()(points), expect)
    data2 = np.array([1e300, 3.0, 5.0, 7.0])           # ... and the weight of the LEFT cell
    expect2 = IC.interpolate(grid, data2, points)
    assert expect2[2] == (1 - 2.0**-50) * 3.0 and expect2[3] > 1e284      # w_l = 8 * 2**-53 dropped, 10 * 2**-53 kept
    same(pde_hip.ScalarField(grid, data2).make_interpolator()(points), expect2)


@pytest.mark.parametrize("rank", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.complex128])
@pytest.mark.parametrize("shape", [(3, 4), (3, 4, 5)])
def test_dtypes_and_ranks(shape, dtype, rank, rng):
    nd = len(shape)
    grid = pde_hip.CartesianGrid(BOUNDS[:nd], shape, periodic=[False, True, False][:nd])
    data = IC.field_data(shape, (nd,) * rank, dtype, seed=rank)
    lo, hi = np.array(BOUNDS[:nd]).T
    points = lo + (hi - lo) * rng.uniform(0, 1, (40, nd))
    got = make_field(grid, data).make_interpolator()(points)
    same(got, IC.interpolate(grid, data, points))
    assert got.shape == (nd,) * rank + (40,) and got.dtype == np.dtype(dtype)


def wall_points(grid):
    """Points within half a cell of one, two and three walls (and a few inside)."""
    per_axis = []
    for (lo, hi), dx in zip(grid.axes_bounds, grid.discretization):
        per_axis.append([lo, lo + 0.1 * dx, lo + 0.5 * dx, 0.5 * (lo + hi), hi - 0.3 * dx, hi])
    return np.array(list(itertools.product(*per_axis)))


@pytest.mark.parametrize("cid,shape,periodic,bc", IC.GOLDEN_CASES, ids=[c[0] for c in IC.GOLDEN_CASES])
def test_ghost_cells_with_edges_and_corners(golden, cid, shape, periodic, bc):
    nd = len(shape)
    grid = pde_hip.CartesianGrid(IC.GOLDEN_BOUNDS[nd], shape, periodic=list(periodic))
    full, valid = golden[cid + "/full"], golden[cid + "/valid"]
    points = wall_points(grid)
    expect = IC.interpolate(grid, full, points, with_ghost_cells=True)
    field = pde_hip.ScalarField(grid, valid)
    # (a) the reference's full array uploaded: edges and corners carry weight next to two and three walls
    same(field.make_interpolator(with_ghost_cells=True)(points, full), expect)
    # (b) the device fills them itself: the full array equals the reference's, and so do the values
    field.set_ghost_cells(bc, set_corners=True)
    np.testing.assert_array_equal(field._data_full, full)
    same(pde_hip.ScalarField(grid, valid).interpolate(points, bc=bc), expect)
    # the default call of the ghost path leaves edges and corners alone
    plain = pde_hip.ScalarField(grid, valid)
    plain._data_full[(0,) * nd] = 123.0
    plain.set_ghost_cells(bc)
    assert plain._data_full[(0,) * nd] == 123.0


def test_fill_and_domain_error(rng):
    grid = pde_hip.CartesianGrid(BOUNDS[:2], (3, 4))
    dom = error_classes()[0]
    inside = np.array([[0.0, 1.0], [1.5, 2.5], [-1.0, 0.5]])
    outside = np.array([[2.5, 1.0], [0.0, 3.5]])
    vec = IC.field_data(grid.shape, (2,), seed=3)
    field = pde_hip.VectorField(grid, vec)
    mixed = np.concatenate([inside, outside])
    same(field.make_interpolator(fill=0.5)(mixed), IC.interpolate(grid, vec, mixed, fill=0.5))
    same(field.make_interpolator(fill=[1.0, -2.0])(mixed), IC.interpolate(grid, vec, mixed, fill=[1.0, -2.0]))
    cplx = IC.field_data(grid.shape, (), np.complex128, seed=4)
    same(pde_hip.ScalarField(grid, cplx).make_interpolator(fill=1 - 2j)(mixed), IC.interpolate(grid, cplx, mixed, fill=1 - 2j))
    interp = field.make_interpolator()
    same(interp(inside), IC.interpolate(grid, vec, inside))              # 0 points outside: no error
    for points in (np.concatenate([inside, outside[:1]]), outside):      # 1 point, all points
        with pytest.raises(dom, match="Point lies outside the grid domain"):
            interp(points)
    with pytest.raises(dom):
        field.make_interpolator(with_ghost_cells=True)(np.array([[-1.0 - 1e-9, 1.0]]), IC.field_data((5, 6), (2,)))
    same(field.interpolate(mixed, fill=3.0), IC.interpolate(grid, vec, mixed, fill=3.0))


def test_launch_geometry(rng):
    """Point shapes, counts around one block, one count above a single grid-stride pass (2048 blocks of 256 threads) and rows of the
    source that are longer than a 128-byte line and off the line grid."""
    grid = pde_hip.CartesianGrid(BOUNDS, (2, 3, 130), periodic=[True, False, False])
    data = IC.field_data(grid.shape, seed=5)
    interp = pde_hip.ScalarField(grid, data).make_interpolator()
    lo, hi = np.array(BOUNDS).T
    base = lo + (hi - lo) * rng.uniform(0, 1, (600, 3))
    expect = IC.interpolate(grid, data, base)
    same(interp(base[0]), expect[0])
    assert interp(base[0]).shape == ()
    same(interp(base[:1]), expect[:1])
    same(interp(base[:21].reshape(7, 3, 3)), expect[:21].reshape(7, 3))
    for count in (255, 256, 257):
        same(interp(base[:count]), expect[:count])
    count = 2048 * 256 + 3
    reps = -(-count // 600)
    same(interp(np.tile(base, (reps, 1))[:count]), np.tile(expect, reps)[:count])
    assert interp(np.zeros((0, 3))).shape == (0,)


REGRID = [((4, 6, 10), (8, 12, 20)), ((4, 6, 10), (3, 5, 7)), ((4, 6, 10), (9, 13, 21)), ((6, 10), (9, 25)), ((10,), (23,)), ((10,), (1500,))]


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("src_shape,dst_shape", REGRID)
def test_regridding(src_shape, dst_shape, periodic):
    nd = len(src_shape)
    src = pde_hip.CartesianGrid(BOUNDS[:nd], src_shape, periodic=periodic)
    dst = pde_hip.CartesianGrid(BOUNDS[:nd], dst_shape, periodic=periodic)
    for rank, dtype in ((0, np.float64), (1, np.float32), (0, np.complex128)):
        data = IC.field_data(src_shape, (nd,) * rank, dtype, seed=nd)
        field = make_field(src, data)
        res = field.interpolate_to_grid(dst, label="fine")
        assert type(res) is type(field) and res.grid is dst and res.label == "fine"
        same(res.data, IC.interpolate(src, data, dst.cell_coords))
        same(res.data, field.make_interpolator()(dst.cell_coords))
        same(pde_hip.interpolate_to_grid(field, dst).data, res.data)


def test_regridding_with_conditions_fill_and_a_larger_target(golden):
    cid, shape, periodic, bc = IC.GOLDEN_CASES[6]                       # 3d-mixed
    src = pde_hip.CartesianGrid(IC.GOLDEN_BOUNDS[3], shape, periodic=list(periodic))
    dst = pde_hip.CartesianGrid(IC.GOLDEN_BOUNDS[3], (5, 7, 9))
    field = pde_hip.ScalarField(src, golden[cid + "/valid"])
    same(field.interpolate_to_grid(dst, bc=bc).data, IC.interpolate(src, golden[cid + "/full"], dst.cell_coords, with_ghost_cells=True))
    larger = pde_hip.CartesianGrid([(-0.5, 2.0), (-1.0, 1.0), (2.0, 5.0)], (5, 4, 6))
    same(field.interpolate_to_grid(larger, fill=-1.0).data, IC.interpolate(src, field.data, larger.cell_coords, fill=-1.0))
    with pytest.raises(error_classes()[0], match="Point lies outside the grid domain"):
        field.interpolate_to_grid(larger)
    # 2-D with walls and conditions
    cid, shape, periodic, bc = IC.GOLDEN_CASES[2]
    src2 = pde_hip.CartesianGrid(IC.GOLDEN_BOUNDS[2], shape, periodic=list(periodic))
    dst2 = pde_hip.CartesianGrid(IC.GOLDEN_BOUNDS[2], (7, 5))
    same(pde_hip.ScalarField(src2, golden[cid + "/valid"]).interpolate_to_grid(dst2, bc=bc).data,
         IC.interpolate(src2, golden[cid + "/full"], dst2.cell_coords, with_ghost_cells=True))


def test_resident_state_is_read_on_the_device(rng, monkeypatch):
    from pde_hip.resident import ResidentState

    grid = pde_hip.UnitGrid([16, 12, 20], periodic=[True, False, True])
    res = pde_hip.DiffusionPDE().solve(pde_hip.ScalarField(grid, rng.uniform(0, 1, grid.shape)), t_range=0.5, dt=0.05, backend="hip")
    link = res.__dict__["_hip_link"]
    assert link.host_stale and link.downloads == 0
    points = rng.uniform(0, 1, (300, 3)) * np.array(grid.shape)

    def no_pull(self, field=None):
        raise AssertionError("the resident state was pulled")

    with monkeypatch.context() as m:
        m.setattr(ResidentState, "pull", no_pull)
        got = res.make_interpolator()(points)
        fine = res.interpolate_to_grid(pde_hip.UnitGrid([16, 12, 20], periodic=[True, False, True]))
    assert link.downloads == 0 and link.host_stale
    advanced = np.array(res.data)                                      # now the download
    assert link.downloads == 1
    same(got, IC.interpolate(grid, advanced, points))
    same(fine.data, advanced)                                          # the same grid: every weight is 1 or 0


def test_conditions_on_a_resident_state(rng, monkeypatch):
    """``interpolate(bc=...)`` and ``interpolate_to_grid(bc=...)`` set the ghost cells, edges and corners included, in the device copy of
    a resident state: nothing is pulled, the values are those of the advanced state with these conditions, and the run goes on from the
    same state as if nobody had looked (every sweep sets the ghost cells it reads)."""
    from pde_hip.resident import ResidentState

    grid = pde_hip.CartesianGrid(IC.GOLDEN_BOUNDS[3], (6, 4, 5))
    bc = IC.GOLDEN_CASES[6][3]                                        # 3d-mixed
    start = pde_hip.ScalarField(grid, rng.uniform(0, 1, grid.shape))
    eq = pde_hip.DiffusionPDE(0.1)
    res = eq.solve(start, t_range=0.02, dt=0.002, backend="hip")
    assert res.__dict__["_hip_link"].host_stale
    points = wall_points(grid)
    dst = pde_hip.CartesianGrid(IC.GOLDEN_BOUNDS[3], (7, 9, 11))
    with monkeypatch.context() as m:
        m.setattr(ResidentState, "pull", lambda self, field=None: pytest.fail("the resident state was pulled"))
        got = res.interpolate(points, bc=bc)
        fine = res.interpolate_to_grid(dst, bc=bc)
    again = eq.solve(res, t_range=0.02, dt=0.002, backend="hip")
    untouched = eq.solve(eq.solve(start, t_range=0.02, dt=0.002, backend="hip"), t_range=0.02, dt=0.002, backend="hip")
    same(np.array(again.data), np.array(untouched.data))
    host = pde_hip.ScalarField(grid, np.array(res.data))
    host.set_ghost_cells(bc, set_corners=True)
    same(got, IC.interpolate(grid, host._data_full, points, with_ghost_cells=True))
    same(fine.data, IC.interpolate(grid, host._data_full, dst.cell_coords, with_ghost_cells=True))


def test_two_runs_give_equal_bits(rng):
    grid = pde_hip.CartesianGrid(BOUNDS, (5, 6, 7))
    data = IC.field_data(grid.shape, (3,), seed=9)
    lo, hi = np.array(BOUNDS).T
    points = lo + (hi - lo) * rng.uniform(-0.05, 1.05, (5000, 3))
    field = pde_hip.VectorField(grid, data)
    a, b = field.make_interpolator(fill=0.0)(points), field.make_interpolator(fill=0.0)(points)
    assert a.tobytes() == b.tobytes()
    dst = pde_hip.CartesianGrid(BOUNDS, (11, 9, 16))
    assert field.interpolate_to_grid(dst).data.tobytes() == field.interpolate_to_grid(dst).data.tobytes()
