"""The yardstick of the interpolation tests: a plain-Python restatement of the reference's two functions, and the case tables.

``axis_data`` is ``make_interpolation_axis_data`` (pde/backends/numba/grids.py:102-190) and ``interpolate_single`` is
``make_single_interpolator`` (pde/backends/numba/grids.py:193-347), transcribed line by line with the builtin ``divmod`` on Python floats.
The reference's own code needs numba to run.  One thing numba does implicitly is written out: a float64 weight times an array element
unifies to float64 (complex128 for complex data), so the data is promoted before the sum and the result is rounded once when it is stored
into the output array of the data's dtype (numba/backend.py:979-981).  ``set_corners`` is the tail of
``BoundariesList.set_ghost_cells(..., set_corners=True)`` (pde/grids/boundaries/axes.py:475-495); tests/golden/interp.npz pins it on the
reference's own output.
"""

from __future__ import annotations

import itertools

import numpy as np


class DomainError(ValueError):
    """Stand-in of ``pde.grids.base.DomainError`` for the restatement."""


def axis_data(size: int, periodic: bool, lo: float, dx: float, coord: float, with_ghost_cells: bool = False):
    """grids.py:136-188 (``cell_coords=False``)."""
    c_l, d_l = divmod((coord - lo) / dx - 0.5, 1.0)
    if periodic:
        c_li = int(c_l) % size
        c_hi = (c_li + 1) % size
    elif with_ghost_cells:
        if -0.5 <= c_l + d_l <= size - 0.5:
            c_li = int(c_l)
            c_hi = c_li + 1
        else:
            return -42, -42, 0.0, 0.0
    else:
        if 0 <= c_l + d_l < size - 1:
            c_li = int(c_l)
            c_hi = c_li + 1
        elif size - 1 <= c_l + d_l <= size - 0.5:
            c_li = c_hi = int(c_l)
        elif -0.5 <= c_l + d_l <= 0:
            c_li = c_hi = int(c_l) + 1
        else:
            return -42, -42, 0.0, 0.0
    w_l, w_h = 1 - d_l, d_l
    if w_l < 1e-15:
        w_l = 0
    if w_h < 1e-15:
        w_h = 0
    if with_ghost_cells:
        c_li += 1
        c_hi += 1
    return c_li, c_hi, w_l, w_h


def interpolate_single(grid, data: np.ndarray, point, fill=None, with_ghost_cells: bool = False):
    """grids.py:230-347; ``data`` already promoted (see the module docstring)."""
    axes = [axis_data(int(grid.shape[a]), bool(grid.periodic[a]), float(grid.axes_bounds[a][0]), float(grid.discretization[a]), float(point[a]),
                      with_ghost_cells) for a in range(grid.num_axes)]
    if any(a[0] == -42 for a in axes):
        if fill is None:
            raise DomainError("Point lies outside the grid domain")
        return fill
    if grid.num_axes == 1:
        ((c_li, c_hi, w_l, w_h),) = axes
        return w_l * data[..., c_li] + w_h * data[..., c_hi]
    if grid.num_axes == 2:
        (c_xli, c_xhi, w_xl, w_xh), (c_yli, c_yhi, w_yl, w_yh) = axes
        return (
            w_xl * w_yl * data[..., c_xli, c_yli]
            + w_xl * w_yh * data[..., c_xli, c_yhi]
            + w_xh * w_yl * data[..., c_xhi, c_yli]
            + w_xh * w_yh * data[..., c_xhi, c_yhi]
        )
    (c_xli, c_xhi, w_xl, w_xh), (c_yli, c_yhi, w_yl, w_yh), (c_zli, c_zhi, w_zl, w_zh) = axes
    return (
        w_xl * w_yl * w_zl * data[..., c_xli, c_yli, c_zli]
        + w_xl * w_yl * w_zh * data[..., c_xli, c_yli, c_zhi]
        + w_xl * w_yh * w_zl * data[..., c_xli, c_yhi, c_zli]
        + w_xl * w_yh * w_zh * data[..., c_xli, c_yhi, c_zhi]
        + w_xh * w_yl * w_zl * data[..., c_xhi, c_yli, c_zli]
        + w_xh * w_yl * w_zh * data[..., c_xhi, c_yli, c_zhi]
        + w_xh * w_yh * w_zl * data[..., c_xhi, c_yhi, c_zli]
        + w_xh * w_yh * w_zh * data[..., c_xhi, c_yhi, c_zhi]
    )


def interpolate(grid, data: np.ndarray, points, fill=None, with_ghost_cells: bool = False) -> np.ndarray:
    """The interpolator of numba/backend.py:948-983: ``data_shape + point_shape`` in the data's dtype."""
    data = np.asarray(data)
    points = np.atleast_1d(np.asarray(points, dtype=np.float64))
    assert points.shape[-1] == grid.num_axes
    point_shape = points.shape[:-1]
    data_shape = data.shape[: data.ndim - grid.num_axes]
    if fill is not None:      # numba/backend.py:927-932
        fill = data.dtype.type(fill) if not data_shape else np.broadcast_to(fill, data_shape).astype(data.dtype)
    wide = data.astype(np.result_type(data.dtype, np.float64))
    out = np.empty(data_shape + point_shape, dtype=data.dtype)
    with np.errstate(all="ignore"):
        for idx in np.ndindex(*point_shape):
            out[(..., *idx)] = interpolate_single(grid, wide, [float(c) for c in points[idx]], fill, with_ghost_cells)
    return out


def set_corners(d: np.ndarray, num_axes: int) -> None:
    """axes.py:475-495, in place on a full array whose face ghost cells are set."""
    nxt = [1, -2]
    if num_axes == 2:
        for i, j in itertools.product([0, -1], [0, -1]):
            d[..., i, j] = (d[..., nxt[i], j] + d[..., i, nxt[j]]) / 2
    elif num_axes == 3:
        for i, j in itertools.product([0, -1], [0, -1]):
            d[..., :, i, j] = (+d[..., :, nxt[i], j] + d[..., :, i, nxt[j]]) / 2
            d[..., i, :, j] = (+d[..., nxt[i], :, j] + d[..., i, :, nxt[j]]) / 2
            d[..., i, j, :] = (+d[..., nxt[i], j, :] + d[..., i, nxt[j], :]) / 2
        for i, j, k in itertools.product(*[[0, -1]] * 3):
            d[..., i, j, k] = (d[..., nxt[i], j, k] + d[..., i, nxt[j], k] + d[..., i, j, nxt[k]]) / 3


# ---- case tables ------------------------------------------------------------------------------------------------------------------
# the golden of tests/golden/interp.npz: (id, shape, periodic, bc per axis)
GOLDEN_CASES = [
    ("2d-dirichlet", (3, 4), (False, False), [{"value": 1.5}, {"value": -0.5}]),
    ("2d-neumann", (3, 4), (False, False), [{"derivative": 0.5}, {"derivative": -1.0}]),
    ("2d-mixed", (3, 4), (False, False), [{"type": "mixed", "value": 2.0, "const": 1.0}, {"value": 0.25}]),
    ("2d-periodic-x", (3, 4), (True, False), ["periodic", {"derivative": 0.75}]),
    ("3d-dirichlet", (3, 4, 5), (False, False, False), [{"value": 1.5}, {"value": -0.5}, {"value": 0.125}]),
    ("3d-neumann", (3, 4, 5), (False, False, False), [{"derivative": 0.5}, {"derivative": -1.0}, {"derivative": 2.0}]),
    ("3d-mixed", (3, 4, 5), (False, False, False), [{"type": "mixed", "value": 2.0, "const": 1.0}, {"value": 0.25}, {"derivative": 0.5}]),
    ("3d-periodic-y", (3, 4, 5), (False, True, False), [{"value": 1.0}, "periodic", {"derivative": -0.5}]),
]
GOLDEN_BOUNDS = {2: [(0.0, 1.5), (-1.0, 1.0)], 3: [(0.0, 1.5), (-1.0, 1.0), (2.0, 4.5)]}


def axis_probe_coords(lo: float, hi: float, n: int) -> list[float]:
    """The coordinates at which the branches of one axis change: the walls, half a cell inside, the cell centres, one ulp either side of
    each, and ``lo - 1e-17 dx`` (the quotient the float ``divmod`` fix-up turns into (-1.0, 1.0))."""
    dx = (hi - lo) / n
    marks = [lo, lo + dx / 2, hi - dx / 2, hi] + [lo + (i + 0.5) * dx for i in range(n)]
    out = []
    for m in marks:
        out += [float(np.nextafter(m, -np.inf)), float(m), float(np.nextafter(m, np.inf))]
    out.append(lo - 1e-17 * dx)
    return out


def field_data(shape, lead=(), dtype=np.float64, seed=0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    data = rng.uniform(-1, 1, size=tuple(lead) + tuple(shape))
    if np.dtype(dtype).kind == "c":
        data = data + 1j * rng.uniform(-1, 1, size=data.shape)
    return data.astype(dtype)
