"""Linear interpolation of fields on the device: ``make_interpolator`` of the backend (``pde/backends/base.py:606-632``, numba twin
``pde/backends/numba/backend.py:895-988``) and regridding onto another Cartesian grid (``pde/fields/scalar.py:468``) -
:class:`InterpolationMixin` and :func:`interpolate_to_grid`.

The kernels (``csrc/pdehip_interp.hip``) restate ``pde/backends/numba/grids.py:102-347`` operation by operation.  A field whose state is
resident on the device (:class:`~pde_hip.resident.ResidentState`) is read where it is: the points go up, ``npoints x ncomp`` values and one
8-byte counter of the points outside the domain come down.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .device import DeviceArray, DeviceBuffer
from .faces import real_dtype_of
from .resident import base_class, field_dtype, valid_link


class DomainError(ValueError):
    """A point lies outside the grid domain (``pde.grids.base.DomainError``; raised when py-pde is absent)."""


class DimensionError(ValueError):
    """Dimensions do not match (``pde.grids.base.DimensionError``; raised when py-pde is absent)."""


def error_classes() -> tuple[type, type]:
    """(DomainError, DimensionError): py-pde's own classes where py-pde is present, else the two above."""
    try:
        from pde.grids.base import DimensionError as dim_err
        from pde.grids.base import DomainError as dom_err
    except ImportError:
        return DomainError, DimensionError
    return dom_err, dim_err


_OOB_MESSAGE = "Point lies outside the grid domain"      # pde/backends/numba/grids.py:254


def _is_cartesian(grid) -> bool:
    """A CartesianGrid (or a subclass of it, UnitGrid among them) of this package's mirror or of py-pde."""
    from .grids import CartesianGrid

    if isinstance(grid, CartesianGrid):
        return True
    if type(grid).__module__.split(".")[0] != "pde":
        return False
    from pde.grids.cartesian import CartesianGrid as PdeCartesianGrid

    return isinstance(grid, PdeCartesianGrid)


def _require_cartesian(grid, what: str = "interpolation") -> None:
    """Cartesian grids of 1 to 3 axes (curvilinear grids are refused)."""
    if not _is_cartesian(grid):
        msg = f"hip backend: {what} supports Cartesian grids only (got {grid.__class__.__name__})"
        raise NotImplementedError(msg)
    if not 1 <= len(grid.shape) <= _abi.MAX_DIM:
        msg = f"Compiled interpolation not implemented for dimension {len(grid.shape)}"      # grids.py:346
        raise NotImplementedError(msg)


def _convert_fill(fill, data_shape: tuple[int, ...], dtype: np.dtype):
    """``fill`` in the type of the data (numba/backend.py:927-932) as the planar fp64 components the kernels store, or None."""
    if fill is None:
        return None
    if not data_shape:
        value = np.asarray(dtype.type(fill))
    else:
        value = np.broadcast_to(fill, data_shape).astype(dtype)
    if dtype.kind == "c":
        value = np.stack([value.real, value.imag], axis=-1)
    return np.ascontiguousarray(value, dtype=np.float64).ravel()


class _Source:
    """Geometry of the grid a field lives on, in the form the C entry points take."""

    def __init__(self, grid):
        nd = len(grid.shape)
        self.periodic = (C.c_int * nd)(*[int(bool(p)) for p in grid.periodic])
        self.lo = (C.c_double * nd)(*[float(grid.axes_bounds[a][0]) for a in range(nd)])


def _planar(host: np.ndarray, lead: int) -> np.ndarray:
    """Complex host data as planar pairs: (real part, imaginary part) on a new axis behind the ``lead`` tensor axes."""
    return np.stack([host.real, host.imag], axis=lead)


class InterpolationMixin:
    """``make_interpolator`` of :class:`~pde_hip.backend.HipBackendMixin`."""

    def _to_interp_source(self, grid, data, data_shape: tuple[int, ...], with_ghost_cells: bool):
        """``data`` (host valid / full array, or a :class:`DeviceArray`) as (device full array, complex?, dtype of the result)."""
        nd = len(grid.shape)
        if isinstance(data, DeviceArray):
            if tuple(data.info.shape) != tuple(grid.shape) or data.host_shape[: len(data.host_shape) - nd] != data_shape:
                msg = f"Incompatible shapes {data.host_shape} != {data_shape + tuple(grid.shape)}"
                raise ValueError(msg)
            return data, data.complex_pairs, np.dtype(data.host_dtype)
        host = np.asarray(data)
        expect = data_shape + (tuple(n + 2 for n in grid.shape) if with_ghost_cells else tuple(grid.shape))
        if host.shape != expect:
            msg = f"Incompatible shapes {host.shape} != {expect}"
            raise ValueError(msg)
        cplx = host.dtype.kind == "c"
        info = self.grid_info(grid, real_dtype_of(host.dtype))
        if cplx:
            host = _planar(host, len(data_shape))
        dev = DeviceArray(info, data_shape + ((2,) if cplx else ()))
        if with_ghost_cells:
            dev.set_hostfull(host, self.stream)
        else:
            dev.set_valid(np.ascontiguousarray(host, dtype=info.dtype), self.stream)
        return dev, cplx, np.dtype(np.asarray(data).dtype)

    def make_interpolator(self, field, *, fill=None, with_ghost_cells: bool = False):
        """``interpolator(point, data=None)``: the values of ``field`` at points given in grid coordinates along the last axis of ``point``
        (shape ``(..., num_axes)``), as an array of shape ``data_shape + point_shape`` in the data's dtype - the contract of
        ``pde/backends/numba/backend.py:895-988``.  ``data``: a host array (valid data, or the full array when ``with_ghost_cells``) or a
        :class:`DeviceArray` on the field's grid.  Without ``data`` the field's own data is read - the device copy while the state is
        resident, without pulling it (``with_ghost_cells=True`` without ``data`` reads the host's full array, whose ghost cells the
        caller has set, and so pulls a resident state; ``field.interpolate(point, bc=...)`` sets them on the device instead).  Points outside the
        domain get ``fill``; without one ``DomainError`` is raised."""
        grid = field.grid
        _require_cartesian(grid)
        num_axes = len(grid.shape)
        data_shape = (grid.dim,) * int(field.rank)
        dtype = field_dtype(field)
        _abi.dtype_code(real_dtype_of(dtype))            # float64 / float32 (and their complex pairs) only
        fill_host = _convert_fill(fill, data_shape, dtype)
        source = _Source(grid)
        dim_error_msg = f"Dimension of point does not match axes count {num_axes}"      # numba/backend.py:945
        state: dict = {}

        def own_data():
            link = valid_link(field)
            if link is not None and not with_ghost_cells:
                return link.dev_state              # the device copy is current: nothing crosses PCIe but points and values
            # with_ghost_cells: the ghost cells are the HOST array's (the caller set them there), so a resident state is pulled first
            return field._data_full if with_ghost_cells else field.data

        def scratch(name: str, nbytes: int) -> DeviceBuffer:
            if name not in state or state[name].nbytes < nbytes:
                state[name] = DeviceBuffer(nbytes)
            return state[name]

        def interpolator(point, data=None):
            point = np.atleast_1d(point)
            if point.shape[-1] != num_axes:
                raise error_classes()[1](dim_error_msg)
            point_shape = point.shape[:-1]
            lib = self._lib
            if not lib.has("interpolate_points"):
                msg = "hip backend: the loaded library has no interpolation kernels"
                raise NotImplementedError(msg)
            dev, cplx, out_dtype = self._to_interp_source(grid, own_data() if data is None else data, data_shape, with_ghost_cells)
            pts = np.ascontiguousarray(point.reshape(-1, num_axes), dtype=np.float64)
            npoints = pts.shape[0]
            nvalues = dev.ncomp * npoints * dev.dtype.itemsize
            at_count = -(-nvalues // 8) * 8                 # values, then the 8-byte counter: one download brings both
            result = np.empty(at_count + 8, dtype=np.uint8)
            if npoints:
                if fill_host is not None and "fill" not in state:
                    state["fill"] = DeviceBuffer(fill_host.nbytes)
                    lib.memcpy_h2d(state["fill"].ptr, fill_host.ctypes.data, fill_host.nbytes, self.stream)
                fill_dev = state.get("fill")
                if fill_dev is not None and fill_host.size != dev.ncomp:
                    msg = f"fill value has {fill_host.size} components, the data {dev.ncomp}"
                    raise ValueError(msg)
                # the buffers are kept between calls (a tracker asks for the same few hundred probes at every interrupt)
                p_dev, o_dev = scratch("points", pts.nbytes), scratch("result", result.nbytes)
                lib.memcpy_h2d(p_dev.ptr, pts.ctypes.data, pts.nbytes, self.stream)
                lib.memset(o_dev.ptr + at_count, 0, 8, self.stream)
                lib.interpolate_points(dev.info.ref, dev.ncomp, source.periodic, source.lo, int(bool(with_ghost_cells)), dev.ptr, p_dev.ptr, npoints,
                                       None if fill_dev is None else fill_dev.ptr, o_dev.ptr, o_dev.ptr + at_count, self.stream)
                lib.memcpy_d2h(result.ctypes.data, o_dev.ptr, result.nbytes, self.stream)
                if result[at_count:].view(np.uint64)[0]:
                    raise error_classes()[0](_OOB_MESSAGE)
            planar = result[:nvalues].view(dev.dtype).reshape(dev.ncomp, npoints)
            if cplx:
                pairs = planar.reshape(data_shape + (2,) + point_shape)
                lead = len(data_shape)
                out = np.take(pairs, 0, axis=lead) + 1j * np.take(pairs, 1, axis=lead)
                return out.astype(out_dtype, copy=False)
            return planar.reshape(data_shape + point_shape).astype(out_dtype, copy=False)

        return interpolator

    def interpolate_field(self, field, point, *, bc=None, fill=None):
        """``field.interpolate(point, bc=..., fill=...)`` (pde/fields/datafield_base.py:664-700) on the device: with ``bc`` the conditions
        are imposed first, edge and corner ghost cells included, and the full array is interpolated."""
        if bc is None:
            return self.make_interpolator(field, fill=fill, with_ghost_cells=False)(np.asarray(point))
        dev = self._full_with_corners(field, bc)
        return self.make_interpolator(field, fill=fill, with_ghost_cells=True)(np.asarray(point), data=dev)

    def _full_with_corners(self, field, bc) -> DeviceArray:
        """The field's data on the device with the ghost cells of ``bc`` set, edges and corners included (``set_corners=True``).  The
        device copy of a resident state is used in place: only its ghost cells are written."""
        grid = field.grid
        bcs = grid.get_boundary_conditions(bc, rank=int(field.rank))
        link = valid_link(field)
        if link is not None:
            # Only ghost cells of the live state are written.  Nothing reads them as they are left here: every operator and every
            # stepper sweep sets the ghost cells of its operand from its own conditions before the stencil reads them, and a pull
            # brings down the valid cells only.
            dev = link.dev_state
        else:
            data_shape = (grid.dim,) * int(field.rank)
            dev = DeviceArray(self.grid_info(grid, field.dtype), data_shape).set_valid(field.data, self.stream)
        self.make_ghost_cell_setter(bcs, set_corners=True)(dev)
        return dev

    def interpolate_to_grid(self, field, grid, *, bc=None, fill=None, label=None):
        """``field.interpolate_to_grid(grid, bc=..., fill=..., label=...)`` (pde/fields/scalar.py:468) with the structured kernel
        (``pdehip_interpolate_to_grid``): Cartesian -> Cartesian, scalar, vector and rank-2 tensor fields; returns a field of the same class."""
        src = field.grid
        _require_cartesian(src, "interpolate_to_grid")
        if getattr(src, "dim", len(src.shape)) != getattr(grid, "dim", None):
            msg = f"Incompatible grid dimensions ({src.dim:d} != {getattr(grid, 'dim', -1):d})"      # scalar.py:496-498
            raise error_classes()[1](msg)
        _require_cartesian(grid, "interpolate_to_grid")
        data_shape = (src.dim,) * int(field.rank)
        dtype = field_dtype(field)
        fill_host = _convert_fill(fill, data_shape, dtype)
        lib = self._lib
        if not lib.has("interpolate_to_grid"):
            msg = "hip backend: the loaded library has no interpolation kernels"
            raise NotImplementedError(msg)
        if bc is not None:
            dev, cplx = self._full_with_corners(field, bc), False
        else:
            link = valid_link(field)
            data = link.dev_state if link is not None else field.data
            dev, cplx, _ = self._to_interp_source(src, data, data_shape, False)
        out = DeviceArray(self.grid_info(grid, dev.dtype), dev.comp_shape, complex_pairs=cplx)
        lib.memset(out.ptr, 0, out.nbytes, self.stream)
        coords = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.float64) for c in grid.axes_coords]))
        c_dev, tables, count = DeviceBuffer(coords.nbytes), DeviceBuffer(40 * coords.size), DeviceBuffer(8)
        lib.memcpy_h2d(c_dev.ptr, coords.ctypes.data, coords.nbytes, self.stream)
        lib.memset(count.ptr, 0, 8, self.stream)
        fill_dev = None
        if fill_host is not None:
            fill_dev = DeviceBuffer(fill_host.nbytes)
            lib.memcpy_h2d(fill_dev.ptr, fill_host.ctypes.data, fill_host.nbytes, self.stream)
        source = _Source(src)
        lib.interpolate_to_grid(dev.info.ref, dev.ncomp, source.periodic, source.lo, int(bc is not None), dev.ptr, out.info.ref, c_dev.ptr,
                                None if fill_dev is None else fill_dev.ptr, out.ptr, tables.ptr, count.ptr, self.stream)
        outside = C.c_uint64(0)
        lib.memcpy_d2h(C.addressof(outside), count.ptr, 8, self.stream)
        if outside.value:
            raise error_classes()[0](_OOB_MESSAGE)
        values = out.get_valid(stream=self.stream)
        return base_class(field)(grid, values.astype(dtype, copy=False), label=label)


def interpolate_to_grid(field, grid, *, bc=None, fill=None, label=None, backend="hip"):
    """Regrid ``field`` (a py-pde or a mirror field) onto the Cartesian ``grid`` on the device; returns a field of the same kind.  The
    documented route to the structured kernel: ``pde_hip.interpolate_to_grid(field, grid, bc=..., fill=...)``."""
    if not isinstance(backend, str):
        impl = backend
    elif type(field).__module__.split(".")[0] == "pde":
        from pde.backends import get_backend as pde_get_backend

        from . import pypde_plugin  # noqa: F401  (registers "hip")

        impl = pde_get_backend(backend)
    else:
        from .backend import get_backend

        impl = get_backend(backend)
    return impl.interpolate_to_grid(field, grid, bc=bc, fill=fill, label=label)
