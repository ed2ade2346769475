"""Projections and cuts of a field where it lives - :class:`ProjectionMixin` of the backend.

What users of 3-D runs write out at an interrupt is rarely the state: it is a projection (``state.project("z")``), a mid-plane
(``state.slice({"z": "mid"})``) or the line / image behind a plot (``get_line_data`` / ``get_image_data``).  In the reference all of them
read ``field.data`` (``pde/fields/scalar.py:269-427``, ``pde/grids/cartesian.py:296-402``) and so pull a device-resident state
(:class:`~pde_hip.resident.ResidentState`) over PCIe.  ``pdehip_project`` and ``pdehip_extract_box`` (``csrc/pdehip_project.hip``)
answer on the device: only the result comes down.

A device sum differs from numpy's in the last bits (another order of the additions), so nothing here replaces a host computation
silently: the functions below are called explicitly, and the methods of a resident field answer from the device only under the
configuration key ``device_projections``.  Maxima, minima, slices and cuts have numpy's bits either way.

Host data, complex states, vector and tensor fields, collections, decomposed steppers (no resident state) and a library without the
two entry points take the host path with the reference's arithmetic; none of them is an error.
"""

from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _abi
from .device import DeviceArray, DeviceBuffer
from .resident import DeviceOption, backend_of, base_class, device_source, is_collection

_METHOD_CODES = {"integral": _abi.PROJECT_SUM, "average": _abi.PROJECT_SUM, "mean": _abi.PROJECT_SUM, "maximum": _abi.PROJECT_MAX,
                 "max": _abi.PROJECT_MAX, "minimum": _abi.PROJECT_MIN, "min": _abi.PROJECT_MIN}


class DomainError(ValueError):
    """A position outside the grid (``pde.grids.base.DomainError``; with py-pde its own class is raised)."""


def _domain_error(grid):
    if type(grid).__module__.split(".")[0] == "pde":
        from pde.grids.base import DomainError as PdeDomainError

        return PdeDomainError
    return DomainError


# ---- what the reference's methods decide before they touch the data (messages as in pde/fields/scalar.py:269-427) --------------------
def parse_axes(grid, axes) -> tuple[tuple[int, ...], tuple[int, ...]]:
    """(removed axes in the order given, retained axes ascending) of ``project(axes)``."""
    if isinstance(axes, str):
        axes = [axes]
    if any(ax not in grid.axes for ax in axes):
        msg = f"The axes {axes} are not all contained in {grid} with axes {grid.axes}"
        raise ValueError(msg)
    ax_remove = tuple(grid.axes.index(ax) for ax in axes)
    ax_retain = tuple(sorted(set(range(grid.num_axes)) - set(ax_remove)))
    return ax_remove, ax_retain


def parse_position(grid, position) -> tuple[dict[int, int], tuple[int, ...]]:
    """({removed axis: index of the nearest cell}, retained axes) of ``slice(position)``."""
    values: dict[int, float] = {}
    for ax, pos in position.items():
        try:
            i = grid.axes.index(ax)
        except ValueError:
            msg = f"The axes {ax} is not contained in {grid} with axes {grid.axes}"
            raise ValueError(msg) from None
        if isinstance(pos, str):
            if pos in {"min", "low", "lower"}:
                values[i] = grid.axes_coords[i][0]
            elif pos in {"max", "high", "upper"}:
                values[i] = grid.axes_coords[i][-1]
            elif pos in {"mid", "middle", "center"}:
                values[i] = np.mean(grid.axes_bounds[i])
            else:
                msg = f"Unknown position `{pos}`"
                raise ValueError(msg)
        else:
            values[i] = float(pos)
    ax_retain = tuple(sorted(set(range(grid.num_axes)) - set(values)))
    return values, ax_retain


def nearest_cells(grid, values: dict[int, float]) -> dict[int, int]:
    """Index of the cell nearest to each position, in ascending order of the axes (the order in which the reference complains)."""
    cells = {}
    for i in sorted(values):
        pos = values[i]
        lo, hi = grid.axes_bounds[i]
        if pos < lo or pos > hi:
            msg = f"Position {grid.axes[i]} = {pos} is outside the domain"
            raise _domain_error(grid)(msg)
        cells[i] = int(np.argmin((grid.axes_coords[i] - pos) ** 2))
    return cells


def removed_weight(grid, ax_remove) -> float:
    """Product of the spacings of the removed axes - the one factor ``grid.integrate(data, axes)`` multiplies every cell with."""
    w = 1.0
    for ax in range(grid.num_axes):
        if ax in ax_remove:
            w = w * float(grid.discretization[ax])
    return w


def line_axis(grid, spec) -> int:
    try:
        return int(spec)
    except ValueError:
        try:
            return grid.axes.index(spec)
        except ValueError:
            msg = f"Axis `{spec}` not defined"
            raise ValueError(msg) from None


# ---- the reference's arithmetic on host data: the mirror fields' own methods, and the host path of everything else -----------------
def host_integrate(grid, data: np.ndarray, ax_remove) -> np.ndarray:
    """``grid.integrate(data, axes=ax_remove)`` (pde/grids/base.py:1286-1341) on a Cartesian grid."""
    if hasattr(grid, "integrate"):
        return grid.integrate(data, axes=ax_remove)
    volumes = functools.reduce(np.outer, [grid.discretization[ax] if ax in ax_remove else 1 for ax in range(grid.num_axes)])
    lead = data.ndim - grid.num_axes
    return (data * volumes).sum(axis=tuple(lead + ax for ax in ax_remove))


def host_project(grid, data: np.ndarray, ax_remove, method: str) -> np.ndarray:
    lead = data.ndim - grid.num_axes
    axes = tuple(lead + ax for ax in ax_remove)
    if method == "integral":
        return host_integrate(grid, data, ax_remove)
    if method in {"average", "mean"}:
        return host_integrate(grid, data, ax_remove) / host_integrate(grid, np.broadcast_to(1, grid.shape), ax_remove)
    if method in {"maximum", "max"}:
        return np.max(data, axis=axes)
    if method in {"minimum", "min"}:
        return np.min(data, axis=axes)
    msg = f"Unknown projection method `{method}`"
    raise ValueError(msg)


def host_line_data(grid, data: np.ndarray, extract: str = "auto") -> dict:
    """The dictionary of ``CartesianGrid.get_line_data`` (pde/grids/cartesian.py:296-372)."""
    dim = grid.num_axes
    if data.shape[-dim:] != tuple(grid.shape):
        msg = f"Shape {data.shape} of the data array is not compatible with grid shape {grid.shape}"
        raise ValueError(msg)
    kind, axis = parse_extract(grid, extract)
    lead = data.ndim - dim
    if kind == "cut":
        index = (slice(None),) * lead + tuple(slice(None) if ax == axis else grid.shape[ax] // 2 for ax in range(dim))
        data_y = data[index]
    else:
        data_y = data.mean(axis=tuple(ax - dim for ax in range(dim) if ax != axis))
    return _line_dict(grid, axis, kind, data_y)


def parse_extract(grid, extract: str) -> tuple[str, int]:
    if extract == "auto":
        extract = "cut_0"
    if extract.startswith("cut_"):
        return "cut", line_axis(grid, extract[4:])
    if extract.startswith("project_"):
        return "project", line_axis(grid, extract[8:])
    msg = f"Unknown extraction method `{extract}`"
    raise ValueError(msg)


def _line_dict(grid, axis: int, kind: str, data_y) -> dict:
    label = f"Cut along {grid.axes[axis]}" if kind == "cut" else f"Projection onto {grid.axes[axis]}"
    return {"data_x": grid.axes_coords[axis], "data_y": data_y, "extent_x": grid.axes_bounds[axis], "label_x": grid.axes[axis],
            "label_y": "" if grid.num_axes == 1 else label}


def host_image_data(grid, data: np.ndarray) -> dict:
    """The dictionary of ``CartesianGrid.get_image_data`` (pde/grids/cartesian.py:374-402)."""
    dim = grid.num_axes
    if data.shape[-dim:] != tuple(grid.shape):
        msg = f"Shape {data.shape} of the data array is not compatible with grid shape {grid.shape}"
        raise ValueError(msg)
    if dim == 2:
        image = data
    elif dim == 3:
        image = data[:, :, grid.shape[-1] // 2]
    else:
        msg = "Creating images is only implemented for 2d and 3d grids"
        raise NotImplementedError(msg)
    return _image_dict(grid, image)


def _image_dict(grid, image) -> dict:
    return {"data": image, "x": grid.axes_coords[0], "y": grid.axes_coords[1], "extent": [float(v) for c in grid.axes_bounds[:2] for v in c],
            "label_x": grid.axes[0], "label_y": grid.axes[1]}


def label_line(field, data: dict) -> dict:
    """What ``DataFieldBase.get_line_data`` adds to the grid's dictionary (pde/fields/datafield_base.py:1037-1050)."""
    if data.get("label_y"):
        if field.label:
            data["label_y"] = f"{field.label} ({data['label_y']})"
    else:
        data["label_y"] = field.label
    return data


def finish_image(field, data: dict, transpose: bool) -> dict:
    """What ``DataFieldBase.get_image_data`` adds (pde/fields/datafield_base.py:1052-1074)."""
    data["title"] = field.label
    if transpose:
        data["x"], data["y"] = data["y"], data["x"]
        data["data"] = data["data"].T
        data["label_x"], data["label_y"] = data["label_y"], data["label_x"]
        data["extent"] = data["extent"][2:] + data["extent"][:2]
    return data


# ---- which objects the device answers for ------------------------------------------------------------------------------------------
def device_copy(backend, obj):
    """The :class:`DeviceArray` a projection of ``obj`` reads on the device, or None (the host path): a bare array of real components,
    or the resident state of a real scalar field while the device copy is the current one."""
    dev, bare = device_source(backend, obj, needs=("project", "extract_box"))
    if dev is None or bare:
        return dev
    scalar = not is_collection(obj) and int(getattr(obj, "rank", 0)) == 0 and dev.comp_shape == ()
    return dev if scalar else None


def _grid_of(obj, grid):
    own = getattr(obj, "grid", None)
    if own is not None:
        return own
    return grid if grid is not None else _ArrayGrid(obj.info)


class ProjectionMixin:
    """``make_projector`` and ``make_slicer`` of :class:`~pde_hip.backend.HipBackendMixin`."""

    device_projections = DeviceOption(
        """Whether ``project`` / ``slice`` / ``get_line_data`` / ``get_image_data`` of a real scalar field whose state is resident on the
        device are answered there, without a download (``config["backend.hip.device_projections"]`` with py-pde,
        ``backend.device_projections = True`` stand-alone).  Default False: a device sum differs from numpy's in the last bits, and
        bit-for-bit behaviour is the default.""")

    # --- the two calls ----------------------------------------------------------------------------------------------------------
    def _result_buffer(self, nbytes: int) -> DeviceBuffer:
        """One output buffer per backend, grown on demand (an allocation per interrupt would cost more than a small projection)."""
        buf = getattr(self, "_projection_out", None)
        if buf is None or buf.nbytes < nbytes:
            self._projection_out = buf = DeviceBuffer(max(int(nbytes), 4096))
        return buf

    def device_project(self, dev: DeviceArray, ax_remove, code: int, weight: float = 1.0) -> np.ndarray:
        """``pdehip_project`` of every component: ``comp_shape + retained extents``, fp64 for the sum, else the field's type."""
        shape = dev.info.shape
        removed = set(int(ax) for ax in ax_remove)
        mask = sum(1 << ax for ax in removed)
        retained = tuple(n for ax, n in enumerate(shape) if ax not in removed)
        host = np.empty(dev.comp_shape + retained, dtype=np.float64 if code == _abi.PROJECT_SUM else dev.dtype)
        out = self._result_buffer(host.nbytes)
        self._lib.project(dev.info.ref, dev.ncomp, dev.ptr, mask, code, float(weight), out.ptr, self.stream)
        self._lib.memcpy_d2h(host.ctypes.data, out.ptr, host.nbytes, self.stream)
        return host

    def device_box(self, dev: DeviceArray, lo, extent) -> np.ndarray:
        """``pdehip_extract_box``: ``comp_shape + extent`` in the field's type."""
        ndim = len(dev.info.shape)
        host = np.empty(dev.comp_shape + tuple(int(n) for n in extent), dtype=dev.dtype)
        out = self._result_buffer(host.nbytes)
        self._lib.extract_box(dev.info.ref, dev.ncomp, dev.ptr, (C.c_long * ndim)(*map(int, lo)), (C.c_long * ndim)(*map(int, extent)), out.ptr,
                              self.stream)
        self._lib.memcpy_d2h(host.ctypes.data, out.ptr, host.nbytes, self.stream)
        return host

    def _device_cut(self, dev: DeviceArray, cells: dict[int, int]) -> np.ndarray:
        """The cells ``cells[axis]`` of the removed axes, everything of the others: ``comp_shape + retained extents``."""
        shape = dev.info.shape
        lo = [cells.get(ax, 0) for ax in range(len(shape))]
        extent = [1 if ax in cells else shape[ax] for ax in range(len(shape))]
        box = self.device_box(dev, lo, extent)
        return box.reshape(dev.comp_shape + tuple(n for ax, n in enumerate(shape) if ax not in cells))

    def _device_mean(self, dev: DeviceArray, ax_remove, weight: float = 1.0) -> np.ndarray:
        count = int(np.prod([dev.info.shape[ax] for ax in ax_remove], dtype=np.int64))
        return self.device_project(dev, ax_remove, _abi.PROJECT_SUM, weight) / (weight * count)

    # --- project ------------------------------------------------------------------------------------------------------------------
    def make_projector(self, grid=None):
        """``project(obj, axes, *, method="integral", label=None)`` with the meaning of ``ScalarField.project``
        (pde/fields/scalar.py:269-339): the axes named are removed by an integral, an average (``"average"`` / ``"mean"``), a maximum or
        a minimum; the result is a host ``ScalarField`` on ``grid.slice(retained axes)``.

        A real scalar field whose state is resident on the device with the device copy current (between the stepper calls of a
        ``backend="hip"`` run) is reduced ON THE DEVICE and only the result comes down.  So is a :class:`DeviceArray` - of any number of
        components up to 64; the result is then the bare array ``components + retained extents`` (``grid`` gives the axis names and the
        spacings, else ``x, y, z`` and the spacings of the array).  Everything else is reduced on the host with the reference's
        arithmetic and is never uploaded for this: host data, complex states, collections (a list, one entry per field), vector and
        tensor fields (the reference has no ``project`` for them: the bare array of the projected components)."""

        def project(obj, axes, *, method: str = "integral", label=None):
            if is_collection(obj):
                return [project(f, axes, method=method, label=label) for f in obj]
            field_grid = _grid_of(obj, grid)
            ax_remove, ax_retain = parse_axes(field_grid, axes)
            dev = device_copy(self, obj) if len(set(ax_remove)) == len(ax_remove) and method in _METHOD_CODES else None
            if dev is None and not isinstance(obj, DeviceArray):
                if int(getattr(obj, "rank", 0)) == 0 and hasattr(base_class(obj), "project"):
                    return base_class(obj).project(obj, axes, method=method, label=label)
                return host_project(field_grid, np.asarray(obj.data), ax_remove, method)       # (reads `data`: a resident state comes down)
            bare = isinstance(obj, DeviceArray)
            sliced = None if bare else field_grid.slice(ax_retain)
            if dev is None:
                data = host_project(field_grid, obj.get_valid(stream=self.stream), ax_remove, method)
            elif method == "integral":
                data = self.device_project(dev, ax_remove, _abi.PROJECT_SUM, removed_weight(field_grid, ax_remove))
            elif method in {"average", "mean"}:
                data = self._device_mean(dev, ax_remove, removed_weight(field_grid, ax_remove))
            else:
                data = self.device_project(dev, ax_remove, _METHOD_CODES[method])
            return data if bare else base_class(obj)(grid=sliced, data=data, label=label)

        return project

    # --- slice --------------------------------------------------------------------------------------------------------------------
    def make_slicer(self, grid=None):
        """``slice(obj, position, *, label=None)`` with the meaning of ``ScalarField.slice`` (pde/fields/scalar.py:341-427): ``position``
        maps axis names to coordinates or to ``"low"`` / ``"mid"`` / ``"high"``; the cells nearest to them are taken and the axes named
        are removed.  Device and host path as for :meth:`make_projector`; the bits are numpy's on either."""

        def slice_(obj, position, *, label=None):
            if is_collection(obj):
                return [slice_(f, position, label=label) for f in obj]
            field_grid = _grid_of(obj, grid)
            values, ax_retain = parse_position(field_grid, position)
            dev = device_copy(self, obj)
            bare = isinstance(obj, DeviceArray)
            if dev is None and not bare:
                if int(getattr(obj, "rank", 0)) == 0 and hasattr(base_class(obj), "slice"):
                    return base_class(obj).slice(obj, position, label=label)
                cells = nearest_cells(field_grid, values)
                data = np.asarray(obj.data)
                lead = data.ndim - field_grid.num_axes
                return data[(slice(None),) * lead + tuple(cells.get(ax, slice(None)) for ax in range(field_grid.num_axes))]
            sliced = None if bare else field_grid.slice(ax_retain)
            cells = nearest_cells(field_grid, values)
            if dev is None:
                data = obj.get_valid(stream=self.stream)
                lead = data.ndim - field_grid.num_axes
                return data[(slice(None),) * lead + tuple(cells.get(ax, slice(None)) for ax in range(field_grid.num_axes))]
            data = self._device_cut(dev, cells)
            return data if bare else base_class(obj)(grid=sliced, data=data, label=label)

        return slice_

    # --- the data behind line and image plots ---------------------------------------------------------------------------------------
    def line_data(self, obj, extract: str = "auto") -> dict:
        """The dictionary of ``field.get_line_data(extract=extract)``: ``cut_#`` is the line through the cells ``shape // 2`` of the
        other axes, ``project_#`` the mean over them (on the device: the fp64 sum divided by their number, in the field's type)."""
        if isinstance(obj, DeviceArray):
            msg = "line_data needs a field (axis names, coordinates and a label), not a bare device array"
            raise TypeError(msg)
        dev = device_copy(self, obj)
        if dev is None:
            return base_class(obj).get_line_data(obj, extract=extract)
        grid = obj.grid
        kind, axis = parse_extract(grid, extract)
        if not 0 <= axis < grid.num_axes:
            return base_class(obj).get_line_data(obj, extract=extract)
        others = [ax for ax in range(grid.num_axes) if ax != axis]
        if kind == "cut" or not others:
            data_y = self._device_cut(dev, {ax: grid.shape[ax] // 2 for ax in others} if kind == "cut" else {})
        else:
            data_y = self._device_mean(dev, others).astype(dev.dtype)
        return label_line(obj, _line_dict(grid, axis, kind, data_y))

    def image_data(self, obj, transpose: bool = False) -> dict:
        """The dictionary of ``field.get_image_data(transpose=transpose)``: the field itself in 2-D, the plane ``shape[-1] // 2`` in 3-D."""
        if isinstance(obj, DeviceArray):
            msg = "image_data needs a field (axis names, coordinates and a label), not a bare device array"
            raise TypeError(msg)
        dev = device_copy(self, obj)
        if dev is None or obj.grid.num_axes not in (2, 3):
            return base_class(obj).get_image_data(obj, transpose=transpose)
        grid = obj.grid
        image = self._device_cut(dev, {2: grid.shape[2] // 2} if grid.num_axes == 3 else {})
        return finish_image(obj, _image_dict(grid, image), transpose)


class _ArrayGrid:
    """Axis names, spacings and coordinates of a bare :class:`DeviceArray` (a unit-offset Cartesian grid with the array's spacings)."""

    def __init__(self, info):
        self.shape, self.discretization = tuple(info.shape), np.array(info.dx)
        self.num_axes = len(self.shape)
        self.axes = list("xyz"[: self.num_axes])
        self.axes_bounds = tuple((0.0, n * dx) for n, dx in zip(self.shape, self.discretization))
        self.axes_coords = tuple((np.arange(n) + 0.5) * dx for n, dx in zip(self.shape, self.discretization))

    def __repr__(self) -> str:
        return f"array grid {self.shape}"


# ---- module level: pde_hip.project(field, axes) ... ---------------------------------------------------------------------------------
def project(field, axes, *, method: str = "integral", label=None, backend="hip"):
    """``field.project(axes, method=method, label=label)`` - on the device while the state of a real scalar field is resident there, else
    on the host: ``pde_hip.project(state, "z", method="mean")`` inside a tracker costs a plane instead of the state."""
    return backend_of(field, backend).make_projector()(field, axes, method=method, label=label)


def slice_field(field, position, *, label=None, backend="hip"):
    """``field.slice(position, label=label)``, on the device while the state is resident there."""
    return backend_of(field, backend).make_slicer()(field, position, label=label)


def line_data(field, extract: str = "auto", *, backend="hip") -> dict:
    """``field.get_line_data(extract=extract)``, on the device while the state is resident there."""
    return backend_of(field, backend).line_data(field, extract)


def image_data(field, *, transpose: bool = False, backend="hip") -> dict:
    """``field.get_image_data(transpose=transpose)``, on the device while the state is resident there."""
    return backend_of(field, backend).image_data(field, transpose)


# ---- the methods of a resident field, answered from the device (opt-in: `device_projections`) ------------------------------------------
def device_method(link, field, name: str):
    """A stand-in for ``field.<name>`` that answers from the device copy what the device path takes and passes every other call on to
    the reference method, or None (the caller then takes the reference method itself)."""
    backend = link.backend
    if device_copy(backend, field) is None:
        return None
    reference = getattr(base_class(field), name)
    if name == "project":
        def method(axes, *, method="integral", label=None):
            return backend.make_projector()(field, axes, method=method, label=label)
    elif name == "slice":
        def method(position, *, method="nearest", label=None):
            if method != "nearest":
                return reference(field, position, method=method, label=label)
            return backend.make_slicer()(field, position, label=label)
    elif name == "get_line_data":
        def method(scalar="auto", extract="auto"):
            if scalar != "auto":
                return reference(field, scalar=scalar, extract=extract)
            return backend.line_data(field, extract)
    else:
        def method(scalar="auto", transpose=False, **kwargs):
            if scalar != "auto" or kwargs:
                return reference(field, scalar=scalar, transpose=transpose, **kwargs)
            return backend.image_data(field, transpose)
    return functools.wraps(reference)(method)
