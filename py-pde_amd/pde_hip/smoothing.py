"""Gaussian smoothing of a field where it lives - :class:`SmoothingMixin` of the backend.

``DataFieldBase.smooth(sigma)`` (``pde/fields/datafield_base.py:988-1035``) runs ``scipy.ndimage.gaussian_filter1d`` axis by axis on
``field.data``: mode ``"wrap"`` on periodic axes, ``"reflect"`` elsewhere, ``sigma / dx`` per axis, in place on the output after the
first axis.  On a device-resident state (:class:`~pde_hip.resident.ResidentState`) that is a download of the state followed by a
single-threaded host filter.  ``pdehip_smooth_axis`` (``csrc/pdehip_smooth.hip``) runs one such pass on the device, bit for bit with
scipy's arithmetic (``include/pdehip.h``): the result can stay there (``device=True``, ``out=state``) and feed
``pde_hip.field_statistics``, ``pde_hip.project`` and ``pde_hip.slice_field`` without ever coming down.

The weights are computed HERE, with numpy, exactly as scipy computes them (:func:`gaussian_weights`): numpy's ``exp`` is the one scipy
uses, the C library's may differ in the last bit.  The arithmetic of a pass does not depend on the fp32 arithmetic mode of the backend
(scipy's line buffers are double for both field types), so the call is served in the pure-fp32 mode too.

The device path takes real fp64 / fp32 fields of at most 64 components on Cartesian grids: a resident state whose device copy is the
current one (read where it is), a host field (uploaded once: the call is explicit and the filter far heavier than the upload) and a bare
:class:`~pde_hip.device.DeviceArray`.  Complex states, collections (field by field), non-Cartesian grids, a ``sigma`` that is not a
positive finite scalar and a library without the entry point take the host path with the reference's arithmetic; none of them is an
error.  The result of the device path has the field's own type (every pass rounds once to it), which is what the reference gives for
``out=`` a field of that type; ``field.smooth()`` of the reference WITHOUT ``out`` allocates a float64 result even for an fp32 field.
"""

from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np

from . import _abi
from .device import DeviceArray
from .resident import DeviceOption, ResidentState, backend_of, base_class, field_dtype, is_collection, link_of, resident_link


# ---- scipy's weights and scipy's arithmetic, in numpy ---------------------------------------------------------------------------------
def gaussian_weights(sigma_cells: float) -> tuple[int, np.ndarray]:
    """``(radius, weights[0..radius])`` of ``gaussian_filter1d(sigma=sigma_cells)`` (``truncate=4``, ``order=0``): the upper half of
    scipy's normalised kernel, centre weight first - the half its symmetric branch reads."""
    sigma_cells = float(sigma_cells)
    if not (math.isfinite(sigma_cells) and sigma_cells > 0):
        msg = f"the standard deviation of a Gaussian filter is a positive finite number (got {sigma_cells} cells)"
        raise ValueError(msg)
    r = int(4.0 * sigma_cells + 0.5)
    phi = np.exp(-0.5 / sigma_cells**2 * np.arange(-r, r + 1) ** 2)
    phi /= phi.sum()
    return r, np.ascontiguousarray(phi[r:], dtype=np.float64)


def extended_index(n: int, r: int, wrap: bool) -> np.ndarray:
    """The cells of ``[0, n)`` that the positions ``-r ... n + r - 1`` of the extended line show."""
    p = np.arange(-r, n + r)
    if wrap:
        return p % n
    q = p % (2 * n)
    return np.where(q < n, q, 2 * n - 1 - q)


def host_filter_axis(data: np.ndarray, axis: int, weights: np.ndarray, wrap: bool, dtype=None) -> np.ndarray:
    """One pass in numpy: the centre term first, then the pairs from the outermost one inwards, every operation one fp64 rounding; the
    result rounded once to ``dtype`` (default: the type of ``data``)."""
    data = np.asarray(data)
    dtype = data.dtype if dtype is None else np.dtype(dtype)
    if np.iscomplexobj(data):      # (scipy filters the real and the imaginary part on their own)
        real = np.float32 if dtype == np.complex64 else np.float64
        return (host_filter_axis(data.real, axis, weights, wrap, real) + 1j * host_filter_axis(data.imag, axis, weights, wrap, real)).astype(dtype)
    n, r = data.shape[axis], len(weights) - 1
    x = np.moveaxis(data.astype(np.float64), axis, -1)[..., extended_index(n, r, wrap)]
    with np.errstate(invalid="ignore", over="ignore"):
        t = x[..., r:r + n] * weights[0]
        for j in range(r, 0, -1):
            t = t + (x[..., r - j:r - j + n] + x[..., r + j:r + j + n]) * weights[j]
        return np.moveaxis(t, -1, axis).astype(dtype)


def host_smooth(grid, data: np.ndarray, sigma: float, out: np.ndarray) -> np.ndarray:
    """``DataFieldBase.smooth`` on host arrays without scipy: the axes in the grid's order, every pass written to ``out`` (and read from it
    after the first)."""
    data_in = data
    for axis in range(-grid.num_axes, 0):
        _, weights = gaussian_weights(sigma / grid.discretization[axis])
        out[...] = host_filter_axis(data_in, axis, weights, bool(grid.periodic[axis]), out.dtype)
        data_in = out
    return out


def mirror_smooth(field, sigma: float = 1, *, out=None, label=None):
    """``smooth`` of the mirror field classes (``pde_hip/fields.py``)."""
    if out is None:
        out = field.__class__(field.grid, label=field.label)
    else:
        assert_field_compatible(field, out)
    host_smooth(field.grid, field.data, sigma, out.data)
    if label:
        out.label = label
    return out


def mirror_smooth_collection(collection, sigma: float = 1, *, out=None, label=None):
    """``FieldCollection.smooth``: field by field."""
    if out is None:
        out = collection.copy(label=label)
    elif len(out) != len(collection):
        msg = f"Fields {collection} and {out} are incompatible"
        raise ValueError(msg)
    for f_in, f_out in zip(collection, out):
        f_in.smooth(sigma=sigma, out=f_out)
    return out


def assert_field_compatible(field, other) -> None:
    """``FieldBase.assert_field_compatible`` (pde/fields/base.py:371-395); a py-pde field checks itself."""
    own = getattr(base_class(field), "assert_field_compatible", None)
    if own is not None:
        own(field, other)
        return
    if base_class(field) is not base_class(other):
        msg = f"Fields {field} and {other} are incompatible"
        raise TypeError(msg)
    if field.grid != other.grid:
        msg = f"Grids {field.grid} and {other.grid} are incompatible"
        raise ValueError(msg)


# ---- which objects the device answers for ------------------------------------------------------------------------------------------
def _is_cartesian(grid) -> bool:
    if not all(hasattr(grid, a) for a in ("shape", "discretization", "periodic")):
        return False
    return 1 <= len(grid.shape) <= _abi.MAX_DIM and len(grid.shape) == getattr(grid, "dim", len(grid.shape))


def _valid_sigma(sigma) -> bool:
    try:
        return np.ndim(sigma) == 0 and not isinstance(sigma, complex) and math.isfinite(sigma) and sigma > 0
    except TypeError:
        return False


def _device_field(field) -> bool:
    """A real fp64 / fp32 field of at most 64 components on a Cartesian grid."""
    if is_collection(field) or not _is_cartesian(getattr(field, "grid", None)):
        return False
    dtype = field_dtype(field)
    return dtype in (np.float64, np.float32) and field.grid.num_axes ** int(getattr(field, "rank", 0)) <= 64


class SmoothingMixin:
    """``make_smoother`` of :class:`~pde_hip.backend.HipBackendMixin`."""

    device_smoothing = DeviceOption(
        """Whether ``state.smooth(...)`` of a real field whose state is resident on the device is answered there, without a download
        (``config["backend.hip.device_smoothing"]`` with py-pde, ``backend.device_smoothing = True`` stand-alone).  Default False: with
        the default, nothing that existed before this option changes its path.  ``pde_hip.smooth`` does not depend on it.""")

    # --- the passes -------------------------------------------------------------------------------------------------------------
    def _smooth_work(self, info, comp_shape, slot: int) -> DeviceArray:
        """Work array ``slot`` for fields of this layout: slots 0 and 1 lie between the passes, slot 2 holds an uploaded host field or a
        result on its way down.  One buffer per slot, owned by the backend, grown on demand only."""
        from .device import DeviceBuffer

        buffers = self.__dict__.setdefault("_smooth_buffers", [None, None, None])
        probe = DeviceArray(info, comp_shape, ptr=0)      # (the size of the layout; owns nothing)
        if buffers[slot] is None or buffers[slot].nbytes < probe.nbytes:
            buffers[slot] = DeviceBuffer(probe.nbytes)
        return DeviceArray(info, comp_shape, buffer=buffers[slot], ptr=buffers[slot].ptr)

    def smooth_axis(self, src: DeviceArray, dst: DeviceArray, axis: int, weights: np.ndarray, wrap: bool, *, cell: bool = False) -> None:
        """One ``pdehip_smooth_axis`` pass ``src -> dst`` (two different arrays of one layout)."""
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        mode = (_abi.SMOOTH_WRAP if wrap else _abi.SMOOTH_REFLECT) | (_abi.SMOOTH_CELL if cell else 0)
        self._lib.smooth_axis(src.info.ref, src.ncomp, src.ptr, dst.ptr, int(axis), mode, len(weights) - 1,
                              weights.ctypes.data_as(C.POINTER(C.c_double)), self.stream)

    def device_smooth(self, src: DeviceArray, dst: DeviceArray, sigma: float, periodic) -> DeviceArray:
        """Every axis of ``src`` in the grid's order, the result in ``dst`` (which may be ``src``: in place).  The passes ping-pong between
        ``dst`` and the work arrays 0 and 1 of the backend; ``src`` is written by the last pass of an in-place call only.  Only a 1-D
        field smoothed in place needs one extra pass (a radius-0 copy of the interior, ``x * 1``) to land the result."""
        ndim = len(src.info.shape)
        passes = [(axis, gaussian_weights(sigma / src.info.dx[axis])[1], bool(periodic[axis])) for axis in range(ndim)]
        in_place = dst.ptr == src.ptr
        if in_place and ndim == 1:
            passes.append((0, np.ones(1), True))
        # the arrays the passes write, found backwards from the destination: never the array the same pass reads
        targets = [dst]
        for k in range(len(passes) - 1, 0, -1):
            spare = ([] if in_place else [dst]) + [self._smooth_work(src.info, src.comp_shape, slot) for slot in (0, 1)]
            targets.insert(0, next(a for a in spare if a.ptr != targets[0].ptr and a.ptr != src.ptr))
        cur = src
        for (axis, weights, wrap), target in zip(passes, targets):
            self.smooth_axis(cur, target, axis, weights, wrap)
            cur = target
        return dst

    def make_smoother(self, grid=None):
        """``smooth(obj, sigma=1, *, out=None, label=None, device=False)`` with the meaning of ``DataFieldBase.smooth``
        (pde/fields/datafield_base.py:988-1035): the axes in the grid's order, ``sigma / grid.discretization[axis]`` per axis, wrap on
        periodic axes and reflect elsewhere, every component of a vector or rank-2 field on its own.

        ``obj``: a field - its resident device copy is read where it is while it is the current one, host data is uploaded once - or a
        bare :class:`DeviceArray` (``grid`` then gives the periodicity: ``TypeError`` without it).  Results: ``out=None`` a new host
        field of the same class (a bare array: a numpy array), only the result comes down; ``device=True`` (without ``out``) a new
        :class:`DeviceArray`, nothing is downloaded; ``out is obj`` for a resident state: smoothed in place on the device, the host
        copy stays stale and the next stepper call continues from the smoothed state; ``out`` another host field: filled after
        ``assert_field_compatible``.  What the device path does not take (module docstring) is smoothed on the host with the
        reference's arithmetic."""

        def smooth(obj, sigma=1, *, out=None, label=None, device: bool = False):
            if device and out is not None:
                msg = "device=True returns a new device array: it takes no `out`"
                raise ValueError(msg)
            served = _valid_sigma(sigma) and self._lib.has("smooth_axis")
            if isinstance(obj, DeviceArray):
                if grid is None:
                    msg = "smoothing a bare device array needs the grid (its periodicity): backend.make_smoother(grid)"
                    raise TypeError(msg)
                if obj.complex_pairs or obj.ncomp > 64 or not served:
                    data = host_smooth(grid, obj.get_valid(stream=self.stream), sigma, np.empty(obj.host_shape, obj.host_dtype))
                    if isinstance(out, DeviceArray):
                        return out.set_valid(data, self.stream)
                    return obj.empty_like().set_valid(data, self.stream) if device else data
                if isinstance(out, DeviceArray):
                    if out.info.key() != obj.info.key() or out.comp_shape != obj.comp_shape:
                        msg = f"Incompatible device arrays {obj} and {out}"
                        raise ValueError(msg)
                    return self.device_smooth(obj, out, sigma, grid.periodic)
                if device:
                    return self.device_smooth(obj, obj.empty_like(), sigma, grid.periodic)
                return self.device_smooth(obj, self._smooth_work(obj.info, obj.comp_shape, 2), sigma, grid.periodic).get_valid(stream=self.stream)
            if not (served and _device_field(obj)) or isinstance(out, DeviceArray):
                return _host_path(obj, sigma, out, label)
            if out is not None and out is not obj:
                assert_field_compatible(obj, out)
                if field_dtype(out) != field_dtype(obj):
                    return _host_path(obj, sigma, out, label)
            field_grid = obj.grid
            link = resident_link(obj)
            if link is not None and (link.dev_state.complex_pairs or link.dev_state.comp_shape != (obj.grid.num_axes,) * int(getattr(obj, "rank", 0))):
                return _host_path(obj, sigma, out, label)
            comp_shape = (field_grid.num_axes,) * int(getattr(obj, "rank", 0))
            staged = self._smooth_work(self.grid_info(field_grid, field_dtype(obj)), comp_shape, 2)
            if link is not None:
                src = link.dev_state
            else:
                src = staged
                with ResidentState.plain_access(obj):
                    src.set_valid(obj.data, self.stream)
            if out is obj and link is not None:
                # in place on the device: `dev_state` keeps its address (steppers hold it), the host copy stays stale, nothing moves
                self.device_smooth(src, src, sigma, field_grid.periodic)
                if label:
                    obj.label = label
                return obj
            if device:
                return self.device_smooth(src, src.empty_like(), sigma, field_grid.periodic)
            # a host result: the passes end in work array 2 (an uploaded source lies there already: in place), then one download
            res = self.device_smooth(src, staged, sigma, field_grid.periodic)
            if out is None:
                out = base_class(obj)(field_grid, "empty", label=obj.label, dtype=field_dtype(obj))
            target = link_of(out)
            if target is not None:      # a resident field as the destination: its host copy becomes the current one
                target.pull(out)
            with ResidentState.plain_access(out, write=True):
                res.get_valid(out=out.data, stream=self.stream)
            if label:
                out.label = label
            return out

        return smooth


def _host_path(obj, sigma, out, label):
    """The reference's arithmetic: the field's own method (py-pde's runs scipy, the mirror classes' the numpy restatement)."""
    return base_class(obj).smooth(obj, sigma, out=out, label=label)


# ---- module level: pde_hip.smooth(field, sigma) -----------------------------------------------------------------------------------------
def smooth(field, sigma=1, *, out=None, label=None, device: bool = False, backend="hip"):
    """``field.smooth(sigma, out=out, label=label)`` - on the device: the resident copy of a state is read where it is, host data is
    uploaded once.  ``device=True`` returns the result as a :class:`~pde_hip.device.DeviceArray` (for ``pde_hip.field_statistics``, the
    projector and the slicer of the backend) and ``out=field`` smooths a resident state in place, both without a download."""
    return backend_of(field, backend).make_smoother()(field, sigma, out=out, label=label, device=device)


# ---- the method of a resident field, answered from the device (opt-in: `device_smoothing`) ---------------------------------------------
def device_method(link, field, name: str):
    """A stand-in for ``field.smooth`` that runs on the device copy, or None (the caller then takes the reference method itself)."""
    backend = link.backend
    if name != "smooth" or not _device_field(field) or not backend._lib.has("smooth_axis") or link.dev_state.complex_pairs:
        return None
    reference = getattr(base_class(field), name)

    def method(sigma=1, *, out=None, label=None):
        return backend.make_smoother()(field, sigma, out=out, label=label)

    return functools.wraps(reference)(method)
