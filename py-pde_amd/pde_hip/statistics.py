"""Statistics of a field where it lives, and the steady-state test against a snapshot - :class:`StatisticsMixin` of the backend.

What a tracker asks of a running simulation - ``state.average``, ``state.fluctuations``, ``state.integral``, ``state.magnitude``, the
extrema, "has it stopped changing?" - reads ``field.data`` in the reference (``pde/fields/datafield_base.py:846-897``,
``pde/trackers/trackers.py:748-875``, ``:1006-1065``) and so pulls a device-resident state (:class:`~pde_hip.resident.ResidentState`) over
PCIe at every interrupt.  ``pdehip_field_stats`` and ``pdehip_steady_state`` (``csrc/pdehip_stats.hip``) answer on the device: 64 bytes
per component, or 16 bytes, come down.

A device sum differs from numpy's in the last bits (another order of the additions), so nothing here replaces a host computation
silently: the functions below are called explicitly, the trackers ``hip_steady_state`` / ``hip_material_conservation`` are selected by
name, and the properties of a resident field answer from the device only under the configuration key ``device_statistics``.

Host data, complex states (planar pairs: the modulus is not a per-component statistic), decomposed steppers (no resident state) and a
library without the two entry points take the host path with the reference's formulas; none of them is an error.
"""

from __future__ import annotations

import numpy as np

from .device import DeviceArray, DeviceBuffer
from .resident import DeviceOption, backend_of, device_source, kernels_take, link_of

_EMPTY_MAX = "zero-size array to reduction operation maximum which has no identity"      # numpy's message for np.max of nothing
STAT_PROPERTIES = frozenset({"integral", "average", "fluctuations", "magnitude"})
COLLECTION_PROPERTIES = frozenset({"integrals", "averages", "magnitudes"})


def _geometry(grid, info=None) -> tuple[float, float]:
    """(cell volume, grid volume) of a Cartesian grid; from the spacings of a bare device array when no grid is at hand."""
    if grid is not None:
        return float(np.prod(grid.discretization)), float(grid.volume)
    cell = float(np.prod(info.dx))
    return cell, cell * info.num_cells


# ---- the reference's formulas on host data (written from pde/fields/datafield_base.py:846-897) ------------------------------------
def host_norm(data: np.ndarray, lead: int) -> np.ndarray:
    """Norm over the ``lead`` tensor axes (``np.linalg.norm`` over them, vectorial.py:430 / tensorial.py:337)."""
    return np.linalg.norm(data, axis=0 if lead == 1 else tuple(range(lead)))


def host_integral(data: np.ndarray, lead: int, cell_volume: float):
    return (data * cell_volume).sum(axis=tuple(range(lead, data.ndim)))


def host_fluctuations(data: np.ndarray, lead: int, cell_volume: float):
    return np.std(data * np.sqrt(cell_volume), axis=tuple(range(lead, data.ndim)))


def host_magnitude(data: np.ndarray, lead: int, num_axes: int, cell_volume: float, volume: float):
    """``field.magnitude``: |average| of a scalar field, else of ``to_scalar("auto")`` - component 0 of a real vector field on one axis,
    the norm over the components otherwise."""
    if lead == 1 and num_axes == 1 and not np.iscomplexobj(data):
        data, lead = data[0], 0
    elif lead > 0:
        data, lead = host_norm(data, lead), 0
    return abs(host_integral(data, 0, cell_volume) / volume)


class FieldStatistics:
    """Result of :meth:`StatisticsMixin.make_statistics`: every entry has the shape of the field's components (``()`` for a scalar field
    and for ``norm=True``).  ``count`` / ``nonfinite``: finite and other cells; ``sum``, ``min``, ``max``, ``mean`` over the finite cells;
    ``m2`` = sum of squared deviations from ``mean`` (NaN unless asked for with ``variance=True``).

    Derived, with the reference's meaning: ``integral`` = sum x cell volume, ``average`` = integral / grid volume, ``fluctuations`` =
    sqrt(cell volume x m2 / count) (``np.std`` of the data scaled by sqrt(cell volume)), ``magnitude`` = |average| (scalar fields and
    ``norm=True``).  With non-finite cells (``nonfinite > 0``; rare) numpy's versions of the four are NaN or infinite where the device
    statistics skip those cells: they are then taken from the pulled state with the reference's own arithmetic."""

    def __init__(self, raw: np.ndarray, comp_shape: tuple[int, ...], cell_volume: float, volume: float, *, on_device: bool, host_derived: dict | None = None):
        self.on_device = on_device
        self.cell_volume, self.volume = cell_volume, volume
        raw = np.asarray(raw, dtype=np.float64).reshape(comp_shape + (8,))
        self.count, self.nonfinite = raw[..., 0].astype(np.int64), raw[..., 1].astype(np.int64)
        self.sum, self.min, self.max, self.mean, self.m2 = (raw[..., k].copy() for k in (2, 3, 4, 5, 6))
        self._host = host_derived or {}

    @property
    def integral(self):
        return self._host["integral"] if "integral" in self._host else self.sum * self.cell_volume

    @property
    def average(self):
        return self._host["average"] if "average" in self._host else self.integral / self.volume

    @property
    def fluctuations(self):
        if "fluctuations" in self._host:
            return self._host["fluctuations"]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.sqrt(self.cell_volume * self.m2 / self.count)

    @property
    def magnitude(self):
        if "magnitude" in self._host:
            return self._host["magnitude"]
        if self.sum.shape != ():
            msg = "the magnitude of a vector or tensor field is that of its norm: ask with norm=True"
            raise ValueError(msg)
        return abs(self.average)

    def __repr__(self) -> str:
        return (f"FieldStatistics(count={self.count}, nonfinite={self.nonfinite}, sum={self.sum}, min={self.min}, max={self.max}, "
                f"mean={self.mean}, m2={self.m2}, on_device={self.on_device})")


def _host_raw(values: np.ndarray, lead: int, variance: bool) -> np.ndarray:
    """The blocks of eight from host data ``(*components, *grid)``: fp64 sums over the finite cells, numpy's two-pass variance."""
    comp_shape = values.shape[:lead]
    flat = np.asarray(values, dtype=np.float64).reshape(int(np.prod(comp_shape, dtype=np.int64)), -1)
    raw = np.full((flat.shape[0], 8), np.nan)
    for c, row in enumerate(flat):
        x = row[np.isfinite(row)]
        raw[c, 0], raw[c, 1], raw[c, 2], raw[c, 7] = x.size, row.size - x.size, x.sum(), 0.0
        if x.size:
            raw[c, 3], raw[c, 4], raw[c, 5] = x.min(), x.max(), raw[c, 2] / x.size
            if variance:
                raw[c, 6] = ((x - raw[c, 5]) ** 2).sum()
    return raw.reshape(comp_shape + (8,))


_NEEDS = ("field_stats", "steady_state")


def device_usable(backend, dev: DeviceArray) -> bool:
    """Real components (no planar complex pairs) and a library that has the two entry points."""
    return kernels_take(backend, dev, _NEEDS, max_comp=None)


class StatisticsMixin:
    """``make_statistics`` and ``make_steady_state_check`` of :class:`~pde_hip.backend.HipBackendMixin`."""

    device_statistics = DeviceOption(
        """Whether ``integral`` / ``average`` / ``fluctuations`` / ``magnitude`` of a field whose state is resident on the device are
        answered there, without a download (``config["backend.hip.device_statistics"]`` with py-pde, ``backend.device_statistics = True``
        stand-alone).  Default False: a device sum differs from numpy's in the last bits, and bit-for-bit behaviour is the default.""")

    def _device_raw(self, dev: DeviceArray, norm: bool, variance: bool) -> np.ndarray:
        blocks = 1 if norm else dev.ncomp
        if blocks > 64 or dev.ncomp > 64:
            msg = f"hip backend: statistics of at most 64 components (got {dev.ncomp})"
            raise ValueError(msg)
        out = DeviceBuffer(64 * blocks)
        self._lib.field_stats(dev.info.ref, dev.ncomp, dev.ptr, int(norm), int(variance), out.ptr, self.stream)
        raw = np.empty((blocks, 8), dtype=np.float64)
        self._lib.memcpy_d2h(raw.ctypes.data, out.ptr, raw.nbytes, self.stream)
        return raw

    def make_statistics(self, grid=None):
        """``stats(obj, *, variance=False, norm=False) -> FieldStatistics``.

        ``obj``: a :class:`DeviceArray`, or a field.  A :class:`DeviceArray` and a field whose state is resident on the device with
        the device copy current (between the stepper calls of a ``backend="hip"`` run) are reduced ON THE DEVICE: ``64 x ncomp`` bytes
        come down instead of the state.  A host array, or a field whose host copy is current, is reduced on the host with the reference's
        formulas - it is never uploaded just for this - and so are complex states and everything else the kernels do not take.
        ``variance``: also the second sweep (``m2``, hence ``fluctuations``).  ``norm``: the statistics of the norm over the
        components (one value) instead of one per component.  ``grid``: the grid of bare arrays (cell volume, volume); a field brings
        its own."""

        def stats(obj, *, variance: bool = False, norm: bool = False) -> FieldStatistics:
            field_grid = getattr(obj, "grid", None)
            if field_grid is None:
                field_grid = grid
            dev, bare = device_source(self, obj, needs=_NEEDS, max_comp=None)      # (more than 64 components: refused by name below)
            if dev is None and bare:
                obj = obj.get_valid(stream=self.stream)
            if dev is not None:
                cell, volume = _geometry(field_grid, dev.info)
                comp_shape = () if norm else dev.comp_shape
                raw = self._device_raw(dev, norm, variance)
                host_derived = None
                if raw[:, 1].any():
                    # non-finite cells: numpy's derived quantities differ from the finite-cell statistics; take them from the pulled state
                    data = dev.get_valid(stream=self.stream) if bare else np.asarray(obj.data)
                    host_derived = _derived_on_host(data, len(dev.comp_shape), len(dev.info.shape), cell, volume, norm, variance)
                return FieldStatistics(raw, comp_shape, cell, volume, on_device=True, host_derived=host_derived)
            data = np.asarray(getattr(obj, "data", obj))
            if field_grid is None:
                msg = "make_statistics(grid) is needed for the statistics of a bare host array"
                raise ValueError(msg)
            num_axes = len(field_grid.shape)
            lead = data.ndim - num_axes
            cell, volume = _geometry(field_grid)
            if np.iscomplexobj(data):
                # complex data: numpy's own reductions; the blocks of eight describe the modulus
                derived = _derived_on_host(data, lead, num_axes, cell, volume, norm, True)
                values = np.abs(host_norm(data, lead) if norm and lead else data)
            else:
                values = host_norm(data, lead) if norm and lead else data
                derived = _derived_on_host(data, lead, num_axes, cell, volume, norm, variance)
            vlead = 0 if norm else lead
            return FieldStatistics(_host_raw(values, vlead, variance), values.shape[:vlead], cell, volume, on_device=False, host_derived=derived)

        return stats

    def make_steady_state_check(self, atol: float = 1e-8, rtol: float = 1e-5) -> "SteadyStateCheck":
        """See :class:`SteadyStateCheck`."""
        return SteadyStateCheck(self, atol, rtol)


def _derived_on_host(data: np.ndarray, lead: int, num_axes: int, cell: float, volume: float, norm: bool, variance: bool) -> dict:
    """integral / average / fluctuations / magnitude with the reference's arithmetic on host data."""
    with np.errstate(invalid="ignore", over="ignore"):
        values, vlead = (host_norm(data, lead), 0) if norm and lead else (data, 0 if norm else lead)
        out = {"integral": host_integral(values, vlead, cell)}
        out["average"] = out["integral"] / volume
        if variance:
            out["fluctuations"] = host_fluctuations(values, vlead, cell)
        if vlead == 0:
            out["magnitude"] = abs(out["average"])
    return out


class SteadyStateCheck:
    """The test of ``SteadyStateTracker`` (pde/trackers/trackers.py:819-847) for a state that stays on the device.

    ``update(obj, t)``: the first call takes a snapshot of the state and returns None; every later call returns
    ``max(|(snapshot - state) / (t - t_snapshot)| - rtol * |state|)`` over the finite cells (NaN if any of them gives NaN, like
    ``np.max``) and moves the snapshot on, in one sweep (``pdehip_steady_state``).  ``converged(value)``: ``value <= atol``.  No finite cell:
    ``ValueError``, which is what ``np.max`` of nothing raises in the reference.

    MEMORY: the snapshot is one more array of the state's size on the device, for as long as this object lives.

    ``obj`` is a :class:`DeviceArray` or a field; a field whose host copy is the current one (or whose state the kernels do not take:
    complex pairs, a library without the entry point) is compared on the host with the same formula, the snapshot following it to
    whichever side the state is on."""

    def __init__(self, backend, atol: float = 1e-8, rtol: float = 1e-5):
        self.backend, self.atol, self.rtol = backend, float(atol), float(rtol)
        self._last = None            # DeviceArray or host array
        self._last_time: float | None = None
        self._out: DeviceBuffer | None = None

    @property
    def started(self) -> bool:
        return self._last is not None

    @property
    def on_device(self) -> bool:
        return isinstance(self._last, DeviceArray)

    def seed(self, host_data: np.ndarray, t: float) -> None:
        """Start from a snapshot somebody else took on the host."""
        self._last, self._last_time = np.array(host_data, copy=True), float(t)

    def release(self):
        """(host copy of the snapshot, its time); the check starts afresh afterwards."""
        last, t = self._last, self._last_time
        if isinstance(last, DeviceArray):
            last = last.get_valid(stream=self.backend.stream)
        self._last = self._last_time = None
        return last, t

    def converged(self, value: float) -> bool:
        return bool(value <= self.atol)

    def _device_state(self, obj):
        backend = self.backend or getattr(link_of(obj), "backend", None)      # (a tracker's check learns its backend from the state)
        if backend is None:
            return None
        dev, _ = device_source(backend, obj, needs=_NEEDS, max_comp=None)
        if dev is not None:
            self.backend = backend
        return dev

    def update(self, obj, t: float):
        dev = self._device_state(obj)
        if dev is not None:
            return self._update_device(dev, float(t))
        data = obj.get_valid(stream=self.backend.stream) if isinstance(obj, DeviceArray) else np.asarray(obj.data if hasattr(obj, "data") else obj)
        return self._update_host(data, float(t))

    def _update_device(self, dev: DeviceArray, t: float):
        lib, stream = self.backend._lib, self.backend.stream
        if self._last is None:
            self._last = dev.empty_like()
            lib.memcpy_d2d(self._last.ptr, dev.ptr, dev.nbytes, stream)
            self._last_time = t
            return None
        if not isinstance(self._last, DeviceArray):      # the snapshot was taken on the host: it follows the state to the device
            host, self._last = self._last, dev.empty_like()
            lib.memset(self._last.ptr, 0, self._last.nbytes, stream)
            self._last.set_valid(host, stream)
        if self._out is None:
            self._out = DeviceBuffer(16)
        lib.steady_state(dev.info.ref, dev.ncomp, dev.ptr, self._last.ptr, t - self._last_time, self.rtol, self._out.ptr, stream)
        self._last_time = t
        out = np.empty(2, dtype=np.float64)
        lib.memcpy_d2h(out.ctypes.data, self._out.ptr, 16, stream)
        if out[1] == 0:
            raise ValueError(_EMPTY_MAX)
        return float(out[0])

    def _update_host(self, data: np.ndarray, t: float):
        if self._last is None:
            self._last, self._last_time = data.copy(), t
            return None
        if isinstance(self._last, DeviceArray):
            self._last = self._last.get_valid(stream=self.backend.stream)
        finite = np.isfinite(data)
        rate = (self._last[finite] - data[finite]) / (t - self._last_time)
        self._last[...] = data
        self._last_time = t
        return float(np.max(np.abs(rate) - self.rtol * np.abs(data[finite])))


def field_statistics(field, *, variance: bool = False, norm: bool = False, backend="hip") -> FieldStatistics:
    """Statistics of ``field`` (a py-pde or a mirror field, or a :class:`DeviceArray`) - on the device while its state is resident
    there, else on the host: ``pde_hip.field_statistics(state, variance=True).fluctuations``."""
    return backend_of(field, backend).make_statistics()(field, variance=variance, norm=norm)


# ---- the properties of a resident field, answered from the device (opt-in: `device_statistics`) -------------------------------------
NOT_ANSWERED = object()


def _components_of(field, dev: DeviceArray):
    """[(sub-field or the field itself, its components as a DeviceArray)]: a collection is cut at its own component slices."""
    subs = getattr(field, "fields", None) or getattr(field, "_fields", None)
    if subs is None:
        return [(field, dev)]
    flat, out, start = dev.flat(), [], 0
    dim = len(dev.info.shape)
    for sub in subs:
        count = dim ** int(sub.rank)
        ptr = flat.ptr + start * flat.info.comp_elems * flat.itemsize
        out.append((sub, DeviceArray(flat.info, (dim,) * int(sub.rank), buffer=flat._buffer, ptr=ptr)))
        start += count
    return out


def device_magnitude(backend, field, dev: DeviceArray) -> float:
    """``field.magnitude`` from the device copy ``dev`` of its data (finite states; see :func:`host_magnitude` for the meaning)."""
    stats = backend.make_statistics(field.grid)
    rank, num_axes = int(field.rank), len(dev.info.shape)
    if rank == 1 and num_axes == 1:
        return float(abs(stats(dev.component(0)).average))
    return float(stats(dev, norm=rank > 0).magnitude)


def device_property(link, field, name: str):
    """Value of ``field.<name>`` from the device copy of a resident state, or NOT_ANSWERED (the caller then takes the host path)."""
    backend, dev = link.backend, link.dev_state
    if not device_usable(backend, dev):
        return NOT_ANSWERED
    parts = _components_of(field, dev)
    collection = len(parts) > 1 or parts[0][0] is not field
    if collection != (name in COLLECTION_PROPERTIES):
        return NOT_ANSWERED
    values = []
    for sub, sub_dev in parts:
        if name in ("magnitude", "magnitudes"):
            values.append(device_magnitude(backend, sub, sub_dev))
            continue
        st = backend.make_statistics(sub.grid)(sub_dev, variance=name == "fluctuations")
        value = getattr(st, {"integrals": "integral", "averages": "average"}.get(name, name))
        values.append(float(value) if np.ndim(value) == 0 else value)
    if not collection:
        return values[0]
    return np.array(values) if name == "magnitudes" else values
