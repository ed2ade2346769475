"""The domains of a field where it lives: connected-component labels and their sizes - :class:`DomainsMixin` of the backend.

What a phase-separating run is asked at every interrupt - how many droplets are there, how large is each: the coarsening law - is
``scipy.ndimage.label(state.data > c0)`` followed by ``np.bincount`` (plus a host merge across periodic faces) inside a tracker callback,
and so pulls a device-resident state (:class:`~pde_hip.resident.ResidentState`) over PCIe.  ``pdehip_label_domains`` and
``pdehip_domain_sizes`` (``csrc/pdehip_label.hip``) answer on the device: the number of domains, the foreground count and one size per
domain come down; the labels stay there until they are asked for.

A labelling is all integers, so the device result EQUALS the host's: scipy's labels (numbered in the C order of each domain's first
cell) after the merge across periodic faces.  Nothing replaces a host computation silently: :func:`field_domains` is called explicitly.

Residency rules: those of :func:`pde_hip.field_histogram`.  A :class:`DeviceArray` without component axes and a real scalar field whose
device copy is the current one are labelled on the device; a field whose host copy is current (never uploaded just for this), complex
states, decomposed steppers (no resident state) and a library without the entry points take the host path with scipy, which gives equal
results by construction.  Vector fields, tensor fields and collections are refused by name: a domain is a property of ONE component.
"""

from __future__ import annotations

import ctypes as C
import itertools

import numpy as np

from .device import DeviceArray, DeviceBuffer
from .resident import backend_of, is_collection, resident_link


class FieldDomains:
    """Result of :func:`field_domains`: ``count`` domains, their ``sizes`` in cells (int64, in label order), ``volumes`` (``sizes`` times
    the cell volume), ``foreground`` cells in all, their ``fraction`` of the grid, the ``largest`` size (0 without a domain), and the
    ``labels`` (int32, the grid's shape; 0: background, 1 ... ``count``: numbered in the C order of each domain's first cell).  On the
    device path ``labels`` is downloaded on first access only and ``labels_device`` is the dense device buffer; ``on_device`` says which
    path was taken."""

    def __init__(self, count: int, foreground: int, sizes, shape, cell_volume: float, *, labels=None, labels_device=None, download=None):
        self.count, self.foreground = int(count), int(foreground)
        self.sizes = np.asarray(sizes, dtype=np.int64)
        self.shape, self.cell_volume = tuple(shape), float(cell_volume)
        self.labels_device, self._labels, self._download = labels_device, labels, download
        self.on_device = labels_device is not None

    @property
    def volumes(self) -> np.ndarray:
        return self.sizes * self.cell_volume

    @property
    def fraction(self) -> float:
        return self.foreground / float(np.prod(self.shape))

    @property
    def largest(self) -> int:
        return int(self.sizes.max()) if self.count else 0

    @property
    def labels(self) -> np.ndarray:
        if self._labels is None:
            self._labels = self._download()
        return self._labels

    def __repr__(self) -> str:
        return f"FieldDomains(count={self.count}, foreground={self.foreground}, largest={self.largest}, on_device={self.on_device})"


# ---- what both paths share -------------------------------------------------------------------------------------------------------------
def interval_bounds(dtype, threshold=0.0, above: bool = True, interval=None) -> tuple[float, float]:
    """The closed interval ``[lo, hi]`` (fp64) whose cells are the foreground.  ``data > threshold`` / ``data < threshold``: the threshold
    is converted to the FIELD'S type, as numpy converts a Python float next to an array, and closed by one step of ``np.nextafter`` in
    that type - an fp32 field compares as numpy compares it.  A threshold beyond which the type has no value is refused."""
    dtype = np.dtype(dtype)
    kind = dtype.type if np.issubdtype(dtype, np.floating) else np.float64
    if interval is not None:
        lo, hi = (float(v) for v in interval)
        if np.isnan(lo) or np.isnan(hi) or lo > hi:
            msg = f"interval={interval!r}: two numbers a <= b are needed"
            raise ValueError(msg)
        return lo, hi
    if np.isnan(threshold):
        msg = "the threshold must be a number"
        raise ValueError(msg)
    with np.errstate(over="ignore"):
        t = kind(threshold)
    end = kind(np.inf if above else -np.inf)
    if t == end:
        msg = f"threshold={threshold!r}: no {dtype.name} value lies {'above' if above else 'below'} it"
        raise ValueError(msg)
    closed = float(np.nextafter(t, end))
    return (closed, float("inf")) if above else (float("-inf"), closed)


def host_domains(mask: np.ndarray, periodic, connectivity: int = 1):
    """(labels int32, count): ``scipy.ndimage.label`` of ``mask``, the labels that touch across periodic faces (edges and corners under
    full connectivity) united, numbered by first cell."""
    from scipy import ndimage

    mask = np.asarray(mask, dtype=bool)
    ndim = mask.ndim
    full = connectivity != 1
    labels, count = ndimage.label(mask, structure=ndimage.generate_binary_structure(ndim, ndim if full else 1))
    periodic = [bool(p) for p in periodic]
    if count and any(periodic):
        root = np.arange(count + 1)

        def find(x):
            while root[x] != x:
                root[x] = root[root[x]]
                x = root[x]
            return x

        for a in range(ndim):
            if not periodic[a]:
                continue
            # the pairs across the wrap of axis a: the last layer against the first one, shifted by e along the other axes
            last, first = labels.take(mask.shape[a] - 1, axis=a), labels.take(0, axis=a)
            others = [b for b in range(ndim) if b != a]
            for e in itertools.product((-1, 0, 1) if full else (0,), repeat=ndim - 1):
                other = np.roll(first, [-x for x in e], axis=tuple(range(ndim - 1))) if ndim > 1 else first          # other[x] = first[x + e]
                ok = (last > 0) & (other > 0) & (last != other)
                for m, b in enumerate(others):
                    if e[m] and not periodic[b]:          # an open axis: x + e leaves the grid at one end
                        edge = [slice(None)] * (ndim - 1)
                        edge[m] = slice(-1, None) if e[m] > 0 else slice(0, 1)
                        ok[tuple(edge)] = False
                if not ok.any():
                    continue
                for x, y in np.unique(np.stack([last[ok], other[ok]], axis=1), axis=0):
                    rx, ry = find(x), find(y)
                    if rx != ry:
                        root[max(rx, ry)] = min(rx, ry)
        merged = np.array([find(x) for x in range(count + 1)])[labels]
        # scipy numbers by first cell, and the smallest label of a merged class is that of its first cell: ranks of the roots keep the order
        kept = np.unique(merged[merged > 0])
        remap = np.zeros(count + 1, dtype=np.int64)
        remap[kept] = np.arange(1, kept.size + 1)
        labels, count = remap[merged], int(kept.size)
    return labels.astype(np.int32), int(count)


def _refuse_components(what: str, comp_shape) -> None:
    first = ", ".join("0" for _ in comp_shape)
    msg = (f"field_domains: {what} has components {tuple(comp_shape)}; domains are those of ONE component - pass a scalar, for instance "
           f"field[{first}] (or DeviceArray.component(0))")
    raise ValueError(msg)


class DomainsMixin:
    """``make_domain_labeller`` of :class:`~pde_hip.backend.HipBackendMixin`."""

    def _label_on_device(self, dev: DeviceArray, lo: float, hi: float, connectivity: int, periodic, cell_volume: float) -> FieldDomains:
        shape = dev.info.shape
        cells = dev.info.num_cells
        labels_dev, info_dev = DeviceBuffer(4 * cells), DeviceBuffer(16)
        per = (C.c_int * len(shape))(*[int(bool(p)) for p in periodic])
        self._lib.label_domains(dev.info.ref, dev.ptr, C.c_double(lo), C.c_double(hi), int(connectivity), per, labels_dev.ptr, info_dev.ptr, self.stream)
        info = np.empty(2, dtype=np.uint64)
        self._lib.memcpy_d2h(info.ctypes.data, info_dev.ptr, 16, self.stream)          # the one read between the two calls: K sizes the second
        count = int(info[0])
        sizes = np.zeros(count, dtype=np.uint64)
        if count:
            sizes_dev = DeviceBuffer(8 * count)
            self._lib.domain_sizes(labels_dev.ptr, cells, count, sizes_dev.ptr, self.stream)
            self._lib.memcpy_d2h(sizes.ctypes.data, sizes_dev.ptr, sizes.nbytes, self.stream)
        lib, stream = self._lib, self.stream

        def download():
            host = np.empty(shape, dtype=np.int32)
            lib.memcpy_d2h(host.ctypes.data, labels_dev.ptr, host.nbytes, stream)
            return host

        return FieldDomains(count, int(info[1]), sizes, shape, cell_volume, labels_device=labels_dev, download=download)

    def make_domain_labeller(self, grid=None):
        """``label(obj, threshold=0.0, *, above=True, interval=None, connectivity=1, periodic=None) -> FieldDomains``.

        ``obj``: a :class:`DeviceArray` without component axes, or a scalar field; where it is labelled follows the rules of
        :meth:`make_histogram`.  Foreground: ``data > threshold`` (``above``), ``data < threshold`` (``above=False``) or the closed
        ``interval=(a, b)``; NaN cells are background.  ``connectivity``: 1 (faces) or the number of axes (all neighbours).  ``periodic``:
        per axis, default the grid's (all open for a bare array without a grid).  ``grid``: the grid of bare arrays; a field brings its own."""

        def label(obj, threshold=0.0, *, above: bool = True, interval=None, connectivity: int = 1, periodic=None) -> FieldDomains:
            if is_collection(obj):
                _refuse_components("a collection", (len(list(obj)),))
            field_grid = getattr(obj, "grid", None) if not isinstance(obj, DeviceArray) else None
            if field_grid is None:
                field_grid = grid
            # (not `device_source`: the refusals below, and the shape and type of the host path, read the device array whether or not
            # the kernels take it)
            dev = obj if isinstance(obj, DeviceArray) else None
            link = None if dev is not None else resident_link(obj)
            if link is not None:
                dev = link.dev_state
            if dev is not None:
                if dev.complex_pairs and dev.comp_shape == (2,):
                    pass                                    # a complex scalar state: the host path below decides
                elif dev.comp_shape:
                    _refuse_components("the state", dev.comp_shape)
            elif getattr(obj, "rank", 0):
                _refuse_components(f"a rank-{obj.rank} field", (field_grid.dim,) * obj.rank if field_grid is not None else (obj.rank,))
            if dev is not None:
                shape, dtype = dev.info.shape, dev.host_dtype
            else:
                data = np.asarray(getattr(obj, "data", obj))
                shape, dtype = data.shape, data.dtype
                if field_grid is not None and data.ndim != len(field_grid.shape):
                    _refuse_components("the array", data.shape[: data.ndim - len(field_grid.shape)])
            ndim = len(shape)
            if connectivity not in (1, ndim):
                msg = f"connectivity={connectivity!r}: 1 (faces) or {ndim} (all neighbours) on a {ndim}-D grid"
                raise ValueError(msg)
            if periodic is None:
                periodic = list(field_grid.periodic) if field_grid is not None else [False] * ndim
            periodic = [bool(p) for p in np.broadcast_to(np.asarray(periodic, dtype=bool), (ndim,))]
            cell_volume = float(np.prod(field_grid.discretization)) if field_grid is not None else (float(np.prod(dev.info.dx)) if dev is not None else 1.0)
            is_complex = np.issubdtype(dtype, np.complexfloating)
            if not is_complex:
                lo, hi = interval_bounds(dtype, threshold, above, interval)
                if dev is not None and not dev.complex_pairs and self._lib.has("label_domains", "domain_sizes"):
                    return self._label_on_device(dev, lo, hi, connectivity, periodic, cell_volume)
            data = dev.get_valid(stream=self.stream) if isinstance(obj, DeviceArray) else np.asarray(getattr(obj, "data", obj))
            with np.errstate(invalid="ignore"):
                if is_complex:          # numpy's own (lexicographic) comparison of complex numbers
                    mask = (data >= interval[0]) & (data <= interval[1]) if interval is not None else (data > threshold if above else data < threshold)
                else:
                    mask = (data >= lo) & (data <= hi)
            labels, count = host_domains(mask, periodic, connectivity)
            sizes = np.bincount(labels.ravel(), minlength=count + 1)[1:]
            return FieldDomains(count, int(np.count_nonzero(mask)), sizes, shape, cell_volume, labels=labels)

        return label


# ---- module level ----------------------------------------------------------------------------------------------------------------------
def field_domains(state, threshold=0.0, *, above: bool = True, interval=None, connectivity: int = 1, periodic=None, backend="hip") -> FieldDomains:
    """The domains of ``state`` (a py-pde or a mirror scalar field, or a :class:`DeviceArray`) - on the device while its state is resident
    there, else on the host: ``pde_hip.field_domains(state).sizes`` inside a tracker costs one number per droplet instead of the state."""
    return backend_of(state, backend).make_domain_labeller()(state, threshold, above=above, interval=interval, connectivity=connectivity,
                                                              periodic=periodic)
