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

``properties=True`` adds where every domain is, what box it fills and how much of the field it holds (``scipy.ndimage.center_of_mass``,
``find_objects``, ``sum_labels``).  ``pdehip_domain_properties`` (``csrc/pdehip_props.hip``) and :func:`host_domain_properties` give the same
INTEGERS per domain - the anchor (first cell), the sums and extremes of the cells' offsets from it (minimal image on periodic axes) and a
fixed-point sum of the field in two 64-bit limbs - and ONE function, :func:`derive_properties`, turns them into centroids, boxes and sums:
the device and the host path agree bit for bit.
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

    def __getattr__(self, name: str):
        # (only called for names that are not there: the per-domain properties live in ``_props``)
        if name in PROPERTY_NAMES:
            props = self.__dict__.get("_props")
            if props is None:
                msg = f"FieldDomains.{name} needs the per-domain properties: call field_domains(..., properties=True)"
                raise AttributeError(msg)
            if props.get(name) is None:
                msg = f"FieldDomains.{name}: the properties were computed without a real field, there are no sums"
                raise AttributeError(msg)
            return props[name]
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    def __repr__(self) -> str:
        return f"FieldDomains(count={self.count}, foreground={self.foreground}, largest={self.largest}, on_device={self.on_device})"


PROPERTY_NAMES = ("anchors", "moments", "boxes", "limbs", "excluded", "centroids", "positions", "bounding_boxes", "extents", "ambiguous",
                  "sums", "means", "radii", "touches_boundary")
_INT32_MAX, _INT32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min
ABSMAX_LIMIT = float(np.nextafter(2.0 ** 1023, 0.0))          # pdehip_domain_properties takes absmax < 2^1023


# ---- what both paths share -------------------------------------------------------------------------------------------------------------
def limb_exponents(ncells: int, absmax: float) -> tuple[int, int]:
    """``(eh, el)``: a cell value ``v`` with ``|v| <= absmax`` is ``hi * 2^eh + lo * 2^el`` up to ``2^(el - 1)`` with ``|hi| <= 2^(62 - L)``
    and ``|lo| <= 2^30``, ``L = ceil(log2(ncells))``: the 64-bit sums of ``hi`` and of ``lo`` over up to ``ncells`` cells cannot overflow."""
    level = max(int(ncells) - 1, 0).bit_length()
    eh = int(np.frexp(float(absmax))[1]) - (62 - level)
    return eh, eh - 31


def finite_absmax(data) -> float:
    """The largest magnitude among the finite cells (0 without one), as the device statistics give it; at most :data:`ABSMAX_LIMIT`."""
    data = np.asarray(data)
    finite = data[np.isfinite(data)]
    if not finite.size:
        return 0.0
    return min(max(abs(float(finite.min())), abs(float(finite.max()))), ABSMAX_LIMIT)


def host_domain_properties(labels, data=None, periodic=None, absmax: float | None = None, count: int | None = None) -> dict:
    """The integers of ``pdehip_domain_properties`` (``include/pdehip.h``) in numpy, for ``labels`` (0: background, 1 ... K) of a grid of one
    to three axes: ``anchor`` (K, int32), ``moment`` (K x 3, int64), ``box`` (K x 3 x 2, int32) and, with real ``data``, ``limb`` (K x 2,
    int64) and ``excluded`` (K, uint32), else None.  Axes are normalised to three like the kernels do.  Every sum is an int64 sum
    (sort and ``np.add.reduceat``), never a floating-point one."""
    labels = np.asarray(labels)
    shape = labels.shape
    ndim = len(shape)
    if not 1 <= ndim <= 3:
        msg = f"labels of a grid of one to three axes are needed (got shape {shape})"
        raise ValueError(msg)
    shape3 = (1,) * (3 - ndim) + tuple(shape)
    per3 = [False] * (3 - ndim) + [bool(p) for p in (np.broadcast_to(np.asarray(periodic, dtype=bool), (ndim,)) if periodic is not None else [False] * ndim)]
    flat = labels.ravel()
    k = int(flat.max(initial=0)) if count is None else int(count)
    bad = int(np.count_nonzero((flat < 0) | (flat > k)))
    if bad:
        msg = f"domain_properties: {bad} cells have a label outside 0 ... {k}"
        raise ValueError(msg)
    cells = np.flatnonzero(flat)                                     # ascending: C order
    order = np.argsort(flat[cells], kind="stable")
    cells = cells[order]
    lab = flat[cells].astype(np.int64) - 1
    present, starts = np.unique(lab, return_index=True)
    anchor = np.full(k, _INT32_MAX, dtype=np.int32)
    moment = np.zeros((k, 3), dtype=np.int64)
    box = np.empty((k, 3, 2), dtype=np.int32)
    box[:, :, 0], box[:, :, 1] = _INT32_MAX, _INT32_MIN
    have_field = data is not None and not np.iscomplexobj(data)
    limb = np.zeros((k, 2), dtype=np.int64) if have_field else None
    excluded = np.zeros(k, dtype=np.uint32) if have_field else None
    out = {"anchor": anchor, "moment": moment, "box": box, "limb": limb, "excluded": excluded}
    if not cells.size:
        return out
    anchor[present] = cells[starts]                                  # (stable sort: the first cell of a label is its smallest)
    index = np.unravel_index(cells, shape3)
    at = np.unravel_index(anchor[lab].astype(np.int64), shape3)
    for a in range(3):
        d = index[a].astype(np.int64) - at[a]
        if per3[a]:
            h = shape3[a] // 2
            d = (d + h) % shape3[a] - h
        moment[present, a] = np.add.reduceat(d, starts)
        box[present, a, 0] = np.minimum.reduceat(d, starts)
        box[present, a, 1] = np.maximum.reduceat(d, starts)
    if have_field:
        data = np.asarray(data)
        if data.shape != shape:
            msg = f"the field has shape {data.shape}, the labels {shape}"
            raise ValueError(msg)
        absmax = finite_absmax(data) if absmax is None else float(absmax)
        eh, el = limb_exponents(flat.size, absmax)
        v = data.ravel()[cells].astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok = np.abs(v) <= absmax
        v = np.where(ok, v, 0.0)
        hi = np.rint(np.ldexp(v, -eh))
        lo = np.rint(np.ldexp(v - np.ldexp(hi, eh), -el))
        limb[present, 0] = np.add.reduceat(hi.astype(np.int64), starts)
        limb[present, 1] = np.add.reduceat(lo.astype(np.int64), starts)
        excluded[present] = np.add.reduceat((~ok).astype(np.int64), starts).astype(np.uint32)
    return out


def derive_properties(raw: dict, sizes, shape, periodic, lower, dx, absmax: float) -> dict:
    """What both paths derive in fp64 from the integers of one labelling (``raw``: :func:`host_domain_properties`): every attribute of
    :data:`PROPERTY_NAMES`, with one row per domain and one column per axis of the grid."""
    ndim = len(shape)
    n = np.asarray(shape, dtype=np.int64)
    per = np.asarray([bool(p) for p in periodic], dtype=bool)
    lower, dx = np.asarray(lower, dtype=np.float64), np.asarray(dx, dtype=np.float64)
    sizes = np.asarray(sizes, dtype=np.int64)
    anchors = raw["anchor"]
    moments = np.ascontiguousarray(raw["moment"][:, 3 - ndim:])
    boxes = np.ascontiguousarray(raw["box"][:, 3 - ndim:, :])
    where = np.where(sizes > 0, anchors, 0).astype(np.int64)
    at = np.stack(np.unravel_index(where, shape), axis=1).astype(np.int64).reshape(-1, ndim)
    with np.errstate(invalid="ignore", divide="ignore"):
        # i(anchor) + moment / size with ONE rounding: the numerator is an integer (below 2^63: sizes and indices are below 2^31)
        centroids = (at * sizes[:, None] + moments).astype(np.float64) / sizes[:, None].astype(np.float64)
        centroids = np.where(per[None, :], np.mod(centroids, n[None, :].astype(np.float64)), centroids)
        bounding = at[:, :, None] + boxes.astype(np.int64)
        extents = boxes[:, :, 1].astype(np.int64) - boxes[:, :, 0].astype(np.int64) + 1
        out = {"anchors": anchors, "moments": moments, "boxes": boxes, "limbs": raw["limb"], "excluded": raw["excluded"],
               "centroids": centroids, "positions": lower[None, :] + (centroids + 0.5) * dx[None, :], "bounding_boxes": bounding,
               "extents": extents, "ambiguous": per[None, :] & (2 * extents > n[None, :]),
               "touches_boundary": np.any(~per[None, :] & ((bounding[:, :, 0] <= 0) | (bounding[:, :, 1] >= n[None, :] - 1)), axis=1),
               "sums": None, "means": None}
        volume = sizes.astype(np.float64) * float(np.prod(dx))
        out["radii"] = (0.5 * volume, np.sqrt(volume / np.pi), np.cbrt(0.75 * volume / np.pi))[ndim - 1]
        if raw["limb"] is not None:
            eh, el = limb_exponents(int(np.prod(n)), absmax)
            sums = np.ldexp(raw["limb"][:, 0].astype(np.float64), eh) + np.ldexp(raw["limb"][:, 1].astype(np.float64), el)
            out["sums"] = np.where(raw["excluded"] > 0, np.nan, sums)
            out["means"] = out["sums"] / sizes.astype(np.float64)
    return out


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


def _geometry(grid, dx, ndim: int):
    """(lower bounds, cell sizes) per axis: the grid's, else those of a device array from 0, else unit cells from 0."""
    if grid is not None:
        return [float(b[0]) for b in grid.axes_bounds], [float(d) for d in grid.discretization]
    return [0.0] * ndim, [float(d) for d in dx] if dx is not None else [1.0] * ndim


def _refuse_components(what: str, comp_shape) -> None:
    first = ", ".join("0" for _ in comp_shape)
    msg = (f"field_domains: {what} has components {tuple(comp_shape)}; domains are those of ONE component - pass a scalar, for instance "
           f"field[{first}] (or DeviceArray.component(0))")
    raise ValueError(msg)


class DomainsMixin:
    """``make_domain_labeller`` of :class:`~pde_hip.backend.HipBackendMixin`."""

    def _properties_on_device(self, shape, dtype, labels_dev, count: int, periodic, dev: DeviceArray | None, absmax: float) -> dict:
        """The integers of ``pdehip_domain_properties`` for the dense device labels ``labels_dev`` (72 bytes per domain come down)."""
        raw = {"anchor": np.empty(count, dtype=np.int32), "moment": np.empty((count, 3), dtype=np.int64), "box": np.empty((count, 3, 2), dtype=np.int32),
               "limb": np.empty((count, 2), dtype=np.int64) if dev is not None else None,
               "excluded": np.empty(count, dtype=np.uint32) if dev is not None else None}
        if not count:
            return raw
        info = dev.info if dev is not None else self._props_info(shape, dtype)
        bufs = {key: DeviceBuffer(max(arr.nbytes, 8)) for key, arr in raw.items() if arr is not None}
        per = (C.c_int * len(shape))(*[int(bool(p)) for p in periodic])
        self._lib.domain_properties(info.ref, dev.ptr if dev is not None else None, labels_dev.ptr, count, per, C.c_double(absmax),
                                    bufs["anchor"].ptr, bufs["moment"].ptr, bufs["box"].ptr, bufs["limb"].ptr if dev is not None else None,
                                    bufs["excluded"].ptr if dev is not None else None, self.stream)
        for key, buf in bufs.items():
            self._lib.memcpy_d2h(raw[key].ctypes.data, buf.ptr, raw[key].nbytes, self.stream)
        return raw

    @staticmethod
    def _props_info(shape, dtype):
        from .device import GridInfo

        return GridInfo(shape, (1.0,) * len(shape), dtype)

    def _device_absmax(self, dev: DeviceArray) -> float:
        """max(|min|, |max|) over the finite cells from the device statistics of the same array: one more download of 16 bytes."""
        out = DeviceBuffer(64)
        self._lib.field_stats(dev.info.ref, 1, dev.ptr, 0, 0, out.ptr, self.stream)
        ends = np.empty(2, dtype=np.float64)
        self._lib.memcpy_d2h(ends.ctypes.data, out.ptr + 24, 16, self.stream)
        return 0.0 if np.isnan(ends).any() else min(max(abs(float(ends[0])), abs(float(ends[1]))), ABSMAX_LIMIT)

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
        """``label(obj, threshold=0.0, *, above=True, interval=None, connectivity=1, periodic=None, properties=False) -> FieldDomains``.

        ``obj``: a :class:`DeviceArray` without component axes, or a scalar field; where it is labelled follows the rules of
        :meth:`make_histogram`.  Foreground: ``data > threshold`` (``above``), ``data < threshold`` (``above=False``) or the closed
        ``interval=(a, b)``; NaN cells are background.  ``connectivity``: 1 (faces) or the number of axes (all neighbours).  ``periodic``:
        per axis, default the grid's (all open for a bare array without a grid).  ``grid``: the grid of bare arrays; a field brings its own.
        ``properties``: also the per-domain attributes of :data:`PROPERTY_NAMES` (module docstring); False is the call without them."""

        def label(obj, threshold=0.0, *, above: bool = True, interval=None, connectivity: int = 1, periodic=None, properties: bool = False) -> FieldDomains:
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
                    found = self._label_on_device(dev, lo, hi, connectivity, periodic, cell_volume)
                    if properties:
                        lower, dx = _geometry(field_grid, dev.info.dx, ndim)
                        if self._lib.has("domain_properties", "field_stats"):
                            absmax = self._device_absmax(dev)
                            raw = self._properties_on_device(shape, dtype, found.labels_device, found.count, periodic, dev, absmax)
                        else:          # a library without the entry point: the labels and the state come down, as for scipy
                            host = dev.get_valid(stream=self.stream) if isinstance(obj, DeviceArray) else np.asarray(obj.data)
                            absmax = finite_absmax(host)
                            raw = host_domain_properties(found.labels, host, periodic, absmax, found.count)
                        found._props = derive_properties(raw, found.sizes, shape, periodic, lower, dx, absmax)
                    return found
            data = dev.get_valid(stream=self.stream) if isinstance(obj, DeviceArray) else np.asarray(getattr(obj, "data", obj))
            with np.errstate(invalid="ignore"):
                if is_complex:          # numpy's own (lexicographic) comparison of complex numbers
                    mask = (data >= interval[0]) & (data <= interval[1]) if interval is not None else (data > threshold if above else data < threshold)
                else:
                    mask = (data >= lo) & (data <= hi)
            labels, count = host_domains(mask, periodic, connectivity)
            sizes = np.bincount(labels.ravel(), minlength=count + 1)[1:]
            found = FieldDomains(count, int(np.count_nonzero(mask)), sizes, shape, cell_volume, labels=labels)
            if properties:
                lower, dx = _geometry(field_grid, dev.info.dx if dev is not None else None, ndim)
                absmax = 0.0 if is_complex else finite_absmax(data)
                raw = host_domain_properties(labels, None if is_complex else data, periodic, absmax, count)          # (complex: no sums)
                found._props = derive_properties(raw, found.sizes, shape, periodic, lower, dx, absmax)
            return found

        return label


# ---- module level ----------------------------------------------------------------------------------------------------------------------
def field_domains(state, threshold=0.0, *, above: bool = True, interval=None, connectivity: int = 1, periodic=None, properties: bool = False,
                  backend="hip") -> FieldDomains:
    """The domains of ``state`` (a py-pde or a mirror scalar field, or a :class:`DeviceArray`) - on the device while its state is resident
    there, else on the host: ``pde_hip.field_domains(state).sizes`` inside a tracker costs one number per droplet instead of the state.
    ``properties=True``: also ``centroids``, ``positions``, ``bounding_boxes``, ``sums``, ... per domain (:data:`PROPERTY_NAMES`)."""
    label = backend_of(state, backend).make_domain_labeller()
    if not properties:
        return label(state, threshold, above=above, interval=interval, connectivity=connectivity, periodic=periodic)
    return label(state, threshold, above=above, interval=interval, connectivity=connectivity, periodic=periodic, properties=True)


def domain_properties(labels, field=None, *, periodic=None, grid=None, backend="hip") -> FieldDomains:
    """The per-domain properties (:data:`PROPERTY_NAMES`) of labels the caller already holds: a :class:`FieldDomains`, a dense device
    label buffer (:class:`~pde_hip.device.DeviceBuffer`; ``grid`` gives its shape) or an integer numpy array (0: background).  ``field``:
    the field whose sums are wanted (a scalar field, a :class:`DeviceArray` or a numpy array; None: no sums).  On the device where the
    labels are there and the field is a device array or resident; else on the host.  A bare label buffer is downloaded once for its
    count and sizes.  ``periodic`` defaults to the grid's, ``grid`` to the field's."""
    if is_collection(field):
        _refuse_components("a collection", (len(list(field)),))
    if grid is None and field is not None and not isinstance(field, (DeviceArray, np.ndarray)):
        grid = getattr(field, "grid", None)
    found = labels if isinstance(labels, FieldDomains) else None
    labels_dev = found.labels_device if found is not None else (labels if isinstance(labels, DeviceBuffer) else None)
    if found is not None:
        shape = found.shape
    elif labels_dev is not None:
        if grid is None:
            msg = "domain_properties: grid= is needed for the shape of a device label buffer"
            raise ValueError(msg)
        shape = tuple(int(n) for n in grid.shape)
    else:
        shape = np.asarray(labels).shape
    ndim = len(shape)
    be = backend_of(field, backend) if labels_dev is not None or (field is not None and not isinstance(field, np.ndarray)) else None
    dev = None
    if be is not None and field is not None:
        dev = field if isinstance(field, DeviceArray) else (resident_link(field).dev_state if resident_link(field) is not None else None)
        if dev is not None and (dev.comp_shape or dev.complex_pairs):
            if not dev.complex_pairs:
                _refuse_components("the state", dev.comp_shape)
            dev = None
    if periodic is None:
        periodic = list(grid.periodic) if grid is not None else [False] * ndim
    periodic = [bool(p) for p in np.broadcast_to(np.asarray(periodic, dtype=bool), (ndim,))]
    lower, dx = _geometry(grid, dev.info.dx if dev is not None else None, ndim)
    cell_volume = float(np.prod(dx))
    if found is None:
        if labels_dev is not None:
            from ._lib import get_lib

            host_labels = np.empty(shape, dtype=np.int32)
            get_lib().memcpy_d2h(host_labels.ctypes.data, labels_dev.ptr, host_labels.nbytes, be.stream if be is not None else None)
        else:
            host_labels = np.ascontiguousarray(labels)
            if not np.issubdtype(host_labels.dtype, np.integer):
                msg = f"domain_properties: integer labels are needed (got {host_labels.dtype})"
                raise ValueError(msg)
        count = int(host_labels.max(initial=0))
        if int(host_labels.min(initial=0)) < 0:
            msg = "domain_properties: labels must not be negative"
            raise ValueError(msg)
        sizes = np.bincount(host_labels.ravel(), minlength=count + 1)[1:]
        found = FieldDomains(count, int(sizes.sum()), sizes, shape, cell_volume, labels=host_labels.astype(np.int32, copy=False), labels_device=labels_dev)
    else:
        found = FieldDomains(found.count, found.foreground, found.sizes, shape, found.cell_volume, labels=found._labels,
                             labels_device=labels_dev, download=found._download)
    on_device = (labels_dev is not None and be._lib.has("domain_properties", "field_stats")
                 and (field is None or (dev is not None and tuple(dev.info.shape) == tuple(shape))))
    if on_device:
        absmax = be._device_absmax(dev) if dev is not None else 0.0
        raw = be._properties_on_device(shape, dev.host_dtype if dev is not None else np.float64, labels_dev, found.count, periodic, dev, absmax)
    else:
        data = None
        if field is not None:
            data = dev.get_valid(stream=be.stream) if isinstance(field, DeviceArray) else np.asarray(getattr(field, "data", field))
            if data.shape != tuple(shape):
                _refuse_components("the field", data.shape[: max(data.ndim - ndim, 0)] or data.shape)
        real = data is not None and not np.iscomplexobj(data)
        absmax = finite_absmax(data) if real else 0.0
        raw = host_domain_properties(found.labels, data if real else None, periodic, absmax, found.count)
    found._props = derive_properties(raw, found.sizes, shape, periodic, lower, dx, absmax)
    return found
