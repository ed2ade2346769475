"""The distribution of a field where it lives: histograms, quantiles and the median - :class:`DistributionMixin` of the backend.

The usual analysis of a phase-separating or pattern-forming run - the order-parameter histogram, the volume fraction above a threshold,
the median, percentile colour limits - is ``np.histogram(state.data)`` or ``np.quantile(state.data, q)`` inside a tracker callback, and so
pulls a device-resident state (:class:`~pde_hip.resident.ResidentState`) over PCIe at every interrupt.  ``pdehip_histogram`` and
``pdehip_quantile_select`` (``csrc/pdehip_hist.hip``) answer on the device: a few kilobytes come down.

Counts are integers and order statistics are elements of the field, so the device results EQUAL numpy's: the counts of ``np.histogram``
for the same edges, the elements of ``np.sort`` at the ranks ``floor((n - 1) q)`` and the next one.  Nothing replaces a host computation
silently all the same: the functions below are called explicitly (numpy fields have no ``histogram`` method to take over).

Residency rules: those of :meth:`~pde_hip.statistics.StatisticsMixin.make_statistics`.  A :class:`DeviceArray` and a field whose device
copy is the current one are reduced on the device; a field whose host copy is current (never uploaded just for this), complex states,
collections, decomposed steppers (no resident state) and a library without the entry points take the host path with numpy, which gives
equal results by construction; none of them is an error.
"""

from __future__ import annotations

import ctypes as C
import operator

import numpy as np

from .device import DeviceArray, DeviceBuffer
from .resident import backend_of, device_source, is_collection

BINS_MAX = 4096
QUANTILES_PER_CALL = 8
METHODS = ("lower", "higher", "linear")


class FieldHistogram:
    """Result of :func:`field_histogram`.  ``counts`` (int64) has the shape of the field's components (``()`` for a scalar field and
    for ``norm=True``) followed by ``(nbins,)``; ``edges`` are the ``nbins + 1`` edges all components share; ``below``, ``above`` and
    ``nan`` (component shape) count the cells under the first edge, over the last one and the NaN cells, which no bin takes.  Bin ``i``
    holds the cells with ``edges[i] <= x < edges[i + 1]``, the last bin also ``x == edges[-1]`` (``np.histogram``).

    Unpacks like numpy's result: ``values, edges = field_histogram(...)``, the values being ``density`` if that was asked for."""

    def __init__(self, counts, edges, below, above, nan, *, on_device: bool, want_density: bool = False):
        self.counts, self.edges = np.asarray(counts, dtype=np.int64), np.asarray(edges)
        self.below, self.above, self.nan = (np.asarray(x, dtype=np.int64) for x in (below, above, nan))
        self.on_device, self._want_density = on_device, bool(want_density)

    @property
    def density(self) -> np.ndarray:
        """``np.histogram(..., density=True)`` from counts and edges: ``counts / widths / counts.sum()``, per component."""
        widths = np.array(np.diff(self.edges), float)
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.counts / widths / self.counts.sum(axis=-1, keepdims=True)

    def fraction_above(self, threshold):
        """The fraction of the cells that are numbers with ``x >= threshold``, per component.  ``threshold`` must be one of the edges but
        the last (a cell ON the last edge is counted in the last bin): only then do the counts decide it."""
        at = np.flatnonzero(self.edges[:-1] == threshold)
        if at.size != 1:
            msg = f"fraction_above({threshold!r}): the threshold must be one of the edges {self.edges[0]!r} ... {self.edges[-2]!r} (the last edge excluded)"
            raise ValueError(msg)
        total = self.counts.sum(axis=-1) + self.below + self.above
        with np.errstate(invalid="ignore", divide="ignore"):
            return (self.counts[..., at[0]:].sum(axis=-1) + self.above) / total

    def __iter__(self):
        yield self.density if self._want_density else self.counts
        yield self.edges

    def __repr__(self) -> str:
        return (f"FieldHistogram(counts={self.counts}, edges={self.edges}, below={self.below}, above={self.above}, nan={self.nan}, "
                f"on_device={self.on_device})")


# ---- what both paths share -------------------------------------------------------------------------------------------------------------
def _explicit_edges(bins) -> np.ndarray | None:
    """The edge array ``bins`` stands for, or None for an integer number of bins; anything else is refused by name."""
    if isinstance(bins, str):
        msg = f"bins={bins!r}: the number of bins or a 1-D array of increasing edges is needed (numpy's estimators look at all the data)"
        raise ValueError(msg)
    if np.ndim(bins) == 0:
        try:
            nbins = operator.index(bins)
        except TypeError as err:
            msg = f"bins={bins!r}: the number of bins or a 1-D array of increasing edges is needed"
            raise ValueError(msg) from err
        if nbins < 1:
            msg = "`bins` must be positive, when an integer"
            raise ValueError(msg)
        if nbins > BINS_MAX:
            msg = f"bins={nbins}: at most {BINS_MAX} bins"
            raise ValueError(msg)
        return None
    edges = np.asarray(bins)
    if edges.ndim != 1 or edges.size < 2 or np.iscomplexobj(edges) or not np.issubdtype(edges.dtype, np.number):
        msg = f"bins={bins!r}: the number of bins or a 1-D array of increasing edges is needed"
        raise ValueError(msg)
    if edges.size - 1 > BINS_MAX:
        msg = f"bins: {edges.size - 1} bins, at most {BINS_MAX}"
        raise ValueError(msg)
    e64 = edges.astype(np.float64)
    if not np.all(np.isfinite(e64)) or np.any(e64[:-1] >= e64[1:]):
        msg = "`bins` must be finite and increase strictly, when an array"
        raise ValueError(msg)
    return edges


def _equal_edges(lo, hi, nbins: int, dtype, supplied: bool) -> np.ndarray:
    """numpy's edges of ``nbins`` equal bins (``np.histogram``: ``_get_outer_edges`` and its ``np.linspace`` line)."""
    if supplied and lo > hi:
        msg = "max must be larger than min in range parameter."
        raise ValueError(msg)
    if not (np.isfinite(lo) and np.isfinite(hi)):
        msg = f"{'supplied' if supplied else 'autodetected'} range of [{lo}, {hi}] is not finite"
        raise ValueError(msg)
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    bin_type = np.result_type(lo, hi, dtype)
    if np.issubdtype(bin_type, np.integer):
        bin_type = np.result_type(bin_type, float)
    edges = np.linspace(lo, hi, nbins + 1, endpoint=True, dtype=bin_type)
    if np.any(edges[:-1] >= edges[1:]):
        msg = f"{nbins} bins between {lo} and {hi} are too narrow for {np.dtype(bin_type).name} numbers: the edges do not increase"
        raise ValueError(msg)
    return edges


def _sequential_norm(data: np.ndarray, lead: int) -> np.ndarray:
    """sqrt(x_0 * x_0 + x_1 * x_1 + ...) over the ``lead`` tensor axes in the field's type, in component order: the device's evaluation."""
    flat = data.reshape((-1,) + data.shape[lead:])
    with np.errstate(invalid="ignore", over="ignore"):
        s = flat[0] * flat[0]
        for c in range(1, flat.shape[0]):
            s = s + flat[c] * flat[c]
        return np.sqrt(s)


def _host_counts(x: np.ndarray, edges: np.ndarray, equal: bool) -> np.ndarray:
    """The ``nbins + 3`` counts of ``pdehip_histogram`` for the 1-D array ``x``; ``equal``: the edges are those of equal bins.  Complex
    data: whatever ``np.histogram`` itself makes of them (its equal bins are not found through the edges)."""
    nbins = edges.size - 1
    if np.iscomplexobj(x) or np.iscomplexobj(edges):
        nan = np.isnan(x)
        v = x[~nan]
        inside = np.histogram(v, nbins, (edges[0], edges[-1]))[0] if equal else np.histogram(v, edges)[0]
        return np.concatenate([inside, [np.count_nonzero(v < edges[0]), np.count_nonzero(v > edges[-1]), np.count_nonzero(nan)]]).astype(np.int64)
    e = edges.astype(np.float64)
    nan = np.isnan(x)
    v = x[~nan].astype(np.float64)
    inside = v[(v >= e[0]) & (v <= e[-1])]
    idx = np.minimum(np.searchsorted(e, inside, side="right") - 1, nbins - 1)
    out = np.empty(nbins + 3, dtype=np.int64)
    out[:nbins] = np.bincount(idx, minlength=nbins)
    out[nbins], out[nbins + 1], out[nbins + 2] = np.count_nonzero(v < e[0]), np.count_nonzero(v > e[-1]), np.count_nonzero(nan)
    return out


def _ranks(n: np.ndarray, q: np.ndarray):
    """(k, g) of ``pdehip_quantile_select``: v = (n - 1) q in fp64, k = floor(v), g = v - k; shapes ``n.shape + q.shape``."""
    v = (n[..., None].astype(np.float64) - 1.0) * q
    k = np.floor(v)
    return k, v - k


def _combine(lower, upper, n, nan, q, method: str, ignore_nan: bool, dtype) -> np.ndarray:
    """The quantiles ``(blocks, nq)`` from the two order statistics: ``lower`` / ``upper`` are the elements at rank k and
    min(k + 1, n - 1) among the cells that are numbers."""
    _, g = _ranks(n, q)
    lo64, up64 = lower.astype(np.float64), upper.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if method == "lower":
            out = lo64
        elif method == "higher":
            out = np.where(g > 0.0, up64, lo64)
        else:
            out = lo64 + (up64 - lo64) * g
    out = np.array(out, dtype=np.float64)
    out[n == 0] = np.nan
    if not ignore_nan:
        out[nan > 0] = np.nan
    return out.astype(dtype)


def _check_q(q) -> np.ndarray:
    q = np.asarray(q, dtype=np.float64)
    if q.ndim > 1:
        msg = "q must be a scalar or one-dimensional"
        raise ValueError(msg)
    if not np.all((q >= 0.0) & (q <= 1.0)):
        msg = "Quantiles must be in the range [0, 1]"
        raise ValueError(msg)
    return q


class DistributionMixin:
    """``make_histogram`` and ``make_quantiles`` of :class:`~pde_hip.backend.HipBackendMixin`."""

    def _distribution_source(self, obj, grid):
        """(device array or None, getter of the host data ``(*components, *grid)`` and the number of its component axes)."""
        if not is_collection(obj):      # (a collection: the host path, whatever its state)
            dev, _ = device_source(self, obj, needs=("histogram", "quantile_select", "field_stats"))
            if dev is not None:
                return dev, None

        def host():
            if isinstance(obj, DeviceArray):
                data = obj.get_valid(stream=self.stream)
                return data, data.ndim - len(obj.info.shape)
            data = np.asarray(getattr(obj, "data", obj))
            field_grid = getattr(obj, "grid", None)
            if field_grid is None:
                field_grid = grid
            if field_grid is None:
                msg = "make_histogram(grid) / make_quantiles(grid) is needed for a bare host array"
                raise ValueError(msg)
            return data, data.ndim - len(field_grid.shape)

        return None, host

    # ---- histogram ---------------------------------------------------------------------------------------------------------------------
    def _device_edges(self, dev: DeviceArray, nbins: int, range, norm: bool) -> np.ndarray:
        if range is not None:
            lo, hi = range
            return _equal_edges(lo, hi, nbins, dev.dtype, True)
        raw = self._device_raw(dev, norm, False)         # minimum and maximum on the device (pdehip_field_stats): no download
        if raw[:, 1].any():
            msg = f"autodetected range is not finite: {int(raw[:, 1].sum())} cells are NaN or infinite"
            raise ValueError(msg)
        # the extrema are elements of the field (or values of the norm in the field's type): the conversion back is exact
        return _equal_edges(dev.dtype.type(raw[:, 3].min()), dev.dtype.type(raw[:, 4].max()), nbins, dev.dtype, False)

    def _device_counts(self, dev: DeviceArray, edges: np.ndarray, norm: bool) -> np.ndarray:
        blocks, nbins = (1 if norm else dev.ncomp), edges.size - 1
        e64 = np.ascontiguousarray(edges, dtype=np.float64)
        edges_dev, counts_dev = DeviceBuffer(e64.nbytes), DeviceBuffer(8 * blocks * (nbins + 3))
        self._lib.memcpy_h2d(edges_dev.ptr, e64.ctypes.data, e64.nbytes, self.stream)
        self._lib.histogram(dev.info.ref, dev.ncomp, dev.ptr, int(norm), nbins, edges_dev.ptr, counts_dev.ptr, self.stream)
        counts = np.empty((blocks, nbins + 3), dtype=np.uint64)
        self._lib.memcpy_d2h(counts.ctypes.data, counts_dev.ptr, counts.nbytes, self.stream)
        return counts.astype(np.int64)

    def make_histogram(self, grid=None):
        """``histogram(obj, bins=10, range=None, *, density=False, norm=False) -> FieldHistogram``.

        ``obj``: a :class:`DeviceArray` (for instance the ``device=True`` result of ``pde_hip.smooth``), or a field; where it is
        reduced follows the rules of :meth:`make_statistics`.  ``bins``: the number of equal bins (at most 4096) or a 1-D array of
        strictly increasing edges; all components of a vector or tensor field share one set of edges.  ``range``: ``(lo, hi)`` of the
        equal bins; None: minimum and maximum over all components, found on the device too.  The edges are numpy's
        (``np.linspace(lo, hi, bins + 1)`` in the field's type), which is what makes the counts equal ``np.histogram``'s.  ``norm``:
        the histogram of the norm over the components.  ``grid``: the grid of bare host arrays; a field brings its own."""

        def histogram(obj, bins=10, range=None, *, density: bool = False, norm: bool = False) -> FieldHistogram:
            edges = _explicit_edges(bins)
            dev, host = self._distribution_source(obj, grid)
            if dev is not None:
                if edges is None:
                    edges = self._device_edges(dev, operator.index(bins), range, norm)
                counts = self._device_counts(dev, edges, norm)
                comp_shape = () if norm else dev.comp_shape
            else:
                data, lead = host()
                values = _sequential_norm(data, lead)[None] if norm and lead else data.reshape((-1,) + data.shape[lead:])
                comp_shape = () if norm or not lead else data.shape[:lead]
                equal = edges is None
                if equal:
                    edges = np.histogram_bin_edges(values, operator.index(bins), range)      # numpy's own edges and its own refusals
                counts = np.stack([_host_counts(row.ravel(), edges, equal) for row in values])
            nbins = edges.size - 1
            counts = counts.reshape(comp_shape + (nbins + 3,))
            return FieldHistogram(counts[..., :nbins], edges, counts[..., nbins], counts[..., nbins + 1], counts[..., nbins + 2],
                                  on_device=dev is not None, want_density=density)

        return histogram

    # ---- quantiles ---------------------------------------------------------------------------------------------------------------------
    def _device_order_statistics(self, dev: DeviceArray, q: np.ndarray, norm: bool):
        """(lower, upper) as ``(blocks, nq)`` in the field's type and (n, n_nan) as ``(blocks,)``; at most 8 values of q per call."""
        blocks = 1 if norm else dev.ncomp
        lower, upper = np.empty((2, blocks, q.size), dtype=dev.dtype)
        info = np.zeros((blocks, 2), dtype=np.uint64)
        for start in np.arange(0, q.size, QUANTILES_PER_CALL):
            part = np.ascontiguousarray(q[start:start + QUANTILES_PER_CALL])
            nbytes = blocks * part.size * dev.itemsize
            bufs = [DeviceBuffer(nbytes), DeviceBuffer(nbytes), DeviceBuffer(info.nbytes)]
            self._lib.quantile_select(dev.info.ref, dev.ncomp, dev.ptr, int(norm), part.size, part.ctypes.data_as(C.POINTER(C.c_double)), bufs[0].ptr,
                                      bufs[1].ptr, bufs[2].ptr, self.stream)
            for out, buf in zip((lower, upper), bufs):
                got = np.empty((blocks, part.size), dtype=dev.dtype)
                self._lib.memcpy_d2h(got.ctypes.data, buf.ptr, got.nbytes, self.stream)
                out[:, start:start + part.size] = got
            self._lib.memcpy_d2h(info.ctypes.data, bufs[2].ptr, info.nbytes, self.stream)
        return lower, upper, info[:, 0].astype(np.int64), info[:, 1].astype(np.int64)

    def make_quantiles(self, grid=None):
        """``quantile(obj, q, *, method="linear", norm=False, ignore_nan=False)``: the quantiles of every component over the grid, with the
        shape of ``q`` followed by the shape of the components, in the field's type.

        With n cells that are numbers, v = (n - 1) q and k = floor(v): ``"lower"`` is the k-th smallest cell, ``"higher"`` the next one
        unless v is whole, ``"linear"`` is ``lower + (upper - lower) * (v - k)`` evaluated in fp64 and rounded once to the field's type.
        A NaN cell makes the result NaN (``np.quantile``) unless ``ignore_nan`` (``np.nanquantile``).  Where the state is reduced follows
        the rules of :meth:`make_statistics`; on the device two elements per quantile and component come down."""

        def quantile(obj, q, *, method: str = "linear", norm: bool = False, ignore_nan: bool = False):
            if method not in METHODS:
                msg = f"method={method!r}: one of {', '.join(METHODS)}"
                raise ValueError(msg)
            qs = _check_q(q)
            flat_q = qs.reshape(-1)
            dev, host = self._distribution_source(obj, grid)
            if dev is not None:
                lower, upper, n, nan = self._device_order_statistics(dev, flat_q, norm)
                comp_shape, dtype = (() if norm else dev.comp_shape), dev.dtype
            else:
                data, lead = host()
                if np.iscomplexobj(data):
                    msg = "a must be an array of real numbers"          # np.quantile's refusal
                    raise TypeError(msg)
                values = _sequential_norm(data, lead)[None] if norm and lead else data.reshape((-1,) + data.shape[lead:])
                comp_shape, dtype = (() if norm or not lead else data.shape[:lead]), data.dtype
                if not np.issubdtype(dtype, np.floating):
                    values, dtype = values.astype(np.float64), np.dtype(np.float64)
                lower, upper = np.full((2, values.shape[0], flat_q.size), np.nan, dtype=dtype)
                n, nan = np.zeros((2, values.shape[0]), dtype=np.int64)
                for c, row in enumerate(values):
                    row = row.ravel()
                    ordered = np.sort(row[~np.isnan(row)])
                    n[c], nan[c] = ordered.size, row.size - ordered.size
                    if ordered.size:
                        k = _ranks(n[c:c + 1], flat_q)[0][0].astype(np.int64)
                        lower[c], upper[c] = ordered[k], ordered[np.minimum(k + 1, ordered.size - 1)]
            out = _combine(lower, upper, n, nan, flat_q, method, ignore_nan, dtype)          # (blocks, nq)
            out = np.moveaxis(out, 0, -1).reshape(qs.shape + comp_shape)
            return out[()] if out.ndim == 0 else out

        return quantile


# ---- module level ----------------------------------------------------------------------------------------------------------------------
def field_histogram(state, bins=10, range=None, *, density: bool = False, norm: bool = False, backend="hip") -> FieldHistogram:
    """Histogram of ``state`` (a py-pde or a mirror field, or a :class:`DeviceArray`) - on the device while its state is resident there,
    else on the host: ``pde_hip.field_histogram(state, 64, (-1, 1)).counts`` inside a tracker costs a few hundred bytes instead of the state."""
    return backend_of(state, backend).make_histogram()(state, bins, range, density=density, norm=norm)


def field_quantile(state, q, *, method: str = "linear", norm: bool = False, ignore_nan: bool = False, backend="hip"):
    """Quantiles of ``state`` over the grid, per component (see :meth:`DistributionMixin.make_quantiles`)."""
    return backend_of(state, backend).make_quantiles()(state, q, method=method, norm=norm, ignore_nan=ignore_nan)


def field_median(state, *, method: str = "linear", norm: bool = False, ignore_nan: bool = False, backend="hip"):
    """The median of ``state`` over the grid, per component: ``field_quantile(state, 0.5, ...)``."""
    return field_quantile(state, 0.5, method=method, norm=norm, ignore_nan=ignore_nan, backend=backend)
