"""The structure factor of a field where it lives: the power spectrum summed over shells of \\|k\\| and the length scale that follows from
it - :class:`SpectrumMixin` of the backend.

The measurement a Cahn-Hilliard or pattern-forming run is judged by is the radially averaged power spectrum S(\\|k\\|).  On the host that is
``np.fft.fftn(state.data)`` inside a tracker callback: a device-resident state (:class:`~pde_hip.resident.ResidentState`) comes over PCIe
and is transformed there at every interrupt.  ``pdehip_shell_spectrum`` (``csrc/pdehip_fft.hip``) transforms and sums on the device: a few
kilobytes come down.

Definition (frequencies, no factor 2 pi): the density of mode k is ``|fftn(data) / data.size|**2 / prod(dx)`` at
``|k| = sqrt(sum_a fftfreq(n_a, dx_a)**2)``; ``power`` of a shell is the sum of the density over the modes inside it, ``density`` of a shell
their mean.  The device sums ``|F|**2`` over the Hermitian half with the mirror images weighted in; the factor ``1 / (size**2 prod(dx))`` is
applied here.

Residency rules: those of :meth:`~pde_hip.statistics.StatisticsMixin.make_statistics`.  A :class:`DeviceArray` and a field whose device
copy is the current one are transformed on the device; a field whose host copy is current (never uploaded just for this), complex states,
decomposed steppers (no resident state), a library without the entry points and a grid the transform does not take (an extent that is not a
power of two, or beyond 1024 cells - 4096 on the last axis) take the host path with numpy, with the same meaning; none of them is an
error.  Collections and curvilinear grids are refused by name.
"""

from __future__ import annotations

import operator
from typing import NamedTuple

import numpy as np

from . import _abi
from .device import DeviceArray, DeviceBuffer
from .distribution import BINS_MAX, _explicit_edges
from .resident import backend_of, device_source, is_collection

NEEDS = ("fft_supported", "shell_spectrum")


class ShellTail(NamedTuple):
    """What lies outside the edges: ``counts`` modes (int) and their ``power`` (component shape)."""

    counts: int
    power: np.ndarray


class FieldSpectrum:
    """Result of :func:`field_spectrum`.  ``edges``: the ``nbins + 1`` edges of the shells in \\|k\\| (bin ``i`` holds the modes with
    ``edges[i] <= |k| < edges[i + 1]``, the last bin also ``|k| == edges[-1]``); ``k``: the centres (for the default shells ``i * dk``,
    bin 0 being the zero mode alone; else the midpoints); ``counts`` (int64): the modes per shell; ``power``, shape of the field's
    components followed by ``(nbins,)``: the sum of the density over the shell; ``below`` / ``above``: modes and power outside the edges."""

    def __init__(self, edges, k, counts, power, below: ShellTail, above: ShellTail, *, cell_volume: float, default_shells: bool, on_device: bool):
        self.edges, self.k = np.asarray(edges, dtype=np.float64), np.asarray(k, dtype=np.float64)
        self.counts, self.power = np.asarray(counts, dtype=np.int64), np.asarray(power, dtype=np.float64)
        self.below, self.above = below, above
        self.cell_volume, self.default_shells, self.on_device = float(cell_volume), bool(default_shells), bool(on_device)

    @property
    def density(self) -> np.ndarray:
        """The mean density of the modes of every shell, ``power / counts``; NaN where a shell is empty."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.counts > 0, self.power / np.where(self.counts > 0, self.counts, 1), np.nan)

    @property
    def total(self) -> np.ndarray:
        """The power of all modes, per component.  By Parseval ``total * prod(dx)`` is the mean square of the field."""
        return self.power.sum(axis=-1) + self.below.power + self.above.power

    def _without_zero_mode(self) -> slice:
        if self.default_shells:
            return slice(1, None)
        if self.edges[0] > 0:
            return slice(None)
        msg = ("k_peak, mean_wavenumber and length_scale leave out the zero mode: they are defined for the default shells (without bin 0) "
               "and for explicit edges with edges[0] > 0")
        raise ValueError(msg)

    @property
    def k_peak(self) -> np.ndarray:
        """The centre of the shell with the largest power, per component (the zero mode left out); NaN without such a shell."""
        part = self._without_zero_mode()
        k, power = self.k[part], self.power[..., part]
        if k.size == 0:
            return np.full(power.shape[:-1], np.nan)[()]
        return k[np.argmax(power, axis=-1)]

    @property
    def mean_wavenumber(self) -> np.ndarray:
        """``sum k power / sum power`` over the shells, the zero mode left out."""
        part = self._without_zero_mode()
        k, power = self.k[part], self.power[..., part]
        with np.errstate(invalid="ignore", divide="ignore"):
            return (k * power).sum(axis=-1) / power.sum(axis=-1)

    @property
    def length_scale(self) -> np.ndarray:
        """``1 / mean_wavenumber``."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return 1.0 / np.asarray(self.mean_wavenumber)

    def __repr__(self) -> str:
        return f"FieldSpectrum(nbins={self.counts.size}, k={self.k}, power={self.power}, on_device={self.on_device})"


# ---- what both paths share -------------------------------------------------------------------------------------------------------------
def axis_frequencies(shape, dx) -> list[np.ndarray]:
    """numpy's own ``np.fft.fftfreq(n_a, dx_a)`` per axis (numpy multiplies by a reciprocal: these values, and no others, define |k|)."""
    return [np.fft.fftfreq(int(n), float(d)).astype(np.float64) for n, d in zip(shape, dx)]


def _largest_k(freqs) -> float:
    sq = [float(np.max(f * f)) for f in freqs]
    while len(sq) < 3:
        sq.insert(0, 0.0)
    return float(np.sqrt((sq[0] + sq[1]) + sq[2]))


def default_edges(shape, dx) -> tuple[np.ndarray, np.ndarray]:
    """(edges, centres) of the shells of width ``dk = min_a 1 / (n_a dx_a)``: edges ``(i - 1/2) dk`` with the first edge 0, up to the
    largest \\|k\\|; centres ``i dk``.  Bin 0 holds the zero mode alone."""
    dk = min(1.0 / (int(n) * float(d)) for n, d in zip(shape, dx))
    kmax = _largest_k(axis_frequencies(shape, dx))
    nbins = int(np.ceil(kmax / dk + 0.5))
    if (nbins - 0.5) * dk <= kmax * (1.0 + 1e-12):
        nbins += 1
    if nbins > BINS_MAX:
        msg = f"the default shells of width {dk:g} up to |k| = {kmax:g} are {nbins}, at most {BINS_MAX}: pass explicit edges as `bins`"
        raise ValueError(msg)
    i = np.arange(nbins + 1, dtype=np.float64)
    edges = (i - 0.5) * dk
    edges[0] = 0.0
    return edges, i[:-1] * dk


def shell_edges(bins, shape, dx) -> tuple[np.ndarray, np.ndarray, bool]:
    """(edges, centres, default shells?) for the ``bins`` argument: None, a number of equal bins from 0 to the largest \\|k\\|, or edges
    (the rules of :func:`pde_hip.distribution._explicit_edges`)."""
    if bins is None:
        return (*default_edges(shape, dx), True)
    edges = _explicit_edges(bins)
    if edges is None:
        kmax = _largest_k(axis_frequencies(shape, dx))
        top = kmax * (1.0 + 1e-12) if kmax > 0 else 1.0
        edges = np.linspace(0.0, top, operator.index(bins) + 1)
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    return edges, 0.5 * (edges[:-1] + edges[1:]), False


def _slots(kk: np.ndarray, edges: np.ndarray) -> np.ndarray:
    """The slot of every \\|k\\|: the bin by ``pdehip_histogram``'s rule, ``nbins`` below the first edge, ``nbins + 1`` above the last."""
    nbins = edges.size - 1
    idx = np.minimum(np.searchsorted(edges, kk, side="right") - 1, nbins - 1)
    idx = np.where(kk < edges[0], nbins, idx)
    return np.where(kk > edges[-1], nbins + 1, idx)


def host_shells(data: np.ndarray, lead: int, dx, edges: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(counts ``(nbins + 2,)``, sums of ``|F|**2`` as ``(components, nbins + 2)``) with numpy: ``np.fft.rfftn`` in fp64 over the Hermitian
    half with the mirror images weighted in (complex data: ``np.fft.fftn``, every mode once), plain sums per shell."""
    shape = data.shape[lead:]
    ndim = len(shape)
    axes = tuple(range(1, ndim + 1))
    flat = data.reshape((-1,) + shape)
    freqs = axis_frequencies(shape, dx)
    if np.iscomplexobj(flat):
        spec = np.fft.fftn(flat.astype(np.complex128), axes=axes)
        weight = np.ones(shape[-1])
    else:
        spec = np.fft.rfftn(flat.astype(np.float64), axes=axes)
        nh = shape[-1] // 2 + 1
        freqs[-1] = freqs[-1][:nh]
        kidx = np.arange(nh)
        weight = np.where((kidx > 0) & (2 * kidx < shape[-1]), 2.0, 1.0)
    sq = [np.zeros(1), np.zeros(1), np.zeros(1)]
    for a, f in enumerate(freqs):
        sq[3 - ndim + a] = f * f
    kk = np.sqrt((sq[0][:, None, None] + sq[1][None, :, None]) + sq[2][None, None, :]).reshape(spec.shape[1:])
    weights = np.broadcast_to(weight, kk.shape)
    slot = _slots(kk, edges).ravel()
    ns = edges.size + 1
    counts = np.bincount(slot, weights=weights.ravel(), minlength=ns).astype(np.int64)
    power = (spec.real * spec.real + spec.imag * spec.imag) * weights
    sums = np.stack([np.bincount(slot, weights=row.ravel(), minlength=ns) for row in power])
    return counts, sums


def _is_cartesian(grid) -> bool:
    if not all(hasattr(grid, a) for a in ("shape", "discretization", "periodic")):
        return False
    return 1 <= len(grid.shape) <= _abi.MAX_DIM and len(grid.shape) == getattr(grid, "dim", len(grid.shape))


class SpectrumMixin:
    """``make_spectrum`` of :class:`~pde_hip.backend.HipBackendMixin`."""

    def _device_shells(self, dev: DeviceArray, edges: np.ndarray):
        """(counts ``(nbins + 2,)``, sums ``(components, nbins + 2)``) of ``pdehip_shell_spectrum``."""
        ns = edges.size + 1
        kf = np.ascontiguousarray(np.concatenate(axis_frequencies(dev.info.shape, dev.info.dx)), dtype=np.float64)
        e64 = np.ascontiguousarray(edges, dtype=np.float64)
        kf_dev, edges_dev = DeviceBuffer(kf.nbytes), DeviceBuffer(e64.nbytes)
        counts_dev, sums_dev = DeviceBuffer(8 * ns), DeviceBuffer(8 * dev.ncomp * ns)
        self._lib.memcpy_h2d(kf_dev.ptr, kf.ctypes.data, kf.nbytes, self.stream)
        self._lib.memcpy_h2d(edges_dev.ptr, e64.ctypes.data, e64.nbytes, self.stream)
        self._lib.shell_spectrum(dev.info.ref, dev.ncomp, dev.ptr, kf_dev.ptr, ns - 2, edges_dev.ptr, counts_dev.ptr, sums_dev.ptr, self.stream)
        counts, sums = np.empty(ns, dtype=np.uint64), np.empty((dev.ncomp, ns), dtype=np.float64)
        self._lib.memcpy_d2h(counts.ctypes.data, counts_dev.ptr, counts.nbytes, self.stream)
        self._lib.memcpy_d2h(sums.ctypes.data, sums_dev.ptr, sums.nbytes, self.stream)
        return counts.astype(np.int64), sums

    def _fft_takes(self, dev: DeviceArray) -> bool:
        try:
            self._lib.fft_supported(dev.info.ref)
        except NotImplementedError:
            return False
        return True

    def make_spectrum(self, grid=None):
        """``spectrum(obj, bins=None) -> FieldSpectrum``.

        ``obj``: a :class:`DeviceArray` (for instance the ``device=True`` result of ``pde_hip.smooth``), or a field; where it is
        transformed follows the rules of :meth:`make_statistics`, and a grid the device transform does not take goes to the host.
        ``bins``: None for shells of width ``dk = min_a 1 / (n_a dx_a)`` around ``i dk`` (bin 0 is the zero mode alone; more than 4096
        of them is a ``ValueError`` that asks for explicit edges), the number of equal bins from 0 to the largest \\|k\\|, or a 1-D array of
        strictly increasing edges.  ``grid``: the grid of bare host arrays; a field brings its own."""

        def spectrum(obj, bins=None) -> FieldSpectrum:
            if is_collection(obj):
                msg = "field_spectrum: a collection has no spectrum of its own - pass one of its fields"
                raise TypeError(msg)
            field_grid = getattr(obj, "grid", None)
            if field_grid is None and not isinstance(obj, DeviceArray):
                field_grid = grid
            if field_grid is not None and not _is_cartesian(field_grid):
                msg = f"field_spectrum: {type(field_grid).__name__} is not a Cartesian grid - shells of |k| need plane waves"
                raise TypeError(msg)
            dev, _ = device_source(self, obj, needs=NEEDS)
            if dev is not None and not self._fft_takes(dev):
                dev = None
            if dev is not None:
                shape, dx, comp_shape = dev.info.shape, dev.info.dx, dev.comp_shape
                edges, centres, default = shell_edges(bins, shape, dx)
                counts, sums = self._device_shells(dev, edges)
            else:
                if isinstance(obj, DeviceArray):
                    data = obj.get_valid(stream=self.stream)
                    shape, dx = obj.info.shape, obj.info.dx
                else:
                    if field_grid is None:
                        msg = "make_spectrum(grid) is needed for a bare host array"
                        raise ValueError(msg)
                    data = np.asarray(getattr(obj, "data", obj))
                    shape, dx = tuple(field_grid.shape), tuple(float(d) for d in field_grid.discretization)
                lead = data.ndim - len(shape)
                comp_shape = data.shape[:lead]
                edges, centres, default = shell_edges(bins, shape, dx)
                counts, sums = host_shells(data, lead, dx, edges)
            nbins = edges.size - 1
            cells = int(np.prod(shape))
            cell_volume = float(np.prod(dx))
            power = (sums / (float(cells) ** 2 * cell_volume)).reshape(comp_shape + (nbins + 2,))
            return FieldSpectrum(edges, centres, counts[:nbins], power[..., :nbins], ShellTail(int(counts[nbins]), power[..., nbins]),
                                 ShellTail(int(counts[nbins + 1]), power[..., nbins + 1]), cell_volume=cell_volume, default_shells=default,
                                 on_device=dev is not None)

        return spectrum


# ---- module level ----------------------------------------------------------------------------------------------------------------------
def field_spectrum(state, bins=None, *, backend=None) -> FieldSpectrum:
    """The shell-summed power spectrum of ``state`` (a py-pde or a mirror field, or a :class:`DeviceArray`) - on the device while its
    state is resident there, else on the host: ``pde_hip.field_spectrum(state).length_scale`` inside a tracker costs a few kilobytes
    instead of the state and a host transform."""
    return backend_of(state, "hip" if backend is None else backend).make_spectrum()(state, bins)
