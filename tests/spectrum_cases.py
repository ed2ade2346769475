"""Cases, inputs, drivers, numpy restatements and bounds for the spectrum entry points ``pdehip_fft_forward`` and
``pdehip_shell_spectrum``.

Shared by ``tests/test_spectrum_cpu.py`` (CPU: the serial C versions of the tests-only shim against numpy) and
``tests/test_hip_spectrum.py`` (GPU: the kernels of ``csrc/pdehip_fft.hip`` against the shim, bit by bit).  The shim is called directly
(``ShimCalls``) on host arrays in its own layout, so that it is available next to the product's library in one process.

Bounds, none of them from what the code gives:

* transform: ``||F - F_np||_2 <= 16 t u ||F_np||_2`` with ``t = log2(cells)``, ``u = 2**-53``.  Higham's bound for radix-2 transforms is
  ``t eta / (1 - t eta)`` with ``eta = mu + gamma_4 (sqrt 2 + mu) <= 8 u`` for twiddles good to ``mu <= 2 u`` (cos and sin of an angle in the
  first octant that is itself good to 2 u pi / 4, each rounded once); doubled because numpy's transform errs by as much.
* limbs: with E the exponent of a shell's largest term, ``L = ceil(log2(count))`` and ``D = 63 - L`` the limbs count units of
  ``2**eh``, ``2**(eh - D)`` and ``2**el``, ``eh = E - (62 - L)``, ``el = eh - 2 D = E - 188 + 3 L``.  The two remainders are exact, so a term
  is off by at most half a unit of the last limb, ``2**(el - 1)``, and the three integer sums by at most ``count 2**(el - 1) <=
  2**(E - 189 + 4 L)``.  The sum is at least its largest term, ``>= 2**(E - 1)``: relative to it the limbs are off by at most
  ``2**(4 L - 188)``, and the one rounding of the conversion adds half an ulp.  A shell holds at most 2**32 modes (1024 x 1024 x 4096
  cells), so ``L <= 32`` and the limb part is at most ``2**-60`` of the sum: ``limb_bound`` is below 2 ulp for every supported shape
  (``test_spectrum_cpu.py`` asserts it for L = 0 ... 32).
* shell sums against numpy: ``sum_shells |S - S_np| <= eps (2 + eps) sum S_np`` with ``eps = 16 t u`` - Cauchy-Schwarz on the transform
  bound (``| |a|^2 - |b|^2 | <= |a - b| (|a| + |b|)`` summed over the modes).
"""

from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import spectrum_shimlib as SS
import stats_cases as S

from pde_hip import _abi
from pde_hip.device import DeviceArray, DeviceBuffer

DTYPES = S.DTYPES
bits = S.bits
U = 2.0 ** -53

# the smallest shapes at which the geometry can go wrong: the shortest lines, a line per wave, the longest row (64 KiB of LDS), rows
# shorter and longer than a tile, tall lines (a 128 KiB tile), ragged tiles everywhere (n2 / 2 + 1 is never a multiple of 8)
SHAPES = ((2,), (4,), (64,), (128,), (4096,), (2, 2), (4, 128), (1024, 8), (8, 1024), (2, 2, 2), (2, 64, 8), (16, 4, 128), (8, 8, 256),
          (64, 64, 64))
# beyond the grid-stride turn of every launch (1024 workgroups of a transform pass, 2048 of a shell sweep) with three components:
# 4096 batches of rows per component, 1920 and 1560 tiles of lines, 1 064 960 modes (4160 workgroups' worth)
TURN = (128, 128, 128)
NCOMPS = (1, 3)
DX = (0.5, 1.25, 2.0)
REFUSED = ((3,), (6, 8), (8, 12), (2048, 8), (8192,), (4, 4, 100))


def shape_id(shape) -> str:
    return "x".join(map(str, shape))


def dx_of(shape):
    return DX[3 - len(shape):]


def draw(shape, ncomp: int, dtype, seed: int = 0) -> np.ndarray:
    """Valid data ``(ncomp, *shape)``: a mean, a few plane waves and noise - a spectrum with a dynamic range, not white."""
    rng = np.random.default_rng([seed, ncomp, *shape])
    out = rng.normal(0.0, 0.1, (ncomp, *shape)) + 0.3
    for c in range(ncomp):
        phase = sum(2.0 * np.pi * (c + 1 + a) * np.arange(n).reshape([-1 if b == a else 1 for b in range(len(shape))]) / n for a, n in enumerate(shape))
        out[c] += np.cos(phase)
    return out.astype(dtype)


# ---- the shim, called directly ------------------------------------------------------------------------------------------------------
class ShimCalls:
    """The tests-only serial C versions on host arrays in the shim's own layout."""

    def __init__(self):
        self.h = SS.load()
        self.h.pdehip_layout.argtypes = [C.POINTER(_abi.Grid), C.POINTER(C.c_int64)]
        for name in ("fft_supported", "fft_forward", "shell_spectrum"):
            fn = getattr(self.h, "pdehip_" + name)
            fn.argtypes, fn.restype = list(_abi.OPTIONAL_PROTOTYPES[name]), C.c_int

    def full(self, shape, valid: np.ndarray):
        """(grid struct, host array in the shim's layout with ``valid`` in the interior and NaN everywhere else)."""
        g = _abi.make_grid(tuple(shape), (1.0,) * len(shape), valid.dtype)
        lay = (C.c_int64 * 8)()
        assert self.h.pdehip_layout(C.byref(g), lay) == 0
        p0, p1, pc, off, slack = int(lay[0]), int(lay[1]), int(lay[2]), int(lay[3]), int(lay[6])
        n = (1,) * (3 - len(shape)) + tuple(shape)
        arr = np.full(valid.shape[0] * pc + slack, np.nan, dtype=valid.dtype)
        idx = off + (np.arange(n[0])[:, None, None] * p0 + np.arange(n[1])[None, :, None] * p1 + np.arange(n[2])[None, None, :])
        for c in range(valid.shape[0]):
            arr[c * pc + idx.ravel()] = valid[c].ravel()
        assert arr.ctypes.data % 16 == 0
        return g, arr

    def forward(self, shape, valid: np.ndarray) -> np.ndarray:
        g, arr = self.full(shape, valid)
        out = np.empty((valid.shape[0], *half_shape(shape)), dtype=np.complex128)
        rc = self.h.pdehip_fft_forward(C.byref(g), valid.shape[0], arr.ctypes.data, out.ctypes.data, None)
        assert rc == 0, rc
        return out

    def shells(self, shape, valid: np.ndarray, freqs, edges):
        g, arr = self.full(shape, valid)
        kf = np.ascontiguousarray(np.concatenate(freqs), dtype=np.float64)
        e = np.ascontiguousarray(edges, dtype=np.float64)
        ns = e.size + 1
        counts, sums = np.empty(ns, dtype=np.uint64), np.empty((valid.shape[0], ns), dtype=np.float64)
        rc = self.h.pdehip_shell_spectrum(C.byref(g), valid.shape[0], arr.ctypes.data, kf.ctypes.data, ns - 2, e.ctypes.data, counts.ctypes.data,
                                          sums.ctypes.data, None)
        assert rc == 0, rc
        return counts, sums

    def supported(self, shape, dtype=np.float64) -> int:
        return self.h.pdehip_fft_supported(C.byref(_abi.make_grid(tuple(shape), (1.0,) * len(shape), np.dtype(dtype))))


@functools.lru_cache(maxsize=None)
def shim() -> ShimCalls:
    return ShimCalls()


def half_shape(shape) -> tuple[int, ...]:
    return (*shape[:-1], shape[-1] // 2 + 1)


# ---- inputs and references, computed once ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(shape, ncomp: int, dtype_name: str) -> np.ndarray:
    valid = draw(shape, ncomp, np.dtype(dtype_name))
    valid.setflags(write=False)
    return valid


@functools.lru_cache(maxsize=None)
def shim_forward(shape, ncomp: int, dtype_name: str) -> np.ndarray:
    out = shim().forward(shape, inputs(shape, ncomp, dtype_name))
    out.setflags(write=False)
    return out


def frequencies(shape, dx=None) -> list[np.ndarray]:
    """numpy's own ``np.fft.fftfreq`` per axis: what Python uploads."""
    return [np.fft.fftfreq(n, d) for n, d in zip(shape, dx_of(shape) if dx is None else dx)]


def full_k(shape, dx=None) -> np.ndarray:
    """\\|k\\| on the FULL frequency grid: ``sqrt`` of the sum of the squares added from the slowest axis on."""
    k2 = 0
    for f in frequencies(shape, dx):
        k2 = np.add.outer(k2, f * f)
    return np.sqrt(k2)


def edge_sets(shape, dx=None) -> dict[str, np.ndarray]:
    """Default shells, equal bins and explicit edges that leave modes below and above."""
    from pde_hip.spectrum import shell_edges

    dx = dx_of(shape) if dx is None else dx
    kmax = float(full_k(shape, dx).max())
    return {
        "default": shell_edges(None, shape, dx)[0],
        "seven": shell_edges(7, shape, dx)[0],
        "explicit": np.array([0.03, 0.1, 0.11, 0.25, 0.4, 0.41, 0.75]) * kmax,
    }


@functools.lru_cache(maxsize=None)
def shim_shells(shape, ncomp: int, dtype_name: str, which: str):
    counts, sums = shim().shells(shape, inputs(shape, ncomp, dtype_name), frequencies(shape), edge_sets(shape)[which])
    counts.setflags(write=False)
    sums.setflags(write=False)
    return counts, sums


# ---- restatements --------------------------------------------------------------------------------------------------------------------
def np_counts(shape, edges, dx=None) -> np.ndarray:
    """``nbins + 2`` counts from ``np.histogram`` on the full frequency grid, then the modes below and above the edges."""
    kk = full_k(shape, dx).ravel()
    return np.concatenate([np.histogram(kk, edges)[0], [np.count_nonzero(kk < edges[0]), np.count_nonzero(kk > edges[-1])]]).astype(np.uint64)


def half_slots(shape, edges, dx=None):
    """(slot, weight) of every mode of the half spectrum, in C order."""
    from pde_hip.spectrum import _slots

    nh = shape[-1] // 2 + 1
    kk = full_k(shape, dx)[..., :nh]
    kidx = np.arange(nh)
    weight = np.broadcast_to(np.where((kidx > 0) & (2 * kidx < shape[-1]), 2.0, 1.0), kk.shape)
    return _slots(kk, np.asarray(edges, dtype=np.float64)).ravel(), weight.ravel()


def weighted_power(spec: np.ndarray, weight: np.ndarray) -> np.ndarray:
    """``weight * (re * re + im * im)`` per component, every operation rounded once: the terms of the device's sums."""
    flat = spec.reshape(spec.shape[0], -1)
    return (flat.real * flat.real + flat.imag * flat.imag) * weight


def exact_shell_sums(v: np.ndarray, slot: np.ndarray, ns: int) -> np.ndarray:
    """``math.fsum`` of the terms of every slot, per component."""
    order = np.argsort(slot, kind="stable")
    bounds = np.searchsorted(slot[order], np.arange(ns + 1))
    return np.array([[math.fsum(row[order[bounds[b]:bounds[b + 1]]]) for b in range(ns)] for row in v])


def np_shell_sums(shape, valid: np.ndarray, edges, dx=None):
    """Sums of ``|fftn|**2`` per slot from numpy's FULL transform in fp64, per component."""
    from pde_hip.spectrum import _slots

    slot = _slots(full_k(shape, dx), np.asarray(edges, dtype=np.float64)).ravel()
    axes = tuple(range(1, valid.ndim))
    power = np.abs(np.fft.fftn(valid.astype(np.float64), axes=axes)) ** 2
    return np.stack([np.bincount(slot, weights=row.ravel(), minlength=len(edges) + 1) for row in power])


# ---- bounds --------------------------------------------------------------------------------------------------------------------------
def transform_eps(shape) -> float:
    return 16.0 * math.log2(math.prod(shape)) * U


def ulp(x: float) -> float:
    return float(np.spacing(abs(x)))


def limb_layout(largest: float, count: int):
    """(eh, L, D, el) of a shell, as the header states them."""
    L = 0
    while (1 << L) < count:
        L += 1
    E = math.frexp(largest)[1]
    D = 63 - L
    eh = E - (62 - L)
    return eh, L, D, eh - 2 * D


def limb_bound(largest: float, count: int, total: float) -> float:
    """What a limb sum may differ by from the exact sum ``total`` of its ``count`` terms, the largest being ``largest``."""
    if largest == 0.0 or count == 0:
        return 0.0
    el = limb_layout(largest, count)[3]
    return count * math.ldexp(1.0, el - 1) + 0.5 * ulp(total)


# ---- drivers on whatever library ``pde_hip._lib`` holds ------------------------------------------------------------------------------------
upload = S.upload
GUARD = 64


def fft_forward(lib, dev: DeviceArray, stream=None) -> np.ndarray:
    """The half spectrum ``(ncomp, *half shape)``; GUARD words of all-ones bits behind the buffer must survive the call."""
    out_shape = (dev.ncomp, *half_shape(dev.info.shape))
    nbytes = 16 * math.prod(out_shape)
    buf = DeviceBuffer(nbytes + 8 * GUARD)
    lib.memset(buf.ptr, 0xFF, buf.nbytes, stream)
    lib.fft_forward(dev.info.ref, dev.ncomp, dev.ptr, buf.ptr, stream)
    host = np.empty(nbytes // 8 + GUARD, dtype=np.uint64)
    lib.memcpy_d2h(host.ctypes.data, buf.ptr, host.nbytes, stream)
    assert (host[-GUARD:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "the guard words behind the spectrum were written"
    return host[:-GUARD].view(np.complex128).reshape(out_shape)


def shell_spectrum(lib, dev: DeviceArray, freqs, edges, stream=None, keep: list | None = None):
    """(counts ``(nbins + 2,)`` uint64, sums ``(ncomp, nbins + 2)``); the outputs hold all-ones bits before the call."""
    kf = np.ascontiguousarray(np.concatenate(freqs), dtype=np.float64)
    e = np.ascontiguousarray(edges, dtype=np.float64)
    ns = e.size + 1
    bufs = [DeviceBuffer(kf.nbytes), DeviceBuffer(e.nbytes), DeviceBuffer(8 * ns + 8 * GUARD), DeviceBuffer(8 * dev.ncomp * ns + 8 * GUARD)]
    lib.memcpy_h2d(bufs[0].ptr, kf.ctypes.data, kf.nbytes, stream)
    lib.memcpy_h2d(bufs[1].ptr, e.ctypes.data, e.nbytes, stream)
    for b in bufs[2:]:
        lib.memset(b.ptr, 0xFF, b.nbytes, stream)
    lib.shell_spectrum(dev.info.ref, dev.ncomp, dev.ptr, bufs[0].ptr, ns - 2, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, stream)
    if keep is not None:
        keep.append((bufs, dev.ncomp, ns))
        return None
    return read_shells(lib, bufs, dev.ncomp, ns, stream)


def read_shells(lib, bufs, ncomp: int, ns: int, stream=None):
    counts, sums = np.empty(ns + GUARD, dtype=np.uint64), np.empty(ncomp * ns + GUARD, dtype=np.uint64)
    lib.memcpy_d2h(counts.ctypes.data, bufs[2].ptr, counts.nbytes, stream)
    lib.memcpy_d2h(sums.ctypes.data, bufs[3].ptr, sums.nbytes, stream)
    assert (counts[-GUARD:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (sums[-GUARD:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    return counts[:ns].copy(), sums[:-GUARD].view(np.float64).reshape(ncomp, ns).copy()


def whole_allocation(lib, dev: DeviceArray) -> np.ndarray:
    """Every byte of the array's allocation (ghost cells, padding and slack included), as words."""
    host = np.empty(dev.nbytes // dev.itemsize, dtype=dev.dtype)
    lib.memcpy_d2h(host.ctypes.data, dev.ptr, dev.nbytes, None)
    return bits(host)


# ---- fields of integer-amplitude cosines -------------------------------------------------------------------------------------------------
def cosine_field(shape, modes) -> np.ndarray:
    """``sum_m a_m cos(2 pi m . x / n)`` for ``modes = ((a, m), ...)`` with integer amplitudes and integer mode vectors."""
    out = np.zeros(shape)
    for amp, m in modes:
        phase = sum(2.0 * np.pi * mi * np.arange(n).reshape([-1 if b == a else 1 for b in range(len(shape))]) / n for a, (mi, n) in enumerate(zip(m, shape)))
        out += amp * np.cos(phase)
    return out


# ---- the golden file ---------------------------------------------------------------------------------------------------------------------
# name -> (shape, dx): 1-D to 3-D, unequal dx, and one shape that is no power of two (the host path)
GOLDEN = {
    "line": ((32,), (0.25,)),
    "plane": ((16, 64), (2.0, 0.5)),
    "box": ((8, 4, 16), (0.5, 1.25, 2.0)),
    "odd": ((12, 10), (1.0, 1.5)),
}


def golden_input(name: str) -> np.ndarray:
    shape, _ = GOLDEN[name]
    rng = np.random.default_rng([11, *shape])
    return rng.normal(0.2, 1.0, shape)
