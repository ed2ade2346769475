"""Cases, inputs, drivers and bounds for the inverse transform ``pdehip_fft_inverse`` and the direct Poisson solve ``pdehip_poisson_fft``.

Shared by ``tests/test_poisson_fft_cpu.py`` (CPU: the serial C versions of the tests-only shim against numpy and the dense restatement)
and ``tests/test_hip_poisson_fft.py`` (GPU: the kernels of ``csrc/pdehip_fft.hip`` and ``csrc/pdehip_fftsolve.hip`` against the shim, bit
by bit).  Shapes, inputs and the forward shim are those of ``tests/spectrum_cases.py``; the shim is called directly on host arrays in its
own layout, so that it is available next to the product's library in one process.

Bounds, none of them from what the code gives:

* inverse of forward: ``max |f' - f| <= 2 eps max |f|`` with ``eps = spectrum_cases.transform_eps(shape)`` - that bound once per transform.
* the sums ``residual``, ``rhs_norm``, ``check_residual``: the device adds bit-equal non-negative terms in another order than the shim.
  A sum of n non-negative fp64 terms in ANY order is within ``(n - 1) u`` relative of the exact sum (Higham, Accuracy and Stability,
  eq. 4.4, ``gamma_{n-1}``), so two orders differ by at most ``2 n u`` relative; the square root halves that and adds its own rounding:
  ``sum_tolerance`` is ``2 cells u`` relative plus one ulp.
* the solve against the dense restatement: ``64 cond u max(1, max |x|)`` with ``cond = mu_max / mu_min`` over the non-zero modes, from the
  eigenvalue tables: the forward error of a backward-stable solve is ``cond`` times the backward error, a few u per transform
  stage and division.  Observed ratios: profiles/poisson_fft_tests.md.
"""

from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import poisson_fft_shimlib as PS
import spectrum_cases as K

from pde_hip import _abi
from pde_hip.device import DeviceArray, DeviceBuffer, GridInfo

U = K.U
DTYPES = K.DTYPES
bits = K.bits
GUARD = K.GUARD
# the grids of the solve tests: 1-D to 3-D, unequal spacings
SOLVE_SHAPES = ((32,), (16, 8), (8, 4, 8))
LONG_LINE = ((4096,), (0.25,))


def eigenvalues(shape, dx) -> list[np.ndarray]:
    """``mu_a[m] = 4 sin(pi m' / n)**2 / dx**2``, ``m' = min(m, n - m)``: the tables of the header, restated with numpy."""
    out = []
    for n, d in zip(shape, dx):
        m = np.arange(n)
        s = np.sin(np.pi * np.minimum(m, n - m) / n)
        out.append(4.0 * (s * s) * float(d) ** -2.0)
    return out


def condition(shape, dx) -> float:
    mu = 0
    for t in eigenvalues(shape, dx):
        mu = np.add.outer(mu, t)
    mu = np.sort(np.asarray(mu).ravel())
    return float(mu[-1] / mu[1])


def sum_tolerance(cells: int, value: float) -> float:
    return 2.0 * cells * U * abs(value) + K.ulp(value)


def white(shape, dtype=np.float64, seed: int = 0, mean: float = 0.0) -> np.ndarray:
    """uniform(-1, 1) with the mean ``mean`` (zero: a consistent right-hand side)."""
    rng = np.random.default_rng([seed, 77, *shape])
    data = rng.uniform(-1.0, 1.0, shape)
    data += mean - data.mean()
    return data.astype(dtype)


# ---- the shim, called directly ------------------------------------------------------------------------------------------------------
class ShimCalls:
    """The tests-only serial C versions on host arrays in the shim's own layout."""

    def __init__(self):
        self.h = PS.load()
        self.h.pdehip_layout.argtypes = [C.POINTER(_abi.Grid), C.POINTER(C.c_int64)]
        for name in ("fft_supported", "fft_forward", "fft_inverse", "poisson_fft"):
            fn = getattr(self.h, "pdehip_" + name)
            fn.argtypes, fn.restype = list(_abi.OPTIONAL_PROTOTYPES[name]), C.c_int

    def layout(self, shape, dx, dtype):
        g = _abi.make_grid(tuple(shape), tuple(dx), np.dtype(dtype))
        lay = (C.c_int64 * 8)()
        assert self.h.pdehip_layout(C.byref(g), lay) == 0
        p0, p1, pc, off = int(lay[0]), int(lay[1]), int(lay[2]), int(lay[3])
        n = (1,) * (3 - len(shape)) + tuple(shape)
        idx = off + (np.arange(n[0])[:, None, None] * p0 + np.arange(n[1])[None, :, None] * p1 + np.arange(n[2])[None, None, :])
        return g, pc, idx.ravel()

    def full(self, shape, valid: np.ndarray, dx=None):
        """(grid struct, host array in the shim's layout with ``valid`` (ncomp, *shape) in the interior and NaN elsewhere, interior index)."""
        g, pc, idx = self.layout(shape, dx or (1.0,) * len(shape), valid.dtype)
        arr = np.full(valid.shape[0] * pc + 2, np.nan, dtype=valid.dtype)
        for c in range(valid.shape[0]):
            arr[c * pc + idx] = valid[c].ravel()
        assert arr.ctypes.data % 16 == 0
        return g, arr, pc, idx

    def forward(self, shape, valid: np.ndarray) -> np.ndarray:
        g, arr, _, _ = self.full(shape, valid)
        out = np.empty((valid.shape[0], *K.half_shape(shape)), dtype=np.complex128)
        assert self.h.pdehip_fft_forward(C.byref(g), valid.shape[0], arr.ctypes.data, out.ctypes.data, None) == 0
        return out

    def inverse(self, shape, spectrum: np.ndarray, dtype) -> np.ndarray:
        """``(ncomp, *shape)`` of type ``dtype``; the spectrum is copied first (the call consumes it)."""
        ncomp = spectrum.shape[0]
        g, arr, pc, idx = self.full(shape, np.zeros((ncomp, *shape), dtype=dtype))
        spec = np.array(spectrum, dtype=np.complex128, order="C")
        rc = self.h.pdehip_fft_inverse(C.byref(g), ncomp, spec.ctypes.data, arr.ctypes.data, None)
        assert rc == 0, rc
        return np.stack([arr[c * pc + idx].reshape(shape) for c in range(ncomp)])

    def solve(self, shape, dx, rhs: np.ndarray, rtol: float = 1e-10, atol: float = 0.0):
        """(solution ``shape``, io dict) of ``pdehip_poisson_fft``."""
        g, arr, pc, idx = self.full(shape, rhs[None], dx)
        before = arr.copy()
        out = np.full_like(arr, np.nan)
        io = _abi.Poisson()
        io.rtol, io.atol = rtol, atol
        rc = self.h.pdehip_poisson_fft(C.byref(g), arr.ctypes.data, out.ctypes.data, C.byref(io), None)
        assert rc == 0, rc
        np.testing.assert_array_equal(bits(arr), bits(before), err_msg="the shim wrote the right-hand side")
        return out[idx].reshape(shape), io_dict(io)


def io_dict(io) -> dict:
    return {k: getattr(io, k) for k in ("iterations", "status", "singular", "residual", "rhs_norm", "check_residual")}


@functools.lru_cache(maxsize=None)
def shim() -> ShimCalls:
    return ShimCalls()


# ---- inputs and references, computed once ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shim_inverse(shape, ncomp: int, dtype_name: str) -> np.ndarray:
    """The shim's inverse (type ``dtype_name``) of the shim's forward of ``spectrum_cases.draw`` (fp64 input)."""
    out = shim().inverse(shape, K.shim_forward(shape, ncomp, "float64"), np.dtype(dtype_name))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def solve_input(shape, dtype_name: str) -> np.ndarray:
    """A right-hand side with a dynamic range and a mean of rounding size: ``draw`` minus its mean."""
    data = K.draw(shape, 1, np.float64)[0]
    data = (data - data.mean()).astype(dtype_name)
    data.setflags(write=False)
    return data


@functools.lru_cache(maxsize=None)
def shim_solve(shape, dtype_name: str):
    out, io = shim().solve(shape, K.dx_of(shape), solve_input(shape, dtype_name))
    out.setflags(write=False)
    return out, io


# ---- drivers on the product's library -------------------------------------------------------------------------------------------------------
def upload_dx(lib, shape, dx, valid: np.ndarray) -> DeviceArray:
    """``valid`` (ncomp, *shape) on the device; ghost cells, row padding and slack hold NaN and a large number in turn."""
    info = GridInfo(shape, tuple(dx), valid.dtype)
    dev = DeviceArray(info, (valid.shape[0],))
    poison = np.empty(dev.nbytes // dev.itemsize, dtype=valid.dtype)
    poison[0::2] = np.nan
    poison[1::2] = 1e300 if valid.dtype == np.float64 else 3e38
    lib.memcpy_h2d(dev.ptr, poison.ctypes.data, dev.nbytes, None)
    return dev.set_valid(valid, None)


def fft_inverse(lib, shape, spectrum: np.ndarray, dtype, stream=None):
    """(valid ``(ncomp, *shape)``, whole allocation before, whole allocation after); the spectrum buffer is followed by guard words."""
    ncomp = spectrum.shape[0]
    dev = K.upload(lib, shape, np.zeros((ncomp, *shape), dtype=dtype))
    before = K.whole_allocation(lib, dev).copy()
    spec = np.ascontiguousarray(spectrum, dtype=np.complex128)
    buf = DeviceBuffer(spec.nbytes + 8 * GUARD)
    lib.memset(buf.ptr, 0xFF, buf.nbytes, stream)
    lib.memcpy_h2d(buf.ptr, spec.ctypes.data, spec.nbytes, stream)
    lib.fft_inverse(dev.info.ref, ncomp, buf.ptr, dev.ptr, stream)
    guard = np.empty(GUARD, dtype=np.uint64)
    lib.memcpy_d2h(guard.ctypes.data, buf.ptr + spec.nbytes, guard.nbytes, stream)
    assert (guard == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "the guard words behind the spectrum were written"
    return dev.get_valid(stream=stream), before, K.whole_allocation(lib, dev)


def interior_mask(lib, dev: DeviceArray) -> np.ndarray:
    """True at the interior cells of the whole allocation of ``dev``: found by writing a marker through ``set_valid``."""
    probe = DeviceArray(dev.info, (dev.ncomp,))
    lib.memset(probe.ptr, 0, probe.nbytes, None)
    probe.set_valid(np.ones((dev.ncomp, *dev.info.shape), dtype=dev.dtype), None)
    return K.whole_allocation(lib, probe) != 0


def poisson_fft(lib, shape, dx, rhs: np.ndarray, rtol: float = 1e-10, atol: float = 0.0, stream=None):
    """(solution, io dict, launch chain); the whole allocations of the right-hand side (unchanged) and of the result (interior only) are checked."""
    dev = upload_dx(lib, shape, dx, rhs[None])
    out = upload_dx(lib, shape, dx, np.zeros_like(rhs)[None])
    rhs_before, out_before = K.whole_allocation(lib, dev).copy(), K.whole_allocation(lib, out).copy()
    io = _abi.Poisson()
    io.rtol, io.atol = rtol, atol
    lib.poisson_fft(dev.info.ref, dev.ptr, out.ptr, C.byref(io), stream)
    chain = lib.last_kernel_name().decode()
    np.testing.assert_array_equal(K.whole_allocation(lib, dev), rhs_before, err_msg="the right-hand side was written")
    outside = ~interior_mask(lib, out)
    np.testing.assert_array_equal(K.whole_allocation(lib, out)[outside], out_before[outside], err_msg="cells outside the interior were written")
    return out.get_valid(stream=stream)[0], io_dict(io), chain


def expected_chain(shape, dtype) -> str:
    name = "double" if np.dtype(dtype) == np.float64 else "float"
    slow = sum(n > 1 for n in shape[:-1])
    return "+".join([f"fft_rows_kernel<{name}>"] + ["fft_lines_kernel"] * slow + ["fftsolve_divide_kernel"] + ["inverse_lines_kernel"] * slow
                    + ["inverse_rows_kernel<double>", "fftsolve_check_kernel"])


def check_io(got: dict, want: dict, cells: int) -> None:
    for k in ("status", "iterations", "singular"):
        assert got[k] == want[k], (k, got, want)
    for k in ("residual", "rhs_norm", "check_residual"):
        assert abs(got[k] - want[k]) <= sum_tolerance(cells, want[k]), (k, got[k], want[k])


def np_inverse_of(shape, spectrum: np.ndarray) -> np.ndarray:
    return np.fft.irfftn(spectrum, s=shape, axes=tuple(range(1, 1 + len(shape))))


def cells_of(shape) -> int:
    return math.prod(shape)
