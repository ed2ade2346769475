"""Cases, numpy restatements and bounds for the statistics entry points ``pdehip_field_stats`` and ``pdehip_steady_state``.

Shared by ``tests/test_stats_cpu.py`` (CPU: the C versions of the tests-only shim) and ``tests/test_hip_stats.py`` (GPU: the kernels of
``csrc/pdehip_stats.hip``).  The restatements are written from the semantics in ``include/pdehip.h``; the drivers below call the entry
points through whatever library ``pde_hip._lib`` holds, so the same checks serve both.

Inputs: values from [0.5, 0.6] u [1.4, 1.5].  Every cell contributes at least 0.5 to ``sum`` and at least 0.16 to ``m2`` (the mean lies
near 1), so a lost or doubled cell moves either by far more than the bounds: at 2^22 cells the bound of ``sum`` is 2e-3, that of ``m2``
about 4e-4.  Ghost cells and row padding of every device array are poisoned (NaN and 1e300 in turn) before the interior is uploaded.

Bounds (u = 2^-53, n finite cells, all values converted exactly to float64):
  sum   |sum - fsum| <= n u sum|x|                           the first-order bound of ANY summation order
  mean  sum / n, bit for bit
  m2    |m2 - exact| <= (n + 4) u exact + n d^2, d = n u max|x|   summation order, rounding of each term ((x - mean) and its square),
                                                             and the error the terms inherit from the mean
``exact`` is the sum of squared deviations about the correctly rounded mean, every deviation and every square kept as an unevaluated
sum of two doubles (TwoSum, Dekker's product), summed with ``math.fsum``: one rounding in all.
"""

from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np

from pde_hip.device import DeviceArray, DeviceBuffer, GridInfo

U = 2.0 ** -53
DTYPES = (np.float64, np.float32)

# (shape, ncomp): extents 1, 2, 3, 4, 5, 63, 64, 65, 257 on the fastest axis (vector widths 2 / 4 / 1, wave and workgroup seams), rows of
# 1-3 cells, 1-D to 3-D, 1 / 3 / 9 components; the last two fill several workgroups
SMALL = (
    ((1,), 1), ((2,), 3), ((3,), 1), ((4,), 9), ((5,), 1), ((63,), 3), ((64,), 1), ((65,), 1), ((257,), 3),
    ((3, 1), 1), ((2, 2), 3), ((1, 3), 9), ((5, 4), 1), ((3, 5), 3), ((2, 63), 1), ((3, 64), 9), ((3, 65), 1), ((5, 257), 1),
    ((2, 3, 1), 3), ((1, 1, 2), 1), ((3, 2, 3), 9), ((2, 3, 4), 1), ((3, 1, 5), 1), ((2, 3, 63), 3), ((3, 2, 64), 1), ((1, 3, 65), 9),
    ((3, 5, 257), 1), ((17, 9, 64), 3),
)
# beyond the grid-stride turn of a launch of 8192 workgroups (2 097 152 pieces): 65 x 129 x 251 = 2 104 635 one-cell pieces (odd rows),
# 129 x 127 x 258 = 2 113 407 fp64 pairs (4 226 814 cells)
TURN_PIECES = 8192 * 256
TURN = {
    "f64x1": ((65, 129, 251), np.float64, 1),
    "f32x1": ((65, 129, 251), np.float32, 1),
    "f64x2": ((129, 127, 258), np.float64, 2),
}
ELAPSED, RTOL = 0.37, 1e-5      # (neither is a float32 number: the rounding to the field's type shows)


def case_id(case) -> str:
    shape, ncomp = case
    return "x".join(map(str, shape)) + f"c{ncomp}"


def vec_width(dtype, n2: int) -> int:
    if np.dtype(dtype) == np.float64:
        return 2 if n2 % 2 == 0 else 1
    return 4 if n2 % 4 == 0 else 1


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def draw(shape, ncomp: int, dtype, seed: int = 0) -> np.ndarray:
    """Valid data ``(ncomp, *shape)`` from the two bands."""
    rng = np.random.default_rng([seed, ncomp, *shape])
    full = (ncomp, *shape)
    return (rng.uniform(0.5, 0.6, full) + 0.9 * rng.integers(0, 2, full)).astype(dtype)


def plant_nonfinite(valid: np.ndarray) -> np.ndarray:
    """NaN, +inf and -inf in the first and the last cell and on the wave / workgroup seams of every component (as far as it has them)."""
    out = valid.copy()
    flat = out.reshape(out.shape[0], -1)
    n = flat.shape[1]
    spots = [0, n - 1, 63, 64, 127, 128, 255, 256, n // 2]
    for c in range(flat.shape[0]):
        for m, at in enumerate(s for s in spots if 0 <= s < n):
            flat[c, at] = (np.nan, np.inf, -np.inf)[(m + c) % 3]
    return out


# ---- device arrays ------------------------------------------------------------------------------------------------------------------
def upload(lib, shape, valid: np.ndarray) -> DeviceArray:
    """``valid`` on the device; ghost cells, row padding and slack hold NaN and 1e300 in turn."""
    info = GridInfo(shape, (1.0,) * len(shape), valid.dtype)
    dev = DeviceArray(info, (valid.shape[0],))
    poison = np.empty(dev.nbytes // dev.itemsize, dtype=valid.dtype)
    poison[0::2] = np.nan
    poison[1::2] = 1e300 if valid.dtype == np.float64 else 3e38
    lib.memcpy_h2d(dev.ptr, poison.ctypes.data, dev.nbytes, None)
    return dev.set_valid(valid, None)


def field_stats(lib, dev: DeviceArray, *, norm: bool = False, want_m2: bool = True, stream=None, out: DeviceBuffer | None = None) -> np.ndarray:
    """The blocks of eight as ``(blocks, 8)``; the output buffer holds all-ones bits before the call."""
    blocks = 1 if norm else dev.ncomp
    out = DeviceBuffer(64 * blocks) if out is None else out
    lib.memset(out.ptr, 0xFF, 64 * blocks, stream)
    lib.field_stats(dev.info.ref, dev.ncomp, dev.ptr, int(norm), int(want_m2), out.ptr, stream)
    host = np.empty((blocks, 8), dtype=np.float64)
    lib.memcpy_d2h(host.ctypes.data, out.ptr, host.nbytes, stream)
    return host


def steady_state(lib, cur: DeviceArray, last: DeviceArray, elapsed: float = ELAPSED, rtol: float = RTOL, stream=None) -> np.ndarray:
    out = DeviceBuffer(16)
    lib.memset(out.ptr, 0xFF, 16, stream)
    lib.steady_state(cur.info.ref, cur.ncomp, cur.ptr, last.ptr, C.c_double(elapsed), C.c_double(rtol), out.ptr, stream)
    host = np.empty(2, dtype=np.float64)
    lib.memcpy_d2h(host.ctypes.data, out.ptr, 16, stream)
    return host


# ---- restatements -------------------------------------------------------------------------------------------------------------------
def np_values(valid: np.ndarray, norm: bool) -> np.ndarray:
    """What is reduced, ``(blocks, *shape)``: the components, or sqrt(x_0 * x_0 + x_1 * x_1 + ...) in the field's type, left to right."""
    if not norm:
        return valid
    with np.errstate(invalid="ignore", over="ignore"):
        s = valid[0] * valid[0]
        for c in range(1, valid.shape[0]):
            s = s + valid[c] * valid[c]
        return np.sqrt(s)[None]


def exact_m2(x: np.ndarray) -> float:
    """Sum of (x - mean)^2 of finite float64 values with one rounding: deviations by TwoSum, squares by Dekker's product, ``math.fsum``."""
    if x.size == 0:
        return math.nan
    m = math.fsum(x) / x.size
    hi = x - m
    bb = hi - x
    lo = (x - (hi - bb)) + (-m - bb)
    c = 134217729.0 * hi
    h = c - (c - hi)
    l = hi - h
    p = hi * hi
    e = ((h * h - p) + 2.0 * h * l) + l * l
    return math.fsum(np.concatenate([p, e, 2.0 * hi * lo]))


def expect_stats(valid: np.ndarray, norm: bool = False) -> list[dict]:
    out = []
    for row in np_values(valid, norm):
        x = row.astype(np.float64).ravel()
        fin = np.isfinite(x)
        xf = x[fin]
        n = int(fin.sum())
        out.append({"n": n, "bad": int(x.size - n), "fsum": math.fsum(xf), "sumabs": math.fsum(np.abs(xf)),
                    "min": xf.min() if n else math.nan, "max": xf.max() if n else math.nan, "maxabs": np.abs(xf).max() if n else 0.0,
                    "m2": exact_m2(xf)})
    return out


def check_stats(got: np.ndarray, expect: list[dict], want_m2: bool = True, what: str = "") -> None:
    """Every figure is printed before it is asserted."""
    assert got.shape == (len(expect), 8), f"{what}: {got.shape}"
    for c, (g, e) in enumerate(zip(got, expect)):
        n = e["n"]
        tag = f"{what} block {c}"
        print(f"{tag}: n {g[0]:.0f}/{n} bad {g[1]:.0f}/{e['bad']} sum {g[2]!r} fsum {e['fsum']!r} min {g[3]!r} max {g[4]!r} mean {g[5]!r} "
              f"m2 {g[6]!r} exact {e['m2']!r}")
        assert g[0] == n and g[1] == e["bad"], f"{tag}: counts {g[0]}, {g[1]} != {n}, {e['bad']}"
        assert g[7] == 0.0, f"{tag}: the last entry is {g[7]!r}"
        if n == 0:
            assert g[2] == 0.0 and all(np.isnan(g[3:7])), f"{tag}: no finite cell, got {g}"
            continue
        assert g[3] == e["min"] and g[4] == e["max"], f"{tag}: extrema {g[3]!r}, {g[4]!r} != {e['min']!r}, {e['max']!r}"
        err, bound = abs(g[2] - e["fsum"]), n * U * e["sumabs"]
        assert err <= bound, f"{tag}: sum off by {err:.3e} > {bound:.3e}"
        assert bits(np.float64(g[5])) == bits(np.float64(g[2]) / np.float64(g[0])), f"{tag}: mean {g[5]!r} is not sum / n = {g[2] / g[0]!r}"
        if not want_m2:
            assert np.isnan(g[6]), f"{tag}: m2 without the second sweep is {g[6]!r}"
            continue
        delta = n * U * e["maxabs"]
        err, bound = abs(g[6] - e["m2"]), (n + 4) * U * e["m2"] + n * delta * delta
        assert err <= bound, f"{tag}: m2 off by {err:.3e} > {bound:.3e}"


def np_steady(cur: np.ndarray, last: np.ndarray, elapsed: float = ELAPSED, rtol: float = RTOL) -> tuple[np.float64, int]:
    """(np.max of the tracker's expression over the finite cells of cur, their number) - pde/trackers/trackers.py:819-844 on arrays of
    the field's type; a Python float next to them is rounded to that type.  No cell: (NaN, 0)."""
    t = cur.dtype.type
    fin = np.isfinite(cur)
    n = int(fin.sum())
    if n == 0:
        return np.float64(np.nan), 0
    with np.errstate(invalid="ignore", over="ignore"):
        diff = last[fin] - cur[fin]
        rate = diff / t(elapsed)
        rate_abs = np.abs(rate) - t(rtol) * np.abs(cur[fin])
        m = np.max(rate_abs)
    assert rate_abs.dtype == cur.dtype
    return (np.float64(np.nan) if np.isnan(m) else np.float64(m)), n


def check_steady(got: np.ndarray, expect: tuple, what: str = "") -> None:
    m, n = expect
    print(f"{what}: max {got[0]!r} expect {m!r}, cells {got[1]:.0f} expect {n}")
    assert got[1] == n, f"{what}: {got[1]} cells took part, expected {n}"
    if np.isnan(m):
        assert np.isnan(got[0]), f"{what}: {got[0]!r}, expected NaN"
    else:
        assert bits(np.float64(got[0])) == bits(m), f"{what}: {got[0]!r} != {m!r}"


@functools.lru_cache(maxsize=None)
def small_inputs(case, dtype_name: str, planted: bool):
    """(valid data, expected statistics per component, expected statistics of the norm) of a small case, computed once."""
    shape, ncomp = case
    valid = draw(shape, ncomp, np.dtype(dtype_name))
    if planted:
        valid = plant_nonfinite(valid)
    valid.setflags(write=False)
    return valid, expect_stats(valid, False), expect_stats(valid, True)


@functools.lru_cache(maxsize=None)
def turn_inputs(key: str):
    shape, dtype, _ = TURN[key]
    valid = draw(shape, 1, dtype, seed=7)
    valid.setflags(write=False)
    return valid, expect_stats(valid, False)
