"""`PDEHIP_E4_MINUS_TWICE(x, c)` of `py-pde_amd/csrc/pdehip_euler4_plan.h` - one fused multiply-add, what the four-step sweep computes every
`neighbour - 2 * centre` with - has the bits of the reference's two operations `vm = 2 * c; x - vm` (cartesian.py:220-227).  Checked on a CPU
through a tests-only probe (`tests/shim/euler4_fma_probe.cpp`, built by g++ here, like tests/test_euler4_plan.py).

Why it holds: doubling is exact in binary floating point (subnormals included) unless it overflows, so `x - vm` is the real number x - 2c
rounded once, and so is fma(-2, c, x).  The cases: random values of equal and of very different magnitude, values a few ulps apart
(cancellation), exact cancellation x = 2c (the sign of the zero), zeros of both signs, subnormals, the largest c whose double is finite,
infinities and NaNs.  Beyond that c the doubling overflows and the two forms differ: that is the documented limit, checked as well."""

from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "py-pde_amd" / "csrc" / "pdehip_euler4_plan.h"
PROBE = ROOT / "tests" / "shim" / "euler4_fma_probe.cpp"
BUILD = ROOT / "tests" / "shim" / "_build"
DMAX = np.finfo(np.float64).max
TINY = np.finfo(np.float64).tiny          # the smallest normal number
SUB = np.nextafter(0.0, 1.0)              # the smallest subnormal


@pytest.fixture(scope="module")
def lib():
    BUILD.mkdir(exist_ok=True)
    so = BUILD / "libe4fma_probe.so"
    if not so.exists() or so.stat().st_mtime < max(HEADER.stat().st_mtime, PROBE.stat().st_mtime):
        tmp = so.with_suffix(f".{os.getpid()}.tmp")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-shared", "-fPIC", str(PROBE), "-o", str(tmp)], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(str(so))
    lib.e4fma_mismatches.restype = C.c_long
    return lib


def mismatches(lib, x, c):
    x, c = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(c, np.float64)
    assert x.shape == c.shape and x.ndim == 1
    first = C.c_long(-1)
    n = lib.e4fma_mismatches(x.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), C.c_long(x.size), C.byref(first))
    return n, (None if n == 0 else (x[first.value], c[first.value]))


def test_random_values(lib):
    rng = np.random.default_rng(5)
    n = 200000
    c = rng.uniform(-0.5, 0.5, n)
    assert mismatches(lib, rng.uniform(-0.5, 0.5, n), c) == (0, None)                       # what a field holds
    scale = 2.0 ** rng.integers(-1000, 1000, n)
    assert mismatches(lib, rng.standard_normal(n) * scale, rng.standard_normal(n) * scale) == (0, None)
    assert mismatches(lib, rng.standard_normal(n) * scale, rng.standard_normal(n) * np.roll(scale, 1)) == (0, None)   # far apart in magnitude


def test_cancellation_and_zeros(lib):
    rng = np.random.default_rng(6)
    c = rng.standard_normal(50000)
    x = 2 * c
    for k in range(-3, 4):   # x within a few ulps of 2c, and exactly 2c: +0 in both forms
        xk = x.copy()
        for _ in range(abs(k)):
            xk = np.nextafter(xk, np.inf if k > 0 else -np.inf)
        assert mismatches(lib, xk, c) == (0, None), k
    zeros = np.array([0.0, -0.0])
    xs, cs = np.meshgrid(np.concatenate([zeros, [1.5, -1.5, SUB, -SUB]]), np.concatenate([zeros, [0.75, -0.75, SUB, -SUB]]))
    assert mismatches(lib, xs.ravel(), cs.ravel()) == (0, None)


def test_subnormals_and_the_largest_magnitudes(lib):
    rng = np.random.default_rng(7)
    n = 50000
    sub = rng.integers(-(2**52), 2**52, n) * SUB                     # every kind of subnormal, and normals just above
    assert mismatches(lib, sub, np.roll(sub, 1)) == (0, None)
    assert mismatches(lib, sub + rng.integers(-4, 5, n) * TINY, np.roll(sub, 1)) == (0, None)
    big = rng.uniform(0.25, 0.5, n) * DMAX * rng.choice([-1.0, 1.0], n)   # 2c stays finite; x - 2c may overflow, in both forms alike
    assert mismatches(lib, rng.uniform(-1, 1, n) * DMAX, big) == (0, None)
    edge = np.array([DMAX / 2, -DMAX / 2, np.nextafter(DMAX / 2, 0), np.inf, -np.inf, np.nan])
    xs, cs = np.meshgrid(np.array([0.0, 1.0, DMAX, -DMAX, np.inf, -np.inf, np.nan]), edge)
    assert mismatches(lib, xs.ravel(), cs.ravel()) == (0, None)


def test_the_limit_is_where_the_doubling_overflows(lib):
    """c beyond half the largest double: 2 * c is infinite in the reference, the fused form still sees the finite product - the one place
    where the two differ, a field of magnitude 1e308."""
    c = np.array([np.nextafter(DMAX / 2, np.inf), 0.75 * DMAX])
    n, first = mismatches(lib, np.array([DMAX, DMAX]), c)
    assert n == 2 and first == (DMAX, c[0])
