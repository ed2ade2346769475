"""Cases and plain numpy restatements for the pointwise and reduction kernels of ``csrc/pdehip_ops.hip``.

Shared by ``tests/test_oracle_pointwise.py`` (CPU: the oracle twins against the restatements) and
``tests/test_hip_pointwise.py`` (GPU: the kernels against both).  The restatements follow the reference's expressions
(``pde/solvers/runge_kutta.py:60``, ``:135-150``, ``pde/solvers/adams_bashforth.py:44``,
``pde/backends/numba/_solvers.py:381-394``): every operand is widened to float64, the expression is evaluated left to right
in float64 and the result is rounded ONCE to the field's type.  All arrays are host arrays in the compact full layout
``(ncomp, n0 + 2, ...)``; the restatements work on whole arrays (ghost cells included), callers look at the interior.
"""

from __future__ import annotations

import math

import numpy as np

# ---- shapes -------------------------------------------------------------------------------------------------------------
# fastest extents: both vector widths (fp64 pairs: n2 % 2 == 0, fp32 quads: n2 % 4 == 0), extents below one vector, the one-cell
# path for n2 % 4 in {1, 2, 3}, one and several rows per workgroup
EXTENTS = (1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 257)
# leading extents 1, 3 and 5 on 1-D, 2-D and 3-D grids
LEADS = ((), (3,), (5, 3), (1,), (3, 1), (5,), (1, 5), (3, 5), (1, 1))


def small_cases():
    """(shape, ncomp): every fastest extent twice, with rotating leading extents and 1, 2 or 3 components."""
    out = []
    for idx, n2 in enumerate(EXTENTS):
        for rep in range(2):
            lead = LEADS[(2 * idx + 4 * rep + rep) % len(LEADS)]
            out.append(((*lead, n2), 1 + (idx + rep) % 3))
    return out


SMALL = small_cases()
# beyond the grid-stride turn of the 16 384-workgroup launches (4 194 304 items): the item count exceeds the cap by more than a
# row and is no multiple of 256.  65 x 129 x 501 = 4 200 585 cells for both one-cell paths; 129 x 127 x 516 gives
# 4 226 814 items as fp64 pairs (one component) and as fp32 quads (two components)
TURN_ITEMS = 16384 * 256
TURN = {
    "f64x2": ((129, 127, 516), 1, np.float64, 2),
    "f64x1": ((65, 129, 501), 1, np.float64, 1),
    "f32x4": ((129, 127, 516), 2, np.float32, 4),
    "f32x1": ((65, 129, 501), 1, np.float32, 1),
}
SCALES = (1.0, 10.0, 0.1, 3.0, 0.3, 30.0, 0.03)


def vec_width(dtype, n2) -> int:
    """Cells per item of PDEHIP_VEC_LAUNCH."""
    if np.dtype(dtype) == np.float64:
        return 2 if n2 % 2 == 0 else 1
    return 4 if n2 % 4 == 0 else 1


def items_of(shape, ncomp, vec) -> int:
    return ncomp * int(np.prod(shape[:-1], dtype=np.int64)) * (shape[-1] // vec)


def cell_of_item(t, shape, vec, lane=0):
    """Index into the host full array of lane ``lane`` of item ``t`` (the decomposition of ``for_each_chunk``)."""
    n = (1,) * (3 - len(shape)) + tuple(shape)
    kc = n[2] // vec
    k = (t % kc) * vec + lane
    r = t // kc
    j = r % n[1]
    r //= n[1]
    i = r % n[0]
    comp = r // n[0]
    return (comp, *[x + 1 for x in (i, j, k)[3 - len(shape):]])


def interior(shape):
    return (slice(None), *[slice(1, -1)] * len(shape))


def ghost_mask(shape):
    m = np.ones(tuple(s + 2 for s in shape), bool)
    m[tuple([slice(1, -1)] * len(shape))] = False
    return m


def fields(shape, ncomp, dtype, count, seed=0):
    """``count`` full arrays, each from its own seeded stream and with its own scale (a swapped or wrong coefficient shows);
    ghost cells carry the recognisable value -(1000 + index)."""
    out = []
    gm = ghost_mask(shape)
    for m in range(count):
        rng = np.random.default_rng([seed, m])
        a = (SCALES[m % len(SCALES)] * rng.uniform(-1, 1, (ncomp, *[s + 2 for s in shape]))).astype(dtype)
        a[:, gm] = -(1000 + m)
        out.append(a)
    return out


TRIPLES = ((3, 4, 5), (5, 12, 13), (8, 15, 17), (7, 24, 25), (20, 21, 29), (12, 35, 37), (9, 40, 41), (28, 45, 53))


def pair_fields(shape, npairs, dtype, seed=0):
    """Planar complex data (component 2p: real part, 2p + 1: imaginary part) whose moduli are exactly representable: Pythagorean
    triples times a power of two, legs swapped and signed at random - every faithful hypot returns the same bits.  Ghost cells
    hold 1e6, larger than any modulus."""
    rng = np.random.default_rng([seed, 99])
    full = (npairs, *[s + 2 for s in shape])
    t = np.array(TRIPLES, dtype=np.float64)[rng.integers(0, len(TRIPLES), full)]
    scale = 2.0 ** rng.integers(-6, 3, full)
    swap = rng.integers(0, 2, full).astype(bool)
    re = np.where(swap, t[..., 1], t[..., 0]) * scale * rng.choice([-1.0, 1.0], full)
    im = np.where(swap, t[..., 0], t[..., 1]) * scale * rng.choice([-1.0, 1.0], full)
    out = np.empty((2 * npairs, *full[1:]), dtype=dtype)
    out[0::2], out[1::2] = re, im
    out[:, ghost_mask(shape)] = 1e6
    return out


def bits(x):
    """Bit pattern(s) as unsigned integers."""
    x = np.asarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def f64_bits(v) -> int:
    return int(np.float64(v).view(np.uint64))


# ---- the restatements ---------------------------------------------------------------------------------------------------
def _w(a):
    return np.asarray(a, dtype=np.float64)


def np_lincomb(y, coefs, ks):
    """`y + b1*k1 + b2*k2 + ...` resp. `b1*k1 + b2*k2 + ...` (runge_kutta.py:135-145)"""
    dtype = ks[0].dtype
    if y is not None:
        acc, start = _w(y), 0
    else:
        acc, start = np.float64(coefs[0]) * _w(ks[0]), 1
    for m in range(start, len(ks)):
        acc = acc + np.float64(coefs[m]) * _w(ks[m])
    return acc.astype(dtype)


def np_rk4(y, k1, k2, k3, k4):
    """runge_kutta.py:60"""
    s = (_w(k1) + 2 * _w(k2) + 2 * _w(k3) + _w(k4)) / 6
    return (_w(y) + s).astype(y.dtype)


def np_ab2(y, rc, rp, dt):
    """adams_bashforth.py:44"""
    s = np.float64(dt) * (1.5 * _w(rc) - 0.5 * _w(rp))
    return (_w(y) + s).astype(y.dtype)


# runge_kutta.py:117-125, the same quotients
R1, R3, R4, R5, R6 = 1.0 / 360, -128.0 / 4275, -2197.0 / 75240, 1.0 / 50, 2.0 / 55
C1, C3, C4, C5 = 25.0 / 216, 1408.0 / 2565, 2197.0 / 4104, -1.0 / 5


def _absmax(e) -> np.float64:
    """`np.abs(e).max()`; numpy's maximum hands a NaN on (with the payload of the operand: the kernels and the oracle return the
    canonical quiet NaN, so a NaN result is canonicalised here)."""
    with np.errstate(invalid="ignore"):
        m = np.abs(e).max()
    return np.float64(np.nan) if np.isnan(m) else np.float64(m)


def np_rkf45(y, ks, where):
    """runge_kutta.py:147-150: (ynew, error); ``where`` selects the interior (the error norm looks at interior cells only)."""
    k1, k3, k4, k5, k6 = _w(ks[0]), _w(ks[2]), _w(ks[3]), _w(ks[4]), _w(ks[5])
    with np.errstate(invalid="ignore", over="ignore"):
        el = R1 * k1 + R3 * k3 + R4 * k4 + R5 * k5 + R6 * k6
        ynew = (_w(y) + C1 * k1 + C3 * k3 + C4 * k4 + C5 * k5).astype(y.dtype)
    return ynew, _absmax(el[where])


def np_euler_adaptive(y, rate, dt, half, k, where):
    """_solvers.py:381-394: (step_small, error); both steps are arrays of the state's type"""
    with np.errstate(invalid="ignore", over="ignore"):
        small = (_w(half) + _w(k)).astype(y.dtype)
        large = (_w(y) + np.float64(dt) * _w(rate)).astype(y.dtype)
        e = _w(large) - _w(small)
    return small, _absmax(e[where])


def np_max_abs_diff(a, b, where):
    with np.errstate(invalid="ignore"):
        e = _w(a) - _w(b)
    return _absmax(e[where])


def np_max_abs_pairs(arr, where):
    """`np.abs(z).max()` of the complex numbers (component 2p) + 1j * (component 2p + 1), the modulus taken with hypot as the
    kernel and the oracle do.  (numpy's own modulus of a complex number is not hypot: for -0.4030177126 + 7.0997100578j it is
    one unit in the last place below the correctly rounded value that glibc's hypot returns.  No libm promises a correctly
    rounded hypot, so the bit comparisons use `pair_fields`, whose moduli are exact.)"""
    with np.errstate(invalid="ignore"):
        z = np.hypot(_w(arr[0::2]), _w(arr[1::2]))
    return _absmax(z[where])


def np_integrate_sequential(arr, vol, where):
    """The numba loop `total += cell_volume * x` in C order (numba/backend.py:600-606), per component."""
    x = _w(arr[where]).reshape(arr.shape[0], -1)
    return np.array([np.cumsum(np.float64(vol) * row)[-1] for row in x])


def fsum_integrate(arr, vol, where):
    """(exact sums of the float64 products per component, sums of their magnitudes)"""
    x = np.float64(vol) * _w(arr[where]).reshape(arr.shape[0], -1)
    return np.array([math.fsum(row) for row in x]), np.array([math.fsum(np.abs(row)) for row in x])


def np_count_nonfinite(arr, where):
    x = arr[where].reshape(arr.shape[0], -1)
    return (~np.isfinite(x)).sum(axis=1).astype(np.float64)
