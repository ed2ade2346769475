"""The pure-fp32 arithmetic mode restated in numpy, with the cases and the seeded data its tests share.

Every operation below is a numpy float32 operation, i.e. rounded to fp32 and never contracted - the contract of ``include/pdehip.h``:

    t_a = ((l_a - 2c) + r_a) * s_a,  s_a = fp32(dx_a ** -2)          lap = t_0 [+ t_1 [+ t_2]] in grid-axis order
    u'  = u + fp32(dt) * (fp32(D) * lap(u))
    a zero-derivative wall: the neighbour beyond it is the adjacent cell itself; a periodic wall: the cell at the other end

``tests/golden/make_golden_f32p.py`` asserts that these functions equal the reference's torch backend bit for bit before it writes
``tests/golden/f32p.npz``; the CPU tests compare them with the goldens, the GPU tests compare the kernels with them.
"""

from __future__ import annotations

import numpy as np

F32 = np.float32


def field_data(shape, seed: int = 0, lo: float = -1.0, hi: float = 1.0) -> np.ndarray:
    """Seeded fp32 data of any shape (valid or full)."""
    return np.random.default_rng(seed).uniform(lo, hi, size=tuple(shape)).astype(F32)


def scales(dx) -> np.ndarray:
    """s_a = fp32(dx_a ** -2): the power in double, rounded once."""
    return (np.asarray(dx, dtype=np.float64) ** -2).astype(F32)


def laplace_full(full: np.ndarray, dx) -> np.ndarray:
    """Laplacian of a ghost-padded fp32 array (its ghost cells are read) -> valid fp32 array."""
    assert full.dtype == F32
    nd = full.ndim
    s = scales(dx)
    mid = (slice(1, -1),) * nd
    c2 = F32(2) * full[mid]
    out = None
    for ax in range(nd):
        lo = tuple(slice(0, -2) if a == ax else slice(1, -1) for a in range(nd))
        hi = tuple(slice(2, None) if a == ax else slice(1, -1) for a in range(nd))
        term = ((full[lo] - c2) + full[hi]) * s[ax]
        out = term if out is None else out + term
    assert out.dtype == F32
    return out


def pad_faces(u: np.ndarray, periodic) -> np.ndarray:
    """Full array of valid data whose axes are periodic (wrapped ghost cells) or zero-derivative (ghost cell = adjacent cell)."""
    full = u
    for ax, per in enumerate(periodic):
        width = [(1, 1) if a == ax else (0, 0) for a in range(u.ndim)]
        full = np.pad(full, width, mode="wrap" if per else "edge")
    return full


def euler_steps(u: np.ndarray, dx, periodic, diffusivity: float, dt: float, nsteps: int) -> np.ndarray:
    """``nsteps`` explicit Euler steps of the diffusion equation on valid fp32 data."""
    assert u.dtype == F32
    d32, dt32 = F32(diffusivity), F32(dt)
    for _ in range(nsteps):
        u = u + dt32 * (d32 * laplace_full(pad_faces(u, periodic), dx))
        assert u.dtype == F32
    return u


def bounds_for(shape, dx):
    """Axis bounds of a CartesianGrid with the given cell counts and spacings (lower bound 0)."""
    return [(0.0, float(n) * float(d)) for n, d in zip(shape, dx)]


# spacings that are not representable sums (non-unit: s_a and its rounding matter) - per number of axes
DX = {1: (0.31,), 2: (0.31, 0.23), 3: (0.31, 0.23, 0.17)}
UNIT = {1: (1.0,), 2: (1.0, 1.0), 3: (1.0, 1.0, 1.0)}

# ---- goldens (tests/golden/f32p.npz) ---------------------------------------------------------------------------------------------
GOLDEN_LAPLACE_SHAPES = [(37,), (9, 21), (9, 13, 70)]
GOLDEN_LAPLACE_BCS = {
    "value": {"value": 0.537},
    "derivative": {"derivative": -1.13},
    "mixed": {"type": "mixed", "value": 0.51, "const": 1.07},
}
GOLDEN_D = 0.7
GOLDEN_EULER_STEPS = (1, 2, 3, 7)
# (id, shape, periodic): "auto_periodic_neumann" conditions - periodic axes wrap, the others are zero-derivative
GOLDEN_EULER_CASES = [
    ("e3p", (9, 13, 70), (True, True, True)),
    ("e3m", (9, 13, 70), (True, False, True)),
    ("e2", (9, 21), (False, True)),
    ("e1", (37,), (False,)),
]


def stable_dt(dx, diffusivity: float) -> float:
    """A time step with dt * D * sum(dx_a ** -2) = 0.2 < 0.5: an unstable run would only test overflow."""
    return 0.2 / (diffusivity * float(np.sum(np.asarray(dx, dtype=np.float64) ** -2)))


def golden_field(shape) -> np.ndarray:
    return field_data(shape, seed=100 + len(shape))


# ---- device tests (tests/test_hip_f32p.py) -----------------------------------------------------------------------------------------
# The march / two-step tile: 4 rows of axis 1 (R), 256 cells of axis 2 per wave in whole 16-byte vectors (axis 2 must be a multiple of 4,
# the two-step instance takes at most 1024 cells), segments of >= 8 planes along axis 0.
LAPLACE_SHAPES = {
    1: [(1,), (5,), (1000,)],
    2: [(1, 4), (7, 1030), (33, 130)],
    3: [(1, 1, 4), (5, 6, 7), (9, 13, 70), (17, 35, 261), (40, 36, 256), (16, 8, 1028), (130, 9, 64),
        (8, 4, 260), (7, 5, 252), (9, 3, 1024)],
}
EULER_SHAPES = [s for nd in (1, 2, 3) for s in LAPLACE_SHAPES[nd] if min(s) >= 2]
EULER_STEPS = (1, 2, 3, 4, 7)


def march_covers(shape) -> bool:
    """Whether the Laplacian's march instance takes this grid (else: one cell per thread)."""
    return len(shape) == 3 and shape[2] % 4 == 0 and shape[2] >= 4


def two_step_covers(shape) -> bool:
    """Whether the two-step Euler instance takes this grid (else: the one-step instance)."""
    return march_covers(shape) and shape[2] <= 1024 and min(shape) >= 2
