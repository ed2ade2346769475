"""Four Euler steps per sweep (pdehip_march4.inc: the time levels exchange their current plane through LDS) == single steps of the oracle,
bit for bit, through `pdehip_euler_run` with the path forced by PDEHIP_EULER4=1.

The tile is 32 x 64 outputs (rows x fastest axis), the smallest grid the gate admits has 16 planes (8 recomputed halo planes + one chunk of 8),
two x-chunks start at 32 planes (pdehip_euler4_plan.h; tests/test_euler4_plan.py pins those numbers on a CPU).  Shapes: one tile whose
periodic halos wrap onto itself, two tiles per axis (seams; non-cubic so that swapped pitches show), one and two x-chunks (seams and the
wrap of the warm-up planes), each at the smallest extent and one plane more (chunks of unequal length, every phase of the unrolled loop as
the last one).
"""

from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
from helpers import expect_steps

import pde_hip
from pde_hip import _abi
from pde_hip.device import DeviceArray

pytestmark = pytest.mark.gpu

TY, TZ, NMIN, NTWO = 32, 64, 16, 32   # tile, fewest planes, fewest planes of two x-chunks
DT = 0.05


def _setup(kind, shape, periodic=True):
    """`unit`: UnitGrid, D = 1 (the E2_DIFFUSION_UNIT instance, what bench.py times); `cart`: unequal spacings and D = 0.7"""
    if kind == "unit":
        return pde_hip.UnitGrid(shape, periodic=periodic), 1.0
    bounds = [[0, n * s] for n, s in zip(shape, (0.8, 1.25, 1.1))]
    return pde_hip.CartesianGrid(bounds, shape, periodic=periodic), 0.7


def _bc(grid, periodic):
    if periodic is True:
        return "periodic"
    bc = {}
    for a, per in zip(grid.axes, periodic):
        if per:
            bc[a] = "periodic"
        else:
            bc[a + "-"], bc[a + "+"] = {"value": 0.3}, {"derivative": -0.2}
    return bc


def _data(shape, dtype=np.float64, seed=7):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, shape).astype(dtype)


@functools.lru_cache(maxsize=None)
def _expect(kind, shape, steps, periodic=True, dtype="float64"):
    grid, D = _setup(kind, shape, periodic)
    out = expect_steps(_abi.RHS_DIFFUSION, D, grid, _bc(grid, periodic), _data(shape, np.dtype(dtype)), DT, steps)
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def backend():
    return pde_hip.get_backend("hip")


def _run(backend, kind, shape, steps, periodic=True, dtype="float64"):
    """(final field, name of the kernel launched last) of `steps` steps through pdehip_euler_run"""
    grid, D = _setup(kind, shape, periodic)
    data = _data(shape, np.dtype(dtype))
    eq = pde_hip.DiffusionPDE(D, bc=_bc(grid, periodic))
    spec = backend.make_rhs_spec(eq, pde_hip.ScalarField(grid, data, dtype=np.dtype(dtype)))
    a, b = DeviceArray(spec.info).set_valid(data), DeviceArray(spec.info)
    res = C.c_void_p()
    lib = backend._lib
    lib.euler_run(spec.info.ref, spec.ref, a.ptr, b.ptr, DT, steps, C.byref(res), None)
    assert res.value in (a.ptr, b.ptr)
    got = (b if res.value == b.ptr else a).get_valid()
    return got, lib.last_kernel_name().decode()


def _check(backend, kind, shape, steps, forced=True, **kw):
    got, name = _run(backend, kind, shape, steps, **kw)
    np.testing.assert_array_equal(got, _expect(kind, tuple(shape), steps, **kw))
    assert np.abs(got.astype(np.float64) - _data(shape)).max() > 1e-3   # a loop that did nothing must not pass
    assert ("euler4_kernel" in name) == forced, name
    return name


@pytest.mark.parametrize("n0", [NMIN, NMIN + 1])
def test_self_wrapping_tile(backend, monkeypatch, n0):
    """One tile in y and z: both periodic halos wrap onto the tile itself; one x-chunk whose warm-up planes wrap onto the chunk itself."""
    monkeypatch.setenv("PDEHIP_EULER4", "1")
    name = _check(backend, "unit", (n0, TY, TZ), 4)
    assert name == "euler4_kernel<double,E2_DIFFUSION_UNIT> (32x64 tile, 4 levels in LDS, all-periodic)"


@pytest.mark.parametrize("shape", [(NMIN + 3, 2 * TY, 2 * TZ), (NMIN + 2, 3 * TY, 2 * TZ), (NMIN + 4, 2 * TY, 3 * TZ)], ids=str)
def test_tile_seams(backend, monkeypatch, shape):
    monkeypatch.setenv("PDEHIP_EULER4", "1")
    _check(backend, "unit", shape, 4)


@pytest.mark.parametrize("n0", [NTWO, NTWO + 1])
@pytest.mark.parametrize("tiles", [(1, 1), (2, 2)], ids=["1x1", "2x2"])
def test_x_chunk_seam(backend, monkeypatch, n0, tiles):
    """Two x-chunks (16 + 16 and 17 + 16 planes): the seam between them and the warm-up planes that wrap around the march axis."""
    monkeypatch.setenv("PDEHIP_EULER4", "1")
    _check(backend, "unit", (n0, tiles[0] * TY, tiles[1] * TZ), 8)


@pytest.mark.parametrize("steps", [4, 5, 6, 7, 8, 9])
def test_step_counts(backend, monkeypatch, steps):
    """Tails of 0 ... 3 steps behind one and two four-step sweeps, and the buffer the run returns: 6 = 4 + 2 is the benchmark's parity digest."""
    monkeypatch.setenv("PDEHIP_EULER4", "1")
    shape = (NTWO + 1, 2 * TY, 2 * TZ)
    # the sweeps in front of the tail are four-step ones: the launcher takes this shape (the gate is a function of shape and knob alone) ...
    assert "euler4_kernel" in _run(backend, "unit", shape, steps - steps % 4)[1]
    name = _check(backend, "unit", shape, steps, forced=steps % 4 == 0)
    if steps % 4:   # ... and the tail is what it was
        assert "euler2" in name or "lap_march" in name, name


GRAPH_STEPS = 2048   # from this length on, runs on small fields are captured into a graph of 32 steps and replayed (pdehip_steppers.hip)


def test_captured_graph(backend, monkeypatch):
    """A run long enough for graph capture: blocks of eight four-step sweeps replayed, then a tail of 4 + 2 steps.  The knob is part of the
    graph's key: the same buffers with PDEHIP_EULER4=0 afterwards capture and run the two-step sweeps, not the cached four-step graph."""
    shape, steps = (NMIN + 1, TY, TZ), GRAPH_STEPS + 6
    grid, D = _setup("unit", shape)
    data = _data(shape)
    spec = backend.make_rhs_spec(pde_hip.DiffusionPDE(D, bc="periodic"), pde_hip.ScalarField(grid, data))
    a, b = DeviceArray(spec.info), DeviceArray(spec.info)
    lib, res = backend._lib, C.c_void_p()
    want = _expect("unit", shape, steps)
    for knob, n, last in (("1", GRAPH_STEPS, "euler4_kernel"), ("1", steps, "euler2"), ("0", GRAPH_STEPS, "euler2"), ("0", steps, "euler2")):
        monkeypatch.setenv("PDEHIP_EULER4", knob)
        a.set_valid(data)
        lib.euler_run(spec.info.ref, spec.ref, a.ptr, b.ptr, DT, n, C.byref(res), None)
        name = lib.last_kernel_name().decode()
        assert last in name and (knob == "1" or "euler4" not in name), (knob, n, name)
        if n == steps:
            np.testing.assert_array_equal((b if res.value == b.ptr else a).get_valid(), want)


@pytest.mark.parametrize("shape", [(NTWO + 1, 2 * TY, 2 * TZ), (NMIN, TY, TZ)], ids=str)
def test_general_spacing(backend, monkeypatch, shape):
    monkeypatch.setenv("PDEHIP_EULER4", "1")
    name = _check(backend, "cart", shape, 8)
    assert name == "euler4_kernel<double,E2_DIFFUSION> (32x64 tile, 4 levels in LDS, all-periodic)"


@pytest.mark.parametrize("case", ["local-rows", "local-march-axis", "fp32", "2-D", "rows-off-tile", "columns-off-tile", "too-few-planes", "knob-0", "default"])
def test_the_gate_declines(backend, monkeypatch, case):
    """What the kernel does not cover runs the two-step and one-step sweeps as before, PDEHIP_EULER4=1 or not; so does a small field by default."""
    monkeypatch.setenv("PDEHIP_EULER4", "0" if case == "knob-0" else "1")
    if case == "default":
        monkeypatch.delenv("PDEHIP_EULER4")
    shape, kw = (NMIN + 4, TY, TZ), {}
    if case == "local-rows":
        kw = {"periodic": (True, False, True)}
    elif case == "local-march-axis":
        kw = {"periodic": (False, True, True)}
    elif case == "fp32":
        kw = {"dtype": "float32"}
    elif case == "2-D":
        shape = (2 * TY, 2 * TZ)
    elif case == "rows-off-tile":
        shape = (NMIN + 4, TY + 16, TZ)
    elif case == "columns-off-tile":
        shape = (NMIN + 4, TY, TZ + 32)
    elif case == "too-few-planes":
        shape = (NMIN - 1, TY, TZ)
    got, name = _run(backend, "unit", shape, 8, **kw)
    np.testing.assert_array_equal(got, _expect("unit", shape, 8, **kw))
    assert "euler4" not in name, name
