"""The four-step sweep with its waves in roles (pdehip_march4.inc; the lane -> patch map and the levels a wave executes: `lane_patch`,
`wave_levels` of pdehip_euler4_plan.h, enumerated on a CPU by tests/test_euler4_lanes.py): bit-identical to single steps of the oracle
through `pdehip_euler_run`, the path forced by PDEHIP_EULER4=1, like tests/test_hip_euler4.py.

The field is seeded noise, so a lane that holds the wrong patch, or a halo wave that skips a level one of its patches is needed at, shows at
the cells concerned.  Shapes: one tile that is its own neighbour on every side (every ring patch reads the tile's own outputs), one and two
sweeps and a bit; 2 x 2 tiles with an odd plane count; general spacing with D != 1 (the other instance); the contracted build.
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

DT = 0.05
UNIT_NAME = "euler4_kernel<double,E2_DIFFUSION_UNIT> (32x64 tile, 4 levels in LDS, all-periodic)"
CART_NAME = "euler4_kernel<double,E2_DIFFUSION> (32x64 tile, 4 levels in LDS, all-periodic)"
FAST_TOL = 1e-10   # tests/test_hip_euler4_image.py::test_contracted_build: the contracted build against the exact one, relative to the field's scale


def _setup(kind, shape):
    if kind == "unit":
        return pde_hip.UnitGrid(shape, periodic=True), 1.0
    bounds = [[0, n * s] for n, s in zip(shape, (0.8, 1.25, 1.1))]
    return pde_hip.CartesianGrid(bounds, shape, periodic=True), 0.7


def _data(shape):
    return np.random.default_rng(23).uniform(-0.5, 0.5, shape)


@functools.lru_cache(maxsize=None)
def _expect(kind, shape, steps):
    grid, D = _setup(kind, shape)
    out = expect_steps(_abi.RHS_DIFFUSION, D, grid, "periodic", _data(shape), DT, steps)
    out.setflags(write=False)
    return out


@pytest.fixture
def backend(monkeypatch):
    monkeypatch.setenv("PDEHIP_EULER4", "1")
    return pde_hip.get_backend("hip")


def _run(backend, kind, shape, steps):
    grid, D = _setup(kind, shape)
    data = _data(shape)
    spec = backend.make_rhs_spec(pde_hip.DiffusionPDE(D, bc="periodic"), pde_hip.ScalarField(grid, data))
    a, b = DeviceArray(spec.info).set_valid(data), DeviceArray(spec.info)
    res = C.c_void_p()
    lib = backend._lib
    lib.euler_run(spec.info.ref, spec.ref, a.ptr, b.ptr, DT, steps, C.byref(res), None)
    assert res.value in (a.ptr, b.ptr)
    return (b if res.value == b.ptr else a).get_valid(), lib.last_kernel_name().decode()


def _check(backend, kind, shape, steps):
    got, name = _run(backend, kind, shape, steps)
    want = _expect(kind, shape, steps)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} cells differ, the first at {bad[0].tolist()} (row % 32, column % 64 = {bad[0][1] % 32}, {bad[0][2] % 64})"
    assert np.abs(got - _data(shape)).max() > 1e-3   # a loop that did nothing must not pass
    return name


@pytest.mark.parametrize("steps", [4, 9])
def test_one_tile_its_own_neighbour(backend, steps):
    """16 x 32 x 64: the halo of the only tile is the tile itself through both wraps, so every patch of both rings holds cells that are also
    outputs.  4 steps: one sweep; 9: two sweeps and a single step behind them."""
    name = _check(backend, "unit", (16, 32, 64), steps)
    if steps % 4 == 0:
        assert name == UNIT_NAME
    else:   # the sweeps in front of the tail are four-step ones: the gate is a function of shape and knob alone
        assert _run(backend, "unit", (16, 32, 64), steps - steps % 4)[1] == UNIT_NAME


def test_four_tiles_odd_plane_count(backend):
    assert _check(backend, "unit", (17, 64, 128), 8) == UNIT_NAME


def test_general_spacing(backend):
    assert _check(backend, "cart", (24, 32, 128), 4) == CART_NAME


def test_contracted_build(backend):
    """pdehip_set_fastmath(1): the same sweep compiled with FMA contraction, held to the bound tests/test_hip_euler4_image.py holds it to
    against the exact result; the exact build is back afterwards."""
    shape = (17, 64, 128)
    want = _expect("unit", shape, 8)
    try:
        backend.fastmath = True
        on = C.c_int(0)
        backend._lib.get_fastmath(C.byref(on))
        assert on.value == 1
        fast, name = _run(backend, "unit", shape, 8)
        assert "euler4_kernel" in name and "fastmath" in name, name
    finally:
        backend.fastmath = None
        _ = backend._lib   # applies the default mode again
    rel = float(np.abs(fast - want).max() / np.abs(want).max())
    print(f"contracted against exact: {rel:.3e} relative to the field's scale")
    assert rel <= FAST_TOL
    assert not np.array_equal(fast, want), "the contracted build produced the exact build's bits everywhere: is it really another build?"
