"""The four-step sweep with its lane-linear LDS image (pdehip_march4.inc; the image: pdehip_euler4_plan.h, enumerated on a CPU by
tests/test_euler4_image.py): bit-identical to single steps of the oracle through `pdehip_euler_run`, the path forced by PDEHIP_EULER4=1.

What these cases add to tests/test_hip_euler4.py: many sweeps in a row and the same run twice (a barrier in the wrong place shows as a
difference between two runs or against the oracle), the smallest self-wrapping tile with general spacing at three plane counts (between them
every phase of the loop unrolled three times is the last one once), non-finite values next to tile seams (a patch at the rim of the region
reads unspecified cells of the image: nothing of that may reach a stored cell, and nothing may be reordered) and the contracted build.
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
FAST_TOL = 1e-10   # tests/test_hip_fastmath.py: the contracted build against the exact one, relative to the field's scale


def _setup(kind, shape):
    if kind == "unit":
        return pde_hip.UnitGrid(shape, periodic=True), 1.0
    bounds = [[0, n * s] for n, s in zip(shape, (0.8, 1.25, 1.1))]
    return pde_hip.CartesianGrid(bounds, shape, periodic=True), 0.7


def _data(shape, special=False):
    data = np.random.default_rng(11).uniform(-0.5, 0.5, shape)
    if special:
        data[5, 31, 63] = np.nan      # the last cell of a tile, next to three others
        data[9, 32, 64] = np.inf      # the first cell of the tile diagonally behind it
        data[0, 0, 0] = -np.inf       # reaches its neighbours through all three periodic wraps
    return data


@functools.lru_cache(maxsize=None)
def _expect(kind, shape, steps, special=False):
    grid, D = _setup(kind, shape)
    with np.errstate(invalid="ignore"):
        out = expect_steps(_abi.RHS_DIFFUSION, D, grid, "periodic", _data(shape, special), DT, steps)
    out.setflags(write=False)
    return out


@pytest.fixture
def backend(monkeypatch):
    monkeypatch.setenv("PDEHIP_EULER4", "1")
    return pde_hip.get_backend("hip")


def _run(backend, kind, shape, steps, special=False):
    grid, D = _setup(kind, shape)
    data = _data(shape, special)
    spec = backend.make_rhs_spec(pde_hip.DiffusionPDE(D, bc="periodic"), pde_hip.ScalarField(grid, data))
    a, b = DeviceArray(spec.info).set_valid(data), DeviceArray(spec.info)
    res = C.c_void_p()
    lib = backend._lib
    lib.euler_run(spec.info.ref, spec.ref, a.ptr, b.ptr, DT, steps, C.byref(res), None)
    assert res.value in (a.ptr, b.ptr)
    return (b if res.value == b.ptr else a).get_valid(), lib.last_kernel_name().decode()


def test_ten_sweeps_twice(backend):
    """Ten sweeps, two x-chunks of unequal length (17 + 16 planes), 2 x 2 tiles: 40 single steps of the oracle, and the same bits both times."""
    shape = (33, 64, 128)
    want = _expect("unit", shape, 40)
    first, name = _run(backend, "unit", shape, 40)
    second, _ = _run(backend, "unit", shape, 40)
    assert name == UNIT_NAME
    np.testing.assert_array_equal(first, second)
    np.testing.assert_array_equal(first, want)
    assert np.abs(first - _data(shape)).max() > 1e-3   # a loop that did nothing must not pass


@pytest.mark.parametrize("shape", [(17, 32, 64), (19, 64, 64), (18, 32, 64)], ids=str)
def test_self_wrapping_tile_general_spacing(backend, shape):
    """The row wrap of the image and its guard cells lie next to valid patches here; n0 + 6 = 23, 25 and 24 iterations: the loop, unrolled
    three times, ends in each of its three phases once."""
    got, name = _run(backend, "cart", shape, 8)
    assert name == CART_NAME
    np.testing.assert_array_equal(got, _expect("cart", shape, 8))
    assert np.abs(got - _data(shape)).max() > 1e-3


def test_non_finite_values_spread_as_in_the_oracle(backend):
    """One NaN at a tile's corner cell, one inf of each sign at the first cell of a tile and of the grid: after four steps (one sweep) the
    non-finite cells are where the oracle has them (assert_array_equal holds NaNs in equal places to be equal) and every other bit agrees."""
    shape = (17, 64, 128)
    want = _expect("unit", shape, 4, True)
    got, name = _run(backend, "unit", shape, 4, True)
    assert name == UNIT_NAME
    assert 0 < np.isnan(want).sum() < want.size // 4 and np.isinf(want).any()   # the case is what it claims to be
    np.testing.assert_array_equal(got, want)


def test_contracted_build(backend):
    """pdehip_set_fastmath(1): the same sweep compiled with FMA contraction, held to the bound of tests/test_hip_fastmath.py against the
    exact result; it is another build, and the exact one is back afterwards."""
    shape = (33, 64, 128)
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
    again, name = _run(backend, "unit", shape, 8)
    assert name == UNIT_NAME
    np.testing.assert_array_equal(again, want)
