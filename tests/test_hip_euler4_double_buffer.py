"""The four-step sweep with two barriers per phase and two buffers for the images of levels 1 and 2 (pdehip_march4.inc; the buffers and the
order of a phase: pdehip_euler4_plan.h, enumerated on a CPU by tests/test_euler4_double_buffer.py): bit-identical to single steps of the
oracle through `pdehip_euler_run`, the path forced by PDEHIP_EULER4=1.

What these cases add to tests/test_hip_euler4_image.py: the buffers change places from phase to phase, so the loop - unrolled three times -
has six different last phases, one per phase of the unrolling and parity; six consecutive plane counts end it in each once.  Two x-chunks of
unequal length end at different parities in one launch, twice with equal bits (a barrier in the wrong place shows as a difference between two
runs or against the oracle).  And non-finite values: the second buffers start as zeros and a wave leaves the cells of a level it skips as
they are - nothing of that may reach a stored cell.
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


def _setup(kind, shape):
    if kind == "unit":
        return pde_hip.UnitGrid(shape, periodic=True), 1.0
    bounds = [[0, n * s] for n, s in zip(shape, (0.8, 1.25, 1.1))]
    return pde_hip.CartesianGrid(bounds, shape, periodic=True), 0.7


def _data(shape, special=False):
    data = np.random.default_rng(23).uniform(-0.5, 0.5, shape)
    if special:   # the cells of tests/test_hip_euler4_image.py
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


@pytest.mark.parametrize("kind", ["unit", "cart"])
@pytest.mark.parametrize("n0", range(16, 22))
def test_every_last_phase_at_every_parity(backend, kind, n0):
    """One x-chunk of n0 planes is n0 + 6 = 22 ... 27 iterations: the last one is each of the three unrolled phases at each parity once.
    Two sweeps, so that the second starts from what the first one's last phases stored."""
    shape = (n0, 32, 64)
    got, name = _run(backend, kind, shape, 8)
    assert name == (UNIT_NAME if kind == "unit" else CART_NAME)
    np.testing.assert_array_equal(got, _expect(kind, shape, 8))
    assert np.abs(got - _data(shape)).max() > 1e-3   # a loop that did nothing must not pass


def test_two_chunks_of_unequal_parity_twice(backend):
    """Three sweeps, two x-chunks of 17 and 16 planes (23 and 22 iterations: they end at different parities), 2 x 2 tiles: 12 single steps
    of the oracle, and the same bits both times."""
    shape = (33, 64, 128)
    want = _expect("unit", shape, 12)
    first, name = _run(backend, "unit", shape, 12)
    second, _ = _run(backend, "unit", shape, 12)
    assert name == UNIT_NAME
    np.testing.assert_array_equal(first, second)
    np.testing.assert_array_equal(first, want)
    assert np.abs(first - _data(shape)).max() > 1e-3


def test_non_finite_values_spread_as_in_the_oracle(backend):
    """One NaN at a tile's corner cell, one inf of each sign at the first cell of a tile and of the grid: after four steps (one sweep) the
    non-finite cells are where the oracle has them (assert_array_equal holds NaNs in equal places to be equal) and every other bit agrees -
    the zeros of the second buffers, of the guard runs and of a skipped level feed no stored cell."""
    shape = (17, 64, 128)
    want = _expect("unit", shape, 4, True)
    got, name = _run(backend, "unit", shape, 4, True)
    assert name == UNIT_NAME
    assert 0 < np.isnan(want).sum() < want.size // 4 and np.isinf(want).any()   # the case is what it claims to be
    np.testing.assert_array_equal(got, want)
