"""The phase of the four-step sweep (pdehip_march4.inc) after its diet: plane bases in scalar registers with a 32-bit byte offset per lane,
the loaded plane straight into the slot of the plane that dies, the buffer parity a compile-time constant of a loop unrolled six times with
one exit.  Bit-identical to single steps of the oracle through `pdehip_euler_run`, the path forced by PDEHIP_EULER4=1, and the kernel name as
`e4plan::format_name` gives it.

The loop runs lx + 6 phases for an x-chunk of lx planes: whole rounds of six, then lx mod 6 phases left over.  Shapes (the smallest that
reach every path; every one with 4 and with 8 steps, one and two sweeps, so that the second sweep starts from what the first one stored):

    16 x 32 x 64     one tile, one chunk, wraps onto itself; 4 phases left over
    32 x 32 x 64     two x-chunks of 16: the chunk seam and the periodic plane wrap
    35 x 64 x 128    four tiles, chunks of 18 and 17 planes: no phase and five phases left over in one launch
    22 x 32 x 64     one chunk of 22: 28 phases
    19, 20, 21 x 32 x 64   one, two and three phases left over

Both instances: unit spacing with D = 1 (E2_DIFFUSION_UNIT) and a CartesianGrid with unequal spacings.  A 5-step run checks the tail (one
sweep and a single step).  One case per instance runs the contracted build against the rounding bound of tests/fastmath_cases.py.  And, as in
tests/test_hip_euler4_stores.py, whose guarded buffers these cases use: ghost cells, row padding and a sentinel run behind both arrays are
untouched after a run - the loads and stores go through a scalar base now, and an offset that left its plane would show here.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
from fastmath_cases import Built, Case, excess
from test_hip_euler4_double_buffer import CART_NAME, UNIT_NAME, _data, _expect, _run
from test_hip_euler4_stores import SENTINEL
from test_hip_euler4_stores import _data as _stores_data
from test_hip_euler4_stores import _expect as _stores_expect
from test_hip_euler4_stores import _run_once

import pde_hip
from pde_hip.device import DeviceArray

pytestmark = pytest.mark.gpu

ISSUE_SHAPES = [(16, 32, 64), (32, 32, 64), (35, 64, 128), (22, 32, 64)]
LEFT_OVER_SHAPES = [(19, 32, 64), (20, 32, 64), (21, 32, 64)]
NAMES = {"unit": UNIT_NAME, "cart": CART_NAME}


@pytest.fixture
def backend(monkeypatch):
    monkeypatch.setenv("PDEHIP_EULER4", "1")
    return pde_hip.get_backend("hip")


def test_the_shapes_reach_every_count_of_left_over_phases():
    """(no device work) x-chunks as e4plan::plan cuts them: at least 16 planes each, as many chunks as fill 256 CUs"""
    left = set()
    for n0, n1, n2 in ISSUE_SHAPES + LEFT_OVER_SHAPES:
        tiles = (n1 // 32) * (n2 // 64)
        nxc = max(1, min(-(-256 // tiles), n0 // 16))
        lx = -(-n0 // nxc)
        chunks = [min(lx, n0 - x0) for x0 in range(0, n0, lx)]
        assert min(chunks) >= 8
        left |= {(c + 6) % 6 for c in chunks}
    assert left == set(range(6))


@pytest.mark.parametrize("steps", [4, 8])
@pytest.mark.parametrize("shape", ISSUE_SHAPES + LEFT_OVER_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["unit", "cart"])
def test_bit_identical_to_the_oracle(backend, kind, shape, steps):
    got, name = _run(backend, kind, shape, steps)
    assert name == NAMES[kind]
    np.testing.assert_array_equal(got, _expect(kind, shape, steps))
    assert np.abs(got - _data(shape)).max() > 1e-3   # a loop that did nothing must not pass


@pytest.mark.parametrize("kind,shape", [("unit", (22, 32, 64)), ("cart", (35, 64, 128))], ids=str)
def test_five_steps_the_tail(backend, kind, shape):
    """one sweep of four steps and a single step behind it"""
    got, _ = _run(backend, kind, shape, 5)
    np.testing.assert_array_equal(got, _expect(kind, shape, 5))


@pytest.mark.parametrize("shape", ISSUE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["unit", "cart"])
def test_loads_and_stores_through_a_scalar_base_stay_inside_the_field(backend, kind, shape):
    """8 steps between two guarded buffers: the valid cells are the oracle's, everything else still holds the sentinel"""
    want = _stores_expect(kind, shape)
    got, raws, valid, name = _run_once(backend, kind, shape)
    assert name == NAMES[kind]
    np.testing.assert_array_equal(got, want)
    assert np.abs(got - _stores_data(shape)).max() > 1e-3
    for raw in raws:   # each array was the output of one sweep
        outside = raw[~valid]
        wrong = np.flatnonzero(outside != SENTINEL)
        assert wrong.size == 0, (wrong.size, np.flatnonzero(~valid)[wrong[:8]])
        assert not np.any(raw[valid] == SENTINEL)
    np.testing.assert_array_equal(raws[0][valid], want.ravel())


def _fast_case(kind, shape, steps):
    if kind == "unit":
        bounds, param = tuple((0.0, float(n)) for n in shape), 1.0
    else:
        bounds, param = tuple((0.0, n * s) for n, s in zip(shape, (0.8, 1.25, 1.1))), 0.7
    return Case(family="launch_euler4", entry="euler_run", shape=shape, dtype="float64", bounds=bounds, periodic=(True,) * 3, bc=("set", "periodic"),
                param=param, dt=0.05, steps=steps, seed=7)


@pytest.mark.parametrize("kind,shape", [("unit", (16, 32, 64)), ("cart", (22, 32, 64))], ids=str)
def test_contracted_build_inside_the_rounding_bound(backend, kind, shape):
    """`pdehip_set_fastmath`: the same instance of the other build, every cell inside the running error bound of the oracle's expression"""
    built = Built(_fast_case(kind, shape, 8))
    (ref, bound), = built.reference()
    data = built.data
    spec = backend.make_rhs_spec(pde_hip.DiffusionPDE(built.case.param, bc="periodic"), pde_hip.ScalarField(built.grid, data))
    try:
        backend.fastmath = True
        lib = backend._lib
        on = C.c_int(0)
        lib.get_fastmath(C.byref(on))
        assert on.value == 1
        a, b = DeviceArray(spec.info).set_valid(data), DeviceArray(spec.info)
        res = C.c_void_p()
        lib.euler_run(spec.info.ref, spec.ref, a.ptr, b.ptr, built.case.dt, built.case.steps, C.byref(res), None)
        assert res.value in (a.ptr, b.ptr)
        fast = (b if res.value == b.ptr else a).get_valid()
        name = lib.last_kernel_name().decode()
    finally:
        backend.fastmath = None
        _ = backend._lib
    assert name.startswith(NAMES[kind]) and "fastmath" in name, name
    assert np.isfinite(fast).all()
    n_over, ratio = excess(fast, ref, bound)
    print(f"{kind} {shape}: |result - reference| / bound <= {ratio:.4f}")
    assert n_over == 0, f"{n_over} cells leave the rounding bound (|diff| / bound up to {ratio:.4g})"
    assert np.abs(fast - data).max() > 1e-3
