"""The pure-fp32 arithmetic mode on the device (csrc/pdehip_f32p.hip) against its numpy restatement (tests/f32p_cases.py) and against the
reference's torch results (tests/golden/f32p.npz).  Every comparison is ``np.array_equal``.

Tile of the march / two-step instances and the shapes that probe it (f32p_cases.LAPLACE_SHAPES[3]):
  axis 2: whole 16-byte vectors (multiple of 4 cells), 256 cells per wave, two-step instance: at most 1024 cells (4 waves)
          multiple: 40x36x256, 9x3x1024      one vector more: 8x4x260, 16x8x1028 (1028 > 1024: one-step instance for Euler)
          one vector less: 7x5x252            not a multiple of 4 (one cell per thread): 17x35x261 (crosses 256, odd), 5x6x7, 9x13x70
          less than a chunk: 130x9x64, 1x1x4
  axis 1: 4 rows per lane       multiple: 40x36x256, 16x8x1028, 8x4x260     one more: 130x9x64, 7x5x252     one less: 9x3x1024
  axis 0: segments of >= 8 planes (small grids: exactly 8)     multiple: 40x36x256, 16x8x1028, 8x4x260
          one more: 9x3x1024 (130x9x64: two more)               one less: 7x5x252 (a single short segment)
"""

from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import f32p_cases as FC
import pde_hip
from helpers import GOLDEN
from pde_hip import _abi
from pde_hip.backend import HipBackend
from pde_hip.device import DeviceArray, GridInfo

pytestmark = pytest.mark.gpu

ALL_SHAPES = [s for nd in (1, 2, 3) for s in FC.LAPLACE_SHAPES[nd]]
FACES = {"periodic": (True, True, True), "zero-derivative": (False, False, False), "pfp": (True, False, True), "fpf": (False, True, False)}
SETTINGS = {"unit-D1": (FC.UNIT, 1.0), "cart-D0.7": (FC.DX, 0.7)}


def ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


@pytest.fixture(scope="module")
def backend():
    """A backend object of its own with the mode on (the shared "hip" backend keeps its default)."""
    b = HipBackend(name="hip-f32p")
    b.f32_arithmetic = "fp32"
    return b


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "f32p.npz", allow_pickle=False)


# ---- Laplacian vs restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx_kind", ["unit", "cart"])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=ids(ALL_SHAPES))
def test_laplace_equals_the_restatement_in_both_layouts(backend, shape, dx_kind):
    lib = backend._lib
    nd = len(shape)
    dx = (FC.UNIT if dx_kind == "unit" else FC.DX)[nd]
    info = GridInfo(shape, dx, np.float32)
    full = FC.field_data(tuple(n + 2 for n in shape), seed=sum(shape))       # ghost cells random too
    expect = FC.laplace_full(full, dx)
    src = DeviceArray(info).set_hostfull(full)
    name = "lap32_kernel<march" if FC.march_covers(shape) else f"lap32_kernel<generic,{nd}>"
    # full layout: the interior is written, the ghost cells are left alone
    marker = FC.field_data(tuple(n + 2 for n in shape), seed=1)
    dst = DeviceArray(info).set_hostfull(marker)
    lib.laplace_f32p(info.ref, src.ptr, dst.ptr, _abi.OUT_FULL, None)
    assert lib.last_kernel_name().decode().startswith(name)
    got = dst.get_hostfull()
    inner = (slice(1, -1),) * nd
    assert np.array_equal(got[inner], expect)
    marker[inner] = expect
    assert np.array_equal(got, marker)
    # valid layout
    valid = DeviceArray(info)                 # (any allocation of at least the valid size)
    lib.memset(valid.ptr, 0xFF, valid.nbytes, None)
    lib.laplace_f32p(info.ref, src.ptr, valid.ptr, _abi.OUT_VALID, None)
    assert lib.last_kernel_name().decode().startswith(name)
    host = np.empty(shape, dtype=np.float32)
    lib.memcpy_d2h(host.ctypes.data, valid.ptr, host.nbytes, None)
    assert np.array_equal(host, expect)
    assert np.array_equal(src.get_hostfull(), full)      # the input is not written


def test_supported_reports_the_instance(backend):
    lib = backend._lib
    for shape in ALL_SHAPES:
        answer = C.c_int(-1)
        lib.f32p_supported(GridInfo(shape, FC.UNIT[len(shape)], np.float32).ref, None, C.byref(answer))
        assert answer.value == (2 if FC.march_covers(shape) else 1)
    answer = C.c_int(-1)
    lib.f32p_supported(GridInfo((4, 4, 4), FC.UNIT[3], np.float64).ref, None, C.byref(answer))
    assert answer.value == 0
    with pytest.raises(NotImplementedError, match="fp32 fields only"):
        info = GridInfo((4, 4, 4), FC.UNIT[3], np.float64)
        a, b = DeviceArray(info), DeviceArray(info)
        lib.laplace_f32p(info.ref, a.ptr, b.ptr, _abi.OUT_FULL, None)


# ---- Laplacian vs goldens at field level ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc_name", list(FC.GOLDEN_LAPLACE_BCS))
@pytest.mark.parametrize("shape", FC.GOLDEN_LAPLACE_SHAPES, ids=ids(FC.GOLDEN_LAPLACE_SHAPES))
def test_field_laplace_equals_the_reference(backend, golden, shape, bc_name):
    nd = len(shape)
    grid = pde_hip.CartesianGrid(FC.bounds_for(shape, FC.DX[nd]), shape)
    field = pde_hip.ScalarField(grid, golden[f"field/{nd}d"], dtype=np.float32)
    res = field.laplace(FC.GOLDEN_LAPLACE_BCS[bc_name], backend=backend)
    assert res.data.dtype == np.float32
    assert backend._lib.last_kernel_name().decode().startswith("lap32_kernel")
    assert np.array_equal(res.data, golden[f"lap/{nd}d/{bc_name}"])


def test_default_mode_still_gives_the_oracle_bits(golden):
    """The same input through a backend in its default mode: fp64 registers, the bits of the CPU oracle - not those of the golden."""
    from oracle import pde_oracle as O
    from pde_hip.backend import convert_bcs

    shape = (9, 13, 70)
    plain = HipBackend(name="hip-default")
    assert plain.f32_arithmetic == "fp64"
    grid = pde_hip.CartesianGrid(FC.bounds_for(shape, FC.DX[3]), shape)
    bc = FC.GOLDEN_LAPLACE_BCS["mixed"]
    valid = golden["field/3d"]
    got = pde_hip.ScalarField(grid, valid, dtype=np.float32).laplace(bc, backend=plain).data
    assert not plain._lib.last_kernel_name().decode().startswith("lap32_kernel")

    class _Host:
        def __init__(self, arr):
            self.arr = np.ascontiguousarray(arr)
            self.ptr = self.arr.ctypes.data

    faces = convert_bcs(grid.get_boundary_conditions(bc), upload=_Host)
    g = _abi.make_grid(grid.shape, grid.discretization, np.float32)
    full = O.valid_to_full(grid.shape, valid)
    O.set_ghost_cells(g, 1, faces.c, full)
    assert np.array_equal(got, O.laplace(g, full))
    assert not np.array_equal(got, golden["lap/3d/mixed"])


# ---- Euler: two-step instance, one-step instance and restatement -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _expected(shape, faces, setting):
    """Restated states after 0..7 steps, computed once per case."""
    nd = len(shape)
    dxs, D = SETTINGS[setting]
    dx = dxs[nd]
    dt = FC.stable_dt(dx, D)
    states = [FC.field_data(shape, seed=3 + sum(shape))]
    for _ in range(max(FC.EULER_STEPS)):
        states.append(FC.euler_steps(states[-1], dx, FACES[faces][:nd], D, dt, 1))
    for s in states:
        s.setflags(write=False)
    return states, dt


def _spec(backend, shape, faces, setting):
    nd = len(shape)
    dxs, D = SETTINGS[setting]
    grid = pde_hip.CartesianGrid(FC.bounds_for(shape, dxs[nd]), shape, periodic=list(FACES[faces][:nd]))
    eq = pde_hip.DiffusionPDE(D)              # auto_periodic_neumann
    return backend.make_rhs_spec(eq, pde_hip.ScalarField(grid, dtype=np.float32))


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("faces", list(FACES))
@pytest.mark.parametrize("shape", FC.EULER_SHAPES, ids=ids(FC.EULER_SHAPES))
def test_euler_instances_equal_the_restatement(backend, shape, faces, setting):
    lib = backend._lib
    states, dt = _expected(shape, faces, setting)
    spec = _spec(backend, shape, faces, setting)
    answer = C.c_int(-1)
    lib.f32p_supported(spec.info.ref, spec.ref, C.byref(answer))
    two_step = FC.two_step_covers(shape)
    assert answer.value == (2 if two_step else 1)
    for generic in (False, True):
        spec.c.reserved = _abi.RHS_F32P_ONE_STEP if generic else 0       # per call: the one-step instance on every grid
        fast = two_step and not generic
        for steps in FC.EULER_STEPS:
            a, b = DeviceArray(spec.info).set_valid(states[0]), DeviceArray(spec.info)
            res = C.c_void_p()
            lib.euler_run_f32p(spec.info.ref, spec.ref, a.ptr, b.ptr, dt, steps, C.byref(res), None)
            name = lib.last_kernel_name().decode()
            if fast and steps >= 2:
                assert name.startswith("euler32_kernel<two-step"), name
            else:
                assert name == f"euler32_kernel<generic,{len(shape)}>", name
            sweeps = steps // 2 + steps % 2 if fast else steps
            assert res.value == (a.ptr if sweeps % 2 == 0 else b.ptr)          # the buffers ping-pong, one swap per sweep
            got = (b if res.value == b.ptr else a).get_valid()
            assert np.array_equal(got, states[steps]), (steps, name, int((got != states[steps]).sum()))


def test_euler_zero_steps_and_refusals_launch_nothing(backend):
    lib = backend._lib
    shape = (8, 4, 260)
    spec = _spec(backend, shape, "periodic", "unit-D1")
    data = FC.field_data(shape, seed=5)
    a, b = DeviceArray(spec.info).set_valid(data), DeviceArray(spec.info)
    res = C.c_void_p()
    lib.euler_run_f32p(spec.info.ref, spec.ref, a.ptr, b.ptr, 0.01, 0, C.byref(res), None)
    assert res.value == a.ptr and np.array_equal(a.get_valid(), data)
    # inhomogeneous faces: refused by the dry run and by the call, before anything is launched (the buffers keep their contents)
    grid = pde_hip.CartesianGrid(FC.bounds_for(shape, FC.DX[3]), shape, periodic=[True, False, True])
    for bc in ({"y": {"value": 0.537}, "x": "periodic", "z": "periodic"}, {"y": {"derivative": -1.13}, "x": "periodic", "z": "periodic"},
               {"y": {"type": "mixed", "value": 0.51, "const": 1.07}, "x": "periodic", "z": "periodic"}):
        bad = backend.make_rhs_spec(pde_hip.DiffusionPDE(0.7, bc=bc), pde_hip.ScalarField(grid, dtype=np.float32))
        answer = C.c_int(-1)
        lib.f32p_supported(bad.info.ref, bad.ref, C.byref(answer))
        assert answer.value == 0
        before = lib.last_kernel_name()
        lib.memset(b.ptr, 0, b.nbytes, None)
        with pytest.raises(NotImplementedError, match="neither periodic nor zero-derivative"):
            lib.euler_run_f32p(bad.info.ref, bad.ref, a.ptr, b.ptr, 0.01, 2, C.byref(res), None)
        assert lib.last_kernel_name() == before
        assert np.array_equal(a.get_valid(), data) and not b.get_valid().any()
        with pytest.raises(NotImplementedError, match="f32_arithmetic"):
            pde_hip.DiffusionPDE(0.7, bc=bc).solve(pde_hip.ScalarField(grid, data, dtype=np.float32), t_range=0.02, dt=0.01, backend=backend,
                                                   solver="euler", tracker=None)


def test_a_second_run_of_the_stepper_continues(backend):
    from pde_hip.solvers import SolverBase

    shape, faces, setting = (9, 3, 1024), "pfp", "cart-D0.7"
    states, dt = _expected(shape, faces, setting)
    dxs, D = SETTINGS[setting]
    grid = pde_hip.CartesianGrid(FC.bounds_for(shape, dxs[3]), shape, periodic=list(FACES[faces]))
    state = pde_hip.ScalarField(grid, states[0], dtype=np.float32)
    solver = SolverBase.from_name("euler", pde=pde_hip.DiffusionPDE(D), backend=backend)
    stepper = solver.make_stepper(state, dt)
    stepper(state, 0.0, 3 * dt)
    assert backend._lib.last_kernel_name().decode().startswith("euler32_kernel<two-step")
    assert np.array_equal(state.data, states[3])
    stepper(state, 3 * dt, 7 * dt)
    assert np.array_equal(state.data, states[7])
    assert solver.info["steps"] == 7


# ---- Euler vs goldens through eq.solve --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", FC.GOLDEN_EULER_STEPS)
@pytest.mark.parametrize("case", FC.GOLDEN_EULER_CASES, ids=[c[0] for c in FC.GOLDEN_EULER_CASES])
def test_solve_equals_the_reference(backend, golden, case, steps):
    cid, shape, periodic = case
    nd = len(shape)
    grid = pde_hip.CartesianGrid(FC.bounds_for(shape, FC.DX[nd]), shape, periodic=list(periodic))
    dt = FC.stable_dt(grid.discretization, FC.GOLDEN_D)
    state = pde_hip.ScalarField(grid, golden[f"field/{nd}d"], dtype=np.float32)
    res, info = pde_hip.DiffusionPDE(FC.GOLDEN_D).solve(state, t_range=steps * dt, dt=dt, backend=backend, solver="euler", tracker=None, ret_info=True)
    assert info["solver"]["steps"] == steps
    assert backend._lib.last_kernel_name().decode().startswith("euler32_kernel")
    assert res.data.dtype == np.float32
    assert np.array_equal(res.data, golden[f"euler/{cid}/{steps}"])


def test_refused_operators_raise_before_anything_is_launched(backend):
    grid = pde_hip.UnitGrid([8, 8])
    field = pde_hip.ScalarField(grid, FC.field_data((8, 8)), dtype=np.float32)
    before = backend._lib.last_kernel_name()
    for call in (lambda: field.gradient("auto_periodic_neumann", backend=backend), lambda: field.laplace("auto_periodic_neumann", backend=backend, corner_weight=0.5)):
        with pytest.raises(NotImplementedError, match="f32_arithmetic"):
            call()
    assert backend._lib.last_kernel_name() == before
    # fp64 fields are not affected by the mode
    f64 = pde_hip.ScalarField(grid, FC.field_data((8, 8)).astype(np.float64))
    assert f64.gradient("auto_periodic_neumann", backend=backend).data.dtype == np.float64
