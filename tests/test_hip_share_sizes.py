"""GPU parity of the decomposed loops AT THE SHARE SIZES of the benchmark (ONE GPU: libpdehip + RCCL to self).

tests/test_hip_distributed.py runs the slab and block loops on toy grids.  Size selects code there: the store form (streaming stores
beyond 192 MiB per launch), the chunking of the march axis (the "thin" rule of sub-slabs below 96 layers against the cost model), the
all-periodic-rows body `euler2_peryz_kernel`, and - only at size - launches that really run side by side on the two streams of the
pipelined four-steps-per-exchange schedule.  Here the same loops run on the shares BASELINE.md and bench.py name (64 / 128 / 256 x 512 x
512 fp64 slabs and 256 x 128 x 512 / 256^3 blocks of cfg4, the 32 x 256 x 256 fp32 slab of cfg5), world size 1 with
``force_exchange=True``, and every case compares the WHOLE field with the CPU oracle bit for bit and asserts which kernel instance /
loop it ran, so that a threshold that moves and drops an instance from the suite fails a test.  No torch in this file.
"""

from __future__ import annotations

import ctypes as C
import functools
import json

import numpy as np
import pytest
from helpers import GOLDEN, expect_steps, max_rel
from test_oracle_golden import oracle_solve

import pde_hip
from pde_hip import _abi

pytestmark = pytest.mark.gpu

DT = 0.05
FACES = {"x": "periodic", "y-": {"value": 0.2}, "y+": {"value": -0.1}, "z-": {"derivative": -0.1}, "z+": {"type": "mixed", "value": 0.5, "const": 0.2}}
# value / derivative / mixed faces on all three axes (a rank that owns both physical faces of the slowest axis)
PAIRS = [({"value": 0.4}, {"derivative": -0.2}), ({"derivative": 0.3}, {"value": -0.1}), ({"type": "mixed", "value": 0.5, "const": 0.2}, {"value": 0.0})]


@functools.lru_cache(maxsize=3)
def _data(shape, dtype="float64", lo=-1.0, hi=1.0):
    """Seeded random data in (lo, hi); cached, so treated as read-only."""
    out = np.random.default_rng(20 + len(shape)).uniform(lo, hi, shape).astype(dtype)
    out.setflags(write=False)
    return out


def _setup(kind, shape):
    """(grid, equation, diffusivity) of the three instances: `unit` - all-periodic UnitGrid, D = 1 (what bench.py times); `cart` - the same
    with unequal spacings and D = 0.7 (the general E2_DIFFUSION instance); `faces` - local faces on the rows and the fastest axis."""
    if kind == "unit":
        return pde_hip.UnitGrid(shape, periodic=True), pde_hip.DiffusionPDE(1.0), 1.0
    if kind == "cart":
        grid = pde_hip.CartesianGrid([[0, shape[0] * 0.8], [0, shape[1] * 1.25], [0, shape[2] * 1.1]], shape, periodic=True)
        return grid, pde_hip.DiffusionPDE(0.7), 0.7
    assert kind == "faces"
    return pde_hip.UnitGrid(shape, periodic=[True, False, False]), pde_hip.DiffusionPDE(0.7, bc=FACES), 0.7


@functools.lru_cache(maxsize=6)
def _expect_diffusion(kind, shape, dtype, steps):
    grid, eq, D = _setup(kind, shape)
    out = expect_steps(_abi.RHS_DIFFUSION, D, grid, eq.bc, _data(shape, dtype), DT, steps)
    out.setflags(write=False)
    return out


def _moved(final, data):
    """A loop that did nothing must not pass."""
    assert np.abs(final.astype(np.float64) - data).max() > 1e-3


def _kernel_name(lib) -> str:
    return lib.last_kernel_name().decode()


def _assert_name(name, *parts):
    """Parts of the name of the instance launched last (the tests-only host shim has no kernels: development runs on a CPU skip this)."""
    if name.startswith("host shim"):
        return
    for part in parts:
        assert part in name, (part, name)


def _store_form(layers, plane_cells, itemsize=8):
    """launch_euler2_tv: streaming stores where the field of ONE launch exceeds 192 MiB."""
    return "NT" if layers * plane_cells * itemsize > 192 * 1048576 else "plain stores"


def _slab_run(kind, shape, steps, dtype="float64", force=True):
    from pde_hip.distributed import SlabStepper

    grid, eq, _ = _setup(kind, shape)
    data = _data(shape, dtype)
    st = SlabStepper(eq, grid, np.dtype(dtype), force_exchange=force)
    try:
        assert st.exchanging == force
        final, info = st.solve(data, t_range=steps * DT, dt=DT, solver="euler")
        name = _kernel_name(st.lib)
        flags = (st._euler2, st._euler4)
    finally:
        st.close()
        del st
    assert info["steps"] == steps
    assert final.dtype == np.dtype(dtype)
    _moved(final, data)
    np.testing.assert_array_equal(final, _expect_diffusion(kind, shape, dtype, steps))
    return info, flags, name


def _interior_instance(kind, name, layers, plane_cells=512 * 512):
    """What launch_euler2_tv is documented to choose for an interior sweep of `layers` layers with halo planes on both sides."""
    store = _store_form(layers, plane_cells)
    if kind == "faces":
        _assert_name(name, "euler2_kernel<double,2,4,", "3-D", "aligned rows", "two-sided", store)
    else:
        _assert_name(name, "euler2_peryz_kernel", "E2_DIFFUSION_UNIT" if kind == "unit" else "E2_DIFFUSION,", store)


# ---- 1. the slab Euler loop at the cfg4 shares ------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [13, 16])
@pytest.mark.parametrize("mode", ["1", "2", "3", "4"])
@pytest.mark.parametrize("kind", ["unit", "cart", "faces"])
def test_slab_euler4_loop_at_64_layers_every_schedule(monkeypatch, kind, mode, steps):
    """64 x 512 x 512 fp64 to self, four steps per exchange, every schedule of `pdehip_slab_euler4_run` (3 is the default: the boundary
    layers a group ahead on the halo stream beside an interior sweep of tens of microseconds), 13 = 3 groups + 1 and 16 steps: the whole
    field equals the oracle bit for bit.  The interior sweeps (60 / 56 layers: the thin chunking rule, plain stores) run
    `euler2_peryz_kernel` on periodic rows, the general 4-row tile with local faces."""
    monkeypatch.setenv("PDEHIP_SLAB_DEEP_MODE", mode)
    info, (e2, e4), name = _slab_run(kind, (64, 512, 512), steps)
    assert e2 and e4 and info["steps_per_exchange"] == 4
    if steps == 16:   # (13 steps end in a single step of the one-level kernel)
        _interior_instance(kind, name, 64 if mode == "1" else 56)   # last launch: B of 64 layers (schedule 1), B_int of 56 (others)
        _assert_name(name, "plain stores")


@pytest.mark.parametrize("kind", ["unit", "cart", "faces"])
@pytest.mark.parametrize("layers", [128, 256])
def test_slab_euler4_loop_at_128_and_256_layers(monkeypatch, kind, layers):
    """128 and 256 x 512 x 512 fp64 to self in the default schedule: interior sweeps of layers - 4 and layers - 8 layers go through the cost
    model of the x-chunks (96 layers and more) and store with streaming stores (240 MiB and more per launch)."""
    monkeypatch.delenv("PDEHIP_SLAB_DEEP_MODE", raising=False)
    steps = 16 if layers == 128 else 14    # (14 = 3 groups + one two-step sweep)
    info, (e2, e4), name = _slab_run(kind, (layers, 512, 512), steps)
    assert e2 and e4 and info["steps_per_exchange"] == 4
    _interior_instance(kind, name, layers - 8 if steps % 4 == 0 else layers)
    _assert_name(name, "NT")


@pytest.mark.parametrize("env,per_exchange", [("PDEHIP_SLAB_EULER4", 2), ("PDEHIP_SLAB_EULER2", 1)])
def test_slab_loops_with_two_and_one_step_per_exchange_at_64_layers(monkeypatch, env, per_exchange):
    monkeypatch.setenv(env, "0")
    info, (e2, e4), name = _slab_run("unit", (64, 512, 512), 13)
    assert info["steps_per_exchange"] == per_exchange and not e4 and e2 == (per_exchange == 2)


@pytest.mark.parametrize("kind,layers", [("unit", 64), ("unit", 128), ("unit", 256), ("cart", 64), ("faces", 64), ("faces", 256)])
def test_slab_share_without_exchange(kind, layers):
    """The benchmark's `without_exchange` column: the same shares, the periodic slowest axis wrapped inside the kernel."""
    info, (e2, e4), name = _slab_run(kind, (layers, 512, 512), 16, force=False)
    assert info["steps_per_exchange"] == 1 and not e2 and not e4
    field = _store_form(layers, 512 * 512)
    if kind == "faces":
        _assert_name(name, "euler2_kernel<double,2,4,", "aligned rows", "two-sided", field)
    else:   # all-periodic: the instances without the face code; 8-row tiles beyond 400 MiB
        _assert_name(name, "euler2_tall_per_kernel" if layers == 256 else "euler2_per_kernel", field)


@pytest.mark.parametrize("steps", [13, 16])
def test_slab_euler4_loop_fp32_at_64_layers(monkeypatch, steps):
    """fp32 storage, fp64 registers: bit-equal to the oracle built for fp32."""
    monkeypatch.delenv("PDEHIP_SLAB_DEEP_MODE", raising=False)
    info, (e2, e4), name = _slab_run("unit", (64, 512, 512), steps, dtype="float32")
    assert e2 and e4 and info["steps_per_exchange"] == 4
    if steps == 16:
        _assert_name(name, "euler2_kernel<float,4,2,", "two-sided", "plain stores")


@pytest.mark.parametrize("kind", ["unit", "faces"])
@pytest.mark.parametrize("shape", [(64, 513, 513), (64, 500, 300)])
def test_slab_euler4_loop_on_off_tile_shares(monkeypatch, kind, shape):
    """Rows that end inside a chunk / a vector and row counts that are no multiple of the tile (moved last tiles, the ragged-row
    instances) next to the slab's halo planes - tests/test_hip_tails.py covers these extents for the undecomposed sweep only."""
    monkeypatch.delenv("PDEHIP_SLAB_DEEP_MODE", raising=False)
    for steps in (13, 16):
        info, (e2, e4), name = _slab_run(kind, shape, steps)
        assert e2 and e4 and info["steps_per_exchange"] == 4
    _assert_name(name, "euler2_kernel<double,2,4,", "ragged", "two-sided", "plain stores")
    info, flags, _ = _slab_run(kind, shape, 16, force=False)      # open rows / open columns of the undecomposed sweep
    assert flags == (False, False)


@pytest.mark.parametrize("kind", ["unit", "cart"])
@pytest.mark.parametrize("layers,chunking", [(56, "thin"), (60, "thin"), (120, "cost model"), (124, "cost model"), (252, "cost model")])
def test_interior_instances_of_the_shares_by_direct_call(kind, layers, chunking):
    """The interior launches of the loops above by themselves (`pdehip_diffusion_euler2_slab`, two real layers beyond both ends): the
    sub-slabs of 56 / 60 layers a 64-layer share issues (below 96 layers: the thin rule, at most 1536 waves), of 120 / 124 and 252 layers
    (the cost model; streaming stores).  In a loop run only the LAST launch leaves its name; here each instance is named next to a
    comparison of every cell it wrote."""
    from pde_hip.backend import convert_bcs
    from pde_hip.device import DeviceArray, GridInfo

    lib = pde_hip.get_backend("hip")._lib
    if _kernel_name(lib).startswith("host shim"):
        pytest.skip("development run on a CPU: the host shim has no sub-slab launch")
    shape = (layers + 4, 512, 512)
    grid, _, D = _setup(kind, shape)
    data = _data(shape)
    info = GridInfo(grid.shape, grid.discretization, np.float64)
    sub = GridInfo((layers, 512, 512), grid.discretization, np.float64)
    faces = convert_bcs(grid.get_boundary_conditions("periodic"))
    f = _abi.FaceArray()
    for i in range(6):
        f[i] = faces.c[i]
    f[0].kind = f[1].kind = _abi.BC_SKIP
    a, b = DeviceArray(info).set_valid(data), DeviceArray(info).set_valid(np.zeros(shape))
    done = C.c_int(0)
    lp = info.layer_pitch * 8
    lib.diffusion_euler2_slab(sub.ref, f, a.ptr + 2 * lp, b.ptr + 2 * lp, D, DT, 1, C.byref(done), None)
    lib.stream_synchronize(None)
    assert done.value == 1
    assert (chunking == "thin") == (layers < 96)
    _assert_name(_kernel_name(lib), "euler2_peryz_kernel", "E2_DIFFUSION_UNIT" if kind == "unit" else "E2_DIFFUSION,", _store_form(layers, 512 * 512))
    got = b.get_valid()
    del a, b
    # (two steps reach two layers far: layers 2 .. n+1 of the periodic run do not see how the slowest axis ends)
    expect = expect_steps(_abi.RHS_DIFFUSION, D, grid, "periodic", data, DT, 2)
    _moved(got[2:-2], data[2:-2])
    np.testing.assert_array_equal(got[2:-2], expect[2:-2])
    assert not got[:2].any() and not got[-2:].any()      # nothing written outside the sub-slab


# ---- 2. the same loop between physical faces, at size -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 512, 512), (64, 513, 513)])
def test_slab_loops_between_physical_faces_at_size(shape):
    """`pdehip_slab_euler4_run`, `_euler2_run` and `_euler_run` on a rank WITHOUT neighbours (direct C calls, lower = upper = -1, no RCCL):
    value / derivative / mixed faces on all three axes; the sweeps meet the physical faces of the slowest axis."""
    from pde_hip.backend import convert_bcs
    from pde_hip.device import DeviceArray, GridInfo
    from pde_hip.distributed import SlabStepper

    grid = pde_hip.UnitGrid(shape, periodic=False)
    bc = {f"{a}{s}": v for a, (lo, hi) in zip(grid.axes, PAIRS) for s, v in (("-", lo), ("+", hi))}
    data = _data(shape)
    helper = SlabStepper(pde_hip.DiffusionPDE(), pde_hip.UnitGrid(shape, periodic=True), force_exchange=True)   # (a communicator of size 1)
    lib, comm = helper.lib, helper.comm
    info = GridInfo(grid.shape, grid.discretization, np.float64)
    rhs = _abi.RHS()
    rhs.kind, rhs.param = _abi.RHS_DIFFUSION, 0.6
    convert_bcs(grid.get_boundary_conditions(bc)).copy_into(rhs.bc_c)
    ok = C.c_int(0)
    lib.slab_euler4_supported(info.ref, C.byref(rhs), C.byref(ok))
    assert ok.value
    a, b = DeviceArray(info), DeviceArray(info)
    res = C.c_void_p()
    for run, steps in [(lib.slab_euler4_run, 13), (lib.slab_euler4_run, 16), (lib.slab_euler2_run, 5), (lib.slab_euler_run, 5)]:
        a.set_valid(data)
        run(comm, info.ref, C.byref(rhs), -1, -1, a.ptr, b.ptr, DT, steps, C.byref(res), None)
        lib.stream_synchronize(None)
        got = (b if res.value == b.ptr else a).get_valid()
        _moved(got, data)
        np.testing.assert_array_equal(got, expect_steps(_abi.RHS_DIFFUSION, 0.6, grid, bc, data, DT, steps), err_msg=f"{steps} steps")
        if steps == 16:
            if shape[1] % 4:   # 513 rows / columns: left open behind the tiles, recomputed by the kernel of the open rows (the name of the tiles stays)
                _assert_name(_kernel_name(lib), "euler2_kernel<double,2,4,", "two-sided", "plain stores")
            else:
                _assert_name(_kernel_name(lib), "euler2_kernel<double,2,4,", "aligned rows", "two-sided", "plain stores")
    del a, b
    helper.close()


# ---- 3. "supported" means "runs" --------------------------------------------------------------------------------------------------
_N1 = [4, 5, 7, 8, 9, 12, 13, 64, 65]
_N2 = [64, 65, 72, 128, 129, 130, 136, 264]
EDGE_SHAPES = [(8 + i % 13, _N1[i % 9], _N2[i % 8]) for i in range(60)]     # (13, 9 and 8 are coprime: 60 different shapes)
FACE_SETS = {
    "x-faces": [PAIRS[0], None, None],
    "xz-faces": [PAIRS[1], None, PAIRS[2]],
    "all-faces": PAIRS,
}


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("face_set", list(FACE_SETS))
def test_supported_slab_euler4_shapes_run_in_every_schedule(monkeypatch, face_set, dtype):
    """Contract of `pdehip_slab_euler4_supported` on the no-neighbour call (lower = upper = -1: no RCCL group is open, a refusal is an error
    code and nothing waits): wherever it answers 1, nine steps of `pdehip_slab_euler4_run` succeed in every schedule and equal the
    oracle; where it answers 0, `SlabStepper` keeps off the loop and still solves the grid.  Shapes around the dispatcher's edges."""
    from pde_hip.backend import convert_bcs
    from pde_hip.device import DeviceArray, GridInfo
    from pde_hip.distributed import SlabStepper

    assert len(set(EDGE_SHAPES)) == 60
    helper = SlabStepper(pde_hip.DiffusionPDE(), pde_hip.UnitGrid((8, 4, 64), periodic=True), force_exchange=True)
    lib, comm = helper.lib, helper.comm
    pairs = FACE_SETS[face_set]
    supported = 0
    for shape in EDGE_SHAPES:
        grid = pde_hip.UnitGrid(shape, periodic=[p is None for p in pairs])
        bc = {}
        for ax, p in zip(grid.axes, pairs):
            bc.update({ax: "periodic"} if p is None else {f"{ax}-": p[0], f"{ax}+": p[1]})
        data = np.random.default_rng(sum(shape)).uniform(-1, 1, shape).astype(dtype)
        info = GridInfo(grid.shape, grid.discretization, np.dtype(dtype))
        rhs = _abi.RHS()
        rhs.kind, rhs.param = _abi.RHS_DIFFUSION, 0.6
        convert_bcs(grid.get_boundary_conditions(bc)).copy_into(rhs.bc_c)
        ok = C.c_int(0)
        lib.slab_euler4_supported(info.ref, C.byref(rhs), C.byref(ok))
        expect = expect_steps(_abi.RHS_DIFFUSION, 0.6, grid, bc, data, DT, 9)
        assert np.abs(expect - data).max() > 1e-3
        if ok.value:
            supported += 1
            a, b = DeviceArray(info), DeviceArray(info)
            res = C.c_void_p()
            for mode in ("1", "2", "3", "4"):
                monkeypatch.setenv("PDEHIP_SLAB_DEEP_MODE", mode)
                a.set_valid(data)
                # (a refusal inside the loop is an error code: the binding raises)
                lib.slab_euler4_run(comm, info.ref, C.byref(rhs), -1, -1, a.ptr, b.ptr, DT, 9, C.byref(res), None)
                lib.stream_synchronize(None)
                np.testing.assert_array_equal((b if res.value == b.ptr else a).get_valid(), expect, err_msg=f"{shape} schedule {mode}")
        else:
            monkeypatch.delenv("PDEHIP_SLAB_DEEP_MODE", raising=False)
            st = SlabStepper(pde_hip.DiffusionPDE(0.6, bc=bc), grid, np.dtype(dtype))
            assert not st._euler4
            final, sinfo = st.solve(data, t_range=9 * DT, dt=DT, solver="euler")
            st.close()
            assert sinfo["steps"] == 9
            np.testing.assert_array_equal(final, expect, err_msg=f"{shape} not supported")
    helper.close()
    assert supported >= 30      # (the list is about the loop: most of it must reach the loop)


# ---- 4. the fast block loop at the cfg4 blocks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [(1, 1, 0), (1, 1, 1)])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape", [(256, 128, 512), (256, 256, 256), (130, 129, 520)])
def test_fast_block_loop_at_the_cfg4_blocks(shape, dtype, cut):
    """`BlockStepper(force_exchange=True)` with the fast loop (csrc/pdehip_block2_loops.h) on the blocks of 512^3 over 8 devices - 256 x 128 x
    512 (`2,4,1`) and 256^3 (`auto`) - and one block off the tile sizes: two steps per sweep on the box (the boxed cap of 1792 waves), the
    rim recomputed behind the exchange, 6 and 7 steps, bit-identical to the oracle's single steps."""
    from pde_hip.distributed import BlockStepper

    grid = pde_hip.CartesianGrid([[0, n * 0.8] for n in shape], shape, periodic=True)
    eq = pde_hip.DiffusionPDE(0.6)
    data = _data(shape, dtype, -0.5, 0.5)
    st = BlockStepper(eq, grid, np.dtype(dtype), force_exchange=True)
    try:
        assert st.exchanging and st.block2 and list(st.cut) == [1, 1, 0]
        st.cut[:] = cut
        st._cut3 = (C.c_int * 3)(*st.cut)
        ok = C.c_int(0)
        st.lib.block2_supported(st.info.ref, C.byref(st._rhs2), st._cut3, C.byref(ok))
        assert ok.value == 1
        for steps in (6, 7):
            final, info = st.solve(data, t_range=steps * 0.02, dt=0.02, solver="euler")
            assert info["steps"] == steps
            _moved(final, data)
            np.testing.assert_array_equal(final, expect_steps(_abi.RHS_DIFFUSION, 0.6, grid, "periodic", data, 0.02, steps), err_msg=f"{steps} steps")
            del final
    finally:
        st.close()
        del st


# ---- 5. the Runge-Kutta loops in C and the cfg5 share -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,t_range", [("diffusion", (64, 512, 512), 0.3), ("cahn_hilliard", (32, 256, 256), 0.05), ("cahn_hilliard", (64, 512), 0.05)])
def test_rk4_and_adaptive_rkf45_at_the_shares(kind, shape, t_range):
    """`pdehip_slab_rk4_run` / `pdehip_slab_rkf45_run` to self at size: bit-identical final state, equal step counts and the same next dt
    as the serial oracle loop (the assertions of test_rk4_and_adaptive_rkf45_in_one_c_call)."""
    from pde_hip.distributed import SlabStepper

    grid = pde_hip.UnitGrid(shape, periodic=True)
    data = _data(shape, "float64", -0.1, 0.1)
    eq = pde_hip.DiffusionPDE(0.5) if kind == "diffusion" else pde_hip.CahnHilliardPDE(1.0)
    code, param = (_abi.RHS_DIFFUSION, 0.5) if kind == "diffusion" else (_abi.RHS_CAHN_HILLIARD, 1.0)
    st = SlabStepper(eq, grid, force_exchange=True)
    try:
        assert st.exchanging
        final, info = st.solve(data, t_range=3e-3, dt=1e-3, solver="runge-kutta")
        assert info["steps"] == 3
        np.testing.assert_array_equal(final, expect_steps(code, param, grid, "auto_periodic_neumann", data, 1e-3, 3, "runge-kutta"))
        final2, info2 = st.solve(data, t_range=t_range, dt=None, solver="runge-kutta")
    finally:
        st.close()
        del st
    case = {"pde": kind, "D": 0.5, "gamma": 1.0, "bc": "auto_periodic_neumann", "t_range": t_range, "dt": None, "solver": "runge-kutta"}
    expect, steps, dt_last = oracle_solve(case, grid, np.float64, data)
    assert 5 <= steps <= 10
    assert info2["steps"] == steps and info2["attempts"] >= steps
    assert info2["dt"] == pytest.approx(dt_last, rel=1e-12)
    assert np.abs(final2 - data).max() > 1e-3
    np.testing.assert_array_equal(final2, expect)


@pytest.mark.parametrize("dims", ["slab", "auto"])
def test_cfg5_share_expression_rkf45_to_self(dims):
    """The slab of cfg5 over 8 devices: `PDE({'c': 'laplace(c**3 - c - laplace(c))'})`, 32 x 256 x 256 fp32 periodic, adaptive RKF45 with the
    tolerance, first dt and t_range of the case definition, the ghost layers of every operand through RCCL to self (twelve exchanges per
    attempt): equal to the single-GPU run bit for bit with an equal step count, and within 1e-5 of the oracle's adaptive loop."""
    from pde_hip.distributed import DecomposedExpressionStepper

    cases = json.loads(str(np.load(GOLDEN / "configs.npz", allow_pickle=False)["cases"]))
    case = next(c for c in cases if c["id"] == "cfg5_expression_256cube_f32_rkf45")
    assert case["dtype"] == "float32" and case["adaptive"] and case["dt"] == 1e-3 and case["solver"] == "runge-kutta"
    shape = (32, 256, 256)
    grid = pde_hip.UnitGrid(shape, periodic=True)
    data = _data(shape, "float32", case["vmin"], case["vmax"])
    eq = pde_hip.PDE(case["rhs"], bc=case["bc"])
    state = pde_hip.ScalarField(grid, data, dtype=np.float32)
    serial, info = eq.solve(state, case["t_range"], None, solver="runge-kutta", backend="hip", ret_info=True)
    assert serial.data.dtype == np.float32 and np.isfinite(serial.data).all()
    st = DecomposedExpressionStepper(eq, state, dims=dims, force_exchange=True)
    try:
        assert st.comm is not None and st.blocks == (dims == "auto")
        final, sinfo = st.solve(data, case["t_range"], None, "runge-kutta")
    finally:
        st.close()
        del st
    assert sinfo["steps"] == info["solver"]["steps"]
    np.testing.assert_array_equal(final, serial.data)
    ocase = {"pde": "cahn_hilliard", "gamma": 1.0, "bc": case["bc"], "t_range": case["t_range"], "dt": None, "solver": "runge-kutta"}
    expect, steps, _ = oracle_solve(ocase, grid, np.float32, data)
    assert sinfo["steps"] == steps and steps >= 5
    assert np.abs(final.astype(np.float64) - data).max() > 1e-3
    assert max_rel(final.astype(np.float64), expect.astype(np.float64)) < 1e-5


# ---- 6. the same bits every time ---------------------------------------------------------------------------------------------------
def test_share_runs_are_repeatable(monkeypatch):
    """64 x 512 x 512 periodic, default schedule: three 16-step solves on one stepper, a 13-step solve in between and a fresh stepper all
    give the oracle's bits (three state arrays in rotation and the private arrays reused from run to run, freed on close)."""
    from pde_hip.distributed import SlabStepper

    monkeypatch.delenv("PDEHIP_SLAB_DEEP_MODE", raising=False)
    shape = (64, 512, 512)
    grid, eq, _ = _setup("unit", shape)
    data = _data(shape)
    expect = _expect_diffusion("unit", shape, "float64", 16)
    for fresh in range(2):
        st = SlabStepper(eq, grid, force_exchange=True)
        try:
            assert st._euler4
            for steps in ((16, 16, 13, 16) if fresh == 0 else (16,)):
                final, info = st.solve(data, t_range=steps * DT, dt=DT, solver="euler")
                assert info["steps"] == steps
                if steps == 16:
                    np.testing.assert_array_equal(final, expect)
                else:
                    np.testing.assert_array_equal(final, _expect_diffusion("unit", shape, "float64", 13))
        finally:
            st.close()
            del st
