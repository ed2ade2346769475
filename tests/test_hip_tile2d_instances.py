"""The multi-step 2-D tile kernel (csrc/pdehip_tile2d.inc) instance by instance: five modes, two tile widths, two types (tests/tile2d_cases.py;
tests/test_tile2d_cases_cpu.py pins the table and keeps its cases from being vacuous).

Modes 0 and 1 (``pdehip_euler_multi_2d``) on the smallest grids that get 64-column tiles and on the grid one tile short of them: the oracle's bits,
the restated instance name, and the WHOLE allocation of input and output compared - the input unchanged, the output changed in its valid cells only
(`small_kernel_cases.Layout`).  Special values through both widths.

Modes 2-4 (run-time built, ``pdehip_jit_euler_run`` through ``eq.solve``): the name of the last launch (mode, width, levels of the remainder) after a
mark, fp64 against the host shim bit for bit, fp32 against the same solve with ``PDEHIP_EXPR_LOOP=0`` (the one-level kernels) bit for bit and against
the shim within `FP32_SHIM_BOUND`.  The refusals of the table must record the one-level instance of their grid (no tile kernel) and still give
the shim's result.
"""

from __future__ import annotations

import ctypes as C
import time

import numpy as np
import pytest
import jit_cases as J
import small_kernel_cases as S
import tile2d_cases as T
from helpers import max_rel

import pde_hip
from pde_hip.device import DeviceArray

pytestmark = pytest.mark.gpu

# fp32 storage, device against shim.  The shim rounds the stencil values to fp32 between the oracle's operator and the epilogue, the kernels keep
# them in fp64 registers; the difference grows with the step count (up to 19 here).  MEASURED: the largest max_rel between the shim and the
# PDEHIP_EXPR_LOOP=0 run (neither is the tile kernel) over all fp32 cases of the table, on an MI355X; the bound is four times that
# (profiles/tile2d_tests_mutations.md).
FP32_SHIM_MEASURED = 2.3782e-07
FP32_SHIM_BOUND = 4 * FP32_SHIM_MEASURED

REPORT = {"fp32 max_rel(shim, one-level kernels)": 0.0, "fp32 max_rel(tile kernel, shim)": 0.0, "cases": 0, "names": set(), "seconds": 0.0}


@pytest.fixture(scope="module")
def backend():
    return pde_hip.get_backend("hip")


@pytest.fixture(scope="module", autouse=True)
def _report():
    start = time.perf_counter()
    yield
    REPORT["seconds"] = round(time.perf_counter() - start, 2)
    print("\ntile kernel instances: " + ", ".join(f"{k}: {sorted(v) if isinstance(v, set) else v}" for k, v in REPORT.items()))


# ---- the mark: a built-in launch no case uses (seven levels of diffusion in fp32 on one tile) --------------------------------------
_MARK = {}
MARK_NAME = "tile2d_kernel<float,mode=0,32x32 tile> (7 steps per launch, time levels in LDS)"


def _mark(backend):
    if not _MARK:
        grid = pde_hip.UnitGrid([5, 7], periodic=True)
        data = np.zeros(grid.shape, np.float32)
        spec = backend.make_rhs_spec(pde_hip.DiffusionPDE(0.5), pde_hip.ScalarField(grid, data, dtype=np.float32))
        _MARK.update(spec=spec, a=DeviceArray(spec.info).set_valid(data), b=DeviceArray(spec.info))
    done = C.c_int(0)
    backend._lib.euler_multi_2d(_MARK["spec"].info.ref, _MARK["spec"].ref, _MARK["a"].ptr, _MARK["b"].ptr, 0.01, 7, C.byref(done), None)
    assert done.value == 1
    assert backend._lib.last_kernel_name().decode() == MARK_NAME
    return MARK_NAME


def _same_bits(got, ref, what):
    """Bit equality; NaNs by position"""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{what}: NaN cells")
    bad = (S.bits(got) != S.bits(ref)) & ~nan
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        with np.errstate(all="ignore"):
            off = np.nanmax(np.abs(got[bad].astype(np.float64) - ref[bad].astype(np.float64)))
        pytest.fail(f"{what}: {int(bad.sum())} of {got.size} elements differ, first at {at}: {got[at]!r} != {ref[at]!r}, largest difference {off:.3e}")


# ---- modes 0 and 1 --------------------------------------------------------------------------------------------------------------
class _Run:
    """One grid, equation and type on the device: input and output as whole allocations"""

    def __init__(self, backend, shape, faces, kind, dtype, data):
        self.lib, self.lay = backend._lib, S.Layout(shape, dtype)
        grid = T.make_grid(shape, faces)
        self.spec = backend.make_rhs_spec(T.builtin_eq(kind, faces), pde_hip.ScalarField(grid, data, dtype=np.dtype(dtype)))
        eight = (C.c_int64 * 8)()
        self.lib.layout(self.spec.info.ref, eight)
        assert list(eight) == self.lay.eight()
        self.a, self.b = DeviceArray(self.spec.info), DeviceArray(self.spec.info)
        assert self.a.nbytes == self.lay.nelem(1) * self.lay.dtype.itemsize
        self.where = S.interior(2)
        self.full = np.zeros((1, *self.lay.full_shape), self.lay.dtype)
        self.full[(slice(None), *self.where)] = data
        # the input: the pattern everywhere but in the valid cells (ghost cells included: the kernel makes its own)
        self.img_in = S.place(S.image(self.lay, 1), self.lay, 1, self.full, self.where)
        self.img_out = S.pattern(self.lay.nelem(1), self.lay.dtype, sign=1.0, base=4096)

    def launch(self, dt, k):
        lib = self.lib
        lib.memcpy_h2d(self.a.ptr, self.img_in.ctypes.data, self.img_in.nbytes, None)
        lib.memcpy_h2d(self.b.ptr, self.img_out.ctypes.data, self.img_out.nbytes, None)
        done = C.c_int(0)
        lib.euler_multi_2d(self.spec.info.ref, self.spec.ref, self.a.ptr, self.b.ptr, dt, k, C.byref(done), None)
        name = lib.last_kernel_name().decode()
        got_in, got_out = np.empty_like(self.img_in), np.empty_like(self.img_out)
        lib.memcpy_d2h(got_in.ctypes.data, self.a.ptr, got_in.nbytes, None)
        lib.memcpy_d2h(got_out.ctypes.data, self.b.ptr, got_out.nbytes, None)
        return done.value, name, got_in, got_out

    def expected_out(self, valid):
        full = self.full.copy()
        full[(slice(None), *self.where)] = valid
        return S.place(self.img_out.copy(), self.lay, 1, full, self.where)


@pytest.mark.parametrize("item", T.builtin_items(), ids=T.builtin_id)
def test_built_in_modes_on_the_wide_tile_and_one_tile_short_of_it(backend, item):
    shape, faces, kind, dtype = item
    mode, _, dt = T.KINDS[kind]
    data = T.field_data(shape, dtype)
    steps = T.builtin_steps(kind)
    levels = T.oracle_levels(shape, faces, kind, dtype, data, steps)
    run = _Run(backend, shape, faces, kind, dtype, data)
    for k in steps:
        _mark(backend)
        done, name, got_in, got_out = run.launch(dt, k)
        what = f"{T.builtin_id(item)}, k={k}"
        assert done == 1, what
        assert name == T.kernel_name(dtype, mode, shape, k), what
        _same_bits(got_in, run.img_in, f"{what}: the input (whole allocation)")
        _same_bits(got_out, run.expected_out(levels[k]), f"{what}: the output (whole allocation: valid cells the oracle's, the rest untouched)")
        REPORT["names"].add(name.split(" (")[0])
        REPORT["cases"] += 1


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("kind", list(T.KINDS))
@pytest.mark.parametrize("shape", T.SPECIAL_SHAPES, ids=T.SPECIAL_IDS)
def test_special_values_stay_bit_identical(backend, shape, kind, dtype):
    """Denormals, huge magnitudes, signed zeros, an infinity and a NaN in the interior, on a tile seam and next to a local face: after kmax levels
    in LDS the bits of kmax single steps of the oracle, NaNs by position (IEEE arithmetic, denormals on, no contraction, no arithmetic masking)."""
    mode, _, dt = T.KINDS[kind]
    k, faces = T.kmax(mode), T.SPECIAL_FACES
    data, _ = T.special_data(shape, dtype)
    with np.errstate(all="ignore"):
        want = T.oracle_levels(shape, faces, kind, dtype, data, [k])[k]
    assert np.isnan(want).any() and np.isfinite(want).sum() > want.size // 2      # (what else the case claims: tests/test_tile2d_cases_cpu.py)
    run = _Run(backend, shape, faces, kind, dtype, data)
    _mark(backend)
    with np.errstate(all="ignore"):
        done, name, got_in, got_out = run.launch(dt, k)
    assert done == 1 and name == T.kernel_name(dtype, mode, shape, k)
    _same_bits(got_in, run.img_in, "the input")
    _same_bits(got_out, run.expected_out(want), "special values, whole allocation")


# ---- modes 2-4 ------------------------------------------------------------------------------------------------------------------
def _device_solve(backend, c):
    """(result, name recorded since the mark or "")"""
    mark = _mark(backend)
    got = T.solve(T.jit_eq(c.mode, c.expr, c.faces), T.state_of(c.mode, c.shape, c.faces, c.dtype), c.t_start, c.dt, c.steps)
    name = backend._lib.last_kernel_name().decode()
    return got, ("" if name == mark else name)


FUSED2_NAME = "pde_kernel<fused2,float,4,RY=1,2-D> (both passes of the expression in one sweep; run-time built)"


def _one_level_name(shape, dtype):
    """The one-level run-time built instance of a grid with faces applied on the fly (restated planner: tests/jit_cases.py)."""
    return J.kernel_name(J.plan(tuple(shape), np.dtype(dtype), fused=True))


@pytest.mark.parametrize("item", T.jit_items(), ids=T.jit_item_id)
def test_run_time_built_modes(backend, monkeypatch, item):
    (mode, expr, dtype, width), cases = item
    monkeypatch.delenv("PDEHIP_EXPR_LOOP", raising=False)
    over = []
    for c in cases:
        got, name = _device_solve(backend, c)
        assert name == c.name, f"{c.id}: expected the last launch to be {c.name!r}"
        ref = T.jit_reference(c)
        assert got.dtype == ref.dtype == np.dtype(dtype)
        if dtype == "float64":
            _same_bits(got, ref, f"{c.id}: against the host shim")
        else:
            monkeypatch.setenv("PDEHIP_EXPR_LOOP", "0")
            single, other = _device_solve(backend, c)
            monkeypatch.delenv("PDEHIP_EXPR_LOOP")
            assert "tile2d_kernel" not in other, f"{c.id}: the one-level comparison ran the tile kernel: {other}"
            # (a two-pass chain of one field runs both passes in one sweep of the two-level kernel where that covers the grid)
            allowed = {_one_level_name(c.shape, dtype)} | ({FUSED2_NAME} if c.mode == 4 else set())
            assert other in allowed, f"{c.id}: the one-level comparison ran {other}"
            base, tile = max_rel(single.astype(np.float64), ref.astype(np.float64)), max_rel(got.astype(np.float64), ref.astype(np.float64))
            print(f"{c.id}: fp32 max_rel against the shim: one-level kernels {base:.3e}, tile kernel {tile:.3e}")
            REPORT["fp32 max_rel(shim, one-level kernels)"] = max(REPORT["fp32 max_rel(shim, one-level kernels)"], base)
            REPORT["fp32 max_rel(tile kernel, shim)"] = max(REPORT["fp32 max_rel(tile kernel, shim)"], tile)
            _same_bits(got, single, f"{c.id}: against the one-level kernels (PDEHIP_EXPR_LOOP=0)")
            if not tile <= FP32_SHIM_BOUND:
                over.append(f"{c.id}: {tile:.3e}")
        REPORT["names"].add(name.split(" (")[0])
        REPORT["cases"] += 1
    assert not over, f"max_rel against the shim above the bound {FP32_SHIM_BOUND:.3e}: {over}"


@pytest.mark.parametrize("index", range(len(T.refusals())), ids=[r[0] for r in T.refusals()])
def test_refusals_leave_the_mark_and_give_the_reference(backend, monkeypatch, index):
    monkeypatch.delenv("PDEHIP_EXPR_LOOP", raising=False)
    rid, eq, state, t_start, dt, steps = T.refusals()[index]
    _mark(backend)
    got = T.solve(eq, state, t_start, dt, steps)
    name = backend._lib.last_kernel_name().decode()
    assert "tile2d_kernel" not in name, f"{rid}: {name}"
    assert name == _one_level_name(state.grid.shape, "float64"), f"{rid}: {name}"
    ref = T.shim_solve(eq, state, t_start, dt, steps)
    assert ref.dtype == np.float64
    _same_bits(got, ref, f"{rid}: against the host shim")
