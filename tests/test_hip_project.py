"""Device tests of ``csrc/pdehip_project.hip``: ``pdehip_project`` and ``pdehip_extract_box`` through the C ABI, and the residency of a run
that uses them through the mirror classes.

Reference, inputs and bounds: ``tests/project_cases.py`` (a numpy restatement of the semantics in ``include/pdehip.h``; sums inside a
bound derived from the arithmetic against ``math.fsum``, maxima, minima and boxes bit for bit, non-finite cells by class).  Shapes: the
smallest at which the launch geometry can go wrong - vector widths, lane groups of 1 to 64, wave and workgroup seams, rows of 1-3 cells,
1 / 3 / 9 components, every axis subset of 1-D to 3-D grids; the removed extents around the cut of the march into segments; one shape
per instance beyond the grid-stride turn of a launch.  The chain of kernel instances every call reports is asserted against the
restatement of the host's choice.  ``tests/test_project_cpu.py`` runs the same checks on the tests-only host versions.
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest
import project_cases as P

import pde_hip
from pde_hip.device import DeviceArray, DeviceBuffer, GridInfo, ptr_array

pytestmark = pytest.mark.gpu

IDS = ["f64", "f32"]


@pytest.fixture(scope="module")
def lib():
    return pde_hip.get_backend("hip")._lib


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
@pytest.mark.parametrize("case", P.SMALL, ids=P.S.case_id)
def test_project(lib, case, dtype):
    """Every non-empty axis subset, the three methods, with distinct extremes and with NaN / +-inf in first, last and seam cells; two
    calls on fresh uploads give equal bits; the instances that ran are the ones the shape asks for."""
    shape, ncomp = case
    for planted in (False, True):
        valid = P.small_inputs(case, np.dtype(dtype).name, planted)
        P.check_all_methods(lib, valid, shape, what=f"planted={planted}", chain=lambda mask, method: P.expected_chain(shape, dtype, mask, method))


@pytest.mark.parametrize("key", sorted(P.MARCH_INSTANCES))
def test_segment_extents(lib, key):
    """The march around its cut into segments: one segment exactly (one stage), one cell more and one cell less than two segments (a
    second stage over two partial results), the removed cells on one axis and spread over two."""
    dtype, n2 = P.MARCH_INSTANCES[key]
    for m in P.SEGMENT_EXTENTS:
        for shape in ((m, 2, n2), (3, -(-m // 3), n2)):
            valid = P.drawn(shape, 1, np.dtype(dtype).name)
            dev = P.upload(lib, shape, valid)
            for mask in (0b001, 0b011):
                removed = math.prod(shape[a] for a in P.removed_axes(mask, 3))
                for method in (P.SUM, P.MAX):
                    got = P.project(lib, dev, mask, method)
                    name, what = P.kernel_name(lib), f"{key} {shape} mask {mask:03b} method {method}"
                    assert name == P.expected_chain(shape, dtype, mask, method) and name.count("+") == (0 if removed <= P.SEGMENT else 1), what
                    assert name.startswith(f"project_march_kernel<{'double' if dtype == np.float64 else 'float'},{P.S.vec_width(dtype, n2)},"), what
                    if method == P.SUM:
                        P.check_sum(got, valid, mask, what=what)
                    else:
                        P.check_extreme(got, valid, mask, method, what=what)


@pytest.mark.parametrize("key", sorted(P.TURN))
def test_project_beyond_the_turn(lib, key):
    """More threads than the workgroups of a launch have: every thread takes a second row or piece, none twice."""
    shape, dtype, mask = P.TURN[key]
    vec = P.S.vec_width(dtype, shape[-1])
    threads = shape[0] * shape[1] * 64 if key.startswith("row") else shape[1] * shape[2] // vec
    assert threads > P.TURN_THREADS and key.endswith(f"x{vec}")
    valid = P.drawn(shape, 1, np.dtype(dtype).name)
    dev = P.upload(lib, shape, valid)
    for method in (P.SUM, P.MAX):
        got = P.project(lib, dev, mask, method)
        assert P.kernel_name(lib) == P.expected_chain(shape, dtype, mask, method) and "+" not in P.kernel_name(lib)
        if method == P.SUM:
            P.check_sum(got, valid, mask, what=key)
        else:
            P.check_extreme(got, valid, mask, method, what=key)


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
@pytest.mark.parametrize("case", [c for c in P.SMALL if c[1] == 3 or len(c[0]) < 3][:14] + [((5, 4, 7), 3)], ids=P.S.case_id)
def test_boxes(lib, case, dtype):
    shape, ncomp = case
    P.check_boxes(lib, P.small_inputs(case, np.dtype(dtype).name, False), shape)
    assert P.kernel_name(lib) == f"extract_box_kernel<{'double' if dtype == np.float64 else 'float'}>"


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_box_beyond_the_turn(lib, dtype):
    shape = P.BOX_TURN
    assert math.prod(shape) > P.TURN_THREADS
    valid = P.drawn(shape, 1, np.dtype(dtype).name)
    got = P.extract_box(lib, P.upload(lib, shape, valid), (0, 0, 0), shape)
    assert np.array_equal(P.bits(got), P.bits(valid))


def test_release_scratch_frees_the_partial_results(lib):
    """`pdehip_release_scratch` hands the per-stream arrays of the stages back; the next call allocates them again and gives the same bits."""
    case = ((17, 9, 64), 3)
    valid = P.small_inputs(case, "float64", False)
    dev = P.upload(lib, case[0], valid)
    before = [P.project(lib, dev, mask, P.SUM) for mask in (0b111, 0b011)]
    lib.release_scratch()
    after = [P.project(lib, dev, mask, P.SUM) for mask in (0b111, 0b011)]
    for mask, b, a in zip((0b111, 0b011), before, after):
        P.check_sum(a, valid, mask, what="after release")
        assert np.array_equal(P.bits(b), P.bits(a))


def test_entry_points_refuse_bad_arguments(lib):
    P.refuse_bad_arguments(lib)


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_project_two_streams(lib, dtype):
    """Two streams project two different fields at the same time: each gets the bits it gets alone (the partial results are kept per
    stream).  Both wait for an event behind a queue of copies on a third stream, so that both chains are enqueued before either starts."""
    shape, ncomp, mask = (65, 64, 65), 3, 0b111
    valids = [P.S.draw(shape, ncomp, dtype, seed=11), (2.0 * P.S.draw(shape, ncomp, dtype, seed=12)).astype(dtype)]
    devs = [P.upload(lib, shape, v) for v in valids]
    alone = [P.project(lib, d, mask, P.SUM) for d in devs]
    assert P.kernel_name(lib).count("+") == 2 and not np.array_equal(alone[0], alone[1])
    big = GridInfo((65, 129, 251), (1.0,) * 3, np.float64)
    src, copy = DeviceArray(big, (1,)), DeviceArray(big, (1,))
    lib.memset(src.ptr, 0, src.nbytes, None)
    one, table = (C.c_double * 1)(1.0), ptr_array([src])
    streams, event = [], C.c_void_p()
    for _ in range(3):
        s = C.c_void_p()
        lib.stream_create(C.byref(s))
        streams.append(s)
    lib.event_create(C.byref(event))
    try:
        outs = [DeviceBuffer(8 * ncomp) for _ in range(2)]
        for _ in range(2):
            for _ in range(150):
                lib.lincomb(big.ref, 1, copy.ptr, None, 1, one, table, streams[2])
            lib.event_record(event, streams[2])
            for q in range(2):
                lib.stream_wait_event(streams[q], event)
            for q in range(2):
                lib.project(devs[q].info.ref, ncomp, devs[q].ptr, mask, P.SUM, C.c_double(P.WEIGHT), outs[q].ptr, streams[q])
            for q in range(2):
                host = np.empty((ncomp,))
                lib.memcpy_d2h(host.ctypes.data, outs[q].ptr, host.nbytes, streams[q])
                np.testing.assert_array_equal(P.bits(host), P.bits(alone[q]), err_msg=f"stream {q}")
    finally:
        for s in streams:
            lib.stream_synchronize(s)
            lib.stream_destroy(s)
        lib.event_destroy(event)


# ---- the Python side, through the mirror classes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_resident_run_keeps_the_state_on_the_device(dtype):
    P.resident_run_checks(pde_hip.get_backend("hip"), dtype)


def test_device_projections_key():
    backend = pde_hip.get_backend("hip")
    assert backend.device_projections is False
    P.resident_key_checks(backend)


def test_projector_on_device_arrays():
    """Bare device arrays of three components: every method and a slice against the mirror methods per component."""
    backend = pde_hip.get_backend("hip")
    shape = (6, 5, 7)
    grid = pde_hip.CartesianGrid([(0.0, 1.5 * n) for n in shape], shape)
    valid = P.S.draw(shape, 3, np.float32, seed=9)
    dev = DeviceArray(backend.grid_info(grid, valid.dtype), (3,)).set_valid(valid)
    projector, slicer = backend.make_projector(grid), backend.make_slicer(grid)
    for method in P.METHOD_NAMES:
        got = projector(dev, ["x", "z"], method=method)
        for c in range(3):
            field = pde_hip.ScalarField(grid, valid[c])
            ref = field.project(["x", "z"], method=method)
            P.check_against_reference(pde_hip.ScalarField(ref.grid, got[c]), ref, valid[c], (0, 2), method, float(grid.discretization[0] * grid.discretization[2]))
    cut = slicer(dev, {"y": "mid"})
    assert cut.dtype == np.float32 and np.array_equal(cut, valid[:, :, 2])
