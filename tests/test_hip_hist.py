"""Device tests of ``csrc/pdehip_hist.hip``: ``pdehip_histogram`` and ``pdehip_quantile_select`` through the C ABI, ``pde_hip.field_histogram``
/ ``field_quantile`` / ``field_median`` on device arrays, and the residency of a run that uses them through the mirror classes.

Reference, inputs and checks: ``tests/hist_cases.py`` (numpy restatements of the semantics in ``include/pdehip.h``, and numpy's own
``np.histogram`` / ``np.sort`` / ``np.quantile``).  Counts are integers and order statistics are elements of the field: every check is for
equality.  Shapes: the smallest at which the launch geometry can go wrong - rows of 1-3 cells, vector widths, wave and workgroup seams,
1 / 3 / 9 components and the norm, and one shape per path beyond the grid-stride turn of a launch.  ``tests/test_hist_cpu.py`` runs the same
checks on the tests-only host versions.
"""

from __future__ import annotations

import ctypes as C
import math

import hist_cases as H
import numpy as np
import pytest

import pde_hip
from pde_hip.device import DeviceArray, GridInfo, ptr_array

pytestmark = pytest.mark.gpu

IDS = ["f64", "f32"]


@pytest.fixture(scope="module")
def lib():
    return pde_hip.get_backend("hip")._lib


# ---- pdehip_histogram ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", H.DTYPES, ids=IDS)
@pytest.mark.parametrize("case", H.SMALL, ids=H.case_id)
def test_histogram(lib, case, dtype):
    H.run_histogram_case(lib, case, dtype)


@pytest.mark.parametrize("key", sorted(H.TURN))
def test_histogram_beyond_the_turn(lib, key):
    """More pieces than the workgroups of a launch have threads, for both caps (64 and 4096 bins) and for general edges."""
    shape, dtype, vec = H.TURN[key]
    assert H.vec_width(dtype, shape[-1]) == vec and math.prod(shape) // vec > H.TURN_PIECES
    valid = H.turn_inputs(key)
    dev = H.upload(lib, shape, valid)
    for nbins in (64, 4096):
        edges = H.equal_edges(nbins, dtype)
        H.check_counts(H.histogram(lib, dev, edges), valid, edges, f"{key} bins={nbins}", lambda x, nbins=nbins: np.histogram(x, nbins, H.RANGE)[0])
        assert lib.last_kernel_name().decode().startswith("hist_sweep_kernel<") and lib.last_kernel_name().decode().endswith(f"{vec},0,1>")
    edges = H.nonuniform_edges(dtype)
    H.check_counts(H.histogram(lib, dev, edges), valid, edges, f"{key} non-uniform", lambda x: np.histogram(x, edges)[0])
    assert lib.last_kernel_name().decode().endswith(f"{vec},0,0>")


@pytest.mark.parametrize("dtype", H.DTYPES, ids=IDS)
def test_histogram_all_cells_in_one_bin(lib, dtype):
    """Worst contention: every lane of every wave adds to the same counter."""
    shape = (17, 9, 64)
    valid = np.full((1, *shape), 0.3, dtype=dtype)
    dev = H.upload(lib, shape, valid)
    for nbins in (7, 4096):
        edges = H.equal_edges(nbins, dtype)
        got = H.histogram(lib, dev, edges)
        H.check_counts(got, valid, edges, f"one bin of {nbins}", lambda x, nbins=nbins: np.histogram(x, nbins, H.RANGE)[0])
        assert got.max() == valid.size


def test_histogram_release_scratch(lib):
    case = ((17, 9, 64), 3)
    valid, edges = H.small_inputs(case, "float64", 64)
    dev = H.upload(lib, case[0], valid)
    before, sel_before = H.histogram(lib, dev, edges), H.select(lib, dev, H.QS)
    lib.release_scratch()
    after, sel_after = H.histogram(lib, dev, edges), H.select(lib, dev, H.QS)
    H.check_counts(after, valid, edges, "after release")
    np.testing.assert_array_equal(before, after)
    H.check_select(sel_after, valid, H.QS, "after release")
    for a, b in zip(sel_before, sel_after):
        np.testing.assert_array_equal(H.bits(a), H.bits(b))


def test_refusals(lib):
    H.run_refusals(lib)


@pytest.mark.parametrize("dtype", H.DTYPES, ids=IDS)
def test_two_streams(lib, dtype):
    """Two streams work on two different fields at the same time: each gets the result it gets alone (edges and control blocks are kept
    per stream).  Both wait for an event behind a queue of copies on a third stream, so that both are enqueued before either starts."""
    shape, ncomp = (33, 32, 65), 3
    edges = H.equal_edges(64, dtype)
    valids = [H.plant(H.draw(shape, ncomp, dtype, seed=11), edges), H.plant((0.5 * H.draw(shape, ncomp, dtype, seed=12)).astype(dtype), edges)]
    devs = [H.upload(lib, shape, v) for v in valids]
    alone = [(H.histogram(lib, d, edges), H.select(lib, d, H.QS)) for d in devs]
    assert not np.array_equal(alone[0][0], alone[1][0])
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
        # the selection enqueues everything without waiting for its stream: both are in flight together
        for _ in range(100):
            lib.lincomb(big.ref, 1, copy.ptr, None, 1, one, table, streams[2])
        lib.event_record(event, streams[2])
        for q in range(2):
            lib.stream_wait_event(streams[q], event)
        kept = [[], []]
        for q in range(2):
            H.select(lib, devs[q], H.QS, stream=streams[q], keep=kept[q])
        for q in range(2):
            got = H.read_select(lib, *kept[q][0], stream=streams[q])
            for a, b in zip(got, alone[q][1]):
                np.testing.assert_array_equal(H.bits(a), H.bits(b), err_msg=f"selection, stream {q}")
        # the histogram reads its edges back before it launches: the second call is enqueued while the first one's sweep may still run
        for q in range(2):
            H.histogram(lib, devs[q], edges, stream=streams[q], keep=kept[q])
        for q in range(2):
            _, out, shape_out = kept[q][1]
            host = np.empty(shape_out, dtype=np.uint64)
            lib.memcpy_d2h(host.ctypes.data, out.ptr, host.nbytes, streams[q])
            np.testing.assert_array_equal(host, alone[q][0], err_msg=f"histogram, stream {q}")
    finally:
        for s in streams:
            lib.stream_synchronize(s)
            lib.stream_destroy(s)
        lib.event_destroy(event)


# ---- pdehip_quantile_select -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", H.DTYPES, ids=IDS)
@pytest.mark.parametrize("case", H.SMALL, ids=H.case_id)
def test_quantile_select(lib, case, dtype):
    H.run_select_case(lib, case, dtype)


@pytest.mark.parametrize("dtype", H.DTYPES, ids=IDS)
def test_quantile_select_fields(lib, dtype):
    """Ties, signs, subnormals next to +-inf, one number, none."""
    for name, valid in H.select_fields(dtype).items():
        dev = H.upload(lib, valid.shape[1:], valid)
        for q in (*H.QS, H.QS):
            H.check_select(H.select(lib, dev, q), valid, q, f"{name} q={q}")


@pytest.mark.parametrize("key", sorted(H.TURN))
def test_quantile_select_beyond_the_turn(lib, key):
    shape, dtype, vec = H.TURN[key]
    valid = H.turn_inputs(key)
    H.check_select(H.select(lib, H.upload(lib, shape, valid), H.QS), valid, H.QS, key)
    assert lib.last_kernel_name().decode() == f"select_sweep_kernel<{'double' if dtype == np.float64 else 'float'},{vec},0>"


# ---- the Python side on device arrays ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", H.DTYPES, ids=IDS)
def test_field_histogram_matches_numpy(dtype):
    """`range=None` on finite data equals `np.histogram(a, bins)` (edges from the device's own minimum and maximum), `density` equals
    numpy's, a vector field shares one set of edges, the norm is one histogram."""
    backend = pde_hip.get_backend("hip")
    shape = (9, 7, 65)
    data = H.draw(shape, 3, dtype, seed=5)
    dev = DeviceArray(backend.grid_info(pde_hip.UnitGrid(shape), dtype), (3,)).set_valid(data)
    for bins in (1, 10, 64):
        got = pde_hip.field_histogram(dev, bins, backend=backend)
        counts, edges = np.histogram(data, bins)
        assert got.on_device and got.edges.dtype == edges.dtype and got.counts.shape == (3, bins)
        np.testing.assert_array_equal(got.edges, edges)
        np.testing.assert_array_equal(got.counts.sum(axis=0), counts)
        for c in range(3):
            np.testing.assert_array_equal(got.counts[c], np.histogram(data[c], edges)[0])
            np.testing.assert_array_equal(got.density[c], np.histogram(data[c], edges, density=True)[0])
        assert not got.below.any() and not got.above.any() and not got.nan.any()
    one = pde_hip.field_histogram(dev.component(1), 10, backend=backend)
    np.testing.assert_array_equal(one.counts, np.histogram(data[1], 10)[0])
    np.testing.assert_array_equal(one.edges, np.histogram(data[1], 10)[1])
    values, edges = pde_hip.field_histogram(dev.component(1), 10, density=True, backend=backend)
    np.testing.assert_array_equal(values, np.histogram(data[1], 10, density=True)[0])
    norm = H.np_values(data, True)[0]
    got = pde_hip.field_histogram(dev, 16, norm=True, backend=backend)
    np.testing.assert_array_equal(got.counts, np.histogram(norm, 16)[0])
    np.testing.assert_array_equal(got.edges, np.histogram(norm, 16)[1])
    # a constant field: numpy's half-unit margins; a threshold on an edge
    flat = DeviceArray(dev.info, ()).set_valid(np.full(shape, 2.0, dtype=dtype))
    got = pde_hip.field_histogram(flat, 4, backend=backend)
    np.testing.assert_array_equal(got.edges, np.histogram(np.full(shape, 2.0, dtype=dtype), 4)[1])
    np.testing.assert_array_equal(got.counts, np.histogram(np.full(shape, 2.0, dtype=dtype), 4)[0])
    got = pde_hip.field_histogram(dev, 8, (-0.5, 0.5), backend=backend)
    np.testing.assert_array_equal(got.fraction_above(got.edges[4]), (data >= got.edges[4]).mean(axis=(1, 2, 3)))
    bad = data.copy()
    bad[1, 2, 3, 4] = np.inf
    with pytest.raises(ValueError, match="autodetected range"):
        pde_hip.field_histogram(dev.set_valid(bad), 10, backend=backend)


@pytest.mark.parametrize("dtype", H.DTYPES, ids=IDS)
def test_field_quantile_matches_numpy(dtype):
    backend = pde_hip.get_backend("hip")
    for shape, qs in H.METHOD_CASES:
        data = H.draw(shape, 3, dtype, seed=9)
        dev = DeviceArray(backend.grid_info(pde_hip.UnitGrid(shape), dtype), (3,)).set_valid(data)
        axes = tuple(range(1, data.ndim))
        for method in ("lower", "higher"):
            got = pde_hip.field_quantile(dev, qs, method=method, backend=backend)
            expect = np.quantile(data, qs, axis=axes, method=method)
            assert got.shape == expect.shape == (len(qs), 3) and got.dtype == dtype
            np.testing.assert_array_equal(H.bits(got), H.bits(expect.astype(dtype)), err_msg=method)
        # "linear": the stated formula on np.sort, rounded once to the field's type
        got = pde_hip.field_quantile(dev, qs, backend=backend)
        ordered = np.sort(data.reshape(3, -1), axis=1).astype(np.float64)
        n = ordered.shape[1]
        v = (np.float64(n) - 1.0) * np.array(qs, dtype=np.float64)
        k = np.floor(v).astype(np.int64)
        lower, upper = ordered[:, k], ordered[:, np.minimum(k + 1, n - 1)]
        expect = (lower + (upper - lower) * (v - k)).astype(dtype).T
        np.testing.assert_array_equal(H.bits(got), H.bits(expect), err_msg="linear")
        if n % 2:
            median = pde_hip.field_median(dev, backend=backend)
            np.testing.assert_array_equal(H.bits(median), H.bits(np.median(data, axis=axes).astype(dtype)))
    # more than 8 values of q go in groups of 8; a NaN cell makes the result NaN unless it is ignored
    qs = np.linspace(0.0, 1.0, 19)
    got = pde_hip.field_quantile(dev.component(0), qs, method="lower", backend=backend)
    np.testing.assert_array_equal(H.bits(got), H.bits(np.quantile(data[0], qs, method="lower").astype(dtype)))
    holed = data.copy()
    holed[2, 0, 0, 0] = np.nan
    dev.set_valid(holed)
    got = pde_hip.field_quantile(dev, 0.5, method="lower", backend=backend)
    assert np.isnan(got[2]) and not np.isnan(got[:2]).any()
    got = pde_hip.field_quantile(dev, 0.5, method="lower", ignore_nan=True, backend=backend)
    np.testing.assert_array_equal(H.bits(got), H.bits(np.nanquantile(holed, 0.5, axis=axes, method="lower").astype(dtype)))


# ---- residency, through the mirror classes --------------------------------------------------------------------------------------------
def test_distribution_in_a_callback_downloads_nothing():
    """A 32^3 diffusion run; the callback asks for a histogram and two quantiles between the stepper calls: the state stays on the device
    and the answers are numpy's on a side copy."""
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.UnitGrid([32, 32, 32], periodic=True)
    x = grid.cell_coords[..., 0]
    state = pde_hip.ScalarField(grid, 1.0 + np.sin(2 * np.pi * x / 32))
    seen = []

    def callback(field, t):
        link = field.__dict__.get("_hip_link")
        if link is None or not link.host_stale:
            return
        hist = pde_hip.field_histogram(field, 16, (0.0, 2.0))
        auto = pde_hip.field_histogram(field, 16)
        quant = pde_hip.field_quantile(field, [0.25, 0.5], method="lower")
        assert hist.on_device and link.downloads == 0
        exact = link.dev_state.get_valid()          # a side copy for the reference: not a download of the field
        seen.append(t)
        np.testing.assert_array_equal(hist.counts, np.histogram(exact, 16, (0.0, 2.0))[0])
        np.testing.assert_array_equal(auto.counts, np.histogram(exact, 16)[0])
        np.testing.assert_array_equal(auto.edges, np.histogram(exact, 16)[1])
        np.testing.assert_array_equal(quant, np.quantile(exact, [0.25, 0.5], method="lower"))

    res = pde_hip.DiffusionPDE(1.0).solve(state, t_range=2.0, dt=0.1, solver="euler", backend=backend, tracker=callback, interval=0.5)
    assert len(seen) >= 3 and res.__dict__["_hip_link"].downloads == 0
