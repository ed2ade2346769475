"""Device tests of ``csrc/pdehip_label.hip``: ``pdehip_label_domains`` and ``pdehip_domain_sizes`` through the C ABI, ``pde_hip.field_domains``
on device arrays, and the residency of a Cahn-Hilliard run that uses it through the mirror classes.

Reference, inputs and checks: ``tests/domains_cases.py`` (``scipy.ndimage.label``, a host union across the periodic wrap, renumbering by
first cell, ``np.bincount``).  A labelling is all integers: every check is for equality, on the whole label array, on K, on the
foreground count and on the sizes.  Shapes: around the tile of the tile kernel (4 x 8 x 32); the labelling kernels have no loop over turns,
``domain_sizes_kernel`` is grid-stride: one shape and hand-made labels lie beyond its turn.  ``tests/test_domains_cpu.py`` runs the same checks on
the tests-only host versions and asserts the conditions that keep the cases from being vacuous.
"""

from __future__ import annotations

import ctypes as C

import domains_cases as D
import numpy as np
import pytest

import pde_hip
from pde_hip.device import DeviceArray, GridInfo, ptr_array
from pde_hip.domains import interval_bounds

pytestmark = pytest.mark.gpu

IDS = ["f64", "f32"]


@pytest.fixture(scope="module")
def lib():
    return pde_hip.get_backend("hip")._lib


@pytest.mark.parametrize("dtype", D.DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", D.SHAPES, ids=D.shape_id)
def test_label_domains(lib, shape, dtype):
    """Random masks at p = 0.3 / 0.5 / 0.7 (all masks of the two smallest shapes), all foreground, all background, checkerboard,
    serpentine, diagonal neighbours, stripes joined by the wrap: both connectivities, periodic none / all / mixed."""
    D.run_shape(lib, shape, dtype)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(130,), (9, 65), (5, 9, 33)], ids=D.shape_id)
def test_special_values(lib, shape, dtype):
    """NaN and +-inf cells under ``interval=(a, inf)``; thresholds that equal cell values, ``>`` and ``<`` against the closed interval."""
    D.run_special_values(lib, shape, dtype)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["smoothed", "ragged"])
def test_beyond_the_turn_of_the_sizes(lib, name, dtype):
    """More cells than the workgroups of ``domain_sizes_kernel`` have threads: waves carry a label into their second turn (smoothed) or
    hand it in (ragged).  Labels and sizes against the reference."""
    D.run_turn_case(lib, name, dtype)


def test_domain_sizes_beyond_the_turn(lib):
    D.run_sizes_beyond_the_turn(lib)


def test_last_kernel_name(lib):
    for dtype, name in ((np.float64, "double"), (np.float32, "float")):
        for shape, conn, full in (((9, 65), 1, 0), ((9, 65), 2, 1), ((130,), 1, 0), ((5, 9, 33), 3, 1)):
            data = D.field_of(D.random_mask(shape, 0.5), dtype)
            D.label(lib, D.upload(lib, data), 0.0, np.inf, conn, (False,) * len(shape))
            assert lib.last_kernel_name().decode() == f"label_tile_kernel<{name},{full}>"


def test_the_same_call_twice_and_after_release_scratch(lib):
    shape, per = (17, 9, 64), (True, False, True)
    data = D.field_of(D.random_mask(shape, 0.3), np.float64)
    lo, hi = interval_bounds(np.float64, 0.0)
    expect = D.expected(shape, "p0.3", per, 3)
    first = D.check(lib, data, lo, hi, 3, per, expect, "first")
    again = D.check(lib, data, lo, hi, 3, per, expect, "again")
    lib.release_scratch()
    after = D.check(lib, data, lo, hi, 3, per, expect, "after release")
    # a smaller and then a larger grid on the same stream: the scratch grows
    small = D.field_of(D.random_mask((5, 9), 0.3), np.float64)
    D.check(lib, small, lo, hi, 1, (False, False), D.expected((5, 9), "p0.3", (False, False), 1), "small")
    larger = D.check(lib, data, lo, hi, 3, per, expect, "larger again")
    for other in (again, after, larger):
        for a, b in zip(first, other):
            np.testing.assert_array_equal(a, b)


def test_refusals(lib):
    D.run_refusals(lib)


def test_labels_above_ndomains(lib):
    D.run_labels_above_ndomains(lib)
    with pytest.raises(ValueError, match="3 cells"):
        host = np.array([0, 1, 9, -1, 5], dtype=np.int32)
        buf, out = pde_hip.device.DeviceBuffer(host.nbytes), pde_hip.device.DeviceBuffer(64)
        lib.memcpy_h2d(buf.ptr, host.ctypes.data, host.nbytes, None)
        lib.domain_sizes(buf.ptr, host.size, 2, out.ptr, None)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=IDS)
def test_two_streams(lib, dtype):
    """Two streams label two different fields at the same time: each gets the result it gets alone (parent array and chunk counts are
    kept per stream).  Both wait for an event behind a queue of copies on a third stream, so that both are enqueued before either starts."""
    shape, per = (17, 9, 64), (True, True, True)
    datas = [D.field_of(D.random_mask(shape, 0.3), dtype), D.field_of(D.random_mask(shape, 0.5), dtype)]
    devs = [D.upload(lib, d) for d in datas]
    lo, hi = interval_bounds(dtype, 0.0)
    expect = [D.expected(shape, "p0.3", per, 1), D.expected(shape, "p0.5", per, 1)]
    alone = [D.label(lib, dev, lo, hi, 1, per)[:2] for dev in devs]
    for (labels, info), e in zip(alone, expect):
        np.testing.assert_array_equal(labels, e[0])
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
        # pdehip_label_domains enqueues everything without waiting for its stream: both are in flight together
        for _ in range(100):
            lib.lincomb(big.ref, 1, copy.ptr, None, 1, one, table, streams[2])
        lib.event_record(event, streams[2])
        for q in range(2):
            lib.stream_wait_event(streams[q], event)
        kept = [[], []]
        for q in range(2):
            D.label(lib, devs[q], lo, hi, 1, per, stream=streams[q], keep=kept[q])
        for q in range(2):
            labels, info, labels_dev = D.read_label(lib, *kept[q][0], stream=streams[q])
            np.testing.assert_array_equal(labels, alone[q][0], err_msg=f"labels, stream {q}")
            np.testing.assert_array_equal(info, alone[q][1], err_msg=f"info, stream {q}")
            np.testing.assert_array_equal(D.sizes(lib, labels_dev, labels.size, int(info[0]), stream=streams[q]), expect[q][3])
    finally:
        for s in streams:
            lib.stream_synchronize(s)
            lib.stream_destroy(s)
        lib.event_destroy(event)


# ---- the Python side on device arrays ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D.DTYPES, ids=IDS)
def test_field_domains_on_a_device_array(dtype):
    backend = pde_hip.get_backend("hip")
    shape = (9, 7, 65)
    grid = pde_hip.CartesianGrid([(0.0, 0.5 * n) for n in shape], shape, periodic=[True, False, True])
    data = np.random.default_rng(8).uniform(-1.0, 1.0, shape).astype(dtype)
    dev = DeviceArray(backend.grid_info(grid, dtype), ()).set_valid(data)
    label = backend.make_domain_labeller(grid)
    third = float(dtype(1.0) / dtype(3.0))
    for kwargs, mask in (({}, data > 0.0), ({"threshold": third}, data > third), ({"threshold": 1.0 / 3.0, "above": False}, data < 1.0 / 3.0),
                         ({"interval": (-0.5, 0.1)}, (data >= -0.5) & (data <= 0.1)), ({"threshold": 0.4, "connectivity": 3}, data > 0.4)):
        got = label(dev, **kwargs)
        e_labels, e_k, e_fg, e_sizes = D.reference(mask, (True, False, True), kwargs.get("connectivity", 1))
        assert got.on_device and (got.count, got.foreground) == (e_k, e_fg) and got.largest == e_sizes.max()
        np.testing.assert_array_equal(got.sizes, e_sizes)
        np.testing.assert_array_equal(got.volumes, e_sizes * 0.125)
        np.testing.assert_array_equal(got.labels, e_labels)
    with pytest.raises(ValueError, match="ONE component"):
        pde_hip.field_domains(DeviceArray(dev.info, (3,)), backend=backend)


# ---- residency, through the mirror classes --------------------------------------------------------------------------------------------
def test_domains_in_a_callback_download_nothing():
    """A Cahn-Hilliard run of a few steps on (16, 16, 32); the tracker counts the domains between the stepper calls: the state stays on
    the device and the counts are the host path's on a side copy."""
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.UnitGrid([16, 16, 32], periodic=True)
    state = pde_hip.ScalarField.random_uniform(grid, -1.0, 1.0, rng=np.random.default_rng(2))
    seen = []

    def callback(field, t):
        link = field.__dict__.get("_hip_link")
        if link is None or not link.host_stale:
            return
        got = pde_hip.field_domains(field, 0.0)
        full = pde_hip.field_domains(field, 0.0, above=False, connectivity=3)
        assert got.on_device and full.on_device and link.downloads == 0
        side = pde_hip.ScalarField(grid, link.dev_state.get_valid())          # a side copy: not a download of the field
        for res, kwargs in ((got, {}), (full, {"above": False, "connectivity": 3})):
            host = pde_hip.field_domains(side, 0.0, **kwargs)
            assert not host.on_device and (res.count, res.foreground) == (host.count, host.foreground)
            np.testing.assert_array_equal(res.sizes, host.sizes)
            np.testing.assert_array_equal(res.labels, host.labels)
        seen.append((t, got.count, full.count))

    # (the mirror's tracker is the callable a DataTracker wraps; tests/test_domains_cpu.py drives py-pde's own DataTracker)
    res = pde_hip.CahnHilliardPDE().solve(state, t_range=1e-2, dt=1e-3, solver="euler", backend=backend, tracker=callback, interval=2e-3)
    print(seen)
    assert len(seen) >= 3 and res.__dict__["_hip_link"].downloads == 0
    assert all(k >= 1 for _, k, _ in seen)
