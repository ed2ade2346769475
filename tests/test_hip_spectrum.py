"""Device tests of ``csrc/pdehip_fft.hip``: ``pdehip_fft_forward`` and ``pdehip_shell_spectrum`` through the C ABI against the serial C
versions of the tests-only shim - EQUAL BITS of every spectrum element, every count and every sum - and ``pde_hip.field_spectrum`` in a
resident run.

Inputs, drivers and the shim's results (computed once per case): ``tests/spectrum_cases.py``.  The shim itself is checked against numpy
in ``tests/test_spectrum_cpu.py``.  Shapes: the smallest at which the geometry can go wrong - the shortest lines, the longest row, tall
lines, ragged tiles - and one beyond the grid-stride turn of every launch.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import spectrum_cases as K

import pde_hip
from pde_hip.device import DeviceArray, DeviceBuffer, GridInfo, ptr_array

pytestmark = pytest.mark.gpu

IDS = ["f64", "f32"]


@pytest.fixture(scope="module")
def lib():
    return pde_hip.get_backend("hip")._lib


def check_forward(lib, shape, ncomp, dtype):
    name = np.dtype(dtype).name
    valid = K.inputs(shape, ncomp, name)
    dev = K.upload(lib, shape, valid)
    before = K.whole_allocation(lib, dev)
    got = K.fft_forward(lib, dev)
    expect = K.shim_forward(shape, ncomp, name)
    differ = np.count_nonzero(got.view(np.uint64) != expect.view(np.uint64))
    print(f"{K.shape_id(shape)} c{ncomp} {name}: {differ} of {2 * got.size} words differ; {lib.last_kernel_name().decode()}")
    assert got.shape == expect.shape and differ == 0
    np.testing.assert_array_equal(K.whole_allocation(lib, dev), before, err_msg="the input allocation was written")
    chain = lib.last_kernel_name().decode().split("+")
    assert chain[0] == f"fft_rows_kernel<{'double' if name == 'float64' else 'float'}>"
    assert chain[1:] == ["fft_lines_kernel"] * sum(n > 1 for n in shape[:-1])


@pytest.mark.parametrize("dtype", K.DTYPES, ids=IDS)
@pytest.mark.parametrize("ncomp", K.NCOMPS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.shape_id)
def test_fft_forward_equals_the_shim(lib, shape, ncomp, dtype):
    check_forward(lib, shape, ncomp, dtype)


def test_fft_forward_beyond_the_turn(lib):
    check_forward(lib, K.TURN, 3, np.float64)


def check_shells(lib, shape, ncomp, dtype, which):
    name = np.dtype(dtype).name
    valid = K.inputs(shape, ncomp, name)
    dev = K.upload(lib, shape, valid)
    before = K.whole_allocation(lib, dev)
    edges = K.edge_sets(shape)[which]
    counts, sums = K.shell_spectrum(lib, dev, K.frequencies(shape), edges)
    e_counts, e_sums = K.shim_shells(shape, ncomp, name, which)
    np.testing.assert_array_equal(counts, e_counts)
    np.testing.assert_array_equal(K.bits(sums), K.bits(e_sums))
    np.testing.assert_array_equal(K.whole_allocation(lib, dev), before, err_msg="the input allocation was written")
    assert lib.last_kernel_name().decode().endswith("+shell_max_kernel+shell_params_kernel+shell_limb_kernel")
    again = K.shell_spectrum(lib, K.upload(lib, shape, valid), K.frequencies(shape), edges)
    np.testing.assert_array_equal(again[0], counts)
    np.testing.assert_array_equal(K.bits(again[1]), K.bits(sums), err_msg="two calls differ")


@pytest.mark.parametrize("dtype", K.DTYPES, ids=IDS)
@pytest.mark.parametrize("ncomp", K.NCOMPS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.shape_id)
def test_shell_spectrum_equals_the_shim(lib, shape, ncomp, dtype):
    for which in ("default", "seven", "explicit"):
        check_shells(lib, shape, ncomp, dtype, which)


def test_shell_spectrum_beyond_the_turn(lib):
    check_shells(lib, K.TURN, 1, np.float64, "default")


def test_shell_spectrum_with_4096_bins(lib):
    """The largest LDS images of both shell sweeps (82 KB and 131 KB)."""
    shape = (8, 8, 256)
    valid = K.inputs(shape, 1, "float64")
    edges = np.linspace(0.0, float(K.full_k(shape).max()) * (1.0 + 1e-12), 4097)
    counts, sums = K.shell_spectrum(lib, K.upload(lib, shape, valid), K.frequencies(shape), edges)
    e_counts, e_sums = K.shim().shells(shape, valid, K.frequencies(shape), edges)
    np.testing.assert_array_equal(counts, e_counts)
    np.testing.assert_array_equal(K.bits(sums), K.bits(e_sums))


def test_release_scratch(lib):
    shape = (16, 4, 128)
    valid = K.inputs(shape, 3, "float64")
    dev = K.upload(lib, shape, valid)
    edges = K.edge_sets(shape)["default"]
    before, spec_before = K.shell_spectrum(lib, dev, K.frequencies(shape), edges), K.fft_forward(lib, dev)
    lib.release_scratch()
    after, spec_after = K.shell_spectrum(lib, dev, K.frequencies(shape), edges), K.fft_forward(lib, dev)
    np.testing.assert_array_equal(before[0], after[0])
    np.testing.assert_array_equal(K.bits(before[1]), K.bits(after[1]))
    np.testing.assert_array_equal(spec_before.view(np.uint64), spec_after.view(np.uint64))
    np.testing.assert_array_equal(K.bits(after[1]), K.bits(K.shim_shells(shape, 3, "float64", "default")[1]))


@pytest.mark.parametrize("dtype", K.DTYPES, ids=IDS)
def test_two_streams(lib, dtype):
    """Two streams work on two different fields of different shapes: each gets the result it gets alone (spectrum, tables and limbs are
    kept per stream).  Both wait for an event behind a queue of copies on a third stream, as in test_hip_hist.py::test_two_streams."""
    name = np.dtype(dtype).name
    shapes = [(8, 8, 256), (16, 4, 128)]
    valids = [K.inputs(s, 3, name) for s in shapes]
    devs = [K.upload(lib, s, v) for s, v in zip(shapes, valids)]
    edges = [K.edge_sets(s)["default"] for s in shapes]
    alone = [K.shell_spectrum(lib, d, K.frequencies(s), e) for d, s, e in zip(devs, shapes, edges)]
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
        for _ in range(100):
            lib.lincomb(big.ref, 1, copy.ptr, None, 1, one, table, streams[2])
        lib.event_record(event, streams[2])
        for q in range(2):
            lib.stream_wait_event(streams[q], event)
        # a call reads its edges and its limbs back: the second one is enqueued while the first one's scratch is still warm
        for q in (0, 1, 0, 1):
            got = K.shell_spectrum(lib, devs[q], K.frequencies(shapes[q]), edges[q], stream=streams[q])
            np.testing.assert_array_equal(got[0], alone[q][0], err_msg=f"counts, stream {q}")
            np.testing.assert_array_equal(K.bits(got[1]), K.bits(alone[q][1]), err_msg=f"sums, stream {q}")
    finally:
        for s in streams:
            lib.stream_synchronize(s)
            lib.stream_destroy(s)
        lib.event_destroy(event)


def test_refusals(lib):
    shape = (4, 8)
    dev = K.upload(lib, shape, K.inputs(shape, 1, "float64"))
    ref = dev.info.ref
    kf = np.concatenate(K.frequencies(shape))
    edges = np.linspace(0.0, 1.0, 5)
    kf_dev, e_dev, counts, sums, spec = DeviceBuffer(kf.nbytes), DeviceBuffer(8 * 4100), DeviceBuffer(8 * 4200), DeviceBuffer(8 * 4200), DeviceBuffer(4096)
    lib.memcpy_h2d(kf_dev.ptr, kf.ctypes.data, kf.nbytes, None)
    lib.memcpy_h2d(e_dev.ptr, edges.ctypes.data, edges.nbytes, None)
    lib.fft_supported(ref)
    lib.fft_forward(ref, 1, dev.ptr, spec.ptr, None)
    lib.shell_spectrum(ref, 1, dev.ptr, kf_dev.ptr, 4, e_dev.ptr, counts.ptr, sums.ptr, None)
    for args in ((ref, 1, None, spec.ptr), (ref, 1, dev.ptr, None), (ref, 0, dev.ptr, spec.ptr), (ref, 65, dev.ptr, spec.ptr),
                 (ref, 1, dev.ptr + 8, spec.ptr), (ref, 1, dev.ptr, spec.ptr + 8)):
        with pytest.raises(ValueError):
            lib.fft_forward(*args, None)
    good = [ref, 1, dev.ptr, kf_dev.ptr, 4, e_dev.ptr, counts.ptr, sums.ptr]
    for at, bad in ((2, None), (3, None), (5, None), (6, None), (7, None), (1, 0), (1, 65), (4, 0), (4, 4097), (2, dev.ptr + 8), (3, kf_dev.ptr + 4),
                    (5, e_dev.ptr + 4), (6, counts.ptr + 4), (7, sums.ptr + 4)):
        args = list(good)
        args[at] = bad
        with pytest.raises(ValueError):
            lib.shell_spectrum(*args, None)
    for bad in ([0.0, 0.25, 0.25, 0.5, 1.0], [0.0, 0.5, 0.25, 0.75, 1.0], [0.0, 0.25, np.nan, 0.5, 1.0], [-np.inf, 0.25, 0.5, 0.75, 1.0],
                [0.0, 0.25, 0.5, 0.75, np.inf]):
        e = np.array(bad)
        lib.memcpy_h2d(e_dev.ptr, e.ctypes.data, e.nbytes, None)
        with pytest.raises(ValueError):
            lib.shell_spectrum(*good, None)
    for shape in K.REFUSED:
        info = GridInfo(shape, (1.0,) * len(shape), np.float64)
        with pytest.raises(NotImplementedError, match="axis"):
            lib.fft_supported(info.ref)
        with pytest.raises(NotImplementedError):
            lib.fft_forward(info.ref, 1, dev.ptr, spec.ptr, None)
        with pytest.raises(NotImplementedError):
            lib.shell_spectrum(info.ref, 1, dev.ptr, kf_dev.ptr, 4, e_dev.ptr, counts.ptr, sums.ptr, None)


# ---- residency, through the mirror classes --------------------------------------------------------------------------------------------
def test_spectrum_in_a_callback_downloads_nothing():
    """A 32^3 diffusion run; the callback asks for the spectrum between the stepper calls: the state stays on the device and the answer
    is that of the host path on a side copy, within the transform bound."""
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.UnitGrid([32, 32, 32], periodic=True)
    state = pde_hip.ScalarField(grid, 1.0 + K.cosine_field((32, 32, 32), ((2, (0, 3, 0)), (1, (4, 0, 1)))))
    host = backend.make_spectrum(grid)
    eps = K.transform_eps((32, 32, 32))
    seen = []

    def callback(field, t):
        link = field.__dict__.get("_hip_link")
        if link is None or not link.host_stale:
            return
        got = pde_hip.field_spectrum(field)
        assert got.on_device and link.downloads == 0
        exact = link.dev_state.get_valid()          # a side copy for the reference: not a download of the field
        expect = host(exact)
        seen.append(t)
        np.testing.assert_array_equal(got.counts, expect.counts)
        assert np.abs(got.power - expect.power).sum() <= eps * (2.0 + eps) * expect.power.sum()
        assert got.k_peak == 3.0 / 32.0 and abs(got.total - np.mean(exact * exact)) <= 1e-12 * np.mean(exact * exact)

    res = pde_hip.DiffusionPDE(1.0).solve(state, t_range=2.0, dt=0.1, solver="euler", backend=backend, tracker=callback, interval=0.5)
    assert len(seen) >= 3 and res.__dict__["_hip_link"].downloads == 0
