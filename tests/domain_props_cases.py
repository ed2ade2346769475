"""Inputs, drivers and checks for ``pdehip_domain_properties`` and ``field_domains(..., properties=True)``.

Shared by ``tests/test_domain_props_cpu.py`` (CPU: the sequential C version of the tests-only shim) and ``tests/test_hip_domain_props.py``
(GPU: the kernels of ``csrc/pdehip_props.hip``).  The drivers call through whatever library ``pde_hip._lib`` holds, so the same checks
serve both.  The reference is ``pde_hip.domains.host_domain_properties``, the numpy restatement of the definitions in
``include/pdehip.h``, which ``tests/test_domain_props_cpu.py`` holds against scipy and ``math.fsum``.  Every output of the entry point is
an integer: every comparison here is ``assert_array_equal``, and derived floating-point attributes are compared bit for bit between the
device and the host path, which share one derivation.  There is no tolerance in this file.

Shapes: rows of 70 and 130 cells are no multiple of the 64 lanes of a wave, so waves span rows and planes (both branches of the masked
reduction); ``TURN_SHAPE`` lies beyond the grid-stride turn of the kernels (at most 4096 workgroups of 256 threads, as in
``domain_sizes_kernel``).
"""

from __future__ import annotations

import ctypes as C
import itertools
import math

import domains_cases as D
import numpy as np
from scipy import ndimage

import pde_hip
from pde_hip.device import DeviceArray, DeviceBuffer
from pde_hip.domains import PROPERTY_NAMES, finite_absmax, host_domain_properties

DTYPES = D.DTYPES
RAW_KEYS = ("anchor", "moment", "box", "limb", "excluded")
TURN_CELLS = D.TURN_CELLS          # the builder's workgroup cap is 4096, that of domain_sizes_kernel
TURN_SHAPE = D.TURN_SHAPE


def smooth_field(shape, dtype, seed: int = 7, sigma: float = 1.0) -> np.ndarray:
    """Smoothed noise with a fixed seed, scaled to a standard deviation of one: thresholded at 0 it gives a handful of ragged domains."""
    rng = np.random.default_rng([seed, *shape])
    data = ndimage.gaussian_filter(rng.standard_normal(shape), sigma, mode="wrap")
    return (data / data.std()).astype(dtype)


def all_periodic(ndim: int):
    return list(itertools.product((False, True), repeat=ndim))


# ---- the bare entry point ----------------------------------------------------------------------------------------------------------------
def call(lib, labels: np.ndarray, data, periodic, ndomains: int, absmax: float, *, dtype=np.float64, stream=None) -> dict:
    """The five outputs of one call on ``labels`` (the grid's shape) and ``data`` (None: no field).  Every output has one row more than
    ``ndomains``, all-ones bits before the call: the last row must keep them."""
    shape = labels.shape
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    dev = D.upload(lib, data) if data is not None else D.upload(lib, np.zeros(shape, dtype=dtype))
    lab_dev = DeviceBuffer(labels.nbytes)
    lib.memcpy_h2d(lab_dev.ptr, labels.ctypes.data, labels.nbytes, stream)
    k = ndomains
    host = {"anchor": np.empty(k + 1, np.int32), "moment": np.empty((k + 1, 3), np.int64), "box": np.empty((k + 1, 3, 2), np.int32),
            "limb": np.empty((k + 1, 2), np.int64), "excluded": np.empty(k + 1, np.uint32)}
    bufs = {key: DeviceBuffer(arr.nbytes) for key, arr in host.items()}
    for buf in bufs.values():
        lib.memset(buf.ptr, 0xFF, buf.nbytes, stream)
    per = (C.c_int * len(shape))(*[int(p) for p in periodic])
    field = data is not None
    lib.domain_properties(dev.info.ref, dev.ptr if field else None, lab_dev.ptr, k, per, C.c_double(absmax), bufs["anchor"].ptr, bufs["moment"].ptr,
                          bufs["box"].ptr, bufs["limb"].ptr if field else None, bufs["excluded"].ptr if field else None, stream)
    out = {}
    for key, arr in host.items():
        lib.memcpy_d2h(arr.ctypes.data, bufs[key].ptr, arr.nbytes, stream)
        assert (arr[k:].view(np.uint8) == 0xFF).all(), f"{key}: written behind its {k} rows"
        out[key] = arr[:k] if field or key not in ("limb", "excluded") else None
        if not field and key in ("limb", "excluded"):
            assert (arr.view(np.uint8) == 0xFF).all(), f"{key}: touched without a field"
    return out


def assert_raw_equal(got: dict, expect: dict, what: str = "") -> None:
    for key in RAW_KEYS:
        if expect[key] is None:
            assert got[key] is None, f"{what}: {key}"
            continue
        assert got[key].dtype == expect[key].dtype and got[key].shape == expect[key].shape, (what, key, got[key].dtype, got[key].shape)
        np.testing.assert_array_equal(got[key], expect[key], err_msg=f"{what}: {key}")


def check_call(lib, labels, data, periodic, what: str = "", absmax: float | None = None, ndomains: int | None = None) -> dict:
    """The entry point's integers equal the restatement's."""
    k = int(labels.max(initial=0)) if ndomains is None else ndomains
    absmax = (finite_absmax(data) if data is not None else 0.0) if absmax is None else absmax
    got = call(lib, labels, data, periodic, k, absmax)
    expect = host_domain_properties(labels, data, periodic, absmax, k)
    print(f"{what}: K {k}, absmax {absmax!r}")
    assert_raw_equal(got, expect, what)
    return got


def pattern_labels(shape) -> dict:
    """Every cell its own label (the checkerboard's foreground under face connectivity), two labels alternating lane by lane, one label
    over everything, and nothing."""
    cells = math.prod(shape)
    board = (np.indices(shape).sum(axis=0) % 2 == 0)
    own = np.zeros(shape, dtype=np.int32)
    own[board] = np.arange(1, int(board.sum()) + 1)
    return {"own": own, "abab": (1 + np.arange(cells) % 2).astype(np.int32).reshape(shape), "one": np.ones(shape, dtype=np.int32),
            "none": np.zeros(shape, dtype=np.int32)}


def run_patterns(lib, shape=(4, 6, 130)) -> None:
    data = smooth_field(shape, np.float64)
    for name, labels in pattern_labels(shape).items():
        for per in ((False, False, False), (True, True, True), (False, True, False)):
            check_call(lib, labels, data, per, f"{name} {per}")
        check_call(lib, labels, None, (True, False, True), f"{name} without a field")
    assert pattern_labels(shape)["own"].max() == math.prod(shape) // 2


def turn_labels() -> np.ndarray:
    """Hand-made labels beyond the turn: label 1 over everything else (it spans all turns), label 2 in the same threads' cells of the
    first and the second turn (a held label is carried across the turn), label 3 in the first turn where the second has label 4 (handed
    in at the turn's first wave), and background in between."""
    n = math.prod(TURN_SHAPE)
    assert TURN_CELLS < n < 2 * TURN_CELLS
    flat = np.ones(n, dtype=np.int32)
    run = 3 * 256 + 40          # three workgroups and a ragged end
    flat[0:run] = 2
    flat[TURN_CELLS:TURN_CELLS + run] = 2
    flat[run:2 * run] = 3
    flat[TURN_CELLS + run:TURN_CELLS + 2 * run] = 4
    flat[2 * run:2 * run + 500] = 0
    flat[n - 1000:n - 900] = 0
    flat[TURN_CELLS - 64:TURN_CELLS - 32] = 5
    return flat.reshape(TURN_SHAPE)


def run_turn(lib) -> None:
    labels = turn_labels()
    rng = np.random.default_rng(3)
    data = rng.standard_normal(TURN_SHAPE)
    check_call(lib, labels, data, (True, False, True), "beyond the turn")


# ---- sums ------------------------------------------------------------------------------------------------------------------------------------
def sum_fields(shape, dtype) -> dict:
    """name -> (data, kwargs of field_domains).  Values over 30 decades; all negative; a +inf foreground cell; all zeros; and (fp64)
    magnitudes near 1e-300 and 1e300."""
    rng = np.random.default_rng([9, *shape])
    sign = np.where(smooth_field(shape, np.float64) > 0, 1.0, -1.0)
    decades = sign * 10.0 ** rng.uniform(-15.0, 15.0, shape)
    inf = decades.copy()
    inf.reshape(-1)[np.flatnonzero(inf.reshape(-1) > 0)[5]] = np.inf
    out = {"decades": (decades.astype(dtype), {}), "negative": ((-np.abs(decades) - 1e-20).astype(dtype), {"above": False}),
           "inf": (inf.astype(dtype), {}), "zero": (np.zeros(shape, dtype=dtype), {"interval": (0.0, 0.0)})}
    if np.dtype(dtype) == np.float64:
        out["tiny"] = (sign * rng.uniform(0.1, 1.0, shape) * 1e-300, {})
        out["huge"] = (sign * rng.uniform(0.1, 1.0, shape) * 1e300, {})
    return out


# ---- field_domains on a device array against the restatement and the host path -------------------------------------------------------------
def device_array(backend, grid, data: np.ndarray) -> DeviceArray:
    return DeviceArray(backend.grid_info(grid, data.dtype), ()).set_valid(data)


def check_field(backend, data: np.ndarray, periodic, what: str = "", **kwargs):
    """``field_domains(device array, properties=True)``: the integers equal the restatement's on the labels it gave, and every attribute
    equals the host path's bit for bit."""
    shape = data.shape
    grid = pde_hip.CartesianGrid([(-1.0, -1.0 + 0.5 * n) for n in shape], shape, periodic=list(periodic))
    label = backend.make_domain_labeller(grid)
    got = label(device_array(backend, grid, data), properties=True, **kwargs)
    host = label(np.array(data), properties=True, **kwargs)
    assert got.on_device and not host.on_device
    print(f"{what}: K {got.count}")
    np.testing.assert_array_equal(got.labels, host.labels, err_msg=what)
    absmax = finite_absmax(data)
    expect = host_domain_properties(got.labels, data, periodic, absmax, got.count)
    ndim = len(shape)
    for key, name in zip(RAW_KEYS, ("anchors", "moments", "boxes", "limbs", "excluded")):
        e = expect[key][:, 3 - ndim:] if key in ("moment", "box") else expect[key]
        assert getattr(got, name).dtype == e.dtype
        np.testing.assert_array_equal(getattr(got, name), e, err_msg=f"{what}: {name}")
    same_properties(got, host, what)
    return got


def same_properties(a, b, what: str = "") -> None:
    for name in PROPERTY_NAMES:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.dtype, y.dtype, x.shape, y.shape)
        if x.dtype.kind == "f":          # bit for bit (NaN included)
            np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64), err_msg=f"{what}: {name}")
        else:
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: {name}")


def run_refusals(lib) -> None:
    import pytest

    shape = (4, 6)
    labels = np.zeros(shape, dtype=np.int32)
    labels[1:3, 2:5] = 1
    labels[3, 0] = 2
    data = smooth_field(shape, np.float64)
    check_call(lib, labels, data, (False, True), "fine")
    dev = D.upload(lib, data)
    lab = DeviceBuffer(labels.nbytes + 16)
    lib.memcpy_h2d(lab.ptr, labels.ctypes.data, labels.nbytes, None)
    a, m, b, l, e = (DeviceBuffer(n) for n in (32, 96, 96, 64, 32))
    per = (C.c_int * 2)(0, 1)
    d = C.c_double
    ref = dev.info.ref
    good = (ref, dev.ptr, lab.ptr, 2, per, d(1.0), a.ptr, m.ptr, b.ptr, l.ptr, e.ptr)
    lib.domain_properties(*good, None)
    for at, value in ((1, dev.ptr + 8), (2, None), (2, lab.ptr + 2), (3, -1), (3, 2 ** 31), (4, None), (5, d(-1.0)), (5, d(np.nan)), (5, d(np.inf)),
                      (6, None), (6, a.ptr + 2), (7, None), (7, m.ptr + 4), (8, None), (8, b.ptr + 2), (9, None), (9, l.ptr + 4), (10, None), (10, e.ptr + 2)):
        args = list(good)
        args[at] = value
        with pytest.raises(ValueError):
            lib.domain_properties(*args, None)
    # without a field the limbs and the counts may be NULL; without a domain everything may
    lib.domain_properties(ref, None, lab.ptr, 2, per, d(0.0), a.ptr, m.ptr, b.ptr, None, None, None)
    zeros = DeviceBuffer(labels.nbytes)
    lib.memset(zeros.ptr, 0, labels.nbytes, None)
    lib.domain_properties(ref, dev.ptr, zeros.ptr, 0, per, d(1.0), None, None, None, None, None, None)


def run_labels_out_of_range(lib) -> None:
    """Labels above ``ndomains`` and below 0 are refused by count and never used as an index: the rows behind keep their bits."""
    import pytest

    labels = np.array([[0, 1, 2, 2, 7, 3], [1, -5, 2 ** 31 - 1, 0, 3, 3]], dtype=np.int32)
    with pytest.raises(ValueError, match="3 cells|outside"):
        call(lib, labels, np.ones(labels.shape), (False, False), 3, 1.0)
    lab = DeviceBuffer(labels.nbytes)
    lib.memcpy_h2d(lab.ptr, labels.ctypes.data, labels.nbytes, None)
    dev = D.upload(lib, np.ones(labels.shape))
    host = np.empty(8, dtype=np.int32)
    a, m, b, l, e = (DeviceBuffer(n) for n in (32, 8 * 24, 8 * 24, 8 * 16, 32))
    for buf in (a, m, b, l, e):
        lib.memset(buf.ptr, 0xFF, buf.nbytes, None)
    with pytest.raises(ValueError):
        lib.domain_properties(dev.info.ref, dev.ptr, lab.ptr, 3, (C.c_int * 2)(0, 0), C.c_double(1.0), a.ptr, m.ptr, b.ptr, l.ptr, e.ptr, None)
    lib.memcpy_d2h(host.ctypes.data, a.ptr, 32, None)
    np.testing.assert_array_equal(host[:3], [1, 2, 5])
    assert (host[3:] == -1).all(), host
    for buf, rows in ((m, 24), (b, 24), (l, 16)):
        tail = np.empty(buf.nbytes - 3 * rows, dtype=np.uint8)
        lib.memcpy_d2h(tail.ctypes.data, buf.ptr + 3 * rows, tail.nbytes, None)
        assert (tail == 0xFF).all()
