"""The field stores of the four-step sweep (pdehip_march4.inc) write the valid cells and nothing else.

A workgroup computes a halo of four cells around its tile and eight planes in front of its x-chunk; of all that only the patches that own
output cells, and only from the fifth output phase on, may store to the field (tests/test_hip_euler4.py compares the valid cells; a store
that strays into a ghost cell, the padding of a row or another allocation would not show there).  Here both arrays of a run live in buffers
of the test's own, filled with a sentinel down to the last byte and 4 KiB longer than the arrays; after 8 steps (two sweeps, each array
written once) the valid cells equal the oracle bit for bit, and every ghost cell, the padding of the rows, the slack behind the array and
the 4 KiB behind that still hold the sentinel.  Twice from the same state, with the same bits.  Path forced by PDEHIP_EULER4=1; shapes: the smallest grid, two tiles per axis with an odd number
of planes, two x-chunks of unequal length, and the general-spacing instance.
"""

from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
from helpers import expect_steps

import pde_hip
from pde_hip import _abi
from pde_hip.device import DeviceArray, DeviceBuffer

pytestmark = pytest.mark.gpu

TY, TZ, NMIN = 32, 64, 16
DT, STEPS = 0.05, 8
SENTINEL = np.float64(-1.2345678901234567e+123)
BEHIND = 4096   # bytes of sentinel behind each array


def _setup(kind, shape):
    if kind == "unit":
        return pde_hip.UnitGrid(shape, periodic=True), 1.0
    bounds = [[0, n * s] for n, s in zip(shape, (0.8, 1.25, 1.1))]
    return pde_hip.CartesianGrid(bounds, shape, periodic=True), 0.7


def _data(shape):
    return np.random.default_rng(11).uniform(-0.5, 0.5, shape)


@functools.lru_cache(maxsize=None)
def _expect(kind, shape):
    grid, D = _setup(kind, shape)
    out = expect_steps(_abi.RHS_DIFFUSION, D, grid, "periodic", _data(shape), DT, STEPS)
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def backend():
    return pde_hip.get_backend("hip")


class _Guarded:
    """A DeviceArray inside a buffer of the test's own, BEHIND bytes longer, all of it sentinel"""

    def __init__(self, lib, info):
        lay = (C.c_int64 * 8)()
        lib.layout(info.ref, lay)
        self.p0, self.p1, self.pc, self.off = (int(lay[k]) for k in range(4))
        self.lib, self.info = lib, info
        self.elems = self.pc + info.slack + BEHIND // 8
        assert info.comp_elems == self.pc and info.dtype == np.float64
        self.buffer = DeviceBuffer(self.elems * 8)
        self.array = DeviceArray(info, buffer=self.buffer, ptr=self.buffer.ptr)
        n0, n1, n2 = info.shape
        cells = self.off + np.arange(n0)[:, None, None] * self.p0 + np.arange(n1)[None, :, None] * self.p1 + np.arange(n2)[None, None, :]
        self.valid = np.zeros(self.elems, bool)
        self.valid[cells.ravel()] = True    # (increasing addresses = C order of the valid cells)
        assert self.valid.sum() == n0 * n1 * n2 and cells.max() < self.pc

    def fill(self):
        host = np.full(self.elems, SENTINEL)
        self.lib.memcpy_h2d(self.buffer.ptr, host.ctypes.data, host.nbytes, None)

    def raw(self):
        host = np.empty(self.elems)
        self.lib.memcpy_d2h(host.ctypes.data, self.buffer.ptr, host.nbytes, None)
        return host


def _run_once(backend, kind, shape):
    """(valid cells of the result, [raw images of both buffers], valid mask, kernel name) of STEPS steps from _data(shape)"""
    grid, D = _setup(kind, shape)
    data = _data(shape)
    spec = backend.make_rhs_spec(pde_hip.DiffusionPDE(D, bc="periodic"), pde_hip.ScalarField(grid, data))
    lib = backend._lib
    a, b = _Guarded(lib, spec.info), _Guarded(lib, spec.info)
    a.fill()
    b.fill()
    a.array.set_valid(data)
    before = a.raw()
    assert np.array_equal(before[a.valid], data.ravel()) and np.all(before[~a.valid] == SENTINEL)   # the upload wrote the valid cells alone
    res = C.c_void_p()
    lib.euler_run(spec.info.ref, spec.ref, a.array.ptr, b.array.ptr, DT, STEPS, C.byref(res), None)
    name = lib.last_kernel_name().decode()
    assert res.value == a.array.ptr            # two sweeps: a -> b -> a
    return a.array.get_valid(), [a.raw(), b.raw()], a.valid, name


@pytest.mark.parametrize("kind,shape", [("unit", (NMIN, TY, TZ)), ("unit", (NMIN + 3, 2 * TY, 2 * TZ)), ("unit", (33, TY, TZ)), ("cart", (NMIN + 3, 2 * TY, 2 * TZ))], ids=str)
def test_stores_hit_the_valid_cells_alone(backend, monkeypatch, kind, shape):
    monkeypatch.setenv("PDEHIP_EULER4", "1")
    want = _expect(kind, shape)
    first = None
    for _ in range(2):
        got, raws, valid, name = _run_once(backend, kind, shape)
        assert "euler4_kernel" in name and ("E2_DIFFUSION_UNIT" in name) == (kind == "unit"), name
        np.testing.assert_array_equal(got, want)
        assert np.abs(got - _data(shape)).max() > 1e-3
        for raw in raws:   # each array was the output of one sweep
            outside = raw[~valid]
            wrong = np.flatnonzero(outside != SENTINEL)
            assert wrong.size == 0, (wrong.size, np.flatnonzero(~valid)[wrong[:8]])
            assert not np.any(raw[valid] == SENTINEL)
        np.testing.assert_array_equal(raws[0][valid], want.ravel())
        if first is None:
            first = raws
        else:
            for x, y in zip(first, raws):
                assert x.tobytes() == y.tobytes()
