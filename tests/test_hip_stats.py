"""Device tests of ``csrc/pdehip_stats.hip``: ``pdehip_field_stats`` and ``pdehip_steady_state`` through the C ABI, and the residency of
a run that uses them through the mirror classes.

Reference, inputs and bounds: ``tests/stats_cases.py`` (a numpy restatement of the semantics in ``include/pdehip.h``; ``min``, ``max`` and
the counts exact, ``sum`` and ``m2`` inside bounds derived from the arithmetic, the steady-state maximum bit for bit).  Shapes: the
smallest at which the launch geometry can go wrong - vector widths, wave and workgroup seams, rows of 1-3 cells, 1 / 3 / 9 components,
and one shape per path beyond the grid-stride turn of a launch of 8192 workgroups.  ``tests/test_stats_cpu.py`` runs the same checks on
the tests-only host versions.
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest
import stats_cases as S

import pde_hip
from pde_hip.device import DeviceArray, DeviceBuffer, GridInfo, ptr_array

pytestmark = pytest.mark.gpu

IDS = ["f64", "f32"]


@pytest.fixture(scope="module")
def lib():
    return pde_hip.get_backend("hip")._lib


# ---- pdehip_field_stats ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
@pytest.mark.parametrize("case", S.SMALL, ids=S.case_id)
def test_field_stats(lib, case, dtype):
    """Per component and of the norm, with and without NaN / +-inf in first, last and seam cells, with and without the second sweep;
    two calls give equal bits."""
    shape, ncomp = case
    for planted in (False, True):
        valid, expect, expect_norm = S.small_inputs(case, np.dtype(dtype).name, planted)
        dev = S.upload(lib, shape, valid)
        got = S.field_stats(lib, dev)
        S.check_stats(got, expect, what=f"planted={planted}")
        again = S.field_stats(lib, S.upload(lib, shape, valid))
        np.testing.assert_array_equal(S.bits(got), S.bits(again), err_msg="two runs differ")
        S.check_stats(S.field_stats(lib, dev, norm=True), expect_norm, what=f"norm planted={planted}")
        S.check_stats(S.field_stats(lib, dev, want_m2=False), expect, want_m2=False, what=f"no m2 planted={planted}")


@pytest.mark.parametrize("key", sorted(S.TURN))
def test_field_stats_beyond_the_turn(lib, key):
    """More pieces than the 8192 workgroups of a launch have threads: every thread takes a second piece, none twice."""
    shape, dtype, vec = S.TURN[key]
    assert S.vec_width(dtype, shape[-1]) == vec and math.prod(shape) // vec > S.TURN_PIECES
    valid, expect = S.turn_inputs(key)
    S.check_stats(S.field_stats(lib, S.upload(lib, shape, valid)), expect, what=key)


def test_field_stats_all_nonfinite(lib):
    valid = np.full((2, 5, 7), np.nan)
    valid[1, 2, 3] = 0.75
    S.check_stats(S.field_stats(lib, S.upload(lib, (5, 7), valid)), S.expect_stats(valid), what="one finite cell in all")


def test_release_scratch_frees_the_slots(lib):
    """`pdehip_release_scratch` hands the per-stream slots back; the next call allocates them again and gives the same bits."""
    case = ((17, 9, 64), 3)
    valid, expect, _ = S.small_inputs(case, "float64", False)
    dev = S.upload(lib, case[0], valid)
    before = S.field_stats(lib, dev)
    lib.release_scratch()
    after = S.field_stats(lib, dev)
    S.check_stats(after, expect, what="after release")
    np.testing.assert_array_equal(S.bits(before), S.bits(after))


def test_field_stats_refuses_bad_arguments(lib):
    dev = S.upload(lib, (4, 4), S.draw((4, 4), 1, np.float64))
    out = DeviceBuffer(64)
    with pytest.raises(ValueError):
        lib.field_stats(dev.info.ref, 1, None, 0, 0, out.ptr, None)
    with pytest.raises(ValueError):
        lib.field_stats(dev.info.ref, 1, dev.ptr, 0, 0, None, None)
    for ncomp in (0, 65):
        with pytest.raises(ValueError):
            lib.field_stats(dev.info.ref, ncomp, dev.ptr, 0, 0, out.ptr, None)
    with pytest.raises(ValueError):
        lib.steady_state(dev.info.ref, 1, dev.ptr, dev.ptr, 1.0, 0.0, out.ptr, None)
    with pytest.raises(ValueError):
        lib.steady_state(dev.info.ref, 1, dev.ptr, None, 1.0, 0.0, out.ptr, None)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
def test_field_stats_two_streams(lib, dtype):
    """Two streams reduce two different fields at the same time: each gets the bits it gets alone (the slots are kept per stream).  Both
    wait for an event behind a queue of copies on a third stream, so that both reductions are enqueued before either starts."""
    shape, ncomp = (65, 64, 65), 3
    valids = [S.draw(shape, ncomp, dtype, seed=11), (2.0 * S.draw(shape, ncomp, dtype, seed=12)).astype(dtype)]
    devs = [S.upload(lib, shape, v) for v in valids]
    alone = [S.field_stats(lib, d) for d in devs]
    assert not np.array_equal(alone[0], alone[1])
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
        outs = [DeviceBuffer(64 * ncomp) for _ in range(2)]
        for _ in range(2):
            for _ in range(150):
                lib.lincomb(big.ref, 1, copy.ptr, None, 1, one, table, streams[2])
            lib.event_record(event, streams[2])
            for q in range(2):
                lib.stream_wait_event(streams[q], event)
            for q in range(2):
                lib.field_stats(devs[q].info.ref, ncomp, devs[q].ptr, 0, 1, outs[q].ptr, streams[q])
            for q in range(2):
                host = np.empty((ncomp, 8))
                lib.memcpy_d2h(host.ctypes.data, outs[q].ptr, host.nbytes, streams[q])
                np.testing.assert_array_equal(S.bits(host), S.bits(alone[q]), err_msg=f"stream {q}")
    finally:
        for s in streams:
            lib.stream_synchronize(s)
            lib.stream_destroy(s)
        lib.event_destroy(event)


# ---- pdehip_steady_state --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS)
@pytest.mark.parametrize("case", S.SMALL, ids=S.case_id)
def test_steady_state(lib, case, dtype):
    shape, ncomp = case
    clean = S.draw(shape, ncomp, dtype, seed=1)
    last = (clean + 1e-3 * S.draw(shape, ncomp, dtype, seed=2)).astype(dtype)
    # all cells finite; then NaN / +-inf planted in cur: excluded and counted out, but copied
    for cur in (clean, S.plant_nonfinite(clean)):
        dcur, dlast = S.upload(lib, shape, cur), S.upload(lib, shape, last)
        S.check_steady(S.steady_state(lib, dcur, dlast), S.np_steady(cur, last), "steady")
        np.testing.assert_array_equal(S.bits(dlast.get_valid()), S.bits(cur), err_msg="the snapshot is not a copy of the state")
        np.testing.assert_array_equal(S.bits(dcur.get_valid()), S.bits(cur), err_msg="the state changed")
    # a NaN in the snapshot under a finite cell of cur makes the maximum NaN
    last2 = last.copy()
    last2.reshape(ncomp, -1)[-1, -1] = np.nan
    S.check_steady(S.steady_state(lib, S.upload(lib, shape, clean), S.upload(lib, shape, last2)), (np.float64(np.nan), clean.size), "NaN snapshot")
    # no finite cell at all
    none = np.full_like(clean, np.inf)
    got = S.steady_state(lib, S.upload(lib, shape, none), S.upload(lib, shape, last))
    assert got[1] == 0 and np.isnan(got[0]), got


def test_steady_state_beyond_the_turn(lib):
    shape, dtype, _ = S.TURN["f64x1"]
    cur = S.turn_inputs("f64x1")[0]
    last = cur * (1.0 + 1e-4)
    last[0, -1, -1, -1] = cur[0, -1, -1, -1] + 0.5        # the deciding cell is the last one: beyond the turn
    dcur, dlast = S.upload(lib, shape, cur), S.upload(lib, shape, last)
    S.check_steady(S.steady_state(lib, dcur, dlast), S.np_steady(cur, last), "turn")
    np.testing.assert_array_equal(S.bits(dlast.get_valid()), S.bits(cur))


# ---- residency, through the mirror classes --------------------------------------------------------------------------------------------
ATOL, INTERVAL = 1e-2, 5.0


def _wave_state(dtype=np.float64):
    grid = pde_hip.UnitGrid([32, 32, 32], periodic=True)
    x = grid.cell_coords[..., 0]
    return pde_hip.ScalarField(grid, (1.0 + np.sin(2 * np.pi * x / 32)).astype(dtype))


def test_steady_state_check_keeps_the_state_on_the_device():
    """A 32^3 diffusion run, the check driven between the stepper calls: it reaches `value <= atol` at the same interrupt as the host
    formula on downloaded copies (with equal bits: a maximum does not depend on the order), and nothing is downloaded meanwhile."""
    backend = pde_hip.get_backend("hip")
    eq = pde_hip.DiffusionPDE(1.0)
    check = backend.make_steady_state_check(atol=ATOL, rtol=1e-5)
    device, host = [], []

    def on_device(field, t):
        link = field.__dict__.get("_hip_link")
        if link is None:                       # before the first stepper call: the state is not on the device yet
            return
        device.append(check.update(field, t))
        assert link.downloads == 0

    snapshot = {}

    def on_host(field, t):
        if field.__dict__.get("_hip_link") is None:
            return
        data = field.data                      # a download per interrupt
        if "last" in snapshot:
            finite = np.isfinite(data)
            rate = (snapshot["last"][finite] - data[finite]) / (t - snapshot["t"])
            host.append(float(np.max(np.abs(rate) - 1e-5 * np.abs(data[finite]))))
        else:
            host.append(None)
        snapshot["last"], snapshot["t"] = data.copy(), t

    res = eq.solve(_wave_state(), t_range=60.0, dt=0.1, solver="euler", backend=backend, tracker=on_device, interval=INTERVAL)
    assert res.__dict__["_hip_link"].downloads == 0 and check.on_device
    eq.solve(_wave_state(), t_range=60.0, dt=0.1, solver="euler", backend=backend, tracker=on_host, interval=INTERVAL)
    print(device, host)
    assert device[0] is None and host[0] is None and len(device) == len(host) > 4
    first = [next(i for i, v in enumerate(vals) if v is not None and v <= ATOL) for vals in (device, host)]
    assert first[0] == first[1] and 1 < first[0] < len(device) - 1
    assert device[1:] == host[1:]
    assert check.converged(device[first[0]]) and not check.converged(device[first[0] - 1])


@pytest.mark.parametrize("flag", [True, False], ids=["on", "off"])
def test_device_statistics_properties(flag):
    """`device_statistics` on: `state.average` / `state.fluctuations` inside a tracker callback leave the state on the device and agree
    with the host values within the bounds of the sums; off: they download, exactly as before."""
    backend = pde_hip.get_backend("hip")
    seen = []

    def callback(field, t):
        link = field.__dict__.get("_hip_link")
        if link is None or not link.host_stale:
            return
        exact = link.dev_state.get_valid()          # a side copy for the reference: not a download of the field
        seen.append((float(field.average), float(field.fluctuations), link.downloads, exact))

    backend.device_statistics = flag
    try:
        pde_hip.DiffusionPDE(1.0).solve(_wave_state(), t_range=2.0, dt=0.1, solver="euler", backend=backend, tracker=callback, interval=0.5)
    finally:
        backend.device_statistics = None
    assert len(seen) >= 3
    if not flag:
        assert [s[2] for s in seen] == list(range(1, len(seen) + 1))
        for avg, fluct, _, exact in seen:          # numpy's own sums (of a strided view there, of a compact copy here)
            assert abs(avg - exact.mean()) < 1e-13 and abs(fluct - exact.std()) < 1e-13
        return
    assert [s[2] for s in seen] == [0] * len(seen)
    for avg, fluct, _, exact in seen:
        x = exact.ravel().astype(np.float64)
        n = x.size
        total, sumabs, m2 = math.fsum(x), math.fsum(np.abs(x)), S.exact_m2(x)
        bound = n * S.U * sumabs / n + 4 * S.U * abs(total) / n           # the sum's bound, the cell volume (1) and the division
        print(f"average {avg!r} exact {total / n!r} bound {bound:.3e}; fluctuations {fluct!r} exact {math.sqrt(m2 / n)!r}")
        assert abs(avg - total / n) <= bound
        delta = n * S.U * np.abs(x).max()
        b2 = (n + 4) * S.U * m2 + n * delta * delta
        lo, hi = math.sqrt(max(m2 - b2, 0.0) / n), math.sqrt((m2 + b2) / n)
        assert lo * (1 - 4 * S.U) <= fluct <= hi * (1 + 4 * S.U)
