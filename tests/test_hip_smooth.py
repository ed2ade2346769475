"""Device tests of ``csrc/pdehip_smooth.hip``: ``pdehip_smooth_axis`` through the C ABI, and the residency of a run that smooths its state
through the mirror classes.

Reference, inputs and drivers: ``tests/smooth_cases.py`` (a numpy restatement of the arithmetic in ``include/pdehip.h``, itself checked
against the reference's results and scipy by ``tests/test_smooth_cpu.py``).  Every comparison is bit for bit - a cell that is not NaN has
the restatement's bits, a NaN cell is NaN - for the instance the host chooses AND for the one-cell-per-thread instance
(``PDEHIP_SMOOTH_CELL``); every pass writes into an array full of sentinels, whose ghost cells and padding must keep them, and leaves its
input as it was; a second call on a fresh upload gives the same bits.  Shapes: the smallest at which the tiling can go wrong - lines of
1 to 5 cells, the seams of a row piece (64 lanes) and of the march tile (64 cells long, 32 wide), vector widths 1 / 2 / 4, radii from 0
beyond twice the extent, each instance's radius cap and the cap plus 1, one shape per instance beyond the grid-stride turn.
"""

from __future__ import annotations

import numpy as np
import pytest
import smooth_cases as G

import pde_hip

pytestmark = pytest.mark.gpu

IDS = ["f64", "f32"]
MODE_IDS = ["wrap", "reflect"]


@pytest.fixture(scope="module")
def lib():
    return pde_hip.get_backend("hip")._lib


@pytest.mark.parametrize("cid", sorted(G.GOLDEN))
def test_golden_cases(lib, cid):
    """The reference's results, axis by axis and chained, with the weights stored beside them (no host exp)."""
    G.check_golden_passes(lib, cid)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", G.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("kind", G.TILING_KINDS)
def test_instances_against_the_yardstick_and_the_restatement(lib, kind, mode, dtype):
    for shape, axis, ncomp in G.tiling_cases(kind):
        valid = G.drawn(shape, ncomp, np.dtype(dtype).name)
        dev = G.upload(lib, shape, valid)
        for r in G.radii(shape[axis]):
            G.check_pass(lib, valid, shape, axis, G.radius_weights(r), mode, f"{shape} axis {axis} r {r}", dev=dev)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", sorted(G.CAPS))
def test_radius_caps(lib, kind, dtype):
    """The largest radius an LDS instance takes and the first one it leaves to the generic instance: the names on both sides of the
    switch, the same bits on both."""
    shape, axis, cap = G.CAPS[kind]
    valid = G.drawn(shape, 1, np.dtype(dtype).name)
    for mode in G.MODES:
        for r in (cap, cap + 1):
            G.check_pass(lib, valid, shape, axis, G.radius_weights(r), mode, f"{kind} r {r}")
            G.smooth_axis(lib, G.upload(lib, shape, valid), G.sentinel_array(lib, G.upload(lib, shape, valid)), axis, G.radius_weights(r), mode)
            assert G.kernel_name(lib).startswith("gauss_cell_kernel<") == (r > cap), f"{kind} r {r}: {G.kernel_name(lib)}"


@pytest.mark.parametrize("key", sorted(G.TURN))
def test_beyond_the_turn(lib, key):
    """More tiles than the workgroups of a capped launch: every workgroup takes a second tile, none twice."""
    shape, dtype, axis = G.TURN[key]
    assert G.turn_workgroups(key) > G.BLOCKS_MAX
    valid = G.drawn(shape, 1, np.dtype(dtype).name)
    dev = G.upload(lib, shape, valid)
    w, mode = G.radius_weights(2), G.REFLECT if axis else G.WRAP
    out = G.sentinel_array(lib, dev)
    G.smooth_axis(lib, dev, out, axis, w, mode | (G.CELL if key.startswith("cell") else 0))
    name = G.kernel_name(lib)
    kind, _, inst = key.partition("_")
    expect = f"gauss_{kind}_kernel<{'double' if dtype == np.float64 else 'float'}" + (f",{inst[-1]}>" if kind == "march" else ">")
    assert name == expect, (name, expect)
    G.assert_same(out.get_valid(), G.filter_axis(valid, axis, w, mode), key)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", G.MODES, ids=MODE_IDS)
def test_nonfinite_cells_propagate(lib, mode, dtype):
    """NaN, +inf and -inf in the first, the last and the seam cells of every component, through every instance."""
    for shape, axis in (((130,), 0), ((3, 130), 1), ((130, 6), 0), ((2, 65, 5), 1), ((65, 3, 64), 0), ((2, 2, 65), 2)):
        valid = G.drawn(shape, 3, np.dtype(dtype).name, planted=True)
        for r in (1, 7, shape[axis] + 1):
            G.check_pass(lib, valid, shape, axis, G.radius_weights(r), mode, f"planted {shape} axis {axis} r {r}")


def test_release_scratch_frees_the_staged_weights(lib):
    shape, axis = (5, 70), 1
    valid = G.drawn(shape, 1, "float64")
    dev = G.upload(lib, shape, valid)
    before = [G.run_pass(lib, dev, axis, G.radius_weights(r), G.WRAP) for r in (3, 100, 3)]
    lib.release_scratch()
    after = [G.run_pass(lib, dev, axis, G.radius_weights(r), G.WRAP) for r in (3, 100, 3)]
    for b, a, r in zip(before, after, (3, 100, 3)):
        assert np.array_equal(G.bits(b), G.bits(a))
        G.assert_same(a, G.filter_axis(valid, axis, G.radius_weights(r), G.WRAP), f"after release r {r}")


def test_weights_are_consumed_before_return(lib):
    """Six passes enqueued back to back from ONE host array that is overwritten after every call: each pass used the weights it was given."""
    shape = (40, 70)
    valid = G.drawn(shape, 1, "float64")
    dev = G.upload(lib, shape, valid)
    outs = [G.sentinel_array(lib, dev) for _ in range(6)]
    scratch = np.zeros(16)
    radii = (1, 5, 2, 7, 0, 3)
    for out, r in zip(outs, radii):
        scratch[: r + 1] = G.radius_weights(r)
        G.smooth_axis(lib, dev, out, r % 2, scratch[: r + 1], G.REFLECT)
        scratch[:] = np.nan
    for out, r in zip(outs, radii):
        G.assert_same(out.get_valid(), G.filter_axis(valid, r % 2, G.radius_weights(r), G.REFLECT), f"r {r}")


def test_entry_point_refuses_bad_arguments(lib):
    G.refuse_bad_arguments(lib)


# ---- the Python side, through the mirror classes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", G.DTYPES, ids=IDS)
def test_resident_run_keeps_the_state_on_the_device(dtype):
    """In place, ``device=True`` into ``slice_field`` and the statistics, a host result: the counters do not move."""
    G.resident_run_checks(pde_hip.get_backend("hip"), dtype)


def test_f32_arithmetic_mode_does_not_change_the_call():
    """The pure-fp32 mode serves the call with the same bits: scipy's line buffers are double for both field types."""
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.CartesianGrid([(0, 7.5), (0, 3.0), (0, 14.0)], (5, 6, 7), periodic=[False, True, False])
    field = pde_hip.ScalarField(grid, G.S.draw(grid.shape, 1, np.float32, seed=8)[0])
    ref = pde_hip.smooth(field, 1.1)
    backend.f32_arithmetic = "fp32"
    try:
        got = pde_hip.smooth(field, 1.1)
    finally:
        backend.f32_arithmetic = None
    assert got.dtype == np.float32 and np.array_equal(G.bits(got.data), G.bits(ref.data))
    G.assert_same(ref.data, field.smooth(1.1, out=field.copy()).data, "against the mirror method")
