"""Dead lanes of the halo waves and the 32-bit plane offsets of the four-step sweep, enumerated on a CPU: `lane_levels` and `offsets_fit` of
`py-pde_amd/csrc/pdehip_euler4_plan.h` through a tests-only probe (`tests/shim/euler4_levels_probe.cpp`, built by g++ here); the lane map,
the roles and the image come from the fixture of tests/test_euler4_lanes.py, whose halo argument by wave this file repeats by lane.

Inside waves 8 ... 10 (pdehip_march4.inc) lane t runs level L of a phase - the neighbour reads of image L - 1, the arithmetic, the image
store of level L - if L <= lane_levels(t); a lane with lane_levels(t) == 0 stores nothing to the image of level 0 either.  The owner waves
and wave 11 run every level of their role in every lane.  Checked here: lane_levels against the ring of the lane's patch; exactly the 48
spare lanes are at 0, each the second holder of its patch; every patch keeps an executing lane at every level it is needed at; whatever a
cell that is valid at level L reads was stored, at that index, by a lane that executes level L - 1; the accesses of the lanes that are left
are conflict-free; and `offsets_fit` at its boundary values.
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from test_euler4_lanes import ABOVE, BELOW, BUILD, HEADER, LEFT, RIGHT, ROOT, lanes  # noqa: F401  (the fixture)

PROBE = ROOT / "tests" / "shim" / "euler4_levels_probe.cpp"
MASKED_WAVES = (8, 9, 10)


@pytest.fixture(scope="module")
def probe():
    BUILD.mkdir(exist_ok=True)
    so = BUILD / "libe4levels_probe.so"
    if not so.exists() or so.stat().st_mtime < max(HEADER.stat().st_mtime, PROBE.stat().st_mtime):
        tmp = so.with_suffix(f".{os.getpid()}.tmp")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", str(PROBE), "-o", str(tmp)], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(str(so))
    lib.e4levels_offsets_fit.argtypes = [C.c_long, C.c_long]
    return lib


@pytest.fixture(scope="module")
def g(lanes, probe):  # noqa: F811
    lanes.ll = np.array([probe.e4levels_lane_levels(t) for t in range(lanes.THREADS)])
    return lanes


def executes(g, t, level):
    """lane t runs level `level` (1 ... 4) of a phase"""
    w = g.wave[t]
    return level <= g.levels[w] and (w not in MASKED_WAVES or level <= g.ll[t])


def stores(g, t, l):
    """lane t stores its cells of the image of level l (0 ... 3)"""
    if l == 0:
        return g.wave[t] not in MASKED_WAVES or g.ll[t] >= 1
    return executes(g, t, l)


def test_lane_levels_follow_the_ring_of_the_patch(g):
    live = g.ll > 0
    assert np.array_equal(g.ll[live], g.need[live])          # 1 for ring 0, 3 for ring 1, 4 for an output patch
    assert (g.ll[g.wave < g.OWNER_WAVES] == g.LEVELS).all()
    assert (g.ll[g.wave == g.WAVES - 1] == 1).all()
    assert (g.ll <= g.levels[g.wave]).all()                  # no lane is needed at more levels than its wave executes


def test_exactly_the_spare_lanes_are_at_zero(g):
    zero = np.flatnonzero(g.ll == 0)
    assert zero.size == g.THREADS - g.PATCHES == 48
    assert set(zero.tolist()) == {64 * w + lane for w in (9, 10) for lane in range(40, 64)}
    for t in zero:
        others = [u for u in np.flatnonzero(g.patch == g.patch[t]) if u != t]
        assert len(others) == 1                              # the second holder of its patch ...
        u = others[0]
        assert g.ll[u] == g.need[u] > 0 and g.wave[u] != g.wave[t] and g.wave[u] in (9, 10)   # ... whose first holder does the work


def test_every_patch_keeps_an_executing_lane_at_every_level_it_is_needed_at(g):
    for p in range(g.PATCHES):
        holders = np.flatnonzero(g.patch == p)
        need = g.need[holders[0]]
        for level in range(1, need + 1):
            assert any(executes(g, t, level) for t in holders), (p, level)
        assert any(stores(g, t, 0) for t in holders), p


def test_lane_levels_executed_per_phase(g):
    """2688 lane-levels per phase without the mask (42 wave-levels), 232 fewer with it"""
    unmasked = sum(64 * g.levels[w] for w in range(g.WAVES))
    masked = sum(executes(g, t, level) for t in range(g.THREADS) for level in range(1, g.LEVELS + 1))
    assert (unmasked, unmasked - masked) == (2688, 232)


def test_valid_cells_read_what_an_executing_lane_stored(g):
    """The lane-granular version of test_valid_cells_read_what_an_executing_wave_stored: for every cell valid at level L = 1 ... 4 its patch
    has a lane that executes level L; each value that lane takes from the image of level L - 1 belongs to a cell valid at level L - 1; and
    that cell's patch has a lane that stores level L - 1, at the index the reading lane reads.  So the cells of a masked lane - they keep
    the zeros of the prologue - are read only by cells that are invalid at their own level."""
    ry, rz = g.NPY * g.PY, g.NPZ * 2

    def valid(level, row, col):
        return level <= row < ry - level and level <= col < rz - level

    lanes_of = {p: np.flatnonzero(g.patch == p) for p in range(g.PATCHES)}
    checked = 0
    for level in range(1, g.LEVELS + 1):
        for p in range(g.PATCHES):
            row0, col0 = p // g.NPZ * g.PY, p % g.NPZ * 2
            if not any(valid(level, row0 + r, col0 + c) for r in range(2) for c in range(2)):
                continue
            uses = [(ABOVE[c], (0, c), (row0 - 1, col0 + c)) for c in range(2)] + [(BELOW[c], (1, c), (row0 + 2, col0 + c)) for c in range(2)]
            uses += [(LEFT[r], (r, 0), (row0 + r, col0 - 1)) for r in range(2)] + [(RIGHT[r], (r, 1), (row0 + r, col0 + 2)) for r in range(2)]
            computing = [t for t in lanes_of[p] if executes(g, t, level)]
            assert computing, (level, p)
            # the neighbours inside the patch are the lane's own registers: the same lane has computed level L - 1 (it executes every level up to L)
            assert all(executes(g, t, lv) for t in computing for lv in range(1, level))
            for kind, (r, c), (nrow, ncol) in uses:
                if not valid(level, row0 + r, col0 + c):
                    continue
                assert valid(level - 1, nrow, ncol), (level, p, kind)
                pn = (nrow // g.PY) * g.NPZ + ncol // 2
                storing = [t for t in lanes_of[pn] if stores(g, t, level - 1)]
                assert storing, (level, p, kind, pn)
                for t in storing:
                    for tr in computing:
                        assert g.read[level - 1, kind, tr] == g.store[level - 1, nrow % g.PY, ncol % 2, t], (level, p, kind)
                checked += 1
    assert checked == 2 * (38 * 70 + 36 * 68 + 34 * 66 + 32 * 64)


def _conflicts(index, active, lanes_per_group, banks):
    """extra LDS cycles of one wave access of 8 bytes per lane, over the active lanes: per lane group and bank, the distinct addresses
    beyond the first (the rule of tests/test_euler4_lanes.py)"""
    extra = 0
    for g0 in range(0, 64, lanes_per_group):
        by_bank = {}
        for i in np.unique(index[g0:g0 + lanes_per_group][active[g0:g0 + lanes_per_group]]):
            for dword in (2 * int(i), 2 * int(i) + 1):
                by_bank.setdefault(dword % banks, set()).add(int(i))
        extra += sum(len(v) - 1 for v in by_bank.values())
    return extra


@pytest.mark.parametrize("wave", MASKED_WAVES)
def test_the_lanes_that_are_left_access_without_conflicts(g, wave):
    sl = slice(64 * wave, 64 * wave + 64)
    ts = np.arange(64 * wave, 64 * wave + 64)
    assert _conflicts(np.r_[np.arange(15), 16, np.zeros(48, int)], np.ones(64, bool), 16, 32) == 2   # (the count counts)
    for l in range(g.LEVELS):
        reading = np.array([executes(g, t, l + 1) for t in ts])
        for k in range(g.READ_KINDS):         # ds_read_b64: 2 x 32 lanes, 64 banks
            assert _conflicts(g.read[l, k, sl], reading, 32, 64) == 0, (wave, l, k)
        storing = np.array([stores(g, t, l) for t in ts])
        for r in range(g.PY):
            for c in range(2):                # ds_write_b64: 4 x 16 lanes, 32 banks
                assert _conflicts(g.store[l, r, c, sl], storing, 16, 32) == 0, (wave, l, r, c)


def test_offsets_fit_at_its_boundary_values(probe):
    fit = probe.e4levels_offsets_fit
    top = 1 << 29                              # doubles in 2^32 bytes
    assert fit(0, top) == 1 and fit(0, top + 1) == 0
    assert fit(1, top - 1) == 1 and fit(1, top) == 0
    assert fit(top - 1, 1) == 1 and fit(top, 1) == 0 and fit(top, 0) == 0
    assert fit(0, 0) == 0 and fit(-1, 8) == 0 and fit(8, -1) == 0
    assert fit(1 << 40, 8) == 0 and fit(8, 1 << 40) == 0 and fit((1 << 62) + top, top) == 0   # no overflow in the sum
    # the benchmark's grid: 512^3 with one ghost layer, rows padded to 528 doubles
    p1 = 528
    p0 = p1 * 514
    assert fit(p0 + p1 + 2, p0) == 1
    # the largest in-plane byte offset of a grid that fits is below 2^32: off + (n1 - 1) * p1 + n2 - 1 < off + p0
    assert 8 * (top - 1) < 1 << 32
