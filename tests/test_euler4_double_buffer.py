"""The second buffers of the images of levels 1 and 2 of the four-step sweep and the order of its phase, enumerated on a CPU: `alt_index`,
`alt_read_index` and `SCHEDULE` of `py-pde_amd/csrc/pdehip_euler4_plan.h` (what pdehip_march4.inc indexes with and the order it follows)
through a tests-only probe (`tests/shim/euler4_alt_probe.cpp`, built by g++ here like the image probe of tests/test_euler4_image.py).

With a second buffer for images 1 and 2 a phase has two barriers instead of four: what level l - 1 computes goes into the buffer of image l
that nobody reads in this phase, and the buffers change places from phase to phase.  The four first buffers are the static image
(tests/test_euler4_image.py, tests/test_euler4_lanes.py); the two second ones lie in an allocation of their own, the kernel's dynamic LDS.
Checked here: every index of every lane lies in that allocation and in its own buffer; arrays and guard runs tile it; every access of every
wave is conflict-free by the bank rule of tests/test_euler4_image.py (restated below); the halo argument for the second buffers; the sum of
static and dynamic LDS; and a walk over three phases of the schedule: between a store and a read of one buffer, in either order, lies a
barrier.
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "py-pde_amd" / "csrc" / "pdehip_euler4_plan.h"
PROBE = ROOT / "tests" / "shim" / "euler4_alt_probe.cpp"
BUILD = ROOT / "tests" / "shim" / "_build"
GEOMETRY = "PY NPY NPZ PATCHES THREADS READ_KINDS WAVES ARR GUARD ALT_LEVELS ALT_LEVEL ALT_IMAGE ALT_BYTES LDS_BYTES SCHEDULE_EVENTS".split()
ABOVE, BELOW, LEFT, RIGHT = (0, 1), (2, 3), (4, 5), (6, 7)   # ReadKind: above / below by cell, left / right by row
ALT = (1, 2)                                                 # the levels whose image has a second buffer
STORE, READ, BARRIER = 0, 1, 2


@pytest.fixture(scope="module")
def alt():
    BUILD.mkdir(exist_ok=True)
    so = BUILD / "libe4alt_probe.so"
    if not so.exists() or so.stat().st_mtime < max(HEADER.stat().st_mtime, PROBE.stat().st_mtime):
        tmp = so.with_suffix(f".{os.getpid()}.tmp")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", str(PROBE), "-o", str(tmp)], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(str(so))
    out = (C.c_long * len(GEOMETRY))()
    lib.e4alt_geometry(out)
    g = SimpleNamespace(**dict(zip(GEOMETRY, out)))
    g.patch = np.array([lib.e4alt_lane_patch(t) for t in range(g.THREADS)])
    g.levels = np.array([lib.e4alt_wave_levels(w) for w in range(g.WAVES)])
    g.wave = np.arange(g.THREADS) // 64
    # store[l - 1, r, c, t], read[l - 1, k, t]: the index (in doubles) lane t uses in the second buffer of image l
    g.store = np.array([[[[lib.e4alt_index(l, r, c, int(p)) for p in g.patch] for c in range(2)] for r in range(g.PY)] for l in ALT])
    g.read = np.array([[[lib.e4alt_read_index(l, k, int(p)) for p in g.patch] for k in range(g.READ_KINDS)] for l in ALT])
    ev = (C.c_int * 4)()
    g.schedule = []
    for k in range(g.SCHEDULE_EVENTS):
        lib.e4alt_schedule(k, ev)
        g.schedule.append(tuple(ev))
    g.lib = lib
    return g


def test_geometry(alt):
    g = alt
    assert (g.ALT_LEVELS, g.ALT_LEVEL, g.ALT_IMAGE) == (2, 36 + 4 * 720 + 36, 2 * (36 + 4 * 720 + 36))
    assert g.ALT_BYTES == 8 * g.ALT_IMAGE == 2 * 23616
    assert g.LDS_BYTES == 102144
    assert 102144 + g.ALT_BYTES <= 160 * 1024          # static and dynamic LDS of one workgroup fit a CU
    assert g.LDS_BYTES % 16 == 0 and g.ALT_BYTES % 16 == 0


def test_every_index_of_every_lane_is_inside_its_buffer(alt):
    g = alt
    assert g.store.shape == (2, 2, 2, 768) and g.read.shape == (2, 8, 768)
    for idx in (g.store, g.read):
        assert idx.min() >= 0 and idx.max() < g.ALT_IMAGE
    for b in range(g.ALT_LEVELS):
        lo, hi = b * g.ALT_LEVEL, (b + 1) * g.ALT_LEVEL
        assert g.read[b].min() >= lo and g.read[b].max() < hi                       # reads: arrays and guard runs of the buffer
        assert g.store[b].min() >= lo + g.GUARD and g.store[b].max() < hi - g.GUARD   # stores: its arrays


def test_arrays_and_guard_runs_tile_the_allocation(alt):
    g = alt
    pieces = []
    for b, l in enumerate(ALT):
        pieces.append(b * g.ALT_LEVEL + np.arange(g.GUARD))
        for r in range(g.PY):
            for c in range(2):
                pieces.append(np.array([g.lib.e4alt_index(l, r, c, p) for p in range(g.PATCHES)]))
        pieces.append((b + 1) * g.ALT_LEVEL - g.GUARD + np.arange(g.GUARD))
    assert len(pieces) == 2 * (g.PY * 2 + 2)
    everything = np.concatenate(pieces)
    assert len(np.unique(everything)) == len(everything) == g.ALT_IMAGE          # no overlap ...
    assert everything.min() == 0 and everything.max() == g.ALT_IMAGE - 1         # ... and no hole


def test_built_like_the_first_buffers(alt):
    """Every access of a lane is a base plus its patch number, and a neighbour is the same constant offset of the patch number as in the
    first buffer: alt_index and alt_read_index differ from image_index and read_index by one constant per level."""
    g = alt
    for l in ALT:
        shift = g.lib.e4alt_index(l, 0, 0, 0) - g.lib.e4alt_image_index(l, 0, 0, 0)
        for p in range(g.PATCHES):
            for r in range(g.PY):
                for c in range(2):
                    assert g.lib.e4alt_index(l, r, c, p) == g.lib.e4alt_image_index(l, r, c, p) + shift
            for k in range(g.READ_KINDS):
                assert g.lib.e4alt_read_index(l, k, p) == g.lib.e4alt_image_read_index(l, k, p) + shift


def _conflicts(index, lanes_per_group, banks):
    """extra LDS cycles of one wave access of 8 bytes per lane: per lane group and bank, the distinct addresses beyond the first
    (the rule of tests/test_euler4_image.py: an 8-byte read is two groups of 32 lanes on 64 banks of 4 bytes, an 8-byte store four groups of
    16 lanes on 32 banks; equal addresses are one access)"""
    extra = 0
    for g0 in range(0, 64, lanes_per_group):
        by_bank = {}
        for i in np.unique(index[g0:g0 + lanes_per_group]):
            for dword in (2 * int(i), 2 * int(i) + 1):
                by_bank.setdefault(dword % banks, set()).add(int(i))
        extra += sum(len(v) - 1 for v in by_bank.values())
    return extra


def test_the_conflict_count_counts():
    assert _conflicts(np.arange(64), 32, 64) == 0
    assert _conflicts(2 * np.arange(64), 32, 64) == 2 * 32
    assert _conflicts(np.zeros(64, int), 32, 64) == 0
    assert _conflicts(np.r_[np.arange(15), 16, np.zeros(48, int)], 16, 32) == 2


@pytest.mark.parametrize("wave", range(12))
def test_reads_and_stores_are_conflict_free(alt, wave):
    """every wave, whether its role executes the level or not, and wherever the allocation begins (a base shifts all banks of an access
    alike: the beginning itself, the end of the static image, an odd number of doubles)"""
    g = alt
    sl = slice(64 * wave, 64 * wave + 64)
    for base in (0, 102144 // 8, 5):
        for b in range(g.ALT_LEVELS):
            for k in range(g.READ_KINDS):     # ds_read_b64: 2 x 32 lanes, 64 banks
                assert _conflicts(base + g.read[b, k, sl], 32, 64) == 0, (wave, b, k)
            for r in range(g.PY):
                for c in range(2):            # ds_write_b64: 4 x 16 lanes, 32 banks
                    assert _conflicts(base + g.store[b, r, c, sl], 16, 32) == 0, (wave, b, r, c)


def test_valid_cells_read_what_the_owner_stored(alt):
    """The halo argument of tests/test_euler4_image.py::test_valid_cells_read_valid_cells_of_the_level_below for the second buffers, by
    lane and by role as in tests/test_euler4_lanes.py: level L = 2, 3 reads the image of level L - 1 = 1, 2.  Whatever a cell that is valid
    at level L reads from the second buffer is the cell of level L - 1 it should be, valid there, at the index where a lane of a wave that
    executes level L - 1 stores it - so the zeros of a skipped level and of the guard runs only feed cells that are invalid at their level."""
    g = alt
    ry, rz = g.NPY * g.PY, g.NPZ * 2

    def valid(level, row, col):
        return level <= row < ry - level and level <= col < rz - level

    lanes_of = {p: np.flatnonzero(g.patch == p) for p in range(g.PATCHES)}
    checked = 0
    for level in (2, 3):
        b = level - 2                    # the buffer of image level - 1
        for p in range(g.PATCHES):
            row0, col0 = p // g.NPZ * g.PY, p % g.NPZ * 2
            uses = [(ABOVE[c], (0, c), (row0 - 1, col0 + c)) for c in range(2)] + [(BELOW[c], (1, c), (row0 + 2, col0 + c)) for c in range(2)]
            uses += [(LEFT[r], (r, 0), (row0 + r, col0 - 1)) for r in range(2)] + [(RIGHT[r], (r, 1), (row0 + r, col0 + 2)) for r in range(2)]
            if not any(valid(level, row0 + r, col0 + c) for r in range(2) for c in range(2)):
                continue
            computing = [t for t in lanes_of[p] if g.levels[g.wave[t]] >= level]
            assert computing, (level, p)
            for kind, (r, c), (nrow, ncol) in uses:
                if not valid(level, row0 + r, col0 + c):
                    continue
                assert valid(level - 1, nrow, ncol), (level, p, kind)
                pn = (nrow // g.PY) * g.NPZ + ncol // 2
                storing = [t for t in lanes_of[pn] if g.levels[g.wave[t]] >= level - 1]     # it has computed level L - 1: it stores it
                assert storing, (level, p, kind, pn)
                for t in storing:
                    for tr in computing:
                        assert g.read[b, kind, tr] == g.store[b, nrow % g.PY, ncol % 2, t], (level, p, kind)
                checked += 1
    assert checked == 2 * (36 * 68 + 34 * 66)      # two reads per valid cell of levels 2 and 3


def _walk(schedule, phases=3):
    """Replay `phases` phases behind the prologue.  Returns the accesses as (time, interval, op, (image, buffer), phase): `interval` counts
    the barriers passed.  Waves run freely between two barriers, so accesses of one interval are unordered among the waves.  The prologue's
    stores carry phase -1 (the middle planes of iteration 0) and -2 (the zeros of the second buffers)."""
    log, interval, time = [], 0, 0
    for image, buffer, phase in ((0, 0, -1), (1, 0, -1), (2, 0, -1), (3, 0, -1), (1, 1, -2), (2, 1, -2)):
        log.append((time, interval, STORE, (image, buffer), phase))
        time += 1
    interval += 1                                                               # its one barrier
    for phase in range(phases):
        parity = phase & 1
        for op, image, other, _ in schedule:
            if op == BARRIER:
                interval += 1
                continue
            buffer = (parity ^ other) if image in ALT else 0
            log.append((time, interval, op, (image, buffer), phase))
            time += 1
    return log


def _hazards(log):
    """pairs (store, read) or (read, store) of one buffer, neighbours in the order of that buffer's accesses, with no barrier between"""
    bad = []
    for key in sorted({e[3] for e in log}):
        mine = [e for e in log if e[3] == key]
        for first, second in zip(mine, mine[1:]):
            if first[2] != second[2] and first[1] == second[1]:
                bad.append((first, second))
    return bad


def test_the_schedule_is_the_one_described(alt):
    g = alt
    sched = g.schedule
    assert [e[0] for e in sched].count(BARRIER) == 2                        # two barriers per phase
    passed = 0
    for op, image, other, interval in sched:
        assert interval == passed                                           # the interval a line claims is the one it lies in
        passed += op == BARRIER
        assert other in (0, 1) and (other == 0 or image in ALT)
    for image in range(4):
        assert [e[:2] for e in sched].count((READ, image)) == 1 and [e[:2] for e in sched].count((STORE, image)) == 1
    order = [e[:3] for e in sched]
    # reads: the buffer of the phase's parity; stores of images 1 and 2: the other one, behind the read they are computed from
    assert all(other == 0 for op, _, other in order if op == READ)
    assert (STORE, 1, 1) in order and (STORE, 2, 1) in order
    assert order.index((READ, 0, 0)) < order.index((STORE, 1, 1)) and order.index((READ, 1, 0)) < order.index((STORE, 2, 1))
    # level 3's plane is computed from image 2 in one phase and stored at the head of the next, before anything else
    assert order[0] == (STORE, 3, 0)


def test_a_barrier_lies_between_every_store_and_read_of_one_buffer(alt):
    log = _walk(alt.schedule, phases=3)
    assert len(log) == 6 + 3 * 8 and log[-1][1] == 1 + 3 * 2 - 1       # (the last access lies in front of the last barrier)
    assert _hazards(log) == []
    assert _hazards(_walk(alt.schedule, phases=6)) == []
    # Every read finds the plane meant for it.  Image 3's is stored at the head of the same phase; the others' in the phase before
    # (iteration 0: by the prologue) - so the buffers of images 1 and 2 change places in step with the reads.
    stored = {(e[3][0], e[4]): e[3][1] for e in log if e[2] == STORE and e[4] != -2}
    for _, _, op, (image, buffer), phase in log:
        if op == READ:
            assert stored[(image, phase if image == 3 else phase - 1)] == buffer, (phase, image, buffer)


def test_the_walk_finds_hazards(alt):
    """the same walk on schedules that are wrong: one buffer per image under two barriers, and the store of image 0 in front of barrier A"""
    single = [(op, image, 0, interval) for op, image, _, interval in alt.schedule]
    assert _hazards(_walk(single))
    early = [e for e in alt.schedule if e != (STORE, 0, 0, 1)]
    early.insert(early.index((BARRIER, -1, 0, 0)), (STORE, 0, 0, 0))
    assert len(early) == len(alt.schedule) and _hazards(_walk(early))
