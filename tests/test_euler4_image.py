"""The LDS image of the four-step sweep, enumerated on a CPU: `py-pde_amd/csrc/pdehip_euler4_plan.h` (`image_index`, `read_index`,
`patch_of_thread`: the functions pdehip_march4.inc indexes with) through a tests-only probe (`tests/shim/euler4_image_probe.cpp`, built by
g++ here like the plan probe of tests/test_euler4_plan.py).

Per level, patch row and patch cell the image holds one array indexed by the patch number; a thread stores its 2 x 2 cells of each of the four
levels (16 stores) and reads, per level, eight cells of its neighbours at constant offsets of its own number (32 reads).  Checked here: every
index lies in the allocation; the arrays and guard runs tile the image without overlap; stores of different patches never meet; by the bank
rule of the hardware (an 8-byte read: two groups of 32 lanes, bank = dword address mod 64; an 8-byte store: four groups of 16 lanes, bank =
dword address mod 32; equal addresses are one access) every access of every wave is conflict-free; and the halo argument: whatever a cell that
is valid at level L reads from the image is the cell of level L - 1 it should be, stored by the patch that owns it, and valid there - so the
unspecified values that patches at the rim of the region read (other arrays, guard runs, through the row wrap) only feed cells outside the
valid region of their level.
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
PROBE = ROOT / "tests" / "shim" / "euler4_image_probe.cpp"
BUILD = ROOT / "tests" / "shim" / "_build"
GEOMETRY = "TY TZ PY HALO LEVELS NPY NPZ PATCHES THREADS ARR NARR GUARD IMAGE READ_KINDS ALLOC".split()
ABOVE, BELOW, LEFT, RIGHT = (0, 1), (2, 3), (4, 5), (6, 7)   # ReadKind: above / below by cell, left / right by row


@pytest.fixture(scope="module")
def img():
    BUILD.mkdir(exist_ok=True)
    so = BUILD / "libe4image_probe.so"
    if not so.exists() or so.stat().st_mtime < max(HEADER.stat().st_mtime, PROBE.stat().st_mtime):
        tmp = so.with_suffix(f".{os.getpid()}.tmp")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", str(PROBE), "-o", str(tmp)], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(str(so))
    out = (C.c_long * len(GEOMETRY))()
    lib.e4image_geometry(out)
    g = SimpleNamespace(**dict(zip(GEOMETRY, out)))
    g.patch = np.array([lib.e4image_patch_of_thread(t) for t in range(g.THREADS)])
    # store[l, r, c, t], read[l, k, t]: the index (in doubles) thread t uses
    g.store = np.array([[[[lib.e4image_index(l, r, c, int(p)) for p in g.patch] for c in range(2)] for r in range(g.PY)] for l in range(g.LEVELS)])
    g.read = np.array([[[lib.e4image_read_index(l, k, int(p)) for p in g.patch] for k in range(g.READ_KINDS)] for l in range(g.LEVELS)])
    g.lib = lib
    return g


def test_geometry_is_the_pinned_one(img):
    assert (img.TY, img.TZ, img.PY, img.HALO, img.LEVELS) == (32, 64, 2, 4, 4)
    assert (img.NPY, img.NPZ, img.PATCHES, img.THREADS) == (20, 36, 720, 768)
    assert (img.ARR, img.NARR, img.GUARD, img.IMAGE, img.READ_KINDS) == (720, 16, 36, 36 + 16 * 720 + 36, 8)
    assert img.ALLOC == 4 * 42 * 76 and img.IMAGE <= img.ALLOC   # the allocation tests/test_kernel_resources_euler4.py pins


def test_every_index_is_inside_the_allocation(img):
    """All 768 threads, 4 levels, the 4 stores and the 8 reads per level, and the two guard runs the first GUARD threads fill once."""
    assert img.store.shape == (4, 2, 2, 768) and img.read.shape == (4, 8, 768)
    for idx in (img.store, img.read):
        assert idx.min() >= 0 and idx.max() < img.ALLOC
    assert img.read.min() >= 0 and img.read.max() < img.IMAGE     # reads stay in the image proper: arrays and guard runs
    guards = np.concatenate([np.arange(img.GUARD), img.IMAGE - img.GUARD + np.arange(img.GUARD)])
    assert guards.min() >= 0 and guards.max() < img.ALLOC


def test_arrays_and_guard_runs_are_disjoint(img):
    pieces = [np.arange(img.GUARD), img.IMAGE - img.GUARD + np.arange(img.GUARD)]
    for l in range(img.LEVELS):
        for r in range(img.PY):
            for c in range(2):
                pieces.append(np.array([img.lib.e4image_index(l, r, c, p) for p in range(img.PATCHES)]))
    assert len(pieces) == img.NARR + 2
    everything = np.concatenate(pieces)
    assert len(np.unique(everything)) == len(everything) == img.IMAGE     # no overlap ...
    assert everything.min() == 0 and everything.max() == img.IMAGE - 1    # ... and no hole: they tile [0, IMAGE)


def test_stores_of_different_patches_never_meet(img):
    first = img.store[..., : img.PATCHES].reshape(-1)
    assert len(np.unique(first)) == first.size == 16 * img.PATCHES
    # the threads behind the last patch repeat a patch: the same cells again (the same values), and a patch that stores nothing to the field
    rest = img.patch[img.PATCHES:]
    assert np.array_equal(img.store[..., img.PATCHES:], img.store[..., rest])
    rows = rest // img.NPZ * img.PY
    assert ((rows < img.HALO) | (rows >= img.HALO + img.TY)).all()


def _conflicts(index, lanes_per_group, banks):
    """extra LDS cycles of one wave access of 8 bytes per lane: per lane group and bank, the distinct addresses beyond the first"""
    extra = 0
    for g0 in range(0, 64, lanes_per_group):
        by_bank = {}
        for i in np.unique(index[g0:g0 + lanes_per_group]):           # equal addresses: one access (broadcast)
            for dword in (2 * int(i), 2 * int(i) + 1):
                by_bank.setdefault(dword % banks, set()).add(int(i))
        extra += sum(len(v) - 1 for v in by_bank.values())
    return extra


def test_the_conflict_count_counts(img):
    """the rule itself, on patterns with a known answer: the row-major picture's left neighbour (16 bytes from lane to lane) was 2-way"""
    assert _conflicts(np.arange(64), 32, 64) == 0
    assert _conflicts(2 * np.arange(64), 32, 64) == 2 * 32       # every second bank pair, each used twice: 16 pairs x 2 dwords per group
    assert _conflicts(np.zeros(64, int), 32, 64) == 0            # broadcast
    assert _conflicts(np.r_[np.arange(16) + 704, np.zeros(48, int)], 32, 64) == 2   # one patch repeated behind the last ones: a second address on its banks


@pytest.mark.parametrize("wave", range(12))
def test_reads_and_stores_are_conflict_free(img, wave):
    lanes = slice(64 * wave, 64 * wave + 64)
    for l in range(img.LEVELS):
        for k in range(img.READ_KINDS):     # ds_read_b64: 2 x 32 lanes, 64 banks
            assert _conflicts(img.read[l, k, lanes], 32, 64) == 0, (wave, l, k)
        for r in range(img.PY):
            for c in range(2):              # ds_write_b64: 4 x 16 lanes, 32 banks
                assert _conflicts(img.store[l, r, c, lanes], 16, 32) == 0, (wave, l, r, c)


def test_valid_cells_read_valid_cells_of_the_level_below(img):
    """The halo argument by enumeration.  Level L is valid on the region of level 0 shrunk by L cells per side (widths 40 x 72, 38 x 70,
    36 x 68, 34 x 66; level 4: the 32 x 64 outputs).  For every patch and every one of its cells that is valid at level L = 1 ... 4, each
    value the cell takes from the image of level L - 1 is read at the index where the owner of the neighbouring cell stored it, and that
    cell is valid at level L - 1.  In particular this holds for every patch whose four cells are valid."""
    ry, rz = img.NPY * img.PY, img.NPZ * 2

    def valid(level, row, col):
        return level <= row < ry - level and level <= col < rz - level

    def stored_at(level, row, col):
        return img.lib.e4image_index(level, row % img.PY, col % 2, (row // img.PY) * img.NPZ + col // 2)

    checked = whole = 0
    for level in range(1, img.LEVELS + 1):
        for p in range(img.PATCHES):
            row0, col0 = p // img.NPZ * img.PY, p % img.NPZ * 2
            # (kind, the cell of the patch that uses it, the neighbour it must be)
            uses = [(ABOVE[c], (0, c), (row0 - 1, col0 + c)) for c in range(2)] + [(BELOW[c], (1, c), (row0 + 2, col0 + c)) for c in range(2)]
            uses += [(LEFT[r], (r, 0), (row0 + r, col0 - 1)) for r in range(2)] + [(RIGHT[r], (r, 1), (row0 + r, col0 + 2)) for r in range(2)]
            whole += all(valid(level, row0 + r, col0 + c) for r in range(2) for c in range(2))
            for kind, (r, c), (nrow, ncol) in uses:
                if not valid(level, row0 + r, col0 + c):
                    continue
                assert valid(level - 1, nrow, ncol), (level, p, kind)
                assert img.read[level - 1, kind, p] == stored_at(level - 1, nrow, ncol), (level, p, kind)
                checked += 1
    # two reads per valid cell; whole patches: 18 x 34 at levels 1 and 2 (rows 2 ... 37), 16 x 32 at levels 3 and 4
    assert checked == 2 * (38 * 70 + 36 * 68 + 34 * 66 + 32 * 64)
    assert whole == 2 * 18 * 34 + 2 * 16 * 32
