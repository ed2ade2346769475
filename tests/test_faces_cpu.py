"""``py-pde_amd/csrc/pdehip_faces.h`` on a CPU: which faces the stencil kernels evaluate on the fly (``scalar_face``), the all-or-nothing conversion
(``faces_to_input_bcs``) and the splitting one (``split_faces``), through ``tests/shim/faces_probe.cpp`` (built with g++ here).  Every expected table
is written out: rows (on, idx, c, f) in the order axis 0 lower, axis 0 upper, axis 1 lower, ... of the NORMALISED axes (grid axis a of an n-D grid is
axis 3 - n + a)."""

from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "py-pde_amd" / "csrc" / "pdehip_faces.h"
PROBE = ROOT / "tests" / "shim" / "faces_probe.cpp"
BUILD = ROOT / "tests" / "shim" / "_build"

SKIP, ORDER1, ORDER2 = 0, 1, 2
OFF = (0, 0, 0.0, 0.0)


@pytest.fixture(scope="module")
def lib():
    BUILD.mkdir(exist_ok=True)
    so = BUILD / "libfaces_probe.so"
    if not so.exists() or so.stat().st_mtime < max(HEADER.stat().st_mtime, PROBE.stat().st_mtime):
        tmp = so.with_suffix(f".{os.getpid()}.tmp")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", str(PROBE), "-o", str(tmp)], check=True)
        os.replace(tmp, so)
    return C.CDLL(str(so))


def _flat(faces):
    vals = [float(v) for face in faces for v in face]
    return (C.c_double * len(vals))(*vals)


def _table(buf):
    return [(int(buf[4 * i]), int(buf[4 * i + 1]), buf[4 * i + 2], buf[4 * i + 3]) for i in range(6)]


def convert_all(lib, n3, faces, first_axis=0, xplain=0):
    """the table, or None where the conversion refuses"""
    fg = (C.c_double * 24)(*([-7.0] * 24))
    ok = lib.faces_probe_all(C.c_long(len(faces) // 2), (C.c_long * 3)(*n3), _flat(faces), C.c_long(first_axis), C.c_long(xplain), fg)
    return _table(fg) if ok else None


def split(lib, n3, faces, can_fuse=True, mask=7):
    """(table, kinds of the table left for the ghost kernel, (fused, rest))"""
    fg = (C.c_double * 24)(*([-7.0] * 24))
    kinds, counts = (C.c_long * 6)(), (C.c_long * 2)()
    lib.faces_probe_split(C.c_long(len(faces) // 2), (C.c_long * 3)(*n3), _flat(faces), C.c_long(can_fuse), C.c_long(mask), fg, kinds, counts)
    return _table(fg), list(kinds), tuple(counts)


# (kind, flags, index1, const_v, factor1): a 4 x 5 x 6 grid, periodic along axis 0, two walls each along axes 1 and 2
N3 = (4, 5, 6)
SIX = [(ORDER1, 0, 3, 0.0, 1.0), (ORDER1, 0, 0, 0.0, 1.0),
       (ORDER1, 0, 0, 2.0, -1.0), (ORDER1, 0, 4, 0.5, 1.0),
       (ORDER1, 0, 0, 0.25, 1.0), (ORDER1, 0, 5, -0.25, 1.0)]
SIX_TABLE = [(1, 3, 0.0, 1.0), (1, 0, 0.0, 1.0),
             (1, 0, 2.0, -1.0), (1, 4, 0.5, 1.0),
             (1, 0, 0.25, 1.0), (1, 5, -0.25, 1.0)]


def test_the_header_is_plain_host_code():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-"], input=f'#include "{HEADER}"\n', text=True, check=True)
    text = HEADER.read_text()
    assert "hip_runtime" not in text and "__device__" not in text and "__global__" not in text


def test_the_face_test(lib):
    ask = lambda face, n: lib.faces_probe_scalar(_flat([face]), C.c_long(n))    # noqa: E731
    assert ask((ORDER1, 0, 0, 1.5, -1.0), 6) == 1 and ask((ORDER1, 0, 5, 0.0, 1.0), 6) == 1
    assert ask((ORDER1, 0, 6, 0.0, 1.0), 6) == 0 and ask((ORDER1, 0, -1, 0.0, 1.0), 6) == 0            # index1 == n, index1 == -1
    assert ask((ORDER2, 0, 0, 0.0, 1.0), 6) == 0 and ask((SKIP, 0, 0, 0.0, 1.0), 6) == 0
    assert ask((ORDER1, 1, 0, 0.0, 1.0), 6) == 0 and ask((ORDER1, 2, 0, 0.0, 1.0), 6) == 0              # coefficient arrays, `normal`
    assert ask((ORDER1, 0, 0, 0.0, 1.0), 1) == 1 and ask((ORDER1, 0, 1, 0.0, 1.0), 1) == 0              # a one-cell axis


def test_six_scalar_faces(lib):
    assert convert_all(lib, N3, SIX) == SIX_TABLE
    assert split(lib, N3, SIX) == (SIX_TABLE, [SKIP] * 6, (6, 0))
    # a call that cannot fuse leaves every face to the ghost kernel
    assert split(lib, N3, SIX, can_fuse=False) == ([OFF] * 6, [ORDER1] * 6, (0, 6))


def test_a_fuse_mask_of_5_leaves_the_middle_axis_to_the_ghost_kernel(lib):
    table = [SIX_TABLE[0], SIX_TABLE[1], OFF, OFF, SIX_TABLE[4], SIX_TABLE[5]]
    assert split(lib, N3, SIX, mask=5) == (table, [SKIP, SKIP, ORDER1, ORDER1, SKIP, SKIP], (4, 2))
    assert split(lib, N3, SIX, mask=0) == ([OFF] * 6, [ORDER1] * 6, (0, 6))


def test_faces_the_kernels_do_not_evaluate(lib):
    # axis 0: index1 == -1 and index1 == n; axis 1: scalar, second order; axis 2: coefficient arrays, scalar
    faces = [(ORDER1, 0, -1, 0.0, 1.0), (ORDER1, 0, 4, 0.0, 1.0),
             (ORDER1, 0, 0, 2.0, -1.0), (ORDER2, 0, 4, 0.5, 2.0),
             (ORDER1, 1, 0, 0.25, 1.0), (ORDER1, 0, 5, -0.25, 1.0)]
    assert convert_all(lib, N3, faces) is None
    table = [OFF, OFF, (1, 0, 2.0, -1.0), OFF, OFF, (1, 5, -0.25, 1.0)]
    assert split(lib, N3, faces) == (table, [ORDER1, ORDER1, SKIP, ORDER2, ORDER1, SKIP], (2, 4))
    # each of them alone refuses the all-or-nothing form
    for i, face in enumerate(faces):
        if i not in (2, 5):
            assert convert_all(lib, N3, [*SIX[:i], face, *SIX[i + 1:]]) is None, i
    # a face that is skipped (towards a neighbour of a decomposed grid) is in neither count and never fused
    faces = [(SKIP, 0, 0, 0.0, 0.0), *SIX[1:]]
    assert convert_all(lib, N3, faces) is None
    assert split(lib, N3, faces) == ([OFF, *SIX_TABLE[1:]], [SKIP] * 6, (5, 0))


def test_axes_of_a_2d_and_a_1d_grid_are_the_trailing_ones(lib):
    two = SIX[2:]                     # grid axis 0 -> axis 1 (5 cells), grid axis 1 -> axis 2 (6 cells)
    table = [OFF, OFF, *SIX_TABLE[2:]]
    assert convert_all(lib, (1, 5, 6), two) == table
    assert split(lib, (1, 5, 6), two) == (table, [SKIP] * 6, (4, 0))
    assert split(lib, (1, 5, 6), two, mask=5) == ([OFF, OFF, OFF, OFF, *SIX_TABLE[4:]], [ORDER1, ORDER1, SKIP, SKIP, SKIP, SKIP], (2, 2))
    # the extent that counts is the normalised axis's: index 5 fits axis 2 (6 cells), not axis 1 (5 cells)
    assert convert_all(lib, (1, 5, 6), [SIX[2], (ORDER1, 0, 5, 0.5, 1.0), *SIX[4:]]) is None
    one = SIX[4:]                     # grid axis 0 -> axis 2
    table = [OFF, OFF, OFF, OFF, *SIX_TABLE[4:]]
    assert convert_all(lib, (1, 1, 6), one) == table
    assert split(lib, (1, 1, 6), one) == (table, [SKIP] * 6, (2, 0))
    assert split(lib, (1, 1, 6), one, mask=3) == ([OFF] * 6, [ORDER1, ORDER1, SKIP, SKIP, SKIP, SKIP], (0, 2))
    assert split(lib, (1, 1, 6), [(ORDER1, 0, 6, 0.0, 1.0), SIX[5]]) == ([OFF] * 5 + [SIX_TABLE[5]], [ORDER1, SKIP, SKIP, SKIP, SKIP, SKIP], (1, 1))


def test_xplain(lib):
    """The slowest axis of a slab: real halo layers on both sides (1), on its upper side only (2: the lower face is a condition), on its lower
    side only (3: the upper face is one); the callers pass first_axis = 1 with each."""
    second = (ORDER2, 0, 0, 0.0, 1.0)
    rest = SIX_TABLE[2:]
    lower_only, upper_only = [SIX[0], second, *SIX[2:]], [second, SIX[1], *SIX[2:]]
    for faces in (SIX, lower_only, upper_only, [second, second, *SIX[2:]]):
        assert convert_all(lib, N3, faces, first_axis=1, xplain=1) == [OFF, OFF, *rest]
    assert convert_all(lib, N3, SIX, first_axis=1, xplain=2) == [SIX_TABLE[0], OFF, *rest]
    assert convert_all(lib, N3, lower_only, first_axis=1, xplain=2) == [SIX_TABLE[0], OFF, *rest]
    assert convert_all(lib, N3, upper_only, first_axis=1, xplain=2) is None
    assert convert_all(lib, N3, SIX, first_axis=1, xplain=3) == [OFF, SIX_TABLE[1], *rest]
    assert convert_all(lib, N3, upper_only, first_axis=1, xplain=3) == [OFF, SIX_TABLE[1], *rest]
    assert convert_all(lib, N3, lower_only, first_axis=1, xplain=3) is None
    # the other axes still decide
    assert convert_all(lib, N3, [*SIX[:3], second, *SIX[4:]], first_axis=1, xplain=1) is None
    # 2-D slabs: the slowest axis is axis 1
    assert convert_all(lib, (1, 5, 6), [second, SIX[3], *SIX[4:]], first_axis=1, xplain=3) == [OFF, OFF, OFF, SIX_TABLE[3], *SIX_TABLE[4:]]


def test_the_test_is_spelled_once_in_the_library():
    spelled = {}
    for path in sorted(HEADER.parent.glob("*")):
        if path.suffix in (".hip", ".h", ".inc"):
            text = path.read_text()
            count = text.count("flags != 0 || r.index1 < 0") + text.count("flags == 0 && r.index1 >= 0")
            if count:
                spelled[path.name] = count
    assert spelled == {"pdehip_faces.h": 1}
