"""The host shim (tests/shimlib.py) with the interpolation entry points (TESTS ONLY).

``tests/shim/pdehip_shim_interp.c`` holds plain C versions of ``pdehip_interpolate_points``, ``pdehip_interpolate_to_grid`` and
``pdehip_set_ghost_corners``; ``build()`` links it with the shim's own objects into ``tests/shim/_build/libpdehip_shim_interp.so``
and ``use_shim()`` is ``shimlib.use_shim()`` with that library.  The plain shim keeps lacking the three entry points, which is
what the tests of a library without them need.
"""

from __future__ import annotations

import contextlib
import os
import subprocess

import shimlib

SOURCE = shimlib.SHIM_DIR / "pdehip_shim_interp.c"
SO = shimlib.SHIM_SO.parent / "libpdehip_shim_interp.so"


def build() -> os.PathLike:
    base = shimlib.build()
    objs = [base.parent / "shim.o"] + ([base.parent / "comm.o"] if (shimlib.SHIM_DIR / "pdehip_shim_comm.cpp").exists() else [])
    if not all(o.exists() for o in objs):
        shimlib.build(force=True)
    header = shimlib.SHIM_DIR.parent.parent / "include" / "pdehip.h"
    if SO.exists() and all(SO.stat().st_mtime >= p.stat().st_mtime for p in (SOURCE, header, *objs)):
        return SO
    obj = base.parent / "interp.o"
    subprocess.run(["gcc", *shimlib._CFLAGS, "-c", str(SOURCE), "-o", str(obj)], check=True)
    tmp = SO.with_suffix(f".{os.getpid()}.tmp")
    subprocess.run(["g++", "-shared", "-fopenmp", "-o", str(tmp), *map(str, objs), str(obj), "-lm", "-ldl", "-lpthread"], check=True)
    os.replace(tmp, SO)
    return SO


@contextlib.contextmanager
def use_shim(**kwargs):
    """``shimlib.use_shim(**kwargs)`` with the library that has the interpolation entry points."""
    so = build()
    saved = shimlib.build
    shimlib.build = lambda force=False: so
    try:
        with shimlib.use_shim(**kwargs) as lib:
            yield lib
    finally:
        shimlib.build = saved
