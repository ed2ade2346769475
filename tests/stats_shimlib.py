"""The host shim (tests/shimlib.py) with the statistics entry points (TESTS ONLY).

``tests/shim/pdehip_shim_stats.c`` holds plain C versions of ``pdehip_field_stats`` and ``pdehip_steady_state``; ``build()`` links it
with the shim's own objects into ``tests/shim/_build/libpdehip_shim_stats.so`` and ``use_shim()`` is ``shimlib.use_shim()`` with that
library.  The plain shim keeps lacking the two entry points, which is what the tests of a library without them need.
"""

from __future__ import annotations

import contextlib
import os
import subprocess

import shimlib

SOURCE = shimlib.SHIM_DIR / "pdehip_shim_stats.c"
SO = shimlib.SHIM_SO.parent / "libpdehip_shim_stats.so"


def build() -> os.PathLike:
    base = shimlib.build()
    objs = [base.parent / "shim.o"] + ([base.parent / "comm.o"] if (shimlib.SHIM_DIR / "pdehip_shim_comm.cpp").exists() else [])
    if not all(o.exists() for o in objs):
        shimlib.build(force=True)
    header = shimlib.SHIM_DIR.parent.parent / "include" / "pdehip.h"
    if SO.exists() and all(SO.stat().st_mtime >= p.stat().st_mtime for p in (SOURCE, header, *objs)):
        return SO
    obj = base.parent / "stats.o"
    subprocess.run(["gcc", *shimlib._CFLAGS, "-c", str(SOURCE), "-o", str(obj)], check=True)
    tmp = SO.with_suffix(f".{os.getpid()}.tmp")
    subprocess.run(["g++", "-shared", "-fopenmp", "-o", str(tmp), *map(str, objs), str(obj), "-lm", "-ldl", "-lpthread"], check=True)
    os.replace(tmp, SO)
    return SO


@contextlib.contextmanager
def use_shim(**kwargs):
    """``shimlib.use_shim(**kwargs)`` with the library that has the statistics entry points."""
    so = build()
    saved = shimlib.build
    shimlib.build = lambda force=False: so
    try:
        with shimlib.use_shim(**kwargs) as lib:
            yield lib
    finally:
        shimlib.build = saved
