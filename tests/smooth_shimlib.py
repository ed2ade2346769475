"""The host shim (tests/shimlib.py) with the smoothing entry point (TESTS ONLY).

``tests/shim/pdehip_shim_smooth.c`` holds a plain C version of ``pdehip_smooth_axis``; ``build()`` links it with the shim's own objects and
the statistics and projection sources of ``tests/stats_shimlib.py`` / ``tests/project_shimlib.py`` into
``tests/shim/_build/libpdehip_shim_smooth.so`` and ``use_shim()`` is ``shimlib.use_shim()`` with that library.  The plain shim, the
statistics shim and the projection shim keep lacking the entry point, which is what the tests of a library without it need.
"""

from __future__ import annotations

import contextlib
import os
import subprocess

import project_shimlib
import shimlib
import stats_shimlib

SOURCE = shimlib.SHIM_DIR / "pdehip_shim_smooth.c"
SO = shimlib.SHIM_SO.parent / "libpdehip_shim_smooth.so"


def build() -> os.PathLike:
    base = shimlib.build()
    build_dir = base.parent
    objs = [build_dir / "shim.o"] + ([build_dir / "comm.o"] if (shimlib.SHIM_DIR / "pdehip_shim_comm.cpp").exists() else [])
    if not all(o.exists() for o in objs):
        shimlib.build(force=True)
    header = shimlib.SHIM_DIR.parent.parent / "include" / "pdehip.h"
    sources = (SOURCE, project_shimlib.SOURCE, stats_shimlib.SOURCE)
    if SO.exists() and all(SO.stat().st_mtime >= p.stat().st_mtime for p in (*sources, header, *objs)):
        return SO
    own = [build_dir / f"{src.stem}.smooth.{os.getpid()}.o" for src in sources]      # (objects of this process alone: test workers build side by side)
    tmp = SO.with_suffix(f".{os.getpid()}.tmp")
    try:
        for src, obj in zip(sources, own):
            subprocess.run(["gcc", *shimlib._CFLAGS, "-c", str(src), "-o", str(obj)], check=True)
        subprocess.run(["g++", "-shared", "-fopenmp", "-o", str(tmp), *map(str, objs), *map(str, own), "-lm", "-ldl", "-lpthread"], check=True)
    finally:
        for obj in own:
            obj.unlink(missing_ok=True)
    os.replace(tmp, SO)
    return SO


@contextlib.contextmanager
def use_shim(**kwargs):
    """``shimlib.use_shim(**kwargs)`` with the library that has the statistics, the projection and the smoothing entry points."""
    so = build()
    saved = shimlib.build
    shimlib.build = lambda force=False: so
    try:
        with shimlib.use_shim(**kwargs) as lib:
            yield lib
    finally:
        shimlib.build = saved
