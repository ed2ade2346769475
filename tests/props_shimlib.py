"""The host shim (tests/shimlib.py) with the statistics, distribution, domain and domain-property entry points (TESTS ONLY).

``tests/shim/pdehip_shim_props.c`` holds a plain sequential C version of ``pdehip_domain_properties``; ``build()`` links it with the shim's
own objects and the statistics, distribution and domain additions into ``tests/shim/_build/libpdehip_shim_props.so`` and ``use_shim()`` is
``shimlib.use_shim()`` with that library.  ``label_shimlib`` keeps lacking the entry point, which is what the test of a library without it
needs.
"""

from __future__ import annotations

import contextlib
import os
import subprocess

import hist_shimlib
import label_shimlib
import shimlib
import stats_shimlib

SOURCE = shimlib.SHIM_DIR / "pdehip_shim_props.c"
SO = shimlib.SHIM_SO.parent / "libpdehip_shim_props.so"


def build() -> os.PathLike:
    base = shimlib.build()
    objs = [base.parent / "shim.o"] + ([base.parent / "comm.o"] if (shimlib.SHIM_DIR / "pdehip_shim_comm.cpp").exists() else [])
    if not all(o.exists() for o in objs):
        shimlib.build(force=True)
    header = shimlib.SHIM_DIR.parent.parent / "include" / "pdehip.h"
    sources = (stats_shimlib.SOURCE, hist_shimlib.SOURCE, label_shimlib.SOURCE, SOURCE)
    if SO.exists() and all(SO.stat().st_mtime >= p.stat().st_mtime for p in (*sources, header, *objs)):
        return SO
    own = [base.parent / f"props_{src.stem}.{os.getpid()}.o" for src in sources]
    for src, obj in zip(sources, own):
        subprocess.run(["gcc", *shimlib._CFLAGS, "-c", str(src), "-o", str(obj)], check=True)
    tmp = SO.with_suffix(f".{os.getpid()}.tmp")
    subprocess.run(["g++", "-shared", "-fopenmp", "-o", str(tmp), *map(str, objs), *map(str, own), "-lm", "-ldl", "-lpthread"], check=True)
    os.replace(tmp, SO)
    for obj in own:
        obj.unlink()
    return SO


@contextlib.contextmanager
def use_shim(**kwargs):
    """``shimlib.use_shim(**kwargs)`` with the library that also has ``pdehip_domain_properties``."""
    so = build()
    saved = shimlib.build
    shimlib.build = lambda force=False: so
    try:
        with shimlib.use_shim(**kwargs) as lib:
            yield lib
    finally:
        shimlib.build = saved
