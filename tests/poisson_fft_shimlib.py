"""The host shim (tests/shimlib.py) with the inverse transform and the direct Poisson solve (TESTS ONLY).

``tests/shim/pdehip_shim_poisson_fft.c`` holds plain serial C versions of ``pdehip_fft_inverse`` and ``pdehip_poisson_fft`` (and, through
the spectrum shim's source it includes, of ``pdehip_fft_supported`` / ``pdehip_fft_forward`` / ``pdehip_shell_spectrum``); ``build()``
links it with the shim's own objects into ``tests/shim/_build/libpdehip_shim_poisson_fft.so`` and ``use_shim()`` is
``shimlib.use_shim()`` with that library.  The plain shim keeps lacking the entry points, which is what the tests of a library without
them need.  ``load()`` opens the library for direct calls next to the product's library (the device tests compare bits).
"""

from __future__ import annotations

import contextlib
import ctypes as C
import os
import subprocess

import shimlib

SOURCE = shimlib.SHIM_DIR / "pdehip_shim_poisson_fft.c"
INCLUDED = shimlib.SHIM_DIR / "pdehip_shim_spectrum.c"
SO = shimlib.SHIM_SO.parent / "libpdehip_shim_poisson_fft.so"


def build() -> os.PathLike:
    base = shimlib.build()
    objs = [base.parent / "shim.o"] + ([base.parent / "comm.o"] if (shimlib.SHIM_DIR / "pdehip_shim_comm.cpp").exists() else [])
    if not all(o.exists() for o in objs):
        shimlib.build(force=True)
    header = shimlib.SHIM_DIR.parent.parent / "include" / "pdehip.h"
    if SO.exists() and all(SO.stat().st_mtime >= p.stat().st_mtime for p in (SOURCE, INCLUDED, header, *objs)):
        return SO
    own = base.parent / f"poisson_fft_{SOURCE.stem}.{os.getpid()}.o"
    subprocess.run(["gcc", *shimlib._CFLAGS, "-c", str(SOURCE), "-o", str(own)], check=True)
    tmp = SO.with_suffix(f".{os.getpid()}.tmp")
    subprocess.run(["g++", "-shared", "-fopenmp", "-o", str(tmp), *map(str, objs), str(own), "-lm", "-ldl", "-lpthread"], check=True)
    os.replace(tmp, SO)
    own.unlink()
    return SO


@contextlib.contextmanager
def use_shim(**kwargs):
    """``shimlib.use_shim(**kwargs)`` with the library that has the transform and direct-solve entry points."""
    so = build()
    saved = shimlib.build
    shimlib.build = lambda force=False: so
    try:
        with shimlib.use_shim(**kwargs) as lib:
            yield lib
    finally:
        shimlib.build = saved


def load() -> C.CDLL:
    """The shim library itself, for calls on host arrays in the shim's own layout (``pdehip_layout`` of that library)."""
    return C.CDLL(str(build()))
