"""The gate of the four-step sweep, decided on a CPU: `py-pde_amd/csrc/pdehip_euler4_plan.h` through a tests-only probe
(`tests/shim/euler4_plan_probe.cpp`, built by g++ here), like tests/test_euler2_plan.py for the two-step planner."""

from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path
from types import SimpleNamespace

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "py-pde_amd" / "csrc" / "pdehip_euler4_plan.h"
PROBE = ROOT / "tests" / "shim" / "euler4_plan_probe.cpp"
BUILD = ROOT / "tests" / "shim" / "_build"
OUT = "accepted unit nty ntz nxc nblocks lx block".split()
P3 = (1, 1, 1)


@pytest.fixture(scope="module")
def lib():
    BUILD.mkdir(exist_ok=True)
    so = BUILD / "libe4plan_probe.so"
    if not so.exists() or so.stat().st_mtime < max(HEADER.stat().st_mtime, PROBE.stat().st_mtime):
        tmp = so.with_suffix(f".{os.getpid()}.tmp")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", str(PROBE), "-o", str(tmp)], check=True)
        os.replace(tmp, so)
    return C.CDLL(str(so))


def ask(lib, shape, per=P3, elem=8, diffusion=True, const_faces=True, unit=True, knob=-1):
    ndim = len(shape)
    n0, n1, n2 = shape if ndim == 3 else (shape[0], 1, shape[1])
    q = (C.c_long * 12)(elem, ndim, n0, n1, n2, *per, diffusion, const_faces, unit, knob)
    out = (C.c_long * 8)()
    name = C.create_string_buffer(192)
    lib.e4plan_probe(q, out, name, 192)
    return SimpleNamespace(**dict(zip(OUT, out)), name=name.value.decode())


def geometry(lib):
    out = (C.c_long * 7)()
    lib.e4plan_geometry(out)
    return SimpleNamespace(**dict(zip("TY TZ PY HALO MIN_CHUNK THREADS LDS_BYTES".split(), out)))


def test_the_header_is_plain_host_code():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-"], input=f'#include "{HEADER}"\n', text=True, check=True)
    text = HEADER.read_text()
    assert "hip_runtime" not in text and "__device__" not in text and "__global__" not in text


def test_default_gate(lib):
    """The table of the default gate: the benchmark's 512^3 runs the four-step sweep, 256 x 512 x 512 (beyond 400 MiB, where the tall
    two-step tile starts) and the cache-resident 256^3 do not; faces, programs of conditions and array faces never do."""
    c = ask(lib, (512, 512, 512))
    assert c.accepted and c.unit
    assert c.name == "euler4_kernel<double,E2_DIFFUSION_UNIT> (32x64 tile, 4 levels in LDS, all-periodic)"
    assert (c.nty, c.ntz, c.nxc, c.lx, c.nblocks) == (16, 8, 2, 256, 256)   # one whole round of the 256 CUs
    assert ask(lib, (512, 512, 512), unit=False).name == "euler4_kernel<double,E2_DIFFUSION> (32x64 tile, 4 levels in LDS, all-periodic)"
    assert not ask(lib, (256, 512, 512)).accepted
    assert not ask(lib, (256, 256, 256)).accepted
    assert not ask(lib, (224, 512, 512), per=(1, 0, 0)).accepted          # local faces on the rows and the fastest axis
    assert not ask(lib, (224, 512, 512), per=(0, 0, 0), knob=1).accepted
    assert not ask(lib, (512, 512, 512), const_faces=False).accepted
    assert not ask(lib, (512, 512, 512), diffusion=False).accepted
    assert not ask(lib, (512, 512, 512), knob=0).accepted
    assert not ask(lib, (512, 512, 512), elem=4).accepted


def test_forced_gate(lib):
    """PDEHIP_EULER4=1: any size the tile rules admit - rows a multiple of TY, columns of TZ, 2 * HALO + MIN_CHUNK planes - and nothing else."""
    g = geometry(lib)
    assert (g.TY, g.TZ, g.HALO) == (32, 64, 4) and g.THREADS % 64 == 0 and g.THREADS <= 1024 and g.LDS_BYTES <= 160 * 1024
    nmin = 2 * g.HALO + g.MIN_CHUNK
    for shape in ((256, 256, 256), (256, 512, 512), (nmin, g.TY, g.TZ), (nmin + 1, 2 * g.TY, 2 * g.TZ), (40, 3 * g.TY, g.TZ)):
        c = ask(lib, shape, knob=1)
        assert c.accepted and c.nty * g.TY == shape[1] and c.ntz * g.TZ == shape[2], shape
        assert c.nblocks == c.nxc * c.nty * c.ntz and c.block == g.THREADS
        assert (c.nxc - 1) * c.lx < shape[0] <= c.nxc * c.lx and c.lx >= g.MIN_CHUNK, shape      # chunks cover the planes, none empty
    for shape, per, kw in (((nmin - 1, 32, 64), P3, {}), ((64, 48, 64), P3, {}), ((64, 32, 96), P3, {}), ((64, 16, 64), P3, {}),
                           ((64, 64), (1, 1, 1), {}), ((64, 32, 64), (1, 1, 0), {}), ((64, 32, 64), (0, 1, 1), {}), ((64, 32, 64), P3, {"elem": 4}),
                           ((64, 32, 64), P3, {"const_faces": False})):
        assert not ask(lib, shape, per=per, knob=1, **kw).accepted, (shape, per, kw)


def test_x_chunks(lib):
    """One chunk below 32 planes, two from 32 on (chunks of 16 planes at least); enough tiles for the 256 CUs: one chunk."""
    assert [ask(lib, (n0, 32, 64), knob=1).nxc for n0 in (16, 17, 31, 32, 33, 48)] == [1, 1, 1, 2, 2, 3]
    c = ask(lib, (33, 32, 64), knob=1)
    assert (c.nxc, c.lx) == (2, 17)
    assert ask(lib, (64, 512, 1024), knob=1).nxc == 1


def test_the_knob_is_read_at_every_call(lib, monkeypatch):
    for value, want in (("0", 0), ("1", 1), (None, -1), ("", -1)):
        if value is None:
            monkeypatch.delenv("PDEHIP_EULER4", raising=False)
        else:
            monkeypatch.setenv("PDEHIP_EULER4", value)
        assert lib.e4plan_knob() == want
