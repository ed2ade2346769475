"""What the two-step sweep runs, decided on a CPU: `py-pde_amd/csrc/pdehip_euler2_plan.h` through a tests-only probe.

The planner is plain host C++ (no HIP header); `tests/shim/euler2_plan_probe.cpp` exports it through `extern "C"` and g++ builds it here
in a second.  tests/test_hip_share_sizes.py pins the same decisions by reading `pdehip_last_kernel_name` after a run on the GPU; these are
the same facts before a GPU visit, plus the invariants of every accepted choice and a table of decisions recorded from the dispatcher
as it was before the planner existed (`tests/golden/e2_dispatch.json`, profiles/e2_dispatch_refactor.md).
"""

from __future__ import annotations

import ctypes as C
import json
import os
import random
import subprocess
from pathlib import Path
from types import SimpleNamespace

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "py-pde_amd" / "csrc" / "pdehip_euler2_plan.h"
PROBE = ROOT / "tests" / "shim" / "euler2_plan_probe.cpp"
BUILD = ROOT / "tests" / "shim" / "_build"
GOLDEN = ROOT / "tests" / "golden" / "e2_dispatch.json"

DIFFUSION, CH_EULER, CH_SCALED, CUSTOM, CUSTOM2, CH_STAGE, DIFFUSION_UNIT = range(7)
FAMILIES = ["euler2_kernel", "euler2_per_kernel", "euler2_peryz_kernel", "euler2_tall_kernel", "euler2_tall_per_kernel", "euler2_wide4_kernel", "euler2_stage1w_kernel"]
PLAIN, PER, PERYZ, TALL, TALL_PER, WIDE4, STAGE1W = range(7)
OUT = "accepted family elem vec ry m2 has_y ragged xs nt unit open_tail open_y ntz nty nxc xstride nblocks lx nwy nwz block per0 has_instance".split()
KNOBS = "ry blocks order off f32_vec f32_ry f32_svec f32_sry wide4_off stage_wide open_off open_y_off per3_off peryz_off minlx unit_off".split()
DEFAULT_KNOBS = dict.fromkeys(KNOBS, 0) | {"order": -1}
MIB = 1048576


@pytest.fixture(scope="module")
def lib():
    BUILD.mkdir(exist_ok=True)
    so = BUILD / "libe2plan_probe.so"
    if not so.exists() or so.stat().st_mtime < max(HEADER.stat().st_mtime, PROBE.stat().st_mtime):
        tmp = so.with_suffix(f".{os.getpid()}.tmp")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", str(PROBE), "-o", str(tmp)], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(str(so))
    lib.e2plan_instances.restype = C.c_int
    return lib


def ask(lib, elem, shape, per, xplain=0, ends=0, m2=DIFFUSION, plan=False, unit=True, alias=False, narrow=False, knobs=None):
    """The planner's choice for one query; `shape` has two (2-D: march axis, fastest axis) or three extents, `per` the class of each kernel axis."""
    ndim = len(shape)
    n0, n1, n2 = shape if ndim == 3 else (shape[0], 1, shape[1])
    q = (C.c_long * 15)(elem, ndim, n0, n1, n2, *per, xplain, ends, m2, plan, unit, alias, narrow)
    k = None if knobs is None else (C.c_long * 16)(*[(DEFAULT_KNOBS | knobs)[name] for name in KNOBS])
    out = (C.c_long * 24)()
    name = C.create_string_buffer(256)
    lib.e2plan_probe(q, k, out, name, 256)
    return SimpleNamespace(**dict(zip(OUT, out)), name=name.value.decode())


def instance(c):
    """The template-id of the instance a choice names, in the spelling of the recorded table: numbers for the enumerators and the flags."""
    T = "double" if c.elem == 8 else "float"
    m2 = DIFFUSION_UNIT if c.unit else c.m2
    if c.family == PLAIN:
        if c.m2 == CH_STAGE:
            return f"euler2_kernel<{T},{c.vec},{c.ry},5,{c.has_y},{c.ragged},0,0>"
        return f"euler2_kernel<{T},{c.vec},{c.ry},{m2},{c.has_y},{c.ragged},{c.xs},{c.nt}>"
    if c.family == TALL:
        return f"euler2_tall_kernel<{T},{c.vec},8,{m2},{c.nt}>"
    if c.family == STAGE1W:
        return f"euler2_stage1w_kernel<{T},{c.vec},2,1>"
    return f"{FAMILIES[c.family]}<{T},{c.vec},{m2},{c.nt}>"


def compiled(lib, elem, vec):
    buf = (C.c_long * (7 * 32))()
    n = lib.e2plan_instances(elem, vec, buf, 32)
    assert 0 < n <= 32
    return [tuple(buf[7 * i : 7 * i + 7]) for i in range(n)]


def in_compiled_list(lib, c):
    """Membership of a choice in the list the launcher instantiates its kernels from (family ry has_y ragged xs nt stage)."""
    for fam, ry, has_y, ragged, xs, nt, stage in compiled(lib, c.elem, c.vec):
        if fam != c.family:
            continue
        if fam != PLAIN:
            return True
        if (ry, has_y, ragged, xs, nt) == (c.ry, c.has_y, c.ragged, c.xs, c.nt) and c.m2 in (DIFFUSION, CH_EULER, CH_SCALED, CH_STAGE):
            return bool(stage) if c.m2 == CH_STAGE else True
    return False


def test_the_header_is_plain_host_code():
    """No HIP header, no device code: g++ compiles it on its own."""
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-"], input=f'#include "{HEADER}"\n', text=True, check=True)
    text = HEADER.read_text()
    assert "hip_runtime" not in text and "__device__" not in text and "__global__" not in text
    # the tuning knobs are read in one function of the header and nowhere in the launcher
    assert "getenv" not in (HEADER.parent / "pdehip_kernels_e2.hip").read_text()
    body = text.split("inline Knobs knobs_from_env()")[1].split("inline const Knobs &knobs()")[0]
    assert text.count("getenv(") == body.count("getenv(") > 0


def test_the_compiled_instance_lists(lib):
    """92 kernels in the code object of pdehip_kernels_e2.hip: a plain entry is diffusion (+ its unit form unless one-sided), two Cahn-Hilliard
    sweeps and, where flagged, the stage sweep; a ladder is unit x NT."""
    total = 0
    for elem, vec in ((8, 2), (4, 4), (4, 2)):
        for fam, ry, has_y, ragged, xs, nt, stage in compiled(lib, elem, vec):
            total += (3 + (not xs) + stage) if fam == PLAIN else (1 if fam == STAGE1W else 4)
    assert total == 92
    assert lib.e2plan_instances(8, 4, (C.c_long * 7)(), 1) == 0


# ---- what the dispatcher chooses at the share sizes -------------------------------------------------------------
@pytest.mark.parametrize("unit", [True, False])
@pytest.mark.parametrize("layers,nt,nxc,lx", [(60, 0, 3, 20), (56, 0, 3, 19), (124, 1, 4, 31), (120, 1, 4, 30), (252, 1, 4, 63), (248, 1, 4, 62), (256, 1, 4, 64)])
def test_interior_sweeps_of_the_shares(lib, layers, nt, nxc, lx, unit):
    """Halo planes on both sides, rows and fastest axis periodic: `euler2_peryz_kernel`; below 96 layers the thin rule (at most 1536 waves),
    from there the cost model; streaming stores beyond 192 MiB per launch."""
    c = ask(lib, 8, (layers, 512, 512), (0, 1, 1), xplain=1, unit=unit)
    assert c.accepted and c.has_instance and c.family == PERYZ and (c.ry, c.vec) == (4, 2)
    assert c.nt == nt == (layers * 512 * 512 * 8 > 192 * MIB)
    assert (c.nxc, c.lx, c.xstride) == (nxc, lx, lx) and (c.ntz, c.nty, c.nwz, c.nwy, c.block) == (4, 128, 4, 1, 256)
    assert c.nblocks == nxc * 128 and c.per0 == 2 and not c.open_tail and not c.open_y
    if layers < 96:
        assert c.nblocks * 4 <= 1536
    form = "E2_DIFFUSION_UNIT" if unit else "E2_DIFFUSION"
    assert c.name == (f"euler2_peryz_kernel<double,2,{form},{'NT' if nt else 'plain stores'}> (4 rows, 2 waves per SIMD, rows and fastest axis periodic, "
                      "halo planes along the march axis)")
    # the same with local faces on rows / fastest axis: the general 4-row tile
    f = ask(lib, 8, (layers, 512, 512), (0, 0, 0), xplain=1, unit=unit)
    assert f.accepted and f.has_instance and f.family == PLAIN and (f.ry, f.ragged, f.xs, f.nt) == (4, 0, 0, nt) and (f.nxc, f.lx) == (nxc, lx)
    assert f.name == f"euler2_kernel<double,2,4,m2=0{' unit' if unit else ''},3-D,aligned rows,two-sided,{'NT' if nt else 'plain stores'}>"


@pytest.mark.parametrize("n0,ends,nt", [(68, 8, 0), (64, 4, 0), (132, 8, 1), (128, 4, 1), (260, 8, 1), (256, 4, 1)])
def test_boundary_launches_of_the_shares(lib, n0, ends, nt):
    """`ends` = 8 / 4 of a range of n + 4 / n layers: two chunks of `ends` planes, the same bodies; the store form follows the RANGE."""
    for per, family in (((0, 1, 1), PERYZ), ((0, 0, 0), PLAIN)):
        c = ask(lib, 8, (n0, 512, 512), per, xplain=1, ends=ends)
        assert c.accepted and c.has_instance and c.family == family and c.ry == 4 and not c.ragged
        assert (c.nxc, c.lx, c.xstride, c.nblocks, c.block) == (2, ends, n0 - ends, 256, 256) and c.nt == nt


@pytest.mark.parametrize("per", [(0, 1, 1), (0, 0, 0)])
@pytest.mark.parametrize("shape", [(64, 513, 513), (64, 500, 300), (60, 513, 513), (56, 500, 300)])
def test_off_tile_shares(lib, shape, per):
    """Halo planes: no open rows / columns - moved last tiles, rows that end inside a chunk: the ragged two-sided 4-row tile, thin rule."""
    c = ask(lib, 8, shape, per, xplain=1)
    assert c.accepted and c.has_instance and c.family == PLAIN and (c.ry, c.ragged, c.xs, c.nt) == (4, 1, 0, 0) and not c.open_tail and not c.open_y
    assert c.name == "euler2_kernel<double,2,4,m2=0 unit,3-D,ragged,two-sided,plain stores>"
    assert c.nty == (shape[1] + 3) // 4 and c.ntz == (shape[2] + 127) // 128 and c.nblocks * c.block // 64 <= max(1536, c.ntz * c.nty)


@pytest.mark.parametrize("layers,family", [(64, PER), (128, PER), (256, TALL_PER)])
def test_shares_without_exchange(lib, layers, family):
    """Axis 0 wraps in the kernel: the all-periodic instances, 8-row tiles beyond 400 MiB; with faces the 4-row tile."""
    nt = int(layers * 512 * 512 * 8 > 192 * MIB)
    c = ask(lib, 8, (layers, 512, 512), (1, 1, 1))
    assert c.accepted and c.has_instance and c.family == family and c.nt == nt and c.ry == (8 if family == TALL_PER else 4) and c.unit
    assert c.name.startswith(FAMILIES[family] + "<double,2,E2_DIFFUSION_UNIT," + ("NT" if nt else "plain stores"))
    f = ask(lib, 8, (layers, 512, 512), (1, 0, 0), unit=False)
    assert f.accepted and f.family == PLAIN and (f.ry, f.ragged, f.xs, f.nt) == (4, 0, 0, nt)
    assert f.name == f"euler2_kernel<double,2,4,m2=0,3-D,aligned rows,two-sided,{'NT' if nt else 'plain stores'}>"


def test_fp32_share_and_physical_faces_and_boxes(lib):
    for layers in (56, 60, 64):   # the wide 2-row tile; the 4-row wide tile needs all three axes to wrap
        c = ask(lib, 4, (layers, 512, 512), (0, 1, 1), xplain=1)
        assert c.accepted and c.has_instance and c.family == PLAIN and (c.vec, c.ry, c.xs, c.nt) == (4, 2, 0, 0)
        assert c.name.startswith("euler2_kernel<float,4,2,") and "two-sided" in c.name and "plain stores" in c.name
        assert c.nblocks * c.block // 64 <= 1536
    # a rank with both physical faces of axis 0: the sweeps see the whole slab; 64 x 513 x 513: open rows and columns
    c = ask(lib, 8, (64, 512, 512), (0, 0, 0))
    assert c.name == "euler2_kernel<double,2,4,m2=0 unit,3-D,aligned rows,two-sided,plain stores>" and (c.nxc, c.lx) == (4, 16)
    c = ask(lib, 8, (64, 513, 513), (0, 0, 0))
    assert c.name == "euler2_kernel<double,2,4,m2=0 unit,3-D,ragged,two-sided,plain stores>" and (c.open_tail, c.open_y, c.ntz, c.nty, c.nxc, c.lx) == (1, 1, 4, 128, 4, 16)
    # boxes of the fast block loop: 7/8 of a round (14 chunks of 128 tiles = 1792 waves; a full round would be 16)
    for elem, per, grid, block in ((8, (0, 2, 1), 448, 256), (8, (0, 2, 2), 448, 256), (4, (0, 2, 1), 896, 128)):
        c = ask(lib, elem, (256, 128, 512), per, xplain=1, unit=False)
        assert c.accepted and c.has_instance and c.family == PLAIN and (c.nxc, c.lx, c.nblocks, c.block) == (14, 19, grid, block) and c.nblocks * block // 64 == 1792
    c = ask(lib, 8, (256, 256, 256), (0, 2, 2), xplain=1, unit=False)
    assert (c.ntz, c.nty, c.nxc, c.nblocks, c.block) == (2, 64, 14, 896, 128)


def test_the_bench_grid(lib):
    """512^3 all-periodic on a UnitGrid with D = 1: the names `bench.py` looks `roofline.traffic` up under (profiles/traffic.json)."""
    c = ask(lib, 8, (512, 512, 512), (1, 1, 1))
    assert c.accepted and c.has_instance and c.family == TALL_PER and (c.ry, c.nt, c.unit) == (8, 1, 1)
    assert c.name == "euler2_tall_per_kernel<double,2,E2_DIFFUSION_UNIT,NT> (8 rows, 3 plane buffers, 1 wave per SIMD, all-periodic)"
    assert (c.ntz, c.nty, c.nxc, c.lx, c.nblocks, c.block) == (4, 64, 4, 128, 256, 256)     # one round of 1024 waves at one wave per SIMD
    traffic = json.loads((ROOT / "profiles" / "traffic.json").read_text())
    assert c.name in json.dumps(traffic)
    c = ask(lib, 4, (512, 512, 512), (1, 1, 1))
    assert c.accepted and c.has_instance and c.family == WIDE4 and (c.vec, c.ry, c.nt) == (4, 4, 1)
    assert c.name == "euler2_wide4_kernel<float,4,E2_DIFFUSION_UNIT,NT> (4 rows, 1 wave per SIMD, all-periodic)"
    assert (c.ntz, c.nty, c.nxc, c.nblocks, c.block) == (2, 128, 4, 512, 128)


# ---- open rows / open columns of tiles, the values of the dispatcher before the planner existed -----------------
# n: (open_tail, open_y, nty, nxc, lx) of n^3
OPEN_F64_FACES = {511: (0, 0, 128, 4, 128), 512: (0, 0, 128, 4, 128), 513: (1, 1, 128, 4, 129), 514: (2, 2, 128, 4, 129), 515: (3, 3, 128, 4, 129), 516: (4, 0, 129, 6, 86),
                  517: (5, 0, 130, 7, 74), 518: (6, 0, 130, 7, 74), 519: (7, 0, 130, 6, 87)}
# the tall tile (8 rows, one wave per SIMD): up to seven rows, six two-layer jobs in all: 519 = 4 + 4 jobs has no open form
OPEN_F64_PERIODIC = {512: (0, 0, 64, 4, 128), 513: (1, 1, 64, 4, 129), 514: (2, 2, 64, 4, 129), 515: (3, 3, 64, 4, 129), 516: (4, 4, 64, 4, 129), 517: (5, 5, 64, 4, 130),
                     518: (6, 6, 64, 4, 130)}
OPEN_F32_PERIODIC = {511: (0, 0, 128, 4, 128), 513: (1, 1, 128, 4, 129), 514: (2, 2, 128, 4, 129), 515: (3, 3, 128, 4, 129), 516: (4, 0, 129, 6, 86), 517: (5, 0, 130, 7, 74),
                     518: (6, 0, 130, 7, 74), 519: (7, 0, 130, 6, 87)}


def test_open_rows_and_open_tile_columns(lib):
    for n, expect in OPEN_F64_FACES.items():
        c = ask(lib, 8, (n, n, n), (0, 0, 0))
        assert c.accepted and c.has_instance and c.family == PLAIN and c.ry == 4 and c.nt, n
        assert (c.open_tail, c.open_y, c.nty, c.nxc, c.lx) == expect and c.ntz == 4, n
        # the virtual FAR column of one open column and the virtual row next to a moved last tile are part of the ragged-row code
        assert c.ragged == (n == 513 or (n - c.open_y) % 4 != 0), n
    for n, expect in OPEN_F64_PERIODIC.items():
        c = ask(lib, 8, (n, n, n), (1, 1, 1))
        assert c.accepted and c.has_instance and c.family == TALL_PER and c.ry == 8 and (c.open_tail, c.open_y, c.nty, c.nxc, c.lx) == expect, n
        assert (c.nblocks, c.block) == (256, 256), n
    for n, family, open_, nty in ((511, PER, (0, 0), 128), (519, PER, (7, 0), 130)):     # no multiple of eight within reach: the 4-row tile, moved
        c = ask(lib, 8, (n, n, n), (1, 1, 1))
        assert c.family == family and not c.ragged and (c.open_tail, c.open_y) == open_ and c.nty == nty and c.ry == 4
    for n, expect in OPEN_F32_PERIODIC.items():
        c = ask(lib, 4, (n, n, n), (1, 1, 1))
        assert c.accepted and c.has_instance and c.family == WIDE4 and (c.vec, c.ry) == (4, 4) and (c.open_tail, c.open_y, c.nty, c.nxc, c.lx) == expect, n
    # only where the fill gain exceeds 0.08: 300 x 513 x 640 (five chunks per row) keeps the moved tile; 512 x 517 x 512 opens five rows under the tall tile only
    for per, family in (((0, 0, 0), PLAIN), ((1, 1, 1), PER)):
        c = ask(lib, 8, (300, 513, 640), per)
        assert c.family == family and (c.open_tail, c.open_y, c.ntz, c.nty, c.nxc, c.lx, c.nblocks, c.block) == (0, 0, 5, 129, 5, 60, 3225, 64)
    c = ask(lib, 8, (512, 517, 512), (1, 1, 1))
    assert c.family == TALL_PER and (c.open_tail, c.open_y, c.nty) == (0, 5, 64)
    c = ask(lib, 8, (512, 517, 512), (0, 0, 0))
    assert c.family == PLAIN and c.ragged and (c.open_tail, c.open_y, c.nty, c.nxc, c.lx) == (0, 0, 130, 6, 86)
    c = ask(lib, 8, (512, 513, 512), (0, 0, 0))
    assert c.family == PLAIN and not c.ragged and (c.open_tail, c.open_y, c.nty) == (0, 1, 128)
    # the switches
    assert ask(lib, 8, (513, 513, 513), (0, 0, 0), knobs={"open_y_off": 1}).open_y == 0
    c = ask(lib, 8, (513, 513, 513), (0, 0, 0), knobs={"open_off": 1})
    assert (c.open_tail, c.open_y, c.ntz) == (0, 0, 5)
    # never with halo planes, slab ends, boxes or another right-hand side
    for kw in ({"xplain": 1}, {"m2": CH_EULER}, {"plan": True}):
        c = ask(lib, 8, (513, 513, 513), (0, 0, 0), **kw)
        assert c.accepted and (c.open_tail, c.open_y) == (0, 0), kw


def test_knobs(lib, monkeypatch):
    for name in ("PDEHIP_EULER2", "PDEHIP_F32_TILE", "PDEHIP_F32_WIDE4", "PDEHIP_F32_STAGE_WIDE", "PDEHIP_OPEN_ROWS", "PDEHIP_OPEN_Y", "PDEHIP_E2_PER3", "PDEHIP_E2_PERYZ",
                 "PDEHIP_E2_MINLX", "PDEHIP_NO_UNIT"):
        monkeypatch.delenv(name, raising=False)
    k = (C.c_long * 16)()
    lib.e2plan_knobs_from_env(k)
    assert dict(zip(KNOBS, k)) == DEFAULT_KNOBS
    for name, value in (("PDEHIP_EULER2", "8,1024,12"), ("PDEHIP_F32_TILE", "2,4,4,1"), ("PDEHIP_F32_WIDE4", "0"), ("PDEHIP_F32_STAGE_WIDE", "1"), ("PDEHIP_OPEN_ROWS", "0"),
                        ("PDEHIP_OPEN_Y", "0"), ("PDEHIP_E2_PER3", "0"), ("PDEHIP_E2_PERYZ", "0"), ("PDEHIP_E2_MINLX", "8"), ("PDEHIP_NO_UNIT", "1")):
        monkeypatch.setenv(name, value)
    lib.e2plan_knobs_from_env(k)
    assert list(k) == [8, 1024, 12, 0, 2, 4, 4, 1, 1, 1, 1, 1, 1, 1, 8, 1]
    monkeypatch.setenv("PDEHIP_EULER2", "off")
    lib.e2plan_knobs_from_env(k)
    assert k[3] == 1
    # what they select
    c = ask(lib, 8, (256, 256, 256), (0, 0, 0), knobs={"ry": 8})
    assert c.family == TALL and c.name == "euler2_tall_kernel<double,2,8,E2_DIFFUSION_UNIT,plain stores> (8 rows, 4 plane buffers, 1 wave per SIMD)"
    assert ask(lib, 8, (512, 512, 512), (1, 1, 1), knobs={"per3_off": 1}).family == PLAIN
    assert ask(lib, 8, (60, 512, 512), (0, 1, 1), xplain=1, knobs={"peryz_off": 1}).family == PLAIN
    assert ask(lib, 4, (512, 512, 512), (1, 1, 1), knobs={"wide4_off": 1}).ry == 2
    c = ask(lib, 4, (64, 256, 256), (1, 1, 1), m2=CH_STAGE, knobs={"stage_wide": 1})
    assert c.accepted and c.family == STAGE1W and c.name == "" and c.nblocks * c.block // 64 <= 1024
    assert not ask(lib, 8, (512, 512, 512), (0, 0, 0), knobs={"unit_off": 1}).unit
    assert ask(lib, 8, (100, 100, 100), (0, 0, 0), knobs={"minlx": 25}).lx == 25


# ---- invariants of every accepted choice ---------------------------------------------------------------------------------------------
EXTENTS = [4, 5, 7, 8, 9, 12, 13, 16, 31, 32, 33, 60, 64, 65, 96, 100, 127, 128, 129, 130, 136, 200, 255, 256, 257, 260, 264, 300, 384, 385, 500, 512, 513, 514, 516, 517, 519, 520, 640, 1024]


def test_invariants_over_a_sweep(lib):
    rng = random.Random(20261016)
    accepted = asked = 0
    families = set()
    quirk = 0
    for _ in range(2500):
        ndim = 3 if rng.random() < 0.85 else 2
        shape = tuple(rng.choice(EXTENTS) for _ in range(ndim))
        faces = (rng.choice((0, 1)), rng.choice((0, 1, 1, 2)) if ndim == 3 else 1, rng.choice((0, 1, 1, 2)) if ndim == 3 else rng.choice((0, 1)))
        if rng.random() < 0.25:
            faces = (1, 1, 1)
        for elem, narrow in ((8, False), (4, False), (4, True)):
            for xplain in ((0, 1, 2, 3) if ndim == 3 else (0,)):
                for ends in (0, rng.choice((2, 4, 8))):
                    for m2 in (DIFFUSION, CH_EULER, CH_SCALED, CH_STAGE, CUSTOM, CUSTOM2):
                        if ends > shape[0]:
                            continue
                        per = (0 if xplain else faces[0], faces[1], faces[2])
                        plan = m2 in (CUSTOM, CUSTOM2)
                        alias = m2 == CH_STAGE and rng.random() < 0.3
                        c = ask(lib, elem, shape, per, xplain=xplain, ends=ends, m2=m2, plan=plan, unit=rng.random() < 0.5, alias=alias, narrow=narrow)
                        asked += 1
                        if not c.accepted:
                            continue
                        accepted += 1
                        families.add(c.family)
                        n0, n1, n2 = shape if ndim == 3 else (shape[0], 1, shape[1])
                        ctx = (elem, shape, per, xplain, ends, m2, narrow, vars(c))
                        cw = 64 * c.vec
                        n1t, n2t = n1 - c.open_y, n2 - c.open_tail
                        # the tiles cover the rows and the columns that are not left open ...
                        assert c.ntz * cw >= n2t > (c.ntz - 1) * cw and c.nty * c.ry >= n1t > (c.nty - 1) * c.ry, ctx
                        # ... and the chunks the march axis (a boundary sweep: the first and the last `ends` planes)
                        if ends:
                            assert (c.nxc, c.lx, c.xstride) == (2, ends, n0 - ends), ctx
                        else:
                            assert c.nxc * c.lx >= n0 > (c.nxc - 1) * c.lx and c.xstride == c.lx, ctx
                        waves = c.nxc * c.ntz * c.nty
                        assert c.block == 64 * c.nwz * c.nwy and c.nwz in (1, 2, 4) and c.nwy == 1 and c.ntz % c.nwz == 0, ctx
                        assert c.nblocks * (c.block // 64) == waves and c.nblocks < 2**31, ctx
                        # where a cap bounds the waves of a sweep (the thin rule of slabs below 96 layers, 2-D grids) it holds unless one chunk already exceeds it
                        if ndim == 3 and xplain and n0 < 96 and not ends:
                            assert waves <= max(1536, c.ntz * c.nty), ctx
                        if ndim == 2:
                            assert waves <= max(4096, c.ntz * c.nty), ctx
                        # a last tile that is moved back reads real rows (periodic rows, boxes) or belongs to the ragged-row code
                        assert c.ry in (1, 2, 4, 8) and (n1t % c.ry == 0 or c.ragged or per[1] != 0), ctx
                        assert c.has_y == (ndim == 3) and c.xs == (xplain > 1) and c.per0 == ((0, 2, 3, 4)[xplain] if xplain else per[0]), ctx
                        assert c.open_tail <= 8 and c.open_y <= 7 and (c.open_tail + 1) // 2 + (c.open_y + 1) // 2 <= 6, ctx     # six two-layer jobs
                        if plan:
                            assert c.ry == (1 if ndim == 2 else c.ry) and c.ry in (1, 2, 4), ctx
                            continue
                        assert c.unit <= (m2 == DIFFUSION) and c.nt <= (elem * n0 * n1 * n2 > 192 * MIB), ctx
                        # the choice is one of the compiled instances.  One exception, kept as the dispatcher had it (profiles/e2_dispatch_refactor.md): an fp64 stage
                        # sweep whose rows make the 4-row tile ragged answers "covered" to a dry run and is declined by the launch (no instance)
                        if in_compiled_list(lib, c):
                            assert c.has_instance, ctx
                        else:
                            assert not c.has_instance and (elem, m2, c.family, c.ry, c.ragged, per[1]) == (8, CH_STAGE, PLAIN, 4, 1, 0) and n1t % 4 != 0 and (n2 + 1) // 2 * 2 % 128 == 0, ctx
                            quirk += 1
    assert asked > 150000 and accepted > 60000 and {PLAIN, PER, PERYZ, TALL_PER, WIDE4} <= families
    assert quirk > 0


# ---- the decisions of the dispatcher before the planner existed ----------------------------------------------------------------------
def test_recorded_decisions(lib):
    """`tests/golden/e2_dispatch.json`: every shape named in DESIGN.md sections 5 and 7 and in the GPU tests of the sweep, and a seeded sample, as
    `launch_euler2_tv` / `launch_euler2_t` decided them at the commit before this file (recorded with the launch replaced by a recorder:
    profiles/e2_dispatch_refactor.md).  Row: elem ndim n0 n1 n2 per0 per1 per2 xplain ends m2 plan unit alias narrow | dry-run answer, launch / plan answer,
    instance, name, grid, block, ntz nty lx nxc xstride nwy z_open per[0], columns and rows handed to shell_open_rows, rows of a planned tile."""
    table = json.loads(GOLDEN.read_text())
    kernels, names = table["kernels"], table["names"]
    assert len(table["cases"]) > 2000
    launched = 0
    for row in table["cases"]:
        elem, ndim, n0, n1, n2, p0, p1, p2, xplain, ends, m2, plan, unit, alias, narrow = row[:15]
        dry, done, kern, name, grid, block, ntz, nty, lx, nxc, xstride, nwy, z_open, per0, cols, rows, plan_ry = row[15:]
        c = ask(lib, elem, (n0, n1, n2) if ndim == 3 else (n0, n2), (p0, p1, p2), xplain=xplain, ends=ends, m2=m2, plan=bool(plan), unit=bool(unit), alias=bool(alias), narrow=bool(narrow))
        assert c.accepted == dry, row
        assert (c.accepted and (plan or c.has_instance)) == done, row
        if not done:
            continue
        assert (c.nblocks, c.block, c.ntz, c.nty, c.lx, c.nxc, c.xstride, c.nwy, int(c.open_tail > 0), c.per0) == (grid, block, ntz, nty, lx, nxc, xstride, nwy, z_open, per0), row
        if plan:
            assert c.ry == plan_ry, row
            continue
        launched += 1
        assert instance(c) == kernels[kern] and c.name == names[name] and (c.open_tail, c.open_y) == (cols, rows), (row, instance(c), c.name)
    assert launched > 1500
