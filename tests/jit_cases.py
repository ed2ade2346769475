"""Cases, planner restatement and references for the run-time built one-level kernels (``csrc/pdehip_jit.hip``: ``lap_march_body<T, VEC, RY, CZ,
WY, 1, LAP_CUSTOM, HASX, true, IBC, TAILS>`` around a generated epilogue, optionally with the stage epilogue, and the one-cell-per-thread
``generic`` kernel).

Shared by ``tests/test_jit_cases_cpu.py`` (CPU: the restated planner against ``csrc/pdehip_jit_plan.h`` through a probe, the references against a
``np.longdouble`` restatement, and the conditions that keep a case from being vacuous) and ``tests/test_hip_jit_instances.py`` (GPU: every case
through the C ABI).  Nothing here touches a device.

**Planner.**  `plan` restates ``jitplan::plan`` and `kernel_name` restates ``jitplan::format_name``; every case of the table states the instance
it was written for (`Case.claim`) and the CPU module asserts that the restatement AND the header give that instance.

**References.**  None comes from the code under test.

* fp64: the tests-only host shim (``tests/shim/pdehip_shim.c``): the oracle's stencils, the epilogue compiled by gcc without contraction, the
  oracle's ``lincomb`` / ``rk4_combine`` / ``rkf45_combine`` / ``euler_adaptive_combine`` behind ``pdehip_jit_apply_stage``.  Equal bits.
* fp32: the kernel widens every stored value to fp64, evaluates stencil and epilogue in fp64 registers and rounds ONCE at the store; a virtual
  cell of an on-the-fly face is rounded to fp32 first (``pdehip_march.inc``).  The shim's fp32 path rounds between operator and epilogue, so the
  reference is the "fp64 twin": ghost cells by the oracle in fp32, the whole array widened exactly, the fp64 shim with ``in_faces = NULL``, the
  slope rounded once to fp32, and for stages the oracle's fp32 combination of that rounded slope (the stage epilogue reads the slope "as stored",
  ``pdehip_march.inc``).  Every step is the arithmetic the kernel documents, so the expectation is equal bits and no tolerance is used.

The epilogues use +, -, * only: no library function whose last bit may differ between gcc's libm and the device's.

**What a case compares** (``tests/test_hip_jit_instances.py``): the whole allocation of every array of the call.  Written cells against the
reference, everything else against the upload pattern `small_kernel_cases.pattern` (values of magnitude >= 1024 against fields of magnitude
<= 2: a store behind the row end or into a ghost cell cannot go unnoticed, see `pattern_is_far`).
"""

from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import small_kernel_cases as S

from oracle import pde_oracle as O
from pde_hip import _abi

# ---- the planner, restated (csrc/pdehip_jit_plan.h) -------------------------------------------------------------------------------
NO_KNOBS = {"ry": 0, "cz": 0, "wy": 0, "blocks": 0}
WORKER_KNOBS = {"ry": 4, "cz": 0, "wy": 2, "blocks": 64}      # PDEHIP_JIT_RY=4 PDEHIP_JIT_WY=2 PDEHIP_JIT_BLOCKS=64


def _ceil(a, b):
    return -(-a // b)


def plan(shape, dtype, *, aligned=True, stage=False, kind=0, nk=0, fused=False, knobs=None):
    """What ``jit_apply_impl`` launches for a grid: ``nk`` counts the earlier slopes of a stage up to two (kind 5 always has two)."""
    t = NO_KNOBS | (knobs or {})
    elem = np.dtype(dtype).itemsize
    nd = len(shape)
    n0, n1, n2 = (1,) * (3 - nd) + tuple(shape)
    c = SimpleNamespace(generic=False, elem=elem, vec=1, ry=1, cz=1, wy=1, hasx=False, ibc=False, stage=False, tails=False, ntz=0, nty=0, lx=1, nxc=1,
                        nblocks=0, threads=256)
    if nd < 2 or not aligned:
        c.generic = True
        c.nblocks = min(8192, max(1, _ceil(n0 * n1 * n2, 256)))
        return c
    vec = c.vec = 2 if elem == 8 else 4
    chunk = 64 * vec
    chunks = _ceil(n2, chunk)
    cz = 4 if chunks >= 4 else (2 if chunks >= 2 else 1)
    ry = 1 if stage else 2
    if t["ry"] > 0:
        ry = t["ry"]
    if 0 < t["cz"] <= cz:
        cz = t["cz"]

    def n_tiles(cz_):
        per_plane = _ceil(n1, ry) * _ceil(n2, chunk * cz_)
        return per_plane * n0 if nd == 3 else per_plane

    while cz > 1 and n_tiles(cz) < 512:
        cz //= 2
    wy = c.wy = t["wy"] if (stage and t["wy"] > 0) else 1
    c.ry, c.cz, c.hasx, c.ibc, c.stage = ry, cz, nd == 3, bool(fused), bool(stage)
    c.tails = n2 % vec != 0 or chunks % cz != 0
    c.ntz, c.nty = _ceil(n2, chunk * cz), _ceil(n1, wy * ry)
    tiles = c.ntz * c.nty
    lx = n0
    if c.hasx:
        want = t["blocks"] if t["blocks"] > 0 else (2048 if stage and (kind == 1 or nk < 2) else 1024)
        nxc = min(max(_ceil(want // wy, tiles), 1), n0)
        lx = _ceil(n0, nxc)
    c.lx, c.nxc = lx, _ceil(n0, lx)
    c.nblocks, c.threads = c.nxc * tiles, 64 * wy
    return c


def kernel_name(c):
    """``pdehip_last_kernel_name`` after the launch of a choice."""
    T = "double" if c.elem == 8 else "float"
    if c.generic:
        return f"pde_kernel<generic,{T}> (run-time built)"
    return (f"pde_kernel<{T},{c.vec},RY={c.ry},CZ={c.cz},WY={c.wy},{'3-D' if c.hasx else '2-D'},{'ibc' if c.ibc else '-'},{'stage' if c.stage else '-'},"
            f"{'tails' if c.tails else '-'}> (lx={c.lx}, {c.nxc} x-chunk{'' if c.nxc == 1 else 's'}; run-time built)")


def tails_kind(shape, dtype, c):
    """"" / "vector" (the row ends inside a lane's vector) / "idle" (chunks of the last tile beyond the row)"""
    if c.generic or not c.tails:
        return ""
    return "vector" if shape[-1] % c.vec else "idle"


PROBE_OUT = "generic elem vec ry cz wy hasx ibc stage tails ntz nty lx nxc nblocks".split()


def probe(lib, shape, dtype, *, aligned=True, stage=False, kind=0, nk=0, fused=False, knobs=None):
    """The same question asked of the header (``tests/shim/jit_plan_probe.cpp``): (fields as a dict, name)."""
    nd = len(shape)
    n = (1,) * (3 - nd) + tuple(shape)
    q = (C.c_long * 10)(np.dtype(dtype).itemsize, nd, *n, aligned, stage, kind, nk, fused)
    k = None if knobs is None else (C.c_long * 4)(*[(NO_KNOBS | knobs)[key] for key in ("ry", "cz", "wy", "blocks")])
    out = (C.c_long * 15)()
    name = C.create_string_buffer(256)
    lib.jitplan_probe.restype = C.c_long
    threads = lib.jitplan_probe(q, k, out, name, 256)
    return dict(zip(PROBE_OUT, out)) | {"threads": threads}, name.value.decode()


def as_dict(c):
    return {k: int(getattr(c, k)) for k in PROBE_OUT} | {"threads": c.threads}


# ---- epilogues: statements of pde_epilogue(c, lap, gsq, e0, e1, e2, p, d); p[0] scales the result (dt of a stage) --------------------
BODIES = {
    "allen_cahn": ("return p[0] * (p[1] * lap + c - c * c * c);", 2, 0),
    "kpz": ("return p[0] * (p[1] * lap + p[2] * gsq);", 3, 0),
    "axes": ("return p[0] * (d.d1[0] + 2.0 * d.d1[1] + 3.0 * d.d1[2] + 0.5 * d.d2[0] + 0.25 * d.d2[1] + 0.125 * d.d2[2] + d.gr[0] * d.gr[1] + d.gr[2] * c);", 1, 0),
    "extras": ("return p[0] * (p[11] * lap + p[3] * e0 + p[7] * e1 * c + p[10] * e2 - p[5] * gsq);", 12, 3),
}
# the two-level sweeps (pdehip_jit_euler2: the Euler update of a one-pass expression applied twice; pdehip_jit_fused2: tmp = f1(u), out = f2(tmp; e0 = u))
TWO_BODIES = {
    "euler_update": ("return c + p[0] * (p[1] * lap + c - c * c * c + p[2] * gsq);", 3, 0),
    "chain_first": ("return p[0] * (c * c * c - c - p[1] * lap);", 3, 0),
    "chain_second": ("return e0 + p[0] * (lap + p[2] * gsq);", 3, 1),
}
ALL_BODIES = BODIES | TWO_BODIES
PARAMS = np.array([0.05, 0.7, -0.3, 1.3, 99.0, 0.45, 98.0, -0.8, 97.0, 96.0, 0.6, 0.9])   # slots 4, 6, 8, 9 are read by no body
DX = (0.5, 0.8, 1.25)     # three different spacings: a swapped gs[] / dd1[] / dd2[] axis changes the result


def body_longdouble(body, c, lap, gsq, e, p, d1, d2, gr):
    """The four epilogues once more, in np.longdouble (the CPU module ties the references to it)."""
    L = np.longdouble
    p = [L(v) for v in p]
    if body == "allen_cahn":
        return p[0] * (p[1] * lap + c - c * c * c)
    if body == "kpz":
        return p[0] * (p[1] * lap + p[2] * gsq)
    if body == "axes":
        return p[0] * (d1[0] + 2 * d1[1] + 3 * d1[2] + L(0.5) * d2[0] + L(0.25) * d2[1] + L(0.125) * d2[2] + gr[0] * gr[1] + gr[2] * c)
    return p[0] * (p[11] * lap + p[3] * e[0] + p[7] * e[1] * c + p[10] * e[2] - p[5] * gsq)


# ---- faces ------------------------------------------------------------------------------------------------------------------------
FACES = ("preset", "periodic", "walls", "order2")
# (const, factor) of ghost = const + factor * edge cell, per normalised axis and side: value / derivative / mixed conditions
_WALLS = {0: ((0.6, -1.0), (-0.16, 1.0)), 1: ((0.15, 0.7), (-0.8, -1.0)), 2: ((0.625, 1.0), (-0.25, 0.6))}


def face_list(shape, faces):
    """The faces of a case as `small_kernel_cases.face_table` takes them (None: ``in_faces = NULL``, ghost cells preset periodically)."""
    nd = len(shape)
    out = []
    for a in range(nd):
        n = shape[a]
        for side in (0, 1):
            if faces in ("preset", "periodic"):
                out.append({"kind": _abi.BC_ORDER1, "flags": 0, "index1": n - 1 if side == 0 else 0, "index2": 0, "c": 0.0, "f1": 1.0, "f2": 0.0})
            else:
                c, f = _WALLS[3 - nd + a][side]
                out.append({"kind": _abi.BC_ORDER1, "flags": 0, "index1": 0 if side == 0 else n - 1, "index2": 0, "c": c, "f1": f, "f2": 0.0})
    if faces == "order2":      # the lower face of the rows' axis extrapolates: it goes through the ghost-cell kernel, the others stay fused
        a = nd - 2
        out[2 * a] = {"kind": _abi.BC_ORDER2, "flags": 0, "index1": 0, "index2": 1, "c": 0.1, "f1": 2.0, "f2": -1.0}
    return out


def rest_faces(shape, faces, generic):
    """The faces ``launch_ghosts`` applies (the others: SKIP): second-order ones, and every face when the generic kernel runs in 2-D / 3-D."""
    fl = face_list(shape, faces)
    skip = {"kind": _abi.BC_SKIP, "flags": 0, "index1": 0, "index2": 0, "c": 0.0, "f1": 0.0, "f2": 0.0}
    return [f if (generic or f["kind"] == _abi.BC_ORDER2) else skip for f in fl]


# ---- the table ----------------------------------------------------------------------------------------------------------------------
class Case(SimpleNamespace):
    @property
    def id(self):
        st = "" if self.stage is None else f"-kind{self.stage['kind']}" + (f"nk{self.stage['nk']}" if self.stage["kind"] == 0 else "") + \
            ("-inplace" if self.stage.get("alias") else "")
        return f"{self.what}-{np.dtype(self.dtype).name}-{'x'.join(map(str, self.shape))}-{self.faces}-{self.body}{st}{'-special' if self.special else ''}" + \
            (f"-shift-{self.shift}" if self.shift else "")


def _case(what, dtype, shape, faces, body, claim, stage=None, special=False, shift=None):
    return Case(what=what, dtype=np.dtype(dtype), shape=tuple(shape), faces=faces, body=body, claim=claim, stage=stage, special=special, shift=shift)


def _claim(ry, cz, tails, lx, nxc):
    return {"ry": ry, "cz": cz, "tails": tails, "lx": lx, "nxc": nxc}


K0 = lambda nk: {"kind": 0, "nk": nk}                       # noqa: E731
K1, K1Y = {"kind": 1, "nk": 3}, {"kind": 1, "nk": 3, "alias": "out2=y"}
K2 = {"kind": 2, "nk": 4}
K4, K4IN = {"kind": 4, "nk": 2}, {"kind": 4, "nk": 2, "alias": "k1=in"}
COEF = (0.11, -0.23, 0.37, 0.41, -0.53)
C_NEW = 0.67
DT4 = 0.07


def cases():
    f8, f4 = "float64", "float32"
    t = []
    # -- slope sweeps (RY = 2), fp64: chunk = 128 cells
    t += [_case("cz1", f8, (8, 6, 128), "preset", "allen_cahn", _claim(2, 1, "", 1, 8)),
          _case("cz1", f8, (8, 6, 128), "walls", "extras", _claim(2, 1, "", 1, 8)),
          _case("cz1-tails-odd-rows", f8, (8, 5, 127), "walls", "axes", _claim(2, 1, "vector", 1, 8), special=True),
          _case("cz2", f8, (32, 32, 192), "periodic", "kpz", _claim(2, 2, "", 1, 32)),
          _case("cz2", f8, (32, 32, 130), "preset", "axes", _claim(2, 2, "", 1, 32)),
          _case("cz2-2d", f8, (1024, 130), "walls", "allen_cahn", _claim(2, 2, "", 1, 1)),
          _case("cz2-tails", f8, (32, 32, 131), "walls", "kpz", _claim(2, 2, "vector", 1, 32), special=True),
          _case("cz2-tails", f8, (32, 32, 131), "preset", "extras", _claim(2, 2, "vector", 1, 32)),
          _case("cz4", f8, (32, 32, 512), "order2", "allen_cahn", _claim(2, 4, "", 1, 32)),
          _case("cz4-2d", f8, (1024, 386), "periodic", "axes", _claim(2, 4, "", 1, 1)),
          _case("cz4-tails", f8, (32, 32, 385), "walls", "extras", _claim(2, 4, "vector", 1, 32), special=True),
          _case("cz4-idle", f8, (32, 32, 640), "walls", "axes", _claim(2, 4, "idle", 1, 32)),
          _case("cz4-idle", f8, (32, 32, 640), "preset", "allen_cahn", _claim(2, 4, "idle", 1, 32)),
          _case("lx2-full", f8, (40, 64, 64), "walls", "kpz", _claim(2, 1, "", 2, 20)),
          _case("lx2-short", f8, (37, 64, 128), "walls", "allen_cahn", _claim(2, 1, "", 2, 19), special=True),
          _case("lx3-one-plane", f8, (40, 128, 64), "walls", "axes", _claim(2, 1, "", 3, 14)),
          _case("lx3-one-plane", f8, (40, 128, 64), "preset", "kpz", _claim(2, 1, "", 3, 14)),
          _case("lx2-swizzle-remainder", f8, (37, 62, 128), "order2", "extras", _claim(2, 1, "", 2, 19))]
    # -- stage sweeps (RY = 1), fp64
    t += [_case("stage-cz4", f8, (16, 32, 512), "walls", "allen_cahn", _claim(1, 4, "", 1, 16), K0(5)),
          _case("stage-cz4", f8, (16, 32, 512), "periodic", "kpz", _claim(1, 4, "", 1, 16), K2),
          _case("stage-cz4-idle", f8, (16, 32, 640), "walls", "extras", _claim(1, 4, "idle", 1, 16), K0(1)),
          _case("stage-cz4-idle", f8, (16, 32, 640), "preset", "allen_cahn", _claim(1, 4, "idle", 1, 16), K4IN, special=True),
          _case("stage-cz4-idle", f8, (16, 32, 640), "order2", "kpz", _claim(1, 4, "idle", 1, 16), K2, special=True),
          _case("stage-cz2", f8, (16, 32, 130), "periodic", "axes", _claim(1, 2, "", 1, 16), K0(0)),
          _case("stage-cz2", f8, (16, 32, 130), "walls", "allen_cahn", _claim(1, 2, "", 1, 16), K1),
          _case("stage-cz2", f8, (16, 32, 130), "preset", "kpz", _claim(1, 2, "", 1, 16), K1Y),
          _case("stage-2d", f8, (512, 130), "walls", "allen_cahn", _claim(1, 2, "", 1, 1), K2),
          _case("stage-2d", f8, (512, 130), "periodic", "kpz", _claim(1, 2, "", 1, 1), K4),
          _case("stage-lx2-short", f8, (37, 32, 128), "walls", "axes", _claim(1, 1, "", 2, 19), K0(5), special=True),
          _case("stage-kind1-lx2", f8, (70, 32, 64), "walls", "kpz", _claim(1, 1, "", 2, 35), K1)]
    # -- slope sweeps, fp32: chunk = 256 cells
    t += [_case("cz1", f4, (7, 6, 256), "preset", "allen_cahn", _claim(2, 1, "", 1, 7)),
          _case("cz1", f4, (7, 6, 256), "walls", "extras", _claim(2, 1, "", 1, 7)),
          _case("cz1-tails-odd-rows", f4, (7, 5, 253), "walls", "axes", _claim(2, 1, "vector", 1, 7), special=True),
          _case("cz2", f4, (32, 32, 512), "periodic", "kpz", _claim(2, 2, "", 1, 32)),
          _case("cz2", f4, (32, 32, 512), "order2", "allen_cahn", _claim(2, 2, "", 1, 32)),
          _case("cz2-tails", f4, (32, 32, 258), "walls", "kpz", _claim(2, 2, "vector", 1, 32), special=True),
          _case("cz2-tails", f4, (32, 32, 258), "preset", "extras", _claim(2, 2, "vector", 1, 32)),
          _case("cz2-2d-tails", f4, (1024, 258), "walls", "allen_cahn", _claim(2, 2, "vector", 1, 1)),
          _case("cz4", f4, (32, 32, 1024), "walls", "axes", _claim(2, 4, "", 1, 32)),
          _case("cz4", f4, (32, 32, 1024), "periodic", "allen_cahn", _claim(2, 4, "", 1, 32)),
          _case("cz4-tails", f4, (32, 32, 770), "walls", "extras", _claim(2, 4, "vector", 1, 32), special=True),
          _case("cz4-idle", f4, (32, 32, 1280), "walls", "allen_cahn", _claim(2, 4, "idle", 1, 32)),
          _case("cz4-idle", f4, (32, 32, 1280), "preset", "axes", _claim(2, 4, "idle", 1, 32)),
          _case("lx3-one-plane", f4, (40, 128, 256), "walls", "kpz", _claim(2, 1, "", 3, 14), special=True),
          _case("lx3-one-plane", f4, (40, 128, 256), "preset", "allen_cahn", _claim(2, 1, "", 3, 14))]
    # -- stage sweeps, fp32
    t += [_case("stage-cz2-tails", f4, (16, 16, 770), "periodic", "axes", _claim(1, 2, "vector", 1, 16), K0(0)),
          _case("stage-cz2-tails", f4, (16, 16, 770), "walls", "extras", _claim(1, 2, "vector", 1, 16), K0(1)),
          _case("stage-cz2-tails", f4, (16, 16, 770), "walls", "allen_cahn", _claim(1, 2, "vector", 1, 16), K0(5)),
          _case("stage-cz2-tails", f4, (16, 16, 770), "walls", "kpz", _claim(1, 2, "vector", 1, 16), K1),
          _case("stage-cz2-tails", f4, (16, 16, 770), "preset", "allen_cahn", _claim(1, 2, "vector", 1, 16), K1Y),
          _case("stage-cz2-tails", f4, (16, 16, 770), "order2", "kpz", _claim(1, 2, "vector", 1, 16), K2, special=True),
          _case("stage-cz2-tails", f4, (16, 16, 770), "preset", "allen_cahn", _claim(1, 2, "vector", 1, 16), K4IN, special=True),
          _case("stage-cz2-tails", f4, (16, 16, 770), "walls", "kpz", _claim(1, 2, "vector", 1, 16), K4),
          _case("stage-2d-tails", f4, (512, 258), "periodic", "kpz", _claim(1, 2, "vector", 1, 1), K2),
          _case("stage-cz4", f4, (16, 32, 1024), "walls", "allen_cahn", _claim(1, 4, "", 1, 16), K0(5))]
    return t


def generic_cases():
    """The same kernels' grids from buffers 8 bytes past a 16-byte boundary: input, output and one extra array shifted in turn."""
    out = []
    for dtype in ("float64", "float32"):
        for shape in ((8, 6, 128), (9, 130)):
            for shift in ("in", "out", "extra"):
                out.append(_case("generic", dtype, shape, "walls", "extras", None, shift=shift))
    return out


def worker_cases():
    """A handful for the process with the tuning knobs set: slope and stage, walls, tails, 3-D (and one 2-D grid)."""
    pick = {("cz2-tails", "float64", "walls"), ("cz4-idle", "float64", "walls"), ("lx3-one-plane", "float64", "walls"), ("stage-cz4-idle", "float64", "walls"),
            ("stage-2d", "float64", "walls"), ("stage-kind1-lx2", "float64", "walls"), ("cz4-tails", "float32", "walls"), ("stage-cz2-tails", "float32", "walls")}
    return [c for c in cases() if (c.what, c.dtype.name, c.faces) in pick]


def case_plan(c, knobs=None):
    if c.shift:
        return plan(c.shape, c.dtype, aligned=False)
    st = c.stage
    nk = 0 if st is None else min(st["nk"], 2)
    return plan(c.shape, c.dtype, stage=st is not None, kind=st["kind"] if st else 0, nk=nk, fused=c.faces != "preset", knobs=knobs)


def case_probe(lib, c, knobs=None):
    if c.shift:
        return probe(lib, c.shape, c.dtype, aligned=False)
    st = c.stage
    nk = 0 if st is None else min(st["nk"], 2)
    return probe(lib, c.shape, c.dtype, stage=st is not None, kind=st["kind"] if st else 0, nk=nk, fused=c.faces != "preset", knobs=knobs)


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def special_cells(c, p):
    """(NaN, +inf, denormal): the last cell of three rows - the last vector of a row that ends inside one - the first two in the first plane of
    the second x-chunk (the first plane when there is only one chunk)."""
    nd = len(c.shape)
    last = c.shape[-1] - 1
    plane = p.lx if (nd == 3 and p.nxc > 1) else 0
    rows = c.shape[-2]
    cells = [(plane, 1 % rows, last), (plane, rows - 1, last), (0, 0, last)]
    return [cell[3 - nd:] for cell in cells]


def arrays(c, p=None):
    """The compact full arrays (ghost cells included) of a case: ``in``, ``e0..e2``, ``y``, ``k0..k4`` as the call uses them."""
    p = p or case_plan(c)
    rng = np.random.default_rng([23, len(c.shape), c.shape[-1], c.dtype.itemsize])
    full = tuple(s + 2 for s in c.shape)
    a = {"in": (2.0 * rng.uniform(-1, 1, full)).astype(c.dtype)}
    if c.special:
        tiny = np.finfo(c.dtype).tiny
        for cell, v in zip(special_cells(c, p), (np.nan, np.inf, tiny / 4)):
            a["in"][tuple(i + 1 for i in cell)] = v
    for m in range(ALL_BODIES[c.body][2]):
        a[f"e{m}"] = rng.uniform(-1, 1, full).astype(c.dtype)
    if c.stage is not None:
        a["y"] = rng.uniform(-1, 1, full).astype(c.dtype)
        for m in range(c.stage["nk"]):
            a[f"k{m}"] = (0.5 * rng.uniform(-1, 1, full)).astype(c.dtype)
    return a


def pattern_is_far(values):
    """Every finite reference value is at least a factor 100 away from the smallest pattern value: a stray store of a computed value shows."""
    with np.errstate(invalid="ignore"):
        v = np.abs(values[np.isfinite(values)].astype(np.float64))
    return v.size > 0 and v.max() * 100 < 1024


# ---- references -----------------------------------------------------------------------------------------------------------------------
_SHIM = {}


def shim():
    """The host shim as a plain ctypes library with the prototypes of ``pde_hip._abi`` (stage sweeps enabled)."""
    if not _SHIM:
        import shimlib
        from pde_hip import _lib

        os.environ["PDEHIP_SHIM_FUSED"] = "1"      # (read by the shim at every call of pdehip_jit_apply_stage)
        _SHIM["lib"] = _lib._Lib(shimlib.build())
        _SHIM["handles"] = {}
    return _SHIM["lib"]


def shim_handle(body):
    lib = shim()
    if body not in _SHIM["handles"]:
        h = C.c_void_p()
        lib.jit_create(ALL_BODIES[body][0].encode(), C.byref(h))
        _SHIM["handles"][body] = h
    return _SHIM["handles"][body]


def _ptrs(arrs):
    out = (C.c_void_p * 3)()
    for m, a in enumerate(arrs):
        out[m] = a.ctypes.data if a is not None else None
    return out


def _pd(values):
    return (C.c_double * len(values))(*values)


def grid_of(c, dtype=None):
    nd = len(c.shape)
    return _abi.make_grid(c.shape, DX[3 - nd:], dtype or c.dtype)


def input_after_call(c, a, generic):
    """The input array after the call: ghost cells written by ``launch_ghosts`` for the faces that are not applied on the fly."""
    out = a["in"].copy()
    if c.faces == "preset":
        return out
    rest = rest_faces(c.shape, c.faces, generic)
    if any(f["kind"] != _abi.BC_SKIP for f in rest):
        O.set_ghost_cells(grid_of(c), 1, S.face_table(rest), out.reshape(1, *out.shape))
    return out


def with_ghosts(c, a, faces=None):
    """The input with every ghost cell the stencil reads set by the oracle in the storage type."""
    out = a["in"].copy()
    O.set_ghost_cells(grid_of(c), 1, S.face_table(face_list(c.shape, faces or c.faces)), out.reshape(1, *out.shape))
    return out


def slope(c, a, faces=None, params=None):
    """The slope of a case on its interior cells (an array of the full shape whose ghost cells are zero), in the case's type."""
    lib = shim()
    params = PARAMS if params is None else params
    g64 = grid_of(c, np.float64)
    src = with_ghosts(c, a, faces).astype(np.float64)              # fp32: widened exactly (the "fp64 twin")
    ex = [a[f"e{m}"].astype(np.float64) if f"e{m}" in a else None for m in range(3)]
    out = np.zeros_like(src)
    lib.jit_apply(shim_handle(c.body), C.byref(g64), src.ctypes.data, _ptrs(ex), out.ctypes.data, _pd(params), ALL_BODIES[c.body][1], None, None)
    with np.errstate(over="ignore"):
        return out.astype(c.dtype)                                  # the one rounding of the store


def stage_reference(c, a, k, coef=COEF, c_new=C_NEW):
    """(out2, error or None) from the slope as stored, by the oracle's combinations in the case's type, in the order pdehip_jit_apply_stage
    documents."""
    st, g = c.stage, grid_of(c)
    ks = [a[f"k{m}"] for m in range(st["nk"])]
    if st["kind"] == 0:
        return O.lincomb(g, 1, a["y"], [*coef[: st["nk"]], c_new], [*ks, k]), None
    if st["kind"] == 1:
        return O.rk4_combine(g, 1, a["y"].copy(), ks[0], ks[1], ks[2], k), None
    if st["kind"] == 2:
        return O.rkf45_combine(g, 1, a["y"], [ks[0], ks[0], ks[1], ks[2], ks[3], k])
    half = a["in"] if st.get("alias") == "k1=in" else ks[1]
    return O.euler_adaptive_combine(g, 1, a["y"], ks[0], DT4, half, k)


def shim_stage(c, a, coef=COEF, c_new=C_NEW):
    """fp64 only: the shim's own pdehip_jit_apply_stage -> (k_out or None, out2, error or None)."""
    assert c.dtype == np.float64
    lib, st, g = shim(), c.stage, grid_of(c)
    src = a["in"].copy()
    table = None if c.faces == "preset" else S.face_table(face_list(c.shape, c.faces))
    if c.faces == "preset":
        src = with_ghosts(c, a)
    ex = [a.get(f"e{m}") for m in range(3)]
    ks = [src if (st.get("alias") == "k1=in" and m == 1) else a[f"k{m}"] for m in range(st["nk"])]
    kp = (C.c_void_p * 5)(*[x.ctypes.data for x in ks])
    cf = _pd([DT4, 0.0] if st["kind"] == 4 else list(coef[: st["nk"]]) + [0.0])
    k_out, out2 = np.zeros_like(src), np.zeros_like(src)
    err = C.c_double(-1.0)
    done = C.c_int(0)
    lib.jit_apply_stage(shim_handle(c.body), C.byref(g), src.ctypes.data, _ptrs(ex), k_out.ctypes.data, _pd(PARAMS), BODIES[c.body][1], table,
                        st["kind"], a["y"].ctypes.data, st["nk"], kp, cf, c_new, out2.ctypes.data, C.cast(C.byref(err), C.c_void_p), C.byref(done), None)
    assert done.value == 1
    return (k_out if st["kind"] == 0 else None), out2, (err.value if st["kind"] in (2, 4) else None)


def reference(c, a=None):
    """{"k": slope or None (not stored), "out2": ..., "err": ...}: interior cells of full-shape arrays."""
    a = a or arrays(c)
    k = slope(c, a)
    if c.stage is None:
        return {"k": k, "out2": None, "err": None}
    out2, err = stage_reference(c, a, k)
    return {"k": k if c.stage["kind"] == 0 else None, "out2": out2, "err": err}


# ---- the two-level run-time built sweeps: one shape per (type, rows per tile, 2-D / 3-D) the two-step planner answers for them -----------------
# (tests/test_jit_cases_cpu.py asks csrc/pdehip_euler2_plan.h through its probe: these are all the keys, and each shape gets its key)
TWO_LEVEL = (("float64", (9, 130), 1), ("float64", (6, 5, 130), 2), ("float64", (6, 8, 130), 4), ("float32", (9, 260), 1), ("float32", (5, 6, 260), 2))


def two_level_name(mode, dtype, shape, ry):
    T, vec = ("double", 2) if np.dtype(dtype) == np.float64 else ("float", 4)
    what = "two applications of the epilogue per sweep" if mode == "two" else "both passes of the expression in one sweep"
    return f"pde_kernel<{mode},{T},{vec},RY={ry},{'3-D' if len(shape) == 3 else '2-D'}> ({what}; run-time built)"


def two_level_reference(mode, dtype, shape):
    """(input, result) as full-shape arrays: two applications of `slope` with walls on every face - the operations of the shim's
    pdehip_jit_euler2 / pdehip_jit_fused2 (fp32: each level through the fp64 twin; the kernel rounds the level it keeps in registers to the
    storage type like the one it stores)."""
    first = _case("two-level", dtype, shape, "walls", "euler_update" if mode == "two" else "chain_first", None)
    a = arrays(first)
    level1 = slope(first, a)
    second = _case("two-level", dtype, shape, "walls", "euler_update" if mode == "two" else "chain_second", None)
    b = {"in": level1}
    if mode == "fused2":
        b["e0"] = a["in"]
    return a["in"], slope(second, b)
