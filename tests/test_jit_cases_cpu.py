"""The table of tests/jit_cases.py on a CPU: the restated planner against ``csrc/pdehip_jit_plan.h`` (through ``tests/shim/jit_plan_probe.cpp``, built
with g++ here), the references against a ``np.longdouble`` restatement, and the conditions that keep a case of
``tests/test_hip_jit_instances.py`` from being vacuous."""

from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import jit_cases as J
import numpy as np
import pytest
import small_kernel_cases as S

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "py-pde_amd" / "csrc" / "pdehip_jit_plan.h"
PROBE = ROOT / "tests" / "shim" / "jit_plan_probe.cpp"
BUILD = ROOT / "tests" / "shim" / "_build"

CASES = J.cases()
IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def lib():
    BUILD.mkdir(exist_ok=True)
    so = BUILD / "libjitplan_probe.so"
    if not so.exists() or so.stat().st_mtime < max(HEADER.stat().st_mtime, PROBE.stat().st_mtime):
        tmp = so.with_suffix(f".{os.getpid()}.tmp")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", str(PROBE), "-o", str(tmp)], check=True)
        os.replace(tmp, so)
    return C.CDLL(str(so))


@pytest.fixture(scope="module")
def refs():
    """arrays and reference of every case, computed once"""
    cache = {}

    def get(c):
        if c.id not in cache:
            a = J.arrays(c)
            cache[c.id] = (a, J.reference(c, a))
        return cache[c.id]

    return get


# ---- the planner --------------------------------------------------------------------------------------------------------------------
def test_the_header_is_plain_host_code():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-"], input=f'#include "{HEADER}"\n', text=True, check=True)
    text = HEADER.read_text()
    assert "hip_runtime" not in text and "__device__" not in text and "__global__" not in text
    # the tuning knobs are read in one function of the header, once per process in pdehip_jit.hip
    jit = (HEADER.parent / "pdehip_jit.hip").read_text()
    for knob in ("RY", "CZ", "WY", "BLOCKS"):
        assert f'getenv("PDEHIP_JIT_{knob}")' not in jit and text.count(f'getenv("PDEHIP_JIT_{knob}")') == 1
    assert jit.count("jitplan::knobs_from_env()") == 1 and "static const jitplan::Knobs k = jitplan::knobs_from_env();" in jit


def test_ids_are_unique():
    assert len(set(IDS)) == len(IDS)
    assert len({c.id for c in J.generic_cases()}) == len(J.generic_cases()) == 12


@pytest.mark.parametrize("knobs", [None, J.WORKER_KNOBS], ids=["defaults", "worker-knobs"])
def test_every_case_plans_the_same_in_the_header_and_here(lib, knobs):
    for c in CASES + J.generic_cases():
        got, name = J.case_probe(lib, c, knobs)
        mine = J.case_plan(c, knobs)
        assert got == J.as_dict(mine), c.id
        assert name == J.kernel_name(mine), c.id


def test_every_case_reaches_the_instance_it_claims():
    for c in CASES:
        p = J.case_plan(c)
        got = {"ry": p.ry, "cz": p.cz, "tails": J.tails_kind(c.shape, c.dtype, p), "lx": p.lx, "nxc": p.nxc}
        assert not p.generic and got == c.claim, f"{c.id}: planned {got}"
        assert p.ibc == (c.faces != "preset") and p.stage == (c.stage is not None) and p.hasx == (len(c.shape) == 3)
    for c in J.generic_cases():
        assert J.case_plan(c).generic
    # what the named rows of the table are about
    by = {c.what: (c, J.case_plan(c)) for c in CASES if c.dtype == np.float64}
    c, p = by["lx2-full"]
    assert c.shape[0] % p.lx == 0
    for what in ("lx2-short", "lx3-one-plane", "stage-lx2-short"):
        c, p = by[what]
        assert c.shape[0] - (p.nxc - 1) * p.lx == 1 < p.lx, what                       # the last x-chunk is one plane
    c, p = by["lx2-swizzle-remainder"]
    assert p.lx > 1 and p.nblocks % 8 != 0
    c, p = by["stage-kind1-lx2"]
    assert p.lx == 2 and J.plan(c.shape, c.dtype, stage=True, kind=0, nk=2, fused=True).lx == 3      # `want` 2048 against 1024: the name tells
    c, p = by["cz1-tails-odd-rows"]
    assert c.shape[1] % p.ry == 1
    for dtype in ("float64", "float32"):
        c = next(c for c in CASES if c.what == "lx3-one-plane" and c.dtype == np.dtype(dtype))
        p = J.case_plan(c)
        assert (p.lx, p.nxc) == (3, 14)


def test_every_axis_value_is_hit_for_both_types():
    for dtype in ("float64", "float32"):
        mine = [c for c in CASES if c.dtype == np.dtype(dtype)]
        plans = [J.case_plan(c) for c in mine]
        assert {p.cz for p in plans if not p.stage} == {1, 2, 4} and {p.cz for p in plans if p.stage} >= {2, 4}
        assert {J.tails_kind(c.shape, c.dtype, p) for c, p in zip(mine, plans)} == {"", "vector", "idle"}
        assert {p.lx > 1 for p in plans} == {False, True}
        assert {(p.hasx, p.stage) for p in plans} == {(False, False), (False, True), (True, False), (True, True)}
        assert {c.faces for c in mine} == set(J.FACES) and {c.body for c in mine} == set(J.BODIES)
        assert {c.faces for c in mine if c.stage} == set(J.FACES)
        kinds = {(c.stage["kind"], c.stage["nk"], c.stage.get("alias")) for c in mine if c.stage}
        assert kinds == {(0, 0, None), (0, 1, None), (0, 5, None), (1, 3, None), (1, 3, "out2=y"), (2, 4, None), (4, 2, None), (4, 2, "k1=in")}, dtype
        # required together: an upper z wall on every tails kind and CZ = 1 / 2 / 4; x walls where a workgroup marches several planes; y walls on an
        # odd number of rows with two rows per tile; special values in a tails row and in the first plane of an x-chunk
        walls = [(c, p) for c, p in zip(mine, plans) if c.faces in ("walls", "order2")]
        assert {(p.cz, J.tails_kind(c.shape, c.dtype, p)) for c, p in walls} >= {(1, "vector"), (2, "vector"), (4, "vector"), (4, "idle")}
        assert any(p.lx > 1 for c, p in walls) and any(c.shape[-2] % 2 == 1 and p.ry == 2 for c, p in walls)
        special = [(c, p) for c, p in zip(mine, plans) if c.special]
        assert any(J.tails_kind(c.shape, c.dtype, p) == "vector" for c, p in special) and any(p.lx > 1 for c, p in special)
        assert any(c.stage and c.stage["kind"] == 2 for c, p in special) and any(c.stage and c.stage["kind"] == 4 for c, p in special)
    f8 = [J.case_plan(c) for c in CASES if c.dtype == np.float64]
    assert any(not p.hasx and p.stage for p in f8) and any(not p.hasx and not p.stage for p in f8)
    assert len({(c.body, c.dtype.name, tuple(sorted(J.as_dict(J.case_plan(c)).items()))) for c in CASES}) < 100       # hiprtc builds stay few


def _thresholds():
    out = []
    for dtype, chunk in (("float64", 128), ("float32", 256)):
        n2s = [chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1, 3 * chunk + 1, 4 * chunk - 1, 4 * chunk, 4 * chunk + 1]
        for n2 in n2s:
            for n0, n1 in ((1, 3), (32, 32), (16, 32), (16, 31), (7, 73)):
                out.append((dtype, (n0, n1, n2)))
            out.append((dtype, (1024, n2)))
            out.append((dtype, (1022, n2)))
            out.append((dtype, (511, n2)))
        # 511 / 512 wave tiles at CZ = 2 and CZ = 4 (two rows per tile; one row per tile for stages)
        for cz in (2, 4):
            for tiles in (511, 512):
                out.append((dtype, (2 * tiles, cz * chunk)))
                out.append((dtype, (tiles, cz * chunk)))
                out.append((dtype, (tiles, 2, cz * chunk)))
                out.append((dtype, (tiles, 1, cz * chunk)))
        # want / tiles on either side of n0: 1024 (2048) waves over 32 tiles per plane = 32 (64) planes
        for n0 in (31, 32, 33, 63, 64, 65, 127, 128, 129):
            out.append((dtype, (n0, 64, chunk // 2)))
            out.append((dtype, (n0, 32, chunk // 2)))
            out.append((dtype, (n0, 16, chunk)))
    return out


def test_threshold_sweep_header_against_restatement(lib):
    count = 0
    for dtype, shape in _thresholds():
        for stage, kind, nk in ((False, 0, 0), (True, 0, 0), (True, 0, 1), (True, 0, 2), (True, 1, 2), (True, 2, 2), (True, 5, 2)):
            for fused in (False, True):
                for knobs in (None, J.WORKER_KNOBS, {"cz": 2}, {"cz": 8, "ry": 1, "wy": 4}):
                    for aligned in (True, False):
                        kw = dict(aligned=aligned, stage=stage, kind=kind, nk=nk, fused=fused, knobs=knobs)
                        got, name = J.probe(lib, shape, dtype, **kw)
                        mine = J.plan(shape, dtype, **kw)
                        assert got == J.as_dict(mine) and name == J.kernel_name(mine), (dtype, shape, kw)
                        count += 1
    assert count > 5000
    # 1-D: always the generic kernel
    got, name = J.probe(lib, (300,), "float64")
    assert got["generic"] == 1 and name == "pde_kernel<generic,double> (run-time built)"


def test_the_documented_name():
    assert J.kernel_name(J.plan((40, 128, 64), "float64", fused=True)) == "pde_kernel<double,2,RY=2,CZ=1,WY=1,3-D,ibc,-,-> (lx=3, 14 x-chunks; run-time built)"
    assert J.kernel_name(J.plan((16, 32, 640), "float32", stage=True, kind=2, nk=2)) == "pde_kernel<float,4,RY=1,CZ=2,WY=1,3-D,-,stage,tails> (lx=1, 16 x-chunks; run-time built)"
    assert J.kernel_name(J.plan((512, 130), "float64", fused=True)) == "pde_kernel<double,2,RY=2,CZ=1,WY=1,2-D,ibc,-,-> (lx=1, 1 x-chunk; run-time built)"


# ---- references and non-vacuity -------------------------------------------------------------------------------------------------------
def _longdouble_slope(c, a):
    """The slope of a case once more: numpy stencils and the epilogue in np.longdouble from the storage-type values (ghost cells by the oracle)."""
    L = np.longdouble
    u = J.with_ghosts(c, a).astype(L)
    nd = len(c.shape)
    inner = S.interior(nd)
    dx = J.DX[3 - nd:]

    def sh(axis, o):
        sl = [slice(1, -1)] * nd
        sl[axis] = slice(1 + o, u.shape[axis] - 1 + o)
        return u[tuple(sl)]

    cen = u[inner]
    lap, gsq = 0, 0
    d1, d2, gr = [L(0)] * 3, [L(0)] * 3, [L(0)] * 3
    for ax in range(nd):
        q = 3 - nd + ax
        hi, lo = sh(ax, 1), sh(ax, -1)
        lap = lap + (hi - 2 * cen + lo) / L(dx[ax]) ** 2
        gsq = gsq + (hi - lo) ** 2 * L(0.25) / L(dx[ax]) ** 2
        d1[q] = (hi - lo) / (2 * L(dx[ax]))
        d2[q] = (hi - 2 * cen + lo) / L(dx[ax]) ** 2
        gr[q] = d1[q]
    e = [a[f"e{m}"][inner].astype(L) if f"e{m}" in a else L(0) for m in range(3)]
    return J.body_longdouble(c.body, cen, lap, gsq, e, J.PARAMS, d1, d2, gr)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_references(c, refs):
    """The reference against the np.longdouble restatement (fp32: within one ulp - the fp64 evaluation error is far below half an fp32 ulp, so the
    twin is the correctly rounded value or its neighbour; fp64: within the rounding of a dozen operations), and what keeps the case from being
    vacuous."""
    a, ref = refs(c)
    inner = S.interior(len(c.shape))
    k = J.slope(c, a)[inner]
    with np.errstate(all="ignore"):
        want = _longdouble_slope(c, a)
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(k), np.isnan(want.astype(np.float64)))
        scale = np.maximum(np.abs(want[fin]), np.abs(J.PARAMS[0]) * 64)        # (the terms of the sums are up to 64 / dx^2 times the field)
        ulps = np.abs(k[fin].astype(np.longdouble) - want[fin]) / (np.finfo(c.dtype).eps * scale)
    assert fin.sum() > 0.9 * fin.size
    assert ulps.max() <= (1.0 if c.dtype == np.float32 else 16.0), f"{ulps.max()} ulp"
    assert J.pattern_is_far(k) and (ref["out2"] is None or J.pattern_is_far(ref["out2"][inner]))
    if c.special:
        assert np.isnan(k).any() and np.isinf(a["in"]).any() and (np.abs(a["in"][np.isfinite(a["in"]) & (a["in"] != 0)]) < np.finfo(c.dtype).tiny).any()
        if c.stage and c.stage["kind"] in (2, 4):
            assert np.isnan(ref["err"])
    elif c.stage and c.stage["kind"] in (2, 4):
        assert ref["err"] > 0
    # walls: the reference differs from the same case with periodic faces (in the cells next to every face)
    if c.faces in ("walls", "order2"):
        per = J.slope(c, a, faces="periodic")[inner]
        for ax in range(len(c.shape)):
            for side in (0, -1):
                sl = [slice(None)] * len(c.shape)
                sl[ax] = side
                assert (S.bits(per[tuple(sl)]) != S.bits(k[tuple(sl)])).any(), f"axis {ax} side {side}"
    # stages: two swapped coefficients (kind 0), two swapped slopes (the fixed-weight kinds) change the result
    st = c.stage
    if st is not None:
        kf = J.slope(c, a)
        if st["kind"] == 0 and st["nk"] >= 1:
            for m in range(st["nk"]):
                coef = list(J.COEF)
                other = (m + 1) % st["nk"] if st["nk"] > 1 else None
                if other is None:
                    swapped, _ = J.stage_reference(c, a, kf, coef=[J.C_NEW], c_new=coef[0])
                else:
                    coef[m], coef[other] = coef[other], coef[m]
                    swapped, _ = J.stage_reference(c, a, kf, coef=coef)
                assert (S.bits(swapped[inner]) != S.bits(ref["out2"][inner])).mean() > 0.9, m
        elif st["kind"] != 0:
            b = dict(a)
            b["k0"], b["k1"] = a["k1"], a["k0"]
            swapped, err = J.stage_reference(c, b, kf)
            assert (S.bits(swapped[inner]) != S.bits(ref["out2"][inner])).mean() > 0.9 or st["kind"] == 4
            if st["kind"] == 4:
                assert err != ref["err"] or np.isnan(err)
        assert (S.bits(ref["out2"][inner]) != S.bits(a["y"][inner])).mean() > 0.9
    # fp64: the shim's own stage entry point gives the same bits as slope + combination
    if st is not None and c.dtype == np.float64:
        k_out, out2, err = J.shim_stage(c, a)
        assert np.array_equal(S.bits(out2[inner])[~np.isnan(out2[inner])], S.bits(ref["out2"][inner])[~np.isnan(out2[inner])])
        assert np.array_equal(np.isnan(out2[inner]), np.isnan(ref["out2"][inner]))
        if k_out is not None:
            assert np.array_equal(S.bits(k_out[inner])[~np.isnan(k)], S.bits(k)[~np.isnan(k)])
        if err is not None:
            assert (np.isnan(err) and np.isnan(ref["err"])) or err == ref["err"]


def test_generic_cases_have_references():
    for c in J.generic_cases()[:2]:
        a = J.arrays(c)
        k = J.slope(c, a)
        assert np.isfinite(k).all() and J.pattern_is_far(k)
        after = J.input_after_call(c, a, generic=True)
        assert (S.bits(after) != S.bits(a["in"])).any()


def test_two_level_shapes_cover_every_key_of_the_two_step_planner():
    """csrc/pdehip_euler2_plan.h with ``plan = true`` (the caller launches a run-time built instance) for the modes E2_CUSTOM and E2_CUSTOM2: the keys
    (type, rows per tile, 2-D / 3-D) it can answer over a sweep of small shapes are the five of `J.TWO_LEVEL`, and each of its shapes gets its key."""
    import test_euler2_plan as E

    E.BUILD.mkdir(exist_ok=True)
    so = E.BUILD / "libe2plan_probe.so"
    if not so.exists() or so.stat().st_mtime < max(E.HEADER.stat().st_mtime, E.PROBE.stat().st_mtime):
        tmp = so.with_suffix(f".{os.getpid()}.tmp")
        subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", str(E.PROBE), "-o", str(tmp)], check=True)
        os.replace(tmp, so)
    lib = C.CDLL(str(so))
    keys = set()
    sizes = (1, 2, 3, 4, 5, 8, 33, 128, 130, 260)
    shapes = [(a, b) for a in sizes for b in sizes] + [(a, b, c) for a in (1, 2, 6) for b in (1, 2, 3, 4, 5, 8, 16) for c in (4, 8, 130, 260)]
    for m2 in (E.CUSTOM, E.CUSTOM2):
        for elem in (8, 4):
            for shape in shapes:
                c = E.ask(lib, elem, shape, (0, 0, 0), m2=m2, plan=True, unit=False)
                if c.accepted:
                    keys.add((elem, c.ry, bool(c.has_y)))
        for dtype, shape, ry in J.TWO_LEVEL:
            c = E.ask(lib, np.dtype(dtype).itemsize, shape, (0, 0, 0), m2=m2, plan=True, unit=False)
            assert c.accepted and c.ry == ry and bool(c.has_y) == (len(shape) == 3), (dtype, shape)
    assert keys == {(np.dtype(d).itemsize, ry, len(s) == 3) for d, s, ry in J.TWO_LEVEL}
    for mode in ("two", "fused2"):
        for dtype, shape, _ in J.TWO_LEVEL:
            src, ref = J.two_level_reference(mode, dtype, shape)
            inner = S.interior(len(shape))
            assert np.isfinite(ref[inner]).all() and J.pattern_is_far(ref[inner]) and (S.bits(ref[inner]) != S.bits(src[inner])).mean() > 0.9
