"""tests/tile2d_cases.py pinned on the CPU: the restated planner against hand-computed rows, and the conditions that keep a case of
tests/test_hip_tile2d_instances.py from being vacuous.

``plan_tile2d`` itself is not reachable from Python without a device (every entry point that calls it launches a kernel), so the restatement is
pinned by rows computed by hand for the named shapes, not by the library.  Which launches take the tile kernel is decided by a restatement of the
predicates of ``pdehip_jit_euler_run`` on the pass descriptors the package hands to the library (`tile_route`): every case of the table must be
routed to its mode and every refusal must not, so that a fall-back cannot pass as a tile test on the device.
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import shimlib
import tile2d_cases as T

from pde_hip import _abi
from pde_hip.rhs import _match_expression_rhs

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "py-pde_amd" / "csrc" / "pdehip_jit_plan.h"
PROBE = ROOT / "tests" / "shim" / "jit_plan_probe.cpp"


def test_the_restated_planner_gives_the_hand_computed_rows():
    for shape, width, tiles, last_rows, last_cols in T.PLAN_ROWS:
        assert T.tile_width(shape) == width, shape
        assert T.tiles(shape) == tiles, shape
        assert shape[0] - (tiles[0] - 1) * T.TILE_ROWS == last_rows and shape[1] - (tiles[1] - 1) * width == last_cols, shape
    for mode, steps, ks in T.LAUNCH_ROWS:
        assert T.launches(mode, steps) == ks, (mode, steps)
    assert [T.kmax(m) for m in range(5)] == [8, 4, 8, 8, 4]
    assert T.kernel_name("float64", 3, (33, 8130), 8) == "tile2d_kernel<double,mode=3,32x64 tile> (8 steps per launch, time levels in LDS; run-time built)"
    assert T.kernel_name("float32", 1, (32, 8130), 4) == "tile2d_kernel<float,mode=1,32x32 tile> (4 steps per launch, time levels in LDS)"
    assert T.last_kernel_name("float32", 4, (64, 64), 11) == "tile2d_kernel<float,mode=4,32x32 tile> (3 steps per launch, time levels in LDS; run-time built)"
    assert T.last_kernel_name("float64", 2, (64, 64), 9) == "tile2d_kernel<double,mode=2,32x32 tile> (1 steps per launch, time levels in LDS; run-time built)"


def test_the_shapes_are_what_they_claim_to_be():
    for shape in T.WIDE_SHAPES:
        assert T.tile_width(shape) == 64 and -(-shape[1] // 64) * -(-shape[0] // 32) == 256      # the smallest count the rule accepts
    assert T.tile_width(T.CONTRAST_SHAPE) == 32 and -(-T.CONTRAST_SHAPE[1] // 64) * -(-T.CONTRAST_SHAPE[0] // 32) == 128
    assert T.CONTRAST_SHAPE[1] == T.WIDE_SHAPES[0][1] and T.CONTRAST_SHAPE[0] == T.WIDE_SHAPES[0][0] - 1
    assert [T.seams(s) for s in T.WIDE_SHAPES] == [(True, True)] * 3
    assert T.tiles((481, 961)) == (16, 16)                                     # seams with tiles on both sides of both axes
    assert T.WIDE_SHAPES[0][1] % 64 == 2 and T.WIDE_SHAPES[0][0] % 32 == 1      # ragged last tile column, second row tile of one row
    assert max(s[0] * s[1] for s in T.BUILTIN_SHAPES) == 481 * 961 < 463_000
    # modes 2-4 at 32 columns: a row seam ((24, 130) of the older test has none), ragged tiles, one row tile
    assert [T.seams(s) for s in T.NARROW_SHAPES] == [(True, True), (True, True), (True, True), (False, True)]
    assert all(T.tile_width(s) == 32 for s in T.NARROW_SHAPES + T.TINY_SHAPES)
    for shape in T.TINY_SHAPES:      # smaller than the halo of a full launch in every mode: periodic axes wrap more than once
        assert min(shape) < T.HALO and T.tiles(shape) == (1, 1)
    assert any(s[0] == 1 for s in T.TINY_SHAPES) and any(s[1] == 1 for s in T.TINY_SHAPES)


def test_the_table_covers_what_it_is_designed_to_cover():
    cases = T.JIT_CASES
    assert 200 <= len(cases) <= 400 and len({c.id for c in cases}) == len(cases)
    assert 20 <= len(T.jit_items()) <= 48
    for mode in (2, 3, 4):
        mine = [c for c in cases if c.mode == mode]
        assert {(T.tile_width(c.shape), c.dtype) for c in mine} == {(w, d) for w in (32, 64) for d in T.DTYPES}
        assert {c.faces for c in mine} == set(T.FACE_NAMES)
        assert {c.steps for c in mine} == set(T.jit_steps(mode))
        assert {c.expr for c in mine} == set(T.EXPRESSIONS[mode])
        for dtype in T.DTYPES:
            wide = [c for c in mine if T.tile_width(c.shape) == 64 and c.dtype == dtype]
            assert {c.shape for c in wide} == set(T.WIDE_SHAPES)
            assert any(c.faces != "pp" for c in wide) and any(len(T.launches(mode, c.steps)) > 1 for c in wide)
            assert any(c.shape == T.CONTRAST_SHAPE for c in mine if c.dtype == dtype)
            # every expression: a second launch (step0 > 0), a short remainder, and the tiny shapes
            for expr in T.EXPRESSIONS[mode]:
                own = [c for c in mine if c.expr == expr and c.dtype == dtype]
                assert any(len(T.launches(mode, c.steps)) > 1 for c in own) and any(T.launches(mode, c.steps)[-1] < T.kmax(mode) for c in own)
                assert {c.shape for c in own} >= set(T.NARROW_SHAPES + T.TINY_SHAPES)
                assert any(c.faces in ("lp", "ll", "nn") and T.seams(c.shape)[0] for c in own)      # a local x face on a grid with a row seam
        assert any(c.tables_differ and T.tile_width(c.shape) == 64 for c in mine) or mode == 2
    assert {2 * T.kmax(m) + 3 for m in (2, 3, 4)} == {19, 11}
    for c in cases:
        assert (c.t_start != 0.0) == (c.expr in T.READS_TIME) == any("(t)" in e or e.endswith("* t") for e in T.EXPRESSIONS[c.mode][c.expr].values())
    # every mode has an expression that reads the time of its level
    assert {m for m, ex in T.EXPRESSIONS.items() for name in ex if name in T.READS_TIME} == {2, 3, 4}


def test_no_expression_is_recognised_as_a_class():
    """`eq.solve` sends an expression the matcher recognises through the hand-written sweeps (modes 0 and 1): none of the table's may be one.  The
    form with `+ 0*c` IS one (sympy folds the term away), which is why the table has `ch_sink` in its place."""
    for exprs in T.EXPRESSIONS.values():
        for rhs in exprs.values():
            if len(rhs) == 1:
                ((var, e),) = rhs.items()
                assert _match_expression_rhs(e, var, {}) is None, e
    assert _match_expression_rhs("laplace(c**3 - c - 0.01 * laplace(c)) + 0*c", "c", {}) is not None


# ---- modes 0 and 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(T.KINDS))
@pytest.mark.parametrize("shape", T.BUILTIN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_references_of_the_built_in_modes(shape, kind):
    """Finite, every level different from the one before, and - with local faces - different when a face constant moves."""
    steps = T.builtin_steps(kind)
    for faces in T.FACE_NAMES:
        for dtype in T.DTYPES:
            data = T.field_data(shape, dtype)
            levels = T.oracle_levels(shape, faces, kind, dtype, data, steps)
            prev = data
            for k in steps:
                assert levels[k].dtype == np.dtype(dtype) and np.isfinite(levels[k]).all() and not np.array_equal(levels[k], prev), (faces, dtype, k)
                prev = levels[k]
            if faces != "pp":
                moved = T.oracle_levels(shape, faces, kind, dtype, data, steps, bump=T.BUMP)
                for k in steps:
                    assert not np.array_equal(moved[k], levels[k]), (faces, dtype, k)


def test_the_second_table_of_cahn_hilliard_matters():
    """mode 1 gets other conditions for mu than for c: with the table of c in both slots the result differs"""
    from helpers import expect_steps

    from pde_hip import _abi

    shape, dtype = (33, 70), "float64"
    data = T.field_data(shape, dtype)
    for faces in ("pl", "lp", "ll", "nn"):
        got = T.oracle_levels(shape, faces, "cahn_hilliard", dtype, data, [4])[4]
        same = expect_steps(_abi.RHS_CAHN_HILLIARD, T.KINDS["cahn_hilliard"][1], T.make_grid(shape, faces), T.table(faces), data, T.KINDS["cahn_hilliard"][2], 4)
        assert not np.array_equal(got, same), faces


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("kind", list(T.KINDS))
@pytest.mark.parametrize("shape", T.SPECIAL_SHAPES, ids=T.SPECIAL_IDS)
def test_the_special_value_cases_are_what_they_claim_to_be(shape, kind, dtype):
    mode = T.KINDS[kind][0]
    k = T.kmax(mode)
    data, spots = T.special_data(shape, dtype)
    width, (n0, n1) = T.tile_width(shape), shape
    assert data.dtype == np.dtype(dtype) and T.seams(shape) == (True, True)
    # planted: every kind of value; on both sides of a row seam and of a column seam; next to each of the four (local) faces
    planted = np.array([data[s] for s in spots])
    tiny = np.finfo(np.dtype(dtype)).tiny
    assert np.isinf(planted).any() and np.isnan(planted).any() and (np.abs(planted[np.isfinite(planted)]) > 1e37).any()
    assert ((np.abs(planted) < tiny) & (planted != 0)).any() and (np.signbit(planted) & (planted == 0)).any() and (~np.signbit(planted) & (planted == 0)).any()
    rows, cols = {r for r, _ in spots}, {c for _, c in spots}
    assert {0, n0 - 1, 31, 32} <= rows and {0, n1 - 1} <= cols and any(c % width == 0 and c - 1 in cols for c in cols if c)
    assert T.PERIODIC[T.SPECIAL_FACES] == (False, False)
    with np.errstate(all="ignore"):
        want = T.oracle_levels(shape, T.SPECIAL_FACES, kind, dtype, data, [k])[k]
    assert np.isnan(want).sum() > len(spots) and np.isfinite(want).sum() > want.size // 2
    assert ((np.abs(want) < tiny) & (want != 0)).sum() > 100, "no denormal results"
    assert np.isinf(want).any() or kind == "cahn_hilliard"


# ---- modes 2-4 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item", T.jit_items(), ids=T.jit_item_id)
def test_shim_references_of_the_run_time_built_modes(item):
    (mode, expr, dtype, width), cases = item
    for c in cases:
        assert T.tile_width(c.shape) == width
        state = T.state_of(c.mode, c.shape, c.faces, c.dtype)
        ref = T.jit_reference(c)
        assert ref.dtype == np.dtype(dtype) and ref.shape == np.asarray(state.data).shape
        assert np.isfinite(ref).all() and not np.array_equal(ref, state.data), c.id
        with shimlib.use_shim(fused=False):
            assert T.tile_route(T.jit_eq(c.mode, c.expr, c.faces), state, c.steps) == mode, f"{c.id}: not routed to mode {mode} of the tile kernel"
        if c.faces != "pp":
            assert not np.array_equal(T.jit_reference(c, "bump"), ref), f"{c.id}: a moved face constant of the first table leaves the reference alone"
        if c.tables_differ:
            assert not np.array_equal(T.jit_reference(c, "bump2"), ref), f"{c.id}: a moved face constant of the second table leaves the reference alone"
            assert not np.array_equal(T.jit_reference(c, "swap"), ref), f"{c.id}: the two tables can be exchanged"
        if c.expr in T.READS_TIME:
            assert not np.array_equal(T.jit_reference(c, t_start=0.0), ref), f"{c.id}: the start time does not matter"
            if len(T.launches(mode, c.steps)) > 1:
                # ... and neither does the time of the second launch: the run continued from the first launch's result with the
                # clock set back to the start differs (what a launch that ignores `step0` computes)
                k0 = T.launches(mode, c.steps)[0]
                eq = T.jit_eq(c.mode, c.expr, c.faces)
                mid = T.shim_solve(eq, state, c.t_start, c.dt, k0)
                again = _state_with(state, mid)
                stale = T.shim_solve(eq, again, c.t_start, c.dt, c.steps - k0)
                assert not np.array_equal(stale, ref), f"{c.id}: a second launch at the first launch's times gives the same result"


def _state_with(state, data):
    out = state.copy()
    out.data[...] = data
    return out


def test_the_refusal_list_is_exactly_the_cases_that_miss_the_tile_kernel():
    """(every case of the table is routed to its mode: test_shim_references_of_the_run_time_built_modes)"""
    ids = []
    for rid, eq, state, t_start, dt, steps in T.refusals():
        ids.append(rid)
        with shimlib.use_shim(fused=False):
            assert T.tile_route(eq, state, steps) is None, rid
            if rid == "one-cell-axis-of-two-classes":
                assert T.tile_route(T.jit_eq(3, "one_way", "ll"), T.state_of(3, (9, 1), "ll", "float64"), steps) == 3
            elif rid not in ("more-cells-than-the-limit", "one-step", "one-step-chain"):
                # ... because of its conditions alone: with those of the table it is a tile case
                mode = 3 if state.__class__.__name__ == "FieldCollection" else 2
                plain = T.jit_eq(mode, "brusselator" if mode == 3 else "allen_cahn", "lp")
                assert T.tile_route(plain, state, steps) == mode, rid
        ref = T.shim_solve(eq, state, t_start, dt, steps)
        assert np.isfinite(ref).all() and not np.array_equal(ref, state.data), rid
    assert ids == ["more-cells-than-the-limit", "one-step", "one-step-chain", "second-order-face", "array-face", "tables-of-other-periodicity",
                   "one-cell-axis-of-two-classes"]
    thin = T.refusals()[0][2].grid.shape
    assert thin[0] * thin[1] == T.TILE_CELLS_DEFAULT + 2
    # one step fewer cells / one step more and the first three are tile cases
    with shimlib.use_shim(fused=False):
        _, eq, state, *_ = T.refusals()[1]
        assert T.tile_route(eq, state, 2) == 3
        _, eq, state, *_ = T.refusals()[2]
        assert T.tile_route(eq, state, 2) == 4
        assert T.tile_route(T.refusals()[0][1], T.state_of(2, (2, 1048576), "pl", "float64"), 3) == 2


# ---- the route of pdehip_jit_euler_run, asked of the library's own header --------------------------------------------------------------
# ``jitplan::tile_mode`` (csrc/pdehip_jit_plan.h) decides from the pass descriptors, the component count, the grid, the step count, "has a
# boundary program" and the knobs; the classes of the faces are plan_tile2d's part and stay outside (`T.tile_route` = `T.loop_route` + faces).
NONE = _abi.JIT_NONE


@pytest.fixture(scope="module")
def probe():
    build = PROBE.parent / "_build"
    build.mkdir(exist_ok=True)
    so = build / "libjitplan_probe.so"
    if not so.exists() or so.stat().st_mtime < max(HEADER.stat().st_mtime, PROBE.stat().st_mtime):
        tmp = so.with_suffix(f".{os.getpid()}.tmp")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", str(PROBE), "-o", str(tmp)], check=True)
        os.replace(tmp, so)
    return C.CDLL(str(so))


def _knobs(knobs):
    return None if knobs is None else (C.c_long * 3)(*knobs)


def header_mode(probe, rows, ncomp, shape, steps, *, bc_program=False, knobs=None, npasses=None):
    """rows: (src, e0, e1, e2, out, faces, second_body) per pass; the mode as `T.loop_route` reports it (None: not the tile kernel)"""
    flat = [int(v) for row in rows[:2] for v in row]
    n = (1,) * (3 - len(shape)) + tuple(shape)
    q = (C.c_long * 7)(len(rows) if npasses is None else npasses, ncomp, len(shape), n[1], n[2], steps, bc_program)
    return probe.jitplan_tile_mode((C.c_long * max(len(flat), 1))(*flat), q, _knobs(knobs)) or None


def rows_of(passes):
    """what the library reads of the descriptors of the package (its handles are made by pdehip_jit_create: no second epilogue)"""
    return [(p.src, *p.extras, p.out, bool(p.faces), False) for p in passes]


def _header_route(probe, eq, state, steps):
    passes, ncomp, program = T.loop_descriptors(eq, state)
    mine = None if program else T.loop_route(passes, ncomp, state.grid.shape, steps)
    assert header_mode(probe, rows_of(passes), ncomp, state.grid.shape, steps, bc_program=program) == mine
    return mine


@pytest.mark.parametrize("item", T.jit_items(), ids=T.jit_item_id)
def test_the_header_routes_every_case_to_its_mode(probe, item):
    (mode, _, _, _), cases = item
    with shimlib.use_shim(fused=False):
        for c in cases:
            eq, state = T.jit_eq(c.mode, c.expr, c.faces), T.state_of(c.mode, c.shape, c.faces, c.dtype)
            assert _header_route(probe, eq, state, c.steps) == T.tile_route(eq, state, c.steps) == mode, c.id


def test_the_header_routes_the_refusals_and_the_launch_rows(probe):
    by_faces = ("second-order-face", "array-face", "tables-of-other-periodicity", "one-cell-axis-of-two-classes")
    with shimlib.use_shim(fused=False):
        for rid, eq, state, _, _, steps in T.refusals():
            mode = _header_route(probe, eq, state, steps)
            assert T.tile_route(eq, state, steps) is None, rid
            # refused by the faces alone: the header has chosen a mode and plan_tile2d declines it
            assert (mode is not None) == (rid in by_faces), rid
        first = {2: "allen_cahn", 3: "brusselator", 4: "swift_hohenberg"}
        rows = [(mode, steps) for mode, steps, _ in T.LAUNCH_ROWS if mode >= 2]       # (modes 0 and 1 are the built-in sweeps: not this loop)
        assert {m for m, _ in rows} == {2, 3, 4}
        for mode, steps in rows:
            eq, state = T.jit_eq(mode, first[mode], "lp"), T.state_of(mode, (33, 70), "lp", "float64")
            assert _header_route(probe, eq, state, steps) == T.tile_route(eq, state, steps) == mode, (mode, steps)


ONE = [(-1, NONE, NONE, NONE, -1, True, False)]
TWO = [(-1, -2, NONE, NONE, -1, True, False), (-2, -1, NONE, NONE, -2, True, False)]
CHAIN = [(-1, NONE, NONE, NONE, 0, True, False), (0, -1, NONE, NONE, -1, True, False)]


def _with(rows, q, **fields):
    names = ("src", "e0", "e1", "e2", "out", "faces", "second_body")
    row = list(rows[q])
    for key, value in fields.items():
        row[names.index(key)] = value
    return [tuple(row) if i == q else r for i, r in enumerate(rows)]


def test_descriptor_tables_the_package_does_not_produce(probe):
    shape = (33, 70)
    ask = lambda rows, ncomp, steps=5, shape=shape, **kw: header_mode(probe, rows, ncomp, shape, steps, **kw)      # noqa: E731
    assert (ask(ONE, 1), ask(TWO, 2), ask(CHAIN, 1)) == (2, 3, 4)
    assert ask(TWO, 2, steps=2) == 3 and ask(_with(TWO, 0, e0=NONE), 2) == 3 and ask(_with(CHAIN, 1, e0=NONE), 1) == 4
    # a handle with a second body, in either pass
    assert ask(_with(ONE, 0, second_body=True), 1) is None
    for table, ncomp in ((TWO, 2), (CHAIN, 1)):
        for q in (0, 1):
            assert ask(_with(table, q, second_body=True), ncomp) is None
    # extras[1] / extras[2] set, a pass without conditions, one field reading itself as e0
    for table, ncomp in ((ONE, 1), (TWO, 2), (CHAIN, 1)):
        for q in range(len(table)):
            assert ask(_with(table, q, e1=0), ncomp) is None and ask(_with(table, q, e2=-1), ncomp) is None
            assert ask(_with(table, q, faces=False), ncomp) is None
    assert ask(_with(ONE, 0, e0=-1), 1) is None and ask(_with(ONE, 0, e0=0), 1) is None
    assert ask(_with(TWO, 0, e0=-1), 2) is None and ask(_with(TWO, 1, e0=0), 2) is None and ask(_with(CHAIN, 0, e0=-1), 1) is None
    # `out` pointing at a fixed array in a one-pass table; the chain broken; the wrong component counts; a third pass
    assert ask(_with(ONE, 0, out=0), 1) is None and ask(_with(ONE, 0, src=0), 1) is None
    assert ask(_with(CHAIN, 1, src=1), 1) is None and ask(_with(CHAIN, 0, out=-1), 1) is None and ask(_with(CHAIN, 1, out=0), 1) is None
    assert ask(ONE, 2) is None and ask(TWO, 1) is None and ask(TWO, 3) is None and ask(CHAIN, 2) is None
    assert ask(_with(TWO, 1, src=-1, out=-1), 2) is None
    assert ask(TWO, 2, npasses=3) is None and ask(CHAIN, 1, npasses=3) is None
    # steps, cells, dimensions, a boundary program
    for table, ncomp in ((ONE, 1), (TWO, 2), (CHAIN, 1)):
        assert ask(table, ncomp, steps=1) is None and ask(table, ncomp, steps=0) is None and ask(table, ncomp, steps=2) is not None
        assert ask(table, ncomp, shape=(2, 1 << 20)) is not None and ask(table, ncomp, shape=(2, (1 << 20) + 1)) is None
        assert ask(table, ncomp, shape=(1 << 21, 1)) is not None and ask(table, ncomp, shape=(2097153,)) is None
        assert ask(table, ncomp, shape=(2, 33, 70)) is None and ask(table, ncomp, shape=(70,)) is None
        assert ask(table, ncomp, bc_program=True) is None
        # each knob: off; a limit of its own, at it and one above; the graph knob does not bear on the tile kernel
        assert ask(table, ncomp, knobs=(0, 1 << 21, 0)) is None and ask(table, ncomp, knobs=(1, 1 << 21, 1)) is not None
        assert ask(table, ncomp, knobs=(1, 33 * 70, 0)) is not None and ask(table, ncomp, knobs=(1, 33 * 70 - 1, 0)) is None


def test_when_the_captured_block_is_replayed(probe):
    """from the third step on, in whole blocks of 16, from four blocks on: 2 + 64 steps"""
    ask = lambda uses_time, steps, comm=False, knobs=(1, 1 << 21, 1): bool(probe.jitplan_replay_applies(uses_time, steps, comm, _knobs(knobs)))   # noqa: E731
    assert [ask(False, n) for n in (65, 66, 67)] == [False, True, True]
    assert [ask(True, n) for n in (65, 66, 67)] == [False, False, False]
    assert [ask(False, n, comm=True) for n in (65, 66, 67)] == [False, False, False]
    assert [ask(False, n, knobs=(1, 1 << 21, 0)) for n in (65, 66, 67)] == [False, False, False]
    assert [ask(False, n, knobs=None) for n in (65, 66, 67, 10 ** 6)] == [False] * 4          # the default: off
    assert ask(False, 66, knobs=(0, 0, 1)) and ask(False, 10 ** 9) and not ask(False, 0) and not ask(False, 1)


def test_the_loop_knobs_are_read_in_one_place(probe):
    assert probe is not None      # (built: the children below load it)
    worker = f"""
import ctypes as C
lib = C.CDLL({str(PROBE.parent / "_build" / "libjitplan_probe.so")!r})
k = (C.c_long * 3)()
lib.jitplan_loop_knobs_from_env(k)
print(list(k))
"""
    def read(**env):
        clean = {k: v for k, v in os.environ.items() if k not in ("PDEHIP_TILE2D", "PDEHIP_TILE2D_CELLS", "PDEHIP_JIT_GRAPH")}
        out = subprocess.run([sys.executable, "-c", worker], env={**clean, **env}, capture_output=True, text=True, check=True).stdout
        return eval(out)      # noqa: S307 - a list of three integers printed above

    assert read() == [1, 1 << 21, 0]
    assert read(PDEHIP_TILE2D="0") == [0, 1 << 21, 0] and read(PDEHIP_TILE2D="off") == [0, 1 << 21, 0] and read(PDEHIP_TILE2D="1") == [1, 1 << 21, 0]
    assert read(PDEHIP_TILE2D_CELLS="4096", PDEHIP_JIT_GRAPH="1") == [1, 4096, 1] and read(PDEHIP_JIT_GRAPH="0") == [1, 1 << 21, 0]
    jit, header = (HEADER.parent / "pdehip_jit.hip").read_text(), HEADER.read_text()
    for knob in ("PDEHIP_TILE2D", "PDEHIP_TILE2D_CELLS", "PDEHIP_JIT_GRAPH"):
        assert f'getenv("{knob}")' not in jit and header.count(f'getenv("{knob}")') == 1
    assert jit.count("jitplan::loop_knobs_from_env()") == 1 and "static const jitplan::LoopKnobs k = jitplan::loop_knobs_from_env();" in jit
