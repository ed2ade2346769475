"""Cases, planner restatement and references for the multi-step 2-D tile kernel (``csrc/pdehip_tile2d.inc``): every mode at both tile widths.

``tile2d_body`` is built in five modes (0 diffusion, 1 Cahn-Hilliard, and the run-time built 2 one generated update, 3 two coupled fields in lockstep,
4 two-pass chain) and two tile widths (32 x 32 and 32 x 64 cells).  Shared by ``tests/test_tile2d_cases_cpu.py`` (CPU: the restatement against
hand-computed rows, and the conditions that keep a case from being vacuous) and ``tests/test_hip_tile2d_instances.py`` (GPU: the kernels against the
references, the instance each launch took by name).  Nothing here touches a device.

Planner.  ``plan_tile2d`` (``csrc/pdehip_kernels_t2.hip``) is reachable from Python only through entry points that launch a kernel, so the rule is
restated here and pinned by hand-computed rows: 64 columns iff ``ceil(cols / 64) * ceil(rows / 32) >= 256``; ``kmax`` = 8 levels per launch, 4 for the
modes with two levels per step (1 and 4); a run of ``steps`` is launched as ``k = min(left, kmax)`` at a time (``pdehip_jit_euler_run``).

References.  Modes 0 and 1: ``O.euler_run`` of the oracle.  Modes 2-4: the tests-only host shim (``shimlib.use_shim(fused=False)``: the oracle's
stencils, gcc for the generated epilogue, one step per loop turn) - it shares no code with the tile kernel.

Conditions.  The reference applies ONE condition per operator NAME in an equation, nested applications included (``pde_hip.rhs.pde_bc_for``).  The two
tables of mode 3 are those of the two fields (``bc_ops`` per field); the two of mode 4 are the conditions of the operator the first pass applies to
the state and of the operator the second pass applies to the temporary - they can differ only where the two operators have different names
(``chain_time`` below: ``gradient_squared`` inside, ``laplace`` outside).  Swift-Hohenberg and the Cahn-Hilliard form nest ``laplace`` in ``laplace``:
both tables are the same one, by the reference's rule.

``laplace(c**3 - c - g*laplace(c)) + 0*c`` is NOT in the table: sympy folds ``0*c`` away, the class matcher (``_match_expression_rhs``) recognises the
Cahn-Hilliard form and ``eq.solve`` takes the hand-written sweeps (mode 1).  ``ch_sink`` (``... - 0.001 * c``) is the form that stays an expression.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import pde_hip
from pde_hip import _abi

TILE_ROWS = 32
HALO = 8
TILE_CELLS_DEFAULT = 1 << 21          # PDEHIP_TILE2D_CELLS
DTYPES = ("float64", "float32")


# ---- the planner, restated ------------------------------------------------------------------------------------------------------
def kmax(mode: int) -> int:
    return HALO // 2 if mode in (1, 4) else HALO


def tile_width(shape) -> int:
    rows, cols = shape
    return 64 if -(-cols // 64) * -(-rows // TILE_ROWS) >= 256 else 32


def tiles(shape) -> tuple[int, int]:
    """(row tiles, column tiles) of the launch"""
    rows, cols = shape
    return -(-rows // TILE_ROWS), -(-cols // tile_width(shape))


def launches(mode: int, steps: int) -> list[int]:
    out, left = [], steps
    while left > 0:
        out.append(min(left, kmax(mode)))
        left -= out[-1]
    return out


def kernel_name(dtype, mode: int, shape, k: int) -> str:
    """``pdehip_last_kernel_name`` after a launch of ``k`` levels (exact build)"""
    tname = "double" if np.dtype(dtype) == np.float64 else "float"
    name = f"tile2d_kernel<{tname},mode={mode},32x{tile_width(shape)} tile> ({k} steps per launch, time levels in LDS"
    return name + ("; run-time built)" if mode >= 2 else ")")


def last_kernel_name(dtype, mode: int, shape, steps: int) -> str:
    return kernel_name(dtype, mode, shape, launches(mode, steps)[-1])


def seams(shape) -> tuple[bool, bool]:
    """(a seam between two row tiles exists, ... two column tiles)"""
    tr, tc = tiles(shape)
    return tr > 1, tc > 1


# shape, tile width, (row tiles, column tiles), cells of the last row tile, cells of the last tile column: computed by hand
PLAN_ROWS = [
    ((33, 8130), 64, (2, 128), 1, 2),
    ((4065, 70), 64, (128, 2), 1, 6),
    ((481, 961), 64, (16, 16), 1, 1),
    ((32, 8130), 32, (1, 255), 32, 2),       # 1 x 128 tiles of 64 columns: one short of the rule
    ((1024, 1024), 64, (32, 16), 32, 64),    # BASELINE config 2
    ((512, 512), 32, (16, 16), 32, 32),      # config 3: 128 tiles of 64 columns
    ((64, 64), 32, (2, 2), 32, 32),
    ((33, 70), 32, (2, 3), 1, 6),
    ((100, 130), 32, (4, 5), 4, 2),
    ((31, 129), 32, (1, 5), 31, 1),
    ((5, 7), 32, (1, 1), 5, 7),
    ((1, 9), 32, (1, 1), 1, 9),
    ((9, 1), 32, (1, 1), 9, 1),
    ((2, 1048577), 64, (1, 16385), 2, 1),
]
LAUNCH_ROWS = [(0, 8, [8]), (0, 9, [8, 1]), (2, 19, [8, 8, 3]), (3, 2, [2]), (3, 3, [3]), (1, 4, [4]), (4, 5, [4, 1]), (4, 11, [4, 4, 3]), (1, 1, [1])]

WIDE_SHAPES = [(33, 8130), (4065, 70), (481, 961)]      # 2 x 128, 128 x 2, 16 x 16 tiles of 32 x 64
CONTRAST_SHAPE = (32, 8130)                             # one tile short: 32 x 32 tiles
NARROW_SHAPES = [(64, 64), (33, 70), (100, 130), (31, 129)]
TINY_SHAPES = [(5, 7), (1, 9), (9, 1)]                  # smaller than the halo

# ---- conditions: the five combinations of test_hip_tile2d.py, and a second table of the same periodicity ---------------------------
PERIODIC = {"pp": (True, True), "pl": (True, False), "lp": (False, True), "ll": (False, False), "nn": (False, False)}
FACE_NAMES = tuple(PERIODIC)


def table(faces: str, second: bool = False, bump: float = 0.0):
    """The conditions of a combination; ``second``: other coefficients, the same periodicity; ``bump``: one face constant moved"""
    if faces in ("pp", "nn") and not second and not bump:
        return "auto_periodic_neumann"
    if faces == "pp":
        return {"x": "periodic", "y": "periodic"}
    if faces == "nn":
        return {"x": {"derivative": 0.1 + bump}, "y": {"derivative": -0.15}} if second else {"x": {"derivative": bump}, "y": {"derivative": 0.0}}
    out = {}
    if PERIODIC[faces][0]:
        out["x"] = "periodic"
    elif second:
        out.update({"x-": {"derivative": 0.3}, "x+": {"type": "mixed", "value": 0.6, "const": -0.1}})
    else:
        out.update({"x-": {"value": 0.4}, "x+": {"derivative": -0.2}})
    if PERIODIC[faces][1]:
        out["y"] = "periodic"
    elif second:
        out.update({"y-": {"value": -0.2 + bump}, "y+": {"derivative": 0.15}})
    else:
        out.update({"y-": {"type": "mixed", "value": 0.5, "const": 0.2}, "y+": {"value": -0.3 + bump}})
    if not PERIODIC[faces][0] and bump:      # (one constant of the lower x face as well: the bumped table differs on every local axis)
        key = "x-"
        out[key] = dict(out[key])
        name = "derivative" if "derivative" in out[key] else "value"
        out[key][name] += bump
    return out


BUMP = 0.05


def make_grid(shape, faces):
    return pde_hip.CartesianGrid([[0, 1.0 * shape[0]], [0, 0.9 * shape[1]]], shape, periodic=list(PERIODIC[faces]))


# ---- modes 0 and 1 through pdehip_euler_multi_2d -------------------------------------------------------------------------------------
KINDS = {"diffusion": (0, 0.7, 0.05), "cahn_hilliard": (1, 0.9, 1e-3)}     # mode, parameter, dt
BUILTIN_SHAPES = [*WIDE_SHAPES, CONTRAST_SHAPE]


def builtin_steps(kind: str) -> list[int]:
    return sorted({1, 2, 3, kmax(KINDS[kind][0])})


def builtin_items():
    """(shape, faces, kind, dtype): each runs K in {1, 2, 3, kmax}"""
    return [(shape, faces, kind, dtype) for shape in BUILTIN_SHAPES for faces in FACE_NAMES for kind in KINDS for dtype in DTYPES]


def builtin_id(item) -> str:
    shape, faces, kind, dtype = item
    return f"{shape[0]}x{shape[1]}-{faces}-{kind}-{dtype}"


def field_data(shape, dtype, seed: int = 3, centre: float = 0.0):
    return (centre + np.random.default_rng([seed, *shape]).uniform(-0.4, 0.4, shape)).astype(dtype)


def builtin_eq(kind, faces, bump: float = 0.0):
    """Cahn-Hilliard: the second table for mu"""
    if kind == "diffusion":
        return pde_hip.DiffusionPDE(KINDS[kind][1], bc=table(faces, bump=bump))
    return pde_hip.CahnHilliardPDE(KINDS[kind][1], bc_c=table(faces, bump=bump), bc_mu=table(faces, second=True))


def oracle_levels(shape, faces, kind, dtype, data, steps, bump: float = 0.0):
    """{K: valid cells after K single steps of the oracle} for the K in ``steps`` (ascending; one run, continued)"""
    from helpers import host_faces, interior, oracle_grid, to_full
    from oracle import pde_oracle as O

    grid = make_grid(shape, faces)
    mode, param, dt = KINDS[kind]
    g = oracle_grid(grid, np.dtype(dtype))
    scratch = np.zeros(grid._shape_full, np.dtype(dtype))
    fc = host_faces(grid.get_boundary_conditions(table(faces, bump=bump)))
    fm = host_faces(grid.get_boundary_conditions(table(faces, second=True) if mode == 1 else table(faces, bump=bump)))
    rhs = O.make_rhs(_abi.RHS_CAHN_HILLIARD if mode == 1 else _abi.RHS_DIFFUSION, param, fc.c, fm.c, scratch)
    full, out, at = to_full(grid, data), {}, 0
    for k in steps:
        full = O.euler_run(g, rhs, full, dt, k - at)
        at = k
        out[k] = interior(grid, full).copy()
    return out


# special values through modes 0 and 1: both 64-column geometries and a 32-column one, local faces on both axes
SPECIAL_SHAPES = [(33, 8130), (481, 961), (40, 200)]
SPECIAL_IDS = ["32x64-two-rows", "32x64", "32x32"]
SPECIAL_FACES = "ll"
SPECIAL_VALUES = {"float64": dict(tiny=4.9e-324, small=1e-307, huge=1e300), "float32": dict(tiny=1e-45, small=1e-37, huge=1e38)}


def special_data(shape, dtype):
    """(data, planted cells): ordinary data with an infinity, a NaN, huge magnitudes, the smallest denormals and signed zeros planted on the last
    row of a row tile and the first of the next, on both sides of a column seam, next to the four faces and inside a tile - and a band of small
    magnitudes, 40 columns over all rows (in the wide shapes across the next column seam), in whose middle every level is denormal.  A value
    spreads 8 cells in kmax levels: the groups are 17 columns apart at least, most of the grid stays finite."""
    n0, n1 = shape
    width = tile_width(shape)
    data = field_data(shape, dtype, seed=31)
    v = SPECIAL_VALUES[dtype]
    values = [np.inf, np.nan, v["huge"], -v["huge"], v["tiny"], -v["tiny"], 0.0, -0.0]
    seam_r, seam_c = TILE_ROWS, width * (n1 // width // 2)
    assert seam_r < n0 and 0 < seam_c and seam_c + 64 < n1
    rows = sorted({0, seam_r - 1, seam_r, n0 - 1, 15})
    cols = sorted({0, seam_c - 1, seam_c, n1 - 1, seam_c + 17})
    spots = [(r, c) for r in rows for c in cols]
    for i, (r, c) in enumerate(spots):
        data[r, c] = values[i % len(values)]
    data[:, seam_c + 24:seam_c + 64] *= np.dtype(dtype).type(v["small"])
    return data, spots


# ---- modes 2-4 through eq.solve ---------------------------------------------------------------------------------------------------
EXPRESSIONS = {
    2: {"allen_cahn": {"c": "c - c**3 + laplace(c)"},
        "stencil": {"c": "0.3 * laplace(c) + 0.5 * gradient_squared(c) - c * d_dx(c) + 0.1 * d2_dy2(c)"},     # every stencil input
        "time": {"c": "c - c**3 + laplace(c) + 0.01 * sin(t)"}},
    3: {"brusselator": {"u": "laplace(u) + 1 - 4 * u + v * u**2", "v": "0.1 * laplace(v) + 3 * u - v * u**2"},
        "one_way": {"u": "laplace(u) - u * d_dx(u)", "v": "0.1 * laplace(v) + gradient_squared(v) - u + 2 * t"}},   # u ignores v
    4: {"swift_hohenberg": {"c": "(0.1 - 1) * c - 0.2 * laplace(c) - 0.01 * laplace(laplace(c)) - c**3"},
        "ch_sink": {"c": "laplace(c**3 - c - 0.01 * laplace(c)) - 0.001 * c"},
        "chain_time": {"c": "laplace(0.5 * c - 0.1 * gradient_squared(c)) - 0.2 * c + 5 * t"}},
}
# `time` keeps `sin(t)` (it agrees in all its cases); a transcendental function of t ties an fp64 comparison with the host shim to two math libraries agreeing in the last
# place (with `0.2 * sin(30 * t)` in `one_way` one cell of one case differed by one unit in the last place, from the one-level kernels alike), so the
# two other expressions read t through exactly rounded operations only
READS_TIME = ("time", "one_way", "chain_time")
TWO_NAMES = ("chain_time",)                 # mode 4: the operators of the two passes have different names
WIDE_EXPRESSION = {2: "stencil", 3: "brusselator", 4: "chain_time"}      # the expression that also runs the 64-column shapes
DT = {2: 0.01, 3: 0.01, 4: 1e-3}
T_START = 0.7


def jit_steps(mode: int) -> list[int]:
    k = kmax(mode)
    return [2, 3, k, k + 1, 2 * k + 3]


@dataclass(frozen=True)
class Case:
    mode: int
    expr: str
    shape: tuple
    faces: str
    dtype: str
    steps: int

    @property
    def id(self) -> str:
        return f"m{self.mode}-{self.expr}-{self.shape[0]}x{self.shape[1]}-{self.faces}-{self.dtype}-{self.steps}"

    @property
    def t_start(self) -> float:
        return T_START if self.expr in READS_TIME else 0.0

    @property
    def dt(self) -> float:
        return DT[self.mode]

    @property
    def tables_differ(self) -> bool:
        return self.faces != "pp" and (self.mode == 3 or self.expr in TWO_NAMES)

    @property
    def name(self) -> str:
        return last_kernel_name(self.dtype, self.mode, self.shape, self.steps)


def _jit_cases() -> list[Case]:
    """A designed subset of the product: every expression on every narrow and tiny shape in both types, faces and step counts rotated so that each
    (mode, faces) and each (mode, step count) appears, twice over the rotation; the 64-column shapes and the contrast shape with one expression per
    mode (a run-time build per expression, type and tile width costs a second)."""
    out = []
    for mode, exprs in EXPRESSIONS.items():
        steps = jit_steps(mode)
        for d, dtype in enumerate(DTYPES):
            for i, expr in enumerate(exprs):
                shapes = [*NARROW_SHAPES, *TINY_SHAPES]
                for j, shape in enumerate(shapes):
                    for turn in (0, 1):
                        faces = FACE_NAMES[(i + j + d + 2 * turn) % 5]
                        if faces == "nn" and min(shape) == 1 and (mode == 3 or expr in TWO_NAMES):
                            # a one-cell axis with a zero-derivative face on both sides IS periodic to `classify_axis` (index 0 on both sides,
                            # c = 0, f = 1), the second table's non-zero derivative is local: the planner refuses tables of two classes
                            faces = "ll"
                        out.append(Case(mode, expr, shape, faces, dtype, steps[(2 * i + j + d + 3 * turn) % 5]))
                if expr == WIDE_EXPRESSION[mode]:
                    for j, shape in enumerate([*WIDE_SHAPES, CONTRAST_SHAPE]):
                        # local faces on the axis with many tiles first; the longest run (a second and a third launch) on the smallest of them
                        faces = ("pl", "lp", "ll", "nn")[(j + d) % 4] if j < 3 else ("pp", "ll")[d]
                        out.append(Case(mode, expr, shape, faces, dtype, steps[(4 - j + d) % 5]))
    return out


JIT_CASES = _jit_cases()


def jit_items():
    """The cases in groups of one run-time build (expression, type, tile width): one pytest item each"""
    groups: dict[tuple, list[Case]] = {}
    for c in JIT_CASES:
        groups.setdefault((c.mode, c.expr, c.dtype, tile_width(c.shape)), []).append(c)
    return list(groups.items())


def jit_item_id(item) -> str:
    (mode, expr, dtype, width), _ = item
    return f"m{mode}-{expr}-{dtype}-32x{width}"


def state_of(mode, shape, faces, dtype):
    grid = make_grid(shape, faces)
    if mode == 3:
        return pde_hip.FieldCollection([pde_hip.ScalarField(grid, field_data(shape, dtype, 5, 1.0), dtype=np.dtype(dtype)),
                                        pde_hip.ScalarField(grid, field_data(shape, dtype, 6, 3.0), dtype=np.dtype(dtype))])
    return pde_hip.ScalarField(grid, field_data(shape, dtype), dtype=np.dtype(dtype))


@lru_cache(maxsize=None)
def jit_eq(mode: int, expr: str, faces: str, variant: str = "plain"):
    """The equation of a case.  ``variant``: "bump" moves a face constant of the FIRST table, "bump2" of the second, "swap" exchanges the tables."""
    first = table(faces, bump=BUMP if variant == "bump" else 0.0)
    second = table(faces, second=True, bump=BUMP if variant == "bump2" else 0.0)
    if variant == "swap":
        first, second = second, first
    rhs = EXPRESSIONS[mode][expr]
    if mode == 2:
        return pde_hip.PDE(rhs, bc=first)
    if mode == 3:
        return pde_hip.PDE(rhs, bc=first, bc_ops={"u:*": first, "v:*": second})
    if expr in TWO_NAMES:
        return pde_hip.PDE(rhs, bc=first, bc_ops={"c:laplace": second})      # the temporary's conditions; `first` for the operator on the state
    return pde_hip.PDE(rhs, bc=first)                                        # laplace nested in laplace: one table for both passes


def solve(eq, state, t_start: float, dt: float, steps: int):
    """``steps`` Euler steps through ``eq.solve`` with whatever library is installed (the device's, or the shim inside ``use_shim``)"""
    res, info = eq.solve(state, t_range=(t_start, t_start + steps * dt), dt=dt, solver="euler", backend="hip", tracker=None, ret_info=True)
    assert info["solver"]["steps"] == steps, (info["solver"]["steps"], steps)
    return np.array(res.data)


def shim_solve(eq, state, t_start: float, dt: float, steps: int):
    import shimlib

    with shimlib.use_shim(fused=False):
        return solve(eq, state, t_start, dt, steps)


def jit_reference(case: Case, variant: str = "plain", t_start: float | None = None):
    return shim_solve(jit_eq(case.mode, case.expr, case.faces, variant), state_of(case.mode, case.shape, case.faces, case.dtype),
                      case.t_start if t_start is None else t_start, case.dt, case.steps)


# ---- what pdehip_jit_euler_run accepts for the tile kernel, restated from the pass descriptors -------------------------------------
def classify_passes(passes, ncomp: int):
    """mode 2 / 3 / 4 of a list of ``pdehip_jit_pass_t`` (``_abi.JitPass``), or None: the predicates `one`, `two`, `chain` of pdehip_jit_euler_run
    (except that a pass carries no second epilogue: not visible from here)"""
    none = lambda v: v == _abi.JIT_NONE    # noqa: E731
    ex = lambda p: list(p.extras)          # noqa: E731

    def own(p, comp, other):
        return p.src == -1 - comp and p.out == -1 - comp and (none(ex(p)[0]) or ex(p)[0] == -1 - other) and none(ex(p)[1]) and none(ex(p)[2]) and bool(p.faces)

    n = len(passes)
    if n == 1 and ncomp == 1 and own(passes[0], 0, 0) and none(ex(passes[0])[0]):
        return 2
    if n == 2 and ncomp == 2 and own(passes[0], 0, 1) and own(passes[1], 1, 0):
        return 3
    if n == 2 and ncomp == 1:
        p, q = passes
        if (p.src == -1 and p.out >= 0 and all(none(v) for v in ex(p)) and bool(p.faces) and q.src == p.out and q.out == -1
                and (none(ex(q)[0]) or ex(q)[0] == -1) and none(ex(q)[1]) and none(ex(q)[2]) and bool(q.faces)):
            return 4
    return None


def face_class(faces_ptr, axis: int, n: int):
    """``classify_axis`` on the table of a pass: 1 periodic, 0 local, -1 neither; None when the planner refuses the table (not first order, or
    coefficient arrays)"""
    f = C.cast(faces_ptr, C.POINTER(_abi.BCFace))
    lo, hi = f[2 * axis], f[2 * axis + 1]
    for r in (lo, hi):
        if r.kind != _abi.BC_ORDER1 or r.flags != 0 or not 0 <= r.index1 < n:
            return None
    if lo.index1 == n - 1 and hi.index1 == 0 and lo.const_v == 0 and hi.const_v == 0 and lo.factor1 == 1 and hi.factor1 == 1:
        return 1
    return 0 if lo.index1 == 0 and hi.index1 == n - 1 else -1


def tile_route(eq, state, steps: int):
    """The mode in which the Euler loop of ``eq`` takes the tile kernel for ``steps`` steps, or None - decided as pdehip_jit_euler_run and
    plan_tile2d decide it, from the pass descriptors the package hands to the library.  Call inside ``shimlib.use_shim``."""
    desc = loop_descriptors(eq, state)
    if desc is None or desc[2]:
        return None
    passes, ncomp, _ = desc
    shape = state.grid.shape
    mode = loop_route(passes, ncomp, shape, steps)
    if mode is None:
        return None
    classes = [[face_class(p.faces, a, shape[a]) for a in range(2)] for p in passes]
    if any(c is None or c < 0 for cl in classes for c in cl) or any(cl != classes[0] for cl in classes):
        return None
    return mode


def loop_descriptors(eq, state):
    """(passes, components, "has a boundary program") as the package hands them to pdehip_jit_euler_run, or None where it does not call it.
    Call inside ``shimlib.use_shim``."""
    backend = pde_hip.get_backend("hip")
    erhs = backend.make_expression_rhs(eq, state)
    if not erhs.has_loops:
        return None
    parts = getattr(erhs, "parts", None) or [erhs]
    if not all(p.loop_ok() for p in parts):
        return None
    return list(erhs.loop_desc("euler")[0]), len(parts) if getattr(erhs, "parts", None) else 1, erhs.bc_program() is not None


def loop_route(passes, ncomp: int, shape, steps: int, cells: int = TILE_CELLS_DEFAULT):
    """The part of `tile_route` that ``jitplan::tile_mode`` (csrc/pdehip_jit_plan.h) decides: everything but the classes of the faces."""
    mode = classify_passes(passes, ncomp)
    if mode is None or len(shape) != 2 or shape[0] * shape[1] > cells or steps < 2:
        return None
    return mode


# ---- cases that must NOT take the tile kernel (and still give the reference's result) -----------------------------------------------
def refusals():
    """[(id, equation, state, t_start, dt, steps)]"""
    ac, br = EXPRESSIONS[2]["allen_cahn"], EXPRESSIONS[3]["brusselator"]
    out = []
    thin = (2, 1048577)       # 2 097 154 cells: two more than the default of PDEHIP_TILE2D_CELLS
    out.append(("more-cells-than-the-limit", pde_hip.PDE(ac, bc=table("pl")), state_of(2, thin, "pl", "float64"), 0.0, DT[2], 3))
    out.append(("one-step", jit_eq(3, "brusselator", "ll"), state_of(3, (33, 70), "ll", "float64"), 0.0, DT[3], 1))
    out.append(("one-step-chain", jit_eq(4, "swift_hohenberg", "lp"), state_of(4, (33, 70), "lp", "float64"), 0.0, DT[4], 1))
    out.append(("second-order-face", pde_hip.PDE(ac, bc={"x": "extrapolate", "y": "periodic"}), state_of(2, (33, 70), "lp", "float64"), 0.0, DT[2], 5))
    out.append(("array-face", pde_hip.PDE(ac, bc={"x": {"value": np.linspace(0, 1, 70)}, "y": "periodic"}), state_of(2, (33, 70), "lp", "float64"), 0.0, DT[2], 5))
    out.append(("tables-of-other-periodicity", pde_hip.PDE(br, bc_ops={"u:*": table("lp"), "v:*": {**table("lp", second=True), "y": "anti-periodic"}}),
                state_of(3, (33, 70), "lp", "float64"), 0.0, DT[3], 5))
    # (see _jit_cases: the zero-derivative faces of a one-cell axis count as periodic, the second field's do not)
    out.append(("one-cell-axis-of-two-classes", jit_eq(3, "one_way", "nn"), state_of(3, (9, 1), "nn", "float64"), T_START, DT[3], 5))
    return out
