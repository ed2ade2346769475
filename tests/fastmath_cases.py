"""Reference, rounding-error bound and case table of the contracted build (`pdehip_set_fastmath`, ``pdehip::fastv``) - pure numpy, no GPU.

The stencil translation units are compiled twice: with ``-ffp-contract=off`` (bit-identical to the oracle) and with ``-ffp-contract=fast``.
Contraction fuses a product with the sum it feeds into one FMA: one rounding is REMOVED, nothing is reordered.  So whichever subset of the
multiply-adds a compiler fuses, the result stays inside the running error bound of the oracle's own expression, evaluated operation by operation:

    add / sub   e = ea + eb + u |v|
    mul         e = |a| eb + |b| ea + ea eb + u |v|          u = 2**-53
    store       e += 2**-24 (|v| + e) for fp32 storage, nothing for fp64

with ``v`` carried in ``np.longdouble`` (64 bits of mantissa).  Plain floats are exact constants.  Three operations are exact in IEEE
arithmetic whatever is fused around them and add no rounding term: the product with 0, +-1 or +-2, and the sum with an exact 0
(``0 + 1 * x`` of a periodic ghost cell, ``2 * mid`` of the Laplacian).  A quotient by an exact constant rounds once (``e = ea / |c| + u |v|``).
No tolerance is chosen by hand anywhere: `excess` / `within` compare ``|got - reference| <= bound`` cell by cell.

The reference functions restate ``oracle/pde_oracle_impl.inc`` / ``oracle/pde_oracle.c`` in their expression order with that class; multi-step and
nonlinear cases (Cahn-Hilliard, Runge-Kutta) need no derivation of their own, the class carries the propagation.  tests/test_fastmath_cases_cpu.py
ties every case to the pinned oracle and to a really contracted CPU build; tests/test_hip_fastmath_instances.py runs the table on the device.
"""

from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import itertools
import json

import numpy as np
from helpers import GOLDEN, face_mask, host_faces, interior, load_cases, make_grid, oracle_grid, to_full

import pde_hip
from oracle import pde_oracle as O
from pde_hip import _abi

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference of the contracted build needs an extended-precision np.longdouble (64-bit mantissa)"

U = LD(2) ** -53
U32 = LD(2) ** -24


# ---------------------------------------------------------------------------------------------------------------------------------
# running-error arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
class RE:
    """Array of values ``v`` (longdouble) with a bound ``e`` on |computed - v| for any IEEE evaluation of the same expression in fp64, fused or not."""

    __slots__ = ("v", "e")
    __array_ufunc__ = None      # numpy scalars / arrays on the left hand side defer to __radd__ & co

    def __init__(self, v, e=None):
        self.v = np.array(v, dtype=LD)
        self.e = np.zeros(self.v.shape, LD) if e is None else np.array(np.broadcast_to(np.asarray(e, dtype=LD), self.v.shape), dtype=LD)

    @staticmethod
    def _const(c):
        assert not isinstance(c, RE)
        return np.asarray(c, dtype=LD)     # fp64 -> longdouble is exact

    # -- sums ------------------------------------------------------------------------------------------------------------------
    def __add__(self, o):
        if isinstance(o, RE):
            v = self.v + o.v
            return RE(v, self.e + o.e + U * np.abs(v))
        c = self._const(o)
        v = self.v + c
        return RE(v, self.e + U * np.abs(v) * (c != 0))          # x + 0 is exact

    __radd__ = __add__

    def __neg__(self):
        return RE(-self.v, self.e)

    def __sub__(self, o):
        return self + (-o if isinstance(o, RE) else -self._const(o))

    def __rsub__(self, o):
        return (-self) + self._const(o)

    # -- products --------------------------------------------------------------------------------------------------------------
    def __mul__(self, o):
        if isinstance(o, RE):
            v = self.v * o.v
            return RE(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e + U * np.abs(v))
        c = self._const(o)
        v = self.v * c
        ac = np.abs(c)
        rounds = ~((ac == 0) | (ac == 1) | (ac == 2))              # those products are exact
        return RE(v, ac * self.e + U * np.abs(v) * rounds)

    __rmul__ = __mul__

    def __truediv__(self, o):
        c = self._const(o)
        v = self.v / c
        return RE(v, self.e / np.abs(c) + U * np.abs(v))

    # -- array plumbing --------------------------------------------------------------------------------------------------------
    def __getitem__(self, key):
        return RE(self.v[key], self.e[key])

    def __setitem__(self, key, o):
        self.v[key], self.e[key] = o.v, o.e

    @property
    def shape(self):
        return self.v.shape

    def roll(self, shift, axis):
        return RE(np.roll(self.v, shift, axis), np.roll(self.e, shift, axis))

    def store(self, dtype):
        """the rounding to the array's type: ``po[k] = (REAL)r``"""
        if np.dtype(dtype) == np.float32:
            return RE(self.v, self.e + U32 * (np.abs(self.v) + self.e))      # the rounding acts on the computed value, |v| + e at most
        return RE(self.v, self.e)


def stack(items):
    return RE(np.stack([r.v for r in items]), np.stack([r.e for r in items]))


# ---------------------------------------------------------------------------------------------------------------------------------
# reference functions (native number of axes; `full` arrays carry one ghost layer per axis)
# ---------------------------------------------------------------------------------------------------------------------------------
LO, MID, HI = slice(0, -2), slice(1, -1), slice(2, None)


def _sl(nd, axis, s):
    """index of the cells at `s` along `axis`, interior cells along the other axes (any leading component axes kept)"""
    return (Ellipsis,) + tuple(s if a == axis else MID for a in range(nd))


def read_faces(table, shape, lead=()):
    """the C face table as plain Python: [{kind, normal, i1, i2, const, f1, f2}] in table order (axis 0 lower, upper, axis 1 ...)"""
    out = []
    for a in range(len(shape)):
        face_shape = tuple(n for j, n in enumerate(shape) if j != a)
        for side in range(2):
            f = table[2 * a + side]
            d = {"kind": int(f.kind), "normal": bool(f.flags & _abi.BCF_NORMAL), "i1": int(f.index1), "i2": int(f.index2),
                 "const": float(f.const_v), "f1": float(f.factor1), "f2": float(f.factor2), "arrays": bool(f.flags & _abi.BCF_ARRAYS)}
            if d["arrays"]:
                target = (() if d["normal"] else tuple(lead)) + face_shape
                count = int(np.prod(target))

                def rd(ptr):
                    return np.ctypeslib.as_array((C.c_double * count).from_address(ptr)).reshape(target).copy()

                d["const"], d["f1"] = rd(f.const_arr), rd(f.factor1_arr)
                d["f2"] = rd(f.factor2_arr) if f.kind == _abi.BC_ORDER2 else 0.0
            out.append(d)
    return out


def ref_ghosts(x: RE, faces, nd, dtype):
    """ghost_kernel: ``const + factor1 * v[index1] (+ factor2 * v[index2])`` per face cell, axis by axis, upper face first; in place"""
    lead = x.v.ndim - nd
    n_full = x.shape[lead:]
    for a in range(nd):
        for side in (1, 0):
            f = faces[2 * a + side]
            if f["kind"] == _abi.BC_SKIP:
                continue
            ghost = n_full[a] - 1 if side else 0
            for comp in ([None] if lead == 0 else range(x.shape[0])):
                if f["normal"] and comp != a:
                    continue
                pre = () if comp is None else (comp,)

                def coef(c):
                    return c[comp] if (isinstance(c, np.ndarray) and comp is not None and not f["normal"]) else c

                def at(i):
                    return pre + _sl(nd, a, i)[1:]

                r = coef(f["const"]) + coef(f["f1"]) * x[at(f["i1"] + 1)]
                if f["kind"] == _abi.BC_ORDER2:
                    r = r + coef(f["f2"]) * x[at(f["i2"] + 1)]
                x[at(ghost)] = r.store(dtype)
    return x


def lap_scales(dx):
    return [float(d) ** -2.0 for d in dx]       # norm_grid: pow(dx, -2.0)


def ref_lap(x: RE, dx):
    """lap_rows: the plain Laplacian of a full array on its valid cells"""
    nd = x.v.ndim
    s = lap_scales(dx)
    mid = x[_sl(nd, 0, MID)]

    def nb(a, w):
        return x[_sl(nd, a, w)]

    if nd == 1:
        return (nb(0, LO) - 2 * mid + nb(0, HI)) * s[0]
    if nd == 2:
        lx = (nb(0, LO) - 2 * mid + nb(0, HI)) * s[0]
        ly = (nb(1, LO) - 2 * mid + nb(1, HI)) * s[1]
        return lx + ly
    vm = 2 * mid                                   # :220-227 val_mid hoisted
    lx = (nb(0, LO) - vm + nb(0, HI)) * s[0]
    ly = (nb(1, LO) - vm + nb(1, HI)) * s[1]
    lz = (nb(2, LO) - vm + nb(2, HI)) * s[2]
    return lx + ly + lz


def embed(valid: RE, dtype):
    """a full array (ghost cells zero) whose valid cells are `valid` rounded to the array's type"""
    nd = valid.v.ndim
    full = RE(np.zeros(tuple(n + 2 for n in valid.shape), LD))
    full[_sl(nd, 0, MID)] = valid.store(dtype)
    return full


def ref_lap_mode(x: RE, dx, mode, s1=0.0, s2=0.0, gamma=0.0, y: RE | None = None):
    """the four epilogues of lap_rows on the valid cells (before the store)"""
    lap = ref_lap(x, dx)
    if mode == "plain":
        return lap
    if mode == "scaled":
        return s2 * (s1 * lap)
    nd = x.v.ndim
    if mode == "euler":
        return y[_sl(nd, 0, MID)] + s2 * (s1 * lap)
    mid = x[_sl(nd, 0, MID)]
    return mid * mid * mid - mid - gamma * lap     # cahn_hilliard.py:116-120


def ref_gradient(x: RE, dx, method):
    nd = x.v.ndim
    out = []
    for a in range(nd):
        hi, lo, mid = x[_sl(nd, a, HI)], x[_sl(nd, a, LO)], x[_sl(nd, a, MID)]
        d = hi - lo if method == "central" else (hi - mid if method == "forward" else mid - lo)
        if nd == 1:
            out.append(d / (2 * dx[a]) if method == "central" else d / dx[a])
        else:
            out.append(d * (0.5 / dx[a] if method == "central" else 1 / dx[a]))
    return stack(out)


def ref_divergence(x: RE, dx, method):
    nd = x.v.ndim - 1
    acc = None
    for a in range(nd):
        c = x[a]
        hi, lo, mid = c[_sl(nd, a, HI)], c[_sl(nd, a, LO)], c[_sl(nd, a, MID)]
        d = hi - lo if method == "central" else (hi - mid if method == "forward" else mid - lo)
        if nd == 1:
            t = d / (2 * dx[a]) if method == "central" else d / dx[a]
        else:
            t = d * (0.5 / dx[a] if method == "central" else 1 / dx[a])
        acc = t if acc is None else acc + t
    return acc


def ref_gradient_squared(x: RE, dx, central):
    nd = x.v.ndim
    acc = None
    for a in range(nd):
        hi, lo, mid = x[_sl(nd, a, HI)], x[_sl(nd, a, LO)], x[_sl(nd, a, MID)]
        if central:
            d = hi - lo
            t = d * d * (0.25 / (dx[a] * dx[a]))
        else:
            dl, dr = hi - mid, mid - lo
            t = (dl * dl + dr * dr) * (0.5 / (dx[a] * dx[a]))
        acc = t if acc is None else acc + t
    return acc


def ref_axis_derivative(x: RE, dx, axis, order, method):
    nd = x.v.ndim
    r, l, c = x[_sl(nd, axis, HI)], x[_sl(nd, axis, LO)], x[_sl(nd, axis, MID)]
    h = dx[axis]
    if order == 2:
        return (r - 2 * c + l) * (1 / (h * h))
    if method == "central":
        return (r - l) / (2 * h)
    return (r - c) / h if method == "forward" else (c - l) / h


@dataclasses.dataclass
class Rhs:
    kind: str            # "diffusion" | "cahn_hilliard"
    param: float
    faces_c: list
    faces_mu: list
    dx: tuple
    dtype: np.dtype


def _mu(rhs: Rhs, y: RE):
    nd = y.v.ndim
    ref_ghosts(y, rhs.faces_c, nd, rhs.dtype)
    mu = embed(ref_lap_mode(y, rhs.dx, "ch_mu", gamma=rhs.param), rhs.dtype)
    return ref_ghosts(mu, rhs.faces_mu, nd, rhs.dtype)


def ref_rhs_scaled(rhs: Rhs, y: RE, dt):
    """oracle_rhs_scaled: ghost cells of y (in place), then dt * (D * lap) resp. dt * (1 * lap(mu)) into a full array"""
    if rhs.kind == "diffusion":
        ref_ghosts(y, rhs.faces_c, y.v.ndim, rhs.dtype)
        return embed(ref_lap_mode(y, rhs.dx, "scaled", rhs.param, dt), rhs.dtype)
    return embed(ref_lap_mode(_mu(rhs, y), rhs.dx, "scaled", 1.0, dt), rhs.dtype)


def ref_euler_step(rhs: Rhs, y: RE, dt):
    """one pass of oracle_euler_run: y + dt * (D * lap(y)) resp. y + dt * (1 * lap(mu))"""
    if rhs.kind == "diffusion":
        ref_ghosts(y, rhs.faces_c, y.v.ndim, rhs.dtype)
        return embed(ref_lap_mode(y, rhs.dx, "euler", rhs.param, dt, y=y), rhs.dtype)
    return embed(ref_lap_mode(_mu(rhs, y), rhs.dx, "euler", 1.0, dt, y=y), rhs.dtype)


def ref_euler_run(rhs: Rhs, y: RE, dt, steps):
    for _ in range(steps):
        y = ref_euler_step(rhs, y, dt)
    return y


def ref_lincomb(y: RE, coefs, ks, dtype):
    r = y
    for c, k in zip(coefs, ks):
        r = r + c * k
    return r.store(dtype)


def ref_rk4_step(rhs: Rhs, y: RE, dt):
    """oracle_rk4_step; runge_kutta.py:60  state += (k1 + 2*k2 + 2*k3 + k4) / 6"""
    k1 = ref_rhs_scaled(rhs, y, dt)
    k2 = ref_rhs_scaled(rhs, ref_lincomb(y, [0.5], [k1], rhs.dtype), dt)
    k3 = ref_rhs_scaled(rhs, ref_lincomb(y, [0.5], [k2], rhs.dtype), dt)
    k4 = ref_rhs_scaled(rhs, ref_lincomb(y, [1.0], [k3], rhs.dtype), dt)
    s = (k1 + 2 * k2 + 2 * k3 + k4) / 6
    return (y + s).store(rhs.dtype)


RK_B = [[1.0 / 4], [3.0 / 32, 9.0 / 32], [1932.0 / 2197, -7200.0 / 2197, 7296.0 / 2197], [439.0 / 216, -8.0, 3680.0 / 513, -845.0 / 4104],
        [-8.0 / 27, 2.0, -3544.0 / 2565, 1859.0 / 4104, -11.0 / 40]]
RK_R = {0: 1.0 / 360, 2: -128.0 / 4275, 3: -2197.0 / 75240, 4: 1.0 / 50, 5: 2.0 / 55}
RK_C = {0: 25.0 / 216, 2: 1408.0 / 2565, 3: 2197.0 / 4104, 4: -1.0 / 5}


def ref_rkf45_attempt(rhs: Rhs, y: RE, dt):
    """oracle_rkf45_attempt: (new state, error estimate = max |e| over the valid cells); |max|a| - max|b|| <= max|a - b|"""
    ks = [ref_rhs_scaled(rhs, y, dt)]
    for b in RK_B:
        ks.append(ref_rhs_scaled(rhs, ref_lincomb(y, b, ks, rhs.dtype), dt))
    e = None
    for q, c in RK_R.items():
        e = c * ks[q] if e is None else e + c * ks[q]
    new = y
    for q, c in RK_C.items():
        new = new + c * ks[q]
    inner = _sl(y.v.ndim, 0, MID)
    e = e[inner]
    return new.store(rhs.dtype), RE(np.abs(e.v).max(), e.e.max())


# ---------------------------------------------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("launch_laplace", "launch_deriv_march", "launch_div_march", "launch_ghosts", "launch_euler2", "launch_euler4", "launch_tile2d")
# pdehip_axis_derivative has ONE build (csrc/pdehip_ops.hip): its reference is checked on the CPU, the device must give the oracle's bits in both modes
SINGLE_BUILD = "axis_derivative"
CZ2_SHAPES = [(32, 32, 192), (32, 32, 130), (32, 32, 131), (1024, 130)]
TILE2D_MAX_STEPS = {"diffusion": 8, "cahn_hilliard": 4}      # test_hip_tile2d.py: kmax


@dataclasses.dataclass(frozen=True)
class Case:
    family: str
    entry: str                 # C entry point (or the variant of it) the device test calls
    shape: tuple
    dtype: str                 # "float64" | "float32"
    bounds: tuple              # ((lo, hi), ...) - the spacing
    periodic: tuple
    bc: tuple                  # how the faces are built: see `_faces_of`
    kind: str = "diffusion"
    param: float = 0.0
    dt: float = 0.0
    steps: int = 1
    seed: int = 3
    bit_equal: bool = False    # no product of the expression feeds a sum: contraction cannot change a bit
    opts: tuple = ()           # (("method", "central"), ...) entry-specific
    env: tuple = ()            # environment the device test sets by monkeypatch

    @property
    def id(self):
        per = "".join("P" if p else "L" for p in self.periodic)
        opts = ",".join(f"{k}={v}" for k, v in self.opts if k not in ("golden", "bc_json"))
        return "-".join(str(s) for s in (self.family[7:], self.entry, "x".join(map(str, self.shape)), self.dtype[-2:], per, "/".join(map(str, self.bc)),
                                         self.kind[:2], self.steps, opts) if s != "")

    def opt(self, key, default=None):
        return dict(self.opts).get(key, default)

    @property
    def cells(self):
        return int(np.prod(self.shape))


def bounds_of(shape, f):
    return tuple((0.0, n * f(i)) for i, n in enumerate(shape))


def _bc_sets():
    from test_hip_steppers import BC_SETS, _bc_for

    return BC_SETS, _bc_for


def _faces_of(case: Case, grid):
    """(bc of c, bc of mu) in the notation of `grid.get_boundary_conditions`, as the exact-build test the case was drawn from builds them"""
    tag = case.bc[0]
    if tag == "set":                       # test_hip_steppers.py: BC_SETS
        if case.bc[1] == "periodic":
            return "periodic", "periodic"
        bc = _bc_sets()[1](case.bc[1], grid)
        return bc, bc
    if tag == "local":                     # test_hip_euler2.py: _setup / LOCAL_MU
        from test_hip_euler2 import LOCAL, LOCAL_MU

        bc_c, bc_mu = {}, {}
        for i, a in enumerate(grid.axes):
            if case.periodic[i]:
                bc_c[a] = bc_mu[a] = "periodic"
            else:
                bc_c[a + "-"], bc_c[a + "+"] = LOCAL[i]
                bc_mu[a + "-"], bc_mu[a + "+"] = LOCAL_MU[i]
        return bc_c, bc_mu
    if tag == "faces2d":                   # test_hip_tile2d.py: FACES
        from test_hip_tile2d import FACES

        return FACES[case.bc[1]][1], FACES[case.bc[1]][1]
    if tag == "apn":
        return "auto_periodic_neumann", "auto_periodic_neumann"
    if tag == "value":
        return {"value": case.bc[1]}, {"value": case.bc[1]}
    if tag == "curvature":
        return {"curvature": case.bc[1]}, {"curvature": case.bc[1]}
    if tag == "golden":                    # tests/golden/ops.npz: the case's own conditions (scalar) resp. auto_periodic_neumann (vector)
        return (json.loads(case.opt("bc_json")) if case.opt("bc_json") else None), None
    msg = f"unknown face tag {tag}"
    raise ValueError(msg)


class Built:
    """grid, data, face tables (host pointers) and the running-error description of one case"""

    def __init__(self, case: Case):
        self.case = case
        self.dtype = np.dtype(case.dtype)
        self.grid = pde_hip.CartesianGrid([list(b) for b in case.bounds], list(case.shape), periodic=list(case.periodic))
        self.dx = tuple(float(d) for d in self.grid.discretization)
        self.g = oracle_grid(self.grid, self.dtype)
        nd = len(case.shape)
        rng = np.random.default_rng(case.seed)
        self.rank = int(case.opt("rank", 0))
        lead = (nd,) * self.rank
        golden = case.opt("golden")
        if golden:
            npz = np.load(GOLDEN / "ops.npz", allow_pickle=False)
            self.data = np.ascontiguousarray(npz[golden]).astype(self.dtype)
        else:
            self.data = rng.uniform(-0.5, 0.5, lead + tuple(case.shape)).astype(self.dtype)
        self.ydata = rng.uniform(-0.5, 0.5, case.shape).astype(self.dtype)       # second operand of laplace_euler
        self.bc_c, self.bc_mu = _faces_of(case, self.grid)
        if self.bc_c is None:
            self.bc_c = "auto_periodic_neumann"
        self.bcs_c = self.grid.get_boundary_conditions(self.bc_c, rank=self.rank)
        self.hf_c = host_faces(self.bcs_c, lead)
        self.faces_c = read_faces(self.hf_c.c, case.shape, lead)
        if self.bc_mu is not None:
            self.bcs_mu = self.grid.get_boundary_conditions(self.bc_mu)
            self.hf_mu = host_faces(self.bcs_mu)
            self.faces_mu = read_faces(self.hf_mu.c, case.shape)
        else:
            self.bcs_mu = self.hf_mu = self.faces_mu = None

    # -- the oracle ----------------------------------------------------------------------------------------------------------
    def full(self, data=None):
        return to_full(self.grid, self.data if data is None else data)

    def oracle_rhs(self):
        c = self.case
        self._scratch = np.zeros(self.grid._shape_full, self.dtype)
        code = _abi.RHS_DIFFUSION if c.kind == "diffusion" else _abi.RHS_CAHN_HILLIARD
        return O.make_rhs(code, c.param, self.hf_c.c, self.hf_mu.c, self._scratch)

    def oracle(self):
        """the oracle's results of the case: a list of arrays (valid cells; full arrays for the ghost cells; the error estimate last)"""
        c, g, grid = self.case, self.g, self.grid
        e = c.entry
        if e == "set_ghost_cells":
            full = self.full()
            O.set_ghost_cells(g, max(1, len(c.shape) ** self.rank), self.hf_c.c, full)
            return [full]
        if e in OPERATORS:
            full = self.full()
            O.set_ghost_cells(g, max(1, len(c.shape) ** self.rank), self.hf_c.c, full)
            if e == "laplace":
                return [O.laplace(g, full)]
            if e == "laplace_scaled":
                return [interior(grid, O.laplace_scaled(g, full, c.opt("s1"), c.opt("s2")))]
            if e == "laplace_euler":
                return [interior(grid, O.laplace_euler(g, full, self.full(self.ydata), c.opt("s1"), c.opt("s2")))]
            if e == "cahn_hilliard_mu":
                return [interior(grid, O.cahn_hilliard_mu(g, full, c.param))]
            if e == "gradient":
                return [O.gradient(g, full, c.opt("method"))]
            if e == "gradient_squared":
                return [O.gradient_squared(g, full, bool(c.opt("central")))]
            if e == "divergence":
                return [O.divergence(g, full, c.opt("method"))]
            return [O.axis_derivative(g, full, c.opt("axis"), c.opt("order"), c.opt("method"))]
        rhs = self.oracle_rhs()
        if e in ("rhs_scaled", "ch_fused_rhs"):
            return [interior(grid, O.rhs_scaled(g, rhs, self.full(), c.dt))]
        if e in EULER_ENTRIES:
            return [interior(grid, O.euler_run(g, rhs, self.full(), c.dt, c.steps))]
        if e == "rk4_step":
            y = self.full()
            for _ in range(c.steps):
                O.rk4_step(g, rhs, y, c.dt)
            return [interior(grid, y)]
        assert e == "rkf45_attempt", e
        new, err = O.rkf45_attempt(g, rhs, self.full(), c.dt)
        return [interior(grid, new), np.array(err)]

    # -- the reference -------------------------------------------------------------------------------------------------------
    def reference(self):
        """[(reference, bound), ...] matching `oracle()` entry by entry, as longdouble arrays"""
        c, nd, dt = self.case, len(self.case.shape), self.dtype
        e = c.entry
        x = RE(self.full())
        inner = _sl(nd, 0, MID)

        def done(*items):
            return [(r.v, r.e) for r in items]

        if e == "set_ghost_cells":
            return done(ref_ghosts(x, self.faces_c, nd, dt))
        if e in OPERATORS:
            ref_ghosts(x, self.faces_c, nd, dt)
            if e == "laplace":
                r = ref_lap_mode(x, self.dx, "plain")
            elif e == "laplace_scaled":
                r = ref_lap_mode(x, self.dx, "scaled", c.opt("s1"), c.opt("s2"))
            elif e == "laplace_euler":
                r = ref_lap_mode(x, self.dx, "euler", c.opt("s1"), c.opt("s2"), y=RE(self.full(self.ydata)))
            elif e == "cahn_hilliard_mu":
                r = ref_lap_mode(x, self.dx, "ch_mu", gamma=c.param)
            elif e == "gradient":
                r = ref_gradient(x, self.dx, c.opt("method"))
            elif e == "gradient_squared":
                r = ref_gradient_squared(x, self.dx, bool(c.opt("central")))
            elif e == "divergence":
                r = ref_divergence(x, self.dx, c.opt("method"))
            else:
                r = ref_axis_derivative(x, self.dx, c.opt("axis"), c.opt("order"), c.opt("method"))
            return done(r.store(dt))
        rhs = Rhs(c.kind, c.param, self.faces_c, self.faces_mu, self.dx, dt)
        if e in ("rhs_scaled", "ch_fused_rhs"):
            return done(ref_rhs_scaled(rhs, x, c.dt)[inner])
        if e in EULER_ENTRIES:
            return done(ref_euler_run(rhs, x, c.dt, c.steps)[inner])
        if e == "rk4_step":
            for _ in range(c.steps):
                x = ref_rk4_step(rhs, x, c.dt)
            return done(x[inner])
        new, err = ref_rkf45_attempt(rhs, x, c.dt)
        return done(new[inner], err)

    def mask(self):
        """the cells that are compared: everything, but for ghost cells the cells the reference defines (no edges / corners; a `normal`
        condition leaves the other components' ghost cells alone)"""
        if self.case.entry != "set_ghost_cells":
            return None
        lead = (len(self.case.shape),) * self.rank
        mask = face_mask(self.grid, lead).copy()
        for a in range(len(self.case.shape)):
            for side in range(2):
                f = self.faces_c[2 * a + side]
                if f["normal"] or f["kind"] == _abi.BC_SKIP:
                    for comp in range(lead[0] if lead else 1):
                        if f["kind"] == _abi.BC_SKIP or comp != a:
                            idx = [slice(None)] * len(self.case.shape)
                            idx[a] = -1 if side else 0
                            mask[((comp,) if lead else ()) + tuple(idx)] = False
        return mask


OPERATORS = ("laplace", "laplace_scaled", "laplace_euler", "cahn_hilliard_mu", "gradient", "gradient_squared", "divergence", "axis_derivative")
EULER_ENTRIES = ("euler_run", "diffusion_euler2", "ch_fused_euler", "euler_multi_2d", "diffusion_euler2_slab")


def excess(got, ref, bound, mask=None):
    """max of (|got - ref| - bound) / scale-free: > 0 where the result leaves the bound; and max |got - ref| / bound over the cells with a bound"""
    diff = np.abs(np.asarray(got).astype(LD) - ref)
    if mask is not None:
        diff, bound = diff[mask], bound[mask]
    over = diff > bound
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / np.where(bound > 0, bound, 1), np.where(diff > 0, np.inf, 0))
    return int(over.sum()), float(ratio.max()) if ratio.size else 0.0


def within(results, reference, mask=None):
    """every result of a case inside its bound"""
    return all(excess(got, ref, bound, mask)[0] == 0 for got, (ref, bound) in zip(results, reference))


def worst_ratio(results, reference, mask=None):
    return max(excess(got, ref, bound, mask)[1] for got, (ref, bound) in zip(results, reference))


# -- the table -----------------------------------------------------------------------------------------------------------------
F64, F32 = "float64", "float32"
PATTERNS3 = list(itertools.product([True, False], repeat=3))
PATTERNS2 = list(itertools.product([True, False], repeat=2))


def _cases():
    from test_hip_tile2d import FACES

    out: list[Case] = []
    bc_sets = list(_bc_sets()[0])

    # ---- launch_laplace: the four entry points on fields whose ghost cells are set (test_hip_operators.py: test_laplace_family_vs_oracle_seeded),
    # and pdehip_rhs_scaled with on-the-fly faces (test_hip_steppers.py: test_on_the_fly_bcs_vs_oracle / the RK stage table for (33,), (7,5,3))
    lap_shapes = [(6, 10, 128), (5, 7, 200), (3, 3, 1032), (9, 256), (5, 600), (2, 2, 4), (1, 1, 8), (33,), (7, 5, 3)]
    for si, shape in enumerate(lap_shapes):
        for dtype in (F64, F32):       # (fp32 rows of 3, 33 cells: one cell per thread, as in test_runge_kutta_stage_sweeps_vs_oracle)
            per = (si + (dtype == F32)) % 2 == 0
            base = dict(family="launch_laplace", shape=shape, dtype=dtype, bounds=bounds_of(shape, lambda a: 0.5 + 0.25 * a),
                        periodic=(per,) * len(shape), bc=("apn",) if per else ("value", 0.3), seed=100 + si)
            out.append(Case(entry="laplace", **base))
            out.append(Case(entry="laplace_scaled", opts=(("s1", 0.7), ("s2", 0.01)), **base))
            out.append(Case(entry="laplace_euler", opts=(("s1", 0.7), ("s2", 0.02)), **base))
            out.append(Case(entry="cahn_hilliard_mu", kind="cahn_hilliard", param=0.9, **base))
    for shape in lap_shapes:
        for name in bc_sets + ["periodic"]:
            if name == "second_order" and min(shape) < 2:
                continue       # a curvature condition needs two support points
            for dtype in (F64, F32):
                for kind in ("diffusion", "cahn_hilliard"):
                    out.append(Case(family="launch_laplace", entry="rhs_scaled", shape=shape, dtype=dtype, bounds=bounds_of(shape, lambda a: 0.8),
                                    periodic=(name in ("antiperiodic", "periodic"),) * len(shape), bc=("set", name), kind=kind,
                                    param=0.6 if kind == "diffusion" else 0.9, dt=0.01, seed=11))

    # ---- rows of two 64-lane chunks (CZ=2): 129 to 256 fp64 cells per row and 512 wave tiles or more - (32,32,192) row ends at the tile,
    # (32,32,130) two cells into the second chunk, (32,32,131) inside a lane's vector too (on-the-fly faces and the derivative epilogues: the
    # plain epilogues split such rows), (1024,130) the 2-D instance.  fp32 rows of two chunks (257 cells and more) need 2.6e5 cells in 2-D and 5.3e5
    # in 3-D: beyond this table's size.
    for shape in CZ2_SHAPES:
        base = dict(shape=shape, dtype=F64, bounds=bounds_of(shape, lambda a: 0.6 + 0.15 * a), seed=23, opts=(("instance", "CZ=2"),))
        if shape not in ((32, 32, 130), (32, 32, 131)):      # (those rows: 128 columns to the CZ=1 instance, the rest to the strip)
            lp = dict(family="launch_laplace", periodic=(False,) * len(shape), bc=("value", 0.3), **base)
            out.append(Case(entry="laplace", **lp))
            out.append(Case(entry="laplace_scaled", **{**lp, "opts": (("s1", 0.7), ("s2", 0.01)) + base["opts"]}))
            out.append(Case(entry="laplace_euler", **{**lp, "opts": (("s1", 0.7), ("s2", 0.02)) + base["opts"]}))
            out.append(Case(entry="cahn_hilliard_mu", kind="cahn_hilliard", param=0.9, **lp))
        for name in ("mixed_faces", "periodic"):
            out.append(Case(family="launch_laplace", entry="rhs_scaled", periodic=(name == "periodic",) * len(shape), bc=("set", name), param=0.6, dt=0.01, **base))
        dv = dict(periodic=tuple(a % 2 == 0 for a in range(len(shape))), bc=("apn",), **base)
        for m in ("central", "forward", "backward"):
            out.append(Case(family="launch_deriv_march", entry="gradient", bit_equal=True, **{**dv, "opts": (("method", m), ("layout", "full")) + base["opts"]}))
            if shape[-1] % 2:
                continue       # (the vectorised divergence takes whole vectors only)
            out.append(Case(family="launch_div_march", entry="divergence", **{**dv, "opts": (("method", m), ("layout", "full"), ("rank", 1)) + base["opts"]}))
        for central in (1, 0):
            out.append(Case(family="launch_deriv_march", entry="gradient_squared", **{**dv, "opts": (("central", central), ("layout", "full")) + base["opts"]}))
    out.append(Case(family="launch_laplace", entry="rk4_step", shape=(32, 32, 192), dtype=F64, bounds=bounds_of((32, 32, 192), lambda a: 0.8), periodic=(True,) * 3,
                    bc=("set", "periodic"), param=0.6, dt=2e-3, seed=13, opts=(("instance", "CZ=2"),)))       # the stage epilogue

    # ---- launch_deriv_march / launch_div_march (test_hip_derivatives.py) ----
    d_shapes = [(6, 10, 128), (5, 7, 200), (33, 130), (2, 2, 4), (40,)]
    for si, shape in enumerate(d_shapes):
        nd = len(shape)
        base = dict(shape=shape, bounds=bounds_of(shape, lambda a: 0.7 + 0.2 * a), periodic=tuple(a % 2 == 0 for a in range(nd)), bc=("apn",), seed=17)
        for dtype in (F64, F32):
            for layout in ("full", "valid"):
                for m in ("central", "forward", "backward"):
                    # r = d * sc (d / dx in 1-D): the product feeds no sum - nothing to contract
                    out.append(Case(family="launch_deriv_march", entry="gradient", dtype=dtype, bit_equal=True, opts=(("method", m), ("layout", layout)), **base))
                for central in (1, 0):
                    # 1-D central: d * d * c, one term, no sum; otherwise the squares feed sums
                    out.append(Case(family="launch_deriv_march", entry="gradient_squared", dtype=dtype, bit_equal=(nd == 1 and central == 1),
                                    opts=(("central", central), ("layout", layout)), **base))
            for mi, m in enumerate(("central", "forward", "backward")):
                # acc + d * sc: contractable from the second axis on; in 1-D a single quotient
                out.append(Case(family="launch_div_march", entry="divergence", dtype=dtype, bit_equal=nd == 1,
                                opts=(("method", m), ("layout", "full" if (si + mi) % 2 == 0 else "valid"), ("rank", 1)), **base))
    for shape, axis in [((5, 7, 200), 1), ((33, 130), 1), ((40,), 0)]:
        base = dict(family=SINGLE_BUILD, entry="axis_derivative", shape=shape, bounds=bounds_of(shape, lambda a: 0.6), periodic=(False,) * len(shape),
                    bc=("value", 0.2), seed=4)
        for m in ("central", "forward", "backward"):
            # (r - l) / (2 dx), (r - c) / dx, (c - l) / dx: a difference and a quotient, no product at all
            out.append(Case(dtype=F64, bit_equal=True, opts=(("axis", axis), ("order", 1), ("method", m), ("layout", "valid")), **base))
        out.append(Case(dtype=F64, opts=(("axis", axis), ("order", 2), ("method", "central"), ("layout", "valid")), **base))
    out.append(Case(family=SINGLE_BUILD, entry="axis_derivative", shape=(33, 130), dtype=F32, bounds=bounds_of((33, 130), lambda a: 0.6), periodic=(False, False),
                    bc=("value", 0.2), seed=4, opts=(("axis", 0), ("order", 2), ("method", "central"), ("layout", "valid"))))

    # ---- launch_ghosts: every case of tests/golden/ops.npz (inputs and face definitions only), scalar and vector field ----
    npz = np.load(GOLDEN / "ops.npz", allow_pickle=False)
    for gc in load_cases(npz):
        grid = make_grid(gc)
        shape, dtype = tuple(gc["shape"]), gc.get("dtype", F64)
        base = dict(family="launch_ghosts", entry="set_ghost_cells", shape=shape, dtype=dtype, bounds=tuple(tuple(float(v) for v in b) for b in gc["bounds"]),
                    periodic=tuple(bool(p) for p in gc["periodic"]))
        hf = host_faces(grid.get_boundary_conditions(gc["bc"]))
        # const + factor * v with const == 0 and |factor| == 1 on every face (periodic, anti-periodic, zero-flux): the ghost cell is a copy
        copies = all((not f["arrays"]) and f["const"] == 0 and abs(f["f1"]) == 1 and f["kind"] != _abi.BC_ORDER2 for f in read_faces(hf.c, shape))
        out.append(Case(bc=("golden", gc["id"]), bit_equal=copies, opts=(("golden", f"{gc['id']}/input"), ("bc_json", json.dumps(gc["bc"]))), **base))
        # the vector field takes auto_periodic_neumann: factor 1, constant 0 everywhere - copies
        out.append(Case(bc=("golden", gc["id"], "vector"), bit_equal=True, opts=(("golden", f"{gc['id']}/vector_input"), ("rank", 1)), **base))
    out.append(Case(family="launch_ghosts", entry="set_ghost_cells", shape=(4, 5), dtype=F64, bounds=((0.0, 4.0), (0.0, 5.0)), periodic=(False, True),
                    bc=("golden", "normal_bc"), opts=(("golden", "normal_bc/input"), ("bc_json", str(npz["normal_bc/bc"])), ("rank", 1))))
    out.append(Case(family="launch_ghosts", entry="set_ghost_cells", shape=(5, 7, 12), dtype=F64, bounds=bounds_of((5, 7, 12), lambda a: 0.8),
                    periodic=(False,) * 3, bc=("set", "inhomogeneous"), seed=11))                           # PDEHIP_BCF_ARRAYS
    for dtype in (F64, F32):
        out.append(Case(family="launch_ghosts", entry="set_ghost_cells", shape=(5, 7, 12), dtype=dtype, bounds=bounds_of((5, 7, 12), lambda a: 0.8),
                        periodic=(False,) * 3, bc=("curvature", 0.3), seed=11))                              # order 2

    # ---- launch_euler2 (test_hip_euler2.py) ----
    e2b = dict(family="launch_euler2", bc=("local",))

    def b2(shape):
        return bounds_of(shape, lambda i: 0.7 + 0.1 * i)

    for per in PATTERNS3:
        for dtype, shape in [(F64, (8, 8, 128)), (F64, (5, 6, 128)), (F64, (9, 7, 129)), (F64, (6, 8, 131)), (F64, (12, 20, 257)),
                             (F32, (9, 8, 256)), (F32, (6, 5, 259)), (F32, (9, 16, 513))]:
            out.append(Case(entry="diffusion_euler2", shape=shape, dtype=dtype, bounds=b2(shape), periodic=per, param=0.6, dt=2e-3, steps=2, seed=3, **e2b))
        for dtype, shape in [(F64, (8, 8, 128)), (F64, (7, 9, 131)), (F32, (5, 4, 264))]:
            out.append(Case(entry="ch_fused_euler", shape=shape, dtype=dtype, bounds=b2(shape), periodic=per, kind="cahn_hilliard", param=0.8, dt=1e-3,
                            steps=1, seed=9, **e2b))
    for dtype, shape in [(F64, (8, 8, 128)), (F64, (7, 9, 131)), (F32, (5, 4, 264))]:      # the same sweep without the Euler update (dt * rhs)
        out.append(Case(entry="ch_fused_rhs", shape=shape, dtype=dtype, bounds=b2(shape), periodic=(True, False, False), kind="cahn_hilliard", param=0.8,
                        dt=0.02, seed=9, **e2b))
    for dtype, shape in [(F64, (9, 200)), (F32, (12, 256)), (F64, (11, 129))]:             # test_two_dimensional_grids
        for per in PATTERNS2:
            out.append(Case(entry="diffusion_euler2", shape=shape, dtype=dtype, bounds=b2(shape), periodic=per, param=0.6, dt=2e-3, steps=2, seed=21, **e2b))
        out.append(Case(entry="ch_fused_euler", shape=shape, dtype=dtype, bounds=b2(shape), periodic=(False, True), kind="cahn_hilliard", param=0.8, dt=1e-3,
                        steps=1, seed=21, **e2b))
    for dtype, shape, split in [(F64, (12, 8, 128), 5), (F32, (10, 6, 256), 6)]:           # test_sub_slabs_with_one_physical_face
        out.append(Case(entry="diffusion_euler2_slab", shape=shape, dtype=dtype, bounds=b2(shape), periodic=(False, False, True), param=0.6, dt=2e-3, steps=2,
                        seed=41, opts=(("split", split),), **e2b))
    for shape in [(6, 10, 128), (5, 7, 200), (9, 256)]:                                    # test_runge_kutta_stage_sweeps_vs_oracle
        for kind in ("diffusion", "cahn_hilliard"):
            for name in ("periodic", "mixed_faces"):
                for entry, dtype in itertools.product(("rk4_step", "rkf45_attempt"), (F64, F32)):
                    out.append(Case(family="launch_euler2" if kind == "cahn_hilliard" else "launch_laplace", entry=entry, shape=shape,
                                    dtype=dtype, bounds=bounds_of(shape, lambda a: 0.8), periodic=(name == "periodic",) * len(shape),
                                    bc=("set", name), kind=kind, param=0.6 if kind == "diffusion" else 0.9, dt=2e-3, seed=13))

    # ---- launch_euler4 (test_hip_euler4.py; PDEHIP_EULER4=1) ----
    cart = lambda shape: tuple((0.0, n * s) for n, s in zip(shape, (0.8, 1.25, 1.1)))       # noqa: E731
    unit = lambda shape: tuple((0.0, float(n)) for n in shape)                              # noqa: E731
    e4 = dict(family="launch_euler4", entry="euler_run", dtype=F64, periodic=(True,) * 3, bc=("set", "periodic"), dt=0.05, seed=7, env=(("PDEHIP_EULER4", "1"),))
    out.append(Case(shape=(17, 32, 64), bounds=cart((17, 32, 64)), param=0.7, steps=8, **e4))
    out.append(Case(shape=(19, 64, 128), bounds=unit((19, 64, 128)), param=1.0, steps=4, **e4))      # test_tile_seams
    out.append(Case(shape=(33, 64, 128), bounds=unit((33, 64, 128)), param=1.0, steps=8, **e4))      # unit spacing: the E2_DIFFUSION_UNIT instance

    # ---- launch_tile2d (test_hip_tile2d.py) ----
    for shape in [(64, 64), (33, 70), (5, 7), (1, 9), (31, 129)]:
        for faces in ("pp", "pl", "lp", "ll", "nn"):
            for kind in ("diffusion", "cahn_hilliard"):
                for dtype in (F64, F32):
                    for steps in (1, TILE2D_MAX_STEPS[kind]):
                        out.append(Case(family="launch_tile2d", entry="euler_multi_2d", shape=shape, dtype=dtype, bounds=((0.0, 1.0 * shape[0]), (0.0, 0.9 * shape[1])),
                                        periodic=tuple(FACES[faces][0]), bc=("faces2d", faces), kind=kind,
                                        param=0.7 if kind == "diffusion" else 0.9, dt=0.05 if kind == "diffusion" else 1e-3, steps=steps, seed=3))
    # the 64-column tile (tests/tile2d_cases.py: 2 x 128 tiles is the smallest grid that gets it): second row tile of one row, last tile column of two cells
    for kind in ("diffusion", "cahn_hilliard"):
        for dtype in (F64, F32):
            out.append(Case(family="launch_tile2d", entry="euler_multi_2d", shape=(33, 8130), dtype=dtype, bounds=((0.0, 33.0), (0.0, 0.9 * 8130)),
                            periodic=tuple(FACES["pl"][0]), bc=("faces2d", "pl"), kind=kind, param=0.7 if kind == "diffusion" else 0.9,
                            dt=0.05 if kind == "diffusion" else 1e-3, steps=TILE2D_MAX_STEPS[kind], seed=3, opts=(("instance", "32x64 tile"),)))
    return out


CASES = _cases()
IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS), "case ids must be unique"


@functools.lru_cache(maxsize=8)
def build_case(index: int) -> Built:
    return Built(CASES[index])
