"""Poisson's and Laplace's equation on the device: the operator ``poisson_solver`` and the functions ``solve_poisson_equation`` /
``solve_laplace_equation``.

Reference: ``pde/backends/scipy/operators/cartesian.py:472-489`` (the operator: the Laplacian with its conditions as a sparse matrix
plus a constant vector), ``pde/backends/scipy/operators/common.py:71-146`` (spsolve, else lsmr, and the ``allclose`` test of the
result), ``pde/pdes/laplace.py:28-125`` (the two functions).  Here the same split system is solved by conjugate gradients in
``libpdehip`` (``pdehip_poisson_create`` / ``_solve`` / ``_destroy``, csrc/pdehip_poisson.h); this module decides on the host what
the loop is allowed to see - which conditions keep the matrix symmetric - and turns its status into the reference's exceptions.

``method="mgcg"`` preconditions the same loop with one geometric multigrid V-cycle per iteration (``pdehip_poisson_set_multigrid``,
csrc/pdehip_poisson_mg.h): the iteration count no longer grows with the extent of the grid.  ``"auto"`` and ``"cg"`` are the plain loop.

``method="fft"`` is a direct solve for grids that are periodic on every axis (``pdehip_poisson_fft``, csrc/pdehip_fftsolve.hip): there the
matrix is diagonal in Fourier space, so a forward transform, one division per mode and an inverse transform give the zero-mean solution
to rounding - no iteration, no handle, ``maxiter`` / ``batch`` / ``mg_*`` do not apply.  Extents must be powers of two (up to 1024, 4096
on the last axis).  ``rtol`` / ``atol`` are tested against the TRUE residual ``||A x - (f - mean f)||``, which no fp64 method brings
below about ``2**-53 ||A|| ||x||``: a solve that misses them raises ``ConvergenceError`` instead of hiding it.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .device import DeviceArray

ENTRY_POINTS = ("poisson_create", "poisson_solve", "poisson_destroy")
MG_ENTRY_POINTS = ("poisson_set_multigrid", "poisson_precondition")
METHODS = ("auto", "cg", "mgcg")
DIRECT_METHODS = ("fft",)
FFT_ENTRY_POINTS = ("fft_supported", "poisson_fft")
MG_DEFAULTS = {"mg_smooth": 2, "mg_coarse": 32, "mg_levels": None}
MG_MAXITER = 200
DEFAULT_RTOL = 1e-10
DEFAULT_BATCH = 32


def check_method(method: str) -> None:
    """``method`` of the operator: "auto", "cg", "mgcg" or the direct "fft" (the reference: "auto" or "scipy", same message,
    common.py:95-97)."""
    if method not in METHODS and method not in DIRECT_METHODS:
        msg = f"Method {method} is not available"
        raise ValueError(msg)


def default_maxiter(shape) -> int:
    """50 x the largest extent, at least 1000: conjugate gradients without a preconditioner need on the order of the extent times
    the number of digits."""
    return max(1000, 50 * max(int(n) for n in shape))


def mg_options(method: str, kwargs: dict) -> dict:
    """The arguments of the multigrid cycle taken out of ``kwargs`` (``mg_smooth``, ``mg_coarse``, ``mg_levels``): valid with
    ``method="mgcg"`` only, positive integers (``mg_levels=None``: as many levels as the grid allows).  No device is touched."""
    given = {k: kwargs.pop(k) for k in list(kwargs) if k in MG_DEFAULTS}
    if method != "mgcg":
        if given:
            msg = f"poisson_solver: argument(s) {sorted(given)} need method=\"mgcg\" (method is {method!r})"
            raise TypeError(msg)
        return {}
    opts = dict(MG_DEFAULTS, **given)
    for name, value in opts.items():
        if value is None and name == "mg_levels":
            continue
        if isinstance(value, bool) or int(value) != value or int(value) < 1:
            msg = f"poisson_solver: {name} must be a positive integer (got {value!r})"
            raise ValueError(msg)
        opts[name] = int(value)
    return opts


def _face_name(axis: int, upper: bool) -> str:
    return f"{'upper' if upper else 'lower'} face of axis {axis}"


def check_faces(faces, shape) -> None:
    """Refuse the faces of a C face table (``pdehip_bc_face_t[6]``) that would make the matrix non-symmetric; the rules of
    ``pdehip_poisson_create``, applied before anything touches the device."""
    for axis, n in enumerate(shape):
        for upper in (False, True):
            face = faces[2 * axis + int(upper)]
            where = _face_name(axis, upper)
            if face.kind == _abi.BC_ORDER2:
                msg = (f"poisson_solver: the {where} is a second-order condition (it reads a second cell, `index2`): the matrix is not "
                       "symmetric and conjugate gradients do not apply")
                raise NotImplementedError(msg)
            if face.kind != _abi.BC_ORDER1:
                msg = f"poisson_solver: the {where} carries no condition the solver can put into its matrix"
                raise NotImplementedError(msg)
            if face.flags & _abi.BCF_NORMAL:
                msg = f"poisson_solver: the {where} is a condition on the normal component of a vector field: the solver takes scalar fields"
                raise NotImplementedError(msg)
            adjacent, wrapped = (n - 1, 0) if upper else (0, n - 1)
            if face.index1 not in (adjacent, wrapped):
                msg = f"poisson_solver: the {where} takes its virtual point from a cell that is neither adjacent nor periodic"
                raise NotImplementedError(msg)
            if face.index1 == wrapped and n > 1:
                other = faces[2 * axis + int(not upper)]
                periodic = all(f.kind == _abi.BC_ORDER1 and not f.flags & _abi.BCF_ARRAYS and f.const_v == 0 and f.factor1 == 1 for f in (face, other))
                if not periodic or other.index1 != adjacent:     # (the other end's wrapped cell is this end's adjacent one)
                    msg = f"poisson_solver: the {where} links the two ends of its axis without being periodic: the matrix is not symmetric"
                    raise NotImplementedError(msg)


def is_singular(faces, ndim: int, factor_arrays=None) -> bool:
    """Every face periodic or Neumann - ``factor1 == 1`` everywhere and no second-order face -: the matrix has the constants in its
    null space (the reference's ``MatrixRankWarning`` branch).  ``factor_arrays``: ``face index -> host array`` for faces with
    coefficient arrays (the library reads them from the device itself)."""
    for q in range(2 * ndim):
        face = faces[q]
        if face.kind != _abi.BC_ORDER1:
            return False
        if face.flags & _abi.BCF_ARRAYS:
            arr = None if factor_arrays is None else factor_arrays.get(q)
            if arr is None or not np.all(np.asarray(arr) == 1.0):
                return False
        elif face.factor1 != 1.0:
            return False
    return True


def check_all_periodic(grid, bcs) -> None:
    """Refuse, for the direct solve, everything but plainly periodic conditions on every axis; nothing touches the device."""
    from .bc_expr import expression_faces
    from .faces import convert_bcs

    for axis, periodic in enumerate(grid.periodic):
        if not periodic:
            msg = f"poisson_solver: method=\"fft\" needs periodic conditions on every axis: the {_face_name(axis, False)} is not periodic"
            raise NotImplementedError(msg)
    if expression_faces(bcs):
        msg = "poisson_solver: method=\"fft\" takes plainly periodic conditions, not expressions"
        raise NotImplementedError(msg)
    table = convert_bcs(bcs, part=None)
    if getattr(table, "time_dependent", False) or getattr(table, "reads_value", False):
        msg = "poisson_solver: method=\"fft\" takes plainly periodic conditions, not time-dependent ones"
        raise NotImplementedError(msg)
    for axis, n in enumerate(grid.shape):
        for upper in (False, True):
            face = table.c[2 * axis + int(upper)]
            plain = (face.kind == _abi.BC_ORDER1 and not face.flags and face.const_v == 0 and face.factor1 == 1
                     and face.index1 == (0 if upper else n - 1))
            if not plain:
                msg = f"poisson_solver: method=\"fft\" needs periodic conditions on every axis: the {_face_name(axis, upper)} is not plainly periodic"
                raise NotImplementedError(msg)


def check_conditions(bcs) -> None:
    """Refuse conditions the face table cannot show: complex factors (they couple real and imaginary part) and expressions that are
    not affine in the adjacent value (the reference refuses expression conditions in its matrix too, local.py:1086-1089)."""
    from .faces import has_complex_factors

    if has_complex_factors(bcs):
        msg = "poisson_solver: a condition multiplies the field by a complex factor: real and imaginary part are coupled and the matrix is not symmetric"
        raise NotImplementedError(msg)


class _Solver:
    """One split system (grid, face table): the handle of the library, created at the first solve and kept for later right-hand sides."""

    def __init__(self, backend, grid, table, params: dict, mg: dict | None = None):
        self.backend, self.grid, self.table, self.params = backend, grid, table, params
        self.mg, self.hierarchy = mg, {}      # mg: the options of the multigrid cycle (method "mgcg"), None: the plain loop
        self._handles: dict[str, int] = {}
        if getattr(table, "reads_value", False):
            msg = "poisson_solver: a condition is not affine in the adjacent value: the problem is not linear"
            raise NotImplementedError(msg)
        check_faces(table.c, grid.shape)

    def _handle(self, lib, info) -> int:
        key = info.dtype.str
        if getattr(self.table, "time_dependent", False):
            self.release()     # the coefficient arrays were rewritten: whether the system is singular is decided per solve
        if key not in self._handles:
            handle = C.c_void_p()
            lib.poisson_create(info.ref, self.table.c, C.byref(handle))
            self._handles[key] = handle.value
            if self.mg is not None:
                opts = _abi.PoissonMg()
                opts.smooth, opts.coarse_sweeps, opts.max_levels = self.mg["mg_smooth"], self.mg["mg_coarse"], self.mg["mg_levels"] or 0
                lib.poisson_set_multigrid(handle.value, C.byref(opts))
                ndim = len(self.grid.shape)
                self.hierarchy = {"levels": int(opts.levels), "level_shapes": [tuple(int(opts.shapes[lv][a]) for a in range(ndim)) for lv in range(opts.levels)],
                                  "bytes": int(opts.bytes), "omega": float(opts.omega)}
        return self._handles[key]

    def precondition(self, r: DeviceArray, z: DeviceArray) -> DeviceArray:
        """``z = M r``: one application of the multigrid cycle to an fp64 array of the grid (tests of the cycle on its own)."""
        lib = self.backend._lib
        lib.poisson_precondition(self._handle(lib, r.info), r.ptr, z.ptr, self.backend.stream)
        return z

    def release(self) -> None:
        handles, self._handles = self._handles, {}
        for handle in handles.values():
            try:
                self.backend._lib.poisson_destroy(handle)
            except Exception:      # noqa: BLE001  (interpreter shutdown)
                pass

    def __del__(self):
        self.release()

    def solve(self, rhs: DeviceArray, out: DeviceArray, args=None) -> dict:
        lib = self.backend._lib
        if getattr(self.table, "time_dependent", False):
            self.table.update(args, state=None, stream=self.backend.stream)
        io = _abi.Poisson()
        io.rtol, io.atol = float(self.params["rtol"]), float(self.params["atol"])
        io.maxiter, io.batch = int(self.params["maxiter"]), int(self.params["batch"])
        lib.poisson_solve(self._handle(lib, rhs.info), rhs.ptr, out.ptr, C.byref(io), self.backend.stream)
        return {"iterations": int(io.iterations), "residual": float(io.residual), "rhs_norm": float(io.rhs_norm),
                "converged": io.status in (_abi.POISSON_CONVERGED, _abi.POISSON_INCONSISTENT), "status": int(io.status),
                "singular": bool(io.singular), "check_residual": float(io.check_residual)}


class _FftSolver:
    """The direct solve of an all-periodic grid: no handle, no faces - one call of ``pdehip_poisson_fft`` per right-hand side."""

    hierarchy: dict = {}

    def __init__(self, backend, grid, params: dict):
        self.backend, self.grid, self.params = backend, grid, params

    def release(self) -> None:
        pass

    def solve(self, rhs: DeviceArray, out: DeviceArray, args=None) -> dict:
        io = _abi.Poisson()
        io.rtol, io.atol = float(self.params["rtol"]), float(self.params["atol"])
        self.backend._lib.poisson_fft(rhs.info.ref, rhs.ptr, out.ptr, C.byref(io), self.backend.stream)
        return {"iterations": int(io.iterations), "residual": float(io.residual), "rhs_norm": float(io.rhs_norm),
                "converged": io.status in (_abi.POISSON_CONVERGED, _abi.POISSON_INCONSISTENT), "status": int(io.status),
                "singular": bool(io.singular), "check_residual": float(io.check_residual),
                "asked": max(float(io.rtol) * float(io.rhs_norm), float(io.atol))}


def raise_for_status(info: dict, maxiter: int, method: str = "cg") -> None:
    """The status of a solve as the exception a caller of the reference would see."""
    status = info["status"]
    if status == _abi.POISSON_CONVERGED:
        return
    if status == _abi.POISSON_MAXITER:
        from .solvers import ConvergenceError

        if method in DIRECT_METHODS:
            msg = f"Poisson problem: the direct FFT solve reached residual {info['residual']:g}, asked {info['asked']:g}"
            raise ConvergenceError(msg)
        name = "Multigrid-preconditioned conjugate gradients (mgcg)" if method == "mgcg" else "Conjugate gradients"
        msg = f"{name} did not converge within {maxiter} iterations (residual {info['residual']:g}, right-hand side {info['rhs_norm']:g})"
        raise ConvergenceError(msg)
    if status == _abi.POISSON_INCONSISTENT:
        msg = f"Poisson problem could not be solved (Residual: {info['check_residual']})"       # common.py:135-137
        raise RuntimeError(msg)
    reason = {_abi.POISSON_NONFINITE: "a scalar of the iteration is not finite",
              _abi.POISSON_BREAKDOWN: "breakdown: the matrix of these conditions is not negative definite"}.get(status, f"status {status}")
    msg = f"Poisson problem could not be solved ({reason}; residual {info['residual']:g} after {info['iterations']} iterations)"
    raise RuntimeError(msg)


def make_poisson_operator(backend, grid, bcs, dtype=None, *, method: str = "auto", rtol: float = DEFAULT_RTOL, atol: float = 0.0,
                          maxiter: int | None = None, batch: int | None = None, **kwargs):
    """``op(arr, out=None, args=None) -> out`` solving ``laplace(out) = arr`` with the conditions ``bcs`` (cartesian.py:472-489).

    ``arr``: host valid data (real or complex; host data is returned) or a :class:`DeviceArray` (a :class:`DeviceArray` is returned).
    ``op.info`` holds the method, iterations, residual norm, norm of the right-hand side and the convergence flag of the last call.

    ``method="mgcg"``: conjugate gradients preconditioned by a multigrid V-cycle, with ``mg_smooth`` Jacobi sweeps before and after
    the coarse-grid correction (default 2), ``mg_coarse`` sweeps on the last level (32) and at most ``mg_levels`` levels (None: all);
    ``maxiter`` defaults to 200 and ``op.info`` also holds ``levels`` and ``level_shapes``.  Axes of odd extent stop coarsening.

    ``method="fft"``: the direct solve of grids that are periodic on every axis with power-of-two extents; takes ``rtol`` and ``atol``
    only.  ``op.info["iterations"]`` is 0 and ``op.info["residual"]`` is the true residual norm ``||A x - (f - mean f)||``."""
    from .bc_expr import convert_bcs_with_expressions, expression_faces
    from .faces import convert_bcs, real_dtype_of

    check_method(method)
    direct = method in DIRECT_METHODS
    if direct:
        given = sorted(name for name, value in (("maxiter", maxiter), ("batch", batch)) if value is not None)
        if given:
            msg = f"poisson_solver: argument(s) {given} need an iterative method (method is {method!r})"
            raise TypeError(msg)
    mg = mg_options(method, kwargs) or None      # the options of the cycle, None for the plain loop
    if kwargs:
        msg = f"poisson_solver: unknown argument(s) {sorted(kwargs)}"
        raise TypeError(msg)
    if not (float(rtol) >= 0 and float(atol) >= 0):
        msg = "poisson_solver: rtol and atol must not be negative"
        raise ValueError(msg)
    params = {"rtol": float(rtol), "atol": float(atol), "maxiter": (MG_MAXITER if mg else default_maxiter(grid.shape)) if maxiter is None else int(maxiter),
              "batch": DEFAULT_BATCH if batch is None else int(batch)}
    if params["maxiter"] < 1 or params["batch"] < 1:
        msg = "poisson_solver: maxiter and batch must be positive"
        raise ValueError(msg)
    if direct:
        check_all_periodic(grid, bcs)
    ginfo64 = backend.grid_info(grid, np.float64)       # Cartesian grids only (raises NotImplementedError otherwise)
    lib = backend._lib
    if direct:
        if not lib.has(*FFT_ENTRY_POINTS):
            missing = sorted("pdehip_" + name for name in FFT_ENTRY_POINTS if name in lib.missing)
            msg = f"hip backend: the loaded library does not export {', '.join(missing)}: no `poisson_solver` with method=\"fft\" with it"
            raise NotImplementedError(msg)
        lib.fft_supported(ginfo64.ref)       # the dry run: NotImplementedError with the library's message
    elif not lib.has(*ENTRY_POINTS):
        missing = sorted("pdehip_" + name for name in ENTRY_POINTS if name in lib.missing)
        msg = f"hip backend: the loaded library does not export {', '.join(missing)}: no `poisson_solver` with it"
        raise NotImplementedError(msg)
    if mg and not lib.has(*MG_ENTRY_POINTS):
        missing = sorted("pdehip_" + name for name in MG_ENTRY_POINTS if name in lib.missing)
        msg = f"hip backend: the loaded library does not export {', '.join(missing)}: no `poisson_solver` with method=\"mgcg\" with it"
        raise NotImplementedError(msg)
    check_conditions(bcs)
    has_expr = bool(expression_faces(bcs))

    def table_for(part):
        return convert_bcs_with_expressions(bcs, part=part) if has_expr else convert_bcs(bcs, part=part)

    solvers: dict = {}

    def solver_for(part) -> _Solver:
        if part not in solvers:
            solvers[part] = _FftSolver(backend, grid, params) if direct else _Solver(backend, grid, table_for(part), params, mg)
        return solvers[part]

    if dtype is None or np.dtype(dtype).kind != "c":
        solver_for(None)       # refusals surface when the operator is made, like the reference's matrix assembly
    shape = tuple(grid.shape)

    def fail(info: dict) -> None:
        solve_poisson.info = {"method": method, **{k: info[k] for k in ("iterations", "residual", "rhs_norm", "converged")}}
        if mg:
            hierarchy = next(iter(solvers.values())).hierarchy
            solve_poisson.info.update(levels=hierarchy["levels"], level_shapes=hierarchy["level_shapes"])
        raise_for_status(info, params["maxiter"], method)

    def solve_poisson(arr, out=None, args=None):
        host = not isinstance(arr, DeviceArray)
        if tuple(arr.shape) != shape:
            msg = f"Incompatible shapes {tuple(arr.shape)} != {shape}"
            raise ValueError(msg)
        if out is not None and tuple(out.shape) != shape:
            msg = f"Incompatible shapes {tuple(out.shape)} != {shape}"
            raise ValueError(msg)
        if not host:
            res = out if isinstance(out, DeviceArray) else DeviceArray(arr.info)
            fail(solver_for(None).solve(arr, res, args))
            return res
        arr = np.asarray(arr)
        if arr.dtype.kind == "c" or (dtype is not None and np.dtype(dtype).kind == "c"):
            # real coefficients: real and imaginary part through the real solver, each with its part of the boundary values
            real = real_dtype_of(arr.dtype if arr.dtype.kind == "c" else dtype)
            ginfo = backend.grid_info(grid, real)
            parts, infos = [], []
            for part, take in (("re", np.real), ("im", np.imag)):
                native = DeviceArray(ginfo).set_valid(np.ascontiguousarray(take(arr), dtype=real), backend.stream)
                res = DeviceArray(ginfo)
                infos.append(solver_for(part).solve(native, res, args))
                parts.append(res.get_valid(stream=backend.stream))
            worst = max(infos, key=lambda i: (i["status"] != 0, i["iterations"]))
            merged = dict(worst, iterations=max(i["iterations"] for i in infos), residual=float(np.hypot(infos[0]["residual"], infos[1]["residual"])),
                          rhs_norm=float(np.hypot(infos[0]["rhs_norm"], infos[1]["rhs_norm"])), converged=all(i["converged"] for i in infos))
            fail(merged)
            result = parts[0] + 1j * parts[1]
            if out is not None:
                out[...] = result
                return out
            return result
        real = arr.dtype if arr.dtype in (np.float32, np.float64) else np.dtype(np.float64)
        if dtype is not None and np.dtype(dtype) in (np.float32, np.float64):
            real = np.dtype(dtype)
        ginfo = backend.grid_info(grid, real)
        native = DeviceArray(ginfo).set_valid(np.ascontiguousarray(arr, dtype=real), backend.stream)
        res = out if isinstance(out, DeviceArray) else DeviceArray(ginfo)
        fail(solver_for(None).solve(native, res, args))
        if isinstance(out, DeviceArray):
            return out
        return res.get_valid(out=out, stream=backend.stream)

    solve_poisson.solver_for = solver_for  # type: ignore[attr-defined]
    solve_poisson.grid = grid  # type: ignore[attr-defined]
    solve_poisson.info = {}  # type: ignore[attr-defined]
    solve_poisson._hip_operator = ("poisson_solver", 0, 0)  # type: ignore[attr-defined]
    return solve_poisson


def make_poisson_solver(grid, *, backend, **kwargs):
    """The factory registered for ``poisson_solver``.  Unlike the stencil operators this one is MADE of the conditions (the
    reference's factory takes ``bcs``, cartesian.py:473-475): without them there is nothing to solve."""
    bcs, dtype = kwargs.pop("bcs", None), kwargs.pop("dtype", None)
    if bcs is None:
        msg = ("hip backend: operator `poisson_solver` is built from the boundary conditions: use `make_operator(grid, \"poisson_solver\", bcs=...)` "
               "(there is no version without boundary conditions)")
        raise ValueError(msg)
    return make_poisson_operator(backend, grid, bcs, dtype, **kwargs)


make_poisson_solver._hip_needs_bcs = True  # type: ignore[attr-defined]


# ---------------------------------------------------------------------------------------------
# the functions of pde/pdes/laplace.py on the mirror classes
# ---------------------------------------------------------------------------------------------
def solve_poisson_equation(rhs, bc, *, label: str = "Solution to Poisson's equation", backend="hip", **kwargs):
    """Solve ``laplace(u) = rhs`` with the conditions ``bc`` (pde/pdes/laplace.py:28-97; ``kwargs``: ``method``, ``rtol``, ``atol``,
    ``maxiter``, ``batch`` and, with ``method="mgcg"``, ``mg_smooth``, ``mg_coarse``, ``mg_levels``; ``method="fft"``: the direct solve
    of all-periodic grids, ``rtol`` and ``atol`` only).  With periodic or Neumann conditions only, the right-hand side has to be compatible with them (its
    integral equals the prescribed flux): otherwise a ``RuntimeError`` with the reference's hint is raised."""
    from .backend import get_backend
    from .fields import ScalarField
    from .solvers import ConvergenceError

    impl = get_backend(backend)
    info = impl.get_operator_info(rhs.grid, "poisson_solver")
    bcs = rhs.grid.get_boundary_conditions(bc)
    solver = impl.make_operator(rhs.grid, info, bcs=bcs, dtype=rhs.dtype, **kwargs)
    result = ScalarField(rhs.grid, label=label, dtype=rhs.dtype)
    try:
        solver(rhs.data, out=result.data)
    except ConvergenceError:
        raise
    except RuntimeError as err:
        magnitude = abs(rhs.data.mean())      # `rhs.magnitude` (fields/datafield_base.py:885-893: |integral / volume| of a scalar field)
        if magnitude > 1e-10:
            msg = ("Could not solve the Poisson problem. One possible reason for this is that only periodic or Neumann conditions are "
                   f"applied although the magnitude of the field is {magnitude} and thus non-zero.")
            raise RuntimeError(msg) from err
        raise
    result.info = dict(solver.info)
    return result


def solve_laplace_equation(grid, bc, *, label: str = "Solution to Laplace's equation", backend="hip"):
    """Solve ``laplace(u) = 0`` with the conditions ``bc`` (pde/pdes/laplace.py:100-125)."""
    from .fields import ScalarField

    return solve_poisson_equation(ScalarField(grid, data=0), bc=bc, label=label, backend=backend)
