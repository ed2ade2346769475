"""A numpy restatement of the multigrid preconditioner of the Poisson solver (tests only): the hierarchy rule as a pure function, the
exact diagonal of -A, damped Jacobi, mean / copy transfers and the V-cycle, built around the CPU oracle's Laplacian and ghost-cell
setter like tests/poisson_cases.py; and preconditioned conjugate gradients around it."""

from __future__ import annotations

import ctypes as C

import numpy as np

from helpers import host_faces
from oracle import pde_oracle as O
from pde_hip import _abi
from poisson_cases import CONVERGED, MAXITER, STATUS_NAMES, cg_loop, laplace_with_bcs


def hierarchy(shape, max_levels=None, stop_cells: int = 512) -> list[tuple[int, ...]]:
    """Level l+1 halves every axis of level l whose extent is even and >= 4; the end: no such axis, <= 512 cells, or `max_levels`.
    (`stop_cells`: the restatement may go on below 512 cells, so that grids a dense matrix can hold have several levels.)"""
    shapes = [tuple(int(n) for n in shape)]
    while True:
        cur = shapes[-1]
        if int(np.prod(cur)) <= stop_cells or (max_levels and len(shapes) >= max_levels):
            break
        halve = [n >= 4 and n % 2 == 0 for n in cur]
        if not any(halve):
            break
        shapes.append(tuple(n // 2 if h else n for n, h in zip(cur, halve)))
    return shapes


def default_omega(ndim: int) -> float:
    return 2.0 * ndim / (2.0 * ndim + 1.0)


class _Level:
    def __init__(self, shape, dx, faces, keep):
        self.shape, self.dx, self.faces, self.keep = tuple(shape), np.asarray(dx, dtype=float), faces, keep
        self.g = _abi.make_grid(self.shape, self.dx, np.float64)
        self.full_shape = tuple(n + 2 for n in self.shape)

    def factor(self, q: int):
        """factor1 of face q: a scalar, or the coefficient array in the shape of the face."""
        face = self.faces[q]
        if face.flags & _abi.BCF_ARRAYS:
            other = tuple(n for a, n in enumerate(self.shape) if a != q // 2)
            size = int(np.prod(other))
            return np.ctypeslib.as_array(C.cast(face.factor1_arr, C.POINTER(C.c_double)), shape=(size,)).reshape(other).copy()
        return float(face.factor1)

    def periodic(self, axis: int) -> bool:
        n = self.shape[axis]
        return n > 1 and self.faces[2 * axis].index1 == n - 1

    def minus_a(self, z: np.ndarray) -> np.ndarray:
        full = np.zeros(self.full_shape)
        full[(slice(1, -1),) * len(self.shape)] = z
        O.set_ghost_cells(self.g, 1, self.faces, full)
        return -O.laplace(self.g, full)

    def diagonal(self) -> np.ndarray:
        """d = sum_a s_a (2 - [lower face] f_lo - [upper face] f_hi); 2 s_a on periodic axes."""
        d = np.zeros(self.shape)
        for axis, n in enumerate(self.shape):
            s = self.dx[axis] ** -2.0
            term = np.full(self.shape, 2.0)
            if not self.periodic(axis):
                for upper in (0, 1):
                    f = self.factor(2 * axis + upper)
                    index = [slice(None)] * len(self.shape)
                    index[axis] = n - 1 if upper else 0
                    term[tuple(index)] -= f
            d += s * term
        return d


class Cycle:
    """z = M r: `smooth` Jacobi sweeps, residual, mean of the children, the coarser levels, copy to the children, `smooth` sweeps;
    `coarse` sweeps from zero on the last level."""

    def __init__(self, grid, bc, smooth: int = 2, coarse: int = 32, max_levels=None, omega=None, stop_cells: int = 512):
        table = host_faces(grid.get_boundary_conditions(bc))
        self.table = table
        self.shapes = hierarchy(grid.shape, max_levels, stop_cells)
        self.smooth, self.coarse = smooth, coarse
        self.omega = default_omega(len(grid.shape)) if omega is None else omega
        self.levels: list[_Level] = []
        shape, dx = tuple(grid.shape), np.asarray(grid.discretization, dtype=float)
        faces, keep = _abi.FaceArray(), []
        for q in range(2 * len(shape)):
            src = table.c[q]
            faces[q].kind, faces[q].flags, faces[q].index1, faces[q].index2 = src.kind, src.flags, src.index1, src.index2
            faces[q].const_v, faces[q].factor1, faces[q].factor2 = 0.0, src.factor1, src.factor2
            if src.flags & _abi.BCF_ARRAYS:
                size = int(np.prod([n for a, n in enumerate(shape) if a != q // 2]))
                zero = np.zeros(size)
                keep.append(zero)
                faces[q].const_arr, faces[q].factor1_arr = zero.ctypes.data, src.factor1_arr
        self.levels.append(_Level(shape, dx, faces, keep))
        for nxt in self.shapes[1:]:
            cur = self.levels[-1]
            halved = [n != m for n, m in zip(cur.shape, nxt)]
            faces, keep = _abi.FaceArray(), []
            for q in range(2 * len(shape)):
                axis, upper = divmod(q, 2)
                src = cur.faces[q]
                faces[q].kind, faces[q].flags, faces[q].index2 = src.kind, src.flags, src.index2
                faces[q].const_v, faces[q].factor1, faces[q].factor2 = 0.0, src.factor1, src.factor2
                local = src.index1 == (cur.shape[axis] - 1 if upper else 0)
                faces[q].index1 = ((nxt[axis] - 1 if upper else 0) if local else (0 if upper else nxt[axis] - 1))
                if src.flags & _abi.BCF_ARRAYS:
                    fine = cur.factor(q)
                    other = [a for a in range(len(shape)) if a != axis]
                    for pos, a in enumerate(other):
                        if halved[a]:
                            fine = 0.5 * (np.take(fine, range(0, fine.shape[pos], 2), axis=pos) + np.take(fine, range(1, fine.shape[pos], 2), axis=pos))
                    coarse_arr, zero = np.ascontiguousarray(fine), np.zeros(fine.size)
                    keep += [coarse_arr, zero]
                    faces[q].const_arr, faces[q].factor1_arr = zero.ctypes.data, coarse_arr.ctypes.data
            self.levels.append(_Level(nxt, cur.dx * np.where(halved, 2.0, 1.0), faces, keep))
        self.wd = []
        for lv in self.levels:
            d = lv.diagonal()
            self.wd.append(np.where(d > 0, self.omega / np.where(d > 0, d, 1.0), 0.0))

    def sweeps(self, l: int, z, r: np.ndarray, count: int) -> np.ndarray:
        lv = self.levels[l]
        for _ in range(count):
            z = self.wd[l] * r if z is None else z + self.wd[l] * (r - lv.minus_a(z))
        return z

    @staticmethod
    def restrict(fine: np.ndarray, coarse_shape) -> np.ndarray:
        out = fine
        for axis, (n, m) in enumerate(zip(fine.shape, coarse_shape)):
            if n != m:
                lo = np.take(out, range(0, n, 2), axis=axis)
                hi = np.take(out, range(1, n, 2), axis=axis)
                out = lo + hi
        return out * (out.size / fine.size)

    @staticmethod
    def prolong(coarse: np.ndarray, fine_shape) -> np.ndarray:
        out = coarse
        for axis, (m, n) in enumerate(zip(coarse.shape, fine_shape)):
            if n != m:
                out = np.repeat(out, 2, axis=axis)
        return out

    def cycle(self, l: int, r: np.ndarray) -> np.ndarray:
        lv = self.levels[l]
        if l + 1 == len(self.levels):
            return self.sweeps(l, None, r, self.coarse)
        z = self.sweeps(l, None, r, self.smooth)
        rc = self.restrict(r - lv.minus_a(z), self.levels[l + 1].shape)
        z = z + self.prolong(self.cycle(l + 1, rc), lv.shape)
        return self.sweeps(l, z, r, self.smooth)

    def __call__(self, r: np.ndarray) -> np.ndarray:
        return self.cycle(0, np.asarray(r, dtype=float))

    def matrix(self) -> np.ndarray:
        size = int(np.prod(self.shapes[0]))
        mat = np.empty((size, size))
        unit = np.zeros(size)
        for j in range(size):
            unit[j] = 1.0
            mat[:, j] = self(unit.reshape(self.shapes[0])).ravel()
            unit[j] = 0.0
        return mat


def mgcg(grid, bc, rhs: np.ndarray, rtol: float = 1e-10, maxiter: int = 200, singular: bool = False, atol: float = 0.0, sums=None,
         keep=None, **cycle_args):
    """(-A) u = v - f by conjugate gradients preconditioned with the cycle: the loop of tests/poisson_cases.py (`cg_loop`) with
    z = M r.  `sums=None`: returns (u, iterations) and raises when `maxiter` is reached (np.sum dot products); `sums="exact"` /
    `"numpy"`: returns the `Trajectory` like `cg`, whatever the status."""
    m = Cycle(grid, bc, **cycle_args)
    v = laplace_with_bcs(grid, bc, np.zeros(grid.shape))
    traj = cg_loop(v, m.levels[0].minus_a, rhs, rtol, atol, maxiter, singular, sums or "numpy", m, keep if sums else ())
    if sums:
        return traj
    if traj.status == MAXITER:
        msg = f"restated mgcg did not converge within {maxiter} iterations"
        raise RuntimeError(msg)
    if traj.status != CONVERGED:
        msg = f"restated mgcg ended with {STATUS_NAMES[traj.status]} after {traj.iterations} iterations"
        raise RuntimeError(msg)
    return traj.x, traj.iterations
