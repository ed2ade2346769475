"""A dense numpy restatement of the reference's `poisson_solver` (tests only): the Laplacian with its boundary conditions as a matrix
plus a constant vector - `L u = A u + v`, the reference's `_get_laplace_matrix` - built from the CPU oracle's Laplacian and ghost-cell
setter (column j of A = L(e_j) - L(0), v = L(0)), solved like pde/backends/scipy/operators/common.py:99-141 solves it: directly when
the matrix is regular, the minimum-norm least-squares solution plus the `allclose` test when it is singular.  And a restatement of the device's own loop
(`cg`): the conjugate gradients of csrc/pdehip_poisson.hip with every scalar and every iterate of the way, for the device tests that
compare iteration by iteration."""

from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

import pde_hip
from helpers import host_faces, oracle_grid, to_full
from oracle import pde_oracle as O
from pde_hip import _abi


# conditions shared by the Poisson tests (one definition: the CPU and the device tests import them)
MIXED = {"type": "mixed", "value": 0.8, "const": 0.3}
FACES1 = [[{"value": 0.2}, {"derivative": 0.1}]]
FACES2 = [[{"value": 0.5}, MIXED], [{"derivative": -0.2}, {"value": 2.0}]]
FACES3 = [[{"value": 0.5}, MIXED], [{"derivative": -0.2}, {"value": 2.0}], "periodic"]
# an indefinite system: on a unit grid this `mixed` condition has factor1 = 7 > 2, so the first diagonal entry of -A is negative
INDEFINITE = {"shape": [8], "bc": [[{"type": "mixed", "value": -1.5, "const": 0.2}, {"value": 0.0}]], "seed": 4}
STATUS_NAMES = {0: "converged", 1: "maxiter", 2: "a non-finite scalar", 3: "breakdown"}


class NotSolved(RuntimeError):
    pass


def make_grid(case: dict):
    return pde_hip.CartesianGrid(case["bounds"], case["shape"], periodic=case["periodic"])


def laplace_with_bcs(grid, bc, data: np.ndarray) -> np.ndarray:
    """L(data): ghost cells of the conditions `bc`, then the oracle's Laplacian."""
    faces = host_faces(grid.get_boundary_conditions(bc))
    g = oracle_grid(grid)
    full = to_full(grid, np.ascontiguousarray(data, dtype=np.float64))
    O.set_ghost_cells(g, 1, faces.c, full)
    return O.laplace(g, full)


class HomogeneousOperator:
    """w = (-A) z: the oracle's Laplacian with the homogeneous part of every face (`ghost = factor1 * adjacent`, the constants and the
    constant arrays zeroed), the copy of the face table the device keeps as `faces_a`."""

    def __init__(self, grid, bc):
        self.grid, self.g = grid, oracle_grid(grid)
        self.table = host_faces(grid.get_boundary_conditions(bc))        # keeps the factor arrays alive
        self.faces, self.keep = _abi.FaceArray(), []
        for q in range(2 * grid.num_axes):
            src, dst = self.table.c[q], self.faces[q]
            dst.kind, dst.flags, dst.index1, dst.index2 = src.kind, src.flags, src.index1, src.index2
            dst.const_v, dst.factor1, dst.factor2 = 0.0, src.factor1, src.factor2
            if src.flags & _abi.BCF_ARRAYS:
                zero = np.zeros(int(np.prod([n for a, n in enumerate(grid.shape) if a != q // 2])))
                self.keep.append(zero)
                dst.const_arr, dst.factor1_arr = zero.ctypes.data, src.factor1_arr

    def __call__(self, z: np.ndarray) -> np.ndarray:
        full = to_full(self.grid, np.ascontiguousarray(z, dtype=np.float64))
        O.set_ghost_cells(self.g, 1, self.faces, full)
        return -O.laplace(self.g, full)


# how the dot products of the restated loops are accumulated.  "exact": the products in fp64 like the device's, their sum without a
# rounding error that matters (80-bit pairwise where numpy has it, else math.fsum) - the reference of the device tests.  "numpy":
# np.sum in fp64 (pairwise), a second legitimate order: how far the two drift apart is the measure of what a third order - the
# device's waves, slots and tree - may differ by.
_LONG = np.finfo(np.longdouble).nmant >= 63


def sum_exact(a: np.ndarray) -> float:
    return float(np.sum(a, dtype=np.longdouble)) if _LONG else math.fsum(a.ravel().tolist())


def sum_numpy(a: np.ndarray) -> float:
    return float(np.sum(a))


SUMS = {"exact": sum_exact, "numpy": sum_numpy}
CONVERGED, MAXITER, NONFINITE, BREAKDOWN = 0, 1, 2, 3


class Trajectory(NamedTuple):
    scalars: list        # (gamma, delta, rr, alpha, beta) of every update done
    iterates: list       # x after update 1, 2, ...: iterates[k - 1] = x_k (None where `keep` left it out)
    status: int          # 0 converged, 1 maxiter, 2 a non-finite scalar, 3 breakdown: the values of `pdehip_poisson_t.status`
    iterations: int
    residual: float      # sqrt(r.r) of the stop test that ended the loop
    rhs_norm: float      # ||v - f||_2 (after the projection of a singular system)
    x: np.ndarray        # the result: the last iterate; mean removed when a singular system converged


def cg_loop(v, minus_a, rhs, rtol, atol, maxiter, singular, sums="exact", precondition=None, keep=None) -> Trajectory:
    """The loop of `poisson_finish_kernel` / `poisson_update_kernel` (Chronopoulos-Gear, one reduction point per iteration) around
    w = (-A) z: gamma = r.z, delta = z.w, rr = r.r; the stop test in the kernel's order - non-finite, converged, maxiter, breakdown -;
    beta = gamma / gamma_prev, alpha = gamma / (delta - beta gamma / alpha_prev); p = z + beta p, q = w + beta q, x += alpha p,
    r -= alpha q.  `precondition`: z = M r (None: z = r and gamma = rr).  `keep`: the iteration numbers whose iterate is kept (None: all)."""
    dot = SUMS[sums] if isinstance(sums, str) else sums
    r = v - np.asarray(rhs, dtype=np.float64)
    size = float(r.size)
    if singular:
        r = r - dot(r) / size
    x, p, q = np.zeros_like(r), np.zeros_like(r), np.zeros_like(r)
    scalars, iterates = [], []
    gamma_prev = alpha_prev = 0.0
    iters, bnorm, tol = 0, 0.0, 0.0
    while True:
        z = r if precondition is None else precondition(r)
        w = minus_a(z)
        rr = dot(r * r)
        gamma = rr if precondition is None else dot(r * z)
        delta = dot(z * w)
        if iters == 0:
            bnorm = math.sqrt(rr) if rr >= 0 else float("nan")
            tol = max(rtol * bnorm, atol) if bnorm == bnorm else atol      # (the kernel: t > atol ? t : atol)
        if not (math.isfinite(gamma) and math.isfinite(delta) and math.isfinite(rr)):
            status = NONFINITE
            break
        if math.sqrt(rr) <= tol:
            status = CONVERGED
            break
        if iters >= maxiter:
            status = MAXITER
            break
        beta, denom = 0.0, delta
        if iters > 0:
            beta = gamma / gamma_prev
            denom = delta - beta * gamma / alpha_prev
        if not (delta > 0) or not (denom > 0) or not (gamma > 0):
            status = BREAKDOWN
            break
        alpha = gamma / denom
        iters += 1
        p = z + beta * p
        q = w + beta * q
        x = x + alpha * p
        r = r - alpha * q
        gamma_prev, alpha_prev = gamma, alpha
        scalars.append((gamma, delta, rr, alpha, beta))
        iterates.append(x if keep is None or iters in keep else None)
    residual = math.sqrt(rr) if rr >= 0 else float("nan")
    result = x - dot(x) / size if singular and status == CONVERGED else x
    return Trajectory(scalars, iterates, status, iters, residual, bnorm, result)


def cg(grid, bc, rhs, rtol=1e-10, atol=0.0, maxiter=1000, singular=False, sums="exact", keep=None) -> Trajectory:
    """Plain conjugate gradients on (-A) u = v - f exactly as the device states them; v = L(0) by `laplace_with_bcs`."""
    v = laplace_with_bcs(grid, bc, np.zeros(grid.shape))
    return cg_loop(v, HomogeneousOperator(grid, bc), rhs, rtol, atol, maxiter, singular, sums, None, keep)


def matrix_and_vector(grid, bc) -> tuple[np.ndarray, np.ndarray]:
    faces = host_faces(grid.get_boundary_conditions(bc))
    g = oracle_grid(grid)
    size = int(np.prod(grid.shape))

    def apply(valid):
        full = to_full(grid, valid)
        O.set_ghost_cells(g, 1, faces.c, full)
        return O.laplace(g, full).ravel().copy()

    vector = apply(np.zeros(grid.shape))
    matrix = np.empty((size, size))
    unit = np.zeros(size)
    for j in range(size):
        unit[j] = 1.0
        matrix[:, j] = apply(unit.reshape(grid.shape)) - vector
        unit[j] = 0.0
    return matrix, vector


def dense_solve(grid, bc, rhs: np.ndarray) -> np.ndarray:
    matrix, vector = matrix_and_vector(grid, bc)
    b = rhs.ravel() - vector
    if np.linalg.matrix_rank(matrix) == matrix.shape[0]:
        x = np.linalg.solve(matrix, b)
    else:
        x = np.linalg.lstsq(matrix, b, rcond=None)[0]      # minimum norm, like lsmr
        if not np.allclose(matrix @ x, b, rtol=1e-5, atol=1e-5):
            residual = np.linalg.norm(matrix @ x - b)
            msg = f"Poisson problem could not be solved (Residual: {residual})"
            raise NotSolved(msg)
    return x.reshape(grid.shape)
