"""A dense numpy restatement of the reference's `poisson_solver` (tests only): the Laplacian with its boundary conditions as a matrix
plus a constant vector - `L u = A u + v`, the reference's `_get_laplace_matrix` - built from the CPU oracle's Laplacian and ghost-cell
setter (column j of A = L(e_j) - L(0), v = L(0)), solved like pde/backends/scipy/operators/common.py:99-141 solves it: directly when
the matrix is regular, the minimum-norm least-squares solution plus the `allclose` test when it is singular."""

from __future__ import annotations

import numpy as np

import pde_hip
from helpers import host_faces, oracle_grid, to_full
from oracle import pde_oracle as O


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
