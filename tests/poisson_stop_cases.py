"""The stop rule and the return statuses of the Poisson solver on the device, for both methods: the bodies of the tests of
tests/test_hip_poisson.py (method "cg") and tests/test_hip_poisson_mg.py (method "mgcg").  The expected iteration counts come from
the restated loops (tests/poisson_cases.py, tests/poisson_mg_cases.py) with exact dot products."""

from __future__ import annotations

import numpy as np
import pytest

import pde_hip
from poisson_cases import BREAKDOWN, CONVERGED, FACES1, INDEFINITE, cg, matrix_and_vector
from poisson_cases import FACES2 as BC2
from poisson_mg_cases import mgcg


def grid2():
    return pde_hip.CartesianGrid([[0, 33.0], [0, 15.5]], [33, 31])


def restate(method, grid, bc, f, **kwargs):
    return (cg if method == "cg" else mgcg)(grid, bc, f, sums="exact", keep=(), **kwargs)


def check_atol(backend, method):
    """rtol = 0, atol = a: the solve stops with residual <= a at the restatement's iteration; an atol below rtol * |b| changes no bit."""
    grid = grid2()
    f = np.random.default_rng(21).uniform(-1, 1, grid.shape)
    first = grid.make_operator("poisson_solver", BC2, backend=backend, method=method, rtol=1e-8)
    base = first(f)
    for scale in (1e-3, 1e-6):
        a = scale * first.info["rhs_norm"]
        want = restate(method, grid, BC2, f, rtol=0.0, atol=a, maxiter=1000 if method == "cg" else 200)
        op = grid.make_operator("poisson_solver", BC2, backend=backend, method=method, rtol=0.0, atol=a)
        op(f)
        assert want.status == CONVERGED and op.info["converged"]
        assert op.info["residual"] <= a and op.info["iterations"] == want.iterations > 0, (op.info, want.iterations)
    below = grid.make_operator("poisson_solver", BC2, backend=backend, method=method, rtol=1e-8, atol=1e-3 * 1e-8 * first.info["rhs_norm"])
    assert np.array_equal(below(f), base)
    assert below.info["iterations"] == first.info["iterations"] and below.info["residual"] == first.info["residual"]
    # ... and one above it ends the solve earlier
    above = grid.make_operator("poisson_solver", BC2, backend=backend, method=method, rtol=1e-8, atol=1e-4 * first.info["rhs_norm"])
    above(f)
    assert 0 < above.info["iterations"] < first.info["iterations"] and above.info["residual"] <= 1e-4 * first.info["rhs_norm"]


def check_zero_iterations(backend, method):
    """f = L(0): the first residual is zero, the solve converges without an update and the result is exactly zero."""
    grid = grid2()
    op = grid.make_operator("poisson_solver", {"value": 0.0}, backend=backend, method=method)
    got = op(np.zeros(grid.shape))                                        # Laplace's equation between homogeneous Dirichlet walls
    assert op.info["converged"] and op.info["iterations"] == 0 and op.info["residual"] == 0.0 and op.info["rhs_norm"] == 0.0
    assert not got.any()
    v = pde_hip.ScalarField(grid, 0.0).laplace(BC2).data                  # inhomogeneous walls: f = v
    assert np.abs(v).max() > 0
    op = grid.make_operator("poisson_solver", BC2, backend=backend, method=method)
    got = op(v)
    assert op.info["converged"] and op.info["iterations"] == 0 and op.info["residual"] == 0.0 and not got.any()
    # the same operator goes on to an ordinary right-hand side
    f = np.random.default_rng(22).uniform(-1, 1, grid.shape)
    assert np.array_equal(op(f), grid.make_operator("poisson_solver", BC2, backend=backend, method=method)(f)) and op.info["iterations"] > 0


def check_nonfinite(backend, method):
    """A NaN or an inf in ONE cell of the right-hand side: status 2 as an exception, and the operator solves afterwards."""
    grid = grid2()
    f = np.random.default_rng(23).uniform(-1, 1, grid.shape)
    fresh = grid.make_operator("poisson_solver", BC2, backend=backend, method=method)(f)
    for bad, where in ((np.nan, (32, 30)), (np.inf, (0, 0)), (-np.inf, (17, 30))):
        op = grid.make_operator("poisson_solver", BC2, backend=backend, method=method)
        g = f.copy()
        g[where] = bad
        with pytest.raises(RuntimeError, match="not finite") as err:
            op(g)
        assert not isinstance(err.value, pde_hip.ConvergenceError)
        assert op.info["iterations"] == 0 and not op.info["converged"]
        assert np.array_equal(op(f), fresh) and op.info["converged"]


def check_breakdown(backend, method="cg"):
    """An indefinite system: status 3 as an exception (not a ConvergenceError, not a device fault), at the restatement's iteration;
    the operator survives.

    Plain loop: delta = r.w is positive for the first residual but the denominator p.q of the second direction is not: breakdown
    after ONE update in either summation mode, and the device must agree exactly.
    Preconditioned loop: the grid has one level, the cycle is 32 Jacobi sweeps whose omega / d is zero in the cell with the negative
    diagonal, so z = M r stays zero there and z.(-A) z is a positive form: no denominator ever turns negative.  The residual in
    that cell is never reduced, gamma = r.z shrinks by a constant factor per iteration and the loop ends when it underflows
    (gamma about 1e-321 after some 30 iterations).  Where exactly a product rounds to zero moves by an iteration with the order
    of the sums (29 and 30 for the two modes of the restatement on one right-hand side): the device may be 3 iterations off the
    exact-sum restatement, and its residual - the part of r the loop cannot reach, constant over the last iterations - must agree."""
    grid = pde_hip.UnitGrid(INDEFINITE["shape"])
    bc = INDEFINITE["bc"]
    f = np.random.default_rng(INDEFINITE["seed"]).uniform(-1, 1, grid.shape)
    want = restate(method, grid, bc, f, rtol=1e-10, maxiter=100)
    assert want.status == BREAKDOWN and (want.iterations == 1 if method == "cg" else 20 <= want.iterations <= 40)
    slack = 0 if method == "cg" else 3
    op = grid.make_operator("poisson_solver", bc, backend=backend, method=method, maxiter=100)
    seen = []
    for _ in range(2):                                                    # the second call: the handle is as it was
        with pytest.raises(RuntimeError, match="breakdown") as err:
            op(f)
        assert not isinstance(err.value, pde_hip.ConvergenceError)
        assert abs(op.info["iterations"] - want.iterations) <= slack and not op.info["converged"], (op.info, want.iterations)
        assert abs(op.info["residual"] - want.residual) <= 1e-12 * want.residual
        seen.append((op.info["iterations"], op.info["residual"]))
    assert seen[0] == seen[1]
    # a right-hand side this operator can solve.  Every right-hand side: f = L(0), which needs no update ...
    v = pde_hip.ScalarField(grid, 0.0).laplace(bc).data
    got = op(v)
    assert op.info["converged"] and op.info["iterations"] == 0 and not got.any()
    if method == "cg":
        # ... plain loop: a first residual that is an eigenvector of -A with a positive eigenvalue is solved by ONE update, which goes
        # through gamma, alpha, p and q of the handle: bits equal to those of an operator that never failed
        matrix, vector = matrix_and_vector(grid, bc)
        values, vectors = np.linalg.eigh(-matrix)
        assert values[0] < 0 < values[3]
        good = vector.reshape(grid.shape) - vectors[:, 3].reshape(grid.shape)
        got = op(good)
        assert op.info["converged"] and op.info["iterations"] >= 1
        fresh = grid.make_operator("poisson_solver", bc, backend=backend, method=method, maxiter=100)
        assert np.array_equal(got, fresh(good)) and fresh.info == op.info
        assert np.abs(got - vectors[:, 3].reshape(grid.shape) / values[3]).max() <= 1e-10 * np.abs(got).max()      # (-A) u = e: u = e / lambda
    # (preconditioned loop: no such right-hand side exists.  Unless r is zero, the first update puts a residual into the cell the cycle
    # cannot reach - q = (-A) z couples it to its neighbour - and the loop ends in breakdown as above.)
    # ... and the device goes on: a definite system on the same grid
    ok = grid.make_operator("poisson_solver", FACES1, backend=backend, method=method)
    assert np.isfinite(ok(f)).all() and ok.info["converged"]
