"""Plain numpy restatement of the reference's fixed-point solvers around the CPU oracle's right-hand sides (the checker of
tests/test_hip_implicit.py and tests/test_implicit_cpu.py; no reference needed).

Implicit Euler (``pde/solvers/implicit.py:74-110``) and Crank-Nicolson (``pde/solvers/crank_nicolson.py:80-113``): the operations of
the reference in their order, evaluated in fp64 and rounded to the state's type where the reference stores an array of that type
at the end of an update; the convergence norm is summed in fp64."""

from __future__ import annotations

import numpy as np

from helpers import host_faces, oracle_grid, to_full
from oracle import pde_oracle as O
from pde_hip import _abi


class NotConverged(RuntimeError):
    pass


def oracle_rhs(grid, eq, dtype=np.float64):
    """``rhs(valid, t) -> valid`` of a class PDE (DiffusionPDE / CahnHilliardPDE of pde_hip) with constant faces, through the oracle."""
    g = oracle_grid(grid, dtype)
    nd = grid.num_axes
    inner = (slice(1, -1),) * nd
    name = type(eq).__name__
    if name == "DiffusionPDE":
        faces = host_faces(grid.get_boundary_conditions(eq.bc))
        spec = O.make_rhs(_abi.RHS_DIFFUSION, float(eq.diffusivity), faces.c)
        keep = (faces,)
    elif name == "CahnHilliardPDE":
        fc = host_faces(grid.get_boundary_conditions(eq.bc_c))
        fm = host_faces(grid.get_boundary_conditions(eq.bc_mu))
        scratch = np.zeros(grid._shape_full, dtype=dtype)
        spec = O.make_rhs(_abi.RHS_CAHN_HILLIARD, float(eq.interface_width), fc.c, fm.c, scratch)
        keep = (fc, fm, scratch)
    else:
        raise NotImplementedError(name)

    def rhs(valid, t):
        full = to_full(grid, np.ascontiguousarray(valid, dtype=dtype))
        return np.ascontiguousarray(O.rhs_scaled(g, spec, full, 1.0)[inner])

    rhs.keep = keep
    return rhs


def err_norm(new, prev) -> float:
    d = (new.astype(np.complex128) - prev) if np.iscomplexobj(new) else (new.astype(np.float64) - prev.astype(np.float64))
    return float(np.sum(d.real**2 + d.imag**2) if np.iscomplexobj(d) else np.sum(d * d)) / new.size


def fixedpoint_run(rhs, state, dt, steps, scheme="implicit", maxiter=100, maxerror=1e-4, explicit_fraction=0.0, t0=0.0, hook=None, errs=None):
    """Returns (final state, right-hand-side evaluations, iterations per step).  ``hook(state, t) -> state`` runs after every step;
    ``errs``: a list that receives every norm the stop test compares."""
    dtype = state.dtype
    wide = np.complex128 if np.iscomplexobj(state) else np.float64
    state = state.copy()
    evals, counts = 0, []
    for s in range(steps):
        t = t0 + s * dt
        state_t = state.astype(wide)
        if scheme == "implicit":
            new = (state_t + dt * rhs(state, t).astype(wide)).astype(dtype)
            evals += 1
        else:
            rate_t = rhs(state, t).astype(wide)
            cn = state_t + dt / 2 * (rhs(state, t + dt).astype(wide) + rate_t)
            new = (explicit_fraction * state_t + (1 - explicit_fraction) * cn).astype(dtype)
            evals += 2
        for n in range(maxiter):
            prev = new
            r = rhs(prev, t + dt).astype(wide)
            evals += 1
            if scheme == "implicit":
                new = (state_t + dt * r).astype(dtype)
            else:
                cn = state_t + dt / 2 * (r + rate_t)
                new = (explicit_fraction * prev.astype(wide) + (1 - explicit_fraction) * cn).astype(dtype)
            err = err_norm(new, prev)
            if errs is not None:
                errs.append(err)
            if err < maxerror**2:
                counts.append(n + 1)
                break
        else:
            counts.append(maxiter)
            msg = ("Implicit Euler" if scheme == "implicit" else "Crank-Nicolson") + " step did not converge."
            raise NotConverged(msg)
        state = new
        if hook is not None:
            state = hook(state, t)
    return state, evals, counts
