"""Timing of the Poisson solver on the device: milliseconds per conjugate-gradient iteration and iterations / wall time to a given
tolerance, all-Dirichlet faces, fp64, random right-hand side.  Prints a markdown table (profiles/poisson_time.md is one run of it).

    python tools/time_poisson.py [--sizes 256 512] [--shape 500 500 300] [--method cg|mgcg] [--periodic] [--rtol 1e-8] [--fixed 200]

Per size two solves on device-resident arrays: `--fixed` iterations with rtol = 0 (the solve ends in ConvergenceError by design: the
time is that of exactly that many iterations, batches of 32) and one solve to `--rtol`.  Bytes an iteration must move: 11 array passes
of 8 bytes per cell (sweep 1 reads r and writes w; sweep 2 reads r, w, p, q, x and writes p, q, x, r).  `--method mgcg` (the multigrid
preconditioner; profiles/poisson_mg_time.md): 26.2 fine-level passes - the cycle with two sweeps before and after: 2 + 2.1 + 2.1 +
2 x 3, sweep 1 three reads and a write less the cached one: 3, sweep 2 six reads and four writes: 10 - and 1/7 of the cycle's for the
coarser levels in 3-D.  `--periodic`: Neumann x periodic faces instead (a singular system; the right-hand side gets mean zero).
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "py-pde_amd")]

import pde_hip  # noqa: E402
from pde_hip.device import DeviceArray  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--fixed", type=int, default=200)
    ap.add_argument("--shape", type=int, nargs="+", default=None, help="one grid of this shape instead of the cubes of --sizes")
    ap.add_argument("--method", default="cg", choices=["cg", "mgcg"])
    ap.add_argument("--periodic", action="store_true", help="Neumann faces on axis 0, periodic axes else (singular)")
    args = ap.parse_args()
    method = {"method": args.method}
    passes = 11 if args.method == "cg" else 13 + 12.2 * 8 / 7
    backend = pde_hip.get_backend("hip")
    print(f"device: {backend.device_name}\n")
    print("| grid | ms / iteration | GB / iteration | TB/s | iterations to rtol | wall s to rtol | true residual / ||f - v|| |")
    print("|---|---|---|---|---|---|---|")
    print(f"method: {args.method}\n")
    for shape in ([args.shape] if args.shape else [[n, n, n] for n in args.sizes]):
        n = shape[0]
        grid = pde_hip.UnitGrid(shape, periodic=[a > 0 for a in range(len(shape))] if args.periodic else False)
        info = backend.grid_info(grid, np.float64)
        f = np.random.default_rng(n).uniform(-1, 1, grid.shape)
        if args.periodic:
            f -= f.mean()
        rhs = DeviceArray(info).set_valid(f, backend.stream)
        out = DeviceArray(info)
        bc = [{"derivative": 0.0}] + ["periodic"] * (len(shape) - 1) if args.periodic else {"value": 0.0}
        fixed = grid.make_operator("poisson_solver", bc, backend=backend, rtol=0.0, maxiter=args.fixed, **method)
        per_iter = []
        for _ in range(3):      # the first call creates the handle
            backend.synchronize()
            t0 = time.perf_counter()
            try:
                fixed(rhs, out=out)
            except pde_hip.ConvergenceError:
                pass
            backend.synchronize()
            per_iter.append((time.perf_counter() - t0) / args.fixed * 1e3)
        ms = min(per_iter[1:])
        gb = passes * 8 * float(np.prod(shape)) / 1e9
        op = grid.make_operator("poisson_solver", bc, backend=backend, rtol=args.rtol, **method)
        op(rhs, out=out)       # warm-up: handle
        backend.synchronize()
        t0 = time.perf_counter()
        op(rhs, out=out)
        backend.synchronize()
        wall = time.perf_counter() - t0
        u = pde_hip.ScalarField(grid, out.get_valid(stream=backend.stream))
        resid = np.linalg.norm((u.laplace(bc).data - f).ravel()) / np.linalg.norm(f.ravel())
        name = " x ".join(str(m) for m in shape) + (f" ({op.info['levels']} levels)" if "levels" in op.info else "")
        print(f"| {name} | {ms:.3f} | {gb:.2f} | {gb / ms:.2f} | {op.info['iterations']} | {wall:.2f} | {resid:.2e} |", flush=True)


if __name__ == "__main__":
    main()
