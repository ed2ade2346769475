"""Time the implicit Euler / Crank-Nicolson loops (pdehip_fixedpoint_run) through the solver interface.

usage: python tools/time_implicit.py [size] [diffusion|cahn_hilliard] [f8|f4] [ndim]
Prints ms per fixed-point iteration (HIP events around `steps` steps after a warm-up, divided by the iterations the steps took,
first estimates included as one more sweep each) for both schemes, next to the plain stage sweep of the same right-hand side
(one `pdehip_ab2_step` sweep: slope + one pointwise combination = the LAP_STAGE / E2_CH_STAGE sweep with the same number of arrays).
PDEHIP_FIXEDPOINT_BATCH=1 times the loop with one read of the control block per iteration (host time per step of small grids).
"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "py-pde_amd"))
import pde_hip  # noqa: E402
from pde_hip.device import DeviceArray  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
kind = sys.argv[2] if len(sys.argv) > 2 else "diffusion"
dtype = np.dtype(sys.argv[3] if len(sys.argv) > 3 else "f8")
ndim = int(sys.argv[4]) if len(sys.argv) > 4 else 3
steps, warm = int(os.environ.get("STEPS", "20")), int(os.environ.get("WARMUP", "5"))
backend = pde_hip.get_backend("hip")
lib = backend._lib
grid = pde_hip.UnitGrid([n] * ndim, periodic=True)
eq = pde_hip.DiffusionPDE(0.5) if kind == "diffusion" else pde_hip.CahnHilliardPDE()
data = (0.3 * np.random.default_rng(0).uniform(-1, 1, grid.shape)).astype(dtype)
dt = 0.05 if kind == "diffusion" else 0.002
e0, e1 = C.c_void_p(), C.c_void_p()
lib.event_create(C.byref(e0)); lib.event_create(C.byref(e1))
ms = C.c_float()
label = f"{'x'.join(str(s) for s in grid.shape)} {dtype.name} {kind}"

for solver in ("implicit", "crank-nicolson"):
    sol = pde_hip.solvers.SolverBase.from_name(solver, pde=eq, backend=backend, maxerror=1e-3 if dtype == np.float32 else 1e-4)
    state = pde_hip.ScalarField(grid, data.copy(), dtype=dtype)
    sol.info["dt"] = dt
    sol.info["steps"] = 0
    inner = backend.make_inner_stepper(sol, state)
    dev = DeviceArray(backend.grid_info(grid, dtype)).set_valid(state.data, backend.stream)
    inner(dev, 0.0, warm * dt)
    lib.stream_synchronize(backend.stream)
    before = len(sol.info["iterations"])
    t0 = time.perf_counter()
    lib.event_record(e0, backend.stream)
    inner(dev, warm * dt, (warm + steps) * dt)
    lib.event_record(e1, backend.stream)
    lib.stream_synchronize(backend.stream)
    wall = (time.perf_counter() - t0) * 1e3
    lib.event_elapsed_ms(e0, e1, C.byref(ms))
    its = sol.info["iterations"][before:]
    sweeps = sum(its) + len(its) * (2 if solver == "crank-nicolson" else 1)
    print(f"| {label} | {solver} | batch={os.environ.get('PDEHIP_FIXEDPOINT_BATCH', 'adaptive')} | {steps} steps, {sum(its)} iterations | "
          f"{ms.value / sweeps:.4f} ms per sweep | {ms.value / steps:.4f} ms per step (events) | {wall / steps:.4f} ms per step (host) | "
          f"{lib.last_kernel_name().decode()} |", flush=True)

# the plain stage sweep of the same right-hand side with the same arrays (slope + one combination): the Adams-Bashforth sweep
spec = backend.make_rhs_spec(eq, pde_hip.ScalarField(grid, data.copy(), dtype=dtype))
arrs = [DeviceArray(spec.info) for _ in range(4)]
arrs[0].set_valid(data, backend.stream)
fused = C.c_int(0)


def stage():
    lib.ab2_step(spec.info.ref, spec.ref, arrs[0].ptr, arrs[1].ptr, arrs[2].ptr, arrs[3].ptr, 1e-6, C.byref(fused), backend.stream)


for _ in range(warm):
    stage()
lib.stream_synchronize(backend.stream)
lib.event_record(e0, backend.stream)
for _ in range(steps * 5):
    stage()
lib.event_record(e1, backend.stream)
lib.stream_synchronize(backend.stream)
lib.event_elapsed_ms(e0, e1, C.byref(ms))
print(f"| {label} | stage sweep (pdehip_ab2_step, fused={fused.value}) | | | {ms.value / (steps * 5):.4f} ms per sweep | | | {lib.last_kernel_name().decode()} |", flush=True)
