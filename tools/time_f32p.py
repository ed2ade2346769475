"""Times the pure-fp32 arithmetic mode of fp32 fields (profiles/f32p_time.md): the Laplacian at 512^3 and the diffusion Euler loop at
512^3 and 513^3, against the default fp32 path (fp64 registers) of this library and of the PARENT commit's library, all three alternating
in the same process on the same device (boxes differ by +-5 %).  HIP events, warm-up, medians of repeated launches.

    python tools/time_f32p.py [--parent <libpdehip.so of the parent commit>] [output.md]

The parent's library: a checkout of the parent commit built into a second directory (`git archive HEAD~ py-pde_amd include | tar -x -C
<dir>; make -C <dir>/py-pde_amd`); device memory is shared by the two libraries (one process, one HIP runtime).
"""

from __future__ import annotations

import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "py-pde_amd")]

import pde_hip  # noqa: E402
from pde_hip import _abi  # noqa: E402
from pde_hip._lib import _Lib  # noqa: E402
from pde_hip.device import DeviceArray  # noqa: E402

REPS, WARM, STEPS, LAPS = 9, 2, 32, 8
PEAK = 8.0e12          # bytes per second of HBM3E (MI355X)

args = sys.argv[1:]
parent = None
if args and args[0] == "--parent":
    parent = _Lib(Path(args[1]))
    args = args[2:]
backend = pde_hip.get_backend("hip")
lib = backend._lib
libs = {"fp32 mode": lib, "default (this library)": lib}
if parent is not None:
    libs["default (parent library)"] = parent


def timed(fn):
    """Milliseconds between two HIP events around one call of ``fn``."""
    e0, e1 = C.c_void_p(), C.c_void_p()
    lib.event_create(C.byref(e0)); lib.event_create(C.byref(e1))
    lib.event_record(e0, None)
    fn()
    lib.event_record(e1, None)
    lib.event_synchronize(e1)
    ms = C.c_float()
    lib.event_elapsed_ms(e0, e1, C.byref(ms))
    lib.event_destroy(e0); lib.event_destroy(e1)
    return ms.value


def alternate(calls: dict):
    """Every call WARM + REPS times, the calls alternating; name -> (array of ms, kernel name of the last launch)."""
    out = {name: [] for name in calls}
    names = {}
    for i in range(WARM + REPS):
        for name, (owner, fn) in calls.items():
            ms = timed(fn)
            names[name] = owner.last_kernel_name().decode()
            if i >= WARM:
                out[name].append(ms)
    return {name: (np.array(v), names[name]) for name, v in out.items()}


def fmt(ms):
    return f"{np.median(ms):.3f} ({ms.min():.3f} .. {ms.max():.3f})"


def make_grid(n, periodic, spacing):
    if spacing == 1.0:
        return pde_hip.UnitGrid([n] * 3, periodic=periodic)
    return pde_hip.CartesianGrid([(0.0, n * spacing)] * 3, [n] * 3, periodic=periodic)


lines = [f"# Pure-fp32 arithmetic mode: timings ({backend.device_name})", "",
         f"`python tools/time_f32p.py --parent <parent library>`: {WARM} warm-up launches, {REPS} timed launches per variant, the variants "
         f"alternating in one process; ms = median (min .. max) of HIP-event times.  An Euler launch is {STEPS} steps; a Laplacian time is one of "
         f"{LAPS} launches timed together.  "
         "\"of 8 TB/s\": the bytes a launch must move (one read and one write of the valid cells per sweep) per second, over 8 TB/s.", ""]
rng = np.random.default_rng(0)

# ---- Laplacian ---------------------------------------------------------------------------------------------------------------------
lines += ["## Laplacian, fp32, 512^3", "", "| spacing | variant | ms per launch | Gcell/s | of 8 TB/s | kernel | time / parent default |", "|---|---|---|---|---|---|---|"]
for spacing in (1.0, 0.5):
    grid = make_grid(512, True, spacing)
    info = backend.grid_info(grid, np.float32)
    src, dst = DeviceArray(info), DeviceArray(info)
    src.set_valid(rng.uniform(-1, 1, grid.shape).astype(np.float32))
    def launches(o, new):
        for _ in range(LAPS):
            (o.laplace_f32p if new else o.laplace)(info.ref, src.ptr, dst.ptr, _abi.OUT_FULL, None)

    calls = {name: (owner, (lambda o=owner, new=(name == "fp32 mode"): launches(o, new))) for name, owner in libs.items()}
    res = {name: (ms / LAPS, kernel) for name, (ms, kernel) in alternate(calls).items()}
    cells = float(np.prod(grid.shape))
    base = np.median(res[list(libs)[-1]][0])
    for name, (ms, kernel) in res.items():
        med = np.median(ms)
        lines.append(f"| {spacing:g} | {name} | {fmt(ms)} | {cells / med / 1e6:.1f} | {cells * 8 / (med * 1e-3) / PEAK:.3f} | `{kernel}` | {med / base:.3f} |")
    del src, dst

# ---- Euler loop ---------------------------------------------------------------------------------------------------------------------
lines += ["", f"## Diffusion Euler loop, fp32, {STEPS} steps per launch", "",
          "| grid | faces | spacing, D | variant | ms per launch | ms per step | Gcell-steps/s | of 8 TB/s | kernel | time / parent default |", "|---|---|---|---|---|---|---|---|---|---|"]
cases = [(512, True, 1.0, 1.0), (512, True, 0.5, 0.7), (513, True, 1.0, 1.0), (513, True, 0.5, 0.7), (512, False, 1.0, 1.0)]
for n, periodic, spacing, D in cases:
    grid = make_grid(n, periodic, spacing)
    eq = pde_hip.DiffusionPDE(D)        # auto_periodic_neumann: zero-derivative faces on the axes that are not periodic
    spec = backend.make_rhs_spec(eq, pde_hip.ScalarField(grid, dtype=np.float32))
    info = spec.info
    a, b = DeviceArray(info), DeviceArray(info)
    a.set_valid(rng.uniform(-1, 1, grid.shape).astype(np.float32))
    dt = 0.2 / (D * 3 * spacing ** -2)
    out = C.c_void_p()
    calls = {name: (owner, (lambda o=owner, new=(name == "fp32 mode"): (o.euler_run_f32p if new else o.euler_run)(info.ref, spec.ref, a.ptr, b.ptr, dt, STEPS, C.byref(out), None)))
             for name, owner in libs.items()}
    res = alternate(calls)
    cells = float(np.prod(grid.shape))
    base = np.median(res[list(libs)[-1]][0])
    for name, (ms, kernel) in res.items():
        med = np.median(ms)
        per_sweep = 4 if "four" in kernel or "euler4" in kernel else (2 if "two-step" in kernel or "euler2" in kernel else 1)
        moved = cells * 8 * STEPS / per_sweep
        lines.append(f"| {n}^3 | {'periodic' if periodic else 'zero-derivative'} | {spacing:g}, {D:g} | {name} | {fmt(ms)} | {med / STEPS:.3f} | "
                     f"{cells * STEPS / med / 1e6:.1f} | {moved / (med * 1e-3) / PEAK:.3f} ({per_sweep} steps per sweep) | `{kernel}` | {med / base:.3f} |")
    del a, b, spec

text = "\n".join(lines)
print(text)
if args:
    Path(args[0]).parent.mkdir(parents=True, exist_ok=True)
    Path(args[0]).write_text(text + "\n")
