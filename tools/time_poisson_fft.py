"""Times the direct Poisson solve of all-periodic grids (profiles/poisson_fft_time.md): ``method="fft"`` ALTERNATING in one process with
``method="mgcg"`` and ``method="cg"`` at their default ``rtol`` on the same grids and right-hand sides - 256^3 and 512^3 in fp64 and fp32,
and 1024 x 4096 in fp64.  Host wall time per solve on a resident right-hand side; between HIP events the whole C entry point
``pdehip_poisson_fft``, and its two transforms alone (``pdehip_fft_forward``, ``pdehip_fft_inverse`` on the same shapes): what is left is
the division, the ghost cells, ``A x``, the test sweep with the store, and the read-back of the sums.  The split of that rest by kernel
comes from a kernel trace in a run of its own.  ``info["residual"] / info["rhs_norm"]`` of each method is recorded next to the times.

    python tools/time_poisson_fft.py [output.md]
    python tools/time_poisson_fft.py --calls-only      (six direct solves at 512^3 fp64 alone, for a kernel trace in a run of its own)
"""

from __future__ import annotations

import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "py-pde_amd")]

import pde_hip  # noqa: E402
from pde_hip import _abi  # noqa: E402
from pde_hip.device import DeviceArray, DeviceBuffer  # noqa: E402
from pde_hip.solvers import ConvergenceError  # noqa: E402

REPS, WARM = 5, 2
SPECTRUM_FORWARD_MS = 3.59      # pdehip_fft_forward at 512^3 fp64, profiles/spectrum_time.md
backend = pde_hip.get_backend("hip")
lib = backend._lib


def events(fn, before=None):
    """Milliseconds between two HIP events around ``fn`` (device work, and whatever the entry point waits for in between)."""
    e0, e1 = C.c_void_p(), C.c_void_p()
    lib.event_create(C.byref(e0)); lib.event_create(C.byref(e1))
    out = []
    for i in range(WARM + REPS):
        if before is not None:
            before()
        lib.event_record(e0, None)
        fn()
        lib.event_record(e1, None)
        lib.event_synchronize(e1)
        ms = C.c_float()
        lib.event_elapsed_ms(e0, e1, C.byref(ms))
        if i >= WARM:
            out.append(ms.value)
    lib.event_destroy(e0); lib.event_destroy(e1)
    return np.array(out)


def once(fn):
    backend.synchronize()
    t0 = time.perf_counter()
    fn()
    backend.synchronize()
    return (time.perf_counter() - t0) * 1e3


def fmt(ms):
    ms = np.asarray(ms)
    return f"{np.median(ms):.3f} ms ({ms.min():.3f} .. {ms.max():.3f})"


def white(shape, dtype):
    data = np.random.default_rng(0).uniform(-1.0, 1.0, shape)
    data -= data.mean()
    return data.astype(dtype)


if "--calls-only" in sys.argv:
    grid = pde_hip.UnitGrid([512, 512, 512], periodic=True)
    dev = DeviceArray(backend.grid_info(grid, np.float64)).set_valid(white(grid.shape, np.float64))
    out = DeviceArray(dev.info)
    op = grid.make_operator("poisson_solver", "periodic", backend=backend, method="fft")
    for _ in range(6):
        op(dev, out=out)
    backend.synchronize()
    print(op.info)
    sys.exit(0)

CASES = [((256, 256, 256), np.float64), ((256, 256, 256), np.float32), ((512, 512, 512), np.float64), ((512, 512, 512), np.float32),
         ((1024, 4096), np.float64)]
# (repetitions of the iterative methods: the plain loop takes seconds at 512^3)
ITER_REPS = {"mgcg": 3, "cg": 1}
head = [f"# The direct Poisson solve of all-periodic grids ({backend.device_name})", "",
        "`python tools/time_poisson_fft.py`: one process.  \"wall\": host wall time of `op(rhs, out=out)` on a resident right-hand side (zero-mean",
        f"uniform(-1, 1)) for `method=\"fft\"` ({WARM} warm-up calls, then {REPS} timed ones, ALTERNATING with the other methods: one solve of each after",
        f"every direct solve until their repetitions are used up - {ITER_REPS['mgcg']} of `mgcg`, {ITER_REPS['cg']} of `cg`, each after one warm-up solve), all at the",
        "default `rtol = 1e-10`.  \"device\": between HIP events around the C entry point, median (min .. max); `pdehip_poisson_fft` waits for its",
        "stream once inside (the sums), which the events include.  \"rest\" is the whole call minus the two transforms: division, ghost cells,",
        "`A x`, the test sweep with the store, the read-back.  \"rel. residual\" is `info[\"residual\"] / info[\"rhs_norm\"]`: for `fft` the true",
        "residual `||A x - (f - mean f)||`, for the loops the recurrence's.", ""]
rows = ["| grid | fft, wall | mgcg, wall (iterations) | cg, wall (iterations) | mgcg / fft | poisson_fft, device | forward, device | inverse, device | rest |"
        " rel. residual fft / mgcg / cg |", "|---|---|---|---|---|---|---|---|---|---|"]
verdict = []
forward_512 = None
for shape, dtype in CASES:
    name = f"{'x'.join(map(str, shape))} {np.dtype(dtype).name}"
    print(f"timing {name}", file=sys.stderr, flush=True)
    grid = pde_hip.UnitGrid(list(shape), periodic=True)
    info = backend.grid_info(grid, dtype)
    dev = DeviceArray(info).set_valid(white(shape, dtype))
    out = DeviceArray(info)
    ops = {m: grid.make_operator("poisson_solver", "periodic", backend=backend, method=m) for m in ("fft", "mgcg", "cg")}
    walls = {m: [] for m in ops}
    failed = {}

    def solve(m):
        try:
            ops[m](dev, out=out)
        except ConvergenceError as err:
            failed[m] = str(err)

    for _ in range(WARM):
        solve("fft")
    for m in ("mgcg", "cg"):
        solve(m)                    # warm-up: the handle, the hierarchy
    for i in range(REPS):
        walls["fft"].append(once(lambda: solve("fft")))
        for m in ("mgcg", "cg"):
            if i < ITER_REPS[m]:
                walls[m].append(once(lambda: solve(m)))
    rel = {m: ops[m].info["residual"] / ops[m].info["rhs_norm"] for m in ops}
    iters = {m: ops[m].info["iterations"] for m in ops}
    # the entry points alone
    cells = int(np.prod(shape))
    half = cells // shape[-1] * (shape[-1] // 2 + 1)
    spec = DeviceBuffer(16 * half)
    io = _abi.Poisson()
    io.rtol, io.atol = 1e-10, 0.0
    t_all = events(lambda: lib.poisson_fft(info.ref, dev.ptr, out.ptr, C.byref(io), None))
    t_fwd = events(lambda: lib.fft_forward(info.ref, 1, dev.ptr, spec.ptr, None))
    info64 = backend.grid_info(grid, np.float64)
    x64 = DeviceArray(info64)
    t_inv = events(lambda: lib.fft_inverse(info64.ref, 1, spec.ptr, x64.ptr, None), before=lambda: lib.fft_forward(info.ref, 1, dev.ptr, spec.ptr, None))
    rest = np.median(t_all) - np.median(t_fwd) - np.median(t_inv)
    if shape == (512, 512, 512) and np.dtype(dtype) == np.float64:
        forward_512 = np.median(t_fwd)
    ratio = np.median(walls["mgcg"]) / np.median(walls["fft"])
    verdict.append((name, np.median(walls["fft"]), np.median(walls["mgcg"]), ratio))
    note = lambda m: f"{fmt(walls[m])} ({iters[m]}{', NOT converged' if m in failed else ''})"          # noqa: E731
    rows.append(f"| {name} | {fmt(walls['fft'])} | {note('mgcg')} | {note('cg')} | {ratio:.1f}x | {fmt(t_all)} | {fmt(t_fwd)} | {fmt(t_inv)} | {rest:.3f} ms |"
                f" {rel['fft']:.2e} / {rel['mgcg']:.2e} / {rel['cg']:.2e} |")
    for op in ops.values():
        op.solver_for(None).release()          # the handles and the hierarchy of this grid
    del dev, out, spec, x64, ops
    lib.release_scratch()
slower = [v for v in verdict if v[3] <= 1.0]
tail = ["", "The one condition of this feature: at every measured shape the direct solve is faster than `mgcg` in the same process.  Measured: "
        + ", ".join(f"{name}: {f:.2f} ms against {m:.2f} ms ({r:.1f} times)" for name, f, m, r in verdict) + "."
        + ("  It HOLDS at every shape." if not slower else "  It FAILS at: " + ", ".join(v[0] for v in slower) + ".")]
if forward_512 is not None:
    tail += ["", f"`pdehip_fft_forward` at 512^3 fp64 in this run: {forward_512:.2f} ms, against the {SPECTRUM_FORWARD_MS} ms of profiles/spectrum_time.md."]
text = "\n".join(head + rows + tail)
print(text)
if len(sys.argv) > 1:
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text(text + "\n")
