"""Times the statistics sweeps on the device (profiles/stats_time.md): ``pdehip_field_stats`` with and without the second sweep and
``pdehip_steady_state`` at 256^3 and 512^3, fp64 and fp32, next to the two yardsticks that exist - ``pdehip_integrate`` on the same array
and the full download (``DeviceArray.get_valid``) of the same state - and to the on-device copy (``pdehip_copy_nt``) of the same bytes.
HIP events for the device work, host wall time for what a tracker interrupt costs end to end.  One process: warm-up, 7 repetitions,
median and spread (min .. max).

    python tools/time_stats.py [output.md]
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
from pde_hip.device import DeviceArray, DeviceBuffer  # noqa: E402

REPS, WARM = 7, 2
backend = pde_hip.get_backend("hip")
lib = backend._lib


def events(fn):
    """Milliseconds between two HIP events around ``fn`` (device work only)."""
    e0, e1 = C.c_void_p(), C.c_void_p()
    lib.event_create(C.byref(e0)); lib.event_create(C.byref(e1))
    out = []
    for i in range(WARM + REPS):
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


def wall(fn):
    out = []
    for i in range(WARM + REPS):
        backend.synchronize()
        t0 = time.perf_counter()
        fn()
        backend.synchronize()
        if i >= WARM:
            out.append((time.perf_counter() - t0) * 1e3)
    return np.array(out)


def fmt(ms):
    return f"{np.median(ms):.3f} ms ({ms.min():.3f} .. {ms.max():.3f})"


def rate(nbytes, ms):
    return nbytes / np.median(ms) / 1e9      # TB/s


lines = [f"# Statistics on the device ({backend.device_name})", "",
         f"`python tools/time_stats.py`: one process, {WARM} warm-up runs, {REPS} timed repetitions, median (min .. max).  Device times between HIP",
         "events; \"interrupt\" columns are host wall time of the whole call, the download of the 64 / 16 result bytes included.  TB/s counts the",
         "bytes the sweep has to move: the interior once (8 B per fp64 cell), twice with the second sweep, three times for the steady-state sweep",
         "(two loads, one store); the copy moves every byte of the array twice.", "",
         "| state | copy_nt (yardstick) | integrate (yardstick) | field_stats | field_stats + m2 | steady_state | download get_valid (wall) |"
         " stats interrupt (wall) | stats + m2 interrupt (wall) | steady interrupt (wall) | download / slowest interrupt |",
         "|---|---|---|---|---|---|---|---|---|---|---|"]
ratios = []
rng = np.random.default_rng(0)
stats = backend.make_statistics()
for n in (256, 512):
    for dtype in (np.float64, np.float32):
        grid = pde_hip.UnitGrid([n, n, n], periodic=True)
        info = backend.grid_info(grid, dtype)
        cur, last = DeviceArray(info), DeviceArray(info)
        host = rng.uniform(0.5, 1.5, grid.shape).astype(dtype)
        cur.set_valid(host)
        lib.memcpy_d2d(last.ptr, cur.ptr, cur.nbytes, None)
        out = DeviceBuffer(64)
        interior = host.nbytes
        t_copy = events(lambda: lib.copy_nt(last.ptr, cur.ptr, cur.nbytes, None))
        t_int = events(lambda: lib.integrate(info.ref, 1, cur.ptr, 1.0, out.ptr, None))
        t_s1 = events(lambda: lib.field_stats(info.ref, 1, cur.ptr, 0, 0, out.ptr, None))
        t_s2 = events(lambda: lib.field_stats(info.ref, 1, cur.ptr, 0, 1, out.ptr, None))
        t_ss = events(lambda: lib.steady_state(info.ref, 1, cur.ptr, last.ptr, 0.37, 1e-5, out.ptr, None))
        t_down = wall(lambda: cur.get_valid(out=host))
        w_s1 = wall(lambda: stats(cur))
        w_s2 = wall(lambda: stats(cur, variance=True))
        check = backend.make_steady_state_check()
        check.update(cur, 0.0)
        clock = [0.0]

        def steady():
            clock[0] += 1.0
            check.update(cur, clock[0])

        w_ss = wall(steady)
        slowest = max(np.median(w_s1), np.median(w_s2), np.median(w_ss))
        ratio = np.median(t_down) / slowest
        ratios.append((n, np.dtype(dtype).name, ratio))
        lines.append(f"| {n}^3 {np.dtype(dtype).name} | {fmt(t_copy)}, {rate(2 * cur.nbytes, t_copy):.2f} TB/s | {fmt(t_int)}, {rate(interior, t_int):.2f} TB/s | "
                     f"{fmt(t_s1)}, {rate(interior, t_s1):.2f} TB/s | {fmt(t_s2)}, {rate(2 * interior, t_s2):.2f} TB/s | "
                     f"{fmt(t_ss)}, {rate(3 * interior, t_ss):.2f} TB/s | {fmt(t_down)} | {fmt(w_s1)} | {fmt(w_s2)} | {fmt(w_ss)} | {ratio:.0f}x |")
        del cur, last, check
lines += ["", "The one condition of this feature: a tracker interrupt through the new path costs less than the download it replaces.  Measured: "
          + ", ".join(f"{n}^3 {name}: the download takes {r:.0f} times as long as the slowest interrupt" for n, name, r in ratios) + "."]
text = "\n".join(lines)
print(text)
if len(sys.argv) > 1:
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text(text + "\n")
