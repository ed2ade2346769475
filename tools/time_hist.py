"""Times histograms and quantiles on the device (profiles/hist_time.md): ``pde_hip.field_histogram`` with 64 and 4096 bins on a
uniform-random field, a two-valued field plus noise (the Cahn-Hilliard case) and an all-equal field (worst contention), and
``pde_hip.field_quantile`` for one and for five quantiles, at 256^3 and 512^3, fp64 and fp32 - next to the two yardsticks measured in the
same process: the full download of the state (``DeviceArray.get_valid``), which every call replaces, and ``pdehip_field_stats`` without the
variance, which reads the same bytes.  HIP events for the device work of the C entry points, host wall time for what a tracker interrupt
costs end to end.  One process: warm-up, 7 repetitions, median and spread (min .. max).

    python tools/time_hist.py [output.md]
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
RANGE = (-1.0, 1.0)
FIVE = [0.01, 0.25, 0.5, 0.75, 0.99]
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


def fields(rng, shape, dtype):
    """name -> host data in [-1, 1]"""
    yield "uniform", rng.uniform(-1.0, 1.0, shape).astype(dtype)
    yield "two-valued + noise", (0.9 * rng.choice([-1.0, 1.0], shape) + rng.normal(0.0, 0.01, shape)).astype(dtype)
    yield "all equal", np.full(shape, 0.3, dtype=dtype)


head = [f"# Histograms and quantiles on the device ({backend.device_name})", "",
        f"`python tools/time_hist.py`: one process, {WARM} warm-up runs, {REPS} timed repetitions, median (min .. max).  \"device\": between HIP events",
        "around the C entry point (`pdehip_histogram` reads its edges back before it launches, which the events include).  \"wall\": host wall time of",
        "the whole call of `pde_hip.field_histogram(dev, bins, (-1, 1))` / `pde_hip.field_quantile(dev, q)`, uploads of edges and downloads of results",
        "included - what a tracker interrupt costs.  Yardsticks per state: the download `DeviceArray.get_valid` (wall) that every call replaces, and",
        "`pdehip_field_stats` without the variance (device and wall), which reads the same bytes once.", ""]
hist_rows = ["| state | field | 64 bins, device | 64 bins, wall | 4096 bins, device | 4096 bins, wall | 64 bins device / stats device |", "|---|---|---|---|---|---|---|"]
sel_rows = ["| state | download (wall) | field_stats (device) | field_stats (wall) | 1 quantile, uniform (wall) | 5 quantiles, uniform (wall) | 1 quantile, all equal (wall) |"
            " 64 bins with range=None, uniform (wall) | download / slowest call |", "|---|---|---|---|---|---|---|---|---|"]
ratios, aims = [], []
rng = np.random.default_rng(0)
stats = backend.make_statistics()
for n in (256, 512):
    for dtype in (np.float64, np.float32):
        name = f"{n}^3 {np.dtype(dtype).name}"
        grid = pde_hip.UnitGrid([n, n, n], periodic=True)
        info = backend.grid_info(grid, dtype)
        dev = DeviceArray(info)
        out = DeviceBuffer(64)
        edges = {b: np.linspace(*RANGE, b + 1, dtype=dtype).astype(np.float64) for b in (64, 4096)}
        bufs = {}
        for b, e in edges.items():
            bufs[b] = (DeviceBuffer(e.nbytes), DeviceBuffer(8 * (b + 3)))
            lib.memcpy_h2d(bufs[b][0].ptr, e.ctypes.data, e.nbytes, None)
        slowest, t_down, t_stats = 0.0, None, None
        sel = {}
        for kind, host in fields(rng, grid.shape, dtype):
            print(f"timing {name}, {kind}", file=sys.stderr, flush=True)
            dev.set_valid(host)
            if t_down is None:
                t_down = wall(lambda: dev.get_valid(out=host))
                t_stats = events(lambda: lib.field_stats(info.ref, 1, dev.ptr, 0, 0, out.ptr, None))
                w_stats = wall(lambda: stats(dev))
            cells = []
            for b in (64, 4096):
                t_dev = events(lambda b=b: lib.histogram(info.ref, 1, dev.ptr, 0, b, bufs[b][0].ptr, bufs[b][1].ptr, None))
                t_wall = wall(lambda b=b: pde_hip.field_histogram(dev, b, RANGE, backend=backend))
                slowest = max(slowest, np.median(t_wall))
                cells += [fmt(t_dev), fmt(t_wall)]
                if b == 64:
                    aim = np.median(t_dev) / np.median(t_stats)
                    aims.append((name, kind, aim))
            hist_rows.append(f"| {name} | {kind} | " + " | ".join(cells) + f" | {aim:.2f} |")
            if kind == "uniform":
                sel["q1"] = wall(lambda: pde_hip.field_quantile(dev, 0.5, backend=backend))
                sel["q5"] = wall(lambda: pde_hip.field_quantile(dev, FIVE, backend=backend))
                sel["auto"] = wall(lambda: pde_hip.field_histogram(dev, 64, backend=backend))
            if kind == "all equal":
                sel["q1eq"] = wall(lambda: pde_hip.field_quantile(dev, 0.5, backend=backend))
            del host
        slowest = max([slowest] + [np.median(v) for v in sel.values()])
        ratio = np.median(t_down) / slowest
        ratios.append((name, ratio))
        sel_rows.append(f"| {name} | {fmt(t_down)} | {fmt(t_stats)} | {fmt(w_stats)} | {fmt(sel['q1'])} | {fmt(sel['q5'])} | {fmt(sel['q1eq'])} | "
                        f"{fmt(sel['auto'])} | {ratio:.1f}x |")
        del dev, bufs
worst = max(aims, key=lambda a: a[2])
tail = ["", "The one condition of this feature: every call costs less host wall time than the download it replaces.  Measured: "
        + ", ".join(f"{name}: the download takes {r:.1f} times as long as the slowest call" for name, r in ratios) + ".",
        "", f"The aim (not a gate): a 64-bin histogram within 1.5 x the statistics call that reads the same bytes, device time against device time.  "
        f"Measured: between {min(a[2] for a in aims):.2f} x and {worst[2]:.2f} x (the largest: {worst[0]}, {worst[1]})."]
text = "\n".join(head + hist_rows + [""] + sel_rows + tail)
print(text)
if len(sys.argv) > 1:
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text(text + "\n")
