"""Times interpolation on the device (profiles/interp_time.md): probes of a resident fp64 field against the full download the host
route needs, and regridding 256^3 -> 512^3 against an on-device copy of the target's bytes.  HIP events, warm-up, 7 repetitions,
median and spread (min .. max) reported.

    python tools/time_interp.py [output.md]
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
from pde_hip.interpolation import _Source  # noqa: E402

REPS, WARM = 7, 2
backend = pde_hip.get_backend("hip")
lib = backend._lib
lines = [f"# Interpolation on the device ({backend.device_name})", "",
         f"`python tools/time_interp.py`: {WARM} warm-up runs, {REPS} timed repetitions, median (min .. max).", ""]


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


rng = np.random.default_rng(0)
lines += ["## Probes of a resident fp64 field", "",
          "| field | points | kernel (events) | interpolator call, host wall time (upload of the points, kernel, download of the values and the counter) | full download `DeviceArray.get_valid` (wall) |",
          "|---|---|---|---|---|"]
for n in (256, 512):
    grid = pde_hip.UnitGrid([n, n, n], periodic=[True, False, True])
    info = backend.grid_info(grid, np.float64)
    dev = DeviceArray(info)
    host = rng.uniform(0, 1, grid.shape)
    dev.set_valid(host)
    field = pde_hip.ScalarField(grid, "zeros")
    interp = backend.make_interpolator(field)
    src = _Source(grid)
    down = wall(lambda: dev.get_valid(out=host))
    for npts in (10**3, 10**6):
        pts = rng.uniform(0, n, (npts, 3))
        p_dev, o_dev, cnt = DeviceBuffer(pts.nbytes), DeviceBuffer(8 * npts), DeviceBuffer(8)
        lib.memcpy_h2d(p_dev.ptr, pts.ctypes.data, pts.nbytes, None)
        lib.memset(cnt.ptr, 0, 8, None)
        kern = events(lambda: lib.interpolate_points(info.ref, 1, src.periodic, src.lo, 0, dev.ptr, p_dev.ptr, npts, None, o_dev.ptr, cnt.ptr, None))
        call = wall(lambda: interp(pts, dev))
        lines.append(f"| {n}^3 | {npts} | {fmt(kern)} | {fmt(call)} | {fmt(down)} |")
    del dev

lines += ["", "## Regridding 256^3 -> 512^3, fp64", ""]
src_grid = pde_hip.UnitGrid([256] * 3, periodic=[True, False, True])
dst_grid = pde_hip.CartesianGrid([(0, 256)] * 3, [512] * 3, periodic=[True, False, True])
si, di = backend.grid_info(src_grid, np.float64), backend.grid_info(dst_grid, np.float64)
a, b, c = DeviceArray(si), DeviceArray(di), DeviceArray(di)
a.set_valid(rng.uniform(0, 1, src_grid.shape))
lib.memset(b.ptr, 0, b.nbytes, None); lib.memset(c.ptr, 0, c.nbytes, None)
coords = np.ascontiguousarray(np.concatenate(dst_grid.axes_coords))
c_dev, tables, cnt = DeviceBuffer(coords.nbytes), DeviceBuffer(40 * coords.size), DeviceBuffer(8)
lib.memcpy_h2d(c_dev.ptr, coords.ctypes.data, coords.nbytes, None)
lib.memset(cnt.ptr, 0, 8, None)
src = _Source(src_grid)
regrid = events(lambda: lib.interpolate_to_grid(si.ref, 1, src.periodic, src.lo, 0, a.ptr, di.ref, c_dev.ptr, None, b.ptr, tables.ptr, cnt.ptr, None))
copy = events(lambda: lib.memcpy_d2d(c.ptr, b.ptr, b.nbytes, None))
valid_bytes = 512**3 * 8
rate_r, rate_c = valid_bytes / np.median(regrid) / 1e9, b.nbytes / np.median(copy) / 1e9
lines += [f"* table kernel + row kernel: {fmt(regrid)} for {valid_bytes / 2**30:.2f} GiB of target cells = {rate_r:.2f} TB/s written",
          f"* on-device copy of the target array ({b.nbytes / 2**30:.2f} GiB, `hipMemcpyAsync` device to device): {fmt(copy)} = {rate_c:.2f} TB/s written",
          f"* fraction of the copy's rate: {rate_r / rate_c:.2f}", ""]
text = "\n".join(lines)
print(text)
if len(sys.argv) > 1:
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text(text + "\n")
