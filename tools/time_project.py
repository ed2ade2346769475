"""Times projections and slices on the device (profiles/project_time.md): ``pdehip_project`` for every axis subset with ``integral`` and
``max``, and ``pdehip_extract_box`` for a mid-plane slice on each axis, at 256^3 and 512^3, fp64 and fp32.  Two yardsticks, measured in
the same process and in turn with the contenders: the full download (``DeviceArray.get_valid``) of the same array, which is what a
projection cost before, against the host wall time of a whole call (result download included); and ``pdehip_field_stats(want_m2=0)`` on
the same array, which reads the same bytes, against the device time between HIP events.  Warm-up, 7 repetitions, median (min .. max).

    python tools/time_project.py [output.md]
"""

from __future__ import annotations

import ctypes as C
import itertools
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "py-pde_amd")]

import pde_hip  # noqa: E402
from pde_hip import _abi  # noqa: E402
from pde_hip.device import DeviceArray, DeviceBuffer  # noqa: E402

REPS, WARM = 7, 2
backend = pde_hip.get_backend("hip")
lib = backend._lib


def alternate(contenders: dict, timer) -> dict:
    """{name: times in ms}: every repetition runs every contender once, in turn."""
    out = {name: [] for name in contenders}
    for i in range(WARM + REPS):
        for name, fn in contenders.items():
            ms = timer(fn)
            if i >= WARM:
                out[name].append(ms)
    return {name: np.array(v) for name, v in out.items()}


_E0, _E1 = C.c_void_p(), C.c_void_p()
lib.event_create(C.byref(_E0)); lib.event_create(C.byref(_E1))


def events(fn) -> float:
    """Milliseconds between two HIP events around ``fn`` (device work only)."""
    lib.event_record(_E0, None)
    fn()
    lib.event_record(_E1, None)
    lib.event_synchronize(_E1)
    ms = C.c_float()
    lib.event_elapsed_ms(_E0, _E1, C.byref(ms))
    return ms.value


def wall(fn) -> float:
    backend.synchronize()
    t0 = time.perf_counter()
    fn()
    backend.synchronize()
    return (time.perf_counter() - t0) * 1e3


def fmt(ms) -> str:
    return f"{np.median(ms):.3f} ms ({ms.min():.3f} .. {ms.max():.3f})"


AXES = "xyz"
lines = [f"# Projections and slices on the device ({backend.device_name})", "",
         f"`python tools/time_project.py`: one process, {WARM} warm-up rounds, {REPS} timed rounds, every round runs every contender once in turn; median",
         "(min .. max).  \"kernel\": device time between HIP events around the C call, next to `pdehip_field_stats(want_m2=0)` on the same array",
         "(it reads the same bytes); \"call\": host wall time of `make_projector()` / `make_slicer()` on the device array, the result's download",
         "included, next to `get_valid()` of the same array (what the projection cost before any host arithmetic)."]
worst = []
rng = np.random.default_rng(0)
for n in (256, 512):
    for dtype in (np.float64, np.float32):
        grid = pde_hip.UnitGrid([n, n, n], periodic=True)
        info = backend.grid_info(grid, dtype)
        cur = DeviceArray(info)
        host = rng.uniform(0.5, 1.5, grid.shape).astype(dtype)
        cur.set_valid(host)
        out = DeviceBuffer(8 * n * n)
        projector, slicer = backend.make_projector(grid), backend.make_slicer(grid)
        subsets = [c for k in (1, 2, 3) for c in itertools.combinations(range(3), k)]
        kernels = {"stats": lambda: lib.field_stats(info.ref, 1, cur.ptr, 0, 0, out.ptr, None)}
        calls = {"download": lambda: cur.get_valid(out=host)}
        chains = {}
        for axes in subsets:
            mask, names = sum(1 << a for a in axes), [AXES[a] for a in axes]
            for method, code in (("integral", _abi.PROJECT_SUM), ("max", _abi.PROJECT_MAX)):
                kernels[(axes, method)] = lambda mask=mask, code=code: lib.project(info.ref, 1, cur.ptr, mask, code, 1.0, out.ptr, None)
                calls[(axes, method)] = lambda names=names, method=method: projector(cur, names, method=method)
            lib.project(info.ref, 1, cur.ptr, mask, _abi.PROJECT_SUM, 1.0, out.ptr, None)
            chains[axes] = lib.last_kernel_name().decode().replace("project_", "").replace("_kernel", "")
        for a in range(3):
            lo, extent = [n // 2 if b == a else 0 for b in range(3)], [1 if b == a else n for b in range(3)]
            kernels[("slice", a)] = lambda lo=lo, extent=extent: lib.extract_box(info.ref, 1, cur.ptr, (C.c_long * 3)(*lo), (C.c_long * 3)(*extent), out.ptr, None)
            calls[("slice", a)] = lambda a=a: slicer(cur, {AXES[a]: "mid"})
        t_k, t_c = alternate(kernels, events), alternate(calls, wall)
        stats, down = np.median(t_k["stats"]), np.median(t_c["download"])
        name = f"{n}^3 {np.dtype(dtype).name}"
        lines += ["", f"## {name}", "", f"`field_stats` kernel: {fmt(t_k['stats'])}, {host.nbytes / stats / 1e9:.2f} TB/s; download `get_valid` (wall): {fmt(t_c['download'])}.", "",
                  "| removed | instances (integral) | kernel integral | x stats | kernel max | x stats | call integral | download / call | call max | download / call |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        for axes in subsets:
            ki, km, ci, cm = t_k[(axes, "integral")], t_k[(axes, "max")], t_c[(axes, "integral")], t_c[(axes, "max")]
            lines.append(f"| {','.join(AXES[a] for a in axes)} | {chains[axes]} | {fmt(ki)} | {np.median(ki) / stats:.2f} | {fmt(km)} | {np.median(km) / stats:.2f} | "
                         f"{fmt(ci)} | {down / np.median(ci):.1f} | {fmt(cm)} | {down / np.median(cm):.1f} |")
            worst += [(down / np.median(ci), name, f"integral over {','.join(AXES[a] for a in axes)}"), (down / np.median(cm), name, f"max over {','.join(AXES[a] for a in axes)}")]
        lines += ["", "| slice at mid | kernel | call | download / call |", "|---|---|---|---|"]
        for a in range(3):
            k, c = t_k[("slice", a)], t_c[("slice", a)]
            lines.append(f"| {AXES[a]} | {fmt(k)} | {fmt(c)} | {down / np.median(c):.1f} |")
            worst.append((down / np.median(c), name, f"slice on {AXES[a]}"))
        del cur, out, projector, slicer, kernels, calls
lines += ["", "The one condition of this feature: at 512^3 fp64 every projection and every slice takes at most a quarter of the download.  Measured, the "
          "smallest ratio download / call per state: " + "; ".join(f"{name}: {min(w for w in worst if w[1] == name)[0]:.1f} ({min(w for w in worst if w[1] == name)[2]})"
                                                                    for name in dict.fromkeys(w[1] for w in worst)) + "."]
text = "\n".join(lines)
print(text)
if len(sys.argv) > 1:
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text(text + "\n")
