"""Times Gaussian smoothing on the device (profiles/smooth_time.md): one ``pdehip_smooth_axis`` pass per axis for sigma = 1, 2 and 4 cells
(radii 4, 8, 16) at 256^3 and 512^3, fp64 and fp32, next to the on-device copy of the same array (``copy_nt_kernel``), device time between
HIP events; and the whole call ``pde_hip.smooth`` on a RESIDENT state - ``device=True``, ``out=state`` (in place) and a host result -
next to the download of the state (``get_valid``), which is what the host path starts with, host wall time.  Everything in one process,
in turn.  Warm-up, 7 repetitions, median (min .. max).

    python tools/time_smooth.py [output.md]
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
from pde_hip.device import DeviceArray  # noqa: E402
from pde_hip.resident import ResidentState  # noqa: E402
from pde_hip.smoothing import gaussian_weights  # noqa: E402

REPS, WARM = 7, 2
SIGMAS = (1.0, 2.0, 4.0)
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
lines = [f"# Gaussian smoothing on the device ({backend.device_name})", "",
         f"`python tools/time_smooth.py`: one process, {WARM} warm-up rounds, {REPS} timed rounds, every round runs every contender once in turn; median",
         "(min .. max).  \"pass\": device time between HIP events around one `pdehip_smooth_axis` call, next to `pdehip_copy_nt` of the same array",
         "(one read and one write of the same bytes); \"call\": host wall time of `pde_hip.smooth` on a resident state (three passes, wrap on every axis),",
         "next to `get_valid()` of the same state - the download the host path starts with, before scipy filters 3 x n^3 cells on one thread."]
condition = []
rng = np.random.default_rng(0)
for n in (256, 512):
    for dtype in (np.float64, np.float32):
        grid = pde_hip.UnitGrid([n, n, n], periodic=True)
        state = pde_hip.ScalarField(grid, rng.uniform(0.5, 1.5, grid.shape).astype(dtype), dtype=dtype)
        info = backend.grid_info(grid, dtype)
        link = ResidentState.attach(state, DeviceArray(info), backend)
        link.push()
        link.device_advanced()
        cur, other = link.dev_state, DeviceArray(info)
        host = np.empty(grid.shape, dtype)
        kernels = {"copy": lambda: lib.copy_nt(other.ptr, cur.ptr, cur.nbytes, None)}
        names = {}
        for sigma in SIGMAS:
            r, w = gaussian_weights(sigma)
            wp = w.ctypes.data_as(C.POINTER(C.c_double))
            for axis in range(3):
                kernels[(sigma, axis)] = lambda axis=axis, r=r, wp=wp, w=w: lib.smooth_axis(info.ref, 1, cur.ptr, other.ptr, axis, _abi.SMOOTH_WRAP, r, wp, None)
                kernels[(sigma, axis)]()
                names[(sigma, axis)] = lib.last_kernel_name().decode()
        calls = {"download": lambda: cur.get_valid(out=host)}
        for sigma in SIGMAS:
            calls[(sigma, "device")] = lambda sigma=sigma: pde_hip.smooth(state, sigma, device=True)
            calls[(sigma, "in place")] = lambda sigma=sigma: pde_hip.smooth(state, sigma, out=state)
            calls[(sigma, "host")] = lambda sigma=sigma: pde_hip.smooth(state, sigma)
        t_k, t_c = alternate(kernels, events), alternate(calls, wall)
        assert link.downloads == 0 and link.uploads == 1 and link.host_stale
        copy, down = np.median(t_k["copy"]), np.median(t_c["download"])
        name = f"{n}^3 {np.dtype(dtype).name}"
        lines += ["", f"## {name}", "", f"`copy_nt` of the array: {fmt(t_k['copy'])}, {2 * host.nbytes / copy / 1e9:.2f} TB/s read + written; download `get_valid` (wall): {fmt(t_c['download'])}.", "",
                  "| sigma (radius) | axis | instance | pass | x copy |", "|---|---|---|---|---|"]
        for sigma in SIGMAS:
            for axis in range(3):
                k = t_k[(sigma, axis)]
                lines.append(f"| {sigma:g} ({gaussian_weights(sigma)[0]}) | {AXES[axis]} | {names[(sigma, axis)]} | {fmt(k)} | {np.median(k) / copy:.2f} |")
        lines += ["", "| sigma | call `device=True` | download / call | call `out=state` | download / call | call, host result | download / call |", "|---|---|---|---|---|---|---|"]
        for sigma in SIGMAS:
            d, i, h = t_c[(sigma, "device")], t_c[(sigma, "in place")], t_c[(sigma, "host")]
            lines.append(f"| {sigma:g} | {fmt(d)} | {down / np.median(d):.1f} | {fmt(i)} | {down / np.median(i):.1f} | {fmt(h)} | {down / np.median(h):.2f} |")
            condition.append((name, sigma, np.median(d), np.median(i), down))
        del cur, other, link, state, kernels, calls
        backend.__dict__.pop("_smooth_buffers", None)
lines += ["", "The condition of this feature: at 512^3 fp64 the in-place call and the `device=True` call cost less than the download alone.  Measured: "
          + "; ".join(f"sigma {s:g}: `device=True` {d:.2f} ms, `out=state` {i:.2f} ms, download {down:.2f} ms" for name, s, d, i, down in condition if name == "512^3 float64") + "."]
text = "\n".join(lines)
print(text)
if len(sys.argv) > 1:
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text(text + "\n")
