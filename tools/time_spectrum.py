"""Times the shell spectrum on the device (profiles/spectrum_time.md): ``pde_hip.field_spectrum`` on a device array at 256^3 and 512^3,
fp64 and fp32, and on 1024 x 4096 (the widest plane the transform takes; 4096 x 4096 goes to the host) - ALTERNATING in one process with
the host path it replaces: the download of the state (``DeviceArray.get_valid``), ``np.fft.rfftn`` in fp64 and the binning.  Next to it,
between HIP events, the two C entry points and a device-to-device copy of the state of the same run, with the bytes each pass moves.
Host wall time is what a tracker interrupt costs end to end.  Warm-up, then repetitions, median and spread (min .. max).

    python tools/time_spectrum.py [output.md]
    python tools/time_spectrum.py --calls-only      (the calls alone, for a kernel trace in a run of its own)
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
from pde_hip.spectrum import axis_frequencies, shell_edges  # noqa: E402

REPS, WARM = 5, 2
HOST_REPS = 2          # (the host path takes seconds)
backend = pde_hip.get_backend("hip")
lib = backend._lib


def events(fn):
    """Milliseconds between two HIP events around ``fn`` (device work, and whatever the entry point waits for in between)."""
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


def once(fn):
    backend.synchronize()
    t0 = time.perf_counter()
    fn()
    backend.synchronize()
    return (time.perf_counter() - t0) * 1e3


def fmt(ms):
    ms = np.asarray(ms)
    return f"{np.median(ms):.3f} ms ({ms.min():.3f} .. {ms.max():.3f})"


if "--calls-only" in sys.argv:
    # for a kernel trace in a run of its own (`rocprofv3 --kernel-trace --stats -- python tools/time_spectrum.py --calls-only`): six calls
    # at 512^3 fp64 with the default shells and as many device-to-device copies of the state
    grid = pde_hip.UnitGrid([512, 512, 512], periodic=True)
    dev = DeviceArray(backend.grid_info(grid, np.float64)).set_valid(np.random.default_rng(0).normal(0.0, 1.0, grid.shape))
    other = DeviceArray(dev.info)
    for _ in range(6):
        assert pde_hip.field_spectrum(dev, backend=backend).on_device
        lib.memcpy_d2d(other.ptr, dev.ptr, dev.nbytes, None)
    backend.synchronize()
    sys.exit(0)

CASES = [((256, 256, 256), np.float64), ((256, 256, 256), np.float32), ((512, 512, 512), np.float64), ((512, 512, 512), np.float32),
         ((1024, 4096), np.float64)]
head = [f"# The shell spectrum on the device ({backend.device_name})", "",
        f"`python tools/time_spectrum.py`: one process.  \"wall\": host wall time of the whole call of `pde_hip.field_spectrum(dev)` with the default",
        f"shells ({WARM} warm-up calls, then {HOST_REPS + REPS} timed ones), uploads of frequencies and edges and downloads of counts and sums included - what a",
        f"tracker interrupt costs; the first {HOST_REPS} timed calls ALTERNATE with the host path it replaces, `DeviceArray.get_valid` + `np.fft.rfftn` in fp64 +",
        "binning (`make_spectrum(grid)(host array)`), measured the same way.  \"device\": between HIP events around the C entry point, median (min .. max)",
        f"of {REPS}; `pdehip_shell_spectrum` waits for its stream twice inside (edges, limbs), which the events include.  The copy is `hipMemcpyAsync`",
        "device to device of the state's allocation in the same run; \"bytes\" are what the passes must move at the least (the row pass reads the",
        "state and writes the half spectrum, each line pass reads and writes it, each shell sweep reads it), \"rate\" is bytes / device time.", ""]
rows = ["| state | shells | field_spectrum, wall | host path, wall | host / device | fft_forward, device | shell_spectrum, device | bytes (forward / shells) |"
        " rate (forward / shells) | copy, device | copy rate |", "|---|---|---|---|---|---|---|---|---|---|---|"]
ratios = []
rng = np.random.default_rng(0)
for shape, dtype in CASES:
    name = f"{'x'.join(map(str, shape))} {np.dtype(dtype).name}"
    print(f"timing {name}", file=sys.stderr, flush=True)
    grid = pde_hip.UnitGrid(list(shape), periodic=True)
    info = backend.grid_info(grid, dtype)
    dev = DeviceArray(info)
    host = rng.normal(0.0, 1.0, shape).astype(dtype)
    dev.set_valid(host)
    host_path = backend.make_spectrum(grid)
    for _ in range(WARM):
        got = pde_hip.field_spectrum(dev, backend=backend)
    assert got.on_device
    t_dev, t_host = [], []
    for _ in range(HOST_REPS):
        t_dev.append(once(lambda: pde_hip.field_spectrum(dev, backend=backend)))
        t_host.append(once(lambda: host_path(dev.get_valid(out=host))))
    for _ in range(REPS):
        t_dev.append(once(lambda: pde_hip.field_spectrum(dev, backend=backend)))
    expect = host_path(host)
    assert (got.counts == expect.counts).all() and np.abs(got.power - expect.power).sum() <= 1e-10 * expect.power.sum()
    # the entry points alone
    cells = int(np.prod(shape))
    half = cells // shape[-1] * (shape[-1] // 2 + 1)
    spec = DeviceBuffer(16 * half)
    t_fwd = events(lambda: lib.fft_forward(info.ref, 1, dev.ptr, spec.ptr, None))
    edges = shell_edges(None, shape, info.dx)[0]
    kf = np.concatenate(axis_frequencies(shape, info.dx))
    ns = edges.size + 1
    bufs = [DeviceBuffer(kf.nbytes), DeviceBuffer(edges.nbytes), DeviceBuffer(8 * ns), DeviceBuffer(8 * ns)]
    lib.memcpy_h2d(bufs[0].ptr, kf.ctypes.data, kf.nbytes, None)
    lib.memcpy_h2d(bufs[1].ptr, edges.ctypes.data, edges.nbytes, None)
    t_shell = events(lambda: lib.shell_spectrum(info.ref, 1, dev.ptr, bufs[0].ptr, ns - 2, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, None))
    other = DeviceArray(info)
    t_copy = events(lambda: lib.memcpy_d2d(other.ptr, dev.ptr, dev.nbytes, None))
    lines = sum(n > 1 for n in shape[:-1])
    b_fwd = cells * dev.itemsize + 16 * half + lines * 32 * half
    b_shell = b_fwd + 2 * 16 * half
    rate = lambda b, ms: b / (np.median(ms) * 1e-3) / 1e12          # noqa: E731
    ratio = np.median(t_host) / np.median(t_dev)
    ratios.append((name, ratio, np.median(t_dev), np.median(t_host)))
    rows.append(f"| {name} | {ns - 2} | {fmt(t_dev)} | {fmt(t_host)} | {ratio:.0f}x | {fmt(t_fwd)} | {fmt(t_shell)} | {b_fwd / 1e9:.2f} GB / {b_shell / 1e9:.2f} GB |"
                f" {rate(b_fwd, t_fwd):.2f} TB/s / {rate(b_shell, t_shell):.2f} TB/s | {fmt(t_copy)} | {rate(2 * dev.nbytes, t_copy):.2f} TB/s |")
    del dev, other, spec, host
# what the transform does not take
grid = pde_hip.UnitGrid([4096, 4096], periodic=True)
dev = DeviceArray(backend.grid_info(grid, np.float64)).set_valid(rng.normal(0.0, 1.0, (4096, 4096)))
t_refused = [once(lambda: pde_hip.field_spectrum(dev, 256, backend=backend)) for _ in range(2)]
assert not pde_hip.field_spectrum(dev, 256, backend=backend).on_device
tail = ["", "The one condition of this feature: every device call costs less host wall time than the host path it replaces.  Measured: "
        + ", ".join(f"{name}: {d:.1f} ms against {h:.0f} ms ({r:.0f} times)" for name, r, d, h in ratios) + ".",
        "", f"4096 x 4096 fp64 (an extent beyond 1024 on a slower axis) is refused by the dry run and takes the host path: {fmt(t_refused)} with 256 bins.",
        "", "Not measured here: hipFFT's D2Z transform of the dense array as a yardstick, and counters per pass."]
text = "\n".join(head + rows + tail)
print(text)
if len(sys.argv) > 1:
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text(text + "\n")
