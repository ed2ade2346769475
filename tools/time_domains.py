"""Times the labelling of domains on the device (profiles/domains_time.md): ``pde_hip.field_domains`` with sizes on a resident fp64 and
fp32 field at 256^3 and 512^3, periodic, face connectivity, for two kinds of field - a Gaussian-smoothed random field thresholded at 0
(coarsened, Cahn-Hilliard-like: few large domains) and white noise with 30 % foreground (about 10^6 domains at 256^3, 7.7 x 10^6 at
512^3) - next to the host path it replaces, measured in the same process: the download (``DeviceArray.get_valid``), ``scipy.ndimage.label`` plus the merge across the
periodic faces, and ``np.bincount``.  Yardsticks in the same process: an on-device copy of the field and ``pdehip_field_stats``.  HIP events
for the device work of the two C entry points, host wall time for what a tracker interrupt costs end to end.

    python tools/time_domains.py [output.md]
    python tools/time_domains.py --calls-only      # two calls per state and kind and nothing else: the run a kernel trace is taken of
    python tools/time_domains.py --reduce-trace kernel_trace.csv [output.md]

The last form needs no GPU: it reduces the kernel trace of a ``--calls-only`` run (``rocprofv3 --kernel-trace --output-format csv``, a run
of its own) to the device time of every kernel in the SECOND call of each state and kind, and appends that table to ``output.md``.
"""

from __future__ import annotations

import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np
from scipy import ndimage

ROOT = Path(__file__).resolve().parent.parent
STATES = [(n, dtype) for n in (256, 512) for dtype in (np.float64, np.float32)]
KINDS = ("smoothed", "white noise, 30 %")
OWN_KERNELS = r"(label_\w+_kernel|domain_sizes_kernel)"


def reduce_trace(trace: str, output: str | None) -> None:
    """Dispatches of the unit's kernels in time order: 2 calls x 7 kernels per state and kind, in the order of the loops below."""
    import csv
    import re

    with open(trace, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    own = [(re.search(OWN_KERNELS, r["Kernel_Name"]).group(1), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
           for r in rows if re.search(OWN_KERNELS, r["Kernel_Name"])]
    names = [f"{n}^3 {np.dtype(dtype).name}, {kind}" for n, dtype in STATES for kind in KINDS]
    assert len(own) == 14 * len(names), f"{len(own)} dispatches, expected {14 * len(names)}"
    text = ["", "## Device time per kernel", "",
            "`rocprofv3 --kernel-trace --output-format csv -- python tools/time_domains.py --calls-only` in a run of its own, reduced by",
            "`python tools/time_domains.py --reduce-trace <kernel_trace.csv>`: two calls per state and kind, the kernels of the second one.", "",
            "| state, field | " + " | ".join(k for k, _ in own[7:14]) + " | largest |", "|---|" + "---|" * 8]
    for c, name in enumerate(names):
        part = own[14 * c + 7: 14 * c + 14]
        assert [k for k, _ in part] == [k for k, _ in own[7:14]]
        text.append(f"| {name} | " + " | ".join(f"{ms:.3f} ms" for _, ms in part) + f" | {max(part, key=lambda kv: kv[1])[0]} |")
    print("\n".join(text))
    if output:
        with open(output, "a") as fh:
            fh.write("\n".join(text) + "\n")


if "--reduce-trace" in sys.argv:
    at = sys.argv.index("--reduce-trace")
    reduce_trace(sys.argv[at + 1], sys.argv[at + 2] if len(sys.argv) > at + 2 else None)
    sys.exit(0)
sys.path[:0] = [str(ROOT / "py-pde_amd")]

import pde_hip  # noqa: E402
from pde_hip.device import DeviceArray, DeviceBuffer, ptr_array  # noqa: E402
from pde_hip.domains import host_domains  # noqa: E402

REPS, WARM = 5, 2
CALLS_ONLY = "--calls-only" in sys.argv
OUTPUT = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
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


def wall(fn, reps=REPS, warm=WARM):
    out = []
    for i in range(warm + reps):
        backend.synchronize()
        t0 = time.perf_counter()
        fn()
        backend.synchronize()
        if i >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return np.array(out)


def fmt(ms):
    return f"{np.median(ms):.3f} ms ({ms.min():.3f} .. {ms.max():.3f})"


def fields(rng, shape, dtype):
    """name -> (host data, threshold)"""
    noise = rng.standard_normal(shape, dtype=np.float32)
    yield "smoothed", ndimage.gaussian_filter(noise, 4.0, mode="wrap").astype(dtype), 0.0
    yield "white noise, 30 %", rng.random(shape, dtype=np.float32).astype(dtype), 0.7


head = [f"# Domains on the device ({backend.device_name})", "",
        f"`python tools/time_domains.py`: one process, {WARM} warm-up runs, {REPS} timed repetitions, median (min .. max); the host path once after one",
        "warm-up (it takes seconds).  Periodic grids, face connectivity.  \"device\": between HIP events around `pdehip_label_domains` and around",
        "`pdehip_domain_sizes` (which waits for its stream).  \"wall\": host wall time of the whole `pde_hip.field_domains(dev, t)` with the sizes -",
        "what a tracker interrupt costs.  Host path: `DeviceArray.get_valid`, `scipy.ndimage.label` plus the merge across the periodic faces",
        "(`pde_hip.domains.host_domains`), `np.bincount`.  Yardsticks: an on-device copy of the field (`pdehip_lincomb`) and `pdehip_field_stats`",
        "without the variance, between HIP events.", ""]
rows = ["| state | field | K | label, device | sizes, device | field_domains, wall | download | label + merge, host | bincount, host | host path / wall |"
        " label device / copy | label device / stats |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
ratios = []
rng = np.random.default_rng(0)
for n, dtype in STATES:
    name = f"{n}^3 {np.dtype(dtype).name}"
    grid = pde_hip.UnitGrid([n, n, n], periodic=True)
    info = backend.grid_info(grid, dtype)
    dev, copy = DeviceArray(info), DeviceArray(info)
    label = backend.make_domain_labeller(grid)
    cells = n ** 3
    labels_dev, info_dev, stats_out = DeviceBuffer(4 * cells), DeviceBuffer(16), DeviceBuffer(64)
    per = (C.c_int * 3)(1, 1, 1)
    one, table = (C.c_double * 1)(1.0), ptr_array([dev])
    for kind, host, threshold in fields(rng, grid.shape, dtype):
        print(f"timing {name}, {kind}", file=sys.stderr, flush=True)
        dev.set_valid(host)
        if CALLS_ONLY:
            for _ in range(2):
                res = label(dev, threshold)
            print(f"{name}, {kind}: {res}", flush=True)
            continue
        lo = float(np.nextafter(dtype(threshold), dtype(np.inf)))
        t_label = events(lambda: lib.label_domains(info.ref, dev.ptr, C.c_double(lo), C.c_double(np.inf), 1, per, labels_dev.ptr, info_dev.ptr, None))
        res = label(dev, threshold)
        sizes_dev = DeviceBuffer(8 * max(res.count, 1))
        t_sizes = events(lambda: lib.domain_sizes(labels_dev.ptr, cells, res.count, sizes_dev.ptr, None))
        t_wall = wall(lambda: label(dev, threshold).sizes)
        t_copy = events(lambda: lib.lincomb(info.ref, 1, copy.ptr, None, 1, one, table, None))
        t_stats = events(lambda: lib.field_stats(info.ref, 1, dev.ptr, 0, 0, stats_out.ptr, None))
        t_down = wall(lambda: dev.get_valid(out=host))
        kept = {}

        def host_label():
            kept["labels"], kept["count"] = host_domains(host > threshold, (True, True, True), 1)

        t_host = wall(host_label, reps=1, warm=1 if n == 256 else 0)
        t_bin = wall(lambda: np.bincount(kept["labels"].ravel()), reps=1, warm=1 if n == 256 else 0)
        assert kept["count"] == res.count, (kept["count"], res.count)
        assert np.array_equal(np.bincount(kept["labels"].ravel(), minlength=res.count + 1)[1:], res.sizes)
        host_path = np.median(t_down) + np.median(t_host) + np.median(t_bin)
        ratio = host_path / np.median(t_wall)
        ratios.append((name, kind, ratio, np.median(t_label) / np.median(t_copy), np.median(t_label) / np.median(t_stats)))
        rows.append(f"| {name} | {kind} | {res.count} | {fmt(t_label)} | {fmt(t_sizes)} | {fmt(t_wall)} | {fmt(t_down)} | {fmt(t_host)} | {fmt(t_bin)} | "
                    f"{ratio:.0f}x | {ratios[-1][3]:.1f} | {ratios[-1][4]:.1f} |")
        del host, kept
    del dev, copy, labels_dev
if not CALLS_ONLY:
    met = all(r[2] > 1.0 for r in ratios)
    tail = ["", "The one condition of this feature: every call costs less host wall time than the host path it replaces, at both sizes and for both kinds "
            f"of field.  {'Met' if met else 'NOT met'}: the host path takes between {min(r[2] for r in ratios):.0f} and {max(r[2] for r in ratios):.0f} times as long.",
            "", f"No rate is promised.  `pdehip_label_domains` takes {min(r[3] for r in ratios):.1f} to {max(r[3] for r in ratios):.1f} times the on-device copy of "
            f"the field and {min(r[4] for r in ratios):.1f} to {max(r[4] for r in ratios):.1f} times the statistics call, device time against device time."]
    text = "\n".join(head + rows + tail)
    print(text)
    if OUTPUT:
        Path(OUTPUT).parent.mkdir(parents=True, exist_ok=True)
        Path(OUTPUT).write_text(text + "\n")
