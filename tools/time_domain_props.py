"""Times the per-domain properties on the device (profiles/domain_props_time.md): ``pde_hip.field_domains(dev, t, properties=True)`` on a
resident fp64 and fp32 field at 256^3 and 512^3, periodic, face connectivity, for the two kinds of field of ``tools/time_domains.py`` - a
Gaussian-smoothed random field thresholded at 0 (few large domains) and white noise with 30 % foreground (millions of one-cell domains) -
next to the host path it replaces, measured in the same process: the download, ``scipy.ndimage.label`` plus the merge across the periodic
faces, ``center_of_mass``, ``find_objects`` and ``sum_labels`` (scipy's open-grid answers: the periodic frame would come on top).
Yardsticks in the same process: ``pdehip_domain_sizes`` (the same label traffic) and an on-device copy of the field.

    python tools/time_domain_props.py [output.md]
    python tools/time_domain_props.py --no-host [output.md]   # without the host path (it takes minutes at 512^3)
    python tools/time_domain_props.py --calls-only            # two bare calls per state and kind: the run a kernel trace is taken of
    python tools/time_domain_props.py --reduce-trace kernel_trace.csv [output.md]
    python tools/time_domain_props.py --against other/libpdehip.so [output.md]

``--reduce-trace`` needs no GPU: it reduces the kernel trace of a ``--calls-only`` run (``rocprofv3 --kernel-trace --output-format csv``, a
run of its own) to the device time of the three launches in the SECOND call of each state and kind.  ``--against``: ``field_domains``
WITHOUT ``properties`` through this library and through another build (the parent commit's), alternating in one process.
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
OWN_KERNELS = r"(props_\w+_kernel)"


def reduce_trace(trace: str, output: str | None) -> None:
    """Dispatches of the unit's kernels in time order: 2 calls x 3 kernels per state and kind, in the order of the loops below."""
    import csv
    import re

    with open(trace, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    own = [(re.search(OWN_KERNELS, r["Kernel_Name"]).group(1), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
           for r in rows if re.search(OWN_KERNELS, r["Kernel_Name"])]
    names = [f"{n}^3 {np.dtype(dtype).name}, {kind}" for n, dtype in STATES for kind in KINDS]
    assert len(own) == 6 * len(names), f"{len(own)} dispatches, expected {6 * len(names)}"
    text = ["", "## Device time per launch", "",
            "`rocprofv3 --kernel-trace --output-format csv -- python tools/time_domain_props.py --calls-only` in a run of its own, reduced by",
            "`python tools/time_domain_props.py --reduce-trace <kernel_trace.csv>`: two calls per state and kind, the launches of the second one.", "",
            "| state, field | " + " | ".join(k for k, _ in own[3:6]) + " | largest |", "|---|" + "---|" * 4]
    for c, name in enumerate(names):
        part = own[6 * c + 3: 6 * c + 6]
        assert [k for k, _ in part] == [k for k, _ in own[3:6]]
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
from pde_hip import _lib as libmod  # noqa: E402
from pde_hip.device import DeviceArray, DeviceBuffer, ptr_array  # noqa: E402
from pde_hip.domains import host_domains  # noqa: E402

REPS, WARM = 5, 2
CALLS_ONLY = "--calls-only" in sys.argv
NO_HOST = "--no-host" in sys.argv
AGAINST = sys.argv[sys.argv.index("--against") + 1] if "--against" in sys.argv else None
OUTPUT = next((a for a in sys.argv[1:] if not a.startswith("--") and a != AGAINST), None)
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
    """name -> (host data, threshold): those of tools/time_domains.py"""
    noise = rng.standard_normal(shape, dtype=np.float32)
    yield "smoothed", ndimage.gaussian_filter(noise, 4.0, mode="wrap").astype(dtype), 0.0
    yield "white noise, 30 %", rng.random(shape, dtype=np.float32).astype(dtype), 0.7


def write(text: str) -> None:
    print(text)
    if OUTPUT:
        Path(OUTPUT).parent.mkdir(parents=True, exist_ok=True)
        with open(OUTPUT, "a" if AGAINST else "w") as fh:
            fh.write(text + "\n")


def against(path: str) -> None:
    """``field_domains`` without ``properties`` through two builds of the library, A B A B ... in one process."""
    other = libmod._Lib(Path(path).resolve())
    assert not other.has("domain_properties") and lib.has("domain_properties")
    rows = ["", "## `field_domains` without `properties`: this library against the parent commit's", "",
            f"`python tools/time_domain_props.py --against <parent's libpdehip.so>`: host wall time of `label(dev, t).sizes`, {REPS * 2} calls per",
            "library after 2 warm-up calls each, alternating A B A B in one process; median (min .. max).  None of its code changes.", "",
            "| state | field | this library | parent's library | ratio |", "|---|---|---|---|---|"]
    rng = np.random.default_rng(0)
    for n, dtype in STATES:
        grid = pde_hip.UnitGrid([n, n, n], periodic=True)
        dev = DeviceArray(backend.grid_info(grid, dtype))
        label = backend.make_domain_labeller(grid)
        for kind, host, threshold in fields(rng, grid.shape, dtype):
            print(f"timing {n}^3 {np.dtype(dtype).name}, {kind}", file=sys.stderr, flush=True)
            dev.set_valid(host)
            times = {id(lib): [], id(other): []}
            for i in range(2 * (2 + 2 * REPS)):
                which = (lib, other)[i % 2]
                libmod._LIB = which          # (what `backend._lib` returns)
                try:
                    assert backend._lib is which
                    t = wall(lambda: label(dev, threshold).sizes, reps=1, warm=0)
                finally:
                    libmod._LIB = lib
                if i >= 4:
                    times[id(which)].append(t[0])
            a, b = np.array(times[id(lib)]), np.array(times[id(other)])
            rows.append(f"| {n}^3 {np.dtype(dtype).name} | {kind} | {fmt(a)} | {fmt(b)} | {np.median(a) / np.median(b):.3f} |")
        del dev
    write("\n".join(rows))


if AGAINST:
    against(AGAINST)
    sys.exit(0)

head = [f"# Domain properties on the device ({backend.device_name})", "",
        f"`python tools/time_domain_props.py`: one process, {WARM} warm-up runs, {REPS} timed repetitions, median (min .. max); every part of the host",
        "path once (it takes seconds to minutes).  Periodic grids, face connectivity.  \"device\": between HIP events around `pdehip_domain_properties`",
        "(three launches; it waits for its stream) and around `pdehip_domain_sizes` (one launch over the same labels; it waits too).  \"wall\": host",
        "wall time of the whole `pde_hip.field_domains(dev, t, properties=True)` - labelling, sizes, statistics for `absmax`, properties, 72 bytes",
        "per domain down, derivation - and of the same call without `properties`.  Host path: `DeviceArray.get_valid`, `scipy.ndimage.label` plus",
        "the merge across the periodic faces (`pde_hip.domains.host_domains`), `center_of_mass`, `find_objects`, `sum_labels` (scipy's open-grid",
        "answers; the periodic frame would come on top).  Yardstick: an on-device copy of the field (`pdehip_lincomb`).", ""]
rows = ["| state | field | K | properties, device | sizes, device | properties / sizes | copy, device | properties=True, wall | without, wall |"
        " download | label + merge, host | center_of_mass | find_objects | sum_labels | host path / wall |", "|---|" + "---|" * 14]
ratios = []
rng = np.random.default_rng(0)
for n, dtype in STATES:
    name = f"{n}^3 {np.dtype(dtype).name}"
    grid = pde_hip.UnitGrid([n, n, n], periodic=True)
    info = backend.grid_info(grid, dtype)
    dev, copy = DeviceArray(info), DeviceArray(info)
    label = backend.make_domain_labeller(grid)
    cells = n ** 3
    per = (C.c_int * 3)(1, 1, 1)
    one, table = (C.c_double * 1)(1.0), ptr_array([dev])
    for kind, host, threshold in fields(rng, grid.shape, dtype):
        print(f"timing {name}, {kind}", file=sys.stderr, flush=True)
        dev.set_valid(host)
        res = label(dev, threshold)
        k = res.count
        absmax = float(np.abs(host).max())
        bufs = [DeviceBuffer(b * max(k, 1)) for b in (4, 24, 24, 16, 4)]
        sizes_dev = DeviceBuffer(8 * max(k, 1))

        def props():
            lib.domain_properties(info.ref, dev.ptr, res.labels_device.ptr, k, per, C.c_double(absmax), *(b.ptr for b in bufs), None)

        if CALLS_ONLY:
            for _ in range(2):
                props()
            print(f"{name}, {kind}: {res}", flush=True)
            continue
        t_props = events(props)
        t_sizes = events(lambda: lib.domain_sizes(res.labels_device.ptr, cells, k, sizes_dev.ptr, None))
        t_copy = events(lambda: lib.lincomb(info.ref, 1, copy.ptr, None, 1, one, table, None))
        t_wall = wall(lambda: label(dev, threshold, properties=True).sums)
        t_plain = wall(lambda: label(dev, threshold).sizes)
        line = (f"| {name} | {kind} | {k} | {fmt(t_props)} | {fmt(t_sizes)} | {np.median(t_props) / np.median(t_sizes):.1f} | {fmt(t_copy)} | "
                f"{fmt(t_wall)} | {fmt(t_plain)} |")
        ratio_sizes = np.median(t_props) / np.median(t_sizes)
        if NO_HOST:
            rows.append(line + " - | - | - | - | - | - |")
            ratios.append((name, kind, None, ratio_sizes))
            continue
        t_down = wall(lambda: dev.get_valid(out=host), reps=1, warm=1)
        kept = {}

        def host_label():
            kept["labels"], kept["count"] = host_domains(host > threshold, (True, True, True), 1)

        t_host = wall(host_label, reps=1, warm=0)
        print("  host: labelled", file=sys.stderr, flush=True)
        index = np.arange(1, kept["count"] + 1)
        t_com = wall(lambda: ndimage.center_of_mass(kept["labels"] > 0, kept["labels"], index), reps=1, warm=0)
        print("  host: center_of_mass", file=sys.stderr, flush=True)
        t_obj = wall(lambda: ndimage.find_objects(kept["labels"]), reps=1, warm=0)
        print("  host: find_objects", file=sys.stderr, flush=True)
        t_sum = wall(lambda: ndimage.sum_labels(host, kept["labels"], index), reps=1, warm=0)
        assert kept["count"] == k, (kept["count"], k)
        host_path = sum(float(np.median(t)) for t in (t_down, t_host, t_com, t_obj, t_sum))
        ratio = host_path / np.median(t_wall)
        ratios.append((name, kind, ratio, ratio_sizes))
        rows.append(line + f" {fmt(t_down)} | {fmt(t_host)} | {fmt(t_com)} | {fmt(t_obj)} | {fmt(t_sum)} | {ratio:.0f}x |")
        del host, kept
    del dev, copy
if not CALLS_ONLY:
    tail = ["", f"No rate is promised.  `pdehip_domain_properties` takes {min(r[3] for r in ratios):.1f} to {max(r[3] for r in ratios):.1f} times "
            "`pdehip_domain_sizes` over the same labels, device time against device time."]
    if not NO_HOST:
        met = all(r[2] > 1.0 for r in ratios)
        tail += ["", "The one condition of this feature: every `properties=True` call costs less host wall time than the host path it replaces, at both "
                 f"sizes and for both kinds of field.  {'Met' if met else 'NOT met'}: the host path takes between {min(r[2] for r in ratios):.0f} and "
                 f"{max(r[2] for r in ratios):.0f} times as long."]
    write("\n".join(head + rows + tail))
