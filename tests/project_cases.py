"""Cases, numpy restatements and bounds for the projection entry points ``pdehip_project`` and ``pdehip_extract_box``.

Shared by ``tests/test_project_cpu.py`` (CPU: the C versions of the tests-only shim) and ``tests/test_hip_project.py`` (GPU: the kernels
of ``csrc/pdehip_project.hip``).  The restatements are written from the semantics in ``include/pdehip.h``; the drivers below call the
entry points through whatever library ``pde_hip._lib`` holds, so the same checks serve both.

Inputs (``stats_cases.draw``): values from [0.5, 0.6] u [1.4, 1.5], so a lost or doubled cell moves a sum by at least 0.5 x weight, far
beyond its bound.  Distinct extremes (above 2, below 0.2) sit in the first, the last and the seam cells of every component, so a cell
left out changes a maximum or a minimum.  Ghost cells and row padding of every device array are poisoned (NaN and 1e300 in turn) before
the interior is uploaded, and the output buffers hold all-ones bits before a call.

Bounds (u = 2^-53, n removed cells per output cell, values converted exactly to float64):
  SUM   |got - exact| <= (n + 1) u sum|x w|     one rounding per product and the first-order bound of ANY summation order; ``exact`` is
        ``math.fsum`` over the products, each kept as an unevaluated sum of two doubles (Dekker's product): one rounding in all
  mean  the same bound divided by w n, plus (n + 1) u |mean| for the divisor and the division
  MAX / MIN, boxes   bit for bit
  non-finite cells   the class of every output cell (NaN, +inf, -inf, finite) is numpy's, for every method
"""

from __future__ import annotations

import ctypes as C
import functools
import itertools
import math

import numpy as np
import pytest
import stats_cases as S

import pde_hip
from pde_hip.device import DeviceArray, DeviceBuffer

U = S.U
DTYPES = S.DTYPES
SMALL = S.SMALL            # fastest-axis extents 1, 2, 3, 4, 5, 63, 64, 65, 257; rows of 1-3 cells; 1-D to 3-D; 1 / 3 / 9 components
SUM, MAX, MIN = 0, 1, 2
METHODS = (SUM, MAX, MIN)
WEIGHT = 0.37              # (not a power of two: every product rounds)
SEGMENT = 128              # kProjectSegment of csrc/pdehip_project.hip: removed cells one thread of the march takes
TURN_THREADS = 1024 * 256  # kProjectBlocksMax workgroups of 256 threads: what is beyond takes a grid-stride turn

# removed extents around the cut of the march into segments: one segment exactly, one cell more, one cell less than two segments
SEGMENT_EXTENTS = (SEGMENT, SEGMENT + 1, 2 * SEGMENT - 1)
# instance -> (dtype, fastest extent): fp64 one cell / pairs, fp32 one cell / quads
MARCH_INSTANCES = {"f64x1": (np.float64, 3), "f64x2": (np.float64, 6), "f32x1": (np.float32, 3), "f32x4": (np.float32, 8)}
# beyond the turn, one shape per instance: rows x 64 lanes > TURN_THREADS for the row kernel (65 pieces per row: the 64 lanes take a second
# piece), output pieces > TURN_THREADS for the march
TURN = {
    "row_f64x1": ((65, 64, 65), np.float64, 0b100), "row_f64x2": ((65, 64, 130), np.float64, 0b100),
    "row_f32x1": ((65, 64, 65), np.float32, 0b100), "row_f32x4": ((65, 64, 260), np.float32, 0b100),
    "march_f64x1": ((3, 513, 513), np.float64, 0b001), "march_f64x2": ((3, 513, 1026), np.float64, 0b001),
    "march_f32x1": ((3, 513, 513), np.float32, 0b001), "march_f32x4": ((3, 513, 2052), np.float32, 0b001),
}
BOX_TURN = (65, 64, 65)


def masks(ndim: int):
    """Every non-empty subset of the axes: bit a removes axis a."""
    return range(1, 1 << ndim)


def removed_axes(mask: int, ndim: int) -> tuple[int, ...]:
    return tuple(a for a in range(ndim) if mask >> a & 1)


def expected_chain(shape, dtype, mask: int, method: int) -> str:
    """The kernel instances ``pdehip_project`` chains for this call, as ``pdehip_last_kernel_name`` reports them."""
    ndim = len(shape)
    n = [1] * (3 - ndim) + list(shape)
    nm = sum(1 << (3 - ndim + a) for a in removed_axes(mask, ndim))
    f64 = np.dtype(dtype) == np.float64
    kind, vec, op = ("double" if f64 else "float"), S.vec_width(dtype, n[2]), ("sum" if method == SUM else "max")
    names = []
    while nm:
        if nm & 4:
            names.append(f"project_row_kernel<{kind},{vec},{op}>")
            n, nm = [1, n[0], n[1]], (nm & 3) << 1
        else:
            names.append(f"project_march_kernel<{kind},{vec},{op}>")
            m = (n[0] if nm & 1 else 1) * (n[1] if nm & 2 else 1)
            nseg = -(-m // SEGMENT)
            n, nm = [nseg, 1, n[0] * n[1] // m * n[2]], (0 if nseg == 1 else 1)
        kind, vec = "double", 1
    return "+".join(names)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _spots(n: int) -> list[int]:
    return sorted({s for s in (0, n - 1, 63, 64, 127, 128, 255, 256, n // 2) if 0 <= s < n})


def plant_extremes(valid: np.ndarray) -> np.ndarray:
    """Distinct values above and below the bands, in turn, in the first, last and seam cells of every component."""
    out = valid.copy()
    flat = out.reshape(out.shape[0], -1)
    for c in range(flat.shape[0]):
        for m, at in enumerate(_spots(flat.shape[1])):
            flat[c, at] = (2.0 + 0.03125 * m + 0.25 * c) if (m + c) % 2 == 0 else 1.0 / (8.0 + m + 16.0 * c)
    return out


def plant_nonfinite(valid: np.ndarray) -> np.ndarray:
    """NaN, +inf and -inf in turn in the first, last and seam cells, and a -inf / +inf pair side by side in the middle of every component."""
    out = S.plant_nonfinite(valid)
    flat = out.reshape(out.shape[0], -1)
    n = flat.shape[1]
    if n >= 6:
        flat[:, n // 2 - 2], flat[:, n // 2 - 1] = -np.inf, np.inf
    return out


@functools.lru_cache(maxsize=None)
def small_inputs(case, dtype_name: str, planted: bool) -> np.ndarray:
    shape, ncomp = case
    valid = S.draw(shape, ncomp, np.dtype(dtype_name))
    valid = plant_nonfinite(valid) if planted else plant_extremes(valid)
    valid.setflags(write=False)
    return valid


@functools.lru_cache(maxsize=None)
def drawn(shape, ncomp: int, dtype_name: str, seed: int = 7) -> np.ndarray:
    valid = plant_extremes(S.draw(shape, ncomp, np.dtype(dtype_name), seed=seed))
    valid.setflags(write=False)
    return valid


upload = S.upload
bits = S.bits


# ---- drivers ------------------------------------------------------------------------------------------------------------------------
def project(lib, dev: DeviceArray, mask: int, method: int, weight: float = WEIGHT, stream=None, out: DeviceBuffer | None = None) -> np.ndarray:
    """``(ncomp, retained extents...)``: float64 for SUM, the field's type else; the output buffer holds all-ones bits before the call."""
    shape = dev.info.shape
    retained = tuple(n for a, n in enumerate(shape) if not mask >> a & 1)
    host = np.empty((dev.ncomp, *retained), dtype=np.float64 if method == SUM else dev.dtype)
    out = DeviceBuffer(max(host.nbytes, 8)) if out is None else out
    lib.memset(out.ptr, 0xFF, host.nbytes, stream)
    lib.project(dev.info.ref, dev.ncomp, dev.ptr, mask, method, C.c_double(weight), out.ptr, stream)
    lib.memcpy_d2h(host.ctypes.data, out.ptr, host.nbytes, stream)
    return host


def extract_box(lib, dev: DeviceArray, lo, extent, stream=None) -> np.ndarray:
    ndim = len(dev.info.shape)
    host = np.empty((dev.ncomp, *extent), dtype=dev.dtype)
    out = DeviceBuffer(max(host.nbytes, 8))
    lib.memset(out.ptr, 0xFF, host.nbytes, stream)
    lib.extract_box(dev.info.ref, dev.ncomp, dev.ptr, (C.c_long * ndim)(*lo), (C.c_long * ndim)(*extent), out.ptr, stream)
    lib.memcpy_d2h(host.ctypes.data, out.ptr, host.nbytes, stream)
    return host


def kernel_name(lib) -> str:
    return lib.last_kernel_name().decode()


# ---- restatements -------------------------------------------------------------------------------------------------------------------
def np_project(valid: np.ndarray, mask: int, method: int, weight: float = WEIGHT) -> np.ndarray:
    """numpy's own result: ``(data * volumes).sum(axes)`` with the volumes as a float64 ARRAY (grid.integrate), ``np.max`` / ``np.min``."""
    axes = tuple(1 + a for a in removed_axes(mask, valid.ndim - 1))
    with np.errstate(invalid="ignore", over="ignore"):
        if method == SUM:
            return (valid * np.full((1,) * valid.ndim, weight)).sum(axis=axes)
        return (np.max if method == MAX else np.min)(valid, axis=axes)


def _lines(valid: np.ndarray, mask: int) -> np.ndarray:
    """float64 values as (output cells, removed cells)."""
    ndim = valid.ndim - 1
    removed = removed_axes(mask, ndim)
    x = np.moveaxis(valid.astype(np.float64), [1 + a for a in removed], range(-len(removed), 0))
    n = int(np.prod([valid.shape[1 + a] for a in removed]))
    return np.ascontiguousarray(x).reshape(-1, n)


def _two_product(a: np.ndarray, b: float):
    """a * b as an unevaluated sum p + e of two doubles (Veltkamp's split, Dekker's product)."""
    p = a * b
    c = 134217729.0 * a
    ah = c - (c - a)
    al = a - ah
    cb = 134217729.0 * b
    bh = cb - (cb - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def check_sum(got: np.ndarray, valid: np.ndarray, mask: int, weight: float = WEIGHT, what: str = "", mean: bool = False) -> None:
    """SUM (or, with ``mean``, SUM / (weight x n)) against ``math.fsum``; output cells whose numpy result is not finite by class."""
    lines = _lines(valid, mask)
    n = lines.shape[1]
    ref = np_project(valid, mask, SUM, weight)
    assert got.shape == ref.shape and got.dtype == np.float64, f"{what}: {got.shape} {got.dtype}, expected {ref.shape} float64"
    got, ref = got.ravel(), ref.ravel()
    finite = np.isfinite(ref)
    for name, fn in (("isnan", np.isnan), ("isposinf", np.isposinf), ("isneginf", np.isneginf)):
        assert np.array_equal(fn(got), fn(ref)), f"{what}: {name} differs from numpy's in {int((fn(got) != fn(ref)).sum())} output cells"
    rows = lines[finite]
    p, e = _two_product(rows, weight)
    exact = np.fromiter(map(math.fsum, np.concatenate([p, e], axis=1).tolist()), dtype=np.float64, count=len(rows))
    bound = (n + 1) * U * np.abs(p).sum(axis=1)
    if mean:
        exact = exact / (weight * n)
        bound = bound / (weight * n) + (n + 1) * U * np.abs(exact)
    err = np.abs(got[finite] - exact)
    worst = int(np.argmax(err - bound)) if len(rows) else 0
    if len(rows):
        print(f"{what}: n {n}, {len(rows)} finite output cells, worst error {err[worst]:.3e} of bound {bound[worst]:.3e}")
    assert np.all(err <= bound), f"{what}: off by {err[worst]:.3e} > {bound[worst]:.3e} (n = {n})"


def check_extreme(got: np.ndarray, valid: np.ndarray, mask: int, method: int, what: str = "") -> None:
    ref = np_project(valid, mask, method)
    assert got.shape == ref.shape and got.dtype == valid.dtype, f"{what}: {got.shape} {got.dtype}, expected {ref.shape} {valid.dtype}"
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN in other output cells than numpy's"
    assert np.array_equal(bits(got[~nan]), bits(ref[~nan])), f"{what}: {int((bits(got[~nan]) != bits(ref[~nan])).sum())} output cells differ from numpy's"


def check_all_methods(lib, valid: np.ndarray, shape, what: str = "", chain=None) -> None:
    """Every non-empty axis subset, the three methods, two calls on fresh uploads; ``chain(mask, method)``: the instances expected."""
    dev = upload(lib, shape, valid)
    for mask, method in itertools.product(masks(len(shape)), METHODS):
        tag = f"{what} mask {mask:03b} method {method}"
        got = project(lib, dev, mask, method)
        if chain is not None:
            assert kernel_name(lib) == chain(mask, method), f"{tag}: ran {kernel_name(lib)}, expected {chain(mask, method)}"
        if method == SUM:
            check_sum(got, valid, mask, what=tag)
        else:
            check_extreme(got, valid, mask, method, what=tag)
        again = project(lib, upload(lib, shape, valid), mask, method)
        assert np.array_equal(bits(got), bits(again)), f"{tag}: two calls differ"


# ---- boxes --------------------------------------------------------------------------------------------------------------------------
def box_cases(shape):
    """(lo, extent): every axis cut at index 0, the middle and the last cell; the whole grid; one cell."""
    ndim = len(shape)
    cases = [((0,) * ndim, tuple(shape)), (tuple(n // 2 for n in shape), (1,) * ndim), (tuple(n - 1 for n in shape), (1,) * ndim)]
    for ax in range(ndim):
        for at in sorted({0, shape[ax] // 2, shape[ax] - 1}):
            cases.append((tuple(at if a == ax else 0 for a in range(ndim)), tuple(1 if a == ax else shape[a] for a in range(ndim))))
    if ndim == 3:      # a line: two axes cut
        cases.append(((shape[0] // 2, 0, shape[2] - 1), (1, shape[1], 1)))
        cases.append(((1 if shape[0] > 1 else 0, 0, 0), (shape[0] - (1 if shape[0] > 1 else 0), max(shape[1] - 1, 1), max(shape[2] - 2, 1))))
    return cases


def check_boxes(lib, valid: np.ndarray, shape, what: str = "") -> None:
    dev = upload(lib, shape, valid)
    for lo, extent in box_cases(shape):
        got = extract_box(lib, dev, lo, extent)
        ref = valid[(slice(None), *(slice(a, a + n) for a, n in zip(lo, extent)))]
        assert np.array_equal(bits(got), bits(ref)), f"{what}: box {lo} + {extent} differs"


# ---- checks the CPU and the GPU test share ------------------------------------------------------------------------------------------
METHOD_NAMES = ("integral", "average", "mean", "maximum", "max", "minimum", "min")


def refuse_bad_arguments(lib) -> None:
    """Shared with the GPU test: NULL pointers, ncomp outside 1 ... 64, empty and foreign masks, an unknown method, boxes outside the grid,
    misaligned arrays."""
    valid = S.draw((4, 6), 1, np.float64)
    dev = upload(lib, (4, 6), valid)
    out = DeviceBuffer(512)
    import ctypes as C

    def longs(*v):
        return (C.c_long * len(v))(*v)

    bad_project = [(1, None, 1, 0, out.ptr), (1, dev.ptr, 1, 0, None), (0, dev.ptr, 1, 0, out.ptr), (65, dev.ptr, 1, 0, out.ptr), (1, dev.ptr, 0, 0, out.ptr),
                   (1, dev.ptr, 4, 0, out.ptr), (1, dev.ptr, 7, 0, out.ptr), (1, dev.ptr, -1, 0, out.ptr), (1, dev.ptr, 1, 3, out.ptr), (1, dev.ptr, 1, -1, out.ptr),
                   (1, dev.ptr + 8, 1, 0, out.ptr), (1, dev.ptr, 1, 0, out.ptr + 4)]
    for ncomp, arr, mask, method, dst in bad_project:
        with pytest.raises(ValueError):
            lib.project(dev.info.ref, ncomp, arr, mask, method, 1.0, dst, None)
    bad_box = [(1, None, longs(0, 0), longs(1, 1), out.ptr), (1, dev.ptr, None, longs(1, 1), out.ptr), (1, dev.ptr, longs(0, 0), None, out.ptr),
               (1, dev.ptr, longs(0, 0), longs(1, 1), None), (0, dev.ptr, longs(0, 0), longs(1, 1), out.ptr), (65, dev.ptr, longs(0, 0), longs(1, 1), out.ptr),
               (1, dev.ptr, longs(-1, 0), longs(1, 1), out.ptr), (1, dev.ptr, longs(0, 0), longs(5, 1), out.ptr), (1, dev.ptr, longs(3, 0), longs(2, 1), out.ptr),
               (1, dev.ptr, longs(0, 6), longs(1, 1), out.ptr), (1, dev.ptr, longs(0, 0), longs(0, 1), out.ptr), (1, dev.ptr, longs(0, 2), longs(1, 5), out.ptr),
               (1, dev.ptr + 8, longs(0, 0), longs(1, 1), out.ptr), (1, dev.ptr, longs(0, 0), longs(1, 1), out.ptr + 4)]
    for ncomp, arr, lo, extent, dst in bad_box:
        with pytest.raises(ValueError):
            lib.extract_box(dev.info.ref, ncomp, arr, lo, extent, dst, None)
    # ... and the good call next to them
    lib.project(dev.info.ref, 1, dev.ptr, 3, SUM, 1.0, out.ptr, None)
    lib.extract_box(dev.info.ref, 1, dev.ptr, longs(3, 5), longs(1, 1), out.ptr, None)


def check_against_reference(got, ref, field_data: np.ndarray, ax_remove, method: str, weight: float) -> None:
    """A projected field against the reference method's: extrema bit for bit, integrals and means inside the bound of the sums."""
    assert got.grid.shape == ref.grid.shape and list(got.grid.axes) == list(ref.grid.axes) and got.data.dtype == ref.data.dtype
    if method in ("maximum", "max", "minimum", "min"):
        assert np.array_equal(bits(np.ascontiguousarray(got.data)), bits(np.ascontiguousarray(ref.data)))
        return
    mask = sum(1 << ax for ax in ax_remove)
    for data in (got.data, ref.data):
        check_sum(np.ascontiguousarray(data)[None], field_data[None], mask, weight, what=method, mean=method != "integral")


def run_mirror(backend, tracker, dtype=np.float64, shape=(8, 6, 10)):
    grid = pde_hip.UnitGrid(shape, periodic=True)
    state = pde_hip.ScalarField(grid, S.draw(shape, 1, dtype, seed=5)[0], label="c")
    return pde_hip.DiffusionPDE(0.5).solve(state, t_range=0.4, dt=0.05, solver="euler", backend=backend, tracker=tracker, interval=0.1)


def resident_run_checks(backend, dtype=np.float64) -> None:
    """Shared with the GPU test.  A diffusion run whose tracker projects and slices the resident state through ``pde_hip.project`` /
    ``pde_hip.slice_field`` / ``line_data`` / ``image_data``: nothing is downloaded, the results equal the mirror methods on a pulled
    copy, and the final state has the bits of the run without a tracker."""
    seen = []

    def tracker(field, t):
        link = field.__dict__.get("_hip_link")
        if link is None or not link.host_stale:
            return
        got = {"int_z": pde_hip.project(field, "z"), "mean_xy": pde_hip.project(field, ["x", "y"], method="mean"),
               "max_y": pde_hip.project(field, "y", method="max"), "min_xz": pde_hip.project(field, ["z", "x"], method="min"),
               "mid": pde_hip.slice_field(field, {"z": "mid"}), "line": pde_hip.slice_field(field, {"x": "low", "y": 2.2}),
               "cut": pde_hip.line_data(field, "cut_y"), "proj": pde_hip.line_data(field, "project_x"), "image": pde_hip.image_data(field)}
        assert link.downloads == 0 and type(field) is not pde_hip.ScalarField
        pulled = pde_hip.ScalarField(field.grid, link.dev_state.get_valid(), label=field.label)      # a side copy: not a download of the field
        seen.append((got, pulled))

    res = run_mirror(backend, tracker, dtype)
    assert res.__dict__["_hip_link"].downloads == 0 and len(seen) >= 3
    plain = run_mirror(backend, None, dtype)
    assert np.array_equal(bits(np.ascontiguousarray(res.data)), bits(np.ascontiguousarray(plain.data)))
    for got, pulled in seen:
        data = np.ascontiguousarray(pulled.data)
        check_against_reference(got["int_z"], pulled.project("z"), data, (2,), "integral", 1.0)
        check_against_reference(got["mean_xy"], pulled.project(["x", "y"], method="mean"), data, (0, 1), "mean", 1.0)
        check_against_reference(got["max_y"], pulled.project("y", method="max"), data, (1,), "max", 1.0)
        check_against_reference(got["min_xz"], pulled.project(["z", "x"], method="min"), data, (0, 2), "min", 1.0)
        for key, position in (("mid", {"z": "mid"}), ("line", {"x": "low", "y": 2.2})):
            ref = pulled.slice(position)
            assert got[key].grid == ref.grid and got[key].data.tobytes() == ref.data.tobytes() and got[key].data.dtype == ref.data.dtype
        for key, ref in (("cut", pulled.get_line_data(extract="cut_y")), ("proj", pulled.get_line_data(extract="project_x")), ("image", pulled.get_image_data())):
            assert set(got[key]) == set(ref)
            for name, value in ref.items():
                if name == "data_y" and key == "proj":
                    assert got[key][name].dtype == value.dtype
                    check_sum(got[key][name].astype(np.float64)[None], data[None], 0b110, 1.0, what="project_x", mean=True) if dtype == np.float64 else \
                        np.testing.assert_allclose(got[key][name], value, rtol=2e-7)
                elif isinstance(value, np.ndarray):
                    assert np.array_equal(got[key][name], value) and got[key][name].dtype == value.dtype, (key, name)
                else:
                    assert got[key][name] == value, (key, name)


def resident_key_checks(backend) -> None:
    """Shared with the GPU test.  ``device_projections`` on: the field's own methods leave the state on the device; off: they download,
    exactly as before, and return numpy's bits."""
    seen = {}
    for flag in (True, False):
        rows = seen[flag] = []

        def tracker(field, t, rows=rows):
            link = field.__dict__.get("_hip_link")
            if link is None or not link.host_stale:
                return
            pulled = pde_hip.ScalarField(field.grid, link.dev_state.get_valid(), label=field.label)
            before = link.downloads
            got = (field.project("z"), field.project(["x", "z"], method="max")) if flag else (field.project("z"),)
            rest = (field.slice({"y": "high"}), field.get_line_data(extract="project_z"), field.get_image_data(transpose=True)) if flag else ()
            rows.append((got + rest, pulled, before, link.downloads))

        backend.device_projections = flag
        try:
            run_mirror(backend, tracker)
        finally:
            backend.device_projections = None
    assert len(seen[True]) >= 3 and len(seen[False]) >= 3
    for got, pulled, before, after in seen[False]:
        assert after == before + 1
        assert got[0].data.tobytes() == pulled.project("z").data.tobytes()
    for got, pulled, before, after in seen[True]:
        assert after == before == 0
        data = np.ascontiguousarray(pulled.data)
        check_against_reference(got[0], pulled.project("z"), data, (2,), "integral", 1.0)
        check_against_reference(got[1], pulled.project(["x", "z"], method="max"), data, (0, 2), "max", 1.0)
        assert got[2].data.tobytes() == pulled.slice({"y": "high"}).data.tobytes()
        np.testing.assert_allclose(got[3]["data_y"], pulled.get_line_data(extract="project_z")["data_y"], rtol=1e-13)
        ref = pulled.get_image_data(transpose=True)
        assert np.array_equal(got[4]["data"], ref["data"]) and got[4]["extent"] == ref["extent"] and got[4]["label_x"] == ref["label_x"] == "y"
