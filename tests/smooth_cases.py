"""Cases, the numpy restatement and the drivers for the smoothing entry point ``pdehip_smooth_axis``.

Shared by ``tests/test_smooth_cpu.py`` (CPU: the C version of the tests-only shim) and ``tests/test_hip_smooth.py`` (GPU: the kernels of
``csrc/pdehip_smooth.hip``).  The restatement is written from the arithmetic in ``include/pdehip.h`` - gathers through an index per tap,
not the extended line of ``pde_hip/smoothing.py`` - and is itself checked against the reference's results (``tests/golden/smooth.npz``,
written by ``tests/golden/make_golden_smooth.py``) and against scipy where it imports.  The drivers call the entry point through whatever
library ``pde_hip._lib`` holds, so the same checks serve both.

Every check is bit for bit: a cell that is not NaN in the restatement has the restatement's bits (+-inf and signed zeros included), a NaN
cell is NaN.  There is no tolerance anywhere: the arithmetic fixes every rounding.

Inputs (``stats_cases.draw``): values from [0.5, 0.6] u [1.4, 1.5] with full mantissas, so another order of the additions, a contracted
product or a neighbour taken from the wrong cell changes last bits or far more in many cells.  Ghost cells and row padding of the input
hold NaN and 1e300 in turn, those of the output a sentinel: a read outside the interior poisons a result, a write outside it shows.
"""

from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import stats_cases as S

import pde_hip
from pde_hip.device import DeviceArray, GridInfo

DTYPES = S.DTYPES
WRAP, REFLECT, CELL = 0, 1, 16
MODES = (WRAP, REFLECT)
# the geometry of csrc/pdehip_smooth.hip (kRowLanes ... kSmoothBlocksMax)
ROW_LANES, ROW_PIECES, ROW_RADIUS_MAX = 64, 4, 608
MARCH_WIDTH, MARCH_LENGTH, MARCH_RADIUS_MAX = 32, 64, 48
BLOCKS_MAX = 2048
SENTINEL = {np.dtype(np.float64): 0x7FF4_5EED_0BAD_F00D, np.dtype(np.float32): 0x7FA5_EED1}      # (NaN payloads no arithmetic produces)

bits = S.bits
upload = S.upload


def kernel_name(lib) -> str:
    return lib.last_kernel_name().decode()


# ---- weights ------------------------------------------------------------------------------------------------------------------------
def gaussian_weights(sigma_cells: float) -> np.ndarray:
    """scipy's ``_gaussian_kernel1d(sigma, 0, int(4 sigma + 0.5))``, upper half, centre first."""
    r = int(4.0 * float(sigma_cells) + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma_cells * sigma_cells) * x**2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[r:])


@functools.lru_cache(maxsize=None)
def radius_weights(r: int) -> np.ndarray:
    """Weights of a GIVEN radius for the tests through the C ABI: a normalised bell of width r / 3 cells, all values distinct, none a
    power of two (every product rounds)."""
    j = np.arange(r + 1, dtype=np.float64)
    w = np.exp(-0.5 * (j / max(r / 3.0, 0.4)) ** 2) + 1e-3 / (1.0 + j)
    w = w / (w[0] + 2.0 * w[1:].sum())
    w.setflags(write=False)
    return w


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def resolve(p: np.ndarray, n: int, mode: int) -> np.ndarray:
    if mode == WRAP:
        return np.mod(p, n)
    q = np.mod(p, 2 * n)
    return np.where(q < n, q, 2 * n - 1 - q)


def filter_axis(valid: np.ndarray, axis: int, w: np.ndarray, mode: int, dtype=None) -> np.ndarray:
    """One pass over ``valid`` = (components, *grid shape) along grid axis ``axis``: include/pdehip.h, tap by tap."""
    ax = 1 + axis
    n, r = valid.shape[ax], len(w) - 1
    x = valid.astype(np.float64)
    i = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x * w[0]
        for j in range(r, 0, -1):
            t = t + (np.take(x, resolve(i - j, n, mode), axis=ax) + np.take(x, resolve(i + j, n, mode), axis=ax)) * w[j]
        return t.astype(valid.dtype if dtype is None else dtype)


def assert_same(got: np.ndarray, ref: np.ndarray, what: str = "") -> None:
    assert got.shape == ref.shape and got.dtype == ref.dtype, f"{what}: {got.shape} {got.dtype}, expected {ref.shape} {ref.dtype}"
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN in other cells than the restatement's ({int((np.isnan(got) != nan).sum())} cells)"
    differ = bits(got)[~nan] != bits(ref)[~nan]
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} cells differ, first at {np.argwhere(bits(got) != bits(ref))[0]}"


# ---- drivers ------------------------------------------------------------------------------------------------------------------------
def raw(lib, dev: DeviceArray) -> np.ndarray:
    """Every element of the allocation, ghost cells, padding and slack included, as unsigned integers."""
    host = np.empty(dev.nbytes // dev.itemsize, dtype=dev.dtype)
    lib.memcpy_d2h(host.ctypes.data, dev.ptr, dev.nbytes, None)
    return bits(host)


@functools.lru_cache(maxsize=64)
def interior_mask(shape, ncomp: int, dtype_name: str) -> np.ndarray:
    """Which elements of an allocation are interior cells."""
    lib = pde_hip._lib.require_device()
    dev = DeviceArray(GridInfo(shape, (1.0,) * len(shape), np.dtype(dtype_name)), (ncomp,))
    lib.memset(dev.ptr, 0, dev.nbytes, None)
    dev.set_valid(np.ones((ncomp, *shape), dtype=dtype_name), None)
    return raw(lib, dev) != 0


def sentinel_array(lib, like: DeviceArray) -> DeviceArray:
    out = DeviceArray(like.info, like.comp_shape)
    fill = np.full(out.nbytes // out.itemsize, SENTINEL[np.dtype(out.dtype)], dtype=np.uint64 if out.itemsize == 8 else np.uint32)
    lib.memcpy_h2d(out.ptr, fill.ctypes.data, out.nbytes, None)
    return out


def smooth_axis(lib, src: DeviceArray, dst: DeviceArray, axis: int, w: np.ndarray, mode: int, stream=None) -> None:
    w = np.ascontiguousarray(w, dtype=np.float64)
    lib.smooth_axis(src.info.ref, src.ncomp, src.ptr, dst.ptr, axis, mode, len(w) - 1, w.ctypes.data_as(C.POINTER(C.c_double)), stream)


def run_pass(lib, dev: DeviceArray, axis: int, w: np.ndarray, mode: int, what: str = "") -> np.ndarray:
    """One pass into an array full of sentinels: the interior comes back; ghost cells, padding and slack of the output still hold the
    sentinel and the input has the bits it had."""
    before = raw(lib, dev)
    out = sentinel_array(lib, dev)
    smooth_axis(lib, dev, out, axis, w, mode)
    got = out.get_valid()
    mask = interior_mask(dev.info.shape, dev.ncomp, np.dtype(dev.dtype).name)
    after = raw(lib, out)
    assert np.all(after[~mask] == SENTINEL[np.dtype(dev.dtype)]), f"{what}: {int((after[~mask] != SENTINEL[np.dtype(dev.dtype)]).sum())} cells outside the interior were written"
    assert np.array_equal(raw(lib, dev), before), f"{what}: the input was modified"
    return got


def expected_instance(shape, dtype, axis: int, r: int) -> str:
    """The instance ``pdehip_smooth_axis`` launches without PDEHIP_SMOOTH_CELL."""
    kind = "double" if np.dtype(dtype) == np.float64 else "float"
    if axis == len(shape) - 1:
        return f"gauss_row_kernel<{kind}>" if r <= ROW_RADIUS_MAX else f"gauss_cell_kernel<{kind}>"
    return f"gauss_march_kernel<{kind},{S.vec_width(dtype, shape[-1])}>" if r <= MARCH_RADIUS_MAX else f"gauss_cell_kernel<{kind}>"


def check_pass(lib, valid: np.ndarray, shape, axis: int, w: np.ndarray, mode: int, what: str = "", device: bool = True, dev=None) -> None:
    """The instance the host chooses and the one-cell-per-thread instance against the restatement, bit for bit; a second call on a fresh
    upload gives the same bits.  ``device``: assert the names of the instances (the shim has none)."""
    ref = filter_axis(valid, axis, w, mode)
    dev = upload(lib, shape, valid) if dev is None else dev
    got = run_pass(lib, dev, axis, w, mode, what)
    if device:
        name, expect = kernel_name(lib), expected_instance(shape, valid.dtype, axis, len(w) - 1)
        assert name == expect, f"{what}: ran {name}, expected {expect}"
    assert_same(got, ref, what)
    yard = run_pass(lib, dev, axis, w, mode | CELL, what + " (cell)")
    if device:
        assert kernel_name(lib).startswith("gauss_cell_kernel<"), f"{what}: PDEHIP_SMOOTH_CELL ran {kernel_name(lib)}"
    assert_same(yard, ref, what + " (cell)")
    again = run_pass(lib, upload(lib, shape, valid), axis, w, mode, what + " (again)")
    assert np.array_equal(bits(got), bits(again)), f"{what}: two calls differ"


def radii(n: int) -> list[int]:
    return sorted({0, 1, 2, 7, max(n - 1, 0), n, n + 1, 2 * n + 3})


# filtered extents: tiny lines, the seams of a wave / a row piece (64), of the march tile (L = 64: L-1, L, L+1, 2L+1) and beyond two pieces
EXTENTS = (1, 2, 3, 5, 63, 64, 65, 129, 130)
FASTEST = (1, 3, 64, 65, 130)      # fastest extents of the march: no / one / two full tiles of 32 cells and a tail, vector widths 1, 2, 4


def tiling_cases(kind: str):
    """(shape, axis, ncomp) for ``kind``: ``row`` (the fastest axis of 1-D, 2-D and 3-D grids), ``march0of3`` / ``march1of3`` (axes 0 and
    1 of 3-D grids), ``march0of2``.  Every filtered extent meets two fastest extents, every fastest extent several filtered ones."""
    cases = []
    for m, n in enumerate(EXTENTS):
        ncomp = 1 if m % 2 else 3
        if kind == "row":
            cases.append(((n,), 0, ncomp) if m % 3 == 0 else (((3, n), 1, ncomp) if m % 3 == 1 else ((2, 3, n), 2, ncomp)))
            continue
        for n2 in (FASTEST[m % 5], FASTEST[(m + 2) % 5]):
            cases.append({"march0of3": ((n, 2, n2), 0, ncomp), "march1of3": ((3, n, n2), 1, ncomp), "march0of2": ((n, n2), 0, ncomp)}[kind])
    return cases


TILING_KINDS = ("row", "march0of3", "march1of3", "march0of2")

# each instance's radius cap and the cap plus 1: (shape, axis, radius below the switch)
CAPS = {"row": ((2, 70), 1, ROW_RADIUS_MAX), "march0of3": ((70, 2, 6), 0, MARCH_RADIUS_MAX), "march1of3": ((2, 70, 5), 1, MARCH_RADIUS_MAX),
        "march0of2": ((70, 36), 0, MARCH_RADIUS_MAX)}

# one shape per instance beyond the grid-stride turn of a launch capped at BLOCKS_MAX workgroups: (shape, dtype, axis)
TURN = {
    "row_f64": ((65, 64, 130), np.float64, 2), "row_f32": ((65, 64, 130), np.float32, 2),
    "march_f64x2": ((65, 130, 260), np.float64, 0), "march_f64x1": ((65, 130, 259), np.float64, 0),
    "march_f32x4": ((65, 130, 260), np.float32, 0), "march_f32x1": ((65, 130, 259), np.float32, 0),
    "cell_f64": ((65, 64, 130), np.float64, 1), "cell_f32": ((65, 64, 130), np.float32, 1),
}


def turn_workgroups(key: str) -> int:
    shape, _, axis = TURN[key]
    if key.startswith("row"):
        return -(-(shape[0] * shape[1] * -(-shape[2] // ROW_LANES)) // ROW_PIECES)
    if key.startswith("march"):
        return shape[1] * -(-shape[0] // MARCH_LENGTH) * -(-shape[2] // MARCH_WIDTH)
    return -(-int(np.prod(shape)) // 256)


@functools.lru_cache(maxsize=None)
def drawn(shape, ncomp: int, dtype_name: str, seed: int = 3, planted: bool = False) -> np.ndarray:
    valid = S.draw(shape, ncomp, np.dtype(dtype_name), seed=seed)
    if planted:
        valid = S.plant_nonfinite(valid)
    valid.setflags(write=False)
    return valid


# ---- the golden cases (tests/golden/make_golden_smooth.py) ------------------------------------------------------------------------------
# id -> (field class, dtype, shape, periodic, spacings, sigma).  Radii per axis, r = int(4 sigma / dx + 0.5), against the extents n:
#   s1d_wrap      n 5: r 4 = n-1            s1d_reflect  n 5: r 5 = n           s1d_over   n 5: r 6 = n+1        s1d_far  n 3: r 7 > 2n
#   s2d           (9, 7): r 0, 4            s3d          (12, 10, 14): r 1, 4, 16 > n          s3d_f32  (6, 5, 7): r 2, 5 = n, 0
#   v3d           (4, 5, 6): r 8 = 2n, 2, 1   t2d_f32    (5, 4): r 1, 9 > 2n       one_cell  (1, 4): r 2 > 2n on n = 1, r 1
GOLDEN = {
    "s1d_wrap": ("ScalarField", "float64", (5,), (True,), (1.0,), 1.0),
    "s1d_reflect": ("ScalarField", "float64", (5,), (False,), (0.5,), 0.6),
    "s1d_over": ("ScalarField", "float32", (5,), (False,), (2.0,), 2.8),
    "s1d_far": ("ScalarField", "float64", (3,), (True,), (1.0,), 1.7),
    "s2d": ("ScalarField", "float64", (9, 7), (False, True), (4.0, 0.4), 0.4),
    "s3d": ("ScalarField", "float64", (12, 10, 14), (True, False, True), (2.0, 0.5, 0.125), 0.5),
    "s3d_f32": ("ScalarField", "float32", (6, 5, 7), (False, True, False), (1.5, 0.6, 6.5), 0.75),
    "v3d": ("VectorField", "float64", (4, 5, 6), (True, True, False), (0.25, 1.0, 2.0), 0.5),
    "t2d_f32": ("Tensor2Field", "float32", (5, 4), (True, False), (2.4, 0.25), 0.55),
    "one_cell": ("ScalarField", "float64", (1, 4), (False, True), (0.5, 1.0), 0.3),
}


def golden_input(cid: str) -> np.ndarray:
    """The data of a golden field, ``(dim,) * rank + shape``."""
    cls, dtype, shape, _, _, _ = GOLDEN[cid]
    rank = {"ScalarField": 0, "VectorField": 1, "Tensor2Field": 2}[cls]
    ncomp = len(shape) ** rank
    return S.draw(shape, ncomp, np.dtype(dtype), seed=len(cid)).reshape((len(shape),) * rank + tuple(shape))


def golden_bounds(cid: str):
    _, _, shape, _, dx, _ = GOLDEN[cid]
    return [(0.25, 0.25 + n * d) for n, d in zip(shape, dx)]


@functools.lru_cache(maxsize=None)
def golden():
    import pathlib

    return dict(np.load(pathlib.Path(__file__).parent / "golden" / "smooth.npz"))


def check_golden_passes(lib, cid: str, device: bool = True) -> None:
    """A golden case through the C ABI: every pass on the stored intermediate result of the pass before (axis by axis), and the passes
    chained on the device between two arrays, against the reference's final result; the stored weights are the ones handed over."""
    cls, dtype, shape, periodic, dx, sigma = GOLDEN[cid]
    data = golden()
    valid = golden_input(cid).reshape((-1, *shape))
    cur, spare = upload(lib, shape, valid), None
    work = [sentinel_array(lib, cur), sentinel_array(lib, cur)]
    stage = valid
    for axis in range(len(shape)):
        w = data[f"{cid}/w{axis}"]
        mode = WRAP if periodic[axis] else REFLECT
        ref = data[f"{cid}/axis{axis}"].reshape(valid.shape)
        got = run_pass(lib, upload(lib, shape, stage), axis, w, mode, f"{cid} axis {axis}")
        if device:
            assert kernel_name(lib) == expected_instance(shape, valid.dtype, axis, len(w) - 1)
        assert_same(got, ref, f"{cid} axis {axis}")
        smooth_axis(lib, cur, work[axis % 2], axis, w, mode)
        cur, stage = work[axis % 2], ref
    assert_same(cur.get_valid(), data[f"{cid}/out"].reshape(valid.shape), f"{cid} chained")


# ---- checks the CPU and the GPU test share ------------------------------------------------------------------------------------------
def refuse_bad_arguments(lib) -> None:
    """NULL pointers, ncomp outside 1 ... 64, an axis the grid does not have, an unknown mode, a negative radius, the same and overlapping
    arrays, misaligned arrays; and the good call next to them."""
    valid = S.draw((4, 6), 2, np.float64)
    dev = upload(lib, (4, 6), valid)
    out = sentinel_array(lib, dev)
    w = np.array([0.5, 0.25])
    wp = w.ctypes.data_as(C.POINTER(C.c_double))
    comp_bytes = dev.info.comp_elems * 8
    bad = [(2, None, out.ptr, 0, WRAP, 1, wp), (2, dev.ptr, None, 0, WRAP, 1, wp), (2, dev.ptr, out.ptr, 0, WRAP, 1, None),
           (0, dev.ptr, out.ptr, 0, WRAP, 1, wp), (65, dev.ptr, out.ptr, 0, WRAP, 1, wp), (2, dev.ptr, out.ptr, 2, WRAP, 1, wp),
           (2, dev.ptr, out.ptr, -1, WRAP, 1, wp), (2, dev.ptr, out.ptr, 0, 2, 1, wp), (2, dev.ptr, out.ptr, 0, -1, 1, wp),
           (2, dev.ptr, out.ptr, 0, CELL | 2, 1, wp), (2, dev.ptr, out.ptr, 0, REFLECT, -1, wp), (2, dev.ptr, dev.ptr, 0, WRAP, 1, wp),
           (2, dev.ptr, dev.ptr + comp_bytes, 0, WRAP, 1, wp), (2, dev.ptr + comp_bytes, dev.ptr, 0, WRAP, 1, wp),
           (1, dev.ptr + 8, out.ptr, 0, WRAP, 1, wp), (1, dev.ptr, out.ptr + 8, 0, WRAP, 1, wp)]
    for ncomp, src, dst, axis, mode, radius, weights in bad:
        with pytest.raises(ValueError):
            lib.smooth_axis(dev.info.ref, ncomp, src, dst, axis, mode, radius, weights, None)
        assert lib.last_error()
    # one component into the other of the same array does not overlap
    lib.smooth_axis(dev.info.ref, 1, dev.ptr, dev.ptr + comp_bytes, 1, REFLECT | CELL, 1, wp, None)
    lib.smooth_axis(dev.info.ref, 2, dev.ptr, out.ptr, 0, WRAP, 1, wp, None)


def run_mirror(backend, tracker, dtype=np.float64, shape=(8, 6, 10), periodic=(True, False, True)):
    grid = pde_hip.CartesianGrid([(0.0, 1.5 * n) for n in shape], shape, periodic=list(periodic))
    state = pde_hip.ScalarField(grid, S.draw(shape, 1, dtype, seed=5)[0], label="c")
    return pde_hip.DiffusionPDE(0.5).solve(state, t_range=0.4, dt=0.05, solver="euler", backend=backend, tracker=tracker, interval=0.1)


def resident_run_checks(backend, dtype=np.float64) -> None:
    """Shared with the GPU test.  A diffusion run through the mirror classes whose tracker smooths the resident state: ``device=True`` into
    ``slice_field`` and ``field_statistics``, a host result, and - once - in place; nothing is downloaded or uploaded by any of them, the
    results equal the mirror method on a pulled copy, and the stepper continues from the state smoothed in place."""
    seen, states = [], []

    def tracker(field, t):
        link = field.__dict__.get("_hip_link")
        if link is None or not link.host_stale:
            return
        counters = (link.downloads, link.uploads)
        pulled = pde_hip.ScalarField(field.grid, link.dev_state.get_valid(), label=field.label)      # a side copy: not a download of the field
        address = link.dev_state.ptr
        dev = pde_hip.smooth(field, 2.0, device=True)
        host = pde_hip.smooth(field, 2.0, label="coarse")
        cut = backend.make_slicer(field.grid)(dev, {"z": "mid"})
        stats = pde_hip.field_statistics(dev)
        row = {"pulled": pulled, "dev": dev.get_valid(), "host": host, "cut": cut, "stats": stats}
        if len(seen) == 1:
            assert pde_hip.smooth(field, 1.0, out=field) is field
            row["in_place"] = link.dev_state.get_valid()
        assert (link.downloads, link.uploads) == counters and link.host_stale and link.dev_state.ptr == address
        assert type(field) is not pde_hip.ScalarField
        seen.append(row)
        states.append(link)

    res = run_mirror(backend, tracker, dtype)
    link = res.__dict__["_hip_link"]
    assert link.downloads == 0 and link.uploads == 1 and len(seen) >= 3
    for row in seen:
        pulled = row["pulled"]
        ref = pulled.smooth(2.0, out=pulled.copy())
        assert row["dev"].dtype == ref.data.dtype and np.array_equal(bits(row["dev"]), bits(ref.data))
        assert type(row["host"]) is pde_hip.ScalarField and row["host"].label == "coarse" and np.array_equal(bits(row["host"].data), bits(ref.data))
        assert np.array_equal(bits(row["cut"]), bits(ref.slice({"z": "mid"}).data))
        np.testing.assert_allclose(row["stats"].average, ref.average, rtol=1e-6 if dtype == np.float32 else 1e-13)
        if "in_place" in row:
            assert np.array_equal(bits(row["in_place"]), bits(pulled.smooth(1.0, out=pulled.copy()).data))
    # the same run on the host: smooth the state at the same interrupt, step on
    count = []

    def host_tracker(field, t):
        link = field.__dict__.get("_hip_link")
        if link is None or not link.host_stale:
            return
        if len(count) == 1:
            field.smooth(1.0, out=field)      # (reads and writes `data`: the state comes down and goes up again)
        count.append(t)

    plain = run_mirror(backend, host_tracker, dtype)
    assert np.array_equal(bits(res.data), bits(plain.data))
    assert not np.array_equal(bits(res.data), bits(run_mirror(backend, None, dtype).data))
