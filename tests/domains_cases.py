"""Reference, inputs and checks for the domain entry points ``pdehip_label_domains`` and ``pdehip_domain_sizes``.

Shared by ``tests/test_domains_cpu.py`` (CPU: the sequential C versions of the tests-only shim) and ``tests/test_hip_domains.py`` (GPU:
the kernels of ``csrc/pdehip_label.hip``).  The drivers call the entry points through whatever library ``pde_hip._lib`` holds, so the same
checks serve both.  A labelling is all integers: every comparison is ``assert_array_equal``, there is no tolerance in this file.

``reference(mask, periodic, connectivity)``: ``scipy.ndimage.label`` with ``generate_binary_structure``, a host union of the labels that
touch through a periodic wrap (faces; edges and corners too under full connectivity), renumbering by first cell, ``np.bincount`` for the
sizes.  It is written apart from the host path of ``pde_hip/domains.py`` (every offset on the whole array instead of boundary layers).

Shapes, with T = TILE = (4, 8, 32) the tile of the tile kernel: one cell, rows shorter and longer than a tile, one cell more than a
tile on every axis, two tiles and a cell with one axis a cell short of a tile.  The labelling kernels take one tile per workgroup, one
cell per thread or one chunk per workgroup, without a loop over turns; ``domain_sizes_kernel`` IS grid-stride (at most 4096 workgroups):
``TURN_SHAPE`` and ``run_sizes_beyond_the_turn`` lie beyond its turn, where a wave carries the label it holds from one turn to the next
or has to hand it in.  Ghost cells and row padding of every device array are poisoned.

Conditions that keep the checks from being vacuous are asserted on the reference in ``check_conditions`` (no GPU needed), for every
random mask: a domain with cells in two tiles wherever the shape has two tiles, at every p and both connectivities; K >= 2 and fewer
domains with the periodic wrap than without (every periodic pattern) at every p under connectivity 1, and at p = 0.3, the ragged regime
below the 3-D site-percolation threshold, under full connectivity too; at p = 0.7 in 3-D one domain that holds most of the foreground.
The one thing left out cannot hold: under full connectivity a mask at p = 0.5 or 0.7 is ONE domain with or without the wrap (an isolated
cell needs 26 background neighbours, probability 0.5^26), so K >= 2 and K_periodic < K are not asked there.  The seeds are picked so
that all of this holds at every shape (``SEEDS``).
"""

from __future__ import annotations

import ctypes as C
import functools
import itertools
import math

import numpy as np
import stats_cases as S
from scipy import ndimage

from pde_hip.device import DeviceArray, DeviceBuffer
from pde_hip.domains import interval_bounds

DTYPES = S.DTYPES
TILE = (4, 8, 32)
T0, T1, T2 = TILE
SHAPES = (
    (1,), (3,), (130,),
    (5, 9), (T1 + 1, 2 * T2 + 1),
    (4, 6, 8), (17, 9, 64), (T0 + 1, T1 + 1, T2 + 1), (2 * T0 + 1, T1 - 1, 2 * T2 + 1),
)
PS = (0.3, 0.5, 0.7)
# seeds of the random masks, per (shape, p), where seed 0 does not meet check_conditions (the smallest seed that does)
SEEDS: dict = {((130,), 0.3): 5, ((130,), 0.5): 8, ((130,), 0.7): 2, ((5, 9), 0.3): 2, ((5, 9), 0.5): 1, ((4, 6, 8), 0.7): 1}
# beyond the grid-stride turn of `domain_sizes_kernel`, the one launch with a loop over turns: at most 4096 workgroups of 256 threads, so
# with 64 x 128 x 160 = 1 310 720 cells the first 1024 workgroups take a second turn
TURN_CELLS = 4096 * 256
TURN_SHAPE = (64, 128, 160)


def shape_id(shape) -> str:
    return "x".join(map(str, shape))


def connectivities(ndim: int):
    return (1,) if ndim == 1 else (1, ndim)


def periodic_patterns(ndim: int):
    """None, all, and one mixed pattern (1-D has only two)."""
    out = [(False,) * ndim, (True,) * ndim]
    if ndim == 2:
        out.append((True, False))
    if ndim == 3:
        out.append((True, False, True))
    return out


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def reference(mask: np.ndarray, periodic, connectivity: int):
    """(labels int32, K, foreground, sizes int64)."""
    mask = np.asarray(mask, dtype=bool)
    ndim = mask.ndim
    labels, count = ndimage.label(mask, structure=ndimage.generate_binary_structure(ndim, connectivity))
    parent = list(range(count + 1))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    if count and any(periodic):
        index = np.indices(mask.shape)
        for d in itertools.product((-1, 0, 1), repeat=ndim):
            steps = sum(1 for x in d if x)
            if steps == 0 or (connectivity == 1 and steps > 1):
                continue
            ok = np.ones(mask.shape, dtype=bool)
            where = []
            for a in range(ndim):
                q = index[a] + d[a]
                if not periodic[a]:
                    ok &= (q >= 0) & (q < mask.shape[a])
                where.append(q % mask.shape[a])
            other = labels[tuple(where)]
            touch = ok & (labels > 0) & (other > 0) & (labels != other)
            for x, y in set(zip(labels[touch].tolist(), other[touch].tolist())):
                rx, ry = find(x), find(y)
                if rx != ry:
                    parent[max(rx, ry)] = min(rx, ry)
    merged = np.array([find(x) for x in range(count + 1)], dtype=np.int64)[labels]
    # numbering by first cell, whatever numbering came in
    flat = merged.ravel()
    values, first = np.unique(flat, return_index=True)
    keep = values > 0
    values, first = values[keep], first[keep]
    order = np.argsort(first)
    remap = np.zeros(count + 1, dtype=np.int64)
    remap[values[order]] = np.arange(1, values.size + 1)
    out = remap[merged].astype(np.int32)
    k = int(values.size)
    return out, k, int(mask.sum()), np.bincount(out.ravel(), minlength=k + 1)[1:].astype(np.int64)


def tiles_of(labels: np.ndarray) -> np.ndarray:
    """The linear tile number of every cell (normalised to three axes like the kernels do)."""
    shape3 = (1,) * (3 - labels.ndim) + labels.shape
    idx = np.indices(shape3)
    return ((idx[0] // T0) * 10000 + idx[1] // T1) * 10000 + idx[2] // T2


def spans_two_tiles(labels: np.ndarray) -> bool:
    tiles = tiles_of(labels).ravel()
    flat = labels.ravel()
    for lab in range(1, int(flat.max()) + 1):
        if np.unique(tiles[flat == lab]).size > 1:
            return True
    return False


# ---- masks --------------------------------------------------------------------------------------------------------------------------------
def random_mask(shape, p: float) -> np.ndarray:
    rng = np.random.default_rng([SEEDS.get((tuple(shape), p), 0), int(p * 10), *shape])
    return rng.random(shape) < p


def serpentine(shape) -> np.ndarray:
    """A one-cell-wide path through every tile: full rows 0, 2, 4, ... joined at alternating ends; in 3-D on the even planes, which one
    cell at the origin of every odd plane joins."""
    def plane(n1, n2):
        m = np.zeros((n1, n2), dtype=bool)
        m[0::2] = True
        for turn, row in enumerate(range(1, n1 - 1, 2)):
            m[row, n2 - 1 if turn % 2 == 0 else 0] = True
        return m

    if len(shape) == 1:
        return np.ones(shape, dtype=bool)
    if len(shape) == 2:
        return plane(*shape)
    m = np.zeros(shape, dtype=bool)
    m[0::2] = plane(*shape[1:])
    m[1:shape[0] - 1:2, 0, 0] = True
    return m


def diagonal(shape) -> np.ndarray:
    """Cells that touch only diagonally: the main diagonal, and two cells either side of the corner where tiles meet on every axis."""
    m = np.zeros(shape, dtype=bool)
    for i in range(min(shape)):
        m[(i,) * len(shape)] = True
    corner = (T0, T1, T2)[3 - len(shape):]
    if all(c < n for c, n in zip(corner, shape)):
        m[corner] = True
        m[tuple(c - 1 for c in corner)] = True
    return m


def fixed_masks(shape) -> dict:
    idx = np.indices(shape)
    stripes = np.zeros(shape, dtype=bool)
    stripes[..., 0] = True
    stripes[..., -1] = True
    return {
        "all": np.ones(shape, dtype=bool),
        "none": np.zeros(shape, dtype=bool),
        "checkerboard": idx.sum(axis=0) % 2 == 0,
        "serpentine": serpentine(shape),
        "diagonal": diagonal(shape),
        "stripes": stripes,
    }


def masks_of(shape) -> dict:
    """Every mask of a shape by name; the two smallest shapes take ALL their masks instead of random ones."""
    out = fixed_masks(shape)
    cells = math.prod(shape)
    if cells <= 3:
        for bits in range(2 ** cells):
            out[f"bits{bits}"] = np.array([(bits >> c) & 1 for c in range(cells)], dtype=bool).reshape(shape)
    else:
        for p in PS:
            out[f"p{p}"] = random_mask(shape, p)
    return out


def field_of(mask: np.ndarray, dtype, seed: int = 1) -> np.ndarray:
    """A field whose cells above 0 are the mask: foreground in [0.25, 1], background in [-1, -0.25]."""
    rng = np.random.default_rng([seed, *mask.shape])
    mag = rng.uniform(0.25, 1.0, mask.shape)
    return np.where(mask, mag, -mag).astype(dtype)


@functools.lru_cache(maxsize=None)
def expected(shape, name: str, periodic, connectivity: int):
    """The reference of a named mask, computed once and shared (read-only)."""
    out = reference(masks_of(shape)[name], periodic, connectivity)
    out[0].setflags(write=False)
    out[3].setflags(write=False)
    return out


def check_conditions(shape) -> None:
    """The conditions of the module docstring, on the reference alone."""
    if math.prod(shape) <= 3:
        return
    ndim = len(shape)
    two_tiles = any(n > t for n, t in zip((1,) * (3 - ndim) + tuple(shape), TILE))
    open_ = (False,) * ndim
    for conn in connectivities(ndim):
        for p in PS:
            labels, k, fg, sizes = expected(shape, f"p{p}", open_, conn)
            assert k >= 1 and fg > 0, (shape, p, conn)
            if two_tiles:
                assert spans_two_tiles(labels), (shape, p, conn)
            if p == 0.7 and ndim == 3:
                assert sizes.max() > fg // 2, (shape, conn, sizes.max(), fg)
            if conn == 1 or p == 0.3:
                assert k >= 2, (shape, p, conn, k)
                for per in periodic_patterns(ndim)[1:]:
                    k_per = expected(shape, f"p{p}", per, conn)[1]
                    assert k_per < k, (shape, p, conn, per, k_per, k)


# ---- drivers ------------------------------------------------------------------------------------------------------------------------------
def upload(lib, data: np.ndarray) -> DeviceArray:
    """One component on the device; ghost cells, row padding and slack are poisoned."""
    return S.upload(lib, data.shape, np.ascontiguousarray(data)[None])


def label(lib, dev: DeviceArray, lo: float, hi: float, connectivity: int, periodic, *, stream=None, keep: list | None = None):
    """(labels int32 of the grid's shape, info uint64[2], the label buffer); both outputs hold all-ones bits before the call."""
    shape = dev.info.shape
    cells = math.prod(shape)
    labels_dev, info_dev = DeviceBuffer(4 * cells), DeviceBuffer(16)
    lib.memset(labels_dev.ptr, 0xFF, 4 * cells, stream)
    lib.memset(info_dev.ptr, 0xFF, 16, stream)
    per = (C.c_int * len(shape))(*[int(p) for p in periodic])
    lib.label_domains(dev.info.ref, dev.ptr, C.c_double(lo), C.c_double(hi), connectivity, per, labels_dev.ptr, info_dev.ptr, stream)
    if keep is not None:          # the caller reads later (two streams)
        keep.append((labels_dev, info_dev, shape))
        return None
    return read_label(lib, labels_dev, info_dev, shape, stream)


def read_label(lib, labels_dev, info_dev, shape, stream=None):
    labels, info = np.empty(shape, dtype=np.int32), np.empty(2, dtype=np.uint64)
    lib.memcpy_d2h(labels.ctypes.data, labels_dev.ptr, labels.nbytes, stream)
    lib.memcpy_d2h(info.ctypes.data, info_dev.ptr, 16, stream)
    return labels, info, labels_dev


def sizes(lib, labels_dev, cells: int, ndomains: int, stream=None) -> np.ndarray:
    """``ndomains`` sizes; the slot behind them must keep its all-ones bits (ndomains == 0: nothing is written at all)."""
    out = DeviceBuffer(8 * (ndomains + 1))
    lib.memset(out.ptr, 0xFF, out.nbytes, stream)
    lib.domain_sizes(labels_dev.ptr, cells, ndomains, out.ptr, stream)
    host = np.empty(ndomains + 1, dtype=np.uint64)
    lib.memcpy_d2h(host.ctypes.data, out.ptr, host.nbytes, stream)
    assert host[-1] == np.uint64(2 ** 64 - 1), f"domain_sizes wrote behind its {ndomains} sizes: {host[-1]}"
    return host[:-1].astype(np.int64)


def check(lib, data: np.ndarray, lo: float, hi: float, connectivity: int, periodic, expect, what: str = ""):
    """Labels, K, the foreground count and the sizes equal the reference's; returns what the library gave."""
    e_labels, e_k, e_fg, e_sizes = expect
    labels, info, labels_dev = label(lib, upload(lib, data), lo, hi, connectivity, periodic)
    print(f"{what}: K {int(info[0])} expect {e_k}, foreground {int(info[1])} expect {e_fg}")
    np.testing.assert_array_equal(info, np.array([e_k, e_fg], dtype=np.uint64), err_msg=f"{what}: K, foreground")
    np.testing.assert_array_equal(labels, e_labels, err_msg=f"{what}: labels")
    got_sizes = sizes(lib, labels_dev, labels.size, e_k)
    np.testing.assert_array_equal(got_sizes, e_sizes, err_msg=f"{what}: sizes")
    return labels, info, got_sizes


# ---- the checks both test files run ---------------------------------------------------------------------------------------------------
def run_shape(lib, shape, dtype) -> None:
    """Every mask of the shape at both connectivities and the three periodic patterns."""
    ndim = len(shape)
    lo, hi = interval_bounds(dtype, 0.0)
    for name, mask in masks_of(shape).items():
        data = field_of(mask, dtype)
        for conn in connectivities(ndim):
            for per in periodic_patterns(ndim):
                check(lib, data, lo, hi, conn, per, expected(shape, name, per, conn), f"{shape_id(shape)} {name} c{conn} {per}")


def run_special_values(lib, shape, dtype) -> None:
    """NaN and +-inf cells under ``interval=(a, inf)``, and a threshold that equals cell values: ``>`` against the closed interval."""
    rng = np.random.default_rng([5, *shape])
    ndim = len(shape)
    data = rng.normal(size=shape).astype(dtype)
    flat = data.reshape(-1)
    for m, at in enumerate(plant_spots(flat.size)):
        flat[at] = (np.nan, np.inf, -np.inf)[m % 3]
    a = dtype(0.1)
    with np.errstate(invalid="ignore"):
        mask = data >= a
    assert mask.any() and np.isinf(data[mask]).any() and np.isnan(data).any()
    for per in periodic_patterns(ndim)[:2]:
        for conn in connectivities(ndim):
            check(lib, data, *interval_bounds(dtype, interval=(a, np.inf)), conn, per, reference(mask, per, conn), f"nonfinite c{conn} {per}")
    # values -1, 0, 1, and third steps that fp32 and fp64 round differently
    third = dtype(1.0) / dtype(3.0)
    data = (rng.integers(-1, 2, shape) * third).astype(dtype)
    per, conn = (False,) * ndim, 1
    for t, above in ((0.0, True), (0.0, False), (float(third), True), (1.0 / 3.0, True), (1.0 / 3.0, False)):
        mask = data > t if above else data < t          # numpy compares an fp32 array with a Python float in fp32
        check(lib, data, *interval_bounds(dtype, t, above), conn, per, reference(mask, per, conn), f"threshold {t} above={above}")
    mask = (data >= 0.0) & (data <= third)
    check(lib, data, *interval_bounds(dtype, interval=(0.0, third)), conn, per, reference(mask, per, conn), "closed interval")


@functools.lru_cache(maxsize=None)
def turn_case(name: str):
    """(mask, reference) beyond the turn, open boundaries, connectivity 1: "smoothed" - a Gaussian-smoothed random field above 0, few
    large domains, so that waves meet the label they hold again a turn later - and "ragged" - white noise at p = 0.3, where they do not."""
    rng = np.random.default_rng(11)
    if name == "smoothed":
        mask = ndimage.gaussian_filter(rng.standard_normal(TURN_SHAPE), 3.0) > 0.0
    else:
        mask = rng.random(TURN_SHAPE) < 0.3
    assert mask.size > TURN_CELLS
    expect = reference(mask, (False,) * 3, 1)
    flat = expect[0].ravel()
    again = np.count_nonzero((flat[:-TURN_CELLS] == flat[TURN_CELLS:]) & (flat[TURN_CELLS:] > 0))
    other = np.count_nonzero((flat[:-TURN_CELLS] != flat[TURN_CELLS:]) & (flat[:-TURN_CELLS] > 0) & (flat[TURN_CELLS:] > 0))
    # a turn later the same thread meets the same label (carried) / another one (handed in): both kinds must occur in their case
    assert (again > 50000) if name == "smoothed" else (other > 10000 and expect[1] > 10000), (name, again, other, expect[1])
    mask.setflags(write=False)
    return mask, expect


def run_turn_case(lib, name: str, dtype) -> None:
    mask, expect = turn_case(name)
    check(lib, field_of(mask, dtype), *interval_bounds(dtype, 0.0), 1, (False,) * 3, expect, f"beyond the turn, {name}")


def run_sizes_beyond_the_turn(lib) -> None:
    """``pdehip_domain_sizes`` alone on hand-made labels of three turns and a bit: one label over a turn and a half, a label per turn, runs
    of 1 to 300 cells, noise over 1000 labels, background in between; against ``np.bincount``."""
    rng = np.random.default_rng(13)
    n, k = 3 * TURN_CELLS + 1000, 1000
    one = np.ones(n, dtype=np.int32)
    one[TURN_CELLS + TURN_CELLS // 2:] = 0
    per_turn = (2 + np.arange(n) // TURN_CELLS).astype(np.int32)
    runs = np.repeat(rng.integers(0, k + 1, n // 100), rng.integers(1, 301, n // 100))[:n].astype(np.int32)
    noise = rng.integers(0, k + 1, n).astype(np.int32)
    mixed = np.where(np.arange(n) % (2 * TURN_CELLS) < TURN_CELLS, 7, noise).astype(np.int32)
    for what, host in (("one label", one), ("a label per turn", per_turn), ("runs", runs), ("noise", noise), ("mixed", mixed)):
        assert host.size == n
        buf = DeviceBuffer(host.nbytes)
        lib.memcpy_h2d(buf.ptr, host.ctypes.data, host.nbytes, None)
        got = sizes(lib, buf, n, k)
        np.testing.assert_array_equal(got, np.bincount(host, minlength=k + 1)[1:], err_msg=what)


def plant_spots(n: int) -> list[int]:
    return sorted({s for s in (0, n - 1, 63, 64, 255, 256, n // 2, n // 3) if 0 <= s < n})


def run_refusals(lib) -> None:
    import pytest

    data = field_of(random_mask((4, 6), 0.5), np.float64)
    dev = upload(lib, data)
    ref = dev.info.ref
    labels, info = DeviceBuffer(4 * 24 + 16), DeviceBuffer(32)
    per = (C.c_int * 2)(0, 0)
    d = C.c_double
    lib.label_domains(ref, dev.ptr, d(0.0), d(np.inf), 1, per, labels.ptr, info.ptr, None)
    lib.label_domains(ref, dev.ptr, d(-np.inf), d(np.inf), 2, per, labels.ptr, info.ptr, None)
    lib.label_domains(ref, dev.ptr, d(0.5), d(0.5), 2, per, labels.ptr, info.ptr, None)
    for args in ((ref, None, d(0.0), d(1.0), 1, per, labels.ptr, info.ptr), (ref, dev.ptr, d(0.0), d(1.0), 1, None, labels.ptr, info.ptr),
                 (ref, dev.ptr, d(0.0), d(1.0), 1, per, None, info.ptr), (ref, dev.ptr, d(0.0), d(1.0), 1, per, labels.ptr, None),
                 (ref, dev.ptr, d(1.0), d(0.0), 1, per, labels.ptr, info.ptr), (ref, dev.ptr, d(np.nan), d(1.0), 1, per, labels.ptr, info.ptr),
                 (ref, dev.ptr, d(0.0), d(np.nan), 1, per, labels.ptr, info.ptr), (ref, dev.ptr, d(0.0), d(1.0), 0, per, labels.ptr, info.ptr),
                 (ref, dev.ptr, d(0.0), d(1.0), 3, per, labels.ptr, info.ptr), (ref, dev.ptr + 8, d(0.0), d(1.0), 1, per, labels.ptr, info.ptr),
                 (ref, dev.ptr, d(0.0), d(1.0), 1, per, labels.ptr + 2, info.ptr), (ref, dev.ptr, d(0.0), d(1.0), 1, per, labels.ptr, info.ptr + 4)):
        with pytest.raises(ValueError):
            lib.label_domains(*args, None)
    # more than 2^31 - 1 cells is refused before anything is touched
    from pde_hip import _abi

    huge = _abi.make_grid((2048, 1024, 1024), (1.0,) * 3, np.float64)
    with pytest.raises(ValueError, match="2\\^31"):
        lib.label_domains(C.byref(huge), dev.ptr, d(0.0), d(1.0), 1, (C.c_int * 3)(0, 0, 0), labels.ptr, info.ptr, None)
    lib.label_domains(ref, dev.ptr, d(0.0), d(np.inf), 1, per, labels.ptr, info.ptr, None)
    out = DeviceBuffer(8 * 32)
    for args in ((None, 24, 3, out.ptr), (labels.ptr, 24, 3, None), (labels.ptr, 0, 3, out.ptr), (labels.ptr, 24, -1, out.ptr),
                 (labels.ptr, 24, 2 ** 31, out.ptr), (labels.ptr + 2, 24, 3, out.ptr), (labels.ptr, 24, 3, out.ptr + 4)):
        with pytest.raises(ValueError):
            lib.domain_sizes(*args, None)


def run_labels_above_ndomains(lib) -> None:
    """Labels above ``ndomains`` (and below 0) are refused by count and never used as an index: the slots behind the sizes keep their bits."""
    import pytest

    host = np.array([0, 1, 2, 2, 7, 3, 1, -5, 2 ** 31 - 1, 0, 3, 3], dtype=np.int32)
    labels = DeviceBuffer(host.nbytes)
    lib.memcpy_h2d(labels.ptr, host.ctypes.data, host.nbytes, None)
    out = DeviceBuffer(8 * 8)
    lib.memset(out.ptr, 0xFF, out.nbytes, None)
    with pytest.raises(ValueError):
        lib.domain_sizes(labels.ptr, host.size, 3, out.ptr, None)
    got = np.empty(8, dtype=np.uint64)
    lib.memcpy_d2h(got.ctypes.data, out.ptr, got.nbytes, None)
    np.testing.assert_array_equal(got[:3], [2, 2, 3])
    assert (got[3:] == np.uint64(2 ** 64 - 1)).all(), got
    # the same labels are fine when they are in range
    lib.domain_sizes(labels.ptr, 4, 2, out.ptr, None)
    lib.memcpy_d2h(got.ctypes.data, out.ptr, got.nbytes, None)
    np.testing.assert_array_equal(got[:2], [1, 2])
