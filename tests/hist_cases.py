"""Cases, inputs and numpy restatements for the distribution entry points ``pdehip_histogram`` and ``pdehip_quantile_select``.

Shared by ``tests/test_hist_cpu.py`` (CPU: the C versions of the tests-only shim) and ``tests/test_hip_hist.py`` (GPU: the kernels of
``csrc/pdehip_hist.hip``).  The restatements are written from the semantics in ``include/pdehip.h`` - ``np.searchsorted`` on the edges,
``np.sort`` of the cells that are numbers; the drivers call the entry points through whatever library ``pde_hip._lib`` holds, so the same
checks serve both.  Counts are integers and order statistics are elements of the field: every comparison is for EQUALITY, there is no
tolerance in this file.

Inputs: half of the cells uniform in [-1, 1), half within 0.01 of -0.75 or +0.75 (a two-phase field: most cells in two bins).  The range of
the equal bins is (-0.8, 0.9), so cells fall below and above as well.  Planted: a value exactly on EVERY edge, and NaN / +inf / -inf, in
the first and the last cell, on the wave and workgroup seams and from the middle on (as far as the component has cells).  Ghost cells
and row padding of every device array are poisoned (``stats_cases.upload``).
"""

from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import stats_cases as S

from pde_hip.device import DeviceArray, DeviceBuffer

DTYPES = S.DTYPES
bits = S.bits
upload = S.upload

# (shape, ncomp): rows of 1, 2, 3 cells; extents across the vector-width, wave and workgroup seams (63 / 64 / 65, 127 / 129); 1-D to 3-D;
# 1 / 3 / 9 components; the last fills several workgroups
SMALL = (
    ((1,), 1), ((2,), 3), ((3,), 1), ((63,), 3), ((64,), 1), ((65,), 9), ((127,), 1), ((129,), 3),
    ((3, 1), 1), ((2, 2), 3), ((5, 3), 9), ((3, 64), 1), ((3, 65), 3), ((4, 127), 1),
    ((2, 3, 1), 3), ((3, 2, 4), 1), ((2, 3, 63), 1), ((3, 5, 129), 1), ((17, 9, 64), 3),
)
# beyond the grid-stride turn of a launch: a sweep has at most 2048 workgroups (524 288 pieces; 768 workgroups, 196 608 pieces, with more
# than 1024 counters).  65 x 129 x 63 = 528 255 one-cell pieces (odd rows), x 126: as many fp64 pairs, x 252: as many fp32 quads
TURN_PIECES = 2048 * 256
TURN = {
    "f64x1": ((65, 129, 63), np.float64, 1),
    "f32x1": ((65, 129, 63), np.float32, 1),
    "f64x2": ((65, 129, 126), np.float64, 2),
    "f32x4": ((65, 129, 252), np.float32, 4),
}
BINS = (1, 2, 7, 64, 4096)
RANGE = (-0.8, 0.9)
NONUNIFORM = (-0.9, -0.75, -0.7, -0.1, 0.0, 0.25, 0.3, 0.31, 0.75, 1.5)
QS = (0.0, 1.0, 0.5, 1.0 / 3.0, 0.999)
# (shape, q) of the `method=` tests: numpy takes floor / ceil of (n - 1) * q for "lower" / "higher", the ABI k = floor((n - 1) * q) and
# the next rank unless the product is whole - test_hist_cpu.py checks on the CPU that the two agree for every pair
METHOD_CASES = (((5, 67), (0.0, 0.25, 0.5, 1.0 / 3.0, 0.999, 1.0)), ((64,), (0.1, 0.5, 2.0 / 3.0)), ((3, 5, 9), (0.37, 0.5, 0.75)))

case_id = S.case_id
vec_width = S.vec_width


def draw(shape, ncomp: int, dtype, seed: int = 0) -> np.ndarray:
    """Valid data ``(ncomp, *shape)``: uniform noise and a two-phase part, cell by cell."""
    rng = np.random.default_rng([seed, ncomp, *shape])
    full = (ncomp, *shape)
    uniform = rng.uniform(-1.0, 1.0, full)
    phases = 0.75 * rng.choice([-1.0, 1.0], full) + rng.uniform(-0.01, 0.01, full)
    return np.where(rng.integers(0, 2, full) == 0, uniform, phases).astype(dtype)


def spots(n: int) -> list[int]:
    """Cells to plant in: first, last, the wave / workgroup seams, then from the middle on."""
    first = [s for s in (0, n - 1, 63, 64, 127, 128, 255, 256) if 0 <= s < n]
    rest = [s % n for s in range(n // 2, n // 2 + n)]
    seen, out = set(), []
    for s in first + rest:
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def plant(valid: np.ndarray, edges, nonfinite: bool = True) -> np.ndarray:
    """NaN, +inf, -inf (in turn) and then a value exactly on every edge, in the cells of ``spots``, for every component."""
    out = valid.copy()
    flat = out.reshape(out.shape[0], -1)
    values = ([np.nan, np.inf, -np.inf] if nonfinite else []) + [e for e in np.asarray(edges, dtype=valid.dtype)]
    for c in range(flat.shape[0]):
        for m, at in enumerate(spots(flat.shape[1])[: len(values)]):
            flat[c, at] = values[(m + c) % len(values)]          # (a component with fewer cells than values: another choice for each)
    return out


def equal_edges(nbins: int, dtype) -> np.ndarray:
    """The edges ``np.histogram(a, nbins, RANGE)`` returns for an array of ``dtype`` (fp32 edges for an fp32 array)."""
    return np.histogram(np.zeros(1, dtype=dtype), nbins, RANGE)[1]


def nonuniform_edges(dtype) -> np.ndarray:
    return np.array(NONUNIFORM, dtype=dtype)


# ---- drivers ----------------------------------------------------------------------------------------------------------------------------
def histogram(lib, dev: DeviceArray, edges, *, norm: bool = False, stream=None, keep: list | None = None) -> np.ndarray:
    """The counts as ``(blocks, nbins + 3)`` uint64; the output buffer holds all-ones bits before the call."""
    e64 = np.ascontiguousarray(edges, dtype=np.float64)
    blocks, nbins = (1 if norm else dev.ncomp), e64.size - 1
    edges_dev, out = DeviceBuffer(e64.nbytes), DeviceBuffer(8 * blocks * (nbins + 3))
    lib.memcpy_h2d(edges_dev.ptr, e64.ctypes.data, e64.nbytes, stream)
    lib.memset(out.ptr, 0xFF, out.nbytes, stream)
    lib.histogram(dev.info.ref, dev.ncomp, dev.ptr, int(norm), nbins, edges_dev.ptr, out.ptr, stream)
    if keep is not None:          # the caller reads the result later (two streams)
        keep.append((edges_dev, out, (blocks, nbins + 3)))
        return None
    host = np.empty((blocks, nbins + 3), dtype=np.uint64)
    lib.memcpy_d2h(host.ctypes.data, out.ptr, host.nbytes, stream)
    return host


def select(lib, dev: DeviceArray, q, *, norm: bool = False, stream=None, keep: list | None = None):
    """(lower, upper) as ``(blocks, nq)`` in the field's type and info ``(blocks, 2)`` uint64; the outputs hold all-ones bits before."""
    qs = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
    blocks = 1 if norm else dev.ncomp
    nbytes = blocks * qs.size * dev.itemsize
    bufs = [DeviceBuffer(nbytes), DeviceBuffer(nbytes), DeviceBuffer(16 * blocks)]
    for b in bufs:
        lib.memset(b.ptr, 0xFF, b.nbytes, stream)
    lib.quantile_select(dev.info.ref, dev.ncomp, dev.ptr, int(norm), qs.size, qs.ctypes.data_as(C.POINTER(C.c_double)), bufs[0].ptr,
                        bufs[1].ptr, bufs[2].ptr, stream)
    if keep is not None:
        keep.append((bufs, blocks, qs.size, dev.dtype))
        return None
    return read_select(lib, bufs, blocks, qs.size, dev.dtype, stream)


def read_select(lib, bufs, blocks: int, nq: int, dtype, stream=None):
    lower, upper = np.empty((2, blocks, nq), dtype=dtype)
    info = np.empty((blocks, 2), dtype=np.uint64)
    for host, buf in ((lower, bufs[0]), (upper, bufs[1]), (info, bufs[2])):
        lib.memcpy_d2h(host.ctypes.data, buf.ptr, host.nbytes, stream)
    return lower, upper, info


# ---- restatements -------------------------------------------------------------------------------------------------------------------
np_values = S.np_values


def np_counts(values: np.ndarray, edges) -> np.ndarray:
    """``(blocks, nbins + 3)``: per bin the cells with e[i] <= x < e[i + 1] (the last bin closed), then below, above, NaN; comparisons in
    float64 on exactly converted values."""
    e = np.asarray(edges, dtype=np.float64)
    nbins = e.size - 1
    out = np.zeros((values.shape[0], nbins + 3), dtype=np.uint64)
    for c, row in enumerate(values):
        x = row.astype(np.float64).ravel()
        nan = np.isnan(x)
        v = x[~nan]
        inside = v[(v >= e[0]) & (v <= e[-1])]
        idx = np.searchsorted(e, inside, side="right") - 1
        idx[inside == e[-1]] = nbins - 1
        out[c, :nbins] = np.bincount(idx, minlength=nbins)
        out[c, nbins], out[c, nbins + 1], out[c, nbins + 2] = (v < e[0]).sum(), (v > e[-1]).sum(), nan.sum()
    return out


def np_select(values: np.ndarray, q):
    """(lower, upper, info): the elements of ``np.sort`` of the cells that are numbers at k = floor((n - 1) q) and min(k + 1, n - 1)."""
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    lower, upper = np.full((2, values.shape[0], qs.size), np.nan, dtype=values.dtype)
    info = np.zeros((values.shape[0], 2), dtype=np.uint64)
    for c, row in enumerate(values):
        x = row.ravel()
        s = np.sort(x[~np.isnan(x)])
        info[c] = s.size, x.size - s.size
        if s.size:
            k = np.floor((np.float64(s.size) - 1.0) * qs).astype(np.int64)
            lower[c], upper[c] = s[k], s[np.minimum(k + 1, s.size - 1)]
    return lower, upper, info


def check_counts(got: np.ndarray, values: np.ndarray, edges, what: str = "", numpy_call=None) -> None:
    """Equal to the restatement, every block sums to the number of cells, and the bins equal ``np.histogram``'s own (``numpy_call(x)``)."""
    expect = np_counts(values, edges)
    nbins = expect.shape[1] - 3
    print(f"{what}: bins {nbins}, below/above/nan {got[:, nbins:].tolist()} expect {expect[:, nbins:].tolist()}, largest bin {got[:, :nbins].max()}")
    assert got.shape == expect.shape, f"{what}: {got.shape}"
    np.testing.assert_array_equal(got, expect, err_msg=what)
    cells = math.prod(values.shape[1:])
    assert (got.sum(axis=1) == cells).all(), f"{what}: block sums {got.sum(axis=1)} != {cells} cells"
    if numpy_call is not None:
        with np.errstate(invalid="ignore"):
            for c, row in enumerate(values):
                np.testing.assert_array_equal(got[c, :nbins].astype(np.int64), numpy_call(row.ravel()), err_msg=f"{what}: block {c} against np.histogram")


def same_elements(got: np.ndarray, expect: np.ndarray) -> np.ndarray:
    """Equal bit patterns; zeros compare by value (the sign of a zero result is unspecified), NaN equals NaN."""
    return (bits(got) == bits(expect)) | ((got == 0) & (expect == 0)) | (np.isnan(got) & np.isnan(expect))


def check_select(got, values: np.ndarray, q, what: str = "") -> None:
    lower, upper, info = got
    e_lower, e_upper, e_info = np_select(values, q)
    print(f"{what}: q {np.atleast_1d(q).tolist()} lower {lower.tolist()} upper {upper.tolist()} info {info.tolist()}")
    np.testing.assert_array_equal(info, e_info, err_msg=f"{what}: n / n_nan")
    assert lower.shape == e_lower.shape and upper.shape == e_upper.shape and lower.dtype == values.dtype
    assert same_elements(lower, e_lower).all(), f"{what}: lower {lower} != {e_lower}"
    assert same_elements(upper, e_upper).all(), f"{what}: upper {upper} != {e_upper}"


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_inputs(case, dtype_name: str, nbins: int):
    """Data of a small case with NaN, +-inf and every edge of ``nbins`` equal bins planted (nbins == 0: the non-uniform edges);
    (valid, edges), computed once."""
    shape, ncomp = case
    dtype = np.dtype(dtype_name)
    edges = equal_edges(nbins, dtype) if nbins else nonuniform_edges(dtype)
    valid = plant(draw(shape, ncomp, dtype), edges)
    valid.setflags(write=False)
    return valid, edges


@functools.lru_cache(maxsize=None)
def turn_inputs(key: str):
    shape, dtype, _ = TURN[key]
    valid = plant(draw(shape, 1, dtype, seed=7), equal_edges(64, dtype))
    valid.reshape(-1)[-1] = RANGE[1]          # the last cell, beyond the turn, lies ON the last edge
    valid.setflags(write=False)
    return valid


def select_fields(dtype) -> dict[str, np.ndarray]:
    """Fields ``(1, 5, 67)`` for the selection: ties (every digit count in one bucket, ranks inside runs of duplicates), signs, the ends of
    the number line, one number, none."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(3)
    shape = (1, 5, 67)
    n = math.prod(shape)
    tiny = np.finfo(dtype).smallest_subnormal
    ends = np.resize(np.array([np.inf, -np.inf, tiny, -tiny, 3 * tiny, 0.0, -0.0, np.finfo(dtype).max, np.finfo(dtype).tiny, 1.0, -1.0], dtype=dtype), n)
    one = np.full(n, np.nan, dtype=dtype)
    one[n // 2] = -2.5
    out = {
        "all_equal": np.full(n, 0.3, dtype=dtype),
        "two_valued": np.where(rng.integers(0, 3, n) == 0, -0.75, 0.75).astype(dtype),
        "runs": rng.integers(-2, 3, n).astype(dtype),
        "all_negative": (-rng.uniform(1e-3, 1e3, n)).astype(dtype),
        "ends": rng.permutation(ends),
        "neighbours": np.nextafter(dtype.type(1.0), dtype.type(2.0)) * np.ones(n, dtype=dtype) - (rng.integers(0, 2, n) * np.finfo(dtype).eps).astype(dtype),
        "one_number": one,
        "none": np.full(n, np.nan, dtype=dtype),
    }
    return {k: v.reshape(shape) for k, v in out.items()}


# ---- the checks both test files run -----------------------------------------------------------------------------------------------------
def run_histogram_case(lib, case, dtype) -> None:
    """Equal bins over RANGE for every count in BINS and the non-uniform edges: per component and of the norm, NaN, +-inf and every edge
    planted; two calls give equal bits."""
    shape, _ = case
    for nbins in (*BINS, 0):
        valid, edges = small_inputs(case, np.dtype(dtype).name, nbins)
        call = (lambda x, nbins=nbins: np.histogram(x, nbins, RANGE)[0]) if nbins else (lambda x, edges=edges: np.histogram(x, edges)[0])
        if nbins:
            np.testing.assert_array_equal(np.histogram(valid[0], nbins, RANGE)[1], edges)
        dev = upload(lib, shape, valid)
        got = histogram(lib, dev, edges)
        check_counts(got, valid, edges, f"bins={nbins}", call)
        np.testing.assert_array_equal(got, histogram(lib, upload(lib, shape, valid), edges), err_msg="two runs differ")
        check_counts(histogram(lib, dev, edges, norm=True), np_values(valid, True), edges, f"norm bins={nbins}", call)


def run_select_case(lib, case, dtype) -> None:
    """Every q of QS alone and all five at once, per component and of the norm, NaN and +-inf planted; two calls give equal bits."""
    shape, _ = case
    valid, _ = small_inputs(case, np.dtype(dtype).name, 7)
    dev = upload(lib, shape, valid)
    for q in (*QS, QS):
        got = select(lib, dev, q)
        check_select(got, valid, q, f"q={q}")
    again = select(lib, upload(lib, shape, valid), QS)
    for a, b in zip(got, again):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg="two runs differ")
    check_select(select(lib, dev, QS, norm=True), np_values(valid, True), QS, "norm")


def run_refusals(lib) -> None:
    import pytest

    valid = draw((4, 4), 1, np.float64)
    dev = upload(lib, (4, 4), valid)
    edges = np.linspace(-1.0, 1.0, 5)
    e_dev, out = DeviceBuffer(8 * 4100), DeviceBuffer(8 * 4200)
    lib.memcpy_h2d(e_dev.ptr, edges.ctypes.data, edges.nbytes, None)
    ref = dev.info.ref
    lib.histogram(ref, 1, dev.ptr, 0, 4, e_dev.ptr, out.ptr, None)
    for args in ((ref, 1, None, 0, 4, e_dev.ptr, out.ptr), (ref, 1, dev.ptr, 0, 4, None, out.ptr), (ref, 1, dev.ptr, 0, 4, e_dev.ptr, None),
                 (ref, 0, dev.ptr, 0, 4, e_dev.ptr, out.ptr), (ref, 65, dev.ptr, 0, 4, e_dev.ptr, out.ptr),
                 (ref, 1, dev.ptr, 0, 0, e_dev.ptr, out.ptr), (ref, 1, dev.ptr, 0, 4097, e_dev.ptr, out.ptr),
                 (ref, 1, dev.ptr + 8, 0, 4, e_dev.ptr, out.ptr), (ref, 1, dev.ptr, 0, 4, e_dev.ptr + 4, out.ptr)):
        with pytest.raises(ValueError):
            lib.histogram(*args, None)
    for bad in ([-1.0, 0.0, 0.0, 0.5, 1.0], [-1.0, 0.5, 0.0, 0.75, 1.0], [-1.0, 0.0, np.nan, 0.5, 1.0], [-np.inf, 0.0, 0.25, 0.5, 1.0],
                [-1.0, 0.0, 0.25, 0.5, np.inf]):
        e = np.array(bad)
        lib.memcpy_h2d(e_dev.ptr, e.ctypes.data, e.nbytes, None)
        with pytest.raises(ValueError):
            lib.histogram(ref, 1, dev.ptr, 0, 4, e_dev.ptr, out.ptr, None)
    q = (C.c_double * 9)(*([0.5] * 9))
    lo, up, info = DeviceBuffer(128), DeviceBuffer(128), DeviceBuffer(16)
    lib.quantile_select(ref, 1, dev.ptr, 0, 1, q, lo.ptr, up.ptr, info.ptr, None)
    for args in ((ref, 1, None, 0, 1, q, lo.ptr, up.ptr, info.ptr), (ref, 1, dev.ptr, 0, 1, None, lo.ptr, up.ptr, info.ptr),
                 (ref, 1, dev.ptr, 0, 1, q, None, up.ptr, info.ptr), (ref, 1, dev.ptr, 0, 1, q, lo.ptr, None, info.ptr),
                 (ref, 1, dev.ptr, 0, 1, q, lo.ptr, up.ptr, None), (ref, 0, dev.ptr, 0, 1, q, lo.ptr, up.ptr, info.ptr),
                 (ref, 65, dev.ptr, 0, 1, q, lo.ptr, up.ptr, info.ptr), (ref, 1, dev.ptr, 0, 0, q, lo.ptr, up.ptr, info.ptr),
                 (ref, 1, dev.ptr, 0, 9, q, lo.ptr, up.ptr, info.ptr), (ref, 1, dev.ptr + 8, 0, 1, q, lo.ptr, up.ptr, info.ptr),
                 (ref, 1, dev.ptr, 0, 1, q, lo.ptr + 4, up.ptr, info.ptr)):
        with pytest.raises(ValueError):
            lib.quantile_select(*args, None)
    for bad in (-0.1, 1.5, np.nan):
        with pytest.raises(ValueError):
            lib.quantile_select(ref, 1, dev.ptr, 0, 1, (C.c_double * 1)(bad), lo.ptr, up.ptr, info.ptr, None)
