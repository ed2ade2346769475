"""Device tests of the pointwise and reduction kernels of ``csrc/pdehip_ops.hip``, below the stepper level.

``pdehip_lincomb``, ``pdehip_rk4_combine``, ``pdehip_ab2_combine``, ``pdehip_rkf45_combine``,
``pdehip_euler_adaptive_combine``, ``pdehip_max_abs_diff``, ``pdehip_max_abs_pairs``, ``pdehip_integrate`` and
``pdehip_count_nonfinite`` are called through the C ABI.  The steppers fuse these combinations into their last stage
sweep wherever an instance carries them, so a stepper test says little about the kernels here.

References, both bit for bit: the oracle twin and the plain numpy restatement of ``tests/pointwise_cases.py``
(float64, left to right, rounded once); ``tests/test_oracle_pointwise.py`` ties the two to each other on the CPU.
``pdehip_integrate`` sums in another order than any host loop and is compared with ``math.fsum`` inside a bound derived
from the kernels (`test_integrate`).

``max_abs_pairs`` takes the modulus with the device library's ``hypot``, the oracle with the host's: no libm promises a
correctly rounded one, so its data are pairs whose modulus is exact (``P.pair_fields``).

Launch paths: PDEHIP_VEC_LAUNCH takes fp64 pairs (``n2 % 2 == 0``), fp64 cells, fp32 quads (``n2 % 4 == 0``) or fp32
cells; a launch is capped at 16 384 workgroups, so a thread takes a second item only beyond 4 194 304 items
(``P.TURN``: one case per kernel and path whose deciding cell lies beyond that turn).  ``pdehip_integrate`` and
``pdehip_count_nonfinite`` cap at 1024 workgroups: 64 x 64 x 64 is exactly one cell per thread, 65 x 64 x 65 turns.
"""

from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import pointwise_cases as P

import pde_hip
from oracle import pde_oracle as O
from pde_hip.device import DeviceArray, DeviceBuffer, DeviceScalar, GridInfo, ptr_array

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
COEFS = [0.25, -1.5, 3.0, 1 / 3, -0.7, 1e-3]
DT = 0.37
COMBINES = ["lincomb", "rk4_combine", "ab2_combine", "rkf45_combine", "euler_adaptive_combine"]
NORMS = ["rkf45_combine", "euler_adaptive_combine", "max_abs_diff", "max_abs_pairs"]
NEG_NAN = np.copysign(np.nan, -1)


@pytest.fixture(scope="module")
def lib():
    return pde_hip.get_backend("hip")._lib


class Dev:
    """One grid on the device: uploads of full host arrays (ghost cells included) and the error cell."""

    def __init__(self, lib, shape, dtype):
        self.lib, self.shape, self.dtype = lib, tuple(shape), np.dtype(dtype)
        self.info = GridInfo(shape, (1.0,) * len(shape), dtype)
        self.g = self.info.c            # the same struct serves the oracle
        self.inner = P.interior(shape)
        self.err = DeviceScalar()

    def up(self, full):
        return DeviceArray(self.info, (full.shape[0],)).set_hostfull(full)

    def norm(self, call):
        """Run ``call(err_ptr)`` with the error cell holding 1e300 and once more holding a NaN of the largest bit pattern: the
        entry point has to clear the cell, and two runs give equal bits.  Returns the bits of the result."""
        seen = []
        for prefill in (np.float64(1e300).view(np.uint64), np.uint64(0xFFFFFFFFFFFFFFFF)):
            host = C.c_uint64(int(prefill))
            self.lib.memcpy_h2d(self.err.ptr, C.addressof(host), 8, None)
            call(self.err.ptr)
            seen.append(P.f64_bits(self.err.value()))
        assert seen[0] == seen[1], f"two runs differ: {seen[0]:#x} {seen[1]:#x}"
        return seen[0]


def _same(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    bad = P.bits(got) != P.bits(ref)
    if bad.any():
        at = tuple(int(x) for x in np.argwhere(bad)[0])
        with np.errstate(invalid="ignore"):
            off = np.nanmax(np.abs(got.astype(np.float64) - ref.astype(np.float64))[bad])
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} cells differ, first at {at}: {got[at]!r} != {ref[at]!r}, largest difference {off:.3e}")


def _expect(before, ref, inner):
    """The full array a kernel must leave: the reference on the interior, every ghost cell as uploaded."""
    out = before.copy()
    out[inner] = ref[inner]
    return out


def _run_combine(d, kernel, ncomp, arrs, alias=None):
    """Run one combine kernel on the device, its oracle twin and its numpy restatement.

    Returns ``(device full array, [oracle full, numpy full], device error bits or None, [oracle error, numpy error])``; the
    expected arrays keep the uploaded ghost cells."""
    y, k1, k2, k3, k4, k5, k6 = arrs
    lib, g, inner = d.lib, d.g, d.inner
    if kernel == "lincomb":
        ks = [k1, k2, k3]
        out0 = k6
        dy, dks, dout = d.up(y), [d.up(k) for k in ks], d.up(out0)
        lib.lincomb(d.info.ref, ncomp, dout.ptr, dy.ptr, 3, (C.c_double * 3)(*COEFS[:3]), ptr_array(dks), None)
        refs = [O.lincomb(g, ncomp, y, COEFS[:3], ks), P.np_lincomb(y, COEFS[:3], ks)]
        return dout.get_hostfull(), [_expect(out0, r, inner) for r in refs], None, None
    if kernel == "rk4_combine":
        dy, dks = d.up(y), [d.up(k) for k in (k1, k2, k3, k4)]   # (named: a device array lives as long as its Python object)
        lib.rk4_combine(d.info.ref, ncomp, dy.ptr, *[k.ptr for k in dks], None)
        refs = [O.rk4_combine(g, ncomp, y.copy(), k1, k2, k3, k4), P.np_rk4(y, k1, k2, k3, k4)]
        return dy.get_hostfull(), [_expect(y, r, inner) for r in refs], None, None
    if kernel == "ab2_combine":
        dy, drc, drp = d.up(y), d.up(k1), d.up(k2)
        lib.ab2_combine(d.info.ref, ncomp, dy.ptr, drc.ptr, drp.ptr, DT, None)
        refs = [O.ab2_combine(g, ncomp, y.copy(), k1, k2, DT), P.np_ab2(y, k1, k2, DT)]
        return dy.get_hostfull(), [_expect(y, r, inner) for r in refs], None, None
    if kernel == "rkf45_combine":
        # k[1] is not read: the loops pass k[0] in its place
        ks = [k1, k1, k3, k4, k5, k6]
        dk = {id(k): d.up(k) for k in ks}
        dy, dnew = d.up(y), d.up(k2)
        table = ptr_array([dk[id(k)] for k in ks])
        err = d.norm(lambda p: lib.rkf45_combine(d.info.ref, ncomp, dy.ptr, dnew.ptr, table, p, None))
        o_new, o_err = O.rkf45_combine(g, ncomp, y, ks)
        n_new, n_err = P.np_rkf45(y, ks, inner)
        return dnew.get_hostfull(), [_expect(k2, o_new, inner), _expect(k2, n_new, inner)], err, [o_err, n_err]
    if kernel == "euler_adaptive_combine":
        dy, dr, dh, dk, dout = d.up(y), d.up(k1), d.up(k2), d.up(k3), d.up(k4)
        err = d.norm(lambda p: lib.euler_adaptive_combine(d.info.ref, ncomp, dy.ptr, dr.ptr, DT, dh.ptr, dk.ptr, dout.ptr, p, None))
        o_out, o_err = O.euler_adaptive_combine(g, ncomp, y, k1, DT, k2, k3)
        n_out, n_err = P.np_euler_adaptive(y, k1, DT, k2, k3, inner)
        return dout.get_hostfull(), [_expect(k4, o_out, inner), _expect(k4, n_out, inner)], err, [o_err, n_err]
    raise AssertionError(kernel)


def _check_combine(d, kernel, ncomp, arrs):
    got, refs, err, err_refs = _run_combine(d, kernel, ncomp, arrs)
    for name, ref in zip(("oracle", "numpy"), refs):
        _same(got, ref, f"{kernel} against {name} (ghost cells included)")
    if err is not None:
        _assert_three((err, *err_refs), f"{kernel}: error norm")


# ---- combine kernels: every fastest extent, 1-D to 3-D, 1 to 3 components -------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,ncomp", P.SMALL)
@pytest.mark.parametrize("kernel", COMBINES)
def test_combine_small(lib, kernel, shape, ncomp, dtype):
    _check_combine(Dev(lib, shape, dtype), kernel, ncomp, P.fields(shape, ncomp, dtype, 7, seed=1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(3, 5, 8), (3, 5, 7), (2, 6)])
def test_lincomb_forms(lib, shape, dtype):
    """1 to 6 terms, with and without ``y``, in place (``out == y``) and with ``out`` one of the ``k`` - the forms in which the
    complex adaptive steps call it.  Elementwise, so an aliased call has to give what the oracle gives without aliasing."""
    ncomp = 2
    d = Dev(lib, shape, dtype)
    arrs = P.fields(shape, ncomp, dtype, 7, seed=4)
    y, ks, spare = arrs[0], arrs[1:7], arrs[6]
    for nk in range(1, 7):
        coef = (C.c_double * nk)(*COEFS[:nk])
        for with_y in (True, False):
            yy = y if with_y else None
            refs = [O.lincomb(d.g, ncomp, yy, COEFS[:nk], ks[:nk]), P.np_lincomb(yy, COEFS[:nk], ks[:nk])]
            forms = [("apart", None)] + ([("out == y", "y")] if with_y else []) + [("out == k[0]", 0), (f"out == k[{nk - 1}]", nk - 1)]
            for form, alias in forms:
                dy, dks = d.up(y), [d.up(k) for k in ks[:nk]]
                if alias is None:
                    dout, before = d.up(spare), spare
                elif alias == "y":
                    dout, before = dy, y
                else:
                    dout, before = dks[alias], ks[alias]
                lib.lincomb(d.info.ref, ncomp, dout.ptr, dy.ptr if with_y else None, nk, coef, ptr_array(dks), None)
                got = dout.get_hostfull()
                for name, ref in zip(("oracle", "numpy"), refs):
                    _same(got, _expect(before, ref, d.inner), f"lincomb, {nk} terms, y {with_y}, {form}, against {name}")
                if alias != "y" and with_y:
                    _same(dy.get_hostfull(), y, "lincomb must not write y")


def test_refusals_launch_nothing(lib):
    """0 and 7 terms and NULL pointers: an error code, a message from pdehip_last_error, and the output as it was."""
    shape, ncomp = (3, 8), 1
    d = Dev(lib, shape, np.float64)
    y, k1, out0 = P.fields(shape, ncomp, np.float64, 3, seed=5)
    dy, dk, dout = d.up(y), d.up(k1), d.up(out0)
    coef = (C.c_double * 7)(*([0.5] * 7))
    table = ptr_array([dk] * 7)
    h, g, null = lib._h, d.info.ref, None
    err = d.err.ptr
    calls = {
        "lincomb 0 terms": (lambda: h.pdehip_lincomb(g, ncomp, dout.ptr, dy.ptr, 0, coef, table, null), "1..6 terms"),
        "lincomb 7 terms": (lambda: h.pdehip_lincomb(g, ncomp, dout.ptr, dy.ptr, 7, coef, table, null), "1..6 terms"),
        "lincomb NULL out": (lambda: h.pdehip_lincomb(g, ncomp, null, dy.ptr, 1, coef, table, null), "NULL"),
        "lincomb NULL coef": (lambda: h.pdehip_lincomb(g, ncomp, dout.ptr, dy.ptr, 1, null, table, null), "NULL"),
        "lincomb NULL table": (lambda: h.pdehip_lincomb(g, ncomp, dout.ptr, dy.ptr, 1, coef, null, null), "NULL"),
        "rk4 NULL k": (lambda: h.pdehip_rk4_combine(g, ncomp, dout.ptr, dk.ptr, dk.ptr, null, dk.ptr, null), "NULL"),
        "ab2 NULL rate": (lambda: h.pdehip_ab2_combine(g, ncomp, dout.ptr, null, dk.ptr, DT, null), "NULL"),
        "rkf45 NULL err": (lambda: h.pdehip_rkf45_combine(g, ncomp, dy.ptr, dout.ptr, table, null, null), "NULL"),
        "rkf45 NULL table": (lambda: h.pdehip_rkf45_combine(g, ncomp, dy.ptr, dout.ptr, null, err, null), "NULL"),
        "euler_adaptive NULL out": (lambda: h.pdehip_euler_adaptive_combine(g, ncomp, dy.ptr, dk.ptr, DT, dk.ptr, dk.ptr, null, err, null), "NULL"),
        "max_abs_diff NULL b": (lambda: h.pdehip_max_abs_diff(g, ncomp, dout.ptr, null, err, null), "NULL"),
        "max_abs_pairs no pairs": (lambda: h.pdehip_max_abs_pairs(g, 0, dout.ptr, err, null), "no pairs"),
        "integrate 0 components": (lambda: h.pdehip_integrate(g, 0, dout.ptr, 1.0, err, null), "1..64"),
        "integrate 65 components": (lambda: h.pdehip_integrate(g, 65, dout.ptr, 1.0, err, null), "1..64"),
        "integrate NULL out": (lambda: h.pdehip_integrate(g, 1, dout.ptr, 1.0, null, null), "NULL"),
        "count_nonfinite 0 components": (lambda: h.pdehip_count_nonfinite(g, 0, dout.ptr, err, null), "1..64"),
        "count_nonfinite 65 components": (lambda: h.pdehip_count_nonfinite(g, 65, dout.ptr, err, null), "1..64"),
    }
    marker = C.c_double(-77.0)
    lib.memcpy_h2d(err, C.addressof(marker), 8, None)
    for name, (call, words) in calls.items():
        rc = call()
        assert rc == 1, f"{name}: code {rc}"
        assert words in lib.last_error(), f"{name}: {lib.last_error()!r}"
    lib.stream_synchronize(None)
    _same(dout.get_hostfull(), out0, "a refused call wrote the output")
    assert d.err.value() == -77.0, "a refused call wrote the error cell"


# ---- error norms ----------------------------------------------------------------------------------------------------------
# one grid per launch path, several workgroups, two components (max_abs_pairs: two pairs); fastest extent 64 is fp64 pairs and
# fp32 quads, 63 one cell per item in both types
NORM_SHAPES = [(5, 7, 64), (5, 7, 63)]


def _norm_inputs(kernel, shape, ncomp, dtype):
    """Host arrays of a norm kernel with a small error everywhere, and the name of the array a larger error is planted in."""
    if kernel == "max_abs_pairs":
        return {"z": P.pair_fields(shape, ncomp, dtype, seed=6)}, "z"
    y, k1, k2, k3, k4, k5, k6 = P.fields(shape, ncomp, dtype, 7, seed=6)
    if kernel == "max_abs_diff":
        return {"a": y, "b": k1}, "a"
    if kernel == "rkf45_combine":
        return {"y": y, "k1": k1, "k3": k3, "k4": k4, "k5": k5, "k6": k6, "new": k2}, "k6"
    return {"y": y, "rate": k1, "half": k2, "k": k3, "out": k4}, "y"


def _norm_three(d, kernel, ncomp, h):
    """(device bits, oracle bits, numpy bits) of the norm of the host arrays ``h``."""
    lib, ref, g, inner = d.lib, d.info.ref, d.g, d.inner
    dv = {name: d.up(a) for name, a in h.items()}
    if kernel == "max_abs_pairs":
        got = d.norm(lambda p: lib.max_abs_pairs(ref, ncomp, dv["z"].ptr, p, None))
        return got, O.max_abs_pairs(g, ncomp, h["z"]), P.np_max_abs_pairs(h["z"], inner)
    if kernel == "max_abs_diff":
        got = d.norm(lambda p: lib.max_abs_diff(ref, ncomp, dv["a"].ptr, dv["b"].ptr, p, None))
        return got, O.max_abs_diff(g, ncomp, h["a"], h["b"]), P.np_max_abs_diff(h["a"], h["b"], inner)
    if kernel == "rkf45_combine":
        names = ["k1", "k1", "k3", "k4", "k5", "k6"]
        table = ptr_array([dv[n] for n in names])
        got = d.norm(lambda p: lib.rkf45_combine(ref, ncomp, dv["y"].ptr, dv["new"].ptr, table, p, None))
        ks = [h[n] for n in names]
        return got, O.rkf45_combine(g, ncomp, h["y"], ks)[1], P.np_rkf45(h["y"], ks, inner)[1]
    got = d.norm(lambda p: lib.euler_adaptive_combine(ref, ncomp, dv["y"].ptr, dv["rate"].ptr, DT, dv["half"].ptr, dv["k"].ptr, dv["out"].ptr, p, None))
    return (got, O.euler_adaptive_combine(g, ncomp, h["y"], h["rate"], DT, h["half"], h["k"])[1],
            P.np_euler_adaptive(h["y"], h["rate"], DT, h["half"], h["k"], inner)[1])


def _assert_three(three, what, expect=None):
    got, o, n = three[0], P.f64_bits(three[1]), P.f64_bits(three[2])
    print(f"{what}: device {got:#018x} oracle {o:#018x} numpy {n:#018x}")
    assert got == o == n, f"{what}: device {got:#018x} oracle {o:#018x} numpy {n:#018x}"
    if expect is not None:
        assert got == P.f64_bits(expect), f"{what}: {got:#018x}, expected {P.f64_bits(expect):#018x}"


def _vec(kernel, dtype, shape):
    return 1 if kernel == "max_abs_pairs" else P.vec_width(dtype, shape[-1])


def _positions(kernel, shape, ncomp, dtype):
    """Where the largest error is placed in turn: (name, item, lane)."""
    vec = _vec(kernel, dtype, shape)
    items = P.items_of(shape, ncomp, vec)
    last_wg = (items - 1) // 256 * 256
    assert items > 3 * 256 and items - last_wg < 256, "several workgroups, the last one ragged"
    pos = [("first cell", 0, 0), ("last cell", items - 1, vec - 1), ("last lane of a vector", 5, vec - 1)]
    pos += [(f"wave {w} of workgroup 1", 256 + 64 * w + 10 + w, 0) for w in range(4)]
    pos += [("first workgroup", 200, 0), ("last workgroup", last_wg + 1, 0)]
    pos += [("second component", items // 2 + 300, vec // 2)]
    return vec, pos


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", NORM_SHAPES)
@pytest.mark.parametrize("kernel", NORMS)
def test_norm_finds_the_largest_entry_anywhere(lib, kernel, shape, dtype):
    """The largest entry in the first and the last cell, the last lane of a vector, each wave of a workgroup, the first and the
    last workgroup and a second component: a wave or workgroup left out of the maximum returns the background error."""
    ncomp = 2
    d = Dev(lib, shape, dtype)
    base, plant = _norm_inputs(kernel, shape, ncomp, dtype)
    background = _norm_three(d, kernel, ncomp, base)
    _assert_three(background, f"{kernel} background")
    vec, positions = _positions(kernel, shape, ncomp, dtype)
    for name, item, lane in positions:
        h = dict(base)
        h[plant] = base[plant].copy()
        cell = P.cell_of_item(item, shape, vec, lane)
        if name == "second component":
            assert cell[0] == 1
        if kernel == "max_abs_pairs":   # 3 + 4j times 2^10: larger than every modulus of the background, and exact
            h[plant][(2 * cell[0], *cell[1:])], h[plant][(2 * cell[0] + 1, *cell[1:])] = 3072.0, -4096.0
        else:
            h[plant][cell] = 4096.0 + item % 7
        three = _norm_three(d, kernel, ncomp, h)
        _assert_three(three, f"{kernel}, largest entry in the {name}")
        assert three[0] != background[0], f"{name}: the planted entry does not decide the norm"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", NORM_SHAPES)
@pytest.mark.parametrize("kernel", NORMS)
def test_norm_zero_denormal_nan_infinity(lib, kernel, shape, dtype):
    """All-equal inputs give 0; the smallest denormal comes back exactly; in the last workgroup, with finite cells everywhere
    else: one infinity gives inf, one NaN gives NaN, an infinity and a NaN in different cells give NaN, a NaN with the sign bit
    set gives NaN.  Pairs: (inf, nan) is inf like numpy's abs, and NaN once a pair (nan, 1) is somewhere else."""
    ncomp = 2
    d = Dev(lib, shape, dtype)
    base, plant = _norm_inputs(kernel, shape, ncomp, dtype)
    vec, positions = _positions(kernel, shape, ncomp, dtype)
    last = dict((n, (i, l)) for n, i, l in positions)["last workgroup"]
    cell = P.cell_of_item(last[0], shape, vec, 0)
    other = P.cell_of_item(last[0] + 3, shape, vec, vec - 1)
    far = P.cell_of_item(70, shape, vec, 0)
    assert cell[0] == other[0] == 1 and far[0] == 0

    # zero, and the smallest denormal of the field's type
    tiny = np.finfo(dtype).smallest_subnormal
    if kernel == "max_abs_pairs":
        zero = {"z": np.zeros_like(base["z"])}
        _assert_three(_norm_three(d, kernel, ncomp, zero), "pairs of zeros", 0.0)
    elif kernel == "max_abs_diff":
        _assert_three(_norm_three(d, kernel, ncomp, {"a": base["a"], "b": base["a"]}), "a == b", 0.0)
        a = base["a"].copy()
        a[cell] = 0.0
        b = a.copy()
        b[cell] = tiny
        _assert_three(_norm_three(d, kernel, ncomp, {"a": a, "b": b}), "difference of one denormal", float(tiny))
    elif kernel == "rkf45_combine":
        zero = {n: (a if n in ("y", "new") else np.zeros_like(a)) for n, a in base.items()}
        _assert_three(_norm_three(d, kernel, ncomp, zero), "all slopes zero", 0.0)
    else:
        zero = dict(base, rate=np.zeros_like(base["y"]), k=np.zeros_like(base["y"]), half=base["y"])
        _assert_three(_norm_three(d, kernel, ncomp, zero), "both steps equal", 0.0)
        y = base["y"].copy()
        half = y.copy()
        y[cell], half[cell] = tiny, 0.0
        _assert_three(_norm_three(d, kernel, ncomp, dict(zero, y=y, half=half)), "steps one denormal apart", float(tiny))

    def planted(values):
        h = dict(base)
        h[plant] = base[plant].copy()
        for where, v in values:
            if kernel == "max_abs_pairs":
                where = (2 * where[0], *where[1:])
            h[plant][where] = v
        return h

    for what, values, expect in [("one infinity", [(cell, np.inf)], np.inf), ("one negative infinity", [(cell, -np.inf)], np.inf),
                                 ("one NaN", [(cell, np.nan)], np.nan), ("an infinity and a NaN", [(cell, np.inf), (other, np.nan)], np.nan),
                                 ("a NaN and an infinity", [(cell, np.nan), (other, np.inf)], np.nan),
                                 ("a NaN and an infinity in another workgroup", [(cell, np.nan), (far, np.inf)], np.nan),
                                 ("a NaN with the sign bit set", [(cell, NEG_NAN)], np.nan)]:
        _assert_three(_norm_three(d, kernel, ncomp, planted(values)), f"{kernel}: {what}", expect)
    if kernel == "max_abs_pairs":
        z = base["z"].copy()
        z[(2 * cell[0], *cell[1:])], z[(2 * cell[0] + 1, *cell[1:])] = np.inf, np.nan
        _assert_three(_norm_three(d, kernel, ncomp, {"z": z}), "the pair (inf, nan)", np.inf)
        z[(2 * far[0], *far[1:])], z[(2 * far[0] + 1, *far[1:])] = np.nan, 1.0
        _assert_three(_norm_three(d, kernel, ncomp, {"z": z}), "the pairs (inf, nan) and (nan, 1)", np.nan)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,ncomp", P.SMALL)
@pytest.mark.parametrize("kernel", ["max_abs_diff", "max_abs_pairs"])
def test_norm_small(lib, kernel, shape, ncomp, dtype):
    """Every fastest extent; the two norms that come with a combine run at these shapes in `test_combine_small`."""
    d = Dev(lib, shape, dtype)
    base, _ = _norm_inputs(kernel, shape, ncomp, dtype)
    _assert_three(_norm_three(d, kernel, ncomp, base), f"{kernel} {shape} x {ncomp}")


# ---- beyond the grid-stride turn ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _turn_fields(path):
    shape, ncomp, dtype, _ = P.TURN[path]
    arrs = P.fields(shape, ncomp, dtype, 7, seed=7)
    for a in arrs:
        a.setflags(write=False)
    return arrs


def _turn_cell(path, kernel):
    """A cell whose item index lies beyond the first pass of every thread: 4 194 304 + 1000 (+ the last lane of its vector)."""
    shape, ncomp, dtype, vec = P.TURN[path]
    if kernel == "max_abs_pairs":   # one pair, one cell per item whatever the extent
        ncomp, vec = 1, 1
    items = P.items_of(shape, ncomp, vec)
    row = shape[-1] // vec
    assert items >= P.TURN_ITEMS + row and items % 256 != 0
    if kernel != "max_abs_pairs":
        assert vec == P.vec_width(dtype, shape[-1])
    return P.cell_of_item(P.TURN_ITEMS + 1000, shape, vec, vec - 1)


@pytest.mark.parametrize("path", list(P.TURN))
@pytest.mark.parametrize("kernel", COMBINES)
def test_combine_beyond_the_turn(lib, kernel, path):
    """More than 4 194 304 items: the cells of the second pass are compared like all others, and for the two kernels with an
    error norm the largest error sits among them."""
    shape, ncomp, dtype, vec = P.TURN[path]
    arrs = list(_turn_fields(path))
    cell = _turn_cell(path, kernel)
    plant = {"rkf45_combine": 6, "euler_adaptive_combine": 0}.get(kernel)
    if plant is not None:
        arrs[plant] = arrs[plant].copy()
        arrs[plant][cell] = 4099.0
    _check_combine(Dev(lib, shape, dtype), kernel, ncomp, arrs)


@pytest.mark.parametrize("path", list(P.TURN))
@pytest.mark.parametrize("kernel", ["max_abs_diff", "max_abs_pairs"])
def test_norm_beyond_the_turn(lib, kernel, path):
    """The one entry that decides the norm lies beyond the turn; everything else differs by less."""
    shape, ncomp, dtype, vec = P.TURN[path]
    d = Dev(lib, shape, dtype)
    cell = _turn_cell(path, kernel)
    if kernel == "max_abs_pairs":
        # one pair: the kernel takes one cell per item whatever the extent, so 129 x 127 x 516 turns with one pair as well
        z = P.pair_fields(shape, 1, dtype, seed=8)
        background = P.np_max_abs_pairs(z, d.inner)
        z[(0, *cell[1:])], z[(1, *cell[1:])] = -3072.0, 4096.0
        three = _norm_three(d, kernel, 1, {"z": z})
        planted = 5120.0
    else:
        a, b = _turn_fields(path)[:2]
        background = P.np_max_abs_diff(a, b, d.inner)
        a = a.copy()
        a[cell] = 4099.0
        three = _norm_three(d, kernel, ncomp, {"a": a, "b": b})
        planted = float(P.np_max_abs_diff(a[cell], b[cell], ()))
    _assert_three(three, f"{kernel} {path}", planted)
    assert 4 * background < planted


def test_turn_cases_cover_the_four_paths():
    for path, (shape, ncomp, dtype, vec) in P.TURN.items():
        assert vec == P.vec_width(dtype, shape[-1]), path
        items = P.items_of(shape, ncomp, vec)
        assert items >= P.TURN_ITEMS + shape[-1] // vec and items % 256, path
    assert sorted((np.dtype(t).itemsize, v) for _, _, t, v in P.TURN.values()) == [(4, 1), (4, 4), (8, 1), (8, 2)]


# ---- pdehip_integrate ------------------------------------------------------------------------------------------------------
SUM_SHAPES = [(64, 64, 64), (65, 64, 65)]
# roundings on the longest path of one cell's product to the result, beyond the thread's own running sum:
#   the product `vol * x`                                                         1
#   the wave butterfly of block_sum (6 exchanges)                                 6
#   the four wave parts, added to 0 in turn (the first addition is exact)         3
#   final_sum_kernel: up to 1024 / 256 = 4 partials per thread (first one exact)  3
#   its butterfly and its four parts                                              6 + 3
# 22 in all, and one more for math.fsum, which rounds the exact sum once: 23.  The bound below takes 24.
SUM_ROUNDINGS = 24


def _sum_bound(cells, mag):
    """`(m + c) * 2^-53 * sum |vol * x|`: m = the largest number of cells one thread adds to its running sum (m roundings at
    most: each addition rounds once, the first one is exact), c = SUM_ROUNDINGS.  Every rounding is relative to a partial
    sum of magnitudes no larger than the whole sum of magnitudes; the second-order terms are below 1e-13 of the bound."""
    nblocks = min(1024, max(1, -(-cells // 256)))
    m = -(-cells // (256 * nblocks))
    return (m + SUM_ROUNDINGS) * 2.0 ** -53 * mag, m


def _integrate(lib, d, dev, ncomp, vol, stream=None, out=None):
    out = out if out is not None else DeviceBuffer(8 * ncomp)
    lib.integrate(d.info.ref, ncomp, dev.ptr, vol, out.ptr, stream)
    host = np.empty(ncomp)
    lib.memcpy_d2h(host.ctypes.data, out.ptr, 8 * ncomp, stream)
    return host


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,ncomp", [((64, 64, 64), 1), ((65, 64, 65), 3), ((64, 64, 64), 3), ((65, 64, 65), 1), ((5, 6, 7), 64), ((257,), 3), ((3, 65), 1)])
def test_integrate(lib, shape, ncomp, dtype):
    """Against `math.fsum` of the float64 products, within the bound derived from the kernels (`_sum_bound`, 24 + m roundings:
    the count is at SUM_ROUNDINGS).  uniform(0.5, 1.5) data: a dropped cell, row, wave or workgroup moves the result by at
    least 0.5 * cell_volume, many orders above the bound.  64^3 is exactly 1024 workgroups of one cell per thread, 65 x 64 x 65
    takes the grid-stride turn (m = 2).  Two runs give equal bits, and a spike in the very last cell of the last component is
    found."""
    vol = 0.37
    d = Dev(lib, shape, dtype)
    rng = np.random.default_rng(11)
    full = rng.uniform(0.5, 1.5, (ncomp, *[s + 2 for s in shape])).astype(dtype)
    full[:, P.ghost_mask(shape)] = 1e30   # a ghost cell in the sum would be seen
    dev = d.up(full)
    got = _integrate(lib, d, dev, ncomp, vol)
    exact, mag = P.fsum_integrate(full, vol, d.inner)
    cells = int(np.prod(shape))
    bound, m = _sum_bound(cells, mag)
    assert m == (2 if cells > 262144 else 1)
    print(f"integrate {shape} x {ncomp} {np.dtype(dtype).name}: largest error {np.abs(got - exact).max():.3e}, bound {bound.min():.3e}, m = {m}")
    assert np.all(np.abs(got - exact) <= bound), f"off by {np.abs(got - exact).max():.3e}, allowed {bound.min():.3e}"
    assert 0.5 * vol > 1e6 * bound.max()
    np.testing.assert_array_equal(P.bits(_integrate(lib, d, dev, ncomp, vol)), P.bits(got))
    # the oracle's sequential sum rounds `cells` times: the two agree within the sum of both bounds
    assert np.all(np.abs(got - O.integrate(d.g, ncomp, full, vol)) <= bound + cells * 2.0 ** -53 * mag)
    # a spike in the very last cell of the last component
    spike = full.copy()
    last = (ncomp - 1, *shape)
    spike[last] = 1e6
    got = _integrate(lib, d, d.up(spike), ncomp, vol)
    exact, mag = P.fsum_integrate(spike, vol, d.inner)
    assert np.all(np.abs(got - exact) <= _sum_bound(cells, mag)[0])
    assert got[-1] > 0.9e6 * vol


@pytest.mark.parametrize("dtype", DTYPES)
def test_integrate_two_streams(lib, dtype):
    """Two streams integrate two different fields at the same time: each gets the bits it gets alone.  Both streams wait for
    an event behind a queue of copies on a third stream, so that the reductions of both are enqueued before either starts and
    then run side by side (without the gate the first stream has finished before the host has launched the second)."""
    shape, ncomp, vol = (65, 64, 65), 8, 0.37
    d = Dev(lib, shape, dtype)
    rng = np.random.default_rng(12)
    fulls = [rng.uniform(0.5, 1.5, (ncomp, *[s + 2 for s in shape])).astype(dtype), rng.uniform(-1.5, -0.5, (ncomp, *[s + 2 for s in shape])).astype(dtype)]
    devs = [d.up(f) for f in fulls]
    alone = [_integrate(lib, d, dev, ncomp, vol) for dev in devs]
    # the gate: copies of a 4.2 million cell field, some 20 microseconds each and slower than the host launches them
    big = GridInfo((65, 129, 501), (1.0,) * 3, np.float64)
    src, copy = DeviceArray(big, (1,)), DeviceArray(big, (1,))
    one, table = (C.c_double * 1)(1.0), ptr_array([src])
    streams, event = [], C.c_void_p()
    for _ in range(3):
        s = C.c_void_p()
        lib.stream_create(C.byref(s))
        streams.append(s)
    lib.event_create(C.byref(event))
    try:
        outs = [DeviceBuffer(8 * ncomp) for _ in range(2)]
        for _ in range(3):
            for _ in range(150):
                lib.lincomb(big.ref, 1, copy.ptr, None, 1, one, table, streams[2])
            lib.event_record(event, streams[2])
            for q in range(2):
                lib.stream_wait_event(streams[q], event)
            for q in range(2):
                lib.integrate(d.info.ref, ncomp, devs[q].ptr, vol, outs[q].ptr, streams[q])
            for q in range(2):
                host = np.empty(ncomp)
                lib.memcpy_d2h(host.ctypes.data, outs[q].ptr, 8 * ncomp, streams[q])
                np.testing.assert_array_equal(P.bits(host), P.bits(alone[q]), err_msg=f"stream {q}: {host} != {alone[q]}")
    finally:
        for s in streams:
            lib.stream_synchronize(s)
            lib.stream_destroy(s)
        lib.event_destroy(event)


# ---- pdehip_count_nonfinite -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SUM_SHAPES + [(3, 65)])
def test_count_nonfinite(lib, shape, dtype):
    """NaN, +inf and -inf counted exactly per component; denormals and +-finfo.max are not.  On 65 x 64 x 65 the bad cells
    sit beyond cell 262 144, where only the second pass of a thread reads them; on 64^3 they include the last workgroup."""
    ncomp = 3
    d = Dev(lib, shape, dtype)
    rng = np.random.default_rng(13)
    full = rng.uniform(-1, 1, (ncomp, *[s + 2 for s in shape])).astype(dtype)
    full[:, P.ghost_mask(shape)] = np.nan   # ghost cells are not counted
    cells = int(np.prod(shape))
    first = 262144 if cells > 262144 else cells // 2
    assert cells - first > 60
    info = np.finfo(dtype)
    if np.dtype(dtype) == np.float32:
        payload = [np.uint32(0x7FC12345).view(np.float32), np.uint32(0xFF812345).view(np.float32)]   # a quiet and a signalling NaN
    else:
        payload = [np.uint64(0x7FF8000000012345).view(np.float64), np.uint64(0xFFF0000000012345).view(np.float64)]
    kinds = [np.nan, np.inf, -np.inf, *payload]
    harmless = [info.max, -info.max, info.smallest_subnormal, -info.smallest_subnormal, info.tiny, 0.0, -0.0]
    inner = full[d.inner].reshape(ncomp, -1).copy()
    for c in range(ncomp):
        spots = first + rng.choice(cells - first, size=40 + 7 * c, replace=False)
        for q, s in enumerate(spots[: 20 + 5 * c]):
            inner[c, s] = kinds[q % len(kinds)]
        for q, s in enumerate(spots[20 + 5 * c:]):
            inner[c, s] = harmless[q % len(harmless)]
        inner[c, cells - 1 - c] = np.nan   # the last cells of the last workgroup
    full[d.inner] = inner.reshape(full[d.inner].shape)
    expect = P.np_count_nonfinite(full, d.inner)
    assert list(expect) == [21.0 + 5 * c for c in range(ncomp)] or cells < 1000
    out = DeviceBuffer(8 * ncomp)
    host = np.empty(ncomp)
    dev = d.up(full)
    for _ in range(2):
        lib.count_nonfinite(d.info.ref, ncomp, dev.ptr, out.ptr, None)
        lib.memcpy_d2h(host.ctypes.data, out.ptr, 8 * ncomp, None)
        print(f"count_nonfinite {shape} {np.dtype(dtype).name}: {host} expected {expect}")
        np.testing.assert_array_equal(host, expect)
        np.testing.assert_array_equal(host, O.count_nonfinite(d.g, ncomp, full))
    clean = np.where(np.isfinite(full), full, 0).astype(dtype)
    clean[:, P.ghost_mask(shape)] = np.inf
    dev = d.up(clean)
    lib.count_nonfinite(d.info.ref, ncomp, dev.ptr, out.ptr, None)
    lib.memcpy_d2h(host.ctypes.data, out.ptr, 8 * ncomp, None)
    np.testing.assert_array_equal(host, np.zeros(ncomp))
