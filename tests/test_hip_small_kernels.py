"""Device tests of the small kernels every run passes through before it reaches a sweep, through the C ABI.

``pdehip_set_ghost_cells`` (``ghost_kernel``), ``pdehip_valid_to_full`` / ``pdehip_full_to_valid`` /
``pdehip_hostfull_to_full`` / ``pdehip_full_to_hostfull`` (``layout_copy_kernel``), ``pdehip_copy_nt``,
``pdehip_add_gaussian_noise``, ``pdehip_field_product`` and ``pdehip_axis_derivative``.  Cases, references and the
conditions that keep a case from being vacuous: ``tests/small_kernel_cases.py``, tied to the oracle on the CPU by
``tests/test_small_kernel_cases_cpu.py``.

Every test reads the WHOLE allocation back (``ncomp * pc + slack`` elements, uploaded as a pattern of distinct values
with ``memcpy_h2d``) and compares every element: what the call must write against the reference, everything else -
interior cells, edge and corner ghost cells, row padding, other components, the slack - against the pattern.  The cells
are placed by a restatement of the layout rule (`S.Layout`); the eight numbers of ``pdehip_layout`` are asserted equal
to it first (`Dev`).  Staging buffers carry 64 sentinel elements behind their end.

Launch geometry: ``ghost_kernel`` takes at most 4096 workgroups (a second item per thread beyond 1 048 576 face items),
the layout copies, the noise and the axis derivative at most 16 384 (4 194 304 items); ``field_product_kernel`` and
``copy_nt_kernel`` are not capped.  None of these entry points records a kernel name (``pdehip_last_kernel_name``).
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import small_kernel_cases as S

import pde_hip
from oracle import pde_oracle as O
from pde_hip import _abi
from pde_hip.backend import convert_bcs
from pde_hip.device import DeviceArray, DeviceBuffer, GridInfo
from pde_hip.faces import _upload_f64

pytestmark = pytest.mark.gpu

DTYPES = list(S.DTYPES)


@pytest.fixture(scope="module")
def lib():
    return pde_hip.get_backend("hip")._lib


class Dev:
    """One grid on the device.  The library's layout has to be the restated one; after that `S.Layout` places the cells."""

    def __init__(self, lib, shape, dtype, dx=None):
        self.lib = lib
        self.lay = S.Layout(shape, dtype)
        self.info = GridInfo(shape, dx if dx is not None else (1.0,) * len(shape), dtype)
        eight = (C.c_int64 * 8)()
        lib.layout(self.info.ref, eight)
        assert list(eight) == self.lay.eight(), f"pdehip_layout {list(eight)} != the documented rule {self.lay.eight()}"

    def array(self, ncomp, img):
        """A device array whose whole allocation holds ``img``."""
        arr = DeviceArray(self.info, (ncomp,))
        assert arr.nbytes == img.nbytes == self.lay.nelem(ncomp) * self.lay.dtype.itemsize and img.flags.c_contiguous
        self.lib.memcpy_h2d(arr.ptr, img.ctypes.data, img.nbytes, None)
        return arr

    def read(self, arr):
        out = np.empty(arr.nbytes // self.lay.dtype.itemsize, self.lay.dtype)
        self.lib.memcpy_d2h(out.ctypes.data, arr.ptr, out.nbytes, None)
        return out


def _buffer(lib, host):
    host = np.ascontiguousarray(host)
    buf = DeviceBuffer(host.nbytes)
    lib.memcpy_h2d(buf.ptr, host.ctypes.data, host.nbytes, None)
    return buf


def _read(lib, buf, like):
    out = np.empty_like(like)
    assert out.nbytes == buf.nbytes
    lib.memcpy_d2h(out.ctypes.data, buf.ptr, out.nbytes, None)
    return out


def _same(got, ref, what, lay=None):
    """Bit equality of two flat images; the message says how many elements differ, where the first lies and by how much."""
    got, ref = np.ascontiguousarray(got).ravel(), np.ascontiguousarray(ref).ravel()
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    bad = np.flatnonzero(S.bits(got) != S.bits(ref))
    if bad.size:
        at = int(bad[0])
        where = f"element {at}"
        if lay is not None:
            comp, e = divmod(at, lay.pc)
            where += f" (component {comp}, row offset {e // lay.p1}, column {e % lay.p1}; interior columns {lay.lpad} .. {lay.lpad + lay.shape[-1] - 1})"
        with np.errstate(invalid="ignore", over="ignore"):
            off = np.nanmax(np.abs(got[bad].astype(np.float64) - ref[bad].astype(np.float64)))
        pytest.fail(f"{what}: {bad.size} of {got.size} elements differ, first at {where}: {got[at]!r} != {ref[at]!r}, largest difference {off:.3e}")


# ---- pdehip_set_ghost_cells ---------------------------------------------------------------------------------------------
def _check_ghosts(lib, shape, ncomp, dtype, faces, seed, table=None):
    d = Dev(lib, shape, dtype)
    lay = d.lay
    inner = S.interior(len(shape))
    img0 = S.start_image(lay, ncomp, S.field(shape, ncomp, dtype, seed), inner)
    before = S.gather(img0, lay, ncomp)                      # what the kernel sees: ghost cells hold the pattern
    ref = S.np_set_ghost_cells(shape, ncomp, faces, before.copy())
    twin = before.copy()
    O.set_ghost_cells(d.info.c, ncomp, S.face_table(faces), twin)
    assert (S.bits(ref) != S.bits(before)).any() or all(f["flags"] & _abi.BCF_NORMAL for f in faces)
    arr = d.array(ncomp, img0)
    dev_table = table if table is not None else S.face_table(faces, upload=_upload_f64)
    lib.set_ghost_cells(d.info.ref, ncomp, dev_table, arr.ptr, None)
    got = d.read(arr)
    case = f"set_ghost_cells, {ncomp} component(s), {np.dtype(dtype).name}"
    _same(got, S.place(img0.copy(), lay, ncomp, ref), f"{case}, against the restatement (whole allocation)", lay)
    _same(got, S.place(img0.copy(), lay, ncomp, twin), f"{case}, against the oracle (whole allocation)", lay)


@pytest.mark.parametrize("variant", S.GHOST_VARIANTS)
@pytest.mark.parametrize("shape", S.GHOST_SHAPES)
def test_ghost_cells(lib, shape, variant):
    """1, 3 and 9 components, both types."""
    for ncomp in S.GHOST_NCOMP:
        for dtype in DTYPES:
            _check_ghosts(lib, shape, ncomp, dtype, S.ghost_faces(shape, ncomp, variant), seed=len(shape))


def test_ghost_cells_beyond_the_turn(lib):
    """1 089 856 face items for 1 048 576 threads: the end of the lower x face and all of the y and z faces are second items."""
    shape, ncomp = S.GHOST_TURN_CASE
    for dtype in DTYPES:
        _check_ghosts(lib, shape, ncomp, dtype, S.ghost_faces(shape, ncomp, "turn"), seed=5)


FRONT_END = [
    # (shape, periodic, rank, conditions per axis)
    ((130,), [False], 0, [[{"value": 1.5}, {"curvature": -0.3}]]),
    ((9, 65), [False, True], 0, [[{"derivative": 0.4}, {"mixed": 0.7, "const": 0.2}], "periodic"]),
    ((3, 5, 7), [False, False, False], 1, [[{"normal_value": 1.5}, {"normal_derivative": -0.4}], [{"curvature": 0.3}, {"value": 2.0}],
                                        [{"normal_curvature": 0.6}, {"normal_mixed": 0.5, "const": -1.0}]]),
    ((9, 4, 130), [True, False, False], 1, ["periodic", [{"value": [1.0, -2.0, 0.5]}, {"derivative": [0.1, 0.2, 0.3]}], {"curvature": 0.25}]),
]


@pytest.mark.parametrize("case", range(len(FRONT_END)))
def test_ghost_cells_of_front_end_conditions(lib, case):
    """The same comparison with tables `convert_bcs` builds from the front end's spellings (value, derivative, mixed, curvature, the
    normal_* conditions of vector fields, periodic axes): device arrays for the kernel, host arrays for the oracle and the restatement."""
    shape, periodic, rank, bc = FRONT_END[case]
    grid = pde_hip.UnitGrid(shape, periodic=periodic)
    bcs = grid.get_boundary_conditions(bc, rank=rank)
    ncomp = len(shape) ** rank
    comp_shape = (len(shape),) * rank
    host = convert_bcs(bcs, comp_shape, upload=S.HostArray)
    faces = S.faces_of_table(host.c, shape, ncomp)
    assert {f["kind"] for f in faces} <= {_abi.BC_ORDER1, _abi.BC_ORDER2}
    for dtype in DTYPES:
        _check_ghosts(lib, shape, ncomp, dtype, faces, seed=11 + case, table=convert_bcs(bcs, comp_shape).c)


def test_ghost_cells_refusals(lib):
    d = Dev(lib, (5, 9), np.float64)
    img = S.image(d.lay, 1)
    arr = d.array(1, img)
    faces = S.ghost_faces((5, 9), 1, "o2_scalar")
    for change in ({"index1": 5}, {"index1": -1}, {"index2": 5}, {"kind": 7}):
        bad = [dict(f) for f in faces]
        bad[1].update(change)
        with pytest.raises(ValueError):
            lib.set_ghost_cells(d.info.ref, 1, S.face_table(bad), arr.ptr, None)
    table = S.face_table(S.ghost_faces((5, 9), 1, "o2_array"), upload=_upload_f64)
    table[2].factor2_arr = None
    with pytest.raises(ValueError):
        lib.set_ghost_cells(d.info.ref, 1, table, arr.ptr, None)
    with pytest.raises(ValueError):
        lib.set_ghost_cells(d.info.ref, 0, S.face_table(faces), arr.ptr, None)
    with pytest.raises(ValueError):
        lib.set_ghost_cells(d.info.ref, 1, S.face_table(faces), None, None)
    _same(d.read(arr), img, "a refused call wrote", d.lay)


# ---- layout copies ------------------------------------------------------------------------------------------------------
def _check_copy(lib, shape, mode, ncomp, dtype):
    d = Dev(lib, shape, dtype)
    lay = d.lay
    img = S.image(lay, ncomp)                                                        # negative, all different
    count = ncomp * (lay.cells if mode < 2 else lay.full_cells)
    stage = S.pattern(count + S.SENTINELS, dtype, sign=1.0)                          # positive, all different
    want_img, want_stage = S.copy_expect(mode, lay, ncomp, img, stage)
    arr, buf = d.array(ncomp, img), _buffer(lib, stage)
    src, dst = (buf.ptr, arr.ptr) if mode in (0, 2) else (arr.ptr, buf.ptr)
    getattr(lib, S.COPY_MODES[mode])(d.info.ref, ncomp, src, dst, None)
    case = f"{S.COPY_MODES[mode]}, {ncomp} component(s), {np.dtype(dtype).name}"
    _same(d.read(arr), want_img, f"{case}: the device array (whole allocation)", lay)
    _same(_read(lib, buf, stage), want_stage, f"{case}: the compact buffer and its sentinels")


@pytest.mark.parametrize("mode", range(4), ids=S.COPY_MODES)
@pytest.mark.parametrize("shape", S.COPY_SHAPES)
def test_layout_copy(lib, shape, mode):
    """1, 3 and 9 components, both types."""
    for ncomp in S.COPY_NCOMP:
        for dtype in DTYPES:
            _check_copy(lib, shape, mode, ncomp, dtype)


@pytest.mark.parametrize("mode", range(4), ids=S.COPY_MODES)
def test_layout_copy_beyond_the_turn(lib, mode):
    """4 276 350 cells (modes 0 and 1) and 132 x 131 x 257 = 4 444 044 cells (modes 2 and 3) for 4 194 304 threads."""
    _check_copy(lib, S.COPY_TURN_SHAPE, mode, 1, np.float64)


def test_layout_copy_refusals(lib):
    d = Dev(lib, (5, 9), np.float64)
    img = S.image(d.lay, 1)
    arr = d.array(1, img)
    for name in S.COPY_MODES:
        with pytest.raises(ValueError):
            getattr(lib, name)(d.info.ref, 1, None, arr.ptr, None)
        with pytest.raises(ValueError):
            getattr(lib, name)(d.info.ref, 1, arr.ptr, None, None)
        with pytest.raises(ValueError):
            getattr(lib, name)(d.info.ref, 0, arr.ptr, arr.ptr, None)
    _same(d.read(arr), img, "a refused call wrote", d.lay)


# ---- pdehip_copy_nt -----------------------------------------------------------------------------------------------------
GUARD = 16   # 32-bit words = 64 bytes of sentinels before and behind


def _nt_buffers(lib, nbytes):
    words = nbytes // 4 + 2 * GUARD
    src = np.arange(words, dtype=np.uint32) + np.uint32(0x10000000)
    dst = np.arange(words, dtype=np.uint32) + np.uint32(0x80000000)
    return src, dst, _buffer(lib, src), _buffer(lib, dst)


@pytest.mark.parametrize("nbytes", S.COPY_NT_BYTES)
def test_copy_nt(lib, nbytes):
    """The yardstick of the benchmark copies the bytes asked for and no others."""
    src, dst, dsrc, ddst = _nt_buffers(lib, nbytes)
    lib.copy_nt(ddst.ptr + 4 * GUARD, dsrc.ptr + 4 * GUARD, nbytes, None)
    want = dst.copy()
    want[GUARD:GUARD + nbytes // 4] = src[GUARD:GUARD + nbytes // 4]
    got = _read(lib, ddst, dst)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {got.size} words differ, first at byte {4 * (int(bad[0]) - GUARD)} of {nbytes}, last at byte {4 * (int(bad[-1]) - GUARD)}"
    assert np.array_equal(_read(lib, dsrc, src), src)


def test_copy_nt_no_op_and_refusals(lib):
    src, dst, dsrc, ddst = _nt_buffers(lib, 4096)
    s, t = dsrc.ptr + 4 * GUARD, ddst.ptr + 4 * GUARD
    lib.copy_nt(t, s, 0, None)                       # zero bytes: nothing happens
    for args in ((None, s, 4096), (t, None, 4096), (t + 8, s, 4096), (t, s + 4, 4096), (t, s, 4088), (t, s, 24)):
        with pytest.raises(ValueError):
            lib.copy_nt(*args, None)
    assert np.array_equal(_read(lib, ddst, dst), dst) and np.array_equal(_read(lib, dsrc, src), src)


# ---- pdehip_add_gaussian_noise ------------------------------------------------------------------------------------------
def _check_noise(lib, shape, key, ncomp, dtype):
    seed, counter, offset = key
    d = Dev(lib, shape, dtype)
    lay = d.lay
    inner = S.interior(len(shape))
    img0 = S.start_image(lay, ncomp, S.noise_field(shape, ncomp, dtype), inner)
    before = S.gather(img0, lay, ncomp)
    arr = d.array(ncomp, img0)
    lib.add_gaussian_noise(d.info.ref, ncomp, arr.ptr, S.NOISE_SCALE, seed, counter, offset, None)
    got = d.read(arr)
    mask = S.interior_mask(lay, ncomp)
    atol = S.NOISE_ATOL[np.dtype(dtype)]
    for name, fn in (("the CPU twin", S.oracle_add_noise), ("the restatement", S.np_add_noise)):
        want = S.place(img0.copy(), lay, ncomp, fn(shape, ncomp, before.copy(), S.NOISE_SCALE, seed, counter, offset))
        _same(got[~mask], want[~mask], f"add_gaussian_noise, {ncomp} component(s), {np.dtype(dtype).name}, against {name}: ghost cells, padding and slack", None)
        diff = np.abs(got[mask].astype(np.float64) - want[mask].astype(np.float64))
        assert diff.max() <= atol, f"add_gaussian_noise, {ncomp} component(s), {np.dtype(dtype).name}, against {name}: {int((diff > atol).sum())} of {diff.size} cells off by up to {diff.max():.3e} (allowed {atol:.0e})"
    moved = np.abs(got[mask].astype(np.float64) - img0[mask].astype(np.float64)) / S.NOISE_SCALE
    assert moved.max() > 2      # (the draws of every case reach beyond two standard deviations: test_small_kernel_cases_cpu.py)


@pytest.mark.parametrize("key", range(len(S.NOISE_KEYS)))
@pytest.mark.parametrize("shape", S.NOISE_SHAPES)
def test_noise(lib, shape, key):
    """1, 2 and 3 components, both types."""
    for ncomp in S.NOISE_NCOMP:
        for dtype in DTYPES:
            _check_noise(lib, shape, S.NOISE_KEYS[key], ncomp, dtype)


def test_noise_beyond_the_turn(lib):
    for dtype in DTYPES:
        _check_noise(lib, S.NOISE_TURN_SHAPE, S.NOISE_KEYS[1], 1, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", S.NOISE_SHAPES)
def test_noise_of_three_components_is_three_calls(lib, shape, dtype):
    for key in S.NOISE_KEYS:
        _check_three_calls(lib, shape, key, dtype)


def _check_three_calls(lib, shape, key, dtype):
    """What the stepper of a collection relies on (pde_hip/noise_hooks.py): one call for k components draws what k calls for one
    component with ``cell_offset + k * cells`` draw, bit for bit."""
    seed, counter, offset = key
    d = Dev(lib, shape, dtype)
    lay = d.lay
    img0 = S.start_image(lay, 3, S.noise_field(shape, 3, dtype), S.interior(len(shape)))
    one, three = d.array(3, img0), d.array(3, img0)
    lib.add_gaussian_noise(d.info.ref, 3, one.ptr, S.NOISE_SCALE, seed, counter, offset, None)
    for k in range(3):
        lib.add_gaussian_noise(d.info.ref, 1, three.ptr + k * lay.pc * lay.dtype.itemsize, S.NOISE_SCALE, seed, counter, offset + k * lay.cells, None)
    got = d.read(one)
    _same(got, d.read(three), "one call for three components against three calls", lay)
    comps = got[: 3 * lay.pc].reshape(3, lay.pc)[:, lay.index_valid()] - S.gather(img0, lay, 3)[(slice(None), *S.interior(len(shape)))]
    assert np.abs(comps[0] - comps[1]).max() > 0.5 and np.abs(comps[1] - comps[2]).max() > 0.5


def test_noise_refusals(lib):
    d = Dev(lib, (100,), np.float64)
    img = S.image(d.lay, 1)
    arr = d.array(1, img)
    with pytest.raises(ValueError):
        lib.add_gaussian_noise(d.info.ref, 1, None, 1.0, 1, 2, 3, None)
    with pytest.raises(ValueError):
        lib.add_gaussian_noise(d.info.ref, 0, arr.ptr, 1.0, 1, 2, 3, None)
    _same(d.read(arr), img, "a refused call wrote", d.lay)


# ---- pdehip_field_product -----------------------------------------------------------------------------------------------
def _whole(lay, data):
    """An allocation image whose components hold ``data`` (``(ncomp, pc)``) and whose slack holds the pattern."""
    img = S.image(lay, data.shape[0])
    img[: data.size] = data.ravel()
    return img


@pytest.mark.parametrize("kind", S.PRODUCT_KINDS)
@pytest.mark.parametrize("shape", S.PRODUCT_SHAPES)
def test_field_product(lib, shape, kind):
    """Bit equality with the documented order of the sums (the library is built without FMA contraction), real and planar complex data,
    with and without the conjugate, both types.  The kernel multiplies every element of a component, ghost cells and padding included, so
    the whole component is compared and the slack keeps the pattern."""
    for cplx, conj in ((0, 0), (0, 1), (1, 0), (1, 1)):
        for dtype in DTYPES:
            _check_product(lib, shape, kind, cplx, conj, dtype)


def _check_product(lib, shape, kind, cplx, conj, dtype):
    d = Dev(lib, shape, dtype)
    lay, dim, w = d.lay, len(shape), 2 if cplx else 1
    a, b = S.product_operands(lay, kind, dim, bool(cplx))
    nout = S.product_entries(kind, dim)[2] * w
    img_a, img_b, img_o = _whole(lay, a), _whole(lay, b), S.image(lay, nout)
    da, db, do = d.array(a.shape[0], img_a), d.array(b.shape[0], img_b), d.array(nout, img_o)
    lib.field_product(d.info.ref, kind, cplx, conj, da.ptr, db.ptr, do.ptr, None)
    ref = S.np_field_product(kind, dim, bool(cplx), bool(conj), a, b)
    assert ref.shape == (nout, lay.pc)
    _same(d.read(do), _whole(lay, ref), f"field_product kind {kind}, complex {cplx}, conjugate {conj}, {np.dtype(dtype).name}, against the documented order (whole allocation)", lay)
    _same(d.read(da), img_a, "field_product wrote its first operand", lay)
    _same(d.read(db), img_b, "field_product wrote its second operand", lay)


def test_field_product_refusals(lib):
    d = Dev(lib, (7, 9), np.float64)
    img = S.image(d.lay, 4)
    a, b, out = d.array(4, img), d.array(4, img), d.array(4, img)
    for kind in (-1, 5):
        with pytest.raises(ValueError):
            lib.field_product(d.info.ref, kind, 0, 0, a.ptr, b.ptr, out.ptr, None)
    for args in ((None, b.ptr, out.ptr), (a.ptr, None, out.ptr), (a.ptr, b.ptr, None), (a.ptr, b.ptr, a.ptr), (a.ptr, b.ptr, b.ptr)):
        with pytest.raises(ValueError):
            lib.field_product(d.info.ref, 3, 0, 0, *args, None)
    for arr in (a, b, out):
        _same(d.read(arr), img, "a refused call wrote", d.lay)


# ---- pdehip_axis_derivative ---------------------------------------------------------------------------------------------
def _check_axis(lib, shape, axis, order, method, layout, dtype):
    dx = S.AXIS_DX[: len(shape)]
    d = Dev(lib, shape, dtype, dx)
    lay = d.lay
    nd = len(shape)
    full = S.field(shape, 1, dtype, seed=7)
    img_in = S.place(S.image(lay, 1), lay, 1, full)
    twin = O.axis_derivative(d.info.c, full[0], axis, order, method, _abi.OUT_VALID)
    ref = S.np_axis_derivative(shape, dx, full[0], axis, order, method)
    assert np.array_equal(S.bits(twin), S.bits(ref)) and np.abs(ref).max() > 0.1
    din = d.array(1, img_in)
    if layout == _abi.OUT_FULL:
        img_out = S.image(lay, 1)
        dout = d.array(1, img_out)
        lib.axis_derivative(d.info.ref, axis, order, _abi.METHODS[method], din.ptr, dout.ptr, layout, None)
        padded = np.zeros((1, *lay.full_shape), dtype)
        padded[(0, *S.interior(nd))] = twin
        want = S.place(img_out.copy(), lay, 1, padded, S.interior(nd))
        _same(d.read(dout), want, f"axis_derivative along axis {axis}, order {order}, {method}, {np.dtype(dtype).name}: the full output (whole allocation)", lay)
    else:
        stage = S.pattern(lay.cells + S.SENTINELS, dtype, sign=1.0)
        dout = _buffer(lib, stage)
        lib.axis_derivative(d.info.ref, axis, order, _abi.METHODS[method], din.ptr, dout.ptr, layout, None)
        want = stage.copy()
        want[: lay.cells] = twin.ravel()
        _same(_read(lib, dout, stage), want, f"axis_derivative along axis {axis}, order {order}, {method}, {np.dtype(dtype).name}: the valid output and its sentinels")
    _same(d.read(din), img_in, "axis_derivative wrote its operand", lay)


@pytest.mark.parametrize("layout", [_abi.OUT_VALID, _abi.OUT_FULL], ids=["valid", "full"])
@pytest.mark.parametrize("shape,axis", sorted({(shape, axis) for shape, axis, _, _ in S.axis_cases()}))
def test_axis_derivative(lib, shape, axis, layout):
    """Order 1 by the three methods and order 2, both types."""
    for order, method in S.AXIS_RULES:
        for dtype in DTYPES:
            _check_axis(lib, shape, axis, order, method, layout, dtype)


@pytest.mark.parametrize("axis,order,method,layout,dtype", [(1, 2, "central", _abi.OUT_FULL, np.float64), (0, 1, "forward", _abi.OUT_VALID, np.float32)])
def test_axis_derivative_beyond_the_turn(lib, axis, order, method, layout, dtype):
    _check_axis(lib, S.AXIS_TURN_SHAPE, axis, order, method, layout, dtype)


def test_axis_derivative_refusals(lib):
    d = Dev(lib, (33, 130), np.float64)
    img = S.image(d.lay, 1)
    a, out = d.array(1, img), d.array(1, img)
    for axis, order, method, layout in ((2, 1, 0, 1), (-1, 1, 0, 1), (0, 3, 0, 1), (0, 0, 0, 1), (0, 1, 3, 1), (0, 1, -1, 1), (0, 1, 0, 2)):
        with pytest.raises(ValueError):
            lib.axis_derivative(d.info.ref, axis, order, method, a.ptr, out.ptr, layout, None)
    with pytest.raises(ValueError):
        lib.axis_derivative(d.info.ref, 0, 1, 0, None, out.ptr, 1, None)
    with pytest.raises(ValueError):
        lib.axis_derivative(d.info.ref, 0, 1, 0, a.ptr, None, 1, None)
    _same(d.read(out), img, "a refused call wrote", d.lay)
