"""Cases and plain numpy restatements for the small kernels every run passes through before it reaches a sweep.

``ghost_kernel`` (``pdehip_set_ghost_cells``), ``layout_copy_kernel`` (``pdehip_valid_to_full`` & co), ``copy_nt_kernel``
(``pdehip_copy_nt``), ``gaussian_noise_kernel`` (``pdehip_add_gaussian_noise``), ``field_product_kernel``
(``pdehip_field_product``) and ``axis_derivative_kernel`` (``pdehip_axis_derivative``).

Shared by ``tests/test_small_kernel_cases_cpu.py`` (CPU: the restatements against the oracle, and the conditions that keep
a case from being vacuous) and ``tests/test_hip_small_kernels.py`` (GPU: the kernels against both, through the C ABI).
Pure numpy: nothing here touches a device.

The device tests compare the WHOLE allocation of an array: `Layout` restates the layout rule of ``include/pdehip.h`` /
``csrc/pdehip_common.h`` (a row is ``[pad .. pad, ghost, n2 interior cells, ghost, pad ..]``, its first interior cell at
column ``lpad = 128 bytes / itemsize``, the row pitch the next multiple of ``lpad`` at or above ``lpad + n2 + 1``, rows
and layers compact above that, 2048 elements of slack behind the last component), `image` / `place` / `gather` move
compact host arrays in and out of such an allocation, and `pattern` fills what a kernel must leave alone.
"""

from __future__ import annotations

import numpy as np

from pde_hip import _abi

ALIGN_BYTES = 128
SLACK = 2048
GHOST_TURN = 4096 * 256      # ghost_kernel: at most 4096 workgroups of 256 threads
CHUNK_TURN = 16384 * 256     # grid_blocks(): at most 16 384 workgroups (layout copies, noise, axis derivative)
DTYPES = (np.float64, np.float32)


# ---- the layout rule ----------------------------------------------------------------------------------------------------
class Layout:
    """Where the cells of a grid's full array lie in its device allocation (restated, not asked of the library)."""

    def __init__(self, shape, dtype):
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        nd = len(self.shape)
        self.n = (1,) * (3 - nd) + self.shape
        self.gh = (0,) * (3 - nd) + (1,) * nd
        self.lpad = ALIGN_BYTES // self.dtype.itemsize
        self.p1 = -(-(self.lpad + self.n[2] + 1) // self.lpad) * self.lpad
        self.p0 = self.p1 * (self.n[1] + 2 * self.gh[1])
        self.pc = self.p0 * (self.n[0] + 2 * self.gh[0])
        self.off = self.gh[0] * self.p0 + self.gh[1] * self.p1 + self.lpad
        self.layer = (self.p0, self.p1, 1)[3 - nd]
        self.full_shape = tuple(s + 2 for s in self.shape)
        self.cells = int(np.prod(self.shape, dtype=np.int64))
        self.full_cells = int(np.prod(self.full_shape, dtype=np.int64))

    def eight(self):
        """The eight numbers of ``pdehip_layout``."""
        return [self.p0, self.p1, self.pc, self.off, self.lpad, self.pc + SLACK, SLACK, self.layer]

    def nelem(self, ncomp):
        return ncomp * self.pc + SLACK

    def index_full(self):
        """Element offset inside one component of every cell of the compact full array, shape ``full_shape``."""
        m = [self.n[a] + 2 * self.gh[a] for a in range(3)]
        i, j, k = np.ogrid[0:m[0], 0:m[1], 0:m[2]]
        return (i * self.p0 + j * self.p1 + (self.lpad - 1) + k).reshape(self.full_shape)

    def index_valid(self):
        return self.index_full()[(slice(1, -1),) * len(self.shape)]


def pattern(n, dtype, sign=-1.0, base=1024):
    """``sign * (base + index)``: finite, every element different, exact in both types."""
    assert np.dtype(dtype) == np.float64 or n + base <= 2**24, "the pattern is no longer exact in fp32"
    return (sign * (base + np.arange(n, dtype=np.float64))).astype(dtype)


def image(lay, ncomp):
    return pattern(lay.nelem(ncomp), lay.dtype)


def place(img, lay, ncomp, full, where=None):
    """Write the compact full array ``(ncomp, *full_shape)`` (or the cells ``where`` of it) into the allocation image."""
    idx = lay.index_full()
    view = img[: ncomp * lay.pc].reshape(ncomp, lay.pc)
    if where is None:
        view[:, idx] = full
    else:
        view[:, idx[where]] = full[(slice(None), *where)]
    return img


def gather(img, lay, ncomp):
    return img[: ncomp * lay.pc].reshape(ncomp, lay.pc)[:, lay.index_full()]


def interior(nd):
    return (slice(1, -1),) * nd


def interior_mask(lay, ncomp):
    """True where the allocation holds an interior cell."""
    m = np.zeros(lay.nelem(ncomp), bool)
    m[: ncomp * lay.pc].reshape(ncomp, lay.pc)[:, lay.index_valid()] = True
    return m


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def field(shape, ncomp, dtype, seed, scale=2.0):
    """A compact full array of unit-order random values (ghost cells included)."""
    rng = np.random.default_rng([17, seed])
    return (scale * rng.uniform(-1, 1, (ncomp, *[s + 2 for s in shape]))).astype(dtype)


def start_image(lay, ncomp, full, where):
    """The allocation before a call: the pattern everywhere, the cells ``where`` of ``full`` in their places."""
    return place(image(lay, ncomp), lay, ncomp, full, where)


# ---- pdehip_set_ghost_cells ---------------------------------------------------------------------------------------------
GHOST_SHAPES = ((1,), (7,), (130,), (1, 33), (5, 9), (9, 65), (1, 1, 8), (3, 5, 7), (9, 4, 130))
GHOST_NCOMP = (1, 3, 9)
GHOST_VARIANTS = ("o1_scalar", "o1_array", "o2_scalar", "o2_array", "normal_scalar", "normal_array", "skip", "six", "far")
GHOST_TURN_CASE = ((4, 520, 516), 2)
# (kind, arrays, normal) of the variant "six", by slot 2 * (normalised axis) + side
_SIX = ((1, False, False), (2, True, False), (1, True, True), (2, False, False), (1, True, False), (2, True, True))


def _face(rng, shape, ncomp, axis, side, kind, arrays, normal, far=0.0):
    n = shape[axis]
    fshape = tuple(s for a, s in enumerate(shape) if a != axis)
    lead = 1 if normal else ncomp

    def coef():
        return rng.uniform(-1.5, 1.5, (lead, *fshape)) if arrays else float(rng.uniform(-1.5, 1.5))

    f = {"kind": kind, "flags": (_abi.BCF_ARRAYS if arrays else 0) | (_abi.BCF_NORMAL if normal else 0),
         "index1": n - 1 if side else 0, "index2": max(n - 2, 0) if side else min(1, n - 1), "c": coef(), "f1": coef(), "f2": 0.0}
    if kind == _abi.BC_ORDER2:
        f["f2"] = coef()
    if far:   # the link to the other side of the axis: a periodic (f = +1) or antiperiodic (f = -1) face
        f.update(index1=0 if side else n - 1, c=0.0, f1=far)
    return f


def ghost_faces(shape, ncomp, variant, seed=0):
    """The face table of a case as a list of dicts in the table's order (slot ``2 * axis + side``, side 1 = upper)."""
    rng = np.random.default_rng([23, seed, GHOST_VARIANTS.index(variant) if variant in GHOST_VARIANTS else 99])
    nd = len(shape)
    skip = {"kind": _abi.BC_SKIP, "flags": 0, "index1": 0, "index2": 0, "c": 0.0, "f1": 0.0, "f2": 0.0}
    out = []
    for a in range(nd):
        for side in (0, 1):
            slot = 2 * (3 - nd + a) + side
            if variant in ("o1_scalar", "o1_array", "o2_scalar", "o2_array"):
                f = _face(rng, shape, ncomp, a, side, 1 if variant[1] == "1" else 2, variant.endswith("array"), False)
            elif variant == "normal_scalar":
                f = _face(rng, shape, ncomp, a, side, 1 + side, False, True)
            elif variant == "normal_array":
                f = _face(rng, shape, ncomp, a, side, 2 - side, True, True)
            elif variant == "skip":
                f = dict(skip) if (a + side) % 2 == 0 else _face(rng, shape, ncomp, a, side, 1 + a % 2, side == 1, False)
            elif variant == "six":
                f = _face(rng, shape, ncomp, a, side, *_SIX[slot])
            elif variant == "far":
                f = _face(rng, shape, ncomp, a, side, 1, False, False, far=-1.0 if side else 1.0)
            elif variant == "turn":   # order-2 array faces on x, mixed scalar and array faces on y and z
                kind, arrays = ((2, True), (2, True), (1, False), (2, True), (1, True), (2, False))[slot]
                f = _face(rng, shape, ncomp, a, side, kind, arrays, False)
            else:
                raise AssertionError(variant)
            out.append(f)
    return out


def np_set_ghost_cells(shape, ncomp, faces, full):
    """``(T)(c + f1 * v[i1])``, then ``+ f2 * v[i2]`` for order 2, in float64 in that order; upper face before lower, axis by
    axis (pde/grids/boundaries/local.py:1636, :2055-2059).  ``full``: ``(ncomp, *full_shape)``, changed in place."""
    nd = len(shape)
    for a in range(nd):
        for side in (1, 0):
            f = faces[2 * a + side]
            if f["kind"] == _abi.BC_SKIP:
                continue

            def at(i, a=a):
                sl = [slice(1, -1)] * nd
                sl[a] = i
                return tuple(sl)

            normal, arrays = bool(f["flags"] & _abi.BCF_NORMAL), bool(f["flags"] & _abi.BCF_ARRAYS)
            for comp in ([a] if normal else range(ncomp)):
                if comp >= ncomp:
                    continue

                def pick(x, comp=comp, normal=normal, arrays=arrays):
                    return np.asarray(x[0 if normal else comp], dtype=np.float64) if arrays else np.float64(x)

                r = pick(f["c"]) + pick(f["f1"]) * full[comp][at(f["index1"] + 1)].astype(np.float64)
                if f["kind"] == _abi.BC_ORDER2:
                    r = r + pick(f["f2"]) * full[comp][at(f["index2"] + 1)].astype(np.float64)
                full[comp][at(shape[a] + 1 if side else 0)] = r.astype(full.dtype)
    return full


class HostArray:
    """Coefficient arrays of a face table for the oracle: they stay on the host."""

    def __init__(self, arr):
        self.arr = np.ascontiguousarray(arr, dtype=np.float64)
        self.ptr = self.arr.ctypes.data


def face_table(faces, upload=HostArray):
    """The C face table of ``ghost_faces`` built by hand; ``upload`` turns an fp64 array into an object with ``.ptr``."""
    table = _abi.FaceArray()
    keep = []
    for slot in range(2 * _abi.MAX_DIM):
        table[slot].kind = _abi.BC_SKIP
    for slot, f in enumerate(faces):
        t = table[slot]
        t.kind, t.flags, t.index1, t.index2 = f["kind"], f["flags"], f["index1"], f["index2"]
        if f["flags"] & _abi.BCF_ARRAYS:
            for name, key in (("const_arr", "c"), ("factor1_arr", "f1"), ("factor2_arr", "f2")):
                if key == "f2" and f["kind"] != _abi.BC_ORDER2:
                    continue
                keep.append(upload(np.ascontiguousarray(f[key], dtype=np.float64)))
                setattr(t, name, keep[-1].ptr)
        else:
            t.const_v, t.factor1, t.factor2 = f["c"], f["f1"], f["f2"]
    table._keepalive = keep
    return table


def ghost_items(shape, ncomp, faces):
    """``[(axis, side, first item, items)]`` in the order ``launch_ghosts`` numbers them, and the total."""
    out, total = [], 0
    for a in range(len(shape)):
        for side in (1, 0):
            if faces[2 * a + side]["kind"] == _abi.BC_SKIP:
                continue
            count = ncomp * int(np.prod([s for b, s in enumerate(shape) if b != a], dtype=np.int64))
            out.append((a, side, total, count))
            total += count
    return out, total


def arrays_differ_between_components(faces):
    """Every coefficient array of a face that is indexed by component has pairwise different components."""
    seen = 0
    for f in faces:
        if not f["flags"] & _abi.BCF_ARRAYS or f["flags"] & _abi.BCF_NORMAL:
            continue
        for key in ("c", "f1") + (("f2",) if f["kind"] == _abi.BC_ORDER2 else ()):
            x = np.asarray(f[key])
            for p in range(x.shape[0]):
                for q in range(p + 1, x.shape[0]):
                    if not np.all(x[p] != x[q]):
                        return False
                    seen += 1
    return seen > 0


# ---- layout copies ------------------------------------------------------------------------------------------------------
COPY_SHAPES = ((1,), (37,), (5, 9), (1, 33), (3, 5, 7), (4, 3, 9), (6, 5, 131))
COPY_NCOMP = (1, 3, 9)
COPY_MODES = ("valid_to_full", "full_to_valid", "hostfull_to_full", "full_to_hostfull")
COPY_TURN_SHAPE = (130, 129, 255)
SENTINELS = 64


def copy_expect(mode, lay, ncomp, img, stage):
    """(allocation, staging buffer) after the layout copy ``mode``; the staging buffer is the compact array followed by
    ``SENTINELS`` elements.  Mode 0 writes interior cells only, mode 2 every cell of the compact full array and no padding;
    modes 1 and 3 leave the allocation alone."""
    img, stage = img.copy(), stage.copy()
    idx = lay.index_valid() if mode < 2 else lay.index_full()
    count = ncomp * idx.size
    assert stage.size == count + SENTINELS
    view = img[: ncomp * lay.pc].reshape(ncomp, lay.pc)
    if mode in (0, 2):
        view[:, idx] = stage[:count].reshape(ncomp, *idx.shape)
    else:
        stage[:count] = view[:, idx].ravel()
    return img, stage


# ---- pdehip_copy_nt -----------------------------------------------------------------------------------------------------
COPY_NT_BYTES = (16, 4080, 4096, 4112, 16 * (2**20 + 1))


# ---- pdehip_add_gaussian_noise ------------------------------------------------------------------------------------------
NOISE_SHAPES = ((100,), (37, 129), (6, 5, 131))
NOISE_NCOMP = (1, 2, 3)
NOISE_TURN_SHAPE = (130, 129, 255)
NOISE_SCALE, NOISE_BASE = 0.7, 0.25
# (seed, counter, cell offset): the words the older comparison uses, then upper words that are not zero.  With the offset
# 2**32 - 5 the cells of ONE call lie on both sides of the carry into the upper word of the cell number.
NOISE_KEYS = ((99, 5, 11),
              (0x9E3779B97F4A7C15, 0x0000000100000007, 2**32 - 5),
              (0xDEADBEEF00000001, 2**40 + 3, 2**33 + 17))
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def noise_cells(shape, ncomp, offset):
    """Cell numbers ``c * cells + linear index + offset`` (modulo 2**64) as ``(ncomp, *shape)`` uint64."""
    cells = int(np.prod(shape, dtype=np.int64))
    q = np.arange(ncomp * cells, dtype=np.uint64) + np.array([offset], dtype=np.uint64)
    return q.reshape(ncomp, *shape)


def philox4x32_10(cell, counter, seed):
    """Philox4x32-10 with counter words (cell lo, cell hi, counter lo, counter hi) and key words (seed lo, seed hi), in
    uint64 arithmetic with masks: integers only, exact.  Returns the four output words as uint64 arrays."""
    cell = np.asarray(cell, dtype=np.uint64)
    one = np.ones_like(cell)
    c0, c1 = cell & _M32, cell >> _S32
    c2, c3 = one * np.uint64(counter & 0xFFFFFFFF), one * np.uint64(counter >> 32)
    k0, k1 = int(seed & 0xFFFFFFFF), int(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def np_normal(cell, counter, seed):
    """Box-Muller on the 53 upper bits of the word pairs, in numpy float64."""
    c0, c1, c2, c3 = philox4x32_10(cell, counter, seed)
    s11 = np.uint64(11)
    u1 = ((((c0 << _S32) | c1) >> s11).astype(np.float64) + 1.0) * (1.0 / 9007199254740992.0)
    u2 = (((c2 << _S32) | c3) >> s11).astype(np.float64) * (1.0 / 9007199254740992.0)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586476925286766559 * u2)


def np_add_noise(shape, ncomp, full, scale, seed, counter, offset):
    """``y = (T)((double)y + scale * xi)`` on the interior of ``full`` (``(ncomp, *full_shape)``, changed in place)."""
    inner = (slice(None), *interior(len(shape)))
    xi = np_normal(noise_cells(shape, ncomp, offset), counter, seed)
    full[inner] = (full[inner].astype(np.float64) + np.float64(scale) * xi).astype(full.dtype)
    return full


def noise_field(shape, ncomp, dtype, seed=0):
    rng = np.random.default_rng([29, seed])
    return (NOISE_BASE + rng.uniform(-1, 1, (ncomp, *[s + 2 for s in shape]))).astype(dtype)


NOISE_ATOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-6}   # tests/test_noise.py, for unit-order scales
# The twin and the restatement share every integer; they differ in the libm behind log, cos and sqrt and in nothing else.
# Each of the three is good to a few units in the last place, on values up to sqrt(2 * 53 * ln 2) = 8.6: 1e-13 is about fifty
# units in the last place of 8.6, a tenth of what the device is allowed against the twin and thirteen orders of magnitude
# below the O(1) change a wrong integer word causes.
NOISE_TWIN_BOUND = 1e-13


# ---- pdehip_field_product -----------------------------------------------------------------------------------------------
PRODUCT_SHAPES = ((9,), (7, 9), (5, 6, 130))   # dim = 1, 2, 3: the tensor dimension is the grid's
PRODUCT_KINDS = (0, 1, 2, 3, 4)                # v.v -> s, T.v -> v, v.T -> v, T.T -> T, outer v (x) v -> T


def product_entries(kind, dim):
    """Tensor entries of (a, b, out)."""
    v, t = dim, dim * dim
    return {0: (v, v, 1), 1: (t, v, v), 2: (v, t, v), 3: (t, t, t), 4: (v, v, t)}[kind]


def np_field_product(kind, dim, cplx, conj, a, b):
    """The kernel's documented order: ``re + (ar*br - ai*bi)``, ``im + (ar*bi + ai*br)``, sums over the contracted index in
    order starting from 0, one rounding to the storage type.  ``a``, ``b``: ``(entries * w, elements)`` with planar complex
    pairs (component = entry * 2 + part) when ``cplx``."""
    w = 2 if cplx else 1
    d = dim
    out = np.empty((product_entries(kind, dim)[2] * w, a.shape[1]), dtype=a.dtype)

    def term(ia, ib, re, im):
        ar, br = a[ia * w].astype(np.float64), b[ib * w].astype(np.float64)
        if not cplx:
            return re + ar * br, im
        ai, bi = a[ia * w + 1].astype(np.float64), b[ib * w + 1].astype(np.float64)
        if conj:
            bi = -bi
        return re + (ar * br - ai * bi), im + (ar * bi + ai * br)

    def put(io, re, im):
        out[io * w] = re.astype(a.dtype)
        if cplx:
            out[io * w + 1] = im.astype(a.dtype)

    zero = np.zeros(a.shape[1])
    if kind == 0:
        re, im = zero, zero
        for i in range(d):
            re, im = term(i, i, re, im)
        put(0, re, im)
    elif kind == 1:
        for i in range(d):
            re, im = zero, zero
            for j in range(d):
                re, im = term(i * d + j, j, re, im)
            put(i, re, im)
    elif kind == 2:
        for j in range(d):
            re, im = zero, zero
            for i in range(d):
                re, im = term(i, i * d + j, re, im)
            put(j, re, im)
    elif kind == 3:
        for i in range(d):
            for k in range(d):
                re, im = zero, zero
                for j in range(d):
                    re, im = term(i * d + j, j * d + k, re, im)
                put(i * d + k, re, im)
    else:
        for i in range(d):
            for j in range(d):
                put(i * d + j, *term(i, j, zero, zero))
    return out


def einsum_field_product(kind, dim, cplx, conj, a, b):
    """The same products by ``np.einsum`` on complex128 / float64 data (numpy/backend.py:285-363): another summation
    order, so close to `np_field_product`, not equal."""
    d = dim

    def cx(x):
        x = x.astype(np.float64)
        return x[0::2] + 1j * x[1::2] if cplx else x

    za, zb = cx(a), cx(b)
    if kind in (0, 4):
        za, zb = za.reshape(d, -1), zb.reshape(d, -1)
    elif kind == 1:
        za, zb = za.reshape(d, d, -1), zb.reshape(d, -1)
    elif kind == 2:
        za, zb = za.reshape(d, -1), zb.reshape(d, d, -1)
    else:
        za, zb = za.reshape(d, d, -1), zb.reshape(d, d, -1)
    if conj and cplx:
        zb = zb.conj()
    res = np.einsum({0: "i...,i...->...", 1: "ij...,j...->i...", 2: "i...,ij...->j...", 3: "ij...,jk...->ik...", 4: "i...,j...->ij..."}[kind], za, zb)
    res = res.reshape(-1, a.shape[1])
    if not cplx:
        return res
    out = np.empty((2 * res.shape[0], a.shape[1]))
    out[0::2], out[1::2] = res.real, res.imag
    return out


def product_operands(lay, kind, dim, cplx, seed=0):
    """Operands over the WHOLE component (the kernel multiplies every element of it, ghost cells and padding included)."""
    rng = np.random.default_rng([31, seed, kind])
    w = 2 if cplx else 1
    ea, eb, _ = product_entries(kind, dim)
    a = (3.0 * rng.uniform(-1, 1, (ea * w, lay.pc))).astype(lay.dtype)
    b = (0.5 * rng.uniform(-1, 1, (eb * w, lay.pc))).astype(lay.dtype)
    return a, b


# ---- pdehip_axis_derivative ---------------------------------------------------------------------------------------------
AXIS_SHAPES = ((1, 1, 8), (2, 5, 256), (7, 9, 12), (33, 130), (40,))
AXIS_TURN_SHAPE = (130, 129, 255)
AXIS_RULES = ((1, "central"), (1, "forward"), (1, "backward"), (2, "central"))
AXIS_DX = (0.7, 1.25, 0.4)


def axis_cases():
    return [(shape, axis, order, method) for shape in AXIS_SHAPES for axis in range(len(shape)) for order, method in AXIS_RULES]


def np_axis_derivative(shape, dx, full, axis, order, method):
    """pde/grids/operators/common.py:60-110, :150-190 on the interior of the compact full array ``full_shape``; float64, one
    rounding.  Returns the valid array."""
    nd = len(shape)

    def shifted(s):
        sl = [slice(1, -1)] * nd
        sl[axis] = slice(1 + s, shape[axis] + 1 + s)
        return full[tuple(sl)].astype(np.float64)

    c, l, r = shifted(0), shifted(-1), shifted(1)
    h = np.float64(dx[axis])
    if order == 2:
        v = (r - 2 * c + l) * (1 / (h * h))
    elif method == "central":
        v = (r - l) / (2 * h)
    elif method == "forward":
        v = (r - c) / h
    else:
        v = (c - l) / h
    return v.astype(full.dtype)


# ---- the oracle's twins that `oracle.pde_oracle` does not wrap, and face tables read back ---------------------------------
def oracle_add_noise(shape, ncomp, full, scale, seed, counter, offset):
    """``oracle_add_gaussian_noise`` on the compact full array ``(ncomp, *full_shape)``, in place."""
    import ctypes as C

    from oracle import pde_oracle as O

    lib = O.lib()
    lib.oracle_add_gaussian_noise.argtypes = [C.POINTER(_abi.Grid), C.c_int, C.c_void_p, C.c_double, C.c_uint64, C.c_uint64, C.c_uint64]
    g = _abi.make_grid(shape, (1.0,) * len(shape), full.dtype)
    assert full.flags.c_contiguous
    assert lib.oracle_add_gaussian_noise(C.byref(g), ncomp, full.ctypes.data, scale, seed, counter, offset) == 0
    return full


def faces_of_table(table, shape, ncomp):
    """A C face table whose coefficient arrays lie on the HOST, as the list of dicts `np_set_ghost_cells` takes."""
    import ctypes as C

    out = []
    for a in range(len(shape)):
        for side in (0, 1):
            t = table[2 * a + side]
            f = {"kind": t.kind, "flags": t.flags, "index1": t.index1, "index2": t.index2, "c": t.const_v, "f1": t.factor1, "f2": t.factor2}
            if t.flags & _abi.BCF_ARRAYS:
                lead = 1 if t.flags & _abi.BCF_NORMAL else ncomp
                fshape = tuple(s for b, s in enumerate(shape) if b != a)
                for key, name in (("c", "const_arr"), ("f1", "factor1_arr"), ("f2", "factor2_arr")):
                    if key == "f2" and t.kind != _abi.BC_ORDER2:
                        continue
                    p = C.cast(getattr(t, name), C.POINTER(C.c_double))
                    f[key] = np.ctypeslib.as_array(p, (lead * int(np.prod(fshape, dtype=np.int64)),)).reshape(lead, *fshape).copy()
            out.append(f)
    return out
