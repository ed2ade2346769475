"""The references of ``tests/small_kernel_cases.py`` against the CPU oracle, and the conditions that keep the cases of
``tests/test_hip_small_kernels.py`` from being vacuous.  No GPU.

Where the oracle has the operation (``O.set_ghost_cells``, ``oracle_add_gaussian_noise``, ``O.axis_derivative``) the numpy
restatement has to give its bits (the noise: its values inside `S.NOISE_TWIN_BOUND`, the two differ in libm only).  The
layout copies and the field product have no oracle twin: the layout rule is tied to ``O.valid_to_full`` and to its own
inverse, the product's restatement to ``np.einsum`` inside a running error bound.
"""

from __future__ import annotations

import numpy as np
import pytest
import small_kernel_cases as S

from oracle import pde_oracle as O
from pde_hip import _abi


def _grid(shape, dtype, dx=None):
    return _abi.make_grid(shape, dx if dx is not None else (1.0,) * len(shape), dtype)


# ---- the layout rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("shape", sorted(set(S.GHOST_SHAPES + S.COPY_SHAPES + S.NOISE_SHAPES + S.PRODUCT_SHAPES + S.AXIS_SHAPES)))
def test_layout_rule(shape, dtype):
    lay = S.Layout(shape, dtype)
    nd = len(shape)
    idx = lay.index_full()
    assert idx.shape == lay.full_shape and np.unique(idx).size == idx.size and idx.min() >= 0 and idx.max() < lay.pc
    # the first interior cell of every row on a 128-byte line, the pitch a multiple of 128 bytes, no row reaching into the next
    inner = lay.index_valid()
    assert inner[(0,) * nd] == lay.off and lay.p1 * lay.dtype.itemsize % 128 == 0
    assert np.all(inner[..., 0] * lay.dtype.itemsize % 128 == 0)
    assert lay.lpad + shape[-1] + 1 <= lay.p1 < 2 * lay.lpad + shape[-1] + 1
    # the compact full array the reference embeds valid data in: placed and gathered again it is itself
    valid = np.arange(1, 3 * lay.cells + 1, dtype=dtype).reshape(3, *shape)
    full = O.valid_to_full(shape, valid)
    img = S.place(S.image(lay, 3), lay, 3, full)
    assert np.array_equal(S.gather(img, lay, 3), full)
    assert np.array_equal(img[:3 * lay.pc].reshape(3, -1)[:, inner], valid)
    mask = S.interior_mask(lay, 3)
    assert mask.sum() == 3 * lay.cells and np.array_equal(img[~mask & (img >= 0)], np.zeros(3 * (lay.full_cells - lay.cells), dtype))
    assert not mask[3 * lay.pc:].any()


def test_the_pattern_is_distinct_and_exact():
    for dtype in S.DTYPES:
        p = S.pattern(5_000_000, dtype)
        assert np.all(np.diff(p.astype(np.float64)) == -1) and np.isfinite(p).all()
    with pytest.raises(AssertionError):
        S.pattern(2**24, np.float32)


# ---- ghost cells --------------------------------------------------------------------------------------------------------
def _ghost_reference(shape, ncomp, variant, dtype):
    faces = S.ghost_faces(shape, ncomp, variant)
    full = S.field(shape, ncomp, dtype, seed=len(shape))
    ref = S.np_set_ghost_cells(shape, ncomp, faces, full.copy())
    twin = full.copy()
    O.set_ghost_cells(_grid(shape, dtype), ncomp, S.face_table(faces), twin)
    return faces, full, ref, twin


@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("ncomp", S.GHOST_NCOMP)
@pytest.mark.parametrize("variant", S.GHOST_VARIANTS)
def test_ghost_restatement_is_the_oracle(variant, ncomp, dtype):
    for shape in S.GHOST_SHAPES:
        faces, full, ref, twin = _ghost_reference(shape, ncomp, variant, dtype)
        assert np.array_equal(S.bits(ref), S.bits(twin)), (shape, variant)
        # only face cells change: interior, edges and corners stay
        changed = S.bits(ref) != S.bits(full)
        nd = len(shape)
        for comp in range(ncomp):
            assert not changed[comp][S.interior(nd)].any()
            ghost_axes = sum(np.indices(changed[comp].shape)[a] % (shape[a] + 1) == 0 for a in range(nd))
            assert not changed[comp][ghost_axes >= 2].any()
        if variant == "normal_scalar" or variant == "normal_array":
            assert not changed[nd:].any() and (nd > ncomp or changed[:nd].any())
        else:
            assert changed.any()


def test_ghost_cases_are_not_vacuous():
    for shape in S.GHOST_SHAPES:
        for ncomp in (3, 9):
            for variant in ("o1_array", "o2_array", "six", "skip"):
                assert S.arrays_differ_between_components(S.ghost_faces(shape, ncomp, variant)), (shape, ncomp, variant)
        # the six faces of a 3-D grid are six different conditions
        if len(shape) == 3:
            six = S.ghost_faces(shape, 3, "six")
            assert len({(f["kind"], f["flags"]) for f in six}) == 6
            kinds = {(f["kind"], f["flags"]) for v in S.GHOST_VARIANTS for f in S.ghost_faces(shape, 3, v)}
            every = {(k, fl) for k in (_abi.BC_ORDER1, _abi.BC_ORDER2) for fl in (0, 1, 2, 3)}
            assert every <= kinds and (_abi.BC_SKIP, 0) in kinds
        far = S.ghost_faces(shape, 1, "far")
        assert {f["f1"] for f in far} == {1.0, -1.0}
        for a in range(len(shape)):
            assert far[2 * a]["index1"] == shape[a] - 1 and far[2 * a + 1]["index1"] == 0
    # a wrong order-2 index shows only where index2 differs from index1
    assert any(f["index1"] != f["index2"] for f in S.ghost_faces((3, 5, 7), 3, "o2_array"))


def test_ghost_turn_case():
    shape, ncomp = S.GHOST_TURN_CASE
    faces = S.ghost_faces(shape, ncomp, "turn")
    items, total = S.ghost_items(shape, ncomp, faces)
    assert total == 1_089_856 and total > S.GHOST_TURN
    assert sum(count for a, _, _, count in items if a == 0) == 1_073_280
    beyond = {a for a, _, start, count in items if start + count > S.GHOST_TURN}
    assert beyond == {0, 1, 2}, "items of at least two axes lie beyond the turn"
    assert [(a, side) for a, side, _, _ in items] == [(0, 1), (0, 0), (1, 1), (1, 0), (2, 1), (2, 0)]
    x_upper, x_lower = faces[1], faces[0]
    assert x_upper["kind"] == x_lower["kind"] == _abi.BC_ORDER2 and x_upper["flags"] == x_lower["flags"] == _abi.BCF_ARRAYS
    flags = [f["flags"] for f in faces[2:]]
    assert 0 in flags and _abi.BCF_ARRAYS in flags
    assert S.arrays_differ_between_components(faces)
    full = S.field(shape, ncomp, np.float64, seed=5)
    ref = S.np_set_ghost_cells(shape, ncomp, faces, full.copy())
    twin = full.copy()
    O.set_ghost_cells(_grid(shape, np.float64), ncomp, S.face_table(faces), twin)
    assert np.array_equal(S.bits(ref), S.bits(twin))


# ---- layout copies ------------------------------------------------------------------------------------------------------
def test_copy_expectations():
    for shape in S.COPY_SHAPES:
        for dtype in S.DTYPES:
            lay = S.Layout(shape, dtype)
            ncomp = 3
            img = S.image(lay, ncomp)
            for mode in range(4):
                count = ncomp * (lay.cells if mode < 2 else lay.full_cells)
                stage = S.pattern(count + S.SENTINELS, dtype, sign=1.0)
                img2, stage2 = S.copy_expect(mode, lay, ncomp, img, stage)
                assert np.array_equal(stage2[count:], stage[count:])
                if mode in (0, 2):
                    assert np.array_equal(stage2, stage) and (img2 > 0).sum() == count
                    assert np.array_equal(img2[img2 > 0], stage[:count])   # in memory order: C order of the compact array
                    if mode == 0:
                        assert np.array_equal(img2 > 0, S.interior_mask(lay, ncomp))
                    else:   # every cell of the compact array, corners included, and no padding
                        cols = (np.flatnonzero(img2 > 0) % lay.p1)
                        assert cols.min() == lay.lpad - 1 and cols.max() == lay.lpad + shape[-1]
                        assert np.array_equal(S.gather(img2, lay, ncomp).ravel(), stage[:count])
                else:
                    assert np.array_equal(img2, img) and (stage2[:count] < 0).all() and np.unique(stage2[:count]).size == count
    lay = S.Layout(S.COPY_TURN_SHAPE, np.float64)
    assert lay.cells == 4_276_350 > S.CHUNK_TURN and lay.full_cells == 132 * 131 * 257 > S.CHUNK_TURN


# ---- noise --------------------------------------------------------------------------------------------------------------
_twin_noise = S.oracle_add_noise


def test_philox_known_answers():
    """Random123's known-answer vectors of philox4x32-10 (kat_vectors): counter and key all zero, all ones, and the digits of pi."""
    def run(ctr, key):
        cell, counter, seed = ctr[0] | ctr[1] << 32, ctr[2] | ctr[3] << 32, key[0] | key[1] << 32
        return tuple(int(w[0]) for w in S.philox4x32_10(np.array([cell], dtype=np.uint64), counter, seed))

    assert run((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    f = 0xFFFFFFFF
    assert run((f, f, f, f), (f, f)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert run((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_noise_restatement_against_the_twin(capsys):
    worst = 0.0
    for shape in (*S.NOISE_SHAPES, S.NOISE_TURN_SHAPE):
        for ncomp in ((1,) if shape == S.NOISE_TURN_SHAPE else S.NOISE_NCOMP):
            for seed, counter, offset in S.NOISE_KEYS:
                zero = np.zeros((ncomp, *[s + 2 for s in shape]))
                ref = S.np_add_noise(shape, ncomp, zero.copy(), 1.0, seed, counter, offset)
                twin = _twin_noise(shape, ncomp, zero.copy(), 1.0, seed, counter, offset)
                worst = max(worst, float(np.abs(ref - twin).max()))
                inner = (slice(None), *S.interior(len(shape)))
                assert np.abs(ref[inner]).max() > 2 and ref[inner].std() > 0.8
                assert np.array_equal(ref == 0, twin == 0) and not (ref[inner] == 0).any()
    with capsys.disabled():
        print(f"\nnoise: twin against restatement, largest difference {worst:.3e} (bound {S.NOISE_TWIN_BOUND:.0e})")
    assert worst <= S.NOISE_TWIN_BOUND
    # base value, scale and the rounding of fp32 fields: (T)((double)y + scale * xi)
    for dtype in S.DTYPES:
        full = S.noise_field((37, 129), 2, dtype)
        seed, counter, offset = S.NOISE_KEYS[1]
        ref = S.np_add_noise((37, 129), 2, full.copy(), S.NOISE_SCALE, seed, counter, offset)
        twin = _twin_noise((37, 129), 2, full.copy(), S.NOISE_SCALE, seed, counter, offset)
        assert np.abs(ref.astype(np.float64) - twin).max() <= S.NOISE_ATOL[np.dtype(dtype)]
        assert ref.dtype == dtype and np.array_equal(ref[:, 0], full[:, 0])


def test_noise_keys_are_not_vacuous():
    assert any(seed >> 32 for seed, _, _ in S.NOISE_KEYS) and any(counter >> 32 for _, counter, _ in S.NOISE_KEYS)
    straddle = [k for k in S.NOISE_KEYS if k[2] == 2**32 - 5]
    assert straddle
    for shape in (*S.NOISE_SHAPES, S.NOISE_TURN_SHAPE):
        for ncomp in S.NOISE_NCOMP:
            hi = S.noise_cells(shape, ncomp, straddle[0][2]) >> np.uint64(32)
            assert set(np.unique(hi[0]).tolist()) == {0, 1}, "the cells of one component lie on both sides of the carry"
    # each word matters: another upper word of seed, counter or cell number gives another field
    cell = S.noise_cells((100,), 1, 11)
    base = S.np_normal(cell, 5, 99)
    for other in (S.np_normal(cell, 5, 99 + 2**32), S.np_normal(cell, 5 + 2**32, 99), S.np_normal(cell + np.uint64(2**32), 5, 99)):
        assert np.abs(other - base).max() > 1
    # one call for three components draws what three calls with shifted offsets draw
    shape = (6, 5, 131)
    cells = int(np.prod(shape))
    seed, counter, offset = S.NOISE_KEYS[2]
    whole = S.np_normal(S.noise_cells(shape, 3, offset), counter, seed)
    for k in range(3):
        assert np.array_equal(whole[k], S.np_normal(S.noise_cells(shape, 1, offset + k * cells), counter, seed)[0])
    assert np.abs(whole[0] - whole[1]).max() > 1 and np.abs(whole[1] - whole[2]).max() > 1
    assert int(np.prod(S.NOISE_TURN_SHAPE)) > S.CHUNK_TURN


# ---- field product ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("cplx,conj", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("kind", S.PRODUCT_KINDS)
def test_product_restatement_against_einsum(kind, cplx, conj, dtype):
    for shape in S.PRODUCT_SHAPES:
        dim = len(shape)
        lay = S.Layout(shape, dtype)
        a, b = S.product_operands(lay, kind, dim, cplx)
        ref = S.np_field_product(kind, dim, cplx, conj, a, b)
        ein = S.einsum_field_product(kind, dim, cplx, conj, a, b)
        assert ref.shape == ein.shape and ref.dtype == dtype
        # either order is a sum of `dim` complex products: at most 4 * dim + 4 roundings, each at most 2**-53 of the sum of the
        # magnitudes (|ar| + |ai|) (|br| + |bi|) over the contracted index; then one rounding to the storage type
        w = 2 if cplx else 1
        mod = [np.abs(x.astype(np.float64)).reshape(-1, w, x.shape[1]).sum(axis=1) for x in (a, b)]
        mag = np.repeat(S.np_field_product(kind, dim, False, False, *mod), w, axis=0)
        bound = 2 * (4 * dim + 4) * 2.0**-53 * mag + (2.0**-24 if dtype == np.float32 else 0.0) * mag
        assert np.all(np.abs(ref.astype(np.float64) - ein) <= bound)
        assert np.abs(ref).max() > 0.5
        if cplx:   # the conjugate matters
            other = S.np_field_product(kind, dim, True, not conj, a, b)
            assert (S.bits(other) != S.bits(ref)).mean() > 0.4
        if not cplx:   # real data: the flag is not read
            assert np.array_equal(S.bits(S.np_field_product(kind, dim, False, True, a, b)), S.bits(ref))


# ---- axis derivative ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES)
def test_axis_restatement_is_the_oracle(dtype):
    for shape, axis, order, method in S.axis_cases():
        dx = S.AXIS_DX[: len(shape)]
        full = S.field(shape, 1, dtype, seed=7)[0]
        g = _grid(shape, dtype, dx)
        ref = S.np_axis_derivative(shape, dx, full, axis, order, method)
        for layout in (_abi.OUT_VALID, _abi.OUT_FULL):
            twin = O.axis_derivative(g, full, axis, order, method, layout)
            got = twin if layout == _abi.OUT_VALID else twin[S.interior(len(shape))]
            assert np.array_equal(S.bits(ref), S.bits(got)), (shape, axis, order, method, layout)
        assert np.abs(ref).max() > 0.1
    assert int(np.prod(S.AXIS_TURN_SHAPE)) > S.CHUNK_TURN
    covered = {(len(shape), axis) for shape, axis, _, _ in S.axis_cases()}
    assert covered == {(3, 0), (3, 1), (3, 2), (2, 0), (2, 1), (1, 0)}
