"""The reference and the rounding-error bound of tests/fastmath_cases.py have to earn their place before the device is held to them (no GPU here).

For every case of the table:
* the pinned oracle (``-ffp-contract=off``) lies within the bound of the reference in every cell - a mistake in the numpy restatement (order,
  coefficient, face index) shows as thousands of ulps;
* so does a really contracted build, ``oracle/libpde_oracle_fastmath.so`` (FMA contraction, reassociation, reciprocal maths; `REASSOCIATED`
  lists the one comparison that its reassociation takes out);
* the bound is sharp: corruptions of the oracle's result far below the 1e-10 of tests/test_hip_fastmath.py are rejected.
"""

from __future__ import annotations

import numpy as np
import pytest
from fastmath_cases import CASES, FAMILIES, IDS, LD, OPERATORS, SINGLE_BUILD, Built, excess, within, worst_ratio

from oracle import pde_oracle as O

INDEX = range(len(CASES))


# Comparisons with the contracted CPU build that are left out, with the flag of oracle/Makefile's FASTFLAGS that causes the miss.  The bound
# holds for any subset of fused multiply-adds in the oracle's ORDER of operations; -fassociative-math may add the three second differences of a cell
# in another order, and where they cancel (here cell (31,21,61): 6.8e-5 from terms of order 1) a partial sum of the other order is larger than any of
# the oracle's and so is its rounding: 1.02 x bound with FASTFLAGS, 1.09 x with -fassociative-math alone and -ffp-contract=off, 0.56 x with every
# flag of FASTFLAGS but that one.  The device build contracts and does not reassociate (py-pde_amd/Makefile), so it is held to the bound there.
# To see it again: empty this table and rebuild the library with `make -B -C oracle libpde_oracle_fastmath.so FASTFLAGS="<the Makefile's value
# without -fassociative-math>"` (passes), resp. `... FASTFLAGS="<its value with -ffp-contract=off for -ffp-contract=fast and without -freciprocal-math>"` (fails).
REASSOCIATED = {
    "laplace-rhs_scaled-32x32x130-64-LLL-set/mixed_faces-di-1-instance=CZ=2": "-fassociative-math",
}
assert set(REASSOCIATED) <= set(IDS)


def _compared(arr, mask):
    return arr[mask] if mask is not None else arr


@pytest.mark.parametrize("index", INDEX, ids=IDS)
def test_both_oracle_builds_lie_within_the_bound(index):
    case = CASES[index]
    built = Built(case)
    reference, mask = built.reference(), built.mask()
    exact = built.oracle()
    assert len(exact) == len(reference)
    for got, (ref, bound) in zip(exact, reference):
        assert np.shape(got) == ref.shape == bound.shape
        assert np.isfinite(np.asarray(got, dtype=np.float64)).all() and (bound >= 0).all()
        n_over, ratio = excess(got, ref, bound, mask)
        assert n_over == 0, f"the exact oracle leaves the bound in {n_over} cells (|diff| / bound up to {ratio:.3g})"
    with O.fastmath_build():
        fast = built.oracle()
    for got, (ref, bound) in zip(fast, reference):
        if case.id in REASSOCIATED:
            break
        n_over, ratio = excess(got, ref, bound, mask)
        assert n_over == 0, f"the contracted oracle leaves the bound in {n_over} cells (|diff| / bound up to {ratio:.3g})"
    # (1-D: the oracle divides, d / (2 dx), and that library is also built with -freciprocal-math, which may turn the quotient into a product:
    # `bit_equal` is a statement about contraction, which the device build alone is held to there)
    if case.bit_equal and len(case.shape) > 1:
        for a, b in zip(fast, exact):
            np.testing.assert_array_equal(_compared(a, mask), _compared(b, mask))


def _single_store(case):
    """one rounding to the array's type between the input and some result cell: a cell away from the faces exists (their ghost cells are rounded
    to the array's type too) and nothing but the result is stored"""
    if min(case.shape) < 3:
        return False
    if case.entry in OPERATORS or case.entry == "set_ghost_cells":
        return True
    return case.kind == "diffusion" and (case.entry == "rhs_scaled" or (case.steps == 1 and case.entry == "euler_multi_2d"))


@pytest.mark.parametrize("index", INDEX, ids=IDS)
def test_the_bound_rejects_corrupted_results(index):
    """1e-12 of the field's scale on one cell (fp64), a cell that holds its neighbour's value, an fp32 cell two fp32 ulps off."""
    case = CASES[index]
    built = Built(case)
    reference, mask = built.reference(), built.mask()
    exact = built.oracle()
    assert within(exact, reference, mask)
    good = np.asarray(exact[0])
    where = np.flatnonzero(mask.reshape(-1) if mask is not None else np.ones(good.size, bool))
    scale = float(np.abs(good.reshape(-1)[where]).max())
    assert scale > 0

    def rejected(flat_index, value):
        bad = good.copy()
        bad.reshape(-1)[flat_index] = value
        return not within([bad] + list(exact[1:]), reference, mask)

    flat = good.reshape(-1)
    if good.dtype == np.float64:
        cell = where[len(where) // 2]
        assert rejected(cell, flat[cell] + 1e-12 * scale), "1e-12 of the field's scale added to one cell passes the check"
    # the first compared cell whose successor in memory (its neighbour along the fastest axis) holds another value takes that value
    pairs = [(p, q) for p, q in zip(where[:-1], where[1:]) if abs(float(flat[p]) - float(flat[q])) > 1e-3 * scale]
    if np.ptp(flat[where].astype(np.float64)) > 0:     # (a periodic grid of one cell: the cell and both its ghost cells hold one value)
        assert pairs, "no two neighbouring cells differ: the case's data is degenerate"
        assert rejected(pairs[0][0], flat[pairs[0][1]]), "a cell replaced by its neighbour's value passes the check"
    if good.dtype == np.float32:
        ref, bound = reference[0]
        ulp = np.spacing(np.abs(good).astype(np.float32)).astype(LD).reshape(-1)[where]
        room = bound.reshape(-1)[where] / ulp
        cell = where[int(np.argmin(room))]
        if room.min() < 2:
            # moved AWAY from the reference the cell ends 2 ulps + |oracle - reference| from it: provably outside a bound below 2 ulps
            away = np.float32(np.inf) if LD(flat[cell]) >= ref.reshape(-1)[cell] else np.float32(-np.inf)
            moved = np.nextafter(np.nextafter(flat[cell], away), away)
            assert rejected(cell, moved), "an fp32 cell moved by two ulps passes the check"
        else:
            # every cell is fed by many roundings to fp32 (eight time levels, the stored mu, Runge-Kutta slopes): the rigorous bound itself
            # reaches two ulps there and such a move is not excluded by the arithmetic - this must not happen to a one-store case
            assert not _single_store(case), f"bound / ulp >= {float(room.min()):.2f} in every cell of a case with one storage rounding"


def test_every_family_both_types_and_every_size_limit():
    families = {c.family for c in CASES}
    assert families == set(FAMILIES) | {SINGLE_BUILD}
    for fam in FAMILIES:
        types = {c.dtype for c in CASES if c.family == fam}
        assert types == ({"float64"} if fam == "launch_euler4" else {"float64", "float32"}), fam   # (the four-step sweep is fp64 only)
    for c in CASES:
        # (the smallest grid of the unit-spacing four-step instance, and the smallest that gets the 64-column tile of the 2-D kernel: 268 290 cells)
        assert c.cells <= 200_000 or c.shape in ((33, 64, 128), (33, 8130)), c.id
        assert 1 <= c.steps <= 8
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("family", FAMILIES)
def test_the_contracted_cpu_build_is_another_build(family):
    """... or the second comparison above would say nothing: in every family some case that contraction can change has other bits"""
    for case in CASES:
        if case.family != family or case.bit_equal:
            continue
        built = Built(case)
        exact = built.oracle()
        with O.fastmath_build():
            fast = built.oracle()
        mask = built.mask()
        if any(not np.array_equal(_compared(a, mask), _compared(b, mask)) for a, b in zip(fast, exact)):
            return
    pytest.fail(f"{family}: the contracted oracle gave the exact one's bits in every case")


def test_worst_ratio_is_reported():
    """`worst_ratio` (the figure the device test prints per family) is 0 on the reference itself and 1 on its edge"""
    built = Built(CASES[0])
    reference = built.reference()
    ref, bound = reference[0]
    assert worst_ratio([ref], reference) == 0
    assert abs(worst_ratio([ref + bound], reference) - 1) < 1e-3     # (ref + bound rounds in longdouble: 2**-64 |ref| against 2**-53 |ref|)
    assert not within([ref + 2 * bound + 1e-30], reference)
