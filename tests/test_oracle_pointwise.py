"""Pin the oracle twins of the pointwise and reduction operations against plain numpy restatements (CPU only).

``tests/test_hip_pointwise.py`` compares the device kernels bit for bit with the oracle AND with these restatements
(``tests/pointwise_cases.py``: float64, left to right, rounded once); this module keeps the two references tied to each
other without a GPU, so that a drift of the oracle cannot carry the device comparison along.  Everything is bit-exact:
the operations are elementwise or a maximum, and ``oracle_integrate`` is the sequential sum that ``np.cumsum`` performs.
"""

from __future__ import annotations

import numpy as np
import pytest
import pointwise_cases as P

from oracle import pde_oracle as O
from pde_hip import _abi

DTYPES = [np.float64, np.float32]


def _grid(shape, dtype):
    return _abi.make_grid(shape, (1.0,) * len(shape), dtype)


def _same(got, ref):
    np.testing.assert_array_equal(P.bits(np.ascontiguousarray(got)), P.bits(np.ascontiguousarray(ref)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,ncomp", P.SMALL)
def test_combine_twins(shape, ncomp, dtype):
    g, inner = _grid(shape, dtype), P.interior(shape)
    y, k1, k2, k3, k4, k5, k6 = P.fields(shape, ncomp, dtype, 7, seed=1)
    ks = [k1, k2, k3, k4, k5, k6]
    coefs = [0.25, -1.5, 3.0, 1 / 3, -0.7, 1e-3]
    for nk in range(1, 7):
        _same(O.lincomb(g, ncomp, y, coefs[:nk], ks[:nk])[inner], P.np_lincomb(y, coefs[:nk], ks[:nk])[inner])
        _same(O.lincomb(g, ncomp, None, coefs[:nk], ks[:nk])[inner], P.np_lincomb(None, coefs[:nk], ks[:nk])[inner])
    _same(O.rk4_combine(g, ncomp, y.copy(), k1, k2, k3, k4)[inner], P.np_rk4(y, k1, k2, k3, k4)[inner])
    _same(O.ab2_combine(g, ncomp, y.copy(), k1, k2, 0.37)[inner], P.np_ab2(y, k1, k2, 0.37)[inner])
    ynew, err = O.rkf45_combine(g, ncomp, y, ks)
    ynew_np, err_np = P.np_rkf45(y, ks, inner)
    _same(ynew[inner], ynew_np[inner])
    assert P.f64_bits(err) == P.f64_bits(err_np)
    small, err = O.euler_adaptive_combine(g, ncomp, y, k1, 0.37, k2, k3)
    small_np, err_np = P.np_euler_adaptive(y, k1, 0.37, k2, k3, inner)
    _same(small[inner], small_np[inner])
    assert P.f64_bits(err) == P.f64_bits(err_np)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,ncomp", P.SMALL)
def test_norm_and_reduction_twins(shape, ncomp, dtype):
    g, inner = _grid(shape, dtype), P.interior(shape)
    a, b = P.fields(shape, ncomp, dtype, 2, seed=2)
    assert P.f64_bits(O.max_abs_diff(g, ncomp, a, b)) == P.f64_bits(P.np_max_abs_diff(a, b, inner))
    assert O.max_abs_diff(g, ncomp, a, a) == 0.0
    pairs = P.pair_fields(shape, ncomp, dtype, seed=2)   # 2 * ncomp components: ncomp complex numbers per cell, exact moduli
    assert P.f64_bits(O.max_abs_pairs(g, ncomp, pairs)) == P.f64_bits(P.np_max_abs_pairs(pairs, inner))
    _same(O.integrate(g, ncomp, a, 0.37), P.np_integrate_sequential(a, 0.37, inner))
    exact, mag = P.fsum_integrate(a, 0.37, inner)
    cells = int(np.prod(shape))
    assert np.all(np.abs(O.integrate(g, ncomp, a, 0.37) - exact) <= cells * 2.0 ** -53 * mag)   # one rounding per product and sum
    bad = a.copy()
    flat = bad[inner].reshape(ncomp, -1).copy()
    special = [np.finfo(dtype).max, -np.finfo(dtype).max, np.finfo(dtype).smallest_subnormal, np.nan, np.inf, -np.inf]
    for c in range(ncomp):
        for q, v in enumerate(special):   # (on the smallest grids a later value replaces an earlier one)
            flat[c, (q + c) % flat.shape[1]] = v
    bad[inner] = flat.reshape(bad[inner].shape)
    bad[:, P.ghost_mask(shape)] = np.nan   # ghost cells are not counted
    _same(O.count_nonfinite(g, ncomp, bad), P.np_count_nonfinite(bad, inner))
    assert np.all(O.count_nonfinite(g, ncomp, bad) == min(3, cells))


@pytest.mark.parametrize("dtype", DTYPES)
def test_norm_twins_order_nan_and_infinity(dtype):
    """NaN wins over infinity, a NaN with the sign bit set is a NaN, |inf + nan j| is inf (numpy's abs of a complex number)."""
    shape, ncomp = (3, 5, 7), 2
    g, inner = _grid(shape, dtype), P.interior(shape)
    a, b = P.fields(shape, ncomp, dtype, 2, seed=3)
    neg_nan = np.copysign(np.nan, -1)
    for values in ([np.inf], [np.nan], [np.inf, np.nan], [np.nan, np.inf], [neg_nan], [-np.inf]):
        x = a.copy()
        for q, v in enumerate(values):
            x[1, 2, 3 + q, 4] = v
        assert P.f64_bits(O.max_abs_diff(g, ncomp, x, b)) == P.f64_bits(P.np_max_abs_diff(x, b, inner))
        assert np.isnan(O.max_abs_diff(g, ncomp, x, b)) == any(np.isnan(v) for v in values)
    z = P.pair_fields(shape, 2, dtype, seed=3)
    z[0, 2, 3, 4], z[1, 2, 3, 4] = np.inf, np.nan
    assert O.max_abs_pairs(g, 2, z) == np.inf == P.np_max_abs_pairs(z, inner)
    z[2, 1, 1, 1], z[3, 1, 1, 1] = np.nan, 1.0
    assert P.f64_bits(O.max_abs_pairs(g, 2, z)) == P.f64_bits(P.np_max_abs_pairs(z, inner)) == P.f64_bits(np.nan)
