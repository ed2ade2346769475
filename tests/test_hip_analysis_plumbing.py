"""Device test of what the analysis kernels share (``csrc/pdehip_scratch.h``, ``dispatch_piece`` and ``piece_width`` of
``csrc/pdehip_pieces.h``): one call of every family on a second stream, at the four fields where the choice of the kernel instance takes
each of its branches, before and after ``pdehip_release_scratch``.

Nothing is restated here: inputs, drivers, numpy restatements and expected instance names are those of ``stats_cases.py``,
``hist_cases.py``, ``project_cases.py``, ``smooth_cases.py`` and ``domains_cases.py``.
"""

from __future__ import annotations

import ctypes as C
import math

import domains_cases as D
import hist_cases as H
import numpy as np
import project_cases as P
import pytest
import smooth_cases as SM
import stats_cases as S

import pde_hip

pytestmark = pytest.mark.gpu

# (type, shape, cells per access): <double,2>, <double,1> (an odd row), <float,4>, <float,1> (a row that is no multiple of four)
FIELDS = ((np.float64, (3, 4, 8), 2), (np.float64, (3, 4, 7), 1), (np.float32, (3, 4, 8), 4), (np.float32, (3, 4, 6), 1))
THRESHOLD = 1.0                      # between the two bands of stats_cases.draw
PERIODIC = (True, False, True)
NBINS = 7
MASK = 0b001                         # axis 0 is removed: the march kernel, whose lanes take VEC cells of the fastest axis
WEIGHTS = SM.radius_weights(2)


@pytest.fixture(scope="module")
def lib():
    return pde_hip.get_backend("hip")._lib


def one_round(lib, stream, valid, last_host, shape, vec):
    """One call of each family on ``stream``; every result as a list of arrays, the instance names checked on the way."""
    dtype = valid.dtype
    kind = "double" if dtype == np.float64 else "float"
    dev = S.upload(lib, shape, valid)
    last = S.upload(lib, shape, last_host)          # (the steady-state sweep moves the snapshot on: a fresh one per round)
    smoothed = SM.sentinel_array(lib, dev)
    lib.stream_synchronize(None)
    out = {}

    out["stats"] = S.field_stats(lib, dev, stream=stream)
    assert P.kernel_name(lib) == f"stats_sweep_kernel<{kind},{vec},0>"
    out["steady"] = S.steady_state(lib, dev, last, stream=stream)
    assert P.kernel_name(lib) == f"steady_sweep_kernel<{kind},{vec}>"
    out["snapshot"] = last.get_valid(stream=stream)
    out["counts"] = H.histogram(lib, dev, H.equal_edges(NBINS, dtype), stream=stream)
    assert P.kernel_name(lib) == f"hist_sweep_kernel<{kind},{vec},0,1>"
    out["lower"], out["upper"], out["ranks"] = H.select(lib, dev, H.QS, stream=stream)
    assert P.kernel_name(lib) == f"select_sweep_kernel<{kind},{vec},0>"
    out["sum"] = P.project(lib, dev, MASK, P.SUM, stream=stream)
    assert P.kernel_name(lib) == P.expected_chain(shape, dtype, MASK, P.SUM) == f"project_march_kernel<{kind},{vec},sum>"
    SM.smooth_axis(lib, dev, smoothed, 0, WEIGHTS, SM.WRAP, stream=stream)
    assert P.kernel_name(lib) == SM.expected_instance(shape, dtype, 0, len(WEIGHTS) - 1) == f"gauss_march_kernel<{kind},{vec}>"
    out["smoothed"] = smoothed.get_valid(stream=stream)
    lo, hi = D.interval_bounds(dtype, THRESHOLD)
    out["labels"], out["info"], labels_dev = D.label(lib, D.upload(lib, valid[0]), lo, hi, 1, PERIODIC, stream=stream)
    out["sizes"] = D.sizes(lib, labels_dev, math.prod(shape), int(out["info"][0]), stream=stream)
    return out


@pytest.mark.parametrize(("dtype", "shape", "vec"), FIELDS, ids=["f64x2", "f64x1", "f32x4", "f32x1"])
def test_every_family_on_a_second_stream_around_release_scratch(lib, dtype, shape, vec):
    assert S.vec_width(dtype, shape[-1]) == vec
    valid = S.draw(shape, 1, dtype, seed=5)
    last_host = (valid * dtype(1.001)).astype(dtype)
    stream = C.c_void_p()
    lib.stream_create(C.byref(stream))
    try:
        first = one_round(lib, stream, valid, last_host, shape, vec)
        lib.stream_synchronize(stream)
        lib.release_scratch()
        second = one_round(lib, stream, valid, last_host, shape, vec)
    finally:
        lib.stream_synchronize(stream)
        lib.stream_destroy(stream)
    assert sorted(first) == sorted(second)
    for name in first:
        a, b = np.ascontiguousarray(first[name]), np.ascontiguousarray(second[name])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{name}: the rounds before and after release_scratch differ"

    got = first
    S.check_stats(got["stats"], S.expect_stats(valid), what="stats")
    S.check_steady(got["steady"], S.np_steady(valid, last_host), what="steady")
    np.testing.assert_array_equal(S.bits(got["snapshot"]), S.bits(valid), err_msg="the snapshot did not move on to the state")
    H.check_counts(got["counts"], valid, H.equal_edges(NBINS, dtype), what="histogram")
    H.check_select((got["lower"], got["upper"], got["ranks"]), valid, H.QS, what="select")
    P.check_sum(got["sum"], valid, MASK, what="project")
    SM.assert_same(got["smoothed"], SM.filter_axis(valid, 0, WEIGHTS, SM.WRAP), "smooth")
    e_labels, e_k, e_fg, e_sizes = D.reference(valid[0] > dtype(THRESHOLD), PERIODIC, 1)
    np.testing.assert_array_equal(got["info"], np.array([e_k, e_fg], dtype=np.uint64), err_msg="K, foreground")
    np.testing.assert_array_equal(got["labels"], e_labels, err_msg="labels")
    np.testing.assert_array_equal(got["sizes"], e_sizes, err_msg="sizes")
    assert e_k >= 1
