"""Device tests of ``csrc/pdehip_props.hip``: ``pdehip_domain_properties`` through the C ABI, ``field_domains(..., properties=True)`` on
device arrays, and the residency of a Cahn-Hilliard run that uses it through the mirror classes.

Reference, inputs and checks: ``tests/domain_props_cases.py``.  Every integer output is compared with ``==`` against the numpy
restatement ``pde_hip.domains.host_domain_properties``; centroids, boxes and ``sums`` bit for bit against the host path.  No tolerance.
``tests/test_domain_props_cpu.py`` runs the same drivers on the tests-only host version and holds the restatement against scipy.
"""

from __future__ import annotations

import domain_props_cases as P
import numpy as np
import pytest

import pde_hip
from pde_hip.domains import finite_absmax

pytestmark = pytest.mark.gpu

IDS = ["f64", "f32"]


@pytest.fixture(scope="module")
def backend():
    return pde_hip.get_backend("hip")


@pytest.fixture(scope="module")
def lib(backend):
    return backend._lib


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
@pytest.mark.parametrize("connectivity", [1, 3], ids=["faces", "full"])
def test_ragged_rows_all_periodic_patterns(backend, connectivity, dtype):
    """5 x 7 x 70: rows are no multiple of 64, so a wave spans rows and planes; all 8 periodic combinations."""
    data = P.smooth_field((5, 7, 70), dtype)
    counts = set()
    for per in P.all_periodic(3):
        got = P.check_field(backend, data, per, f"c{connectivity} {per}", connectivity=connectivity)
        counts.add(got.count)
    assert min(counts) >= 1 and max(counts) >= 3 and len(counts) > 1          # several domains, and the wrap joins some


def test_label_patterns(lib):
    """4 x 6 x 130 through the bare entry point: every cell its own label, A B A B ..., one label over everything, K == 0."""
    P.run_patterns(lib)


def test_beyond_the_turn(lib):
    """64 x 128 x 160 with hand-made labels: a held label carried across the turn, one handed in, one domain over all turns."""
    P.run_turn(lib)


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_one_and_two_axes(backend, dtype):
    for shape in ((200,), (9, 150)):
        data = P.smooth_field(shape, dtype, sigma=2.0)
        for per in P.all_periodic(len(shape)):
            got = P.check_field(backend, data, per, f"{shape} {per}")
            assert got.count >= 2 and got.centroids.shape == (got.count, len(shape))


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_sums(backend, dtype):
    shape = (5, 7, 70)
    for name, (data, kwargs) in P.sum_fields(shape, dtype).items():
        got = P.check_field(backend, data, (True, False, True), name, **kwargs)
        assert got.count >= 1
        if name == "inf":
            at = got.labels[np.isinf(data)]
            assert at.size == 1 and at[0] > 0
            nan = np.isnan(got.sums)
            assert nan.sum() == 1 and nan[at[0] - 1] and got.excluded[at[0] - 1] == 1 and got.excluded.sum() == 1
        else:
            assert not got.excluded.any() and np.isfinite(got.sums).all()
        if name == "zero":
            assert got.count == 1 and not got.limbs.any() and got.sums[0] == 0.0
        if name == "negative":
            assert got.count == 1 and got.sums[0] < 0.0
        if name in ("tiny", "huge"):
            assert (got.sums != 0.0).all()


def test_two_calls_give_equal_bytes(lib):
    shape = (5, 7, 70)
    data = P.smooth_field(shape, np.float64)
    labels = (1 + np.arange(data.size) % 5).astype(np.int32).reshape(shape)
    first = P.call(lib, labels, data, (True, True, False), 5, finite_absmax(data))
    again = P.call(lib, labels, data, (True, True, False), 5, finite_absmax(data))
    lib.release_scratch()
    after = P.call(lib, labels, data, (True, True, False), 5, finite_absmax(data))
    for other in (again, after):
        for key in P.RAW_KEYS:
            assert first[key].tobytes() == other[key].tobytes(), key
    assert lib.last_kernel_name().decode() == "props_sum_kernel<double,1>"


def test_refusals(lib):
    P.run_refusals(lib)


def test_labels_out_of_range(lib):
    P.run_labels_out_of_range(lib)
    labels = np.array([0, 1, 9, -1, 5], dtype=np.int32)
    with pytest.raises(ValueError, match="3 cells"):
        P.call(lib, labels, np.ones(5), (False,), 2, 1.0)


def test_domain_properties_of_held_labels(backend):
    """``pde_hip.domain_properties`` on a FieldDomains, on its device label buffer and on its downloaded labels."""
    shape, per = (5, 7, 70), (True, False, True)
    data = P.smooth_field(shape, np.float64)
    grid = pde_hip.CartesianGrid([(-1.0, -1.0 + 0.5 * n) for n in shape], shape, periodic=list(per))
    dev = P.device_array(backend, grid, data)
    found = backend.make_domain_labeller(grid)(dev, properties=True)
    plain = backend.make_domain_labeller(grid)(dev)
    with pytest.raises(AttributeError, match="properties=True"):
        plain.centroids
    for labels in (plain, plain.labels_device, plain.labels):
        again = pde_hip.domain_properties(labels, dev, grid=grid, backend=backend)
        P.same_properties(again, found)
        np.testing.assert_array_equal(again.sizes, found.sizes)
    bare = pde_hip.domain_properties(plain, grid=grid, backend=backend)          # no field: no sums
    np.testing.assert_array_equal(bare.centroids, found.centroids)
    with pytest.raises(AttributeError, match="no sums"):
        bare.sums


def test_properties_in_a_callback_download_nothing():
    """A Cahn-Hilliard run of a few steps on (16, 16, 64); the tracker asks for the properties between the stepper calls: the state stays
    on the device and the results are the host path's on a side copy."""
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.UnitGrid([16, 16, 64], periodic=True)
    state = pde_hip.ScalarField.random_uniform(grid, -1.0, 1.0, rng=np.random.default_rng(2))
    seen = []

    def callback(field, t):
        link = field.__dict__.get("_hip_link")
        if link is None or not link.host_stale:
            return
        got = pde_hip.field_domains(field, 0.0, properties=True)
        assert got.on_device and link.downloads == 0
        side = pde_hip.ScalarField(grid, link.dev_state.get_valid())          # a side copy: not a download of the field
        host = pde_hip.field_domains(side, 0.0, properties=True)
        assert not host.on_device
        np.testing.assert_array_equal(got.labels, host.labels)
        P.same_properties(got, host, f"t = {t}")
        seen.append((t, got.count))

    res = pde_hip.CahnHilliardPDE().solve(state, t_range=1e-2, dt=1e-3, solver="euler", backend=backend, tracker=callback, interval=2e-3)
    print(seen)
    assert len(seen) >= 3 and res.__dict__["_hip_link"].downloads == 0
    assert all(k >= 1 for _, k in seen)
