"""Domain properties without a GPU.

* the numpy restatement ``pde_hip.domains.host_domain_properties`` and the shared derivation against scipy on open grids
  (``find_objects`` exactly, ``center_of_mass`` to 1 ulp, ``math.fsum`` per label within the bound of the fixed-point sum);
* periodic grids: a compact droplet cut by one, two and three periodic faces has the centroid and box of the droplet rolled to the
  middle; a stripe that spans an axis is ``ambiguous`` there;
* the shim's sequential C version of ``pdehip_domain_properties`` (tests/props_shimlib.py) against the restatement, on the drivers of the
  GPU test (``tests/domain_props_cases.py``);
* the Python side: device and host path bit for bit, a library without the entry point, ``properties=False``.
The kernels are tested on the GPU (tests/test_hip_domain_props.py)."""

from __future__ import annotations

import itertools
import math

import domain_props_cases as P
import label_shimlib
import numpy as np
import props_shimlib
import pytest
from scipy import ndimage

import pde_hip
from pde_hip import _abi
from pde_hip.domains import PROPERTY_NAMES, derive_properties, finite_absmax, host_domain_properties, limb_exponents

IDS = ["f64", "f32"]


@pytest.fixture
def shim():
    with props_shimlib.use_shim() as lib:
        yield lib


def _props(labels, data, periodic, count=None):
    labels = np.asarray(labels)
    k = int(labels.max(initial=0)) if count is None else count
    absmax = finite_absmax(data) if data is not None else 0.0
    raw = host_domain_properties(labels, data, periodic, absmax, k)
    sizes = np.bincount(labels.ravel(), minlength=k + 1)[1:]
    ndim = labels.ndim
    return derive_properties(raw, sizes, labels.shape, periodic, [0.0] * ndim, [1.0] * ndim, absmax), sizes, absmax


def test_abi_table():
    assert _abi.ABI_VERSION == 8
    assert "domain_properties" in _abi.OPTIONAL_PROTOTYPES
    assert "domain_properties" not in set(_abi.COMPUTE_PROTOTYPES) | set(_abi.COMM_PROTOTYPES) | set(_abi.RUNTIME_PROTOTYPES)


# ---- the restatement against scipy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(200,), (9, 150), (5, 7, 70)], ids=P.D.shape_id)
def test_open_grids_against_scipy(shape):
    ndim = len(shape)
    data = P.smooth_field(shape, np.float64, sigma=2.0 if ndim < 3 else 1.0)
    mask = data > 0.0
    for conn in (1, ndim):
        labels, k = ndimage.label(mask, structure=ndimage.generate_binary_structure(ndim, conn))
        assert k >= 2
        props, sizes, _ = _props(labels, data, [False] * ndim)
        for i, obj in enumerate(ndimage.find_objects(labels)):
            np.testing.assert_array_equal(props["bounding_boxes"][i], [[s.start, s.stop - 1] for s in obj])
            np.testing.assert_array_equal(props["extents"][i], [s.stop - s.start for s in obj])
        com = np.array(ndimage.center_of_mass(mask, labels, range(1, k + 1))).reshape(k, ndim)
        assert (np.abs(props["centroids"] - com) <= np.spacing(np.abs(com))).all(), np.abs(props["centroids"] - com).max()
        assert not props["ambiguous"].any()
        touches = np.array([any(s.start == 0 or s.stop == n for s, n in zip(obj, shape)) for obj in ndimage.find_objects(labels)])
        np.testing.assert_array_equal(props["touches_boundary"], touches)


@pytest.mark.parametrize("decades", [5, 20, 35])
def test_sums_against_fsum(decades):
    """Per label within ``size * 2^(el - 1) + 3 * 2^-53 * |sum|`` of the exactly rounded sum (``math.fsum``)."""
    shape = (5, 7, 70)
    rng = np.random.default_rng(decades)
    mask = P.smooth_field(shape, np.float64) > 0.0
    data = rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-decades / 2, decades / 2, shape)
    labels, k = ndimage.label(mask)
    props, sizes, absmax = _props(labels, data, [False] * 3)
    eh, el = limb_exponents(data.size, absmax)
    for i in range(k):
        exact = math.fsum(data[labels == i + 1].tolist())
        bound = float(sizes[i]) * math.ldexp(1.0, el - 1) + 3 * 2.0 ** -53 * abs(exact)
        print(decades, i, props["sums"][i], exact, abs(props["sums"][i] - exact), bound)
        assert abs(props["sums"][i] - exact) <= bound
    np.testing.assert_array_equal(props["means"], props["sums"] / sizes)


# ---- periodic grids -------------------------------------------------------------------------------------------------------------------------
def test_a_droplet_cut_by_periodic_faces_is_the_droplet_rolled_to_the_middle():
    """A 4 x 4 x 4 block with a corner cell taken out and a cell added on a face (64 cells: every centroid is a dyadic fraction, so the
    comparison is exact), in the middle of a 10 x 12 x 14 grid, rolled across one, two and three periodic faces."""
    shape = (10, 12, 14)
    middle = np.zeros(shape, dtype=np.int32)
    middle[3:7, 4:8, 5:9] = 1
    middle[3, 4, 5] = 0
    middle[7, 5, 6] = 1
    assert middle.sum() == 64
    data = np.where(middle > 0, 0.75, -1.0)
    for per in itertools.product((False, True), repeat=3):
        if not any(per):
            continue
        ref, _, _ = _props(middle, data, per)
        assert not ref["ambiguous"].any()
        shift = tuple(-s if p else 0 for s, p in zip((5, 6, 7), per))          # across the lower face of every periodic axis
        cut = np.roll(middle, shift, axis=(0, 1, 2))
        assert all((cut.take(0, axis=a).any() and cut.take(-1, axis=a).any()) == p for a, p in enumerate(per))
        got, _, _ = _props(cut, np.roll(data, shift, axis=(0, 1, 2)), per)
        n = np.array(shape, dtype=np.float64)
        moved = np.where(per, np.mod(ref["centroids"] + np.array(shift), n), ref["centroids"])
        np.testing.assert_array_equal(got["centroids"], moved)
        np.testing.assert_array_equal(got["extents"], ref["extents"])
        np.testing.assert_array_equal(np.mod(got["bounding_boxes"], np.array(shape)[None, :, None]),
                                      np.mod(ref["bounding_boxes"] + np.array(shift)[None, :, None], np.array(shape)[None, :, None]))
        np.testing.assert_array_equal(got["sums"], ref["sums"])
        assert not got["ambiguous"].any() and not got["touches_boundary"].any()


def test_a_stripe_is_ambiguous_along_the_axis_it_spans():
    shape = (8, 9, 10)
    labels = np.zeros(shape, dtype=np.int32)
    labels[:, 3:5, 2:4] = 1                          # spans axis 0
    labels[1, 1, 7] = 2
    props, _, _ = _props(labels, None, (True, True, True))
    np.testing.assert_array_equal(props["ambiguous"], [[True, False, False], [False, False, False]])
    np.testing.assert_array_equal(props["extents"], [[8, 2, 2], [1, 1, 1]])
    assert props["sums"] is None
    open_, _, _ = _props(labels, None, (False, True, True))
    assert not open_["ambiguous"].any() and open_["touches_boundary"].tolist() == [True, False]


# ---- the shim against the restatement ---------------------------------------------------------------------------------------------------
def test_shim_label_patterns(shim):
    P.run_patterns(shim)


def test_shim_beyond_the_turn(shim):
    P.run_turn(shim)


def test_shim_refusals(shim):
    P.run_refusals(shim)
    P.run_labels_out_of_range(shim)


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_device_and_host_path_agree(shim, dtype):
    backend = pde_hip.get_backend("hip")
    assert shim.has("domain_properties")
    for shape in ((200,), (9, 150), (5, 7, 70)):
        data = P.smooth_field(shape, dtype, sigma=2.0 if len(shape) < 3 else 1.0)
        for per in P.all_periodic(len(shape)):
            for conn in (1, len(shape)):
                P.check_field(backend, data, per, f"{shape} {per} c{conn}", connectivity=conn)
    for name, (data, kwargs) in P.sum_fields((5, 7, 70), dtype).items():
        got = P.check_field(backend, data, (True, False, True), name, **kwargs)
        if name == "inf":
            assert np.isnan(got.sums).sum() == 1 and got.excluded.sum() == 1


def test_a_library_without_the_entry_point_takes_the_host_path():
    shape, per = (5, 7, 70), (True, False, True)
    data = P.smooth_field(shape, np.float64)
    grid = pde_hip.CartesianGrid([(-1.0, -1.0 + 0.5 * n) for n in shape], shape, periodic=list(per))
    with props_shimlib.use_shim():
        backend = pde_hip.get_backend("hip")
        expect = backend.make_domain_labeller(grid)(P.device_array(backend, grid, data), properties=True)
    with label_shimlib.use_shim() as lib:
        assert lib.has("label_domains") and not lib.has("domain_properties")
        backend = pde_hip.get_backend("hip")
        got = backend.make_domain_labeller(grid)(P.device_array(backend, grid, data), properties=True)
        assert got.on_device          # the labelling itself ran there
        P.same_properties(got, expect)


def test_without_the_keyword_nothing_changes(shim):
    shape = (9, 150)
    data = P.smooth_field(shape, np.float64, sigma=2.0)
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.UnitGrid(shape, periodic=True)
    dev = P.device_array(backend, grid, data)
    calls = []
    real = shim.domain_properties
    shim.domain_properties = lambda *args: calls.append(args) or real(*args)
    try:
        plain = backend.make_domain_labeller(grid)(dev)
        also = pde_hip.field_domains(dev, backend=backend, periodic=True)
        assert not calls
        for found in (plain, also):
            assert "_props" not in found.__dict__
            for name in PROPERTY_NAMES:
                with pytest.raises(AttributeError, match="properties=True"):
                    getattr(found, name)
                assert not hasattr(found, name)
        with pytest.raises(AttributeError):
            plain.no_such_attribute
        full = backend.make_domain_labeller(grid)(dev, properties=True)
        assert len(calls) == 1
        np.testing.assert_array_equal(full.sizes, plain.sizes)
        np.testing.assert_array_equal(full.labels, plain.labels)
        assert full.positions.shape == (full.count, 2)
        np.testing.assert_array_equal(full.positions, full.centroids + 0.5)
        np.testing.assert_array_equal(full.radii, np.sqrt(full.sizes / np.pi))
    finally:
        shim.domain_properties = real


def test_domain_properties_of_held_labels(shim):
    shape, per = (9, 150), (True, False)
    data = P.smooth_field(shape, np.float32, sigma=2.0)
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.CartesianGrid([(0.0, 2.0 * n) for n in shape], shape, periodic=list(per))
    dev = P.device_array(backend, grid, data)
    found = backend.make_domain_labeller(grid)(dev, properties=True)
    plain = backend.make_domain_labeller(grid)(dev)
    for labels, field in ((plain, dev), (plain.labels_device, dev), (plain.labels, dev), (plain.labels, data), (plain.labels.astype(np.int64), pde_hip.ScalarField(grid, data))):
        again = pde_hip.domain_properties(labels, field, grid=grid, backend=backend)
        P.same_properties(again, found)
    with pytest.raises(ValueError):
        pde_hip.domain_properties(plain.labels.astype(float), data, grid=grid)
    with pytest.raises(ValueError, match="ONE component"):
        pde_hip.domain_properties(plain.labels, pde_hip.VectorField.random_uniform(grid, rng=np.random.default_rng(1)), grid=grid)
