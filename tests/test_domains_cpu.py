"""Domains without a GPU: the host shim with the domain entry points (tests/label_shimlib.py) stands in for the library.

* the conditions that keep the cases of ``tests/domains_cases.py`` from being vacuous, on the reference alone;
* the shim's sequential C versions of ``pdehip_label_domains`` / ``pdehip_domain_sizes`` against the reference, on the cases of the GPU
  test: this keeps reference and shim honest;
* the Python side (``pde_hip/domains.py``) through the mirror classes and, where py-pde is importable, through the real py-pde: device and
  host path give equal results, the refusals, the fp32 threshold rule, a library without the entry points.
The kernels are tested on the GPU (tests/test_hip_domains.py)."""

from __future__ import annotations

import domains_cases as D
import hist_shimlib
import label_shimlib
import numpy as np
import pytest
import refpath
import shimlib

import pde_hip
from pde_hip import _abi
from pde_hip.device import DeviceArray
from pde_hip.domains import host_domains, interval_bounds

IDS = ["f64", "f32"]


@pytest.fixture
def shim():
    with label_shimlib.use_shim() as lib:
        yield lib


@pytest.fixture
def pde():
    mod = refpath.import_reference()
    if mod is None:
        pytest.skip("py-pde (reference) not available")
    import pde_hip.pypde_plugin  # noqa: F401

    return mod


def test_abi_table():
    assert _abi.ABI_VERSION == 8
    assert {"label_domains", "domain_sizes"} <= set(_abi.OPTIONAL_PROTOTYPES)
    assert not {"label_domains", "domain_sizes"} & (set(_abi.COMPUTE_PROTOTYPES) | set(_abi.COMM_PROTOTYPES) | set(_abi.RUNTIME_PROTOTYPES))


def test_other_shims_lack_the_entry_points_and_still_load():
    for module in (shimlib, hist_shimlib):
        with module.use_shim() as lib:
            assert not lib.has("label_domains") and not lib.has("domain_sizes")
    with label_shimlib.use_shim() as lib:
        assert lib.has("label_domains", "domain_sizes", "histogram", "field_stats")


@pytest.mark.parametrize("shape", D.SHAPES, ids=D.shape_id)
def test_cases_are_not_vacuous(shape):
    D.check_conditions(shape)


def test_fixed_masks_are_what_they_claim():
    """One serpentine through every tile, a checkerboard of single cells that is one domain under full connectivity, diagonal cells
    that only full connectivity joins, stripes that only the wrap joins."""
    for shape in ((9, 65), (9, 7, 65), (17, 9, 64)):
        ndim, open_ = len(shape), (False,) * len(shape)
        labels, k, fg, sizes = D.expected(shape, "serpentine", open_, 1)
        tiles = D.tiles_of(labels).ravel()
        assert k == 1 and np.unique(tiles[labels.ravel() > 0]).size == np.unique(tiles).size > 1
        assert D.expected(shape, "checkerboard", open_, 1)[1] == D.expected(shape, "checkerboard", open_, 1)[2] > 1
        assert D.expected(shape, "checkerboard", open_, ndim)[1] == 1
        assert D.expected(shape, "diagonal", open_, 1)[1] == D.expected(shape, "diagonal", open_, 1)[2] >= min(shape)
        assert D.expected(shape, "diagonal", open_, ndim)[1] <= 2
        assert D.expected(shape, "stripes", open_, 1)[1] == 2 and D.expected(shape, "stripes", (True,) * ndim, 1)[1] == 1


def test_scipy_numbers_domains_by_their_first_cell():
    """What the host path of pde_hip/domains.py relies on: the reference renumbers explicitly, the host path does not."""
    for shape in D.SHAPES:
        for name, mask in D.masks_of(shape).items():
            for conn in D.connectivities(len(shape)):
                for per in D.periodic_patterns(len(shape)):
                    labels, count = host_domains(mask, per, conn)
                    e_labels, e_k, _, _ = D.expected(shape, name, per, conn)
                    assert count == e_k, (shape, name, conn, per)
                    np.testing.assert_array_equal(labels, e_labels, err_msg=f"{shape} {name} c{conn} {per}")


@pytest.mark.parametrize("dtype", D.DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", D.SHAPES, ids=D.shape_id)
def test_shim_label_domains(shim, shape, dtype):
    D.run_shape(shim, shape, dtype)


@pytest.mark.parametrize("dtype", D.DTYPES, ids=IDS)
def test_shim_special_values(shim, dtype):
    for shape in ((130,), (9, 65), (5, 9, 33)):
        D.run_special_values(shim, shape, dtype)


def test_shim_beyond_the_turn(shim):
    """The cases beyond the turn of the device's size kernel: their own conditions hold, and the shim agrees with the reference."""
    for name in ("smoothed", "ragged"):
        D.run_turn_case(shim, name, np.float64)
    D.run_sizes_beyond_the_turn(shim)


def test_entry_points_refuse_bad_arguments(shim):
    D.run_refusals(shim)
    D.run_labels_above_ndomains(shim)


# ---- the Python side through the mirror classes -------------------------------------------------------------------------------------
def _same(a, b):
    assert a.count == b.count and a.foreground == b.foreground and a.largest == b.largest and a.fraction == b.fraction
    np.testing.assert_array_equal(a.sizes, b.sizes)
    np.testing.assert_array_equal(a.volumes, b.volumes)
    np.testing.assert_array_equal(a.labels, b.labels)
    assert a.labels.dtype == b.labels.dtype == np.int32 and a.sizes.dtype == np.int64


@pytest.mark.parametrize("dtype", D.DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,periodic", [((40,), True), ((9, 12), [True, False]), ((5, 6, 9), True), ((5, 6, 9), False)])
def test_device_and_host_path_agree(shim, shape, periodic, dtype):
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.CartesianGrid([(0.0, 1.5 * n) for n in shape], shape, periodic=periodic)
    field = pde_hip.ScalarField.random_uniform(grid, -1.0, 1.0, rng=np.random.default_rng(3), dtype=dtype)
    dev = DeviceArray(backend.grid_info(grid, field.dtype), ()).set_valid(field.data)
    label = backend.make_domain_labeller(grid)
    ndim = len(shape)
    for kwargs in ({}, {"threshold": 0.25}, {"threshold": -0.1, "above": False}, {"interval": (-0.2, 0.4)}, {"connectivity": ndim},
                   {"periodic": [False] * ndim}, {"periodic": True, "connectivity": ndim}):
        got, host = label(dev, **kwargs), label(field, **kwargs)
        assert got.on_device and not host.on_device and got.labels_device is not None and host.labels_device is None
        _same(got, host)
        if "interval" in kwargs:
            mask = (field.data >= kwargs["interval"][0]) & (field.data <= kwargs["interval"][1])
        else:
            t = kwargs.get("threshold", 0.0)
            mask = field.data > t if kwargs.get("above", True) else field.data < t
        per = np.broadcast_to(kwargs.get("periodic", grid.periodic), (ndim,))
        e_labels, e_k, e_fg, e_sizes = D.reference(mask, tuple(bool(p) for p in per), kwargs.get("connectivity", 1))
        assert (got.count, got.foreground) == (e_k, e_fg)
        np.testing.assert_array_equal(got.labels, e_labels)
        np.testing.assert_array_equal(got.sizes, e_sizes)
        np.testing.assert_array_equal(got.volumes, e_sizes * 1.5 ** ndim)
        assert got.fraction == e_fg / field.data.size and got.largest == (e_sizes.max() if e_k else 0)
        _same(label(np.array(field.data), **kwargs), host)          # a bare host array with the grid of make_domain_labeller
    empty = label(dev, threshold=5.0)
    assert empty.count == 0 and empty.largest == 0 and empty.sizes.shape == (0,) and not empty.labels.any()


def test_refusals_of_the_python_side(shim):
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.UnitGrid([4, 6])
    scalar = pde_hip.ScalarField.random_uniform(grid, rng=np.random.default_rng(1))
    vector = pde_hip.VectorField.random_uniform(grid, rng=np.random.default_rng(1))
    tensor = pde_hip.Tensor2Field.random_uniform(grid, rng=np.random.default_rng(1))
    collection = pde_hip.FieldCollection([scalar, scalar.copy()]) if hasattr(scalar, "copy") else None
    for obj in (vector, tensor, DeviceArray(backend.grid_info(grid, np.float64), (2,))) + ((collection,) if collection is not None else ()):
        with pytest.raises(ValueError, match="ONE component"):
            pde_hip.field_domains(obj)
    one = pde_hip.field_domains(pde_hip.ScalarField(grid, vector.data[1]), 0.5)
    assert one.count == D.reference(vector.data[1] > 0.5, (False, False), 1)[1]
    for bad in ({"connectivity": 0}, {"connectivity": 3}, {"interval": (1.0, 0.0)}, {"interval": (np.nan, 1.0)}, {"threshold": np.nan}):
        with pytest.raises(ValueError):
            pde_hip.field_domains(scalar, **bad)


def test_thresholds_compare_as_numpy_compares_them():
    """The closed interval behind ``>`` / ``<`` selects the cells numpy selects, for thresholds on, between and beyond the values of the
    field's type; 1/3 and 0.1 are not fp32 numbers."""
    for dtype in D.DTYPES:
        third = dtype(1.0) / dtype(3.0)
        values = np.array([-np.inf, -1.0, np.nextafter(third, dtype(0)), third, np.nextafter(third, dtype(1)), 0.0, -0.0, 0.1, 1.0, np.inf,
                           np.finfo(dtype).max, np.finfo(dtype).smallest_subnormal, np.nan], dtype=dtype)
        for t in (0.0, 1.0 / 3.0, float(third), 0.1, float(dtype(0.1)), -1.0, 1e300, -1e300, np.inf, -np.inf):
            with np.errstate(invalid="ignore", over="ignore"):
                for above, expect in ((True, values > dtype(t)), (False, values < dtype(t))):
                    if dtype(t) == (np.inf if above else -np.inf):
                        with pytest.raises(ValueError, match="no float"):
                            interval_bounds(dtype, t, above)
                        continue
                    lo, hi = interval_bounds(dtype, t, above)
                    got = (values.astype(np.float64) >= lo) & (values.astype(np.float64) <= hi)
                    np.testing.assert_array_equal(got, expect, err_msg=f"{np.dtype(dtype).name} t={t!r} above={above}")
        # numpy converts a Python float next to an array to the array's type: 1/3 compares as float32(1/3) with an fp32 field
        np.testing.assert_array_equal(values > 1.0 / 3.0, values > dtype(1.0 / 3.0))


# ---- through the real py-pde ------------------------------------------------------------------------------------------------------------
def _callback(seen):
    def callback(field, t):
        link = field.__dict__.get("_hip_link")
        resident = link is not None and link.host_stale
        before = link.downloads if link is not None else None
        got = pde_hip.field_domains(field, 0.0)
        full = pde_hip.field_domains(field, 0.0, above=False, connectivity=field.grid.num_axes)
        seen.append({"t": t, "resident": resident, "on_device": got.on_device, "before": before,
                     "after": link.downloads if link is not None else None, "got": got, "full": full,
                     "side": link.dev_state.get_valid() if resident else np.array(field.data)})
        return 0.0

    return callback


def _check_seen(seen, periodic):
    for s in seen:
        side, ndim = s["side"], s["side"].ndim
        for res, mask, conn in ((s["got"], side > 0.0, 1), (s["full"], side < 0.0, ndim)):
            e_labels, e_k, e_fg, e_sizes = D.reference(mask, periodic, conn)
            assert (res.count, res.foreground) == (e_k, e_fg)
            np.testing.assert_array_equal(res.sizes, e_sizes)
            np.testing.assert_array_equal(res.labels, e_labels)


def _problem(pde):
    grid = pde.UnitGrid([16, 16], periodic=[True, False])
    state = pde.ScalarField.random_uniform(grid, -1.0, 1.0, rng=np.random.default_rng(4))
    return pde.DiffusionPDE(0.1), state


def test_data_tracker_callback_leaves_the_state_on_the_device(pde):
    eq, state = _problem(pde)
    seen = []
    with label_shimlib.use_shim():
        res = eq.solve(state, t_range=2.0, dt=0.1, solver="euler", backend="hip", tracker=[pde.DataTracker(_callback(seen), interrupts=0.5)])
        link = res.__dict__["_hip_link"]
        resident = [s for s in seen if s["resident"]]
        assert len(resident) >= 3 and all(s["on_device"] and s["before"] == s["after"] == 0 for s in resident), seen
        assert link.downloads == 0
        _check_seen(seen, (True, False))
        assert any(s["got"].count >= 2 for s in resident)
        # the host copy is current (before the first stepper call, and after the result was read): the host path, nothing uploaded
        assert not seen[0]["resident"] and not seen[0]["on_device"]
        res.data                                             # noqa: B018  (the download)
        uploads = link.uploads
        late = pde_hip.field_domains(res)
        assert not late.on_device and link.uploads == uploads
        np.testing.assert_array_equal(late.labels, D.reference(res.data > 0.0, (True, False), 1)[0])


def test_a_library_without_the_entry_points_takes_the_host_path(pde):
    eq, state = _problem(pde)
    seen = []
    with hist_shimlib.use_shim():
        eq.solve(state, t_range=1.0, dt=0.1, solver="euler", backend="hip", tracker=[pde.DataTracker(_callback(seen), interrupts=0.5)])
    assert seen and not any(s["on_device"] for s in seen)
    assert any(s["after"] > s["before"] for s in seen if s["before"] is not None)          # it pulled the state, as scipy would
    _check_seen(seen, (True, False))


def test_complex_fields_take_the_host_path_and_collections_are_refused(pde):
    grid = pde.UnitGrid([16, 16], periodic=True)
    rng = np.random.default_rng(6)
    complex_state = pde.ScalarField(grid, rng.uniform(-1, 1, (16, 16)) + 1j * rng.uniform(-1, 1, (16, 16)))
    collection = pde.FieldCollection([pde.ScalarField.random_uniform(grid, -1, 1, rng=rng), pde.ScalarField.random_uniform(grid, -1, 1, rng=rng)])
    vector = pde.VectorField.random_uniform(grid, -1, 1, rng=rng)
    seen = []

    def on_complex(field, t):
        got = pde_hip.field_domains(field, 0.0)
        data = np.array(field.data)
        np.testing.assert_array_equal(got.labels, D.reference(data > 0.0, (True, True), 1)[0])
        seen.append(got.on_device)

    with label_shimlib.use_shim():
        pde.DiffusionPDE(1.0).solve(complex_state, t_range=1.0, dt=0.1, solver="euler", backend="hip", tracker=[pde.CallbackTracker(on_complex, interrupts=0.5)])
        for obj in (collection, vector):
            with pytest.raises(ValueError, match="ONE component"):
                pde_hip.field_domains(obj)
        assert pde_hip.field_domains(collection[1], -0.5).count == D.reference(collection[1].data > -0.5, (True, True), 1)[1]
    assert seen and not any(seen)
