"""Histograms and quantiles without a GPU: the host shim with the distribution entry points (tests/hist_shimlib.py) stands in for the library.

* the shim's plain C versions of ``pdehip_histogram`` / ``pdehip_quantile_select`` against the numpy restatements of ``tests/hist_cases.py``
  and against ``np.histogram`` itself, on the shapes of the GPU test: this keeps restatement and shim honest;
* the Python side (``pde_hip/distribution.py``) through the mirror classes: device and host path give equal results;
* where py-pde is importable, a ``DataTracker`` callback that calls ``pde_hip.field_histogram`` / ``field_quantile`` during
  ``eq.solve(backend="hip")`` sees numpy's values without a download, and the cases that take the host path (a field whose host copy is
  current, a complex field, a FieldCollection, a library without the entry points).
The kernels are tested on the GPU (tests/test_hip_hist.py)."""

from __future__ import annotations

import hist_cases as H
import hist_shimlib
import numpy as np
import pytest
import refpath
import shimlib
import stats_shimlib

import pde_hip
from pde_hip import _abi
from pde_hip.device import DeviceArray

IDS = ["f64", "f32"]


@pytest.fixture
def shim():
    with hist_shimlib.use_shim() as lib:
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
    assert {"histogram", "quantile_select"} <= set(_abi.OPTIONAL_PROTOTYPES)
    assert not {"histogram", "quantile_select"} & (set(_abi.COMPUTE_PROTOTYPES) | set(_abi.COMM_PROTOTYPES) | set(_abi.RUNTIME_PROTOTYPES))


def test_other_shims_lack_the_entry_points_and_still_load():
    for module in (shimlib, stats_shimlib):
        with module.use_shim() as lib:
            assert not lib.has("histogram") and not lib.has("quantile_select")
    with hist_shimlib.use_shim() as lib:
        assert lib.has("histogram", "quantile_select", "field_stats")


def test_method_cases_agree_with_numpys_index_arithmetic():
    """For every (n, q) of METHOD_CASES numpy's "lower" / "higher" pick the ranks k = floor((n - 1) q) and k, or k + 1 where the product
    is not whole."""
    for shape, qs in H.METHOD_CASES:
        n = int(np.prod(shape))
        ramp = np.arange(n, dtype=np.float64)
        v = (np.float64(n) - 1.0) * np.array(qs)
        k = np.floor(v)
        np.testing.assert_array_equal(np.quantile(ramp, qs, method="lower"), k)
        np.testing.assert_array_equal(np.quantile(ramp, qs, method="higher"), np.where(v - k > 0, np.minimum(k + 1, n - 1), k))


@pytest.mark.parametrize("dtype", H.DTYPES, ids=IDS)
@pytest.mark.parametrize("case", H.SMALL, ids=H.case_id)
def test_shim_histogram(shim, case, dtype):
    H.run_histogram_case(shim, case, dtype)


@pytest.mark.parametrize("dtype", H.DTYPES, ids=IDS)
@pytest.mark.parametrize("case", H.SMALL, ids=H.case_id)
def test_shim_quantile_select(shim, case, dtype):
    H.run_select_case(shim, case, dtype)


@pytest.mark.parametrize("dtype", H.DTYPES, ids=IDS)
def test_shim_quantile_select_fields(shim, dtype):
    for name, valid in H.select_fields(dtype).items():
        dev = H.upload(shim, valid.shape[1:], valid)
        for q in (*H.QS, H.QS):
            H.check_select(H.select(shim, dev, q), valid, q, f"{name} q={q}")


def test_entry_points_refuse_bad_arguments(shim):
    H.run_refusals(shim)


# ---- the Python side through the mirror classes -------------------------------------------------------------------------------------
def _same_histograms(a, b):
    for name in ("counts", "edges", "below", "above", "nan", "density"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)
    assert a.edges.dtype == b.edges.dtype


@pytest.mark.parametrize("dtype", H.DTYPES, ids=IDS)
@pytest.mark.parametrize("cls,shape", [("ScalarField", (6, 5)), ("VectorField", (4, 3, 5)), ("Tensor2Field", (5, 4)), ("VectorField", (9,))])
def test_device_and_host_path_agree_with_numpy(shim, cls, shape, dtype):
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.CartesianGrid([(0.0, 1.5 * n) for n in shape], shape)
    field = getattr(pde_hip, cls).random_uniform(grid, -1.0, 1.0, rng=np.random.default_rng(3), dtype=dtype)
    data = field.data
    lead = data.ndim - len(shape)
    rows = data.reshape((-1,) + data.shape[lead:])
    hist, quant = backend.make_histogram(grid), backend.make_quantiles(grid)
    dev = DeviceArray(backend.grid_info(grid, field.dtype), field.data_shape).set_valid(data)
    for bins, rng_ in ((10, None), (7, (-0.5, 0.25)), (np.array([-2.0, -0.5, 0.0, 0.1, 3.0]), None)):
        got, host = hist(dev, bins, rng_), hist(field, bins, rng_)
        assert got.on_device and not host.on_device
        _same_histograms(got, host)
        assert got.counts.shape == field.data_shape + (got.edges.size - 1,)
        np.testing.assert_array_equal(got.edges, np.histogram(data, bins, rng_)[1])
        flat_counts = got.counts.reshape(rows.shape[0], -1)
        for c, row in enumerate(rows):
            np.testing.assert_array_equal(flat_counts[c], np.histogram(row, got.edges)[0])
        _same_histograms(hist(data, bins, rng_), host)                  # a bare host array with the grid of make_histogram
    if lead:
        _same_histograms(hist(dev, 5, norm=True), hist(field, 5, norm=True))
        assert hist(dev, 5, norm=True).counts.shape == (5,)
    qs = [0.0, 0.2, 0.5, 1.0]
    for method in ("lower", "higher", "linear"):
        got, host = quant(dev, qs, method=method), quant(field, qs, method=method)
        assert got.shape == (4,) + field.data_shape and got.dtype == np.dtype(dtype)
        np.testing.assert_array_equal(H.bits(got), H.bits(host), err_msg=method)
        if method != "linear":
            expect = np.quantile(rows, qs, axis=tuple(range(1, rows.ndim)), method=method).reshape(got.shape)
            np.testing.assert_array_equal(H.bits(got), H.bits(expect.astype(dtype)), err_msg=method)
    assert np.ndim(quant(dev.flat().component(0) if lead else dev, 0.5)) == 0
    np.testing.assert_array_equal(pde_hip.field_median(field, norm=bool(lead)), quant(dev, 0.5, norm=bool(lead)))
    # NaN cells: counted apart, and a quantile is NaN unless they are ignored
    data[..., 0] = np.nan
    dev.set_valid(data)
    got = hist(dev, 4, (-1.0, 1.0))
    _same_histograms(got, hist(field, 4, (-1.0, 1.0)))
    assert got.nan.min() >= 1
    assert np.isnan(quant(dev, 0.5)).all() and np.isnan(quant(field, 0.5)).all()
    np.testing.assert_array_equal(quant(dev, 0.5, ignore_nan=True), quant(field, 0.5, ignore_nan=True))
    assert not np.isnan(quant(dev, 0.5, ignore_nan=True)).any()
    with pytest.raises(ValueError, match="autodetected range"):
        hist(dev, 4)
    with pytest.raises(ValueError, match="autodetected range"):
        hist(field, 4)


def test_arguments_are_checked(shim):
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.UnitGrid([4, 6])
    field = pde_hip.ScalarField.random_uniform(grid, rng=np.random.default_rng(1))
    dev = DeviceArray(backend.grid_info(grid, field.dtype), ()).set_valid(field.data)
    hist, quant = backend.make_histogram(grid), backend.make_quantiles(grid)
    for obj in (dev, field):
        with pytest.raises(ValueError, match="auto"):
            hist(obj, "auto")
        with pytest.raises(ValueError, match="4097"):
            hist(obj, 4097)
        with pytest.raises(ValueError):
            hist(obj, np.linspace(0, 1, 4099))
        with pytest.raises(ValueError):
            hist(obj, 0)
        with pytest.raises(ValueError):
            hist(obj, [0.0, 0.5, 0.5, 1.0])
        with pytest.raises(ValueError):
            hist(obj, 4, (1.0, 0.0))
        with pytest.raises(ValueError):
            hist(obj, 4, (0.0, np.inf))
        with pytest.raises(ValueError, match="nearest"):
            quant(obj, 0.5, method="nearest")
        with pytest.raises(ValueError):
            quant(obj, 1.5)
        assert hist(obj, 4096).counts.shape == (4096,)
        with pytest.raises(ValueError):
            hist(obj, 4, (0.0, 1.0)).fraction_above(0.3)
        assert hist(obj, 4, (0.0, 1.0)).fraction_above(0.5) == (field.data >= 0.5).mean()
    qs = np.linspace(0.0, 1.0, 19)          # more than 8 values of q: groups of 8
    np.testing.assert_array_equal(quant(dev, qs, method="lower"), np.quantile(field.data, qs, method="lower"))


# ---- through the real py-pde ------------------------------------------------------------------------------------------------------------
def _problem(pde, dtype=np.float64):
    grid = pde.UnitGrid([16, 16], periodic=[True, False])
    state = pde.ScalarField.random_uniform(grid, 0.5, 1.5, rng=np.random.default_rng(4), dtype=dtype)
    return pde.DiffusionPDE(1.0), state


def _callback(seen):
    def callback(field, t):
        link = field.__dict__.get("_hip_link")
        resident = link is not None and link.host_stale
        before = link.downloads if link is not None else None
        hist = pde_hip.field_histogram(field, 12, (0.5, 1.5))
        auto = pde_hip.field_histogram(field, 12)
        quant = pde_hip.field_quantile(field, [0.1, 0.5, 0.9], method="lower")
        median = pde_hip.field_median(field)
        seen.append({"t": t, "resident": resident, "on_device": hist.on_device, "before": before,
                     "after": link.downloads if link is not None else None, "hist": hist, "auto": auto, "quant": quant, "median": median,
                     "side": link.dev_state.get_valid() if resident else np.array(field.data)})
        return 0.0

    return callback


def _check_seen(seen):
    for s in seen:
        side = s["side"]
        np.testing.assert_array_equal(s["hist"].counts, np.histogram(side, 12, (0.5, 1.5))[0])
        np.testing.assert_array_equal(s["auto"].counts, np.histogram(side, 12)[0])
        np.testing.assert_array_equal(s["auto"].edges, np.histogram(side, 12)[1])
        np.testing.assert_array_equal(s["quant"], np.quantile(side, [0.1, 0.5, 0.9], method="lower"))
        ordered = np.sort(side.ravel())
        k = (ordered.size - 1) // 2
        assert s["median"] == ordered[k] + (ordered[k + 1] - ordered[k]) * 0.5


def test_data_tracker_callback_leaves_the_state_on_the_device(pde):
    eq, state = _problem(pde)
    seen = []
    with hist_shimlib.use_shim():
        res = eq.solve(state, t_range=4.0, dt=0.2, solver="euler", backend="hip", tracker=[pde.DataTracker(_callback(seen), interrupts=1.0)])
        link = res.__dict__["_hip_link"]
        resident = [s for s in seen if s["resident"]]
        assert len(resident) >= 3 and all(s["on_device"] and s["before"] == s["after"] == 0 for s in resident), seen
        assert link.downloads == 0
        _check_seen(seen)
        # the host copy is current (before the first stepper call, and after the result was read): the host path, nothing uploaded
        assert not seen[0]["resident"] and not seen[0]["on_device"]
        res.data                                             # noqa: B018  (the download)
        uploads = link.uploads
        late = pde_hip.field_histogram(res, 12, (0.5, 1.5))
        assert not late.on_device and link.uploads == uploads
        np.testing.assert_array_equal(late.counts, np.histogram(res.data, 12, (0.5, 1.5))[0])


def test_a_library_without_the_entry_points_takes_the_host_path(pde):
    eq, state = _problem(pde)
    seen = []
    with stats_shimlib.use_shim():
        eq.solve(state, t_range=2.0, dt=0.2, solver="euler", backend="hip", tracker=[pde.DataTracker(_callback(seen), interrupts=1.0)])
    assert seen and not any(s["on_device"] for s in seen)
    assert any(s["after"] > s["before"] for s in seen if s["before"] is not None)          # it pulled the state, as numpy would
    _check_seen(seen)


def test_complex_fields_and_collections_take_the_host_path(pde):
    grid = pde.UnitGrid([16, 16], periodic=True)
    rng = np.random.default_rng(6)
    complex_state = pde.ScalarField(grid, rng.uniform(0.5, 1.5, (16, 16)) + 1j * rng.uniform(0.5, 1.5, (16, 16)))
    collection = pde.FieldCollection([pde.ScalarField.random_uniform(grid, 0.5, 1.5, rng=rng), pde.ScalarField.random_uniform(grid, 2.5, 3.5, rng=rng)])
    eq_col = pde.PDE({"a": "laplace(a)", "b": "laplace(b) - 0.01 * b"})
    seen = []

    def on_complex(field, t):
        hist = pde_hip.field_histogram(field, 6)
        counts, edges = np.histogram(field.data, 6)
        np.testing.assert_array_equal(hist.counts, counts)
        np.testing.assert_array_equal(hist.edges, edges)
        with pytest.raises(TypeError):
            pde_hip.field_quantile(field, 0.5)
        seen.append(("complex", hist.on_device))

    def on_collection(field, t):
        hist = pde_hip.field_histogram(field, 6)
        data = np.array(field.data)
        assert hist.counts.shape == (2, 6)
        np.testing.assert_array_equal(hist.edges, np.histogram(data, 6)[1])
        for c in range(2):
            np.testing.assert_array_equal(hist.counts[c], np.histogram(data[c], hist.edges)[0])
        np.testing.assert_array_equal(pde_hip.field_quantile(field, 0.25, method="higher"), np.quantile(data, 0.25, axis=(1, 2), method="higher"))
        seen.append(("collection", hist.on_device))

    with hist_shimlib.use_shim():
        pde.DiffusionPDE(1.0).solve(complex_state, t_range=1.0, dt=0.1, solver="euler", backend="hip", tracker=[pde.CallbackTracker(on_complex, interrupts=0.5)])
        eq_col.solve(collection, t_range=1.0, dt=0.1, solver="euler", backend="hip", tracker=[pde.CallbackTracker(on_collection, interrupts=0.5)])
    assert {kind for kind, _ in seen} == {"complex", "collection"} and not any(on_device for _, on_device in seen)
