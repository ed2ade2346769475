"""Device statistics without a GPU: the host shim with the two statistics entry points (tests/stats_shimlib.py) stands in for the library.

* the shim's plain C versions of ``pdehip_field_stats`` / ``pdehip_steady_state`` against the numpy restatement and the bounds of
  ``tests/stats_cases.py``, on the shapes of the GPU test: this keeps restatement and shim honest;
* the Python side (``pde_hip/statistics.py``, the resident-field properties under ``device_statistics``) through the mirror classes;
* where py-pde is importable, the trackers ``hip_steady_state`` and ``hip_material_conservation`` on ``backend="hip"`` runs against the
  stock trackers on the same problem, and the cases that take the host path (a library without the entry points, complex states,
  ``progress=True``, ``evolution_rate=...``, a FieldCollection).
The kernels are tested on the GPU (tests/test_hip_stats.py)."""

from __future__ import annotations

import numpy as np
import pytest

import pde_hip
import refpath
import shimlib
import stats_cases as S
import stats_shimlib
from pde_hip import _abi
from pde_hip.device import DeviceArray


@pytest.fixture
def shim():
    with stats_shimlib.use_shim() as lib:
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
    assert {"field_stats", "steady_state"} <= set(_abi.OPTIONAL_PROTOTYPES)
    assert not {"field_stats", "steady_state"} & (set(_abi.COMPUTE_PROTOTYPES) | set(_abi.COMM_PROTOTYPES) | set(_abi.RUNTIME_PROTOTYPES))


def test_plain_shim_lacks_the_entry_points_and_still_loads():
    with shimlib.use_shim() as lib:
        assert not lib.has("field_stats") and not lib.has("steady_state")
    with stats_shimlib.use_shim() as lib:
        assert lib.has("field_stats", "steady_state")


@pytest.mark.parametrize("dtype", S.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", S.SMALL, ids=S.case_id)
def test_shim_field_stats(shim, case, dtype):
    shape, ncomp = case
    for planted in (False, True):
        valid, expect, expect_norm = S.small_inputs(case, np.dtype(dtype).name, planted)
        dev = S.upload(shim, shape, valid)
        S.check_stats(S.field_stats(shim, dev), expect, what=f"planted={planted}")
        S.check_stats(S.field_stats(shim, dev, norm=True), expect_norm, what=f"norm planted={planted}")
        S.check_stats(S.field_stats(shim, dev, want_m2=False), expect, want_m2=False, what=f"no m2 planted={planted}")


@pytest.mark.parametrize("dtype", S.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", S.SMALL, ids=S.case_id)
def test_shim_steady_state(shim, case, dtype):
    shape, ncomp = case
    cur = S.plant_nonfinite(S.draw(shape, ncomp, dtype, seed=1)) if np.prod(shape) > 4 else S.draw(shape, ncomp, dtype, seed=1)
    last = (S.draw(shape, ncomp, dtype, seed=1) + 1e-3 * S.draw(shape, ncomp, dtype, seed=2)).astype(dtype)
    dcur, dlast = S.upload(shim, shape, cur), S.upload(shim, shape, last)
    S.check_steady(S.steady_state(shim, dcur, dlast), S.np_steady(cur, last), "steady")
    np.testing.assert_array_equal(S.bits(dlast.get_valid()), S.bits(cur))
    # a NaN in the snapshot under a finite cell; nothing finite at all
    last2 = last.copy()
    last2.reshape(ncomp, -1)[-1, -1] = np.nan
    cur2 = S.draw(shape, ncomp, dtype, seed=1)
    S.check_steady(S.steady_state(shim, S.upload(shim, shape, cur2), S.upload(shim, shape, last2)), (np.float64(np.nan), cur2.size), "NaN snapshot")
    none = np.full_like(cur, np.inf)
    got = S.steady_state(shim, S.upload(shim, shape, none), S.upload(shim, shape, last))
    assert got[1] == 0 and np.isnan(got[0])


def test_entry_points_refuse_bad_arguments(shim):
    valid = S.draw((4, 4), 1, np.float64)
    dev = S.upload(shim, (4, 4), valid)
    from pde_hip.device import DeviceBuffer

    out = DeviceBuffer(64)
    with pytest.raises(ValueError):
        shim.field_stats(dev.info.ref, 1, None, 0, 0, out.ptr, None)
    with pytest.raises(ValueError):
        shim.field_stats(dev.info.ref, 65, dev.ptr, 0, 0, out.ptr, None)
    with pytest.raises(ValueError):
        shim.steady_state(dev.info.ref, 1, dev.ptr, dev.ptr, 1.0, 0.0, out.ptr, None)


# ---- the Python side through the mirror classes -------------------------------------------------------------------------------------
def _close(a, b, rel=1e-12):
    np.testing.assert_allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=rel, atol=0)


@pytest.mark.parametrize("cls,shape", [("ScalarField", (6, 5)), ("VectorField", (4, 3, 5)), ("Tensor2Field", (5, 4)), ("VectorField", (9,))])
def test_make_statistics_device_and_host_agree(shim, cls, shape):
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.CartesianGrid([(0.0, 1.5 * n) for n in shape], shape)
    field = getattr(pde_hip, cls).random_uniform(grid, 0.5, 1.5, rng=np.random.default_rng(3))
    stats = backend.make_statistics(grid)
    host = stats(field, variance=True)
    assert not host.on_device
    dev = DeviceArray(backend.grid_info(grid, field.dtype), field.data_shape).set_valid(field.data)
    got = stats(dev, variance=True)
    assert got.on_device and got.sum.shape == field.data_shape
    _close(got.integral, field.integral)
    _close(got.average, field.average)
    _close(got.fluctuations, field.fluctuations, 1e-10)
    _close(host.integral, field.integral)
    _close(host.fluctuations, field.fluctuations)
    np.testing.assert_array_equal(got.min, field.data.min(axis=tuple(range(field.rank, field.data.ndim))))
    np.testing.assert_array_equal(got.count, np.full(field.data_shape, grid.cell_coords[..., 0].size))
    from pde_hip.statistics import device_magnitude

    _close(device_magnitude(backend, field, dev), field.magnitude)
    if field.rank:
        _close(stats(dev, norm=True).magnitude, stats(field, norm=True).magnitude)
    # non-finite cells: counted, and the derived quantities are numpy's
    field.data[..., 0] = np.nan
    dev.set_valid(field.data)
    bad = stats(dev, variance=True)
    assert bad.nonfinite.min() >= 1 and np.all(np.isnan(bad.average)) and np.all(np.isfinite(bad.mean))
    assert pde_hip.field_statistics(field).nonfinite.min() >= 1


def test_mirror_collection_properties():
    grid = pde_hip.UnitGrid([4, 6])
    rng = np.random.default_rng(1)
    fields = [pde_hip.ScalarField.random_uniform(grid, rng=rng), pde_hip.VectorField.random_uniform(grid, rng=rng)]
    col = pde_hip.FieldCollection(fields)
    assert len(col.integrals) == 2 and np.shape(col.integrals[1]) == (2,)
    _close(col.averages[0], fields[0].data.mean())
    _close(col.magnitudes, [abs(fields[0].data.mean()), np.linalg.norm(fields[1].data, axis=0).mean()])
    _close(fields[0].fluctuations, fields[0].data.std())


def _run_mirror(backend, device_statistics, seen):
    """A diffusion run whose tracker callback reads the properties of the state; returns the link of the state."""
    backend.device_statistics = device_statistics
    grid = pde_hip.UnitGrid([8, 8, 8], periodic=True)
    state = pde_hip.ScalarField.random_uniform(grid, 0.5, 1.5, rng=np.random.default_rng(5))

    def callback(field, t):
        link = field.__dict__.get("_hip_link")
        before = link.downloads if link is not None else None
        seen.append((t, float(field.average), float(field.fluctuations), float(field.integral), float(field.magnitude), before,
                     link.downloads if link is not None else None))

    try:
        res = pde_hip.DiffusionPDE(0.5).solve(state, t_range=0.4, dt=0.05, solver="euler", backend=backend, tracker=callback, interval=0.1)
    finally:
        backend.device_statistics = None
    return res


def test_resident_properties_opt_in(shim):
    backend = pde_hip.get_backend("hip")
    on, off = [], []
    _run_mirror(backend, True, on)
    _run_mirror(backend, False, off)
    resident_on = [s for s in on if s[5] is not None]
    assert resident_on and all(s[5] == s[6] == 0 for s in resident_on), on
    assert any(s[6] is not None and s[6] > 0 for s in off), off
    for a, b in zip(on, off):
        _close(a[1:5], b[1:5], 1e-11)


# ---- the trackers through the real py-pde -------------------------------------------------------------------------------------------
def _steady_problem(pde, dtype=np.float64):
    grid = pde.UnitGrid([16, 16], periodic=[True, False])
    state = pde.ScalarField.random_uniform(grid, 0.5, 1.5, rng=np.random.default_rng(4), dtype=dtype)
    return pde.DiffusionPDE(1.0), state


LINKS: list = []


def _solve(pde, eq, state, tracker, t_range=60.0, dt=0.2, **kw):
    """(result, controller info); LINKS[-1] = (resident-state link, its downloads) at the last interrupt, before the trackers ran (the probe reads no data)."""
    def probe(field, t):
        link = field.__dict__.get("_hip_link")
        LINKS.append((link, link.downloads if link is not None else None))

    tracker = [pde.CallbackTracker(probe, interrupts=0.5), *tracker]
    res, info = eq.solve(state, t_range=t_range, dt=dt, solver="euler", backend="hip", tracker=tracker, ret_info=True, **kw)
    return res, info["controller"]


def test_steady_state_tracker_matches_the_stock_tracker(pde):
    from pde_hip.pypde_plugin import HipSteadyStateTracker

    eq, state = _steady_problem(pde)
    with stats_shimlib.use_shim():
        ref, cref = _solve(pde, eq, state, [pde.SteadyStateTracker(interrupts=1.0, atol=1e-3)])
        tracker = HipSteadyStateTracker(interrupts=1.0, atol=1e-3)
        got, cgot = _solve(pde, eq, state, [tracker])
        assert tracker._check.on_device, "the check never ran on the device copy"
        assert LINKS[-1][0] is not None and LINKS[-1][1] == 0
        byname, cname = _solve(pde, eq, state, ["hip_steady_state"], t_range=3.0)
    assert cref["t_final"] < 60.0 and cref["stop_reason"] == "Reached stationary state"
    assert (cgot["t_final"], cgot["stop_reason"]) == (cref["t_final"], cref["stop_reason"])
    np.testing.assert_array_equal(got.data, ref.data)
    assert cname["stop_reason"] == "Reached final time"


def test_steady_state_tracker_fallbacks(pde):
    """A library without the entry points, progress=True and evolution_rate=...: the parent's host path, equal results."""
    from pde_hip.pypde_plugin import HipSteadyStateTracker

    eq, state = _steady_problem(pde)
    with stats_shimlib.use_shim():
        ref, cref = _solve(pde, eq, state, [pde.SteadyStateTracker(interrupts=1.0, atol=1e-3)])

        def rate(data, t):      # the right-hand side of _steady_problem in numpy: periodic along x, zero derivative along y
            p = np.pad(data, ((0, 0), (1, 1)), mode="edge")
            return (np.roll(data, 1, 0) - 2 * data + np.roll(data, -1, 0)) + (p[:, 2:] - 2 * data + p[:, :-2])

        rref, crref = _solve(pde, eq, state, [pde.SteadyStateTracker(interrupts=1.0, atol=1e-3, evolution_rate=rate)])
        for kwargs in ({"progress": True}, {"evolution_rate": rate}):
            tracker = HipSteadyStateTracker(interrupts=1.0, atol=1e-3, **kwargs)
            got, cgot = _solve(pde, eq, state, [tracker])
            want, cwant = (rref, crref) if "evolution_rate" in kwargs else (ref, cref)
            assert not tracker._check.started
            assert (cgot["t_final"], cgot["stop_reason"]) == (cwant["t_final"], cwant["stop_reason"]), kwargs
            np.testing.assert_array_equal(got.data, want.data)
    with shimlib.use_shim():
        tracker = HipSteadyStateTracker(interrupts=1.0, atol=1e-3)
        got, cgot = _solve(pde, eq, state, [tracker])
        assert not tracker._check.on_device
        assert (cgot["t_final"], cgot["stop_reason"]) == (cref["t_final"], cref["stop_reason"])
        np.testing.assert_array_equal(got.data, ref.data)


def test_trackers_on_complex_states_take_the_host_path(pde):
    from pde_hip.pypde_plugin import HipSteadyStateTracker

    grid = pde.UnitGrid([16, 16], periodic=True)
    rng = np.random.default_rng(6)
    state = pde.ScalarField(grid, rng.uniform(0.5, 1.5, (16, 16)) + 1j * rng.uniform(0.5, 1.5, (16, 16)))
    eq = pde.DiffusionPDE(1.0)
    with stats_shimlib.use_shim():
        ref, cref = _solve(pde, eq, state, [pde.SteadyStateTracker(interrupts=1.0, atol=1e-3), pde.MaterialConservationTracker(interrupts=1.0)])
        tracker = HipSteadyStateTracker(interrupts=1.0, atol=1e-3)
        got, cgot = _solve(pde, eq, state, [tracker, "hip_material_conservation"])
    assert not tracker._check.on_device
    assert (cgot["t_final"], cgot["stop_reason"]) == (cref["t_final"], cref["stop_reason"])
    np.testing.assert_array_equal(got.data, ref.data)


def test_material_conservation_tracker_matches_the_stock_tracker(pde):
    from pde_hip.pypde_plugin import HipMaterialConservationTracker

    grid = pde.UnitGrid([16, 16], periodic=True)
    state = pde.ScalarField.random_uniform(grid, 0.5, 1.5, rng=np.random.default_rng(7))
    decay = pde.PDE({"c": "laplace(c) - 0.0001 * c"})
    with stats_shimlib.use_shim():
        for eq, reason in ((decay, "Material is not conserved"), (pde.DiffusionPDE(1.0), "Reached final time")):
            ref, cref = _solve(pde, eq, state, [pde.MaterialConservationTracker(interrupts=0.5)], t_range=5.0, dt=0.05)
            tracker = HipMaterialConservationTracker(interrupts=0.5)
            got, cgot = _solve(pde, eq, state, [tracker], t_range=5.0, dt=0.05)
            assert LINKS[-1][1] == 0
            assert cref["stop_reason"] == reason
            assert (cgot["t_final"], cgot["stop_reason"]) == (cref["t_final"], cref["stop_reason"])
            np.testing.assert_array_equal(got.data, ref.data)
        _, cname = _solve(pde, decay, state, ["hip_material_conservation"], t_range=5.0, dt=0.05)
        assert cname["stop_reason"] == "Material is not conserved"


def test_material_conservation_of_vector_fields_and_collections(pde):
    """A vector field (the norm over the components on the device) and a FieldCollection (not resident: the host path)."""
    from pde_hip.pypde_plugin import HipMaterialConservationTracker

    grid = pde.UnitGrid([16, 16], periodic=True)
    rng = np.random.default_rng(8)
    vec = pde.VectorField.random_uniform(grid, 0.5, 1.5, rng=rng)
    col = pde.FieldCollection([pde.ScalarField.random_uniform(grid, 0.5, 1.5, rng=rng), pde.ScalarField.random_uniform(grid, 2.5, 3.5, rng=rng)])
    eq_vec = pde.PDE({"u": "vector_laplace(u) - 0.0001 * u"})
    eq_col = pde.PDE({"a": "laplace(a) - 0.0001 * a", "b": "laplace(b)"})
    with stats_shimlib.use_shim():
        for eq, state, reason in ((eq_vec, vec, "Material is not conserved"), (eq_col, col, "Material of field [0] is not conserved")):
            ref, cref = _solve(pde, eq, state, [pde.MaterialConservationTracker(interrupts=0.5)], t_range=5.0, dt=0.05)
            got, cgot = _solve(pde, eq, state, [HipMaterialConservationTracker(interrupts=0.5)], t_range=5.0, dt=0.05)
            assert cref["stop_reason"] == reason
            assert (cgot["t_final"], cgot["stop_reason"]) == (cref["t_final"], cref["stop_reason"])
            np.testing.assert_array_equal(got.data, ref.data)
        # the device magnitude of a vector field is the reference's, and a collection's component slices give each field's own
        backend = pde.backends.get_backend("hip")
        from pde_hip.statistics import _components_of, device_magnitude

        dev = DeviceArray(backend.grid_info(grid, vec.dtype), (2,)).set_valid(vec.data)
        _close(device_magnitude(backend, vec, dev), vec.magnitude)
        three = pde.FieldCollection([col[0], vec, col[1]])
        dev3 = DeviceArray(backend.grid_info(grid, three.dtype), (4,)).set_valid(three.data)
        parts = _components_of(three, dev3)
        assert [p[1].comp_shape for p in parts] == [(), (2,), ()]
        _close([device_magnitude(backend, f, d) for f, d in parts], three.magnitudes)


def test_device_statistics_key_with_pypde(pde):
    """config["backend.hip.device_statistics"]: off by default; on, the properties of a resident state come from the device."""
    eq, state = _steady_problem(pde)
    seen = {}

    def callback(field, t):
        link = field.__dict__.get("_hip_link")
        if link is not None and link.host_stale:
            seen.setdefault("values", []).append((float(field.average), float(field.fluctuations), float(field.magnitude), float(field.integral)))
            seen.setdefault("downloads", []).append(link.downloads)

    with stats_shimlib.use_shim():
        backend = pde.backends.get_backend("hip")
        assert backend.device_statistics is False
        for flag in (True, False):
            backend.device_statistics = flag
            try:
                _solve(pde, eq, state, [pde.CallbackTracker(callback, interrupts=1.0)], t_range=4.0)
            finally:
                backend.device_statistics = None
            seen[flag] = (seen.pop("values"), seen.pop("downloads"))
    assert set(seen[True][1]) == {0}, seen[True][1]
    assert seen[False][1] == list(range(1, len(seen[False][1]) + 1))          # off: one download per interrupt, as before
    _close(seen[True][0][0], seen[False][0][0], 1e-12)
