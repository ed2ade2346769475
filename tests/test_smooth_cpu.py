"""Device smoothing without a GPU: the host shim with the smoothing entry point (tests/smooth_shimlib.py) stands in for the library.

* the numpy restatement of ``tests/smooth_cases.py`` against the reference's results (``tests/golden/smooth.npz``) and against
  ``scipy.ndimage.gaussian_filter1d`` where scipy imports, bit for bit; ``pde_hip.smoothing.gaussian_weights`` against the stored weights;
* the shim's plain C version of ``pdehip_smooth_axis`` against the restatement on the shapes of the GPU test, and its refusals;
* the Python side (``pde_hip/smoothing.py``, the resident-field method under ``device_smoothing``) through the mirror classes and, where
  py-pde is importable, through the real fields: every form of result, the residency counters, a stepper continuing from a state
  smoothed in place, and the cases that take the host path.
The kernels are tested on the GPU (tests/test_hip_smooth.py)."""

from __future__ import annotations

import numpy as np
import pytest

import pde_hip
import project_shimlib
import refpath
import shimlib
import smooth_cases as G
import smooth_shimlib
import stats_shimlib
from pde_hip import _abi, smoothing
from pde_hip.device import DeviceArray

IDS = ["f64", "f32"]
MODE_IDS = ["wrap", "reflect"]


@pytest.fixture
def shim():
    with smooth_shimlib.use_shim() as lib:
        yield lib


@pytest.fixture
def pde():
    mod = refpath.import_reference()
    if mod is None:
        pytest.skip("py-pde (reference) not available")
    import pde_hip.pypde_plugin  # noqa: F401

    return mod


def test_abi_table():
    assert _abi.ABI_VERSION == 8 and hasattr(pde_hip, "smooth")
    assert "smooth_axis" in _abi.OPTIONAL_PROTOTYPES
    assert "smooth_axis" not in set(_abi.COMPUTE_PROTOTYPES) | set(_abi.COMM_PROTOTYPES) | set(_abi.RUNTIME_PROTOTYPES)
    assert (_abi.SMOOTH_WRAP, _abi.SMOOTH_REFLECT, _abi.SMOOTH_CELL) == (G.WRAP, G.REFLECT, G.CELL)


def test_other_shims_lack_the_entry_point_and_still_load():
    for other in (shimlib, stats_shimlib, project_shimlib):
        with other.use_shim() as lib:
            assert not lib.has("smooth_axis")
    with smooth_shimlib.use_shim() as lib:
        assert lib.has("smooth_axis", "project", "extract_box", "field_stats")


# ---- restatement, weights, golden, scipy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(G.GOLDEN))
def test_restatement_equals_the_reference(cid):
    """Axis by axis on the reference's own intermediate results, and chained, with weights computed here: bit for bit."""
    cls, dtype, shape, periodic, dx, sigma = G.GOLDEN[cid]
    data = G.golden()
    stage = chained = G.golden_input(cid).reshape((-1, *shape))
    for axis in range(len(shape)):
        r, w = smoothing.gaussian_weights(sigma / dx[axis])
        stored = data[f"{cid}/w{axis}"]
        assert r == len(stored) - 1 and np.array_equal(G.bits(w), G.bits(stored)) and np.array_equal(G.bits(G.gaussian_weights(sigma / dx[axis])), G.bits(stored))
        mode = G.WRAP if periodic[axis] else G.REFLECT
        ref = data[f"{cid}/axis{axis}"].reshape(stage.shape)
        G.assert_same(G.filter_axis(stage, axis, stored, mode), ref, f"{cid} axis {axis}")
        G.assert_same(smoothing.host_filter_axis(stage, 1 + axis, stored, bool(periodic[axis])), ref, f"{cid} axis {axis} (package)")
        chained = G.filter_axis(chained, axis, w, mode)
        stage = ref
    G.assert_same(chained, data[f"{cid}/out"].reshape(chained.shape), f"{cid} chained")
    assert str(chained.dtype) == dtype


@pytest.mark.parametrize("dtype", G.DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", G.MODES, ids=MODE_IDS)
def test_restatement_equals_scipy(mode, dtype):
    """1-D to 3-D, every axis, sigma from 0.3 to 6 cells, extents down to 1 cell below a radius of 24."""
    ndimage = pytest.importorskip("scipy.ndimage")
    for shape in ((1,), (3,), (13,), (4, 9), (2, 1, 5), (3, 6, 7)):
        valid = G.drawn(shape, 2, np.dtype(dtype).name, planted=len(shape) == 2)
        for axis in range(len(shape)):
            for sigma in (0.3, 0.7, 1.0, 2.4, 6.0):
                w = G.gaussian_weights(sigma)
                with np.errstate(invalid="ignore"):
                    ref = ndimage.gaussian_filter1d(valid, sigma=sigma, axis=1 + axis, mode="wrap" if mode == G.WRAP else "reflect")
                G.assert_same(G.filter_axis(valid, axis, w, mode), ref, f"{shape} axis {axis} sigma {sigma}")


def test_tiling_cases_cover_what_they_claim():
    seen_n, seen_n2 = set(), set()
    for kind in G.TILING_KINDS:
        for shape, axis, ncomp in G.tiling_cases(kind):
            seen_n.add(shape[axis])
            if kind != "row":
                seen_n2.add(shape[-1])
    assert seen_n == set(G.EXTENTS) >= {G.MARCH_LENGTH - 1, G.MARCH_LENGTH, G.MARCH_LENGTH + 1, 2 * G.MARCH_LENGTH + 1} and seen_n2 == set(G.FASTEST)
    assert all(G.turn_workgroups(key) > G.BLOCKS_MAX for key in G.TURN)
    assert G.ROW_PIECES * (G.ROW_LANES + 2 * G.ROW_RADIUS_MAX) * 8 <= 40960 < G.ROW_PIECES * (G.ROW_LANES + 2 * G.ROW_RADIUS_MAX + 2) * 8
    assert (G.MARCH_LENGTH + 2 * G.MARCH_RADIUS_MAX) * G.MARCH_WIDTH * 8 <= 40960 < (G.MARCH_LENGTH + 2 * G.MARCH_RADIUS_MAX + 2) * G.MARCH_WIDTH * 8


# ---- the shim entry -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", G.DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", G.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("kind", G.TILING_KINDS)
def test_shim_equals_the_restatement(shim, kind, mode, dtype):
    for shape, axis, ncomp in G.tiling_cases(kind)[::2]:
        valid = G.drawn(shape, ncomp, np.dtype(dtype).name, planted=shape[axis] == 65)
        for r in G.radii(shape[axis])[1::2]:
            G.check_pass(shim, valid, shape, axis, G.radius_weights(r), mode, f"{shape} axis {axis} r {r}", device=False)


@pytest.mark.parametrize("cid", sorted(G.GOLDEN))
def test_shim_golden(shim, cid):
    G.check_golden_passes(shim, cid, device=False)


def test_entry_point_refuses_bad_arguments(shim):
    G.refuse_bad_arguments(shim)


# ---- the Python side through the mirror classes -------------------------------------------------------------------------------------
MIRROR_CLASSES = {"ScalarField": pde_hip.ScalarField, "VectorField": pde_hip.VectorField, "Tensor2Field": pde_hip.Tensor2Field}


def mirror_golden(cid):
    cls, dtype, shape, periodic, dx, sigma = G.GOLDEN[cid]
    grid = pde_hip.CartesianGrid(G.golden_bounds(cid), shape, periodic=list(periodic))
    return MIRROR_CLASSES[cls](grid, G.golden_input(cid), dtype=dtype, label="c"), sigma, G.golden()[f"{cid}/out"]


@pytest.mark.parametrize("cid", sorted(G.GOLDEN))
def test_every_result_form_on_mirror_fields(shim, cid):
    """A host field (uploaded once) through ``pde_hip.smooth``: a new field, ``device=True``, in place, into another field; a bare device
    array; and the mirror method (the host path) - all the reference's bits."""
    backend = pde_hip.get_backend("hip")
    field, sigma, ref = mirror_golden(cid)
    before = field.data.copy()
    new = pde_hip.smooth(field, sigma)
    assert type(new) is type(field) and new is not field and new.label == "c" and new.dtype == field.dtype and new.grid is field.grid
    G.assert_same(new.data, ref, "new field")
    assert np.array_equal(field.data, before)
    dev = pde_hip.smooth(field, sigma, device=True)
    assert isinstance(dev, DeviceArray) and dev.comp_shape == field.data_shape
    G.assert_same(dev.get_valid(), ref, "device=True")
    other = field.copy(label="other")
    assert pde_hip.smooth(field, sigma, out=other, label="named") is other and other.label == "named"
    G.assert_same(other.data, ref, "out=other")
    # a bare device array: the grid is needed for the periodicity
    again = backend.make_smoother(field.grid)(dev, sigma)
    G.assert_same(again, field.smooth(sigma, out=field.copy()).smooth(sigma, out=field.copy()).data, "bare array, smoothed twice")
    twice = backend.make_smoother(field.grid)(dev, sigma, device=True)
    assert isinstance(twice, DeviceArray) and twice.ptr != dev.ptr and np.array_equal(G.bits(twice.get_valid()), G.bits(again))
    with pytest.raises(TypeError):
        backend.make_smoother()(dev, sigma)
    with pytest.raises(ValueError):
        pde_hip.smooth(field, sigma, out=other, device=True)
    # the mirror method itself: numpy, no scipy
    G.assert_same(field.smooth(sigma, out=field.copy()).data, ref, "mirror method")
    work = field.copy()
    assert pde_hip.smooth(work, sigma, out=work) is work
    G.assert_same(work.data, ref, "in place on a host field")
    plain = field.smooth(sigma)
    assert plain.dtype == np.float64      # (the reference allocates `out` without a dtype)
    if field.dtype == np.float64:
        G.assert_same(plain.data, ref, "mirror method, new field")


def test_incompatible_out_is_refused_like_the_method_refuses(shim):
    field, sigma, _ = mirror_golden("s2d")
    vec, _, _ = mirror_golden("v3d")
    for call in (lambda: pde_hip.smooth(field, sigma, out=vec), lambda: field.smooth(sigma, out=vec)):
        with pytest.raises(TypeError):
            call()
    other_grid = pde_hip.ScalarField(pde_hip.UnitGrid([9, 7]), 1.0)
    for call in (lambda: pde_hip.smooth(field, sigma, out=other_grid), lambda: field.smooth(sigma, out=other_grid)):
        with pytest.raises(ValueError):
            call()


def test_resident_run_through_the_mirror(shim):
    for dtype in G.DTYPES:
        G.resident_run_checks(pde_hip.get_backend("hip"), dtype)


def test_device_smoothing_key_through_the_mirror(shim):
    """``device_smoothing`` off (the default): ``state.smooth`` pulls the state; on: it does not, and gives the same bits."""
    backend = pde_hip.get_backend("hip")
    assert backend.device_smoothing is False
    seen = {}
    for flag in (True, False):
        rows = seen[flag] = []

        def tracker(field, t, rows=rows):
            link = field.__dict__.get("_hip_link")
            if link is None or not link.host_stale:
                return
            before = link.downloads
            rows.append((field.smooth(1.5, label="coarse"), before, link.downloads, link.host_stale))

        backend.device_smoothing = flag
        try:
            G.run_mirror(backend, tracker)
        finally:
            backend.device_smoothing = None
    assert len(seen[True]) >= 3 and len(seen[True]) == len(seen[False])
    for (got, before, after, stale), (ref, ref_before, ref_after, ref_stale) in zip(seen[True], seen[False]):
        assert before == after == 0 and stale and ref_after == ref_before + 1 and not ref_stale
        assert type(got) is pde_hip.ScalarField and got.label == ref.label == "coarse" and np.array_equal(G.bits(got.data), G.bits(ref.data))


def test_host_paths_of_the_mirror(shim):
    """Complex fields, collections, a sigma that is no positive finite scalar and a library without the entry point: the host path."""
    grid = pde_hip.CartesianGrid([(0, 3.0), (0, 8.0)], (6, 8), periodic=[True, False])
    rng = np.random.default_rng(4)
    sca = pde_hip.ScalarField(grid, rng.uniform(0.5, 1.5, grid.shape))
    vec = pde_hip.VectorField(grid, rng.uniform(0.5, 1.5, (2, *grid.shape)))
    cplx = pde_hip.ScalarField(grid, rng.uniform(0.5, 1.5, grid.shape) + 1j * rng.uniform(0.5, 1.5, grid.shape))
    np.testing.assert_array_equal(pde_hip.smooth(cplx, 0.8, out=cplx.copy()).data,
                                  pde_hip.smooth(pde_hip.ScalarField(grid, cplx.data.real), 0.8).data + 1j * pde_hip.smooth(pde_hip.ScalarField(grid, cplx.data.imag), 0.8).data)
    col = pde_hip.FieldCollection([sca, vec])
    res = pde_hip.smooth(col, 0.8)
    assert isinstance(res, pde_hip.FieldCollection) and res is not col
    assert np.array_equal(res[0].data, pde_hip.smooth(sca, 0.8).data) and np.array_equal(res[1].data, pde_hip.smooth(vec, 0.8).data)
    assert np.array_equal(col.smooth(0.8).data, res.data)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            pde_hip.smooth(sca, bad)
    expect = pde_hip.smooth(sca, 0.8).data
    with project_shimlib.use_shim() as lib:
        assert not lib.has("smooth_axis")
        assert np.array_equal(pde_hip.smooth(sca, 0.8).data, expect)


# ---- through the real py-pde --------------------------------------------------------------------------------------------------------
def _problem(pde, dtype=np.float64, shape=(8, 6, 10), cls="ScalarField"):
    grid = pde.CartesianGrid([(0.0, 1.5 * n) for n in shape], shape, periodic=[True, False, True])
    rank = {"ScalarField": 0, "VectorField": 1}[cls]
    data = G.S.draw(shape, 3 ** rank, dtype, seed=4).reshape((3,) * rank + shape)
    return getattr(pde, cls)(grid, data, label="c", dtype=dtype)


def _solve(pde, eq, state, trackers, **kw):
    return eq.solve(state, t_range=1.0, dt=0.05, solver="euler", backend="hip", tracker=trackers, **kw)


@pytest.mark.parametrize("cid", sorted(G.GOLDEN))
def test_pypde_host_fields_equal_the_reference_method(pde, cid):
    cls, dtype, shape, periodic, dx, sigma = G.GOLDEN[cid]
    grid = pde.CartesianGrid(G.golden_bounds(cid), shape, periodic=list(periodic))
    field = getattr(pde, cls)(grid, G.golden_input(cid), dtype=dtype, label="c")
    ref = field.smooth(sigma, out=field.copy())
    G.assert_same(ref.data, G.golden()[f"{cid}/out"], "the reference here against the stored one")
    with smooth_shimlib.use_shim():
        new = pde_hip.smooth(field, sigma)
        assert type(new) is type(field) and new.label == "c" and new.grid is grid
        G.assert_same(new.data, ref.data, "new field")
        G.assert_same(pde_hip.smooth(field, sigma, device=True).get_valid(), ref.data, "device=True")
        other = field.copy()
        assert pde_hip.smooth(field, sigma, out=other, label="s") is other and other.label == "s"
        G.assert_same(other.data, ref.data, "out=other")


@pytest.mark.parametrize("dtype", G.DTYPES, ids=IDS)
def test_pypde_resident_state(pde, dtype):
    """A ``backend="hip"`` run of the real py-pde whose tracker smooths the resident state: ``device=True`` into the statistics and the
    slicer, a host result, in place once; the counters do not move, and the stepper continues from the smoothed state."""
    state = _problem(pde, dtype)
    eq = pde.DiffusionPDE(1.0)
    rows, count = [], []

    def tracker(field, t):
        link = field.__dict__.get("_hip_link")
        if link is None or not link.host_stale:
            return
        counters = (link.downloads, link.uploads)
        pulled = pde.ScalarField(field.grid, link.dev_state.get_valid(), label=field.label, dtype=dtype)
        dev = pde_hip.smooth(field, 2.0, device=True)
        row = {"pulled": pulled, "dev": dev.get_valid(), "host": pde_hip.smooth(field, 2.0), "stats": pde_hip.field_statistics(dev),
               "cut": link.backend.make_slicer(field.grid)(dev, {"x": "mid"})}
        if len(rows) == 1:
            assert pde_hip.smooth(field, 1.0, out=field) is field
            row["in_place"] = link.dev_state.get_valid()
        assert (link.downloads, link.uploads) == counters and link.host_stale
        rows.append(row)

    def host_tracker(field, t):
        link = field.__dict__.get("_hip_link")
        if link is None or not link.host_stale:
            return
        if len(count) == 1:
            field.smooth(1.0, out=field)
        count.append(t)

    with smooth_shimlib.use_shim():
        res = _solve(pde, eq, state, [pde.CallbackTracker(tracker, interrupts=0.25)])
        assert res.__dict__["_hip_link"].downloads == 0
        plain = _solve(pde, eq, state, [pde.CallbackTracker(host_tracker, interrupts=0.25)])
        untouched = _solve(pde, eq, state, None)
        assert np.array_equal(res.data, plain.data) and not np.array_equal(res.data, untouched.data)
    assert len(rows) >= 3
    for row in rows:
        ref = row["pulled"].smooth(2.0, out=row["pulled"].copy())
        G.assert_same(row["dev"], ref.data, "device=True")
        assert type(row["host"]) is pde.ScalarField and row["host"].label == "c"
        G.assert_same(row["host"].data, ref.data, "host result")
        assert np.array_equal(row["cut"], ref.slice({"x": "mid"}).data)
        np.testing.assert_allclose(row["stats"].average, ref.average, rtol=1e-6 if dtype == np.float32 else 1e-13)
        if "in_place" in row:
            G.assert_same(row["in_place"], row["pulled"].smooth(1.0, out=row["pulled"].copy()).data, "in place")


def test_device_smoothing_key_with_pypde(pde):
    """config["backend.hip.device_smoothing"]: off by default, ``state.smooth`` downloads; on, it leaves the state on the device."""
    state = _problem(pde)
    eq = pde.DiffusionPDE(1.0)
    seen = {}

    def tracker(field, t):
        link = field.__dict__.get("_hip_link")
        if link is None or not link.host_stale:
            return
        before = link.downloads
        got = field.smooth(1.5, label="coarse")
        seen["rows"].append((got, before, link.downloads, link.host_stale))

    with smooth_shimlib.use_shim():
        backend = pde.backends.get_backend("hip")
        assert backend.device_smoothing is False and pde.config["backend.hip.device_smoothing"] is False
        for flag in (True, False):
            seen["rows"] = []
            backend.device_smoothing = flag
            try:
                _solve(pde, eq, state, [pde.CallbackTracker(tracker, interrupts=0.25)])
            finally:
                backend.device_smoothing = None
            seen[flag] = seen.pop("rows")
    assert len(seen[True]) >= 3 and len(seen[True]) == len(seen[False])
    for (got, before, after, stale), (ref, ref_before, ref_after, ref_stale) in zip(seen[True], seen[False]):
        assert before == after == 0 and stale and ref_after == ref_before + 1 and not ref_stale
        assert type(got) is pde.ScalarField and got.label == ref.label == "coarse" and np.array_equal(got.data, ref.data)


def test_pypde_host_paths(pde):
    """Complex states, collections, a vector state (device), a cylindrical grid, a sigma that is no positive finite scalar, a library
    without the entry point: the reference's own results, no error of ours."""
    grid = pde.UnitGrid([6, 5, 4], periodic=[True, False, True])
    rng = np.random.default_rng(6)
    sca = pde.ScalarField(grid, rng.uniform(0.5, 1.5, grid.shape))
    cplx = pde.ScalarField(grid, rng.uniform(0.5, 1.5, grid.shape) + 1j * rng.uniform(0.5, 1.5, grid.shape))
    vec = pde.VectorField.random_uniform(grid, 0.5, 1.5, rng=rng)
    col = pde.FieldCollection([sca, vec])
    cyl = pde.ScalarField.random_uniform(pde.CylindricalSymGrid(3.0, (0.0, 4.0), (6, 8)), rng=rng)
    with smooth_shimlib.use_shim():
        for field in (cplx, vec, cyl, col):
            got, ref = pde_hip.smooth(field, 0.9, out=field.copy()), field.smooth(0.9, out=field.copy())
            assert type(got) is type(ref) and np.array_equal(got.data, ref.data)
        for bad in (0.0, -1.0):
            try:
                ref = sca.smooth(bad)
            except Exception as err:  # noqa: BLE001 - whatever scipy says about it
                with pytest.raises(type(err)):
                    pde_hip.smooth(sca, bad)
            else:
                assert np.array_equal(pde_hip.smooth(sca, bad).data, ref.data, equal_nan=True)
    with project_shimlib.use_shim() as lib:
        assert not lib.has("smooth_axis")
        assert np.array_equal(pde_hip.smooth(sca, 0.9).data, sca.smooth(0.9).data)
