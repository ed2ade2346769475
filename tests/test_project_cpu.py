"""Device projections without a GPU: the host shim with the two projection entry points (tests/project_shimlib.py) stands in for the
library.

* the shim's plain C versions of ``pdehip_project`` / ``pdehip_extract_box`` against the numpy restatement and the bounds of
  ``tests/project_cases.py``, on the shapes of the GPU test - and numpy's own results against the same bounds: this keeps restatement,
  bounds and shim honest;
* the Python side (``pde_hip/projection.py``, the resident-field methods under ``device_projections``) through the mirror classes;
* where py-pde is importable, ``backend="hip"`` runs whose trackers project and slice the state, against the reference's own methods on
  pulled copies, and the cases that take the host path (a library without the entry points, complex and vector states, collections).
The kernels are tested on the GPU (tests/test_hip_project.py)."""

from __future__ import annotations

import itertools

import numpy as np
import pytest

import pde_hip
import project_cases as P
import project_shimlib
import refpath
import shimlib
import stats_shimlib
from pde_hip import _abi
from pde_hip.device import DeviceArray, DeviceBuffer

IDS = ["f64", "f32"]


@pytest.fixture
def shim():
    with project_shimlib.use_shim() as lib:
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
    assert {"project", "extract_box"} <= set(_abi.OPTIONAL_PROTOTYPES)
    assert not {"project", "extract_box"} & (set(_abi.COMPUTE_PROTOTYPES) | set(_abi.COMM_PROTOTYPES) | set(_abi.RUNTIME_PROTOTYPES))


def test_other_shims_lack_the_entry_points_and_still_load():
    for other in (shimlib, stats_shimlib):
        with other.use_shim() as lib:
            assert not lib.has("project") and not lib.has("extract_box")
    with project_shimlib.use_shim() as lib:
        assert lib.has("project", "extract_box", "field_stats")


def test_expected_chain_of_instances():
    """The restatement of the host's chaining: row reductions while the fastest axis goes, marches in segments for the slower ones."""
    f64, f32 = np.float64, np.float32
    assert P.expected_chain((4, 6, 8), f64, 0b100, P.SUM) == "project_row_kernel<double,2,sum>"
    assert P.expected_chain((4, 6, 8), f32, 0b111, P.MIN) == "project_row_kernel<float,4,max>+project_row_kernel<double,1,max>+project_row_kernel<double,1,max>"
    assert P.expected_chain((4, 6, 7), f64, 0b101, P.MAX) == "project_row_kernel<double,1,max>+project_march_kernel<double,1,max>"
    assert P.expected_chain((129, 2, 8), f32, 0b001, P.SUM) == "project_march_kernel<float,4,sum>+project_march_kernel<double,1,sum>"
    assert P.expected_chain((128, 8), f64, 0b01, P.SUM) == "project_march_kernel<double,2,sum>"
    assert P.expected_chain((9,), f64, 0b1, P.SUM) == "project_row_kernel<double,1,sum>"


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
@pytest.mark.parametrize("case", P.SMALL, ids=P.S.case_id)
def test_shim_project(shim, case, dtype):
    shape, ncomp = case
    for planted in (False, True):
        P.check_all_methods(shim, P.small_inputs(case, np.dtype(dtype).name, planted), shape, what=f"planted={planted}")


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
@pytest.mark.parametrize("case", P.SMALL, ids=P.S.case_id)
def test_numpy_lies_inside_the_bounds(case, dtype):
    """numpy's own sums against ``math.fsum`` and the bound of the kernels: the bound tests the summation, not the inputs."""
    shape, ncomp = case
    for planted in (False, True):
        valid = P.small_inputs(case, np.dtype(dtype).name, planted)
        for mask in P.masks(len(shape)):
            P.check_sum(P.np_project(valid, mask, P.SUM), valid, mask, what=f"numpy mask {mask:03b}")


@pytest.mark.parametrize("key", sorted(P.MARCH_INSTANCES))
def test_shim_segment_extents(shim, key):
    dtype, n2 = P.MARCH_INSTANCES[key]
    for m in P.SEGMENT_EXTENTS:
        for shape in ((m, 2, n2), (3, -(-m // 3), n2)):
            valid = P.drawn(shape, 1, np.dtype(dtype).name)
            dev = P.upload(shim, shape, valid)
            for mask in (0b001, 0b011):
                P.check_sum(P.project(shim, dev, mask, P.SUM), valid, mask, what=f"{key} {shape} mask {mask:03b}")
                P.check_extreme(P.project(shim, dev, mask, P.MAX), valid, mask, P.MAX, what=f"{key} {shape} mask {mask:03b}")


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
@pytest.mark.parametrize("case", [c for c in P.SMALL if c[1] == 3 or len(c[0]) < 3][:14] + [((5, 4, 7), 3)], ids=P.S.case_id)
def test_shim_boxes(shim, case, dtype):
    shape, ncomp = case
    P.check_boxes(shim, P.small_inputs(case, np.dtype(dtype).name, False), shape)


def test_entry_points_refuse_bad_arguments(shim):
    P.refuse_bad_arguments(shim)


# ---- the Python side through the mirror classes -------------------------------------------------------------------------------------


def mirror_field(shape, dtype=np.float64, seed=3):
    grid = pde_hip.CartesianGrid([(0.0, 1.5 * n) for n in shape], shape)
    return pde_hip.ScalarField(grid, P.S.draw(shape, 1, dtype, seed=seed)[0], label="c")


def on_device(backend, field) -> DeviceArray:
    return DeviceArray(backend.grid_info(field.grid, field.dtype), field.data_shape).set_valid(field.data)


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(6, 5, 7), (9, 4), (11,)])
def test_projector_and_slicer_device_and_host_agree(shim, shape, dtype):
    backend = pde_hip.get_backend("hip")
    field = mirror_field(shape, dtype)
    grid, dev = field.grid, on_device(backend, field)
    projector, slicer = backend.make_projector(grid), backend.make_slicer(grid)
    for count in range(1, len(shape) + (0 if len(shape) > 1 else 1)):
        for ax_remove in itertools.combinations(range(len(shape)), count):
            axes = [grid.axes[a] for a in ax_remove]
            weight = float(np.prod([grid.discretization[a] for a in ax_remove]))
            for method in P.METHOD_NAMES:
                got = projector(dev, axes, method=method)
                if len(ax_remove) == len(shape):
                    continue
                ref = field.project(axes, method=method)
                assert pde_hip.project(field, axes, method=method).data.tobytes() == ref.data.tobytes()      # host data: the host path
                P.check_against_reference(pde_hip.ScalarField(ref.grid, got), ref, np.ascontiguousarray(field.data), ax_remove, method, weight)
    for ax, where in itertools.product(range(len(shape)), ("low", "mid", "high", 0.0, 2.3, 1.5 * shape[0] if len(shape) == 1 else 4.4)):
        if len(shape) == 1:
            continue
        position = {grid.axes[ax]: where}
        ref = field.slice(position)
        got = slicer(dev, position)
        assert got.dtype == ref.data.dtype and np.array_equal(P.bits(got), P.bits(np.ascontiguousarray(ref.data)))
        assert list(ref.grid.axes) == [a for a in grid.axes if a != grid.axes[ax]]
    if len(shape) == 3:
        both = slicer(dev, {"x": "mid", "z": 1.0})
        assert np.array_equal(both, field.slice({"x": "mid", "z": 1.0}).data)


def test_messages_are_the_mirror_methods_own(shim):
    backend = pde_hip.get_backend("hip")
    field = mirror_field((6, 5, 7))
    dev = on_device(backend, field)
    projector, slicer = backend.make_projector(field.grid), backend.make_slicer(field.grid)
    calls = [(lambda f: f(["x", "w"]), "project"), (lambda f: f("x", method="median"), "project"), (lambda f: f({"w": 1.0}), "slice"),
             (lambda f: f({"x": "centre"}), "slice"), (lambda f: f({"y": -0.1}), "slice"), (lambda f: f({"y": 7.6}), "slice")]
    for call, name in calls:
        with pytest.raises(ValueError) as ref:
            call(getattr(field, name))
        with pytest.raises(ValueError) as got:
            call(lambda *a, **k: (projector if name == "project" else slicer)(dev, *a, **k))
        expect = str(ref.value).replace(repr(field.grid), "GRID")
        assert str(got.value).replace(repr(field.grid), "GRID") == expect and type(got.value) is type(ref.value), (str(got.value), str(ref.value))
    with pytest.raises(pde_hip.projection.DomainError):
        slicer(dev, {"y": 7.6})


def test_resident_run_through_the_mirror(shim):
    for dtype in P.DTYPES:
        P.resident_run_checks(pde_hip.get_backend("hip"), dtype)


def test_resident_key_through_the_mirror(shim):
    backend = pde_hip.get_backend("hip")
    assert backend.device_projections is False
    P.resident_key_checks(backend)


def test_host_paths_of_the_mirror(shim):
    """Vector fields, collections and a library without the entry points: the host path, no error."""
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.UnitGrid([4, 5, 6])
    rng = np.random.default_rng(2)
    vec = pde_hip.VectorField.random_uniform(grid, rng=rng)
    sca = pde_hip.ScalarField.random_uniform(grid, rng=rng)
    got = pde_hip.project(vec, "y", method="max")
    assert np.array_equal(got, vec.data.max(axis=2))
    assert np.array_equal(pde_hip.slice_field(vec, {"z": "low"}), vec.data[..., 0])
    col = pde_hip.project(pde_hip.FieldCollection([sca, vec]), "x")
    assert len(col) == 2 and col[0].data.tobytes() == sca.project("x").data.tobytes() and np.shape(col[1]) == (3, 5, 6)
    dev = on_device(backend, sca)
    with stats_shimlib.use_shim():
        assert np.array_equal(backend.make_projector(grid)(dev, "z"), sca.project("z").data)
        assert np.array_equal(backend.make_slicer(grid)(dev, {"x": "mid"}), sca.slice({"x": "mid"}).data)


# ---- through the real py-pde --------------------------------------------------------------------------------------------------------
def _problem(pde, dtype=np.float64, shape=(8, 6, 10)):
    grid = pde.CartesianGrid([(0.0, 1.5 * n) for n in shape], shape, periodic=[True, False, True])
    state = pde.ScalarField(grid, P.S.draw(shape, 1, dtype, seed=4)[0], label="c")
    return pde.DiffusionPDE(1.0), state


def _solve(pde, eq, state, trackers, **kw):
    return eq.solve(state, t_range=1.0, dt=0.05, solver="euler", backend="hip", tracker=trackers, **kw)


def test_trackers_that_project_keep_the_state_on_the_device(pde):
    """A DataTracker and a StorageTracker(transformation=...) that call pde_hip.project / pde_hip.slice_field, against the reference methods
    on pulled copies; the final state has the bits of the run without trackers."""
    eq, state = _problem(pde)
    weight_z = float(state.grid.discretization[2])
    pulled, downloads = [], []

    def probe(field, t):
        link = field.__dict__.get("_hip_link")
        if link is not None and link.host_stale:
            pulled.append(pde.ScalarField(field.grid, link.dev_state.get_valid(), label=field.label))
            downloads.append(link)

    def record(field, t):
        line = pde_hip.slice_field(field, {"x": "mid", "z": "low"})
        return {"max": pde_hip.project(field, ["x", "y", "z"][:2], method="max").data.copy(), "line": line.data.copy()}

    with project_shimlib.use_shim():
        plain = _solve(pde, eq, state, None)
        data_tracker = pde.DataTracker(record, interrupts=0.25)
        storage = pde.MemoryStorage()
        trackers = [pde.CallbackTracker(probe, interrupts=0.25), data_tracker,
                    storage.tracker(interrupts=0.25, transformation=lambda f: pde_hip.project(f, "z"))]
        got = _solve(pde, eq, state, trackers)
        assert downloads and all(link.downloads == 0 for link in downloads)
        assert np.array_equal(got.data, plain.data)
    resident = len(pulled)
    assert resident >= 3 and len(storage) >= resident
    for ref_state, stored, row in zip(pulled[::-1], list(storage)[::-1], data_tracker.data[::-1]):
        data = np.ascontiguousarray(ref_state.data)
        ref = ref_state.project("z")
        assert stored.grid == ref.grid
        P.check_against_reference(stored, ref, data, (2,), "integral", weight_z)
        assert np.array_equal(row["max"], ref_state.project(["x", "y"], method="max").data)
        assert np.array_equal(row["line"], ref_state.slice({"x": "mid", "z": "low"}).data)


def test_device_projections_key_with_pypde(pde):
    """config["backend.hip.device_projections"]: off by default, the methods download and return numpy's bits; on, a plain
    ``state.project("z")`` in a tracker leaves the state on the device."""
    eq, state = _problem(pde)
    weight_z = float(state.grid.discretization[2])
    seen = {}

    def tracker(field, t):
        link = field.__dict__.get("_hip_link")
        if link is None or not link.host_stale:
            return
        ref = pde.ScalarField(field.grid, link.dev_state.get_valid(), label=field.label)
        before = link.downloads
        got = field.project("z")
        extra = (field.slice({"y": "mid"}), field.get_line_data(extract="project_y"), field.get_image_data(), field.project("x", method="min")) if seen["flag"] else ()
        seen.setdefault("rows", []).append((got, extra, ref, before, link.downloads))
        if seen["flag"] and t > 0.7:
            # any `scalar=` other than "auto" is the reference method's business: it reads the data, the state comes down
            norm = field.get_line_data(scalar="norm", extract="cut_z")
            seen["norm"] = (norm, ref.get_line_data(scalar="norm", extract="cut_z"), link.downloads - seen["rows"][-1][4])

    with project_shimlib.use_shim():
        backend = pde.backends.get_backend("hip")
        assert backend.device_projections is False
        plain = _solve(pde, eq, state, None)
        for flag in (True, False):
            seen["flag"] = flag
            backend.device_projections = flag
            try:
                res = _solve(pde, eq, state, [pde.CallbackTracker(tracker, interrupts=0.25)])
            finally:
                backend.device_projections = None
            seen[flag] = seen.pop("rows")
            assert np.array_equal(res.data, plain.data)
    assert len(seen[True]) >= 3 and len(seen[False]) >= 3
    assert seen[True][0][3] == 0
    for got, extra, ref, before, after in seen[True]:
        assert before == after      # (0 until the one call with scalar="norm" below, 1 after it)
        data = np.ascontiguousarray(ref.data)
        P.check_against_reference(got, ref.project("z"), data, (2,), "integral", weight_z)
        assert np.array_equal(extra[0].data, ref.slice({"y": "mid"}).data) and extra[0].grid == ref.slice({"y": "mid"}).grid
        line = ref.get_line_data(extract="project_y")
        np.testing.assert_allclose(extra[1]["data_y"], line["data_y"], rtol=1e-13)
        assert extra[1]["label_y"] == line["label_y"] and extra[1]["label_x"] == "y"
        image = ref.get_image_data()
        assert np.array_equal(extra[2]["data"], image["data"]) and extra[2]["extent"] == image["extent"] and extra[2]["title"] == "c"
        assert np.array_equal(extra[3].data, ref.project("x", method="min").data)
    for got, _, ref, before, after in seen[False]:
        assert after == before + 1
        assert got.data.tobytes() == ref.project("z").data.tobytes()
    norm, ref_norm, downloads = seen["norm"]
    assert downloads == 1 and np.array_equal(norm["data_y"], ref_norm["data_y"]) and norm["label_y"] == ref_norm["label_y"]


def test_messages_are_the_references_own(pde):
    eq, state = _problem(pde)
    errors = []

    def tracker(field, t):
        link = field.__dict__.get("_hip_link")
        if link is None or not link.host_stale or errors:
            return
        calls = [lambda f, p, s: p(f, ["x", "w"]), lambda f, p, s: p(f, "x", method="median"), lambda f, p, s: s(f, {"w": 1.0}),
                 lambda f, p, s: s(f, {"x": "centre"}), lambda f, p, s: s(f, {"y": -0.1}), lambda f, p, s: s(f, {"z": 99.0})]
        ref_field = pde.ScalarField(field.grid, link.dev_state.get_valid())
        for call in calls:
            with pytest.raises(ValueError) as ref:
                call(ref_field, lambda f, *a, **k: f.project(*a, **k), lambda f, *a, **k: f.slice(*a, **k))
            with pytest.raises(ValueError) as got:
                call(field, pde_hip.project, pde_hip.slice_field)
            errors.append((type(got.value), str(got.value), type(ref.value), str(ref.value)))
        assert link.downloads == 0

    with project_shimlib.use_shim():
        _solve(pde, eq, state, [pde.CallbackTracker(tracker, interrupts=0.25)])
    assert len(errors) == 6
    for got_type, got_msg, ref_type, ref_msg in errors:
        assert got_type is ref_type and got_msg == ref_msg
    from pde.grids.base import DomainError

    assert errors[-1][0] is DomainError and errors[-2][0] is DomainError


def test_complex_vector_and_collection_states_take_the_host_path(pde):
    grid = pde.UnitGrid([6, 5, 4], periodic=True)
    rng = np.random.default_rng(6)
    cplx = pde.ScalarField(grid, rng.uniform(0.5, 1.5, grid.shape) + 1j * rng.uniform(0.5, 1.5, grid.shape))
    vec = pde.VectorField.random_uniform(grid, 0.5, 1.5, rng=rng)
    col = pde.FieldCollection([pde.ScalarField.random_uniform(grid, 0.5, 1.5, rng=rng), pde.ScalarField.random_uniform(grid, 2.5, 3.5, rng=rng)])
    seen = []

    def tracker(field, t):
        seen.append((pde_hip.project(field, "z"), pde_hip.slice_field(field, {"x": "mid"}), field.copy()))

    with project_shimlib.use_shim():
        backend = pde.backends.get_backend("hip")
        backend.device_projections = True
        try:
            for eq, state in ((pde.DiffusionPDE(1.0), cplx), (pde.PDE({"u": "vector_laplace(u)"}), vec), (pde.PDE({"a": "laplace(a)", "b": "laplace(b)"}), col)):
                del seen[:]
                eq.solve(state, t_range=0.2, dt=0.05, solver="euler", backend="hip", tracker=[pde.CallbackTracker(tracker, interrupts=0.1)])
                assert len(seen) >= 2
                proj, cut, copy = seen[-1]
                if state is cplx:
                    assert np.array_equal(proj.data, copy.project("z").data) and np.array_equal(cut.data, copy.slice({"x": "mid"}).data)
                elif state is vec:
                    assert np.array_equal(proj, grid.integrate(copy.data, axes=(2,))) and np.array_equal(cut, copy.data[:, 2])      # (x = 3.0 lies between two cells: argmin takes the first)
                else:
                    assert [np.array_equal(p.data, f.project("z").data) for p, f in zip(proj, copy)] == [True, True]
                    assert [np.array_equal(c.data, f.slice({"x": "mid"}).data) for c, f in zip(cut, copy)] == [True, True]
        finally:
            backend.device_projections = None
    # a library without the entry points: the reference method on the downloaded state
    eq, state = _problem(pde)
    rows = []

    def plain_tracker(field, t):
        link = field.__dict__.get("_hip_link")
        if link is not None and link.host_stale:
            before = link.downloads
            rows.append((pde_hip.project(field, "z"), before, link.downloads, field.copy()))

    with stats_shimlib.use_shim():
        _solve(pde, eq, state, [pde.CallbackTracker(plain_tracker, interrupts=0.25)])
    assert rows and all(after == before + 1 and np.array_equal(got.data, copy.project("z").data) for got, before, after, copy in rows)
