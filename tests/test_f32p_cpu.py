"""The pure-fp32 arithmetic mode without a GPU: the restatement against the reference's torch results (tests/golden/f32p.npz), the option and
its parsing, and the refusals - through the host library of the CPU tests (tests/shimlib.py), which has none of the new entry points, so
whatever the mode serves on the device is refused here with the symbols named, and whatever it refuses is refused before the library is
asked.  The kernels themselves are tested on the GPU (tests/test_hip_f32p.py)."""

from __future__ import annotations

import numpy as np
import pytest

import f32p_cases as FC
import pde_hip
import refpath
import shimlib
from helpers import GOLDEN
from pde_hip import f32p
from pde_hip.backend import HipBackend


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "f32p.npz", allow_pickle=False)


@pytest.fixture
def shim():
    with shimlib.use_shim() as lib:
        yield lib


def fp32_backend():
    b = HipBackend(name="hip-f32p")
    b.f32_arithmetic = "fp32"
    return b


# ---- restatement == goldens -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc_name", list(FC.GOLDEN_LAPLACE_BCS))
@pytest.mark.parametrize("shape", FC.GOLDEN_LAPLACE_SHAPES, ids=str)
def test_restated_laplace_equals_the_reference(golden, shape, bc_name):
    """Ghost cells by the mirror's ``set_ghost_cells`` on the fp32 field (numpy, the reference's formulas), then the restated stencil."""
    nd = len(shape)
    grid = pde_hip.CartesianGrid(FC.bounds_for(shape, FC.DX[nd]), shape)
    valid = golden[f"field/{nd}d"]
    assert np.array_equal(valid, FC.golden_field(shape))
    field = pde_hip.ScalarField(grid, valid, dtype=np.float32)
    with shimlib.use_shim():
        field.set_ghost_cells(FC.GOLDEN_LAPLACE_BCS[bc_name])
    full = field._data_full
    assert full.dtype == np.float32
    got = FC.laplace_full(full, grid.discretization)
    assert got.dtype == np.float32 and np.array_equal(got, golden[f"lap/{nd}d/{bc_name}"])


@pytest.mark.parametrize("steps", FC.GOLDEN_EULER_STEPS)
@pytest.mark.parametrize("case", FC.GOLDEN_EULER_CASES, ids=[c[0] for c in FC.GOLDEN_EULER_CASES])
def test_restated_euler_equals_the_reference(golden, case, steps):
    cid, shape, periodic = case
    nd = len(shape)
    dx = np.array([hi / n for (_, hi), n in zip(FC.bounds_for(shape, FC.DX[nd]), shape)])     # grid.discretization
    dt = FC.stable_dt(dx, FC.GOLDEN_D)
    assert dt * FC.GOLDEN_D * float(np.sum(dx ** -2)) < 0.5
    got = FC.euler_steps(golden[f"field/{nd}d"], dx, periodic, FC.GOLDEN_D, dt, steps)
    assert np.array_equal(got, golden[f"euler/{cid}/{steps}"])


def test_a_sweep_of_k_steps_is_k_single_steps():
    u = FC.field_data((5, 6, 8), seed=2)
    one = u
    for _ in range(4):
        one = FC.euler_steps(one, FC.DX[3], (True, False, True), 0.7, 0.001, 1)
    assert np.array_equal(one, FC.euler_steps(u, FC.DX[3], (True, False, True), 0.7, 0.001, 4))


def test_golden_file_is_smaller_than_the_largest_one():
    sizes = {p.name: p.stat().st_size for p in GOLDEN.glob("*.npz")}
    assert sizes["f32p.npz"] < max(v for k, v in sizes.items() if k != "f32p.npz")


# ---- the option ------------------------------------------------------------------------------------------------------------------
def test_option_default_parsing_and_errors(monkeypatch):
    monkeypatch.delenv("PDEHIP_F32_ARITHMETIC", raising=False)
    b = HipBackend(name="hip-option")
    assert b.f32_arithmetic == "fp64"
    assert pde_hip.get_backend("hip").f32_arithmetic == "fp64"
    b.f32_arithmetic = "fp32"
    assert b.f32_arithmetic == "fp32"
    for bad in ("fp16", "FP32", "", 32, True):
        with pytest.raises(ValueError, match="f32_arithmetic"):
            b.f32_arithmetic = bad
    assert b.f32_arithmetic == "fp32"
    b.f32_arithmetic = None                      # back to the configuration / the environment
    assert b.f32_arithmetic == "fp64"
    monkeypatch.setenv("PDEHIP_F32_ARITHMETIC", "fp32")
    assert b.f32_arithmetic == "fp32"
    monkeypatch.setenv("PDEHIP_F32_ARITHMETIC", "double")
    with pytest.raises(ValueError, match="f32_arithmetic"):
        _ = b.f32_arithmetic
    monkeypatch.delenv("PDEHIP_F32_ARITHMETIC")
    assert HipBackend({"f32_arithmetic": "fp32"}, name="hip-config").f32_arithmetic == "fp32"
    with pytest.raises(ValueError, match="f32_arithmetic"):
        _ = HipBackend({"f32_arithmetic": "single"}, name="hip-config").f32_arithmetic


def test_config_key_is_among_the_plugin_defaults():
    pde = refpath.import_reference()
    if pde is None:
        pytest.skip("py-pde (reference) not available")
    from pde_hip import pypde_plugin

    par = pypde_plugin.DEFAULT_CONFIG["f32_arithmetic"]
    assert par.value == "fp64" and par.cls is str
    assert pde.config["backend.hip.f32_arithmetic"] == "fp64"


def test_abi_lists_the_entry_points_as_optional():
    from pde_hip import _abi

    assert set(f32p.ENTRY_POINTS) <= set(_abi.OPTIONAL_PROTOTYPES)
    assert _abi.ABI_VERSION == 8


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_library_without_the_entry_points_is_refused_with_their_names(shim):
    if refpath.REAL:
        pytest.skip("the real library has the entry points")
    assert not shim.has(*f32p.ENTRY_POINTS)
    b = fp32_backend()
    grid = pde_hip.UnitGrid([6, 8], periodic=[True, False])
    field = pde_hip.ScalarField(grid, FC.field_data((6, 8)), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="pdehip_laplace_f32p"):
        field.laplace("auto_periodic_neumann", backend=b)
    with pytest.raises(NotImplementedError, match="pdehip_euler_run_f32p.*pdehip_f32p_supported.*f32_arithmetic"):
        pde_hip.DiffusionPDE(0.7).solve(field, t_range=0.1, dt=0.05, backend=b, solver="euler", tracker=None)


def test_refusal_table(shim):
    b = fp32_backend()
    grid = pde_hip.UnitGrid([6, 8], periodic=[True, False])
    data = FC.field_data((6, 8))
    field = pde_hip.ScalarField(grid, data, dtype=np.float32)
    bc = "auto_periodic_neumann"
    match = "no pure-fp32 kernel.*backend.hip.f32_arithmetic = 'fp32'"
    # operators: named in the message
    refused = {
        "gradient": lambda: field.gradient(bc, backend=b),
        "gradient_squared": lambda: field.gradient_squared(bc, backend=b),
        "laplace.*laplace9": lambda: field.laplace(bc, backend=b, corner_weight=1 / 3),
        "d_dx": lambda: field.apply_operator("d_dx", bc, backend=b),
        "divergence": lambda: pde_hip.VectorField(grid, np.stack([data, data]), dtype=np.float32).divergence(bc, backend=b),
        "vector_laplace": lambda: pde_hip.VectorField(grid, np.stack([data, data]), dtype=np.float32).laplace(bc, backend=b),
    }
    for name, call in refused.items():
        with pytest.raises(NotImplementedError, match=f"operator `{name}.*{match}"):
            call()
    per = pde_hip.ScalarField(pde_hip.UnitGrid([6, 8], periodic=True), data, dtype=np.float32)
    with pytest.raises(NotImplementedError, match=f"laplace_spectral.*{match}"):
        per.laplace("periodic", backend=b, spectral=True)
    # time loops: other equations, other solvers, adaptive steps, noise
    solve = dict(t_range=0.1, dt=0.05, backend=b, tracker=None)
    with pytest.raises(NotImplementedError, match=f"equation CahnHilliardPDE.*{match}"):
        pde_hip.CahnHilliardPDE().solve(field, solver="euler", **solve)
    with pytest.raises(NotImplementedError, match=f"solver RungeKuttaSolver.*{match}"):
        pde_hip.DiffusionPDE().solve(field, solver="runge-kutta", **solve)
    with pytest.raises(NotImplementedError, match=f"solver EulerSolver.*{match}"):
        pde_hip.DiffusionPDE().solve(field, solver="euler", adaptive=True, **solve)
    with pytest.raises(NotImplementedError, match=f"noise.*{match}"):
        pde_hip.DiffusionPDE(noise=0.1).solve(field, solver="euler", **solve)
    with pytest.raises(NotImplementedError, match=f"right-hand side of DiffusionPDE.*{match}"):
        b.make_pde_rhs(pde_hip.DiffusionPDE(), field)
    # a post-step hook runs between the steps: no pure-fp32 loop around it
    class Hooked(pde_hip.DiffusionPDE):
        def make_post_step_hook(self, state, backend="numpy"):
            return (lambda data, t, post_step_data: (data, post_step_data)), 0

    with pytest.raises(NotImplementedError, match=f"solver EulerSolver with a post-step hook.*{match}"):
        Hooked().solve(field, solver="euler", **solve)
    # poisson_solver: refused for fp32 right-hand sides before the solver is built (host data with a dtype, and by the array's own type)
    for dtype in (np.float32, None):
        solver = pde_hip.UnitGrid([6, 8]).make_operator("poisson_solver", {"value": 0.0}, backend=b, dtype=dtype)
        with pytest.raises(NotImplementedError, match=f"operator `poisson_solver`.*{match}"):
            solver(data)
    # complex64 fields are pairs of fp32 parts: no operator serves them in this mode, `laplace` included
    c64 = pde_hip.ScalarField(grid, data + 1j * data, dtype=np.complex64)
    for name, call in (("laplace", lambda: c64.laplace(bc, backend=b)), ("gradient", lambda: c64.gradient(bc, backend=b))):
        with pytest.raises(NotImplementedError, match=f"operator `{name}` on a complex64 field.*{match}"):
            call()
    assert pde_hip.ScalarField(grid, data + 1j * data, dtype=np.complex128).laplace(bc, backend=b).data.dtype == np.complex128
    # fastmath contracts operations: not together with this mode
    b.fastmath = True
    try:
        with pytest.raises(NotImplementedError, match="fastmath"):
            field.laplace(bc, backend=b)
        with pytest.raises(NotImplementedError, match="fastmath"):
            pde_hip.DiffusionPDE().solve(field, solver="euler", **solve)
    finally:
        b.fastmath = False


def test_decomposed_grids_are_refused_through_the_plugin(shim):
    """The real py-pde with the plugin: the configuration value reaches the backend, the decomposed solver refuses fp32 states before it
    touches a device, the environment variable is NOT consulted there (the plugin's configuration always holds a value)."""
    pde = refpath.import_reference()
    if pde is None:
        pytest.skip("py-pde (reference) not available")
    import pde_hip.pypde_plugin  # noqa: F401  (registers "hip" and the solver `hip_slab`)

    grid = pde.UnitGrid([8, 6], periodic=[True, False])
    f32 = pde.ScalarField(grid, FC.field_data((8, 6)), dtype=np.float32)
    f64 = pde.ScalarField(grid, FC.field_data((8, 6)).astype(np.float64))
    old = pde.config["backend.hip.f32_arithmetic"]
    pde.config["backend.hip.f32_arithmetic"] = "fp32"
    try:
        with pytest.raises(NotImplementedError, match="solver `hip_slab`.*decomposed grids.*no pure-fp32 kernel.*backend.hip.f32_arithmetic = 'fp32'"):
            pde.DiffusionPDE().solve(f32, t_range=0.1, dt=0.05, solver="hip_slab", backend="hip", tracker=None)
        with pytest.raises(NotImplementedError, match="operator `gradient`.*no pure-fp32 kernel"):
            f32.gradient("auto_periodic_neumann", backend="hip")
        with pytest.raises(NotImplementedError, match="pdehip_laplace_f32p"):        # served on the device; the host library lacks the symbols
            f32.laplace("auto_periodic_neumann", backend="hip")
        res = pde.DiffusionPDE().solve(f64, t_range=0.1, dt=0.05, solver="hip_slab", backend="hip", tracker=None)     # fp64 states are not affected
        assert res.data.dtype == np.float64
    finally:
        pde.config["backend.hip.f32_arithmetic"] = old
    # back in the default mode (a new grid: py-pde caches the operators of a grid, and an operator keeps the mode it was made in)
    again = pde.ScalarField(pde.UnitGrid([8, 6], periodic=[True, False]), FC.field_data((8, 6)), dtype=np.float32)
    assert again.gradient("auto_periodic_neumann", backend="hip").data.dtype == np.float32


def test_environment_variable_is_for_the_stand_alone_backend(monkeypatch):
    pde = refpath.import_reference()
    if pde is None:
        pytest.skip("py-pde (reference) not available")
    import pde_hip.pypde_plugin  # noqa: F401

    monkeypatch.setenv("PDEHIP_F32_ARITHMETIC", "fp32")
    assert HipBackend(name="hip-env").f32_arithmetic == "fp32"           # stand-alone: no configuration entry
    assert pde.backends.backend_registry.get_backend("hip").f32_arithmetic == "fp64"                      # plugin: the configuration's value


def test_fp64_fields_and_data_movement_are_not_affected(shim):
    b = fp32_backend()
    plain = HipBackend(name="hip-plain")
    grid = pde_hip.UnitGrid([6, 8], periodic=[True, False])
    data = FC.field_data((6, 8))
    bc = "auto_periodic_neumann"
    f64 = pde_hip.ScalarField(grid, data.astype(np.float64))
    assert np.array_equal(f64.gradient(bc, backend=b).data, f64.gradient(bc, backend=plain).data)
    assert np.array_equal(f64.laplace(bc, backend=b).data, f64.laplace(bc, backend=plain).data)
    res = pde_hip.DiffusionPDE().solve(f64, t_range=0.1, dt=0.05, backend=b, solver="euler", tracker=None)
    assert res.data.dtype == np.float64
    # ghost cells of an fp32 field are data movement, not stencil arithmetic
    f32 = pde_hip.ScalarField(grid, data, dtype=np.float32)
    setter = b.make_ghost_cell_setter(grid.get_boundary_conditions(bc))
    full = f32._data_full.copy()
    setter(full)
    assert np.array_equal(full[1:-1, 0], full[1:-1, 1]) and np.array_equal(full[0, 1:-1], full[-2, 1:-1])
    # the default mode serves fp32 fields as before
    assert plain.f32_arithmetic == "fp64"
    assert f32.gradient(bc, backend=plain).data.dtype == np.float32
