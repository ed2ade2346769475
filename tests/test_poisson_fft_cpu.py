"""The direct Poisson solve without a GPU: the serial C versions of the tests-only shim (tests/shim/pdehip_shim_poisson_fft.c) against
numpy, the dense restatement of ``tests/poisson_cases.py`` and the reference's golden solutions, and ``method="fft"`` of
``pde_hip/poisson.py`` through the shim.

Bounds: ``tests/poisson_fft_cases.py``.  Observed ratios: ``profiles/poisson_fft_tests.md``.  The device kernels are compared with the shim
bit by bit in ``tests/test_hip_poisson_fft.py``.
"""

from __future__ import annotations

import math

import numpy as np
import poisson_fft_cases as P
import poisson_fft_shimlib
import pytest
import refpath
import shimlib
import spectrum_cases as K
import spectrum_shimlib
from helpers import GOLDEN, get_case, load_cases, make_grid
from poisson_cases import dense_solve

import pde_hip
from pde_hip import _abi, poisson
from pde_hip.device import DeviceArray
from pde_hip.solvers import ConvergenceError

IDS = ["f64", "f32"]
NPZ = np.load(GOLDEN / "poisson_fft.npz", allow_pickle=False)
NEW = ("fft_inverse", "poisson_fft")
# the shapes of spectrum_cases.SHAPES that are cheap on the host: all but 64^3
HOST_SHAPES = tuple(s for s in K.SHAPES if math.prod(s) <= 1 << 16)


@pytest.fixture
def shim():
    with poisson_fft_shimlib.use_shim() as lib:
        yield lib


def periodic_grid(shape, dx):
    return pde_hip.CartesianGrid([[0, n * d] for n, d in zip(shape, dx)], list(shape), periodic=True)


def test_abi_table():
    assert _abi.ABI_VERSION == 8 and set(NEW) <= set(_abi.OPTIONAL_PROTOTYPES)
    assert not set(NEW) & (set(_abi.COMPUTE_PROTOTYPES) | set(_abi.COMM_PROTOTYPES) | set(_abi.RUNTIME_PROTOTYPES))
    for module in (shimlib, spectrum_shimlib):
        with module.use_shim() as lib:
            assert not lib.has("fft_inverse") and not lib.has("poisson_fft")
    with poisson_fft_shimlib.use_shim() as lib:
        assert lib.has("fft_supported", "fft_forward", "fft_inverse", "poisson_fft")


def test_methods():
    assert poisson.METHODS == ("auto", "cg", "mgcg") and poisson.DIRECT_METHODS == ("fft",)
    poisson.check_method("fft")
    with pytest.raises(ValueError, match="Method fftw is not available"):
        poisson.check_method("fftw")


# ---- the inverse transform -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", HOST_SHAPES, ids=K.shape_id)
def test_shim_inverse_of_forward_returns_the_input(shape):
    assert (4096,) in HOST_SHAPES and (1024, 8) in HOST_SHAPES
    valid = K.inputs(shape, 3, "float64")
    back = P.shim_inverse(shape, 3, "float64")
    err, bound = np.abs(back - valid).max(), 2.0 * K.transform_eps(shape) * np.abs(valid).max()
    print(f"{K.shape_id(shape)}: {err / bound:.3g} of the bound")
    assert err <= bound
    # fp32 output: the same numbers rounded once
    np.testing.assert_array_equal(P.shim_inverse(shape, 3, "float32"), back.astype(np.float32))


def test_shim_inverse_mirror_rule_and_stray_imaginary_parts():
    """Element N - k is the conjugate of element k; imaginary parts at k = 0 and N / 2 enter the lines as they are and only their real
    contribution survives: the result is numpy's ``irfftn`` of the same half spectrum within the transform bound."""
    shape = (8, 16)
    rng = np.random.default_rng(5)
    spec = (rng.normal(size=(1, 8, 9)) + 1j * rng.normal(size=(1, 8, 9)))
    got = P.shim().inverse(shape, spec, np.float64)
    rows = np.fft.ifft(spec, axis=1)                                             # the slow axis first, on the half spectrum
    full = np.concatenate([rows, np.conj(rows[..., -2:0:-1])], axis=-1)          # the mirror rule of a row, stated with numpy
    want = np.fft.ifft(full, axis=2).real
    assert np.abs(got - want).max() <= 2.0 * K.transform_eps(shape) * np.abs(spec).max()


# ---- the solve -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", P.SOLVE_SHAPES, ids=K.shape_id)
def test_shim_solve_against_the_dense_restatement(shape):
    dx = K.dx_of(shape)
    rhs = P.white(shape)
    got, io = P.shim().solve(shape, dx, rhs)
    want = dense_solve(periodic_grid(shape, dx), "periodic", rhs)
    cond = P.condition(shape, dx)
    err, bound = np.abs(got - want).max(), 64.0 * cond * P.U * max(1.0, np.abs(want).max())
    print(f"{K.shape_id(shape)}: cond {cond:.3g}, error {err:.3g} = {err / (cond * P.U * max(1.0, np.abs(want).max())):.3g} cond u max(1, |x|)")
    assert err <= bound
    assert io["status"] == 0 and io["iterations"] == 0 and io["singular"] == 1 and abs(got.mean()) <= 4 * P.U * np.abs(got).max()


@pytest.mark.parametrize("shape,dx", [(s, K.dx_of(s)) for s in P.SOLVE_SHAPES] + [P.LONG_LINE], ids=lambda v: K.shape_id(v) if isinstance(v[0], int) else None)
def test_shim_residual_and_norms(shape, dx):
    from helpers import host_faces, oracle_grid, to_full
    from oracle import pde_oracle as O

    rhs = P.white(shape)
    got, io = P.shim().solve(shape, dx, rhs)
    print(f"{K.shape_id(shape)}: residual / rhs_norm = {io['residual'] / io['rhs_norm']:.3g}")
    assert io["residual"] <= 1e-11 * io["rhs_norm"]
    grid = periodic_grid(shape, dx)
    full = to_full(grid, got)
    O.set_ghost_cells(oracle_grid(grid), 1, host_faces(grid.get_boundary_conditions("periodic")).c, full)
    w = O.laplace(oracle_grid(grid), full)
    # the same arrays: x as returned, A x by the oracle's stencil, the mean from the shim's own forward transform
    mean = P.shim().forward(shape, rhs[None]).flat[0].real / rhs.size
    for key, want in (("residual", np.linalg.norm(w - (rhs - mean))), ("rhs_norm", np.linalg.norm(rhs - mean)), ("check_residual", np.linalg.norm(w - rhs))):
        assert abs(io[key] - want) <= 2.0 * rhs.size * P.U * want, (key, io[key], want)


def golden_cases(raises: bool):
    return [c["id"] for c in load_cases(NPZ) if bool(c.get("raises")) == raises]


@pytest.mark.parametrize("cid", golden_cases(False))
def test_golden_solutions(cid, shim):
    case = get_case(NPZ, cid)
    grid = make_grid(case)
    np.testing.assert_allclose(grid.discretization, NPZ[f"{cid}/dx"], rtol=1e-15)
    op = grid.make_operator("poisson_solver", case["bc"], backend="hip", method="fft")
    got, want = op(NPZ[f"{cid}/rhs"]), NPZ[f"{cid}/solution"]
    assert abs(got.mean()) < 1e-10
    want = want - want.mean()          # lsmr's member of the family, compared up to the constant
    assert np.abs(got - want).max() / max(1.0, np.abs(want).max()) < 1e-8
    assert op.info["method"] == "fft" and op.info["iterations"] == 0 and op.info["converged"]
    assert op.info["residual"] <= 1e-11 * op.info["rhs_norm"]
    res = pde_hip.solve_poisson_equation(pde_hip.ScalarField(grid, NPZ[f"{cid}/rhs"]), case["bc"], method="fft")
    assert res.label == str(NPZ[f"{cid}/label"]) and np.array_equal(res.data, got) and res.info["method"] == "fft"


def test_inconsistent_right_hand_side_raises_like_the_reference(shim):
    (cid,) = golden_cases(True)
    case = get_case(NPZ, cid)
    grid = make_grid(case)
    rhs = pde_hip.ScalarField(grid, NPZ[f"{cid}/rhs"])
    with pytest.raises(RuntimeError) as err:
        pde_hip.solve_poisson_equation(rhs, case["bc"], method="fft")
    want = str(NPZ[f"{cid}/message"])
    assert str(err.value).split("magnitude")[0] == want.split("magnitude")[0]
    assert "Poisson problem could not be solved (Residual:" in str(err.value.__cause__)
    op = grid.make_operator("poisson_solver", case["bc"], backend="hip", method="fft")
    with pytest.raises(RuntimeError, match=r"could not be solved \(Residual"):
        op(rhs.data)
    assert op.info["iterations"] == 0 and op.info["method"] == "fft"


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------
class NoLibrary:
    """Stands in for the library while the refusals are checked: any call is an error."""

    missing: set = set()

    def has(self, *names):
        return True

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the refusal")


def test_refusals_come_before_any_library_call(shim, monkeypatch):
    backend = pde_hip.get_backend("hip")
    per = pde_hip.CartesianGrid([[0, 8], [0, 8]], [8, 8], periodic=[True, True])
    half = pde_hip.CartesianGrid([[0, 8], [0, 8]], [8, 8], periodic=[True, False])
    info = backend.get_operator_info(per, "poisson_solver")
    backend.grid_info(per, np.float64), backend.grid_info(half, np.float64)          # (the layouts are cached: no call below)
    monkeypatch.setattr(type(backend), "_lib", property(lambda self: NoLibrary()))
    for name, value in (("maxiter", 10), ("batch", 4)):
        with pytest.raises(TypeError, match=rf"{name}.*need an iterative method \(method is 'fft'\)"):
            info.factory(per, backend=backend, bcs=per.get_boundary_conditions("periodic"), method="fft", **{name: value})
    with pytest.raises(TypeError, match="mg_smooth.*need method=\"mgcg\""):
        info.factory(per, backend=backend, bcs=per.get_boundary_conditions("periodic"), method="fft", mg_smooth=2)
    with pytest.raises(TypeError, match="unknown argument"):
        info.factory(per, backend=backend, bcs=per.get_boundary_conditions("periodic"), method="fft", cycles=2)
    with pytest.raises(ValueError, match="must not be negative"):
        info.factory(per, backend=backend, bcs=per.get_boundary_conditions("periodic"), method="fft", rtol=-1.0)
    for bc, face in (({"value": 0.0}, "lower face of axis 1"), ({"derivative": 0.0}, "lower face of axis 1"), ({"value_expression": "sin(x)"}, "lower face of axis 1")):
        with pytest.raises(NotImplementedError, match=face):
            info.factory(half, backend=backend, bcs=half.get_boundary_conditions(["periodic", bc]), method="fft")


def test_refused_grids_carry_the_librarys_message(shim):
    for shape in ((12,), (8, 6)):
        grid = pde_hip.UnitGrid(list(shape), periodic=True)
        with pytest.raises(NotImplementedError, match="fft"):
            grid.make_operator("poisson_solver", "periodic", backend="hip", method="fft")
    grid = pde_hip.UnitGrid([8, 8], periodic=[False, True])
    with pytest.raises(NotImplementedError, match="lower face of axis 0"):
        grid.make_operator("poisson_solver", [{"value": 0}, "periodic"], backend="hip", method="fft")


def test_a_library_without_the_entry_points_is_named():
    if refpath.REAL:
        pytest.skip("the real library has the entry points")
    grid = pde_hip.UnitGrid([8, 8], periodic=True)
    with shimlib.use_shim():
        with pytest.raises(NotImplementedError, match="pdehip_fft_supported, pdehip_poisson_fft"):
            grid.make_operator("poisson_solver", "periodic", backend="hip", method="fft")
    with spectrum_shimlib.use_shim():
        with pytest.raises(NotImplementedError, match="does not export pdehip_poisson_fft:"):
            grid.make_operator("poisson_solver", "periodic", backend="hip", method="fft")


def test_zero_tolerances_raise_convergence_error(shim):
    grid = pde_hip.UnitGrid([16, 8], periodic=True)
    op = grid.make_operator("poisson_solver", "periodic", backend="hip", method="fft", rtol=0.0, atol=0.0)
    with pytest.raises(ConvergenceError, match="the direct FFT solve reached residual .*, asked 0"):
        op(P.white((16, 8)))
    assert op.info["iterations"] == 0 and not op.info["converged"]
    op = grid.make_operator("poisson_solver", "periodic", backend="hip", method="fft", rtol=0.0, atol=1e-9)
    op(P.white((16, 8)))
    assert op.info["converged"]


def test_nonfinite_right_hand_side(shim):
    grid = pde_hip.UnitGrid([16, 8], periodic=True)
    rhs = P.white((16, 8))
    rhs[3, 3] = np.nan
    with pytest.raises(RuntimeError, match="not finite"):
        grid.make_operator("poisson_solver", "periodic", backend="hip", method="fft")(rhs)


def test_fp32_complex_and_device_arrays(shim):
    shape, dx = (16, 8), (0.75, 1.5)
    grid = periodic_grid(shape, dx)
    backend = pde_hip.get_backend("hip")
    rhs = P.white(shape)
    op = grid.make_operator("poisson_solver", "periodic", backend="hip", method="fft")
    want = op(rhs)
    # fp32: the same solve of the rounded right-hand side (whose mean is of rounding size), rounded once at the end
    rhs32 = rhs.astype(np.float32)
    got32 = op(rhs32)
    assert got32.dtype == np.float32
    ref32 = P.shim().solve(shape, dx, rhs32)[0]
    np.testing.assert_array_equal(got32, ref32)
    assert np.abs(got32 - want).max() <= 64.0 * P.condition(shape, dx) * 2.0 ** -24 * np.abs(want).max()
    # complex: real and imaginary part in turn
    other = P.white(shape, seed=1)
    cop = grid.make_operator("poisson_solver", "periodic", backend="hip", method="fft", dtype=np.complex128)
    got = cop(rhs + 1j * other)
    np.testing.assert_array_equal(got.real, want)
    np.testing.assert_array_equal(got.imag, op(other))
    assert cop.info["method"] == "fft" and cop.info["iterations"] == 0
    # a DeviceArray in, a DeviceArray out; `out=` is used
    ginfo = backend.grid_info(grid, np.float64)
    dev = DeviceArray(ginfo).set_valid(rhs, backend.stream)
    res = op(dev)
    assert isinstance(res, DeviceArray)
    np.testing.assert_array_equal(res.get_valid(stream=backend.stream), want)
    out = DeviceArray(ginfo)
    assert op(dev, out=out) is out
    np.testing.assert_array_equal(out.get_valid(stream=backend.stream), want)
    host_out = np.empty(shape)
    assert op(rhs, out=host_out) is host_out and np.array_equal(host_out, want)


def test_through_the_real_py_pde(shim):
    pde = refpath.import_reference()
    if pde is None:
        pytest.skip("py-pde (reference) not available")
    import pde_hip.pypde_plugin  # noqa: F401

    cid = "2d-16x8"
    case = get_case(NPZ, cid)
    grid = pde.CartesianGrid(case["bounds"], case["shape"], periodic=case["periodic"])
    op = grid.make_operator("poisson_solver", case["bc"], backend="hip", method="fft")
    got, want = op(NPZ[f"{cid}/rhs"]), NPZ[f"{cid}/solution"]
    want = want - want.mean()
    assert np.abs(got - want).max() / max(1.0, np.abs(want).max()) < 1e-8 and op.info["method"] == "fft"
    res = pde_hip.solve_poisson_equation(pde.ScalarField(grid, NPZ[f"{cid}/rhs"]), case["bc"], method="fft", backend=pde.backends.get_backend("hip"))
    np.testing.assert_array_equal(res.data, got)
    with pytest.raises(NotImplementedError, match="lower face of axis 1"):
        half = pde.CartesianGrid(case["bounds"], case["shape"], periodic=[True, False])
        half.make_operator("poisson_solver", ["periodic", {"value": 0}], backend="hip", method="fft")
